"""The weight average of --use-ema (Classification/ConvNets/image_classification/models/common.py:191-212) restated on CPU
tensors: the helper the GPU tests of tests/test_gpu_rn50_ema.py compare against, checked here against the reference's own EMA
class and against the three-rounding fp32 expression the kernel implements.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import _ref_import as R  # noqa: E402

needs_ref = pytest.mark.skipif(not R.have_reference(), reason="reference tree not mounted")


# ---------------------------------------------------------------------------------------------- the helper
def ema_mu(mu, step=None):
    """The decay of one update, in Python doubles (common.py:197-200)."""
    return mu if step is None else min(mu, (1.0 + step) / (10 + step))


def ema_update_(shadow, state, mu, step=None):
    """One EMA.__call__ on CPU fp32 tensors: `shadow` and `state` are state_dict-like mappings; counters are left alone."""
    m = ema_mu(mu, step)
    with torch.no_grad():
        for name, x in state.items():
            if name.endswith("num_batches_tracked"):
                continue
            shadow[name].mul_(m)
            shadow[name].add_((1.0 - m) * x)


def ema_three_roundings(e, x, mu_t):
    """e' = rn(rn(fp32(mu_t) * e) + rn(fp32(1 - mu_t) * x)) on numpy float32 arrays; 1 - mu_t is taken in double first."""
    a = np.float32(mu_t) * e
    b = np.float32(1.0 - mu_t) * x
    assert a.dtype == np.float32 and b.dtype == np.float32
    return a + b


@pytest.fixture
def ref_convnets(monkeypatch):
    """The reference's ConvNets modules imported on CPU.  oracle/_ref_import prepends to sys.path, stubs `dllogger` and replaces
    torch.cuda.synchronize to do so: all three are put back afterwards, so later test modules see the real shims."""
    monkeypatch.setattr(torch.cuda, "synchronize", torch.cuda.synchronize)     # (registered now: undone on teardown)
    monkeypatch.setattr(sys, "path", list(sys.path))
    before = dict(sys.modules)
    yield R.import_convnets()
    for k in list(sys.modules):
        if k not in before and (k == "dllogger" or k.split(".")[0] == "image_classification"):
            del sys.modules[k]
    if "dllogger" in before:
        sys.modules["dllogger"] = before["dllogger"]


def _small_model(seed):
    torch.manual_seed(seed)
    m = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3, bias=False), torch.nn.BatchNorm2d(8))
    with torch.no_grad():
        m[1].running_mean.normal_()
        m[1].running_var.uniform_(0.5, 2.0)
        m[1].weight.normal_()
        m[1].bias.normal_()
        m[1].num_batches_tracked.fill_(seed)
    return m


@needs_ref
@pytest.mark.parametrize("mu", [0.999, 0.9999])
def test_helper_matches_the_reference_ema_class(mu, ref_convnets):
    EMA = ref_convnets.models.common.EMA
    src = _small_model(3)
    ema_ref_model, shadow = _small_model(5), {k: v.clone() for k, v in _small_model(5).state_dict().items()}
    ema = EMA(mu, ema_ref_model)
    for i, step in enumerate([None, 0, 1, 37, 10 ** 5]):
        with torch.no_grad():                                  # the source moves between updates, as a training model does
            for p in src.state_dict().values():
                if p.dtype.is_floating_point:
                    p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(100 + i)) * 0.1)
        ema(src, step=step)
        ema_update_(shadow, src.state_dict(), mu, step)
        got = ema_ref_model.state_dict()
        assert set(got) == set(shadow)
        for k in got:
            assert torch.equal(got[k], shadow[k]), (k, step)
        assert int(got["1.num_batches_tracked"]) == 5 and int(shadow["1.num_batches_tracked"]) == 5


@pytest.mark.parametrize("mu,step", [(0.9999, None), (0.9999, 0), (0.999, 37), (0.999, None), (0.5, None), (0.99, 10 ** 5)])
def test_three_rounding_expression_equals_the_helper(mu, step):
    g = torch.Generator().manual_seed(11)
    for n in (1, 3, 64, 2049, 1 << 20):
        e = torch.randn(n, generator=g) * 3.0
        x = torch.randn(n, generator=g) * 3.0
        if n >= 64:
            e[:6] = torch.tensor([0.0, -0.0, 1e-40, -1e-42, 3e38, -1e30])
            x[:6] = torch.tensor([-0.0, 0.0, -1e-41, 1e-39, 1e30, -3e38])
        want = ema_three_roundings(e.numpy().copy(), x.numpy().copy(), ema_mu(mu, step))
        shadow = {"w": e.clone()}
        ema_update_(shadow, {"w": x}, mu, step)
        assert np.array_equal(shadow["w"].numpy().view(np.uint32), want.view(np.uint32)), (mu, step, n)


def test_warmup_decay_rule():
    assert ema_mu(0.999, None) == 0.999
    assert ema_mu(0.999, 0) == 0.1 and ema_mu(0.999, 1) == 2.0 / 11 and ema_mu(0.999, 37) == 38.0 / 47
    assert ema_mu(0.999, 10 ** 5) == 0.999 and ema_mu(0.9999, 10 ** 5) == 0.9999


def test_use_ema_is_accepted_by_the_rn50_command_line():
    import argparse
    from deeplearningexamples_amd.convnets import main as M
    args = M.add_parser_arguments(argparse.ArgumentParser()).parse_args(["--amp", "--use-ema", "0.999"])
    assert args.use_ema == 0.999
    M._reject_unbuilt(args)                                    # exits on flags that select machinery this path does not have
    assert M.add_parser_arguments(argparse.ArgumentParser()).parse_args(["--amp"]).use_ema is None
