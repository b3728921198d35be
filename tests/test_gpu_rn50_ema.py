"""--use-ema for ResNet-50 (Classification/ConvNets/image_classification/models/common.py:191-212, training.py:148-202): the
multi-tensor kernel dle_mt_ema, the averaged model inside ResNetTrainer (update after every train_step call, evaluation, lazy
16-bit copies), the `state_dict_ema` checkpoint entry, the command line and a captured step.  The reference is the CPU helper of
tests/test_ema_reference.py (the reference's two tensor ops on fp32 CPU tensors); the kernel must agree with it to the bit.
GPU only."""
import json

import numpy as np
import pytest
import torch

from tests.test_ema_reference import ema_mu, ema_update_

pytestmark = pytest.mark.gpu

MU = 0.999


# ---------------------------------------------------------------------------------------------- kernel
def _kernel_case(cuda, seed):
    """~20 (source, average) pairs: tiny, odd, BatchNorm-sized, one element past a vector multiple, exactly one chunk, several
    chunks plus a tail; some are views 1-3 elements into a larger buffer (not 16-byte aligned: the scalar path), in every
    combination of aligned / unaligned source and average.  Values: normal, +-0, denormals, magnitudes near the fp32 limits."""
    from deeplearningexamples_amd import multi_tensor as mt
    g = torch.Generator().manual_seed(seed)
    sizes = [1, 3, 64, 2049, mt.CHUNK, 3 * 65536 + 5, 2, 4, 5, 63, 65, 256, 511, 512, 1000, 2048, 4097, mt.CHUNK - 1,
             mt.CHUNK + 1, 147 * 64]
    offs = [(0, 0), (1, 0), (0, 2), (3, 3), (2, 1)]
    special_e = torch.tensor([0.0, -0.0, 1e-40, -1e-42, 3e38, -1e30, 1.17549435e-38, 1e-45])
    special_x = torch.tensor([-0.0, 0.0, -1e-41, 1e-39, 1e30, -3e38, -1.17549435e-38, -1e-45])
    xs, es = [], []
    for i, n in enumerate(sizes):
        ox, oe = offs[i % len(offs)]
        x = torch.randn(n + 4, generator=g) * 2.0
        e = torch.randn(n + 4, generator=g) * 2.0
        k = min(n, special_e.numel())
        x[ox:ox + k] = special_x[:k]
        e[oe:oe + k] = special_e[:k]
        xs.append(x.to(cuda)[ox:ox + n])
        es.append(e.to(cuda)[oe:oe + n])
    assert any(t.data_ptr() % 16 for t in xs) and any(t.data_ptr() % 16 for t in es) and any(t.data_ptr() % 16 == 0 for t in es)
    return xs, es


@pytest.mark.parametrize("device_coef", [False, True], ids=["host_coef", "device_coef"])
def test_mt_ema_is_bit_exact(cuda, device_coef):
    from deeplearningexamples_amd import multi_tensor as mt
    xs, es = _kernel_case(cuda, 7)
    x_before = [x.clone() for x in xs]
    table = mt.TensorTable([xs, es])
    shadow = {str(i): e.cpu().clone() for i, e in enumerate(es)}
    coef = torch.empty(2, dtype=torch.float32, device=cuda) if device_coef else None
    g = torch.Generator().manual_seed(8)
    for r, (mu, step) in enumerate([(0.9999, None), (0.9999, 0), (0.999, 37)]):
        m = ema_mu(mu, step)
        if device_coef:
            coef.copy_(torch.tensor([m, 1.0 - m], dtype=torch.float64).to(torch.float32))
            mt.ema(table, -1.0, one_minus_mu=-1.0, coef=coef)        # (host values must be ignored when the pointer is given)
        else:
            mt.ema(table, m)
        ema_update_(shadow, {str(i): x.cpu() for i, x in enumerate(xs)}, mu, step)
        for i, e in enumerate(es):
            assert torch.equal(e.cpu().view(torch.int32), shadow[str(i)].view(torch.int32)), (r, i, e.numel())
        for x, xb in zip(xs, x_before):
            assert torch.equal(x.view(torch.int32), xb.view(torch.int32)), "the source list was written"
        for x, xb in zip(xs, x_before):                               # the sources move between updates
            d = (torch.randn(x.numel(), generator=g) * 0.5).to(cuda)
            x.add_(d)
            xb.copy_(x)


def test_mt_ema_rejects_wrong_lists(cuda):
    from deeplearningexamples_amd import multi_tensor as mt
    a = torch.zeros(8, device=cuda)
    with pytest.raises(ValueError):
        mt.ema(mt.TensorTable([[a], [a.clone()], [a.clone()]]), 0.9)
    with pytest.raises(ValueError):
        mt.ema(mt.TensorTable([[a], [a.to(torch.bfloat16)]]), 0.9)
    with pytest.raises(ValueError):
        mt.ema(mt.TensorTable([[a], [a.clone()]]), 0.9, coef=torch.zeros(3, device=cuda))


# ---------------------------------------------------------------------------------------------- trainer
def _cfg():
    from oracle import resnet_oracle as RO
    return RO, RO.RN50_STEP_CONFIG


def _batch(cuda, i=0):
    RO, c = _cfg()
    x, y = RO.seeded_batch(c["seed"] + 100 + i, 8, c["size"])
    return x.to(cuda), y.to(cuda)


def _build(cuda, ema=MU, seeded=True, seed=1, **kw):
    """The batch-8 configuration of test_gpu_checkpoint.py: seeded state, bf16, scale 128."""
    from deeplearningexamples_amd.convnets.resnet import ResNet50
    from deeplearningexamples_amd.convnets.engine import ResNetTrainer
    RO, c = _cfg()
    torch.manual_seed(seed)
    m = ResNet50(device=cuda)
    if seeded:
        m.load_state_dict({k: v.clone() for k, v in RO.seeded_state(c["seed"]).items()}, strict=False)
    return m, ResNetTrainer(m, lr=c["lr"], compute_dtype=torch.bfloat16, static_loss_scale=128.0, ema=ema, **kw)


def _cpu(state):
    return {k: v.detach().cpu().clone() for k, v in state.items()}


def _assert_ema_equals(trainer, shadow, what):
    got = trainer.ema_model.state_dict()
    assert list(got) == list(shadow)
    n = 0
    for k, v in got.items():
        assert torch.equal(v.cpu(), shadow[k]), (what, k)
        n += not k.endswith("num_batches_tracked")
    return n


def test_trainer_average_follows_the_reference(cuda):
    x, y = _batch(cuda)
    m, t = _build(cuda)
    shadow = _cpu(m.state_dict())
    counters = {k: v.clone() for k, v in shadow.items() if k.endswith("num_batches_tracked")}
    assert len(counters) == 53
    for k in range(4):
        t.train_step(x, y, step=k)
        ema_update_(shadow, _cpu(m.state_dict()), MU, k)
        assert _assert_ema_equals(t, shadow, "step %d" % k) == 267
    t.sync_counters()                                                   # the model's counters move, the average's never do
    assert int(m.bn1.num_batches_tracked) == 4
    for k, v in counters.items():
        assert torch.equal(t.ema_model.state_dict()[k].cpu(), v), k
    # without `step` the decay is the plain mu (EMA.__call__(step=None)) once set_ema_step(None) has said so
    t.set_ema_step(None)
    t.train_step(x, y)
    ema_update_(shadow, _cpu(m.state_dict()), MU, None)
    _assert_ema_equals(t, shadow, "step=None")


def test_average_moves_on_every_micro_batch(cuda):
    x, y = _batch(cuda)
    m, t = _build(cuda, grad_acc_steps=2)
    start = _cpu(m.state_dict())
    shadow = _cpu(start)
    t.train_step(x, y, step=0)                                          # accumulates only: no optimizer step
    mid = _cpu(m.state_dict())
    assert all(torch.equal(mid[n], start[n]) for n, _ in m.named_parameters())
    assert not torch.equal(mid["bn1.running_mean"], start["bn1.running_mean"])
    ema_update_(shadow, mid, MU, 0)
    _assert_ema_equals(t, shadow, "non-stepping micro-batch")
    assert not torch.equal(t.ema_model.bn1.running_mean.cpu(), start["bn1.running_mean"])
    t.train_step(x, y, step=1)                                          # the optimizer steps
    end = _cpu(m.state_dict())
    assert not torch.equal(end["fc.weight"], start["fc.weight"]) and not torch.equal(end["conv1.weight"], start["conv1.weight"])
    ema_update_(shadow, end, MU, 1)
    _assert_ema_equals(t, shadow, "stepping micro-batch")


def test_average_does_not_change_training(cuda):
    x, y = _batch(cuda)
    m1, t1 = _build(cuda, ema=MU)
    m2, t2 = _build(cuda, ema=None)
    assert t2.ema is None and t2.ema_model is None and not hasattr(t2, "t_ema")
    la = [float(t1.train_step(x, y, step=k).item()) for k in range(4)]
    lb = [float(t2.train_step(x, y).item()) for k in range(4)]
    np.testing.assert_allclose(la, lb, rtol=2e-6)                       # (the loss reduction uses fp32 atomics)
    for (n, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.allclose(a.float(), b.float(), rtol=1e-4, atol=1e-6), n
    with pytest.raises(ValueError):
        t2.infer(x, ema=True)


def _fresh_eval_logits(cuda, state, x, y):
    from deeplearningexamples_amd.convnets.resnet import ResNet50
    from deeplearningexamples_amd.convnets.engine import ResNetTrainer
    _, c = _cfg()
    m = ResNet50(device=cuda)
    m.load_state_dict({k: v.clone() for k, v in state.items()})
    t = ResNetTrainer(m, lr=c["lr"], compute_dtype=torch.bfloat16, static_loss_scale=128.0)
    t.refresh_working_copies()
    return t.eval_step(x, y)[1]


def test_evaluation_of_the_average(cuda):
    x, y = _batch(cuda)
    xe, ye = _batch(cuda, 1)
    m, t = _build(cuda)
    for k in range(2):
        t.train_step(x, y, step=k)
    loss_e, le = t.eval_step(xe, ye, ema=True)
    assert not t.ema_dirty and torch.isfinite(le).all() and torch.isfinite(loss_e).all()
    assert torch.equal(le, _fresh_eval_logits(cuda, t.ema_model.state_dict(), xe, ye))
    plain = t.eval_step(xe, ye)[1]
    assert not torch.equal(le, plain)
    assert torch.equal(plain, _fresh_eval_logits(cuda, m.state_dict(), xe, ye))
    assert torch.equal(t.infer(xe, ema=True), le)                       # (clean copies: nothing is re-cast, nothing changes)
    # one more update: the 16-bit copies of the average are stale and the next averaged inference refreshes them
    t.train_step(x, y, step=2)
    assert t.ema_dirty
    le2 = t.eval_step(xe, ye, ema=True)[1]
    assert not t.ema_dirty and not torch.equal(le2, le)
    assert torch.equal(le2, _fresh_eval_logits(cuda, t.ema_model.state_dict(), xe, ye))


def test_checkpoint_carries_the_average(cuda, tmp_path):
    from deeplearningexamples_amd.utils import checkpoint as CK
    x, y = _batch(cuda)
    m1, t1 = _build(cuda)
    for k in range(2):
        t1.train_step(x, y, step=k)
    st = CK.rn50_trainer_state(t1, epoch=1, best_prec1=3.0)
    assert list(st["state_dict_ema"]) == list(st["state_dict"])
    assert int(st["state_dict"]["bn1.num_batches_tracked"]) == 2 and int(st["state_dict_ema"]["bn1.num_batches_tracked"]) == 0
    for k in st["state_dict"]:
        assert st["state_dict_ema"][k].shape == st["state_dict"][k].shape and st["state_dict_ema"][k].stride() == st["state_dict"][k].stride()
    torch.save(st, tmp_path / "ck.pth.tar")
    load = lambda: torch.load(tmp_path / "ck.pth.tar", map_location=cuda, weights_only=False)  # noqa: E731
    # a trainer built from DIFFERENT weights and resumed continues the average identically
    m2, t2 = _build(cuda, seeded=False, seed=2)
    assert (CK.rn50_trainer_load(t2, load())) == (1, 3.0) and t2.ema_dirty
    shadow = _cpu(load()["state_dict_ema"])
    _assert_ema_equals(t2, shadow, "after load")
    _assert_ema_equals(t1, shadow, "the saved trainer")
    for k in (2, 3):
        t2.train_step(x, y, step=k)
        ema_update_(shadow, _cpu(m2.state_dict()), MU, k)
        _assert_ema_equals(t2, shadow, "resumed step %d" % k)
    assert torch.equal(t2.eval_step(x, y, ema=True)[1], _fresh_eval_logits(cuda, t2.ema_model.state_dict(), x, y))
    # no state_dict_ema in the file: the average is re-seeded from the model that was just loaded
    m3, t3 = _build(cuda, seeded=False, seed=3)
    t3.train_step(x, y, step=0)                                         # (an average that has already moved away from its model)
    ck = load()
    del ck["state_dict_ema"]
    CK.rn50_trainer_load(t3, ck)
    _assert_ema_equals(t3, _cpu(m3.state_dict()), "re-seeded")
    _assert_ema_equals(t3, _cpu(ck["state_dict"]), "re-seeded from the file's model")
    assert torch.equal(t3.eval_step(x, y, ema=True)[1], t3.eval_step(x, y)[1])
    # a trainer without the average ignores the key
    m4, t4 = _build(cuda, ema=None, seeded=False, seed=4)
    assert CK.rn50_trainer_load(t4, load()) == (1, 3.0) and t4.ema_model is None
    assert "state_dict_ema" not in CK.rn50_trainer_state(t4, epoch=1)
    for (n, a), (_, b) in zip(m4.state_dict().items(), st["state_dict"].items()):
        assert torch.equal(a, b), n


def test_command_line_trains_validates_and_saves_the_average(cuda, tmp_path):
    from deeplearningexamples_amd.convnets import main as rn
    common = ["--data-backend", "synthetic", "--amp", "--use-ema", "0.999", "--epochs", "1", "--prof", "2", "--steps-per-epoch", "2",
              "--batch-size", "8", "--image-size", "64", "--num-classes", "16", "--lr", "0.01", "--print-freq", "1", "--seed", "3"]
    ws = tmp_path / "ws"
    t = rn.main(common + ["--workspace", str(ws)])
    assert t.ema == 0.999 and t.steps_done == 2
    ck = torch.load(ws / "checkpoint.pth.tar", map_location="cpu", weights_only=False)
    assert list(ck["state_dict_ema"]) == list(ck["state_dict"])
    assert not torch.equal(ck["state_dict_ema"]["fc.weight"], ck["state_dict"]["fc.weight"])
    recs = [json.loads(l[5:]) for l in open(ws / "experiment_raport.json")]
    data = [r.get("data", {}) for r in recs]
    assert any("val_ema.top1" in d and "val_ema.top5" in d and "val_ema.loss" in d for d in data)
    assert any("val.top1" in d for d in data)
    # --evaluate --use-ema X --resume F reports both models
    ws2 = tmp_path / "ws2"
    t2 = rn.main(common + ["--workspace", str(ws2), "--resume", str(ws / "checkpoint_0000.pth.tar"), "--evaluate", "--epochs", "2"])
    data2 = [json.loads(l[5:]).get("data", {}) for l in open(ws2 / "experiment_raport.json")]
    assert any("val_ema.top1" in d for d in data2) and any("val.top1" in d for d in data2)
    assert torch.equal(t2.ema_model.fc.weight.cpu(), ck["state_dict_ema"]["fc.weight"])


def test_captured_step_carries_the_average(cuda):
    from deeplearningexamples_amd.utils.graph import GraphedStep
    RO, c = _cfg()
    batches = [[b.to(cuda) for b in RO.seeded_batch(c["seed"] + 200 + i, 8, c["size"])] for i in range(5)]
    m1, t1 = _build(cuda)
    eager = [float(t1.train_step(*b, step=k).item()) for k, b in enumerate(batches)]
    m2, t2 = _build(cuda)
    step = GraphedStep(t2.train_step, warmup_steps=2)
    graphed = []
    for k, b in enumerate(batches):
        t2.set_ema_step(k)                                              # the captured step reads the decay from the device
        graphed.append(float(step(*b).item()))
    assert step.graph is not None
    np.testing.assert_allclose(graphed, eager, rtol=2e-6)               # (the loss reduction uses fp32 atomics)
    s1, s2 = m1.state_dict(), m2.state_dict()
    same_params = all(torch.equal(s1[k], s2[k]) for k in s1 if not k.endswith("num_batches_tracked"))
    e1, e2 = t1.ema_model.state_dict(), t2.ema_model.state_dict()
    for k in e1:
        if same_params:
            assert torch.equal(e1[k], e2[k]), "parameters bit-identical, so the averages must be too: %s" % k
        else:
            assert torch.allclose(e1[k].float(), e2[k].float(), rtol=1e-4, atol=1e-6), \
                "parameters differ within the fp32-atomic noise, averages compared under the same allclose terms: %s" % k
    # the replays ran no Python: set_ema_step() is what marked the average's 16-bit copies stale
    assert t2.ema_dirty
    x, y = batches[0]
    assert torch.equal(t2.eval_step(x, y, ema=True)[1], _fresh_eval_logits(cuda, e2, x, y))
