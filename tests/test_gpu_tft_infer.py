"""TFTForecaster (deeplearningexamples_amd/tft/infer.py) against the float64 forward of tests/_tft_ref.py, its launch list, the
absence of host reads and the command line.  GPU only.

Cases: 'elec' (one static categorical, three known continuous, one target: the shape of both published datasets) and 'obs' (two
static continuous variables, one observed continuous, two known, one target, no categorical), each at (T, encoder_length) =
(12, 8) and (40, 33), batch 5, hidden 128, fp16 and bf16, weights and inputs from seeds (tests/_tft_ref.seeded_state / seeded_batch).

Reference.  _tft_ref.forward(Mode('exact')): float64, nothing rounded; tests/test_tft_host.py pins it to the host model and to the
reference's recorded forecasts.  Yardstick, the project's established one: the same chain with every value rounded to the 16-bit
type where the forecaster rounds (Mode('emul'): 16-bit weights and tables, every kernel's output, the ELU and lin_i images inside
a GRN, h per step, q | k | v, the mean probabilities and the context as operands; fp32 input projections, selection weights,
quantile tail).  With E the RMS error of the forecasts against the unrounded forward: E_new <= 1.5 E_emulated; the factor and its
justification are those of tests/test_gpu_resnext_infer.py (the forecaster's fp32 accumulations are not the emulation's float64
ones, so the two sets of roundings fall differently: equal in distribution, not in value).  Both values are printed.
On the MI355X (a record): E_new / E_emulated 0.985 - 1.024 in fp16 (E_emulated 4.7e-4, 4.8e-4, 4.7e-4, 1.7e-3 for the four cases),
0.979 - 0.985 in bf16 (4.6e-3, 4.0e-3, 3.8e-3, 6.3e-3); forecasts of rms 1.0 - 1.2.  Command line: q-risk within 7e-4 (fp16) and
4e-3 (bf16) of the float64 forward's, bars 2.2e-3 and 2.7e-2.
"""
import functools

import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.tft import model as TM
from deeplearningexamples_amd.tft.infer import TFTForecaster
from tests import _tft_ref as R

pytestmark = pytest.mark.gpu

HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
CASES = [("elec", 12, 8), ("elec", 40, 33), ("obs", 12, 8), ("obs", 40, 33)]
CASE_IDS = ["%s_T%d_enc%d" % c for c in CASES]
BATCH = 5
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def case(kind, T, enc):
    cfg = R.small_config(kind, T, enc)
    sd = R.seeded_state(cfg, 11)
    batch = R.seeded_batch(cfg, BATCH, 12)
    exact = R.forward(R.Mode("exact"), sd, cfg, batch)
    return cfg, sd, batch, exact


@functools.lru_cache(maxsize=None)
def forecaster(kind, T, enc, dtype):
    cfg, sd, _, _ = case(kind, T, enc)
    m = TM.TemporalFusionTransformer(cfg)
    m.load_state_dict(sd)
    return TFTForecaster(m.eval(), dtype=dtype)


def on_dev(batch, rows=None):
    return {k: (None if v is None else (v if rows is None else v[rows]).to(DEV)) for k, v in batch.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_forecast_against_float64(c, dtype):
    cfg, sd, batch, exact = case(*c)
    fc = forecaster(*c, dtype)
    out, hist_w, fut_w, probs = fc.forecast(on_dev(batch), explain=True)
    assert out.dtype == torch.float32 and tuple(out.shape) == (BATCH, c[1] - c[2], 3) and out.is_cuda
    emu = R.forward(R.Mode("emul", dtype), sd, cfg, batch)
    rms = lambda a, b: float((a.double().cpu() - b).pow(2).mean().sqrt())
    e_new, e_emu = rms(out, exact["out"]), rms(emu["out"], exact["out"])
    print("%s %s: E_new %.4e  E_emulated %.4e  ratio %.3f  (rms forecast %.3f)" % (c, dtype, e_new, e_emu, e_new / e_emu,
                                                                                   float(exact["out"].pow(2).mean().sqrt())))
    assert e_new <= 1.5 * e_emu, "RMS forecast error %.4e against %.4e of the emulated roundings" % (e_new, e_emu)
    # the explanations: weights against float64 under the same yardstick, rows summing to one, nothing behind the mask
    for name, got in (("hist_w", hist_w), ("fut_w", fut_w), ("probs", probs)):
        g_new, g_emu = rms(got, exact[name]), rms(emu[name], exact[name])
        print("   %s: E_new %.3e  E_emulated %.3e" % (name, g_new, g_emu))
        assert g_new <= 1.5 * g_emu + 2.0 ** -22, name
        assert float((got.double().sum(-1) - 1).abs().max()) <= (got.shape[-1] + 8) * 2.0 ** -24
    T, enc = c[1], c[2]
    behind = torch.arange(T)[None, :] > torch.arange(enc, T)[:, None]
    assert float(probs.cpu()[:, behind].abs().max()) == 0.0
    # explain changes nothing
    assert torch.equal(fc.forecast(on_dev(batch)), out)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", [CASES[0], CASES[3]], ids=[CASE_IDS[0], CASE_IDS[3]])
def test_batch_equals_alone_and_the_future_target_is_not_read(c, dtype):
    cfg, sd, batch, _ = case(*c)
    fc = forecaster(*c, dtype)
    out = fc.forecast(on_dev(batch))
    for b in (0, BATCH - 1):
        alone = fc.forecast(on_dev(batch, slice(b, b + 1)))
        assert torch.equal(alone[0], out[b]), "row %d alone and in the batch differ" % b
    changed = dict(batch)
    changed["target"] = batch["target"].clone()
    changed["target"][:, c[2]:] = float("nan")                       # whatever the target holds behind the encoder, NaN included
    assert torch.equal(fc.forecast(on_dev(changed)), out), "the target behind encoder_length reached the forecast"
    changed["target"][:, c[2] - 1] += 1.0
    assert not torch.equal(fc.forecast(on_dev(changed)), out), "the last encoder step of the target did not reach the forecast"


def test_explanations_are_the_kernels_own():
    """The selection weights and the mean probabilities that forecast(explain=True) returns are bit for bit what the kernels
    return when called on the forecaster's own intermediate tensors (recomputed here through functional)."""
    from deeplearningexamples_amd import functional as F
    c = CASES[2]
    cfg, sd, batch, _ = case(*c)
    fc = forecaster(*c, HF)
    b = on_dev(batch)
    out, hist_w, fut_w, probs = fc.forecast(b, explain=True)
    T, enc = c[1], c[2]
    sctx = F.tft_vsn_fwd([b["s_cont"].float()], fc.s_vsn, HF, 1).view(BATCH, 128)
    cs = F.tft_grn_fwd(sctx, fc.ctx_grns[0])
    _, w1 = F.tft_vsn_fwd([b["o_cont"], b["k_cont"], b["target"]], fc.hist_vsn, HF, enc, ctx=cs, want_weights=True)
    _, w2 = F.tft_vsn_fwd([b["k_cont"]], fc.fut_vsn, HF, T - enc, t0=enc, ctx=cs, want_weights=True)
    assert torch.equal(w1, hist_w) and torch.equal(w2, fut_w)
    assert tuple(probs.shape) == (BATCH, T - enc, T)


def test_launch_list_and_no_host_reads(monkeypatch):
    c = CASES[1]
    cfg, sd, batch, _ = case(*c)
    fc = forecaster(*c, BF)
    b = on_dev(batch)
    b["s_cat"] = b["s_cat"].to(torch.int32)
    fc.forecast(b)                                                     # warm: nothing lazily built is counted below
    names, copies = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (copies.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (copies.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.Tensor, "numpy", (lambda real_np: lambda self, *a, **k: (copies.append("numpy") if self.is_cuda else None,
                                                                                           real_np(self, *a, **k))[1])(torch.Tensor.numpy))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: copies.append("synchronize"))
    fc.forecast(b, explain=True)
    monkeypatch.undo()
    assert copies == [], copies
    g, v, l, a, m = "dle_tft_grn_fwd", "dle_tft_vsn_fwd", "dle_tft_lstm_fwd", "dle_tft_attention_fwd", "dle_gemm"
    assert names == [g] * 5 + [v, v, m, l, l, g, g, m, a, g, g, g], names
    # continuous static variables: the static selection is the VSN kernel, the rest is the same
    del names[:]
    c2 = CASES[2]
    fc2 = forecaster(*c2, BF)
    b2 = on_dev(case(*c2)[2])
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    fc2.forecast(b2)
    monkeypatch.undo()
    assert names == [v] + [g] * 4 + [v, v, m, l, l, g, g, m, a, g, g, g], names


def test_one_line_rejections():
    cfg = R.small_config("elec", 12, 8, hidden=64)
    with pytest.raises(ValueError, match="hidden_size 128"):
        TFTForecaster(TM.TemporalFusionTransformer(cfg))
    cfg = R.small_config("elec", 12, 8)
    with pytest.raises(ValueError, match="16 bits"):
        TFTForecaster(TM.TemporalFusionTransformer(cfg), dtype=torch.float32)
    fc = forecaster("elec", 12, 8, HF)
    b = on_dev(case("elec", 12, 8)[2])
    b["k_cat"] = torch.zeros(BATCH, 12, 1, dtype=torch.long, device=DEV)
    with pytest.raises(NotImplementedError, match="temporal categorical"):
        fc.forecast(b)


@pytest.mark.parametrize("amp", ["fp16", "bf16"])
def test_command_line(amp, tmp_path):
    """A hidden-size-128 checkpoint in the reference's form, a small CSV split and pickled per-id scalers; the command line runs in
    a fresh child process.  Its q-risk line against the q-risk of the float64 forward on the same examples: the quantile loss is
    0.9-Lipschitz in the forecast, so |risk - risk_64| <= 2 * 0.9 * max(scale) * mean|forecast error| / mean|target|, and
    mean|error| <= RMS error E <= 1.5 E_emulated (the bound of test_forecast_against_float64)."""
    import os
    import pickle
    import re
    import subprocess
    import sys
    import numpy as np
    from deeplearningexamples_amd.tft import data as D
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = TM.ElectricityConfig(example_length=12, encoder_length=8, static_categorical_inp_lens=[11])
    sd = R.seeded_state(cfg, 21)
    torch.save({"config": cfg, "model": sd}, str(tmp_path / "checkpoint.pt"))
    rng = np.random.RandomState(3)
    cols = ["id", "hours_from_start", "power_usage", "hour", "day_of_week", "categorical_id"]
    with open(str(tmp_path / "test.csv"), "w") as f:
        f.write("," + ",".join(cols) + "\n")
        n = 0
        for sid in (0, 1, 2):
            for t in range(14):
                f.write("%d,%d,%r,%r,%r,%r,%d\n" % (n, sid, float(t) / 14, rng.randn(), rng.randn(), rng.randn(), sid))
                n += 1
    scalers = {i: R.Scaler(0.5 * i, 1.0 + 0.5 * i) for i in range(3)}
    pickle.dump(scalers, open(str(tmp_path / "tgt_scalers.bin"), "wb"))
    pickle.dump({}, open(str(tmp_path / "cat_encodings.bin"), "wb"))
    argv = [sys.executable, "-m", "deeplearningexamples_amd.tft.inference", "--checkpoint", str(tmp_path / "checkpoint.pt"), "--data",
            str(tmp_path / "test.csv"), "--tgt_scalers", str(tmp_path / "tgt_scalers.bin"), "--cat_encodings", str(tmp_path / "cat_encodings.bin"),
            "--batch_size", "4", "--save_predictions", "--results", str(tmp_path / "results"), "--amp", "--amp-dtype", amp]
    r = subprocess.run(argv, cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"Test q-risk: P10 (\S+) \| P50 (\S+) \| P90 (\S+)", r.stdout)
    assert m and "Latency:\n\tAverage " in r.stdout and "\tp99 " in r.stdout, r.stdout
    got = np.array([float(x) for x in m.groups()])
    # the same examples through the float64 forward and the emulated one
    ds = D.TFTDataset(str(tmp_path / "test.csv"), cfg)
    assert len(ds) == 9
    batch = next(D.batches(ds, 9))
    b = {k: (v if v.numel() else None) for k, v in batch.items() if k != "id"}
    dtype = HF if amp == "fp16" else BF
    exact = R.forward(R.Mode("exact"), sd, cfg, b)["out"]
    emu = R.forward(R.Mode("emul", dtype), sd, cfg, b)["out"]
    ids = batch["id"][:, 0, 0].numpy()
    un = lambda v: D.unscale_per_id(v, ids, scalers)
    u_pred = np.stack([un(exact[:, :, i].numpy()) for i in range(3)], -1)
    u_tgt = un(batch["target"][:, 8:, 0].numpy())[:, :, None]
    want = D.qrisk(u_pred, u_tgt, np.array(cfg.quantiles))
    e_emu = float((emu - exact).pow(2).mean().sqrt())
    bar = 2 * 0.9 * 2.0 * 1.5 * e_emu / np.abs(u_tgt).mean()
    print("q-risk %s against %s of the float64 forward; bar %.3e (E_emulated %.3e)" % (got, want, bar, e_emu))
    assert np.abs(got - want).max() <= bar
    for sid in (0, 1, 2):
        d = tmp_path / "results" / "predictions" / str(sid)
        assert sorted(os.listdir(str(d))) == ["P10.csv", "P50.csv", "P90.csv", "targets.csv"]
        rows = [l.strip().split(",") for l in open(str(d / "targets.csv"))]
        assert rows[0] == [""] + ["t+%d" % (i + 1) for i in range(4)] and len(rows) == 1 + 3
        saved = np.array([[float(x) for x in row[1:]] for row in rows[1:]])
        assert np.array_equal(saved, u_tgt[ids == sid, :, 0])
        p50 = np.array([[float(x) for x in l.strip().split(",")[1:]] for l in list(open(str(d / "P50.csv")))[1:]])
        assert np.abs(p50 - u_pred[ids == sid, :, 1]).max() <= 2.0 * 40 * 1.5 * e_emu            # per element: far inside 40 RMS


@pytest.mark.parametrize("c", [CASES[1], CASES[2]], ids=[CASE_IDS[1], CASE_IDS[2]])
def test_graph_replay_equals_eager(c):
    """graphs=True: two eager warm-up calls, the capture and replays, each on other inputs, against the eager forecaster."""
    cfg, sd, _, _ = case(*c)
    eager = forecaster(*c, HF)
    m = TM.TemporalFusionTransformer(cfg)
    m.load_state_dict(sd)
    graphed = TFTForecaster(m.eval(), dtype=HF, graphs=True)
    for i in range(5):
        b = on_dev(R.seeded_batch(cfg, BATCH, 30 + i))
        want = eager.forecast(b, explain=True)
        got = graphed.forecast(b, explain=True)
        for w, g in zip(want, got):
            assert torch.equal(w, g), "call %d" % i
    assert graphed._graphs[(BATCH, c[1], True)].graph is not None
