"""BratsSegmenter (deeplearningexamples_amd/nnunet/infer.py) against the reference's recorded float64 outputs and the float64
restatement of tests/_nnunet_ref.py, with the project's yardstick: E_new <= 1.5 E_emulated, E the largest absolute logit error and
E_emulated that of the reference's own --amp arithmetic emulated in float64.  Both are computed here and printed."""
import functools
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.nnunet import model as M
from deeplearningexamples_amd.nnunet.infer import BratsSegmenter
from tests import _exact_grid as G
from tests import _nnunet_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEV = "cuda"
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
VOLUME, PATCH = (5, 12, 20, 12), (8, 8, 8)


@functools.lru_cache(maxsize=None)
def state(levels):
    return M.seeded_state(levels, R.WEIGHT_SEED)


@functools.lru_cache(maxsize=None)
def recorded(tag):
    return torch.from_numpy(np.load(os.path.join(GOLDEN, "nnunet_unet3d.npz"))[tag])


@functools.lru_cache(maxsize=None)
def emulated_patch(tag, dtype):
    levels, shape, seed = R.GEOMETRIES[tag]
    return R.unet3d(state(levels), R.seeded_input(shape, seed), "amp", dtype)


@functools.lru_cache(maxsize=None)
def segmenter(levels, dtype, graphs=False, patch=PATCH, batch=1):
    return BratsSegmenter(state(levels), dtype, graphs=graphs, patch_size=patch, val_batch_size=batch)


# ---------------------------------------------------------------------------------------------- one patch
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", sorted(R.GEOMETRIES))
def test_logits_patch_against_recorded_reference(tag, dtype):
    levels, shape, seed = R.GEOMETRIES[tag]
    x = R.seeded_input(shape, seed)
    want = recorded(tag)
    got = segmenter(levels, dtype).logits_patch(x.to(DEV)).cpu().double()
    assert got.shape == want.shape
    e_new, e_emul = float((got - want).abs().max()), float((emulated_patch(tag, dtype) - want).abs().max())
    print("%s %s: E_new %.4g, E_emulated %.4g" % (tag, dtype, e_new, e_emul))
    assert e_new <= 1.5 * e_emul, (e_new, e_emul)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sample_in_a_batch_equals_the_sample_alone(dtype):
    levels, shape, seed = R.GEOMETRIES["l2"]
    x = R.seeded_input(shape, seed).to(DEV)
    seg = segmenter(levels, dtype)
    both = seg.logits_patch(x).clone()
    for n in range(shape[0]):
        alone = seg.logits_patch(x[n:n + 1])
        G.assert_same(G.bits(alone[0].cpu()), G.bits(both[n].cpu()), "sample %d" % n)
    assert torch.equal(seg.forward(x), torch.argmax(both, 1))


# ---------------------------------------------------------------------------------------------- sliding window
@functools.lru_cache(maxsize=None)
def volume():
    return R.seeded_input(VOLUME, 77)


@functools.lru_cache(maxsize=None)
def window_logits(mode, dtype):
    """The model's float64 (or emulated) logits of every distinct window of the test volume, computed once: window origin -> logits."""
    sd, out = state(2), {}
    for overlap in (0.25, 0.5):
        for o in R.windows(VOLUME[1:], PATCH, overlap):
            if o not in out:
                w = volume()[:, o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8][None]
                out[o] = R.unet3d(sd, w, mode, dtype)
    return out


def reference_segment(mode, dtype, overlap, blend):
    table = window_logits(mode, dtype)
    vol = volume()

    def predict(win):                                   # the restatement asks window by window: look the window up by its content
        for o, logits in table.items():
            if torch.equal(win[0], vol[:, o[0]:o[0] + 8, o[1]:o[1] + 8, o[2]:o[2] + 8]):
                return logits
        raise AssertionError("window not in the table")
    return R.sliding_window(predict, vol, PATCH, overlap, blend)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("blend", ["constant", "gaussian"])
@pytest.mark.parametrize("overlap", [0.25, 0.5])
def test_segment_against_float64_restatement(overlap, blend, dtype):
    want = reference_segment("exact", None, overlap, blend)
    emul = reference_segment("amp", dtype, overlap, blend)
    got = segmenter(2, dtype, batch=3).segment(volume().to(DEV), overlap=overlap, blend=blend).cpu().double()
    assert got.shape == want.shape == (3,) + VOLUME[1:]
    e_new, e_emul = float((got - want).abs().max()), float((emul - want).abs().max())
    print("overlap %s %s %s: E_new %.4g, E_emulated %.4g" % (overlap, blend, dtype, e_new, e_emul))
    assert e_new <= 1.5 * e_emul, (e_new, e_emul)


def test_segment_pads_a_small_volume():
    vol = volume()[:, :5, :8, :11]                      # 5 < 8 along d: one voxel of zeros in front, two behind
    sd = state(2)
    want = R.sliding_window(lambda w: R.unet3d(sd, w), vol, PATCH, 0.25, "gaussian")
    emul = R.sliding_window(lambda w: R.unet3d(sd, w, "amp", HF), vol, PATCH, 0.25, "gaussian")
    got = segmenter(2, HF).segment(vol.to(DEV), overlap=0.25, blend="gaussian").cpu().double()
    assert got.shape == want.shape == (3, 5, 8, 11)
    e_new, e_emul = float((got - want).abs().max()), float((emul - want).abs().max())
    print("small volume: E_new %.4g, E_emulated %.4g" % (e_new, e_emul))
    assert e_new <= 1.5 * e_emul, (e_new, e_emul)


def test_tta_is_the_mean_of_the_eight_flips():
    """nn_unet.py:55,212-217: flips over the volume axes [2], [3], [4], [2,3], [2,4], [3,4], [2,3,4] of the batch (here 1, 2, 3 of the
    volume), each prediction flipped back, the mean of the eight.  Composed here from plain segment() calls, bit for bit, and held
    to the float64 restatement of the whole."""
    seg, vol = segmenter(2, HF, batch=3), volume().to(DEV)
    got = seg.segment(vol, overlap=0.25, blend="constant", tta=True)
    total = seg.segment(vol, 0.25, "constant")
    for ax in ([1], [2], [3], [1, 2], [1, 3], [2, 3], [1, 2, 3]):
        total = total + torch.flip(seg.segment(torch.flip(vol, ax), 0.25, "constant"), ax)
    G.assert_same(G.bits((total / 8).cpu()), G.bits(got.cpu()), "tta")
    sd = state(2)
    want = R.tta(lambda v: R.sliding_window(lambda w: R.unet3d(sd, w), v, PATCH, 0.25, "constant"), volume())
    emul = R.tta(lambda v: R.sliding_window(lambda w: R.unet3d(sd, w, "amp", HF), v, PATCH, 0.25, "constant"), volume())
    e_new, e_emul = float((got.cpu().double() - want).abs().max()), float((emul - want).abs().max())
    print("tta: E_new %.4g, E_emulated %.4g" % (e_new, e_emul))
    assert e_new <= 1.5 * e_emul, (e_new, e_emul)
    assert not torch.equal(got, seg.segment(vol, 0.25, "constant"))                          # the flips are no no-ops on this volume


# ---------------------------------------------------------------------------------------------- launches, host reads, graphs
def test_launch_list_six_levels_and_no_host_reads(monkeypatch):
    """The task-11 network (six levels, 22 convolutions) on a 32^3 patch, N = 2, with zero weights allocated on the device."""
    sd = {k: torch.zeros(s, device=DEV) for k, s in M.state_shapes(6).items()}
    seg = BratsSegmenter(sd, HF, patch_size=(32, 32, 32), val_batch_size=2)
    x = torch.randn(2, 5, 32, 32, 32, device=DEV)
    seg.logits_patch(x)                                 # allocates the plan
    vol = torch.randn(5, 32, 32, 48, device=DEV)
    seg.segment(vol, overlap=0.5)                       # ... and the volume geometry: windows at w = 0, 16
    names, reads = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: reads.append("synchronize"))
    out = seg.logits_patch(x)
    patch_names = list(names)
    del names[:]
    seg_out = seg.segment(vol, overlap=0.5)
    monkeypatch.undo()
    assert reads == [], reads
    assert patch_names == seg.launch_list(2, 32, 32, 32) == names       # two windows = one batch of two
    count = lambda n: sum(1 for k in patch_names if k == n)
    assert count("dle_conv3d_in_fwd") == 22 and count("dle_upsample3d_x2_fwd") == 5 and count("dle_nnunet_head_blend_fwd") == 2
    assert count("dle_instnorm_fold") == 21 + 5 and len(patch_names) == 22 + 5 + 26 + 2
    assert patch_names[0] == "dle_conv3d_in_fwd" and patch_names[-2:] == ["dle_nnunet_head_blend_fwd"] * 2
    # zero weights: every logit is the output block's bias, 0
    assert out.shape == (2, 3, 32, 32, 32) and float(out.abs().max()) == 0.0 and bool(torch.isfinite(seg_out).all())
    with pytest.raises(ValueError):
        seg.logits_patch(torch.zeros(1, 5, 24, 32, 32, device=DEV))     # 24 does not halve five times


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_equals_eager(dtype):
    levels, shape, seed = R.GEOMETRIES["l3"]
    eager, graphed = segmenter(levels, dtype), segmenter(levels, dtype, graphs=True)
    for s in (seed, seed + 1, seed + 2, seed + 3):      # two warm-up calls, the capture, a replay
        x = R.seeded_input(shape, s).to(DEV)
        G.assert_same(G.bits(graphed.logits_patch(x).cpu()), G.bits(eager.logits_patch(x).cpu()), "seed %d" % s)
    assert graphed._graphs[("logits", shape[0]) + tuple(shape[2:])].graph is not None
    e2, g2 = segmenter(2, dtype, batch=3), segmenter(2, dtype, graphs=True, batch=3)
    vol = volume().to(DEV)
    for _ in range(2):                                  # 12 windows in batches of 3: warm-up, capture and replays inside one volume
        G.assert_same(G.bits(g2.segment(vol, 0.25, "gaussian").cpu()), G.bits(e2.segment(vol, 0.25, "gaussian").cpu()), "segment")
    assert g2._graphs[("features", 3) + PATCH].graph is not None


# ---------------------------------------------------------------------------------------------- checkpoint and command line
def write_ckpt(path, levels):
    import argparse
    torch.save({"epoch": 3, "state_dict": {"model." + k: v for k, v in state(levels).items()},
                "hyper_parameters": {"args": argparse.Namespace(task="11", brats22_model=True), "triton": False}}, path)


def test_checkpoint_round_trip(tmp_path):
    path = str(tmp_path / "epoch=3-dice=88.00.ckpt")
    write_ckpt(path, 2)
    sd, hp = M.load_checkpoint(path)
    assert hp["task"] == "11"
    levels, shape, seed = R.GEOMETRIES["l2"]
    x = R.seeded_input(shape, seed).to(DEV)
    G.assert_same(G.bits(BratsSegmenter(sd, HF, patch_size=PATCH).logits_patch(x).cpu()), G.bits(segmenter(2, HF).logits_patch(x).cpu()),
                  "checkpoint against the state it was written from")


def data_dir(tmp_path, n=6):
    """A synthetic preprocessed directory: n volumes [5, 12, 16, 12], labels, metas, config.pkl with patch 8^3 (two levels at
    --min_fmap 4)."""
    d = tmp_path / "12_3d" / "test"
    d.mkdir(parents=True)
    for i in range(n):
        x = R.seeded_input((5, 12, 16, 12), 200 + i).float().numpy()
        np.save(str(d / ("BraTS_%02d_x.npy" % i)), x)
        np.save(str(d / ("BraTS_%02d_y.npy" % i)), (np.arange(12 * 16 * 12).reshape(1, 12, 16, 12) % 4).astype(np.uint8))
        np.save(str(d / ("BraTS_%02d_meta.npy" % i)), np.array([[1, 2, 3], [13, 18, 15], [15, 20, 16], [12, 16, 12]]))
    pickle.dump({"patch_size": [8, 8, 8], "spacings": [1.0, 1.0, 1.0], "n_class": 4, "in_channels": 5}, open(str(d / "config.pkl"), "wb"))
    return str(d)


def run_main(argv):
    r = subprocess.run([sys.executable, "-m", "deeplearningexamples_amd.nnunet.main"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_command_line_predict_saves_predictions(tmp_path):
    d, ckpt, res = data_dir(tmp_path, 2), str(tmp_path / "epoch=3-dice=88.00.ckpt"), str(tmp_path / "results")
    write_ckpt(ckpt, 2)
    run_main(["--exec_mode", "predict", "--brats", "--brats22_model", "--amp", "--task", "12", "--data", d, "--ckpt_path", ckpt,
              "--results", res, "--save_preds", "--overlap", "0.5", "--blend", "gaussian", "--val_batch_size", "2"])
    out_dir = os.path.join(res, "predictions_epoch=3-dice=88_00_task=12_fold=0")
    assert sorted(os.listdir(out_dir)) == ["BraTS_00.npy", "BraTS_01.npy"]
    pred = np.load(os.path.join(out_dir, "BraTS_01.npy"))
    assert pred.shape == (3, 15, 20, 16) and pred.dtype == np.float64
    # the same volume in this process: expit of the logits inside the crop box, expit(0) = 0.5 outside
    vol = torch.from_numpy(np.load(os.path.join(d, "BraTS_01_x.npy"))).to(DEV)
    logits = segmenter(2, HF, batch=2).segment(vol, overlap=0.5, blend="gaussian").cpu().double().numpy()
    assert np.array_equal(pred[:, 1:13, 2:18, 3:15], 1.0 / (1.0 + np.exp(-logits)))
    outside = np.ones(pred.shape, dtype=bool)
    outside[:, 1:13, 2:18, 3:15] = False
    assert np.all(pred[outside] == 0.5)


def test_command_line_benchmark_and_evaluate(tmp_path):
    d, ckpt, res = data_dir(tmp_path, 6), str(tmp_path / "last.ckpt"), str(tmp_path / "results")
    write_ckpt(ckpt, 2)
    out = run_main(["--exec_mode", "predict", "--brats", "--brats22_model", "--amp", "--task", "12", "--data", d, "--ckpt_path", ckpt,
                    "--results", res, "--benchmark", "--val_batch_size", "2", "--test_batches", "5", "--logname", "perf.json"])
    stats = {l.split(" : ")[0][len("DLL - "):]: float(l.split(" : ")[1]) for l in out.splitlines() if l.startswith("DLL - ")}
    assert set(stats) == {"throughput_predict", "latency_predict_mean", "latency_predict_90", "latency_predict_95", "latency_predict_99"}
    assert stats["throughput_predict"] > 0 and stats["latency_predict_mean"] <= stats["latency_predict_99"]
    assert abs(stats["throughput_predict"] * stats["latency_predict_mean"] / 1000 - 2) <= 0.02
    assert os.path.exists(os.path.join(res, "perf.json"))
    out = run_main(["--exec_mode", "evaluate", "--brats", "--brats22_model", "--bf16", "--task", "12", "--data", d, "--ckpt_path", ckpt,
                    "--results", res, "--tta"])
    line = [l for l in out.splitlines() if l.startswith("DLL - {")]
    assert len(line) == 1 and 0.0 <= __import__("json").loads(line[0][len("DLL - "):])["Dice"] <= 100.0
