"""MoFlowGenerator on the fixture checkpoint against the reference's recorded float64 results (tests/golden/moflow_reverse.npz).

Yardstick, as for the other front ends (tests/test_gpu_resnext_infer.py): E_new <= 1.5 E_emulated, E the largest absolute error
against the reference's float64 result, E_emulated that of the generator's own rounding points emulated in float64
(tests/_moflow_ref.py, Mode 'emul'); the factor 1.5 leaves room for fp32 accumulation order and for 16-bit roundings that fall the
other way on values the fp32 sums move by an ulp.  The test prints both.

Bond bits: a position is clear when the gap between the two largest exact symmetrised values exceeds twice the h_adj bar
(1.5 E_emulated): an h_adj error within the bar cannot change its decision.  There the bits must be the reference's; at most 10 % of
the positions may be unclear.  x is held against the float64 atom statement fed the generator's OWN bit mask, so a flipped bond is
not charged twice.

A reverse pass is 3 n_flow + 3 library launches: the 2 n_flow GEMMs, n_flow couplings, the decision and the atom launch, and one
dle_mf_squeeze_fwd in front, which makes the fp32 state and the first 16-bit operand out of z."""
import functools
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.moflow import config as MC
from deeplearningexamples_amd.moflow import generate as MG
from deeplearningexamples_amd.moflow import model as MM
from deeplearningexamples_amd.moflow.infer import MoFlowGenerator
from tests import _exact_grid as G
from tests import _moflow_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
HF, BF = torch.float16, torch.bfloat16
DTYPES = [pytest.param(HF, id="fp16"), pytest.param(BF, id="bf16")]
DEV = "cuda"
N, T, FOLD, A_SIZE = 8, 4, 4, 32


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "moflow_reverse.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


@functools.lru_cache(maxsize=None)
def model():
    m = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    MG.load_snapshot(os.path.join(GOLDEN, "moflow_checkpoint.pt"), m)
    return m.eval()


@functools.lru_cache(maxsize=None)
def generator(dtype, graphs=False):
    return MoFlowGenerator(model(), dtype, graphs=graphs)


@functools.lru_cache(maxsize=None)
def emulated_h_adj(dtype):
    fx = fixture()
    return R.bond_reverse(R.Mode("emul", dtype), MM.folded_bond_flows(model()), fx["z"].double()[:, A_SIZE:].reshape(-1, 4, N, N), FOLD).v


@functools.lru_cache(maxsize=None)
def reversed_fixture(dtype):
    return tuple(t.cpu() for t in generator(dtype).reverse_all(fixture()["z"].to(DEV), want_h=True))


@pytest.mark.parametrize("dtype", DTYPES)
def test_h_adj_and_bond_bits(dtype):
    fx = fixture()
    adj, x, mask, code, h = reversed_fixture(dtype)
    e_emu = float((emulated_h_adj(dtype) - fx["h_adj"]).abs().max())
    e_new = float((h.double() - fx["h_adj"]).abs().max())
    print("%s h_adj: E_new %.4e  E_emulated %.4e  ratio %.3f" % (dtype, e_new, e_emu, e_new / e_emu))
    assert e_new <= 1.5 * e_emu
    clear = R.clear_positions(fx["h_adj"], False, 2 * 1.5 * e_emu)
    print("unclear positions: %.2f %%" % (100 * (1 - float(clear.double().mean()))))
    assert float(clear.double().mean()) >= 0.9
    want_mask, want_code, _ = R.decide(fx["h_adj"], False)
    assert torch.equal(R.bits_to_adj(want_mask), fx["adj"].double())              # the rule is the reference's adj on this fixture
    assert torch.equal(mask[clear], want_mask[clear]) and torch.equal(code[clear], want_code[clear])
    assert torch.equal(adj.double(), R.bits_to_adj(mask)) and torch.equal(mask, mask.transpose(1, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_x_against_the_float64_atom_statement(dtype):
    fx = fixture()
    adj, x, mask, code, h = reversed_fixture(dtype)
    m64 = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    m64.load_state_dict(model().state_dict())
    zx = fx["z"].double()[:, :A_SIZE].reshape(-1, N, T)
    want = R.atom_reverse(R.Mode("exact"), MM.folded_atom_flows(m64.double().eval(), torch.float64), R.bits_to_adj(mask), zx, False).v
    emu = R.atom_reverse(R.Mode("emul", dtype), MM.folded_atom_flows(model()), R.bits_to_adj(mask), zx, False).v
    e_emu, e_new = float((emu - want).abs().max()), float((x.double() - want).abs().max())
    print("%s x: E_new %.4e  E_emulated %.4e  ratio %.3f" % (dtype, e_new, e_emu, e_new / e_emu))
    assert e_new <= 1.5 * e_emu
    same = (mask == R.decide(fx["h_adj"], False)[0]).all(dim=2).all(dim=1)       # samples with the reference's bonds: the recorded x
    assert int(same.sum()) >= 20
    assert float((x.double()[same] - fx["x"][same]).abs().max()) <= 1.5 * e_emu


def test_launch_list_and_no_host_read(monkeypatch):
    gen = generator(BF)
    z = fixture()["z"].to(DEV)
    gen.reverse(z)                                                      # warm
    names, reads = [], []
    real = C.call
    monkeypatch.setattr(C, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    real_cpu, real_tolist, real_item = torch.Tensor.cpu, torch.Tensor.tolist, torch.Tensor.item
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu") if self.is_cuda else None, real_cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist") if self.is_cuda else None, real_tolist(self))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item") if self.is_cuda else None, real_item(self))[1])
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: reads.append("synchronize"))
    adj, x = gen.reverse(z)
    code = gen.reverse_all(z)[3]
    n_reverse = len(names) // 2
    gen.decode(code, x)
    monkeypatch.undo()
    n_flow = MC.FIXTURE_CONFIG.model_config.bond_config.n_flow
    want = ["dle_mf_squeeze_fwd"] + ["dle_gemm", "dle_gemm", "dle_mf_couple_fwd"] * n_flow + ["dle_mf_bond_decide_fwd", "dle_mf_atom_reverse_fwd"]
    assert names == want * 2 and n_reverse == 3 * n_flow + 3, names
    assert names.count("dle_gemm") == 4 * n_flow and names.count("dle_mf_couple_fwd") == 2 * n_flow
    assert reads == ["cpu"], reads                                      # decode's one read; none inside reverse
    assert adj.shape == (33, 4, N, N) and x.shape == (33, N, T) and adj.dtype == x.dtype == torch.float32


def test_graph_replay_equals_eager():
    eager, graphed = generator(HF), generator(HF, True)
    for b, seed in ((33, 0), (5, 1), (33, 2), (33, 3), (33, 4)):              # warm-up calls, the capture, replays with new inputs
        z = (torch.randn(b, MC.FIXTURE_CONFIG.z_dim, generator=torch.Generator().manual_seed(seed)) * 0.6).to(DEV)
        for got, want in zip(graphed.reverse_all(z), eager.reverse_all(z)):
            assert torch.equal(G.bits(got), G.bits(want)), (b, seed)
    assert graphed._graphs[("reverse", 33, False)].graph is not None


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_equals_alone(dtype):
    gen, z = generator(dtype), fixture()["z"].to(DEV)
    whole = gen.reverse_all(z)
    for i in (0, 16, 32):
        for got, want in zip(gen.reverse_all(z[i:i + 1].contiguous()), whole):
            assert torch.equal(G.bits(got), G.bits(want[i:i + 1])), i
    assert all(t.shape[0] == 0 for t in gen.reverse_all(z[:0]))


def test_sample_is_reproducible_and_decodes():
    gen = generator(BF)
    runs = []
    for _ in range(2):
        g = torch.Generator(device=DEV).manual_seed(7)
        runs.append(gen.sample(12, temperature=0.6, ln_var=-0.25, generator=g))
    for a, b in zip(*runs):
        assert torch.equal(G.bits(a), G.bits(b))
    z, adj, x, code = runs[0]
    sigma = 0.6 * float(np.sqrt(np.exp(-0.25)))
    assert z.shape == (12, MC.FIXTURE_CONFIG.z_dim) and abs(float(z.std()) - sigma) < 0.05
    atoms, bonds = gen.decode(code, x)
    assert atoms.shape == (12, 7) and bonds.shape == (12, 7, 7) and set(np.unique(atoms)) <= {0, 6, 7, 8} and bonds.max() <= 3
    assert np.array_equal(bonds, torch.argmax(adj, dim=1)[:, :7, :7].cpu().numpy())
    with pytest.raises(ValueError, match="contiguous fp32"):
        gen.reverse(z.double())
    with pytest.raises(C.DleError):
        gen.reverse(z.cpu())


def test_command_line(tmp_path):
    results = tmp_path / "results"
    results.mkdir()
    shutil.copy(os.path.join(GOLDEN, "moflow_checkpoint.pt"), str(results / "model_snapshot_epoch_8"))
    cfg, log, out = str(tmp_path / "cfg.json"), str(tmp_path / "log.json"), str(tmp_path / "out.npz")
    MC.FIXTURE_CONFIG.save(cfg)
    base = ["--amp", "--amp-dtype", "bf16", "--config_path", cfg, "--results_dir", str(results), "--batch_size", "20", "--steps", "6",
            "--warmup_steps", "2", "--log_interval", "3", "--temperature", "0.6", "--seed", "3", "--jit"]
    # one child process (one interpreter start) runs the command line twice: without predictions and with an .npz path
    prog = "import json, sys; from deeplearningexamples_amd.moflow.generate import main; [main(a) for a in json.loads(sys.argv[1])]"
    runs = [base + ["--predictions_path", "", "--log_path", log], base + ["--predictions_path", out]]
    r = subprocess.run([sys.executable, "-c", prog, json.dumps(runs)], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    recs = [json.loads(line[len("DLLL "):]) for line in open(log)]
    final = [q for q in recs if q["type"] == "LOG" and q["step"] == []][-1]["data"]
    for key in ("throughput_generate", "latency_generate_mean", "latency_generate_90", "latency_generate_95", "latency_generate_99",
                "total_time_generate"):
        assert final[key] > 0, key
    got = np.load(out)
    assert got["atoms"].shape == (120, 7) and got["bonds"].shape == (120, 7, 7) and int(got["epoch"]) == 7
    gen, g = generator(BF), torch.Generator(device=DEV).manual_seed(3)           # the same generation in this process: the same molecules
    _, _, x, code = gen.sample(20, 0.6, fixture()["ln_var"], generator=g)
    atoms, bonds = gen.decode(code, x)
    assert np.array_equal(got["atoms"][:20], atoms) and np.array_equal(got["bonds"][:20], bonds)
