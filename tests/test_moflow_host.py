"""MoFlow on the host: the restated model against the reference's recorded float64 results (tests/golden/moflow_*), the regroupings
the kernels rest on (row-only aggregate-first atom flow, folded dense convolution), names / shapes / flags, snapshots, decode, every
one-line rejection, the behaviour without rdkit and the self-test of the error bars of tests/_moflow_ref.py.  No GPU."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from deeplearningexamples_amd.moflow import config as MC
from deeplearningexamples_amd.moflow import generate as MG
from deeplearningexamples_amd.moflow import model as MM
from deeplearningexamples_amd.moflow import mols
from tests import _moflow_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HAVE_RDKIT = importlib.util.find_spec("rdkit") is not None


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(os.path.join(GOLDEN, "moflow_reverse.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].ndim else z[k].item()) for k in z.files}


@functools.lru_cache(maxsize=None)
def model64():
    m = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    MG.load_snapshot(os.path.join(GOLDEN, "moflow_checkpoint.pt"), m)
    return m.double().eval()


def test_reverse_float64_against_the_reference():
    fx, m = fixture(), model64()
    with torch.no_grad():
        h = m.bond_reverse(fx["z"].double())
        adj, x = m.reverse(fx["z"].double())
    assert float((h - fx["h_adj"]).abs().max()) <= 1e-12
    assert torch.equal(adj, fx["adj"].double())
    assert float((x - fx["x"]).abs().max()) <= 1e-12


def test_folded_bond_flow_statement_float64():
    """The generator's bond chain (folded dense maps, BatchNorm folded, [B, P, C] state) in float64 is the reference's h_adj."""
    fx, m = fixture(), model64()
    n, a = m.a_n_node, m.a_size
    h = R.bond_reverse(R.Mode("exact"), MM.folded_bond_flows(m, torch.float64), fx["z"].double()[:, a:].reshape(-1, 4, n, n), 4).v
    assert float((h - fx["h_adj"]).abs().max()) <= 1e-12


def test_row_only_aggregate_first_against_full_rows():
    fx, m = fixture(), model64()
    zx = fx["z"].double()[:, :m.a_size].reshape(-1, m.a_n_node, m.a_n_type)
    flows = MM.folded_atom_flows(m, torch.float64)
    assert [f["row"] for f in flows] == [i % 8 for i in range(10)]                    # the row index wraps
    g = torch.Generator().manual_seed(3)
    for adj in (fx["adj"].double(), (torch.rand(33, 4, 8, 8, generator=g) < 0.3).double(), torch.zeros(33, 4, 8, 8, dtype=torch.float64)):
        full = R.atom_full_rows(m, adj, zx)
        ours = R.atom_reverse(R.Mode("exact"), flows, adj, zx, False).v
        assert float((ours - full).abs().max()) <= 1e-12
    assert float((R.atom_reverse(R.Mode("exact"), flows, fx["adj"], zx, False).v - fx["x"]).abs().max()) <= 1e-12


@pytest.mark.parametrize("grid", [1, 2, 3])
def test_folded_dense_map_is_the_convolution(grid):
    g = torch.Generator().manual_seed(grid)
    w, b = torch.randn(6, 5, 3, 3, generator=g, dtype=torch.float64), torch.randn(6, generator=g, dtype=torch.float64)
    x = torch.randn(7, 5, grid, grid, generator=g, dtype=torch.float64)
    want = torch.nn.functional.conv2d(x, w, b, padding=1)
    p = grid * grid
    dense = MM.fold_conv(w, grid).reshape(p * 6, p * 5)
    got = x.permute(0, 2, 3, 1).reshape(7, -1) @ dense.T + b.repeat(p)
    assert float((got.reshape(7, grid, grid, 6).permute(0, 3, 1, 2) - want).abs().max()) <= 1e-12
    # live blocks: position pairs at most one step apart in both directions (1, 16, 49 of 1, 16, 81)
    assert int((dense != 0).sum()) == {1: 1, 2: 16, 3: 49}[grid] * 30


def test_fold_conv_rejects_more_than_nine_positions():
    with pytest.raises(ValueError, match="at most 3 x 3"):
        MM.fold_conv(torch.zeros(2, 2, 3, 3), 4)


@pytest.mark.parametrize("tag,cfg", [("zinc250k", MC.ZINC250K_CONFIG), ("fixture", MC.FIXTURE_CONFIG)])
def test_state_dict_names_shapes_and_z_dim(tag, cfg):
    want = json.load(open(os.path.join(GOLDEN, "moflow_state_dict.json")))[tag]
    with torch.device("meta"):
        m = MM.MoFlowModel(cfg)
    got = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
    assert list(got) == list(want["state"]) and got == want["state"]
    assert cfg.z_dim == want["z_dim"]
    if tag == "zinc250k":
        assert cfg.z_dim == 40 * 40 * 4 + 40 * 10 and cfg.num_node_features == 10


def test_every_flag_and_default():
    want = json.load(open(os.path.join(GOLDEN, "moflow_cli_flags.json")))
    acts = {a.option_strings[0]: a for a in MG.get_parser()._actions if a.option_strings}
    assert len(want) == 27
    for rec in want:
        a = acts[rec["flags"][0]]
        assert list(a.option_strings) == rec["flags"]
        if rec["action"] == "store_true":
            assert a.const is True and a.default is False
        else:
            assert getattr(a.type, "__name__", None) == rec["type"], rec
        if isinstance(rec["default"], dict):                         # an expression in the reference: LOCAL_RANK of the environment
            assert rec["flags"] == ["--local_rank"]
        else:
            assert a.default == rec["default"], rec
        if isinstance(rec["choices"], dict):
            assert list(a.choices) in (list(MC.CONFIGS), [0, 1, 2, 3])
    assert MG.get_parser().parse_args(["--jit"]).jit is True


def test_config_json_round_trip(tmp_path):
    path = str(tmp_path / "cfg.json")
    MC.FIXTURE_CONFIG.save(path)
    back = MC.Config.load(path)
    assert repr(back) == repr(MC.FIXTURE_CONFIG) and back.z_dim == 8 * 4 + 4 * 64
    assert json.load(open(path))["model_config"]["bond_config"]["n_squeeze"] == 4


def test_snapshot_round_trip_and_newest_rule(tmp_path):
    m = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    assert MG.newest_checkpoint(str(tmp_path)) is None
    for epoch in (1, 8, 10):
        MG.save_snapshot(str(tmp_path), R.seed_model(m, epoch), -0.5 * epoch, epoch)
    want = {k: v.clone() for k, v in m.state_dict().items()}
    newest = MG.newest_checkpoint(str(tmp_path))
    assert os.path.basename(newest) == "model_snapshot_epoch_11"     # by number, not by name ('9' sorts behind '11')
    m2 = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    assert MG.load_snapshot(newest, m2) == (10, -5.0)
    assert all(torch.equal(v, want[k]) for k, v in m2.state_dict().items())
    open(os.path.join(str(tmp_path), "model_snapshot_epoch_12"), "wb").write(b"torn")
    assert os.path.basename(MG.newest_checkpoint(str(tmp_path))) == "model_snapshot_epoch_11"      # an unreadable file is passed over
    assert os.path.basename(MG.newest_checkpoint(str(tmp_path), validate=False)) == "model_snapshot_epoch_12"
    fx = fixture()
    assert MG.load_snapshot(os.path.join(GOLDEN, "moflow_checkpoint.pt"), m2) == (fx["epoch"], fx["ln_var"])


def test_decode_against_postprocess_predictions():
    fx = fixture()
    code = torch.argmax(fx["adj"].long(), dim=1).to(torch.uint8)
    atoms, bonds = mols.decode_predictions(code, fx["x"], MC.FIXTURE_CONFIG)
    assert atoms.shape == (33, 7) and bonds.shape == (33, 7, 7)
    assert np.array_equal(atoms, fx["atoms"].numpy()) and np.array_equal(bonds, fx["bonds"].numpy())
    assert np.array_equal(R.decide(fx["h_adj"], False)[1].numpy(), code.numpy())        # the rule's code is the reference's argmax here


def _cfg(**kw):
    a = dict(n_flow=10, hidden_gnn=[16], hidden_lin=[32, 8])
    b = dict(n_squeeze=4, hidden_ch=[32, 32], conv_lu=2, n_flow=3)
    a.update({k[2:]: v for k, v in kw.items() if k.startswith("a_")})
    b.update({k[2:]: v for k, v in kw.items() if k.startswith("b_")})
    return MC.Config(max_num_nodes=kw.get("n", 8), dataset_config=MC.FIXTURE_CONFIG.dataset_config,
                     model_config=MC.ModelConfig(MC.AtomFlowConfig(**a), MC.BondFlowConfig(**b)))


@pytest.mark.parametrize("kw,text", [
    (dict(b_conv_lu=0), "conv_lu 0 is not built"), (dict(b_conv_lu=1), "conv_lu 1 is not built"),
    (dict(b_n_block=2), "one block and two hidden"), (dict(b_hidden_ch=[32]), "one block and two hidden"),
    (dict(b_n_squeeze=2), "<= 9 positions"), (dict(n=9), "<= 9 positions")])
def test_bond_envelope_rejections(kw, text):
    with pytest.raises(ValueError, match=text) as e:
        MM.check_bond_envelope(_cfg(**kw))
    assert "\n" not in str(e.value)


@pytest.mark.parametrize("kw", [dict(a_hidden_gnn=[16, 16]), dict(a_hidden_lin=[32]), dict(a_n_block=2), dict(a_mask_row_size_list=[2])])
def test_atom_envelope_rejections(kw):
    with pytest.raises(ValueError, match="one block, one graph-convolution layer") as e:
        MM.check_atom_envelope(_cfg(**kw))
    assert "\n" not in str(e.value)


def test_model_and_generator_rejections():
    from deeplearningexamples_amd import _cabi as C
    from deeplearningexamples_amd.moflow.infer import MoFlowGenerator
    with pytest.raises(ValueError, match="conv_lu 1 is not built"):
        MM.MoFlowModel(_cfg(b_conv_lu=1))
    m = MM.MoFlowModel(MC.FIXTURE_CONFIG)
    with pytest.raises(ValueError, match="computes in 16 bits"):
        MoFlowGenerator(m, torch.float32)
    with pytest.raises(ValueError, match="dtype must be"):
        MoFlowGenerator(m, torch.float64)
    with pytest.raises(C.DleError, match="MI355X only"):
        MoFlowGenerator(m, torch.float16, device="cpu")


@pytest.mark.parametrize("argv,text", [
    ([], "computes in 16 bits"),
    (["--amp", "--predictions_path", "", "--results_dir", "/nonexistent/moflow"], "untrained network")])
def test_command_line_exits(argv, text):
    with pytest.raises(SystemExit) as e:
        MG.main(argv)
    assert text in str(e.value) and "\n" not in str(e.value)


def test_training_and_metrics_exit():
    from deeplearningexamples_amd.moflow import evaluate, train
    for mod in (train, evaluate):
        with pytest.raises(SystemExit) as e:
            mod.main([])
        assert "not built" in str(e.value) and "\n" not in str(e.value)


@pytest.mark.skipif(HAVE_RDKIT, reason="rdkit is installed: the SMILES route is taken")
@pytest.mark.parametrize("argv", [["--amp", "--predictions_path", "out.smi"], ["--amp", "--predictions_path", "", "--correct_validity"],
                                  ["--amp"]])
def test_without_rdkit(argv):
    with pytest.raises(SystemExit) as e:
        MG.main(argv)
    assert "rdkit" in str(e.value) and ".npz" in str(e.value) and "\n" not in str(e.value)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_bars_self_test(dtype):
    """The emulated-rounding model stays inside the bar around the exact one; a float32 model with a planted fault leaves it."""
    fx, m = fixture(), model64()
    n, a = m.a_n_node, m.a_size
    z4 = fx["z"].double()[:, a:].reshape(-1, 4, n, n)
    zx = fx["z"].double()[:, :a].reshape(-1, n, m.a_n_type)
    bond = R.representable(MM.folded_bond_flows(m.float()), dtype, ("w1", "w2", "w3"))
    atom = R.representable(MM.folded_atom_flows(m), dtype, ("wg", "w1", "w2", "w3"))
    m.double()
    bar = R.bond_reverse(R.Mode("bar", dtype), bond, z4, 4)
    emu = R.bond_reverse(R.Mode("emul", dtype), bond, z4, 4).v
    assert bool(((emu - bar.v).abs() <= bar.bar()).all()) and float(bar.bar().max()) < 0.1
    for fault in ("swap_st", "drop_loc", "state16"):
        bad = R.bond_reverse(R.Mode("emul", dtype), bond, z4.float().double(), 4, faults=(fault,)).v
        assert bool(((bad - bar.v).abs() > bar.bar()).any()), fault
    adj = fx["adj"].double()
    bar = R.atom_reverse(R.Mode("bar", dtype), atom, adj, zx, False)
    emu = R.atom_reverse(R.Mode("emul", dtype), atom, adj, zx, False).v
    assert bool(((emu - bar.v).abs() <= bar.bar()).all()) and float(bar.bar().max()) < 0.1
    for fault in ("swap_st", "drop_loc"):
        bad = R.atom_reverse(R.Mode("emul", dtype), atom, adj, zx, False, faults=(fault,)).v
        assert bool(((bad - bar.v).abs() > bar.bar()).any()), fault
