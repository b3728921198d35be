"""Writes the MoFlow fixtures under tests/golden/ from a checkout of the reference recipe (CPU only).  Recorded data only: results of
the reference's programs, never their text.

    python tools/make_moflow_fixture.py --reference /path/to/DeepLearningExamples/PyTorch/DrugDiscovery/MoFlow

  moflow_state_dict.json   parameter / buffer names, shapes and dtypes of the reference's MoFlow at ZINC250k and at the fixture config
  moflow_cli_flags.json    flags, defaults and kinds of moflow/runtime/arguments.py, read from its syntax tree
  moflow_reverse.npz       z (B = 33, temperature 0.6), the float64 reference's bond-model output h_adj, MoFlow.reverse's adj and x,
                           and postprocess_predictions' atoms and bonds
  moflow_checkpoint.pt     the fixture model in the reference's snapshot form (keys model / optimizer / ln_var / epoch)

The fixture config is moflow.config.FIXTURE_CONFIG (N 8, 7 atoms, T 4; bond n_squeeze 4, hidden [32, 32], 3 flows; atom 10 flows, gnn
[16], lin [32, 8]); the weights are tests/_moflow_ref.seed_model's.  rdkit is stubbed in sys.modules: the model path touches
Chem.rdchem.BondType.SINGLE / DOUBLE / TRIPLE only.  The tool asserts, with the generator's roundings emulated in float64, that at
most 10 % of the bond positions are unclear (gap of the two largest symmetrised values <= 2 * 1.5 E_emulated) in both 16-bit types.
"""
import argparse
import ast
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED, B, TEMPERATURE, LN_VAR, EPOCH = 2025, 33, 0.6, -0.25, 7


def reference_modules(ref):
    chem = types.ModuleType("rdkit.Chem")
    chem.rdchem = types.SimpleNamespace(BondType=types.SimpleNamespace(SINGLE="SINGLE", DOUBLE="DOUBLE", TRIPLE="TRIPLE"))
    chem.Mol = object
    rdkit = types.ModuleType("rdkit")
    rdkit.Chem = chem
    sys.modules["rdkit"], sys.modules["rdkit.Chem"] = rdkit, chem
    sys.path.insert(0, ref)
    import moflow.config as rc
    import moflow.model.model as rm
    import moflow.utils as ru
    return rc, rm, ru


def parser_flags(path):
    """(flags, default, action, type, choices) of every add_argument call, from the syntax tree.  A default or a choice list that is
    not a literal (an environment read, a table of the module) is recorded as the marker {"nonliteral": true}: none of the
    reference's text goes into the fixture."""
    out = []
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: k.value for k in node.keywords}

            def lit(k):
                if k not in kw:
                    return None
                try:
                    return ast.literal_eval(kw[k])
                except ValueError:
                    return {"nonliteral": True}
            action = lit("action")
            out.append({"flags": [ast.literal_eval(a) for a in node.args], "default": False if action == "store_true" and "default" not in kw
                        else lit("default"), "action": action, "type": getattr(kw.get("type"), "id", None), "choices": lit("choices")})
    return out


def reference_config(rc, ours):
    d, a, b = ours.dataset_config, ours.model_config.atom_config, ours.model_config.bond_config
    return rc.Config(
        max_num_nodes=ours.max_num_nodes,
        dataset_config=rc.DatasetConfig(dataset_name=d.dataset_name, atomic_num_list=list(d.atomic_num_list), max_num_atoms=d.max_num_atoms,
                                        labels=list(d.labels), smiles_col=d.smiles_col),
        model_config=rc.ModelConfig(rc.AtomFlowConfig(n_flow=a.n_flow, hidden_gnn=list(a.hidden_gnn), hidden_lin=list(a.hidden_lin)),
                                    rc.BondFlowConfig(n_squeeze=b.n_squeeze, hidden_ch=list(b.hidden_ch), conv_lu=b.conv_lu, n_flow=b.n_flow),
                                    noise_scale=ours.model_config.noise_scale, learn_dist=ours.model_config.learn_dist))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    args = ap.parse_args()
    rc, rm, ru = reference_modules(args.reference)
    import torch
    from deeplearningexamples_amd.moflow import config as OC
    from deeplearningexamples_amd.moflow import model as OM
    from tests import _moflow_ref as R
    os.makedirs(GOLDEN, exist_ok=True)

    # 1. names, shapes, dtypes
    shapes = {}
    for tag, cfg in (("zinc250k", rc.ZINC250K_CONFIG), ("fixture", reference_config(rc, OC.FIXTURE_CONFIG))):
        with torch.device("meta"):
            m = rm.MoFlow(cfg)
        shapes[tag] = {"z_dim": cfg.z_dim, "state": {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}}
    json.dump(shapes, open(os.path.join(GOLDEN, "moflow_state_dict.json"), "w"), indent=0)

    # 2. the command line
    json.dump(parser_flags(os.path.join(args.reference, "moflow", "runtime", "arguments.py")),
              open(os.path.join(GOLDEN, "moflow_cli_flags.json"), "w"), indent=1)

    # 3. the fixture model and its float64 reverse
    cfg = reference_config(rc, OC.FIXTURE_CONFIG)
    torch.manual_seed(SEED)
    ref = R.seed_model(rm.MoFlow(cfg), SEED + 1).eval()
    sd = {k: v.clone() for k, v in ref.state_dict().items()}
    z = torch.randn(B, cfg.z_dim, generator=torch.Generator().manual_seed(SEED + 2)) * TEMPERATURE
    ref = ref.double()
    n = cfg.max_num_nodes
    with torch.no_grad():
        h_adj = ref.bond_model.reverse(z.double()[:, ref.a_size:].reshape(B, 4, n, n))
        adj, x = ref.reverse(z.double())
    atoms, bonds = ru.postprocess_predictions(x, adj, config=cfg)

    # its own assertions: our restatement loads the state and agrees; the emulated roundings leave at most 10 % unclear positions
    ours = OM.MoFlowModel(OC.FIXTURE_CONFIG)
    ours.load_state_dict(sd)
    ours.eval()
    with torch.no_grad():
        o_adj, o_x = ours.double().reverse(z.double())
    assert torch.equal(o_adj, adj.contiguous()) and float((o_x - x).abs().max()) <= 1e-12
    ours = ours.float()
    unshift = cfg.model_config.noise_scale == 0
    for dtype in (torch.float16, torch.bfloat16):
        emu = R.bond_reverse(R.Mode("emul", dtype), OM.folded_bond_flows(ours), z.double()[:, ref.a_size:].reshape(B, 4, n, n),
                             cfg.model_config.bond_config.n_squeeze).v
        e_emul = float((emu - h_adj).abs().max())
        clear = R.clear_positions(h_adj, unshift, 2 * 1.5 * e_emul)
        mask_e, mask_r = R.decide(emu, unshift)[0], R.decide(h_adj, unshift)[0]
        print("%s: E_emulated(h_adj) %.3e, unclear %.2f %%, emulated bits differ at %d clear positions" %
              (dtype, e_emul, 100 * (1 - float(clear.double().mean())), int(((mask_e != mask_r) & clear).sum())))
        assert float(clear.double().mean()) >= 0.9 and not bool(((mask_e != mask_r) & clear).any())
    np.savez_compressed(os.path.join(GOLDEN, "moflow_reverse.npz"), z=z.numpy(), h_adj=h_adj.numpy(), adj=adj.numpy().astype(np.uint8),
                        x=x.numpy(), atoms=atoms.astype(np.int64), bonds=bonds.astype(np.int64), ln_var=np.float64(LN_VAR),
                        epoch=np.int64(EPOCH), temperature=np.float64(TEMPERATURE))

    # 4. the checkpoint, as save_state writes it
    torch.save({"model": sd, "optimizer": {}, "ln_var": LN_VAR, "epoch": EPOCH}, os.path.join(GOLDEN, "moflow_checkpoint.pt"))
    for f in ("moflow_state_dict.json", "moflow_cli_flags.json", "moflow_reverse.npz", "moflow_checkpoint.pt"):
        print(f, os.path.getsize(os.path.join(GOLDEN, f)), "bytes")


if __name__ == "__main__":
    main()
