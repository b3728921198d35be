"""Command line of MoFlow's molecule generation (the reference's moflow/runtime/generate.py with the flags of arguments.py):

    python -m deeplearningexamples_amd.moflow.generate --amp [--amp-dtype bf16] --results_dir DIR [--batch_size 512] [--steps K]
        [--temperature 0.3] [--predictions_path out.smi | out.npz | ''] [--correct_validity] [--allow_untrained] [--log_path log.json]

Every flag and default of arguments.py is parsed; --amp-dtype, --graphs and --config_path (a Config JSON instead of a named config)
are additions.  The newest model_snapshot_epoch_N of --results_dir is loaded (keys model / ln_var / epoch).  Per step one batch is
sampled, reversed and decoded; throughput_generate, latency_generate_mean / 90 / 95 / 99 and total_time_generate are logged as the
reference's PerformanceLogger computes them (time stamps from step --warmup_steps on, every --log_interval steps and at the end).
With rdkit importable the molecules are written as SMILES, optionally after --correct_validity; without it a .npz path receives the
atomic numbers and bond codes, and a .smi path or --correct_validity exits with one line.  fp32 (no --amp), training, evaluate.py's
metrics and conv_lu 0 / 1 are one-line exits; --jit is accepted and does nothing.
"""
import argparse
import glob
import os
import sys
import time

import numpy as np
import torch

from ..utils import dllogger
from .config import CONFIGS, Config

CHECKPOINT_PATTERN = "model_snapshot_epoch_%s"


def get_parser():
    p = argparse.ArgumentParser(description="MoFlow molecule generation")
    p.add_argument("--data_dir", type=str, default="/data", help="Location for the dataset.")
    p.add_argument("--config_name", type=str, default="zinc250k", choices=list(CONFIGS), help="The config to choose.")
    p.add_argument("--results_dir", type=str, default="/results", help="Directory where checkpoints are stored.")
    p.add_argument("--predictions_path", type=str, default="/results/predictions.smi",
                   help="Path to store generated molecules (.smi needs rdkit; .npz: atomic numbers and bond codes); '' saves nothing.")
    p.add_argument("--log_path", type=str, default=None, help="Path for the JSON log; new records are appended.")
    p.add_argument("--log_interval", type=int, default=20, help="Frequency for writing logs, expressed in steps.")
    p.add_argument("--warmup_steps", type=int, default=20, help="Number of warmup steps (left out of the statistics).")
    p.add_argument("--steps", type=int, default=-1, help="Number of batches to generate (-1: one).")
    p.add_argument("--save_epochs", type=int, default=5, help="(training)")
    p.add_argument("--eval_epochs", type=int, default=5, help="(training)")
    p.add_argument("--learning_rate", type=float, default=0.0005, help="(training)")
    p.add_argument("--beta1", type=float, default=0.9, help="(training)")
    p.add_argument("--beta2", type=float, default=0.99, help="(training)")
    p.add_argument("--clip", type=float, default=1, help="(training)")
    p.add_argument("--epochs", type=int, default=300, help="(training)")
    p.add_argument("--batch_size", type=int, default=512, help="Batch size per GPU.")
    p.add_argument("--num_workers", type=int, default=4, help="(training)")
    p.add_argument("--seed", type=int, default=1, help="Random seed.")
    p.add_argument("--local_rank", default=os.environ.get("LOCAL_RANK", 0), type=int, help="rank of the GPU")
    p.add_argument("--temperature", type=float, default=0.3, help="Temperature used for sampling.")
    p.add_argument("--val_batch_size", type=int, default=100, help="(training)")
    p.add_argument("--allow_untrained", action="store_true", help="Allow sampling molecules from an untrained network.")
    p.add_argument("--correct_validity", action="store_true", help="Apply validity correction after the generation (needs rdkit).")
    p.add_argument("--amp", action="store_true", help="16-bit operands (the only precision built).")
    p.add_argument("--cuda_graph", action="store_true", help="(training)")
    p.add_argument("--jit", action="store_true", help="accepted, does nothing")
    p.add_argument("--verbosity", type=int, default=1, choices=[0, 1, 2, 3], help="Verbosity level.")
    p.add_argument("--amp-dtype", default=None, choices=["fp16", "bf16"], help="16-bit storage type (--amp = fp16)")
    p.add_argument("--graphs", action="store_true", help="replay one captured graph per batch size")
    p.add_argument("--config_path", type=str, default=None, help="a Config JSON (Config.save) instead of --config_name")
    return p


def _epoch_of(path):
    return int(path.split("_")[-1])


def newest_checkpoint(model_dir, validate=True):
    """common.py:67-93: the snapshot with the largest epoch number in its name that torch.load can read, or None."""
    paths = sorted((q for q in glob.glob(os.path.join(model_dir, CHECKPOINT_PATTERN % "*")) if q.split("_")[-1].isdigit()), key=_epoch_of)
    for path in reversed(paths):
        if not validate:
            return path
        try:
            torch.load(path, map_location="cpu", weights_only=False)
            return path
        except Exception:
            continue
    return None


def save_snapshot(model_dir, model, ln_var, epoch):
    """save_state's file (common.py:32-43), without an optimizer: model_snapshot_epoch_{epoch + 1}."""
    path = os.path.join(model_dir, CHECKPOINT_PATTERN % (epoch + 1))
    torch.save({"model": model.state_dict(), "optimizer": {}, "ln_var": ln_var, "epoch": epoch}, path)
    return path


def load_snapshot(path, model):
    """load_state (common.py:55-64) -> (epoch, ln_var)."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    model.load_state_dict(state["model"])
    ln_var = state["ln_var"]
    return state["epoch"], float(ln_var.reshape(-1)[0]) if isinstance(ln_var, torch.Tensor) else float(ln_var)


class PerformanceLogger:
    """logger.py:67-101, mode 'generate'."""

    def __init__(self, batch_size, warmup_steps):
        self.batch_size, self.warmup_steps, self.step, self.stamps = batch_size, warmup_steps, 0, []

    def update(self):
        self.step += 1
        if self.step >= self.warmup_steps:
            self.stamps.append(time.time())

    def summarize(self, step):
        if len(self.stamps) < 2:
            return {}
        t = np.asarray(self.stamps)
        d = np.diff(t)
        stats = {"throughput_generate": float((self.batch_size / d).mean()), "latency_generate_mean": float(d.mean()),
                 "total_time_generate": float(t[-1] - t[0])}
        for q in (90, 95, 99):
            stats["latency_generate_%d" % q] = float(np.percentile(d, q))
        dllogger.log(step=step, data=stats)
        dllogger.flush()
        return stats


def main(argv=None):
    args = get_parser().parse_args(argv)
    if not args.amp and args.amp_dtype is None:
        raise SystemExit("this path computes in 16 bits: pass --amp (or --amp-dtype bf16); the reference's fp32 / TF32 recipe is not built")
    dtype = torch.bfloat16 if args.amp_dtype == "bf16" else torch.float16
    path = args.predictions_path
    chem = None
    if args.correct_validity or (path and not path.endswith(".npz")):
        from .mols import require_rdkit
        chem = require_rdkit("--correct_validity" if args.correct_validity else "writing SMILES to %s" % path)
    config = Config.load(args.config_path) if args.config_path else CONFIGS[args.config_name]
    from .model import MoFlowModel, check_atom_envelope, check_bond_envelope
    try:
        check_bond_envelope(config)
        check_atom_envelope(config)
    except ValueError as err:
        raise SystemExit(str(err))
    backends = [dllogger.StdOutBackend(dllogger.Verbosity.VERBOSE)]
    if args.log_path is not None:
        backends.append(dllogger.JSONStreamBackend(dllogger.Verbosity.VERBOSE, args.log_path, append=True))
    dllogger.init(backends=backends)
    dllogger.log(data=vars(args), step="PARAMETER")
    snapshot = newest_checkpoint(args.results_dir)
    if snapshot is None and not args.allow_untrained:
        raise SystemExit("Generating molecules from an untrained network! If this was intentional, pass --allow_untrained flag.")
    model = MoFlowModel(config)
    epoch, ln_var = load_snapshot(snapshot, model) if snapshot is not None else (0, 0.0)
    from .infer import MoFlowGenerator
    gen = MoFlowGenerator(model.eval(), dtype, graphs=args.graphs)
    rng = torch.Generator(device=gen.device).manual_seed(args.seed)
    steps = 1 if args.steps == -1 else args.steps
    perf = PerformanceLogger(args.batch_size, args.warmup_steps)
    atoms_all, bonds_all = [], []
    writer = chem.SmilesWriter(path) if path and chem is not None else None
    for i in range(steps):
        perf.update()
        _, _, x, code = gen.sample(args.batch_size, args.temperature, ln_var, generator=rng)
        atoms, bonds = gen.decode(code, x)
        if (i + 1) % args.log_interval == 0:
            perf.summarize(step=(0, i, i))
        if path and chem is None:
            atoms_all.append(atoms)
            bonds_all.append(bonds)
        elif path:
            from .mols import predictions_to_mols
            for mol in predictions_to_mols(chem, atoms, bonds, args.correct_validity):
                writer.write(mol)
    stats = perf.summarize(step=tuple())
    if path and chem is None:
        np.savez_compressed(path, atoms=np.concatenate(atoms_all), bonds=np.concatenate(bonds_all), epoch=epoch)
    elif path:
        writer.close()
    return stats


if __name__ == "__main__":
    main(sys.argv[1:])
