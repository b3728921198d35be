"""What every inference front end (the Python layer between a checkpoint and the C ABI) does before its first launch: the 16-bit
guard, the device guard, and the per-shape cache of captured graphs.  A front end calls the guards in the order its arguments are
rejected in; require_16bit comes first everywhere and touches no device, so a host-only machine gets its message.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from .graph import GraphedStep

CAST_CHUNK_ROWS = 1 << 20


def require_16bit(dtype, who):
    if dtype == torch.float32:
        raise ValueError("this path computes in 16 bits: pass torch.float16 or torch.bfloat16 (the reference's fp32 / TF32 "
                         "recipes are not built)")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("%s: dtype must be torch.float16 or torch.bfloat16 (got %s)" % (who, dtype))


def gpu_device(device, who):
    """`device`, or the current GPU -> torch.device; anything but a GPU is an error."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise C.DleError("%s runs on the MI355X only (got device %s); there is no CPU path" % (who, dev))
    return dev


class GraphCache(dict):
    """key -> GraphedStep, one captured graph (a single chain) and its static input buffers per key; `graphs` off: plain calls.
    What a captured call returns lives in buffers the graph owns: copy it before the next call with that key."""

    def __init__(self, graphs):
        super().__init__()
        self.graphs = bool(graphs)

    def run(self, key, fn, *tensors):
        if not self.graphs:
            return fn(*tensors)
        g = self.get(key)
        if g is None:
            g = self[key] = GraphedStep(fn, warmup_steps=2)
        return g(*tensors)


def cast_table_chunked(weight, dtype, chunk_rows=CAST_CHUNK_ROWS):
    """16-bit copy of a [rows, dim] fp32 table, cast chunk_rows rows at a time straight into the copy (round to nearest even, once
    per element): nothing table-sized besides the copy itself is ever allocated."""
    if weight.dim() != 2 or chunk_rows < 1:
        raise ValueError("cast_table_chunked: a 2-D table and a positive chunk")
    out = torch.empty(weight.shape, dtype=dtype, device=weight.device)
    for r0 in range(0, weight.shape[0], chunk_rows):
        src, dst = weight[r0:r0 + chunk_rows], out[r0:r0 + chunk_rows]
        if weight.is_cuda:
            F.cast_rows(src, dtype, out=dst)
        else:
            dst.copy_(src)
    return out
