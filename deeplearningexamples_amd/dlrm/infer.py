"""DLRM inference on the gfx950 library: (numerical, categorical) -> logits, the forward the reference serves from model.half()
(Recommendation/DLRM/dlrm/scripts/main.py:277-385, 514-542).

The training forward (model.DlrmBottom.forward) gathers from the fp32 tables, writes a 16-bit [B, 1 + T, D] tensor and reads it
back in the interaction.  Here the joint table is held in 16 bits (one rounding per element, the rounding dle_emb_gather_fwd
applies to every row it gathers) and one launch, functional.gather_interact, takes the rows straight into the MFMA operands.
Outside that kernel's envelope, or with fused=False, the gather and dot_interact_fwd run as two launches; both routes, and
DistributedDlrm.forward on the same weights, give the same bits.

One stream, no side stream: cast_rows -> bottom-MLP GEMMs -> gather_interact -> top-MLP GEMMs -> out-layer GEMM.  graphs=True keeps
one captured graph (a linear chain) and one set of static buffers per batch size; a call is then a copy-in and a replay.  The logits
of a call live in a buffer owned by the predictor (one per batch size): copy them before the next call at that batch size.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import CAST_CHUNK_ROWS, cast_table_chunked  # noqa: F401  (shared with the other table front ends)
from .model import DistributedDlrm

# Batch sizes at which the fused launch measured slower than the unfused pair (tools/dlrm_infer_perf.py): routed to the
# pair.  Empty: the fused route did not lose at any measured size.
UNFUSED_BATCH_SIZES = frozenset()


class DlrmPredictor:
    def __init__(self, model: DistributedDlrm, dtype=None, fused=True, graphs=False, release_fp32=False):
        """model: a single-rank DistributedDlrm that owns the bottom MLP and every table.  dtype: the 16-bit type (default: the
        model's compute type; the MLPs' working copies are the model's own, so it must be that type).  fused=False: always the
        gather + dot_interact_fwd pair.  release_fp32: drop the model's fp32 table storage once the 16-bit copy exists (the model
        can no longer train or run its own forward)."""
        if model.distributed:
            raise ValueError("DlrmPredictor: a single-rank model (the bottom -> top exchange belongs to DlrmTrainer)")
        bottom, top = model.bottom_model, model.top_model
        if bottom.mlp is None or bottom.embeddings is None:
            raise ValueError("DlrmPredictor: the model must own the bottom MLP and the embedding tables")
        self.dtype = dtype or model.compute_dtype
        if self.dtype != model.compute_dtype or self.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("DlrmPredictor: dtype must be the model's 16-bit compute type (%s)" % model.compute_dtype)
        self.model, self.fused, self.graphs = model, bool(fused), bool(graphs)
        emb = bottom.embeddings
        self.dev = emb.weight.device
        self.dim, self.tables = emb.embedding_dim, emb.num_tables
        self.offsets, self.hash_sizes = emb.offsets, emb._sizes_dev
        self.table16 = cast_table_chunked(emb.weight.data, self.dtype)
        self._w32 = None if release_fp32 else emb.weight
        if release_fp32:
            emb.weight.data = torch.empty((0, self.dim), dtype=torch.float32, device=self.dev)
        self._bottom = [(w, lin.bias.data, lin.out_features) for w, lin in zip(bottom.mlp.working_copies(), bottom.mlp.linears)]
        self._top = [(w, lin.bias.data, lin.out_features) for w, lin in zip(top.mlp.working_copies(), top.mlp.linears)]
        self._out_w, self._out_b = top.out_working_copy(), top.out.bias.data
        self._k0 = bottom.mlp.k_padded(0)
        self._num_features = bottom.mlp.input_dim
        self._static = {}                     # batch size -> dict(num, cat, out[, graph])

    def refresh(self):
        """Re-cast the table after the model's fp32 weights changed (in place: a captured graph holds the copy by address).  The MLP
        copies are the model's own (DistributedDlrm.refresh_working_copies rewrites them in place)."""
        if self._w32 is None:
            raise RuntimeError("DlrmPredictor.refresh: the fp32 tables were released")
        for r0 in range(0, self.table16.shape[0], CAST_CHUNK_ROWS):
            F.cast_rows(self._w32.data[r0:r0 + CAST_CHUNK_ROWS], self.dtype, out=self.table16[r0:r0 + CAST_CHUNK_ROWS])

    # ------------------------------------------------------------------ the chain
    def _mlp(self, h, layers, last_out=None):
        for i, (w, bias, n) in enumerate(layers):
            dst = last_out if i == len(layers) - 1 else None
            h = F.gemm(h, w, h.shape[0], n, w.shape[1], True, True, out=dst, out_dtype=self.dtype, bias=bias, act=C.ACT_RELU)
        return h

    def _interact_unfused(self, x16, cat):
        """The two-launch route: rows into slots 1.. of X, the bottom MLP into slot 0, then dot_interact_fwd."""
        b, r, d = x16.shape[0], self.tables + 1, self.dim
        x = torch.empty((b, r, d), dtype=self.dtype, device=self.dev)
        rows = F.emb_offset_indices(cat, self.offsets, self.hash_sizes)
        if self._w32 is not None:             # the training forward's gather (fp32 rows, rounded on the way)
            F.emb_gather_fwd(self._w32.data, rows, out_dtype=self.dtype, out=x[:, 1:, :], out_batch_stride=r * d)
        else:                                 # fp32 storage released: the same rows from the 16-bit copy
            g = F.rows_gather(self.table16, rows.view(-1))
            F.cast_rows(g.view(b, self.tables * d), self.dtype, out=x.view(b, r * d)[:, d:])
        self._mlp(x16, self._bottom, last_out=x[:, 0, :])
        return F.dot_interact_fwd(x)

    def _chain(self, num, cat, out):
        b = num.shape[0]
        x16 = F.cast_rows(num, self.dtype, cols_out=self._k0)
        z = None
        if self.fused and b not in UNFUSED_BATCH_SIZES:
            z = F.gather_interact(self.table16, cat, self.offsets, self.hash_sizes, self._mlp(x16, self._bottom))
            # (declined: the bottom MLP runs again below, into its slot of X -- off the envelope only)
        if z is None:
            z = self._interact_unfused(x16, cat)
        h = self._mlp(z, self._top)
        F.gemm(h, self._out_w, b, self._out_w.shape[0], self._out_w.shape[1], True, True, out=out, bias=self._out_b)

    # ------------------------------------------------------------------ the call
    def _buffers(self, b):
        st = self._static.get(b)
        if st is None:
            st = dict(out=torch.empty((b, self._out_w.shape[0]), dtype=self.dtype, device=self.dev))
            if self.graphs:
                st["num"] = torch.zeros((b, self._num_features), dtype=torch.float32, device=self.dev)
                st["cat"] = torch.zeros((b, self.tables), dtype=torch.int64, device=self.dev)
                self._chain(st["num"], st["cat"], st["out"])      # eager once: every kernel is loaded outside the capture
                torch.cuda.synchronize()
                st["graph"] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(st["graph"]):
                    self._chain(st["num"], st["cat"], st["out"])
            self._static[b] = st
        return st

    @torch.no_grad()
    def predict(self, numerical, categorical):
        """numerical fp32 [B, num_numerical], categorical int64 [B, tables] -> logits [B] in the 16-bit type (no sigmoid, as in the
        reference): a view of the predictor's output buffer for this batch size."""
        C.require_cuda(numerical, categorical)
        if numerical.dim() != 2 or categorical.dim() != 2 or numerical.shape[0] != categorical.shape[0]:
            raise ValueError("predict: numerical [B, F] and categorical [B, T]")
        if numerical.shape[1] != self._num_features or categorical.shape[1] != self.tables:
            raise ValueError("predict: %d numerical features and %d tables" % (self._num_features, self.tables))
        if categorical.dtype != torch.int64:
            raise ValueError("predict: categorical must be int64")
        st = self._buffers(numerical.shape[0])
        if self.graphs:
            st["num"].copy_(numerical)
            st["cat"].copy_(categorical)
            st["graph"].replay()
        else:
            self._chain(numerical.float() if numerical.dtype != torch.float32 else numerical, categorical.contiguous(), st["out"])
        return st["out"].view(-1) if st["out"].shape[1] == 1 else st["out"]


def benchmark_latencies(predict, batches, num_batches, warmup_steps=0, synchronize=None, clock=None):
    """The reference's inference_benchmark loop (scripts/main.py:284-320): for each (numerical, categorical, click) of `batches`,
    up to step num_batches inclusive, host time around predict + synchronize; the latencies of steps >= warmup_steps are kept.
    -> (latencies, y_true list, logits list)."""
    import time
    synchronize = synchronize or torch.cuda.synchronize
    clock = clock or time.time
    latencies, y_true, y_score = [], [], []
    for step, (num, cat, click) in enumerate(batches):
        if step > num_batches:
            break
        t0 = clock()
        out = predict(num, cat)
        synchronize()
        dt = clock() - t0
        if step >= warmup_steps:
            latencies.append(dt)
        y_true.append(click)
        y_score.append(out.reshape(-1).clone())
    return latencies, y_true, y_score


def summarize_latencies(latencies, batch_size):
    """scripts/main.py:532-538: drop the first 10 as a warm-up, mean latency and the throughput it implies."""
    kept = list(latencies)[10:]
    if not kept:
        raise ValueError("inference benchmark: no latency left after dropping the first 10 (got %d): raise "
                         "--inference_benchmark_steps or lower --benchmark_warmup_steps" % len(latencies))
    mean = sum(kept) / len(kept)
    return {"mean_inference_latency_batch_%d" % batch_size: mean,
            "mean_inference_throughput_batch_%d" % batch_size: batch_size / mean}
