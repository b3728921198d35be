"""NeuMF scores on the gfx950 library: NeuMF.forward of PyTorch/Recommendation/NCF/neumf.py:80-98 as the reference's inference.py
(:90, model.half(), sigmoid=True) and val_epoch (ncf.py:141-144) call it.

fused (the default, inside dle_ncf_score_supported's envelope: --factors 64 --layers 256 256 128 64): ONE launch,
functional.ncf_score_fwd -- four gathers, the GMF product, three ReLU layers, the final dot product, the sigmoid and the loss
partials; nothing of a sample but its score leaves the compute unit.  Rounding contract: tables and W1..W3 in 16 bits, the outputs
of layers 1 and 2 rounded once, everything else fp32.
unfused (fused=False, outside the envelope, or a batch size in UNFUSED_BATCH_SIZES): existing launches on the same 16-bit weights --
rows_gather x 4, gemm + bias + ReLU x 3, a last gemm with an fp32 output -- with torch for the product, the concatenations and the
sigmoid.  It rounds more (the product, the third layer, the final weight) and is the baseline the fused launch is timed against.

Both routes: an index outside its table gives NaN for that sample and adds nothing to the loss.  graphs=True keeps one captured
graph per (call, batch size, index type); what a captured call returns lives in buffers the graph owns.
"""
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import GraphCache, cast_table_chunked, gpu_device, require_16bit
from .model import NeuMFModel

# Batch sizes at which the fused launch did not measure faster than the unfused chain by more than the run's spread
# (tools/ncf_infer_perf.py, profiles/ncf_infer_perf.json): routed to the chain.  Filled from measurements only.
# Empty: the fused launch won at every size of the reference's list in fp16 and bf16 (us, fused against unfused, eager: 21 / 175 at
# 1, 32 / 165 at 65,536 -- the closest --, 306 / 1671 at 1,048,576).
UNFUSED_BATCH_SIZES = frozenset()


class NeuMFScorer:
    def __init__(self, model, dtype=torch.float16, graphs=False, fused=True, device=None, max_workgroups=0):
        require_16bit(dtype, "NeuMFScorer")
        if not isinstance(model, NeuMFModel):
            raise TypeError("model must be a NeuMFModel")
        self.dev = dev = gpu_device(device, "NeuMFScorer")
        self.dtype, self.max_workgroups = dtype, int(max_workgroups)
        self.factors, self.layers = model.mf_dim, model.mlp_layer_sizes
        self.in_envelope = F.ncf_score_supported(self.factors, self.layers)
        self.fused = bool(fused) and self.in_envelope
        self.n_users, self.n_items = model.nb_users, model.nb_items
        sd = {k: v.detach() for k, v in model.state_dict().items()}
        with torch.no_grad():
            self.tables = tuple(cast_table_chunked(sd[n + ".weight"].to(dev, torch.float32).contiguous(), dtype)
                                for n in ("mf_user_embed", "mf_item_embed", "mlp_user_embed", "mlp_item_embed"))
            n_mlp = len(self.layers) - 1
            self.weights = tuple(sd["mlp.%d.weight" % i].to(dev, torch.float32).to(dtype).contiguous() for i in range(n_mlp))
            self.biases = tuple(sd["mlp.%d.bias" % i].to(dev, torch.float32).contiguous() for i in range(n_mlp))
            self.wf = sd["final.weight"].to(dev, torch.float32).reshape(-1).contiguous()
            self.bf = sd["final.bias"].to(dev, torch.float32).reshape(1).contiguous()
            self.wf16 = self.wf.to(dtype).view(1, -1).contiguous()                   # the unfused route's last GEMM operand
        self._graphs = GraphCache(graphs)

    # ------------------------------------------------------------------ the two routes
    def _route_fused(self, b):
        return self.fused and b not in UNFUSED_BATCH_SIZES

    def _unfused_logits(self, user, item):
        u, i = user.long(), item.long()
        bad = (u < 0) | (u >= self.n_users) | (i < 0) | (i >= self.n_items)
        u, i = u.clamp(0, self.n_users - 1), i.clamp(0, self.n_items - 1)
        mfu, mfi, mlu, mli = self.tables
        xmf = F.rows_gather(mfu, u) * F.rows_gather(mfi, i)
        h = torch.cat((F.rows_gather(mlu, u), F.rows_gather(mli, i)), dim=1)
        b = h.shape[0]
        for w, bias in zip(self.weights, self.biases):
            h = F.gemm(h, w, b, w.shape[0], w.shape[1], True, True, out_dtype=self.dtype, bias=bias, act=C.ACT_RELU)
        x = torch.cat((xmf, h), dim=1)
        logit = F.gemm(x, self.wf16, b, 1, x.shape[1], True, True, out_dtype=torch.float32, bias=self.bf).view(-1)
        return torch.where(bad, torch.full_like(logit, float("nan")), logit), bad

    def _score(self, user, item, label, want_prob, prob_out=None):
        """-> (logit, prob or None, loss sum as a float64 scalar on the device or None)"""
        if self._route_fused(user.numel()):
            logit, prob, partials = F.ncf_score_fwd(*self.tables, self.weights, self.biases, self.wf, self.bf, user, item, label=label,
                                                    want_prob=want_prob, max_workgroups=self.max_workgroups, prob_out=prob_out)
            return logit, prob, (partials.sum(dtype=torch.float64) if partials is not None else None)
        logit, bad = self._unfused_logits(user, item)
        prob = (torch.sigmoid(logit) if prob_out is None else torch.sigmoid(logit, out=prob_out)) if want_prob else None
        loss = None
        if label is not None:
            lp = torch.clamp(torch.nn.functional.logsigmoid(logit), min=-100.0)
            lq = torch.clamp(torch.nn.functional.logsigmoid(-logit), min=-100.0)
            per = -(label * lp + (1.0 - label) * lq)
            loss = torch.where(bad, torch.zeros_like(per), per).sum(dtype=torch.float64)
        return logit, prob, loss

    # ------------------------------------------------------------------ the calls
    def _check(self, user, item, label=None):
        C.require_cuda(user, item, label)
        if user.dim() != 1 or user.shape != item.shape or user.dtype != item.dtype or user.dtype not in (torch.int32, torch.int64):
            raise ValueError("NeuMFScorer: user and item are int32 or int64 vectors of one length")
        if label is not None and (label.dim() != 1 or label.numel() != user.numel()):
            raise ValueError("NeuMFScorer: one label per sample")
        return user.contiguous(), item.contiguous(), (label.float().contiguous() if label is not None else None)

    @torch.no_grad()
    def logits(self, user, item):
        """fp32 [B], no sigmoid (NeuMF.forward(sigmoid=False))."""
        user, item, _ = self._check(user, item)
        return self._graphs.run(("logits", user.numel(), user.dtype), lambda u, i: self._score(u, i, None, False)[0], user, item)

    @torch.no_grad()
    def predict(self, user, item):
        """fp32 [B] probabilities (NeuMF.forward(sigmoid=True))."""
        user, item, _ = self._check(user, item)
        return self._graphs.run(("predict", user.numel(), user.dtype), lambda u, i: self._score(u, i, None, True)[1], user, item)

    @torch.no_grad()
    def score_with_loss(self, user, item, label, prob_out=None):
        """-> (probabilities fp32 [B], the batch's binary cross-entropy SUM as a float64 scalar on the device).  prob_out: an fp32
        [B] tensor to receive the probabilities."""
        user, item, label = self._check(user, item, label)
        if not self._graphs.graphs:                   # straight into the caller's tensor
            return self._score(user, item, label, True, prob_out)[1:]
        prob, loss = self._graphs.run(("loss", user.numel(), user.dtype), lambda u, i, y: self._score(u, i, y, True)[1:], user, item, label)
        if prob_out is not None:
            prob_out.copy_(prob)
            prob = prob_out
        return prob, loss
