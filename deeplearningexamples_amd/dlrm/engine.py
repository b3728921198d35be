"""DLRM train step on MI355X: forward, loss, backward, sparse + dense SGD, loss-scale update.

Mirrors the reference's step (Recommendation/DLRM/dlrm/scripts/main.py):
    forward_backward  :585-594   autocast forward, BCEWithLogits on this rank's label slice, scaled backward
    weight_update     :596-608   scaler.step(mlp_optimizer); scaler.unscale_(embedding_optimizer);
                                 embedding_optimizer.step(); scaler.update()
    LR compensation   :444-452   model-parallel parts (embeddings, bottom MLP) use lr / world_size under SGD; under Adam
                                 (--Adam_embedding_optimizer / --Adam_MLP_optimizer) they keep lr and their gradients are
                                 divided by world_size instead (scale_embeddings_gradients / scale_MLP_gradients, :720-730;
                                 the top MLP is not divided)
    optimizers        :468-482   FusedSGD / apex FusedAdam over both MLPs, SGD / torch.optim.SparseAdam over the joint table
    CudaGraphWrapper  :194-274   whole-step capture  (here: HIP graph through torch.cuda.CUDAGraph)
and the hybrid-parallel exchange (dlrm/model/distributed.py:25-98): one all-to-all forward, one backward,
plus the data-parallel all-reduce (mean) of the top-MLP gradients, both through torch.distributed
(backend "nccl" == RCCL over xGMI) on side streams overlapped with the remaining backward work.

One deliberate difference: on a gradient overflow the reference still applies the embedding update
(embedding_optimizer.step() is called directly, main.py:606); here the sparse update is skipped together
with the dense one (found_inf gates both), the scale is backed off exactly as GradScaler does.  With sparse Adam this means:
on an overflow step the embedding rows, their exp_avg / exp_avg_sq and the embedding step counter all stay unchanged, where
the reference would write inf / nan into the moments of the touched rows for good.  Optimizer state lives in the trainer (the
MLPs' moments) and the JointEmbedding (the tables' moments); checkpoints do not hold it, as in the reference, so a resumed run
starts Adam from zero moments at step 1.
"""
from typing import Optional, Sequence

import os

import torch
import torch.distributed as dist

from .. import functional as F
from .. import multi_tensor as mt
from ..utils import comm
from ..utils.amp import GradScalerState
from ..utils.comm import allreduce_mean_
from .model import DistributedDlrm
from .placement import ExchangePlan


def optimizer_plan(lr, world, adam_embeddings=False, adam_mlps=False):
    """The reference's learning-rate compensation (main.py:444-452) and Adam gradient scaling (scale_embeddings_gradients /
    scale_MLP_gradients, main.py:720-730): part -> (learning rate, divisor of its gradient).  SGD: the model-parallel parts
    (embeddings, bottom MLP) step with lr / world; Adam: they keep lr and their gradients are divided by world; the
    data-parallel top MLP always steps with lr on the (all-reduce mean) gradient."""
    return {"embeddings": (lr, world) if adam_embeddings else (lr / world, 1),
            "bottom_mlp": (lr, world) if adam_mlps else (lr / world, 1),
            "top_mlp": (lr, 1)}


class _FlatGrads:
    """fp32 gradients of a list of Linear layers as views of ONE flat buffer (a single all-reduce bucket)."""

    def __init__(self, linears, device, storage=None):
        n = sum(l.weight.numel() + l.bias.numel() for l in linears)
        self.flat = torch.zeros(n, dtype=torch.float32, device=device) if storage is None else storage
        assert self.flat.numel() == n
        self.views = []
        o = 0
        for l in linears:
            gw = self.flat[o:o + l.weight.numel()].view_as(l.weight)
            o += l.weight.numel()
            gb = self.flat[o:o + l.bias.numel()]
            o += l.bias.numel()
            self.views.append((gw, gb))

    def tensors(self):
        return [t for pair in self.views for t in pair]


class DlrmTrainer:
    def __init__(self, model: DistributedDlrm, lr: float, batch_sizes_per_gpu: Sequence[int],
                 vectors_per_gpu: Optional[Sequence[int]] = None, rank: int = 0, world_size: int = 1,
                 amp: bool = True, init_scale: float = 65536.0, freeze_mlps=False, freeze_embeddings=False,
                 process_group=None, adam_embeddings=False, adam_mlps=False, adam_betas=(0.9, 0.999), adam_eps=1e-8):
        """adam_embeddings: torch.optim.SparseAdam on the joint table in place of SGD; adam_mlps: apex FusedAdam on both MLPs in
        place of FusedSGD (betas / eps: both optimizers' defaults)."""
        self.model = model
        self.rank, self.world = rank, world_size
        self.device = model.top_model.out.weight.device
        self.pg = process_group
        self.freeze_mlps, self.freeze_embeddings = freeze_mlps, freeze_embeddings
        self.adam_embeddings, self.adam_mlps = bool(adam_embeddings), bool(adam_mlps)
        self.adam_betas, self.adam_eps = tuple(adam_betas), float(adam_eps)
        d = model._embedding_dim
        if vectors_per_gpu is None:
            vectors_per_gpu = [model.bottom_model.num_feature_vectors]
        self.plan = ExchangePlan(batch_sizes_per_gpu, vectors_per_gpu, d, rank)
        self.scaler = GradScalerState(self.device, enabled=amp and model.compute_dtype == torch.float16,
                                      init_scale=init_scale)
        self.base_lr = lr
        self.lr_factor = 1.0
        # device-resident learning rates (no host sync / graph friendly)
        self.lr_dp = torch.full((1,), lr, dtype=torch.float32, device=self.device)               # top model
        self.lr_mp = torch.full((1,), lr / world_size, dtype=torch.float32, device=self.device)  # bottom parts
        # per part (embeddings, bottom MLP, top MLP): the learning rate and the gradient divisor of the reference's rules
        self.opt_plan = optimizer_plan(lr, world_size, self.adam_embeddings, self.adam_mlps)
        self.lr_emb = self._lr_tensor(self.opt_plan["embeddings"][0])
        top = model.top_model
        self.top_linears = top.mlp.linears + [top.out]
        bm = model.bottom_model.mlp
        self.bot_linears = bm.linears if bm is not None else []
        # ONE buffer behind the dense gradients of both MLPs (top first: the data-parallel all-reduce bucket stays a contiguous
        # view): the GradScaler's inf / nan sweep over them is one launch
        count = lambda ls: sum(l.weight.numel() + l.bias.numel() for l in ls)
        n_top, n_bot = count(self.top_linears), count(self.bot_linears)
        pad = (n_top + 63) // 64 * 64                 # (the second view starts on a 256-byte boundary; the gap stays zero)
        self.dense_grads = torch.zeros(pad + n_bot, dtype=torch.float32, device=self.device)
        self.top_grads = _FlatGrads(self.top_linears, self.device, self.dense_grads[:n_top])
        self.bot_grads = _FlatGrads(self.bot_linears, self.device, self.dense_grads[pad:]) if bm is not None else None
        if world_size > 1:
            # the top MLP is the data-parallel part: every replica starts from rank 0's weights (the reference wraps it
            # in torch DDP, dlrm/scripts/main.py:463-466); embeddings / bottom MLP are model parallel and stay local
            comm.broadcast_parameters_(list(model.top_model.parameters()), 0, process_group)
        model.refresh_working_copies()
        self._tables = {}
        self._build_tables()
        if self.adam_embeddings or self.adam_mlps:
            self._build_adam()
        self.noop = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.comm_stream = torch.cuda.Stream(device=self.device) if world_size > 1 else None
        self.moving_loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        import os
        # last layer + loss + their backward as one kernel (DLE_DLRM_FUSE_HEAD=0: the separate GEMM / loss launches)
        self.fuse_head = (os.environ.get("DLE_DLRM_FUSE_HEAD", "1") != "0" and self.device.type == "cuda"
                          and model.top_model.head_fusable())

    # ------------------------------------------------------------------ optimizer plumbing
    def _build_tables(self):
        top = self.model.top_model
        w16 = top.mlp.working_copies() + [top.out_working_copy()]
        # weights whose 16-bit copy has the same shape get the copy refreshed inside the SGD kernel
        def split(linears, grads, copies):
            same = [i for i, l in enumerate(linears) if copies[i].shape == l.weight.shape]
            g, p, c = [], [], []
            for i in same:
                g.append(grads.views[i][0]); p.append(linears[i].weight.data); c.append(copies[i])
            gb = [grads.views[i][1] for i in range(len(linears))]
            pb = [l.bias.data for l in linears]
            padded = [i for i in range(len(linears)) if i not in same]
            gp = [grads.views[i][0] for i in padded]
            pp = [linears[i].weight.data for i in padded]
            return (mt.TensorTable([g, p, c], mt.streaming_chunk([g])) if g else None,
                    mt.TensorTable([gb + gp, pb + pp], mt.streaming_chunk([gb + gp])), padded)
        self.t_top_w, self.t_top_b, self.top_padded = split(self.top_linears, self.top_grads, w16)
        if self.bot_grads is not None:
            bw16 = self.model.bottom_model.mlp.working_copies()
            self.t_bot_w, self.t_bot_b, self.bot_padded = split(self.bot_linears, self.bot_grads, bw16)
        self.t_top_all = mt.TensorTable([[self.top_grads.flat]])
        # One learning rate for both MLPs (one rank, or the row-sharded placement's data-parallel bottom MLP): ONE update launch
        # over every dense tensor -- weights with a same-shape 16-bit copy refresh it in the kernel, biases and the K-padded first
        # layers carry no copy (their padded copies follow by cast_rows).  Nine launches at the tail of the step become four.
        self.t_dense = None
        if self.bot_grads is not None and (self.world == 1 or getattr(self, "bottom_dp", False)) and \
                os.environ.get("DLE_DLRM_ONE_DENSE_STEP", "1") != "0":
            bw = self.model.bottom_model.mlp.working_copies()
            g, pp, c = [], [], []
            for lins, grads, copies in ((self.top_linears, self.top_grads, w16), (self.bot_linears, self.bot_grads, bw)):
                for i, l in enumerate(lins):
                    g += [grads.views[i][0], grads.views[i][1]]
                    pp += [l.weight.data, l.bias.data]
                    c += [copies[i] if copies[i].shape == l.weight.shape else None, None]
            self.t_dense = mt.TensorTable([g, pp, c], mt.streaming_chunk([g]))

    def _lr_tensor(self, rate):
        """The device tensor that carries `rate` (one of optimizer_plan's rates: lr or lr / world) through set_lr_factor."""
        if rate == self.base_lr:
            return self.lr_dp
        if rate == self.base_lr / self.world:
            return self.lr_mp
        raise ValueError("no device learning rate for %r (lr %r, world %d)" % (rate, self.base_lr, self.world))

    def _build_adam(self):
        """Device-resident Adam state: one int32 step counter per optimizer (advanced on the device only when its step is taken),
        the embedding gradient multiplier, the MLPs' fp32 moments and ONE FusedAdam table over both MLPs (one learning rate under
        Adam; the bottom MLP's 1 / world rides on a per-tensor gradient multiplier).  State is allocated only for the parts that
        step (not under freeze_embeddings / freeze_mlps); the sparse update's scratch is sized here for the batch the bottom model
        sees, so the step itself allocates nothing."""
        dev = self.device
        plan = self.opt_plan
        self.emb_step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.mlp_step = torch.zeros(1, dtype=torch.int32, device=dev)
        emb = self.model.bottom_model.embeddings
        if self.adam_embeddings and not self.freeze_embeddings and emb is not None:
            emb.adam_state()
            ws = emb.workspace()
            ws.adam_scratch_for(self.plan.global_batch, dev)
            ws.next_for(self.plan.global_batch * emb.num_tables, dev)
            # g = sum * inv_scale / world (scale_embeddings_gradients, then GradScaler.unscale_)
            self.emb_div = plan["embeddings"][1]
            self.emb_gmul = torch.full((1,), 1.0 / self.emb_div, dtype=torch.float32, device=dev)
        if self.adam_mlps and not self.freeze_mlps:
            # one launch over both MLPs: Adam steps them with one rate (the top MLP's); the bottom's divisor is per tensor
            assert plan["bottom_mlp"][0] == plan["top_mlp"][0]
            self.lr_mlp = self._lr_tensor(plan["top_mlp"][0])
            top = self.model.top_model
            w16 = top.mlp.working_copies() + [top.out_working_copy()]
            parts = [(self.top_linears, self.top_grads, w16, 1.0 / plan["top_mlp"][1])]
            if self.bot_grads is not None:
                parts.append((self.bot_linears, self.bot_grads, self.model.bottom_model.mlp.working_copies(),
                              1.0 / plan["bottom_mlp"][1]))
            g, pp, mm, vv, c, mul = [], [], [], [], [], []
            for lins, grads, copies, f in parts:
                for i, l in enumerate(lins):
                    for gt, pt, cp in ((grads.views[i][0], l.weight.data, copies[i] if copies[i].shape == l.weight.shape else None),
                                       (grads.views[i][1], l.bias.data, None)):
                        g.append(gt); pp.append(pt); c.append(cp); mul.append(f)
                        mm.append(torch.zeros_like(pt)); vv.append(torch.zeros_like(pt))
            self.mlp_adam_state = (mm, vv)
            self.mlp_gmul = torch.tensor(mul, dtype=torch.float32, device=dev)
            self.t_adam = mt.TensorTable([g, pp, mm, vv, c], mt.streaming_chunk([g]))

    def _advance(self, counter):
        """counter += 1 unless the GradScaler found an inf / nan (the step is skipped then), on the device."""
        sc = self.scaler
        if sc.enabled:
            counter.add_((sc.found_inf == 0).to(torch.int32))
        else:
            counter.add_(1)

    def _emb_adam_args(self):
        """The sparse Adam arguments of this step (advances the embedding step counter on the current stream)."""
        sc = self.scaler
        self._advance(self.emb_step)
        if sc.enabled:
            gmul = self.emb_gmul if self.emb_div != 1 else sc.inv_scale
            if self.emb_div != 1:
                torch.mul(sc.inv_scale, 1.0 / self.emb_div, out=self.emb_gmul)
        else:
            gmul = self.emb_gmul
        return dict(step=self.emb_step, grad_mul=gmul, betas=self.adam_betas, eps=self.adam_eps)

    def _dense_adam_step(self):
        sc = self.scaler
        self._advance(self.mlp_step)
        mt.adam_copy(self.t_adam, self.lr_mlp, self.mlp_step, beta1=self.adam_betas[0], beta2=self.adam_betas[1], eps=self.adam_eps,
                     skip_flag=sc.found_inf if sc.enabled else None, inv_scale=sc.inv_scale if sc.enabled else None,
                     tensor_mul=self.mlp_gmul)
        top = self.model.top_model
        copies = top.mlp.working_copies() + [top.out_working_copy()]
        for i in self.top_padded:
            F.cast_rows(self.top_linears[i].weight.data, copies[i].dtype, cols_out=copies[i].shape[1], out=copies[i])
        if self.bot_grads is not None:
            bm = self.model.bottom_model.mlp
            for i in self.bot_padded:
                cp = bm.working_copies()[i]
                F.cast_rows(self.bot_linears[i].weight.data, cp.dtype, cols_out=cp.shape[1], out=cp)

    def set_lr_factor(self, factor: float):
        """LearningRateScheduler.step() (dlrm/scripts/utils.py:278-286): lr = base * factor per group."""
        if factor != self.lr_factor:
            self.lr_factor = factor
            self.lr_dp.fill_(self.base_lr * factor)
            self.lr_mp.fill_(self.base_lr * factor / self.world)

    def _dense_step(self):
        sc = self.scaler
        skip = sc.found_inf if sc.enabled else None
        inv = sc.inv_scale if sc.enabled else None
        if self.t_dense is not None:
            mt.sgd(self.t_dense, self.lr_dp, skip_flag=skip, inv_scale=inv, has_momentum=False, model_copy=True)
            top = self.model.top_model
            copies = top.mlp.working_copies() + [top.out_working_copy()]
            for i in self.top_padded:
                F.cast_rows(self.top_linears[i].weight.data, copies[i].dtype, cols_out=copies[i].shape[1], out=copies[i])
            bm = self.model.bottom_model.mlp
            for i in self.bot_padded:
                cp = bm.working_copies()[i]
                F.cast_rows(self.bot_linears[i].weight.data, cp.dtype, cols_out=cp.shape[1], out=cp)
            return
        if self.t_top_w is not None:
            mt.sgd(self.t_top_w, self.lr_dp, skip_flag=skip, inv_scale=inv, has_momentum=False, model_copy=True)
        mt.sgd(self.t_top_b, self.lr_dp, skip_flag=skip, inv_scale=inv, has_momentum=False)
        top = self.model.top_model
        for i in self.top_padded:
            lin = self.top_linears[i]
            copies = top.mlp.working_copies() + [top.out_working_copy()]
            F.cast_rows(lin.weight.data, copies[i].dtype, cols_out=copies[i].shape[1], out=copies[i])
        if self.bot_grads is not None:
            # (row-sharded placement, dlrm/row_sharded.py: the bottom MLP is data parallel there)
            lr_bot = self.lr_dp if getattr(self, "bottom_dp", False) else self.lr_mp
            if self.t_bot_w is not None:
                mt.sgd(self.t_bot_w, lr_bot, skip_flag=skip, inv_scale=inv, has_momentum=False, model_copy=True)
            mt.sgd(self.t_bot_b, lr_bot, skip_flag=skip, inv_scale=inv, has_momentum=False)
            bm = self.model.bottom_model.mlp
            for i in self.bot_padded:
                c = bm.working_copies()[i]
                F.cast_rows(self.bot_linears[i].weight.data, c.dtype, cols_out=c.shape[1], out=c)

    # ------------------------------------------------------------------ hybrid-parallel exchange
    def _exchange(self, out, inp, out_splits, in_splits):
        """The all-to-all on the COMMUNICATION stream, ordered after what the compute stream has enqueued; the caller waits
        (`_exchange_wait`) right before the first consumer, so independent compute launched in between overlaps the transfer."""
        cur = torch.cuda.current_stream()
        self.comm_stream.wait_stream(cur)
        with torch.cuda.stream(self.comm_stream):
            comm.all_to_all_single(out, inp, out_splits, in_splits, group=self.pg)
            self._a2a_event = torch.cuda.Event()
            self._a2a_event.record(self.comm_stream)
        for t in (out, inp):
            t.record_stream(self.comm_stream)

    def _exchange_wait(self):
        """The compute stream waits for the LAST all-to-all only (not for what was queued behind it on the communication stream)."""
        torch.cuda.current_stream().wait_event(self._a2a_event)

    def _bottom_to_top(self, local_out, plan=None):
        """[B_global, n_r, D] -> [B_r, n_total, D] (device feature order).  all_to_all_single over RCCL, then ONE unpack launch
        (the reference's torch.cat(dim=1) of the received blocks, dlrm/model/distributed.py:70-75)."""
        p = plan or self.plan
        recv = torch.empty(sum(p.fwd_recv_splits), dtype=local_out.dtype, device=local_out.device)
        self._exchange(recv, local_out.view(-1), p.fwd_recv_splits, p.fwd_send_splits)
        self._exchange_wait()
        x = torch.empty((p.local_batch, p.n_total, p.dim), dtype=local_out.dtype, device=local_out.device)
        F.a2a_blocks(recv, x, p.local_batch, [v * p.dim for v in p.vectors], pack=False)
        return x

    def _top_to_bottom_start(self, grad_x):
        """Reverse exchange of the gradient: [B_r, n_total, D] -> [B_global, n_r, D].  ONE pack launch, then the all-to-all on
        the communication stream; returns the receive buffer -- call _exchange_wait() before reading it."""
        p = self.plan
        send = torch.empty(sum(p.fwd_recv_splits), dtype=grad_x.dtype, device=grad_x.device)
        F.a2a_blocks(send, grad_x.contiguous(), p.local_batch, [v * p.dim for v in p.vectors], pack=True)
        out = torch.empty((p.global_batch, p.n_local, p.dim), dtype=grad_x.dtype, device=grad_x.device)
        self._exchange(out.view(-1), send, p.fwd_send_splits, p.fwd_recv_splits)
        return out

    # ------------------------------------------------------------------ validation (dlrm/scripts/main.py:733-835 dist_evaluate)
    @torch.no_grad()
    def evaluate(self, batches, batch_sizes_per_gpu=None):
        """Forward only over `batches` = iterable of (numerical or None, categorical or None, click[, valid rows]); with several
        ranks every rank's logits are gathered; AUC (utils.roc_auc_score) and the BCE loss over the whole set -> (auc, loss) on
        the main process, (None, None) elsewhere.  Batches may use a different (static) size than the train step."""
        from .utils import roc_auc_score
        m = self.model
        y_true, y_score = [], []
        plan = None
        for item in batches:
            num, cat, click = item[:3]
            valid = item[3] if len(item) > 3 else click.shape[0]
            x = m.bottom_model(num, cat)
            if self.world > 1:
                if plan is None or plan.global_batch != x.shape[0]:
                    sizes = list(batch_sizes_per_gpu) if batch_sizes_per_gpu and sum(batch_sizes_per_gpu) == x.shape[0] else \
                        [x.shape[0] // self.world] * self.world
                    plan = ExchangePlan(sizes, self.plan.vectors, self.plan.dim, self.rank)
                x = self._bottom_to_top(x, plan)
            out = m.top_model(x).reshape(-1).float()
            if self.world > 1:
                parts = [torch.empty(b, dtype=out.dtype, device=out.device) for b in plan.batch_sizes]
                if dist.get_backend(self.pg) == "nccl":
                    dist.all_gather(parts, out, group=self.pg)
                else:                                   # one-GPU test rig: staged through the host (utils/comm.py)
                    hp = [t.cpu() for t in parts]
                    dist.all_gather(hp, out.cpu(), group=self.pg)
                    parts = [t.to(out.device) for t in hp]
                out = torch.cat(parts)
            y_true.append(click.reshape(-1).float()[:valid])
            y_score.append(out[:valid])
        if self.rank != 0:
            if self.world > 1:
                dist.barrier(group=self.pg)
            return None, None
        y_true, y_score = torch.cat(y_true), torch.cat(y_score)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(y_score, y_true)
        auc = roc_auc_score(y_true, torch.sigmoid(y_score))
        if self.world > 1:
            dist.barrier(group=self.pg)
        return auc, float(loss.item())

    # ------------------------------------------------------------------ the step
    def _wgrad_stream(self):
        """Second stream for the top model's weight gradients (one rank; None with DLE_DLRM_TWO_STREAMS=0 or off the GPU)."""
        import os
        dev = self.scaler.scale.device
        if dev.type != "cuda" or os.environ.get("DLE_DLRM_TWO_STREAMS", "1") == "0":
            return None
        if getattr(self, "_wside", None) is None:
            self._wside = torch.cuda.Stream(device=dev)
        return self._wside

    def train_step(self, numerical_features, categorical_features, click):
        """One optimisation step on a (global) batch.  Returns the device-resident fp32 loss [1]."""
        m, p, sc = self.model, self.plan, self.scaler
        bottom_out = m.bottom_model(numerical_features, categorical_features)
        x = self._bottom_to_top(bottom_out) if self.world > 1 else bottom_out
        labels = click[p.batch_start[self.rank]:p.batch_start[self.rank + 1]] if self.world > 1 else click
        if self.fuse_head:
            # last layer + loss + their backward in one pass over the last hidden activation (csrc/dlrm_head.hip)
            loss = m.top_model.forward_loss_backward_head(x, labels, grad_scale=sc.scale if sc.enabled else None,
                                                          grads=self.top_grads.views[:-1], out_grads=self.top_grads.views[-1])
            dlogits = None
        else:
            logits = m.top_model(x)
            loss, dlogits = F.bce_with_logits(logits, labels, grad_scale=sc.scale if sc.enabled else None)
            dlogits = dlogits.view(-1, 1)
        # one rank: the interaction backward itself reports inf / nan in the gradient it writes (no sweep over 450 MB)
        fused_check = sc.enabled and self.world == 1
        if self.world > 1:
            # data-gradient chain of the top model first; the gradient all-to-all (xGMI) then runs on the communication stream
            # UNDER the top model's weight gradients, and the data-parallel mean of those follows it on the same stream
            grad_x, finish = m.top_model.backward(dlogits, grads=self.top_grads.views[:-1],
                                                  out_grads=self.top_grads.views[-1], defer_wgrad=True)
            grad_bottom = self._top_to_bottom_start(grad_x)
            finish()
            self.comm_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self.comm_stream):
                allreduce_mean_(self.top_grads.flat, self.pg)
            # (stream order on comm_stream: all-to-all, then the all-reduce; the compute stream needs only the former here)
            self._exchange_wait()
        else:
            # one rank: the top model's weight / bias gradients are leaves -- they run on a second stream beside the bottom model's
            # backward (embedding update on its own stream there), joined before anything reads the flat gradient buffers
            wside = self._wgrad_stream()
            grad_x, finish = m.top_model.backward(dlogits, grads=self.top_grads.views[:-1],
                                                  out_grads=self.top_grads.views[-1],
                                                  found_inf=sc.found_inf if fused_check else None, defer_wgrad=True)
            if wside is not None:
                wside.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(wside):
                    finish()
            else:
                finish()
            grad_bottom = grad_x
        if sc.enabled:
            if not fused_check:
                F.check_nonfinite_(grad_bottom, sc.found_inf)
            if self.world > 1:
                # grad_bottom is this rank's slice of a model-parallel gradient: ranks must agree on skipping the step
                # (torch's GradScaler all-reduces found_inf across the process group in the same way)
                comm.allreduce_max_(sc.found_inf, self.pg)
        emb_adam = None
        if self.adam_embeddings and not self.freeze_embeddings and m.bottom_model.embeddings is not None:
            emb_adam = self._emb_adam_args()
        m.bottom_model.backward(grad_bottom, self.lr_emb, inv_scale=sc.inv_scale if sc.enabled else None,
                                skip_flag=sc.found_inf if sc.enabled else None,
                                mlp_grads=self.bot_grads.views if self.bot_grads is not None else None,
                                freeze_embeddings=self.freeze_embeddings, emb_adam=emb_adam)
        if self.world > 1:
            torch.cuda.current_stream().wait_stream(self.comm_stream)
        elif self._wgrad_stream() is not None:
            torch.cuda.current_stream().wait_stream(self._wgrad_stream())
        if sc.enabled:
            F.check_nonfinite_(self.dense_grads, sc.found_inf)      # the dense gradients of both MLPs: one buffer, one sweep
            if self.world > 1:
                comm.allreduce_max_(sc.found_inf, self.pg)
        if not self.freeze_mlps:
            if self.adam_mlps:
                self._dense_adam_step()
            else:
                self._dense_step()
        sc.update()
        return loss
