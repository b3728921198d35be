"""Thin tensor-level wrappers over the C ABI (allocation + argument marshalling only).

Every function here launches hand-written HIP kernels from libdle_mi355x.so on the current
torch stream; there is no eager fallback.  torch is used for memory, streams and autograd plumbing.
"""
import ctypes
import os

import torch

from . import _cabi as C


# ------------------------------------------------------------------ DLRM dot interaction
def dot_interact_out_width(rows, cols):
    return C.lib().dle_dot_interact_out_width(rows, cols)


def dot_interact_fwd(x, force_generic=False):
    """x [B,R,C] -> [B, ceil8(R(R-1)/2 + C)]  (dotBasedInteractFwd)."""
    C.require_cuda(x)
    if x.dim() != 3:
        raise ValueError("dot_interact: expected [batch, rows, cols], got %s" % (tuple(x.shape),))
    x = x.contiguous()
    b, r, c = x.shape
    out = torch.empty((b, dot_interact_out_width(r, c)), dtype=x.dtype, device=x.device)
    C.annotate(bytes=float(b) * (r * c + out.shape[1]) * x.element_size())
    C.call("dle_dot_interact_fwd", C.ptr(x), C.ptr(out), b, r, c, C.dt(x), int(force_generic), C.stream())
    return out


def dot_interact_bwd(x, upstream, force_generic=False, fuse_mlp_grad=False, grad_out=None, found_inf=None):
    """-> (grad [B,R,C], mlp_grad [B,C])  (dotBasedInteractBwd).  fuse_mlp_grad: mlp_grad is added onto
    grad[:,0,:] in the kernel and None is returned in its place.  found_inf (fp32 [1], optional): set to 1 by the kernel
    when the gradient it stores holds an inf / nan (GradScaler's check without a pass over the tensor)."""
    C.require_cuda(x, upstream)
    x = x.contiguous()
    b, r, c = x.shape
    ow = dot_interact_out_width(r, c)
    if tuple(upstream.shape) != (b, ow):
        raise ValueError("dot_interact_bwd: upstream grad must be [%d, %d], got %s" % (b, ow, tuple(upstream.shape)))
    upstream = upstream.to(x.dtype).contiguous()
    grad = torch.empty_like(x) if grad_out is None else grad_out
    mlp_grad = None if fuse_mlp_grad else torch.empty((b, c), dtype=x.dtype, device=x.device)
    C.annotate(bytes=float(b) * (2 * r * c + ow + (0 if fuse_mlp_grad else c)) * x.element_size())
    if found_inf is not None:
        C.require_cuda(found_inf)
        C.call("dle_dot_interact_bwd_checked", C.ptr(x), C.ptr(upstream), C.ptr(grad), C.ptr(mlp_grad), b, r, c,
               C.dt(x), int(force_generic), C.ptr(found_inf), C.stream())
    else:
        C.call("dle_dot_interact_bwd", C.ptr(x), C.ptr(upstream), C.ptr(grad), C.ptr(mlp_grad), b, r, c,
               C.dt(x), int(force_generic), C.stream())
    return grad, mlp_grad


def gather_interact(table16, indices, offsets, hash_sizes, mlp_out, out=None):
    """Inference forward of the embedding gather and the dot interaction in one launch: table16 [sum rows, D] 16-bit joint table,
    indices int64 [B, T], offsets / hash_sizes int64 [T] or None (as emb_gather_fwd), mlp_out [B, D] = row 0 of X ->
    [B, ceil8((T+1)T/2 + D)], the bits of dot_interact_fwd(cat(mlp_out, table16[rows])).  -> None when the kernel declines (the
    caller runs the gather and dot_interact_fwd); `out` is not written then."""
    C.require_cuda(table16, indices, offsets, hash_sizes, mlp_out, out)
    if table16.dim() != 2 or indices.dim() != 2 or mlp_out.dim() != 2:
        raise ValueError("gather_interact: table16 [rows, dim], indices [batch, tables], mlp_out [batch, dim]")
    indices, offsets, hash_sizes = _i64(indices, "indices"), _i64(offsets, "offsets"), _i64(hash_sizes, "hash_sizes")
    b, t = indices.shape
    d = table16.shape[1]
    if tuple(mlp_out.shape) != (b, d) or mlp_out.dtype != table16.dtype:
        raise ValueError("gather_interact: mlp_out must be [%d, %d] %s" % (b, d, table16.dtype))
    if not (table16.is_contiguous() and mlp_out.is_contiguous()):
        raise ValueError("gather_interact: table16 and mlp_out must be contiguous")
    for name, v in (("offsets", offsets), ("hash_sizes", hash_sizes)):
        if v is not None and v.numel() < t:
            raise ValueError("%s has %d entries for %d tables" % (name, v.numel(), t))
    ow = dot_interact_out_width(t + 1, d)
    if out is None:
        out = torch.empty((b, ow), dtype=table16.dtype, device=table16.device)
    elif tuple(out.shape) != (b, ow) or out.dtype != table16.dtype or not out.is_contiguous():
        raise ValueError("gather_interact: out must be a contiguous [%d, %d] %s" % (b, ow, table16.dtype))
    C.annotate(bytes=float(b) * ((t + 1) * d * table16.element_size() + t * 8 + ow * out.element_size()))
    rc = _timed_optional("dle_dlrm_gather_interact_try", C.lib().dle_dlrm_gather_interact_try,
                         (C.ptr(table16), C.ptr(indices), C.ptr(offsets), C.ptr(hash_sizes), C.ptr(mlp_out), C.ptr(out), b, t, d,
                          C.dt(table16), C.stream()))
    if rc not in (0, 1):
        C.check(rc - 1000 if rc > 1000 else -1, "dle_dlrm_gather_interact_try")
    return out if rc == 1 else None


# ------------------------------------------------------------------ DLRM embeddings
def _i64(t, name):
    if t is None:
        return None
    if t.dtype != torch.int64:
        raise ValueError("%s must be int64 (got %s)" % (name, t.dtype))
    return t.contiguous()


def emb_gather_fwd(weight, indices, offsets=None, hash_sizes=None, out_dtype=torch.float32, out=None,
                   out_batch_stride=0):
    """out[b,t,:] = W[(idx[b,t] mod size_t) + offsets[t], :].  `out` (+ out_batch_stride in elements) lets
    the rows land inside a wider [B, 1+T, D] buffer."""
    C.require_cuda(weight, indices, offsets, hash_sizes)
    if weight.dtype != torch.float32 or weight.dim() != 2:
        raise ValueError("embedding table must be a 2-D fp32 tensor")
    if indices.dim() != 2:
        raise ValueError("indices must be [batch, tables]")
    weight = weight.contiguous() if not weight.is_contiguous() else weight
    indices, offsets, hash_sizes = _i64(indices, "indices"), _i64(offsets, "offsets"), _i64(hash_sizes, "hash_sizes")
    b, t = indices.shape
    d = weight.shape[1]
    if offsets is not None and offsets.numel() < t:
        raise ValueError("offsets has %d entries for %d tables" % (offsets.numel(), t))
    if out is None:
        out = torch.empty((b, t, d), dtype=out_dtype, device=weight.device)
    C.annotate(bytes=float(b) * t * (d * 4 + d * out.element_size() + 8))
    C.call("dle_emb_gather_fwd", C.ptr(weight), C.ptr(indices), C.ptr(offsets), C.ptr(hash_sizes), C.ptr(out),
           b, t, d, C.dt(out.dtype), out_batch_stride, C.stream())
    return out


def emb_offset_indices(indices, offsets=None, hash_sizes=None):
    C.require_cuda(indices, offsets, hash_sizes)
    indices, offsets, hash_sizes = _i64(indices, "indices"), _i64(offsets, "offsets"), _i64(hash_sizes, "hash_sizes")
    b, t = indices.shape
    rows = torch.empty_like(indices)
    C.call("dle_emb_offset_indices", C.ptr(indices), C.ptr(offsets), C.ptr(hash_sizes), C.ptr(rows), b, t, C.stream())
    return rows


def emb_grad_values(grad, scale=None):
    """fp32 COO values of the sparse embedding gradient (optionally * device scalar)."""
    C.require_cuda(grad, scale)
    grad = grad.contiguous()
    values = torch.empty(grad.shape, dtype=torch.float32, device=grad.device)
    C.call("dle_emb_grad_values", C.ptr(grad), C.ptr(values), C.ptr(scale), grad.numel(), C.dt(grad), C.stream())
    return values


def emb_sparse_sgd_(weight, rows, grad, lr, scale=None, skip_flag=None):
    """In place: W[rows[i]] -= lr * scale * grad[i] (duplicates accumulate). lr: float or device tensor."""
    C.require_cuda(weight, rows, grad, scale, skip_flag)
    if weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError("embedding table must be contiguous fp32")
    rows = _i64(rows.reshape(-1), "rows")
    d = weight.shape[1]
    grad = grad.reshape(-1, d).contiguous()
    if grad.shape[0] != rows.numel():
        raise ValueError("sparse sgd: %d gradient rows for %d indices" % (grad.shape[0], rows.numel()))
    lr_dev = lr if isinstance(lr, torch.Tensor) else None
    lr_host = 0.0 if lr_dev is not None else float(lr)
    C.call("dle_emb_sparse_sgd", C.ptr(weight), C.ptr(rows), C.ptr(grad), C.ptr(lr_dev), lr_host, C.ptr(scale),
           C.ptr(skip_flag), rows.numel(), 1, d, 0, C.dt(grad), C.stream())
    return weight


class EmbUpdateWorkspace:
    """Persistent state of the duplicate-free sparse SGD: head[total_rows] (all -1 between calls),
    next[batch*tables] scratch, the small-table mask and the host copy of the table offsets."""

    def __init__(self, table_offsets, dim, device):
        import ctypes
        import numpy as np
        off = np.ascontiguousarray(np.asarray(table_offsets, dtype=np.int64))
        self.offsets_host = off
        self.tables = off.size - 1
        self.dim = dim
        mask = np.zeros(self.tables, dtype=np.uint8)
        C.call("dle_emb_small_table_mask", off.ctypes.data_as(ctypes.c_void_p), self.tables, dim,
               mask.ctypes.data_as(ctypes.c_void_p))
        self.mask_host = mask
        self.is_small = torch.from_numpy(mask).to(device)
        self.head = torch.full((int(off[-1]),), -1, dtype=torch.int32, device=device)
        self.next = None
        # scratch of the update (one-hot partial blocks of the tiny tables, sub-lists of the mid tables), sized per batch
        sizes = off[1:] - off[:-1]
        self.n_onehot = int((sizes <= 128).sum()) if dim == 128 else 0
        self.scratch = None

    def scratch_for(self, batch, device):
        import ctypes
        need = int(C.lib().dle_emb_sgd_workspace_bytes(self.offsets_host.ctypes.data_as(ctypes.c_void_p), self.tables, self.dim,
                                                       batch))
        if need == 0:
            return None
        if self.scratch is None or self.scratch.numel() * 4 < need:
            self.scratch = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
        return self.scratch

    def next_for(self, n, device):
        if self.next is None or self.next.numel() < n:
            self.next = torch.empty(n, dtype=torch.int32, device=device)
        return self.next

    def adam_scratch_for(self, batch, device):
        """Scratch of the sparse Adam update (dle_emb_adam_workspace_bytes), kept apart from the SGD's and grown on demand."""
        import ctypes
        need = int(C.lib().dle_emb_adam_workspace_bytes(self.offsets_host.ctypes.data_as(ctypes.c_void_p), self.tables, self.dim,
                                                        batch))
        if getattr(self, "adam_scratch", None) is None or self.adam_scratch.numel() * 4 < max(need, 4):
            self.adam_scratch = torch.empty(max((need + 3) // 4, 1), dtype=torch.float32, device=device)
        return self.adam_scratch


def emb_sgd_dedup_(weight, rows, grad, ws, lr, scale=None, skip_flag=None, grad_batch_stride=0):
    """In place W[rows[b,t]] -= lr*scale*grad[b,t] with duplicate rows summed first (no float atomics).
    rows int64 [B,T]; grad: tensor whose element (b,t,0) sits at data_ptr + b*grad_batch_stride + t*dim."""
    import ctypes
    C.require_cuda(weight, rows, grad, scale, skip_flag)
    if weight.dtype != torch.float32 or not weight.is_contiguous():
        raise ValueError("embedding table must be contiguous fp32")
    rows = _i64(rows, "rows")
    b, t = rows.shape
    if t != ws.tables or weight.shape[1] != ws.dim:
        raise ValueError("workspace was built for %d tables x dim %d" % (ws.tables, ws.dim))
    lr_dev = lr if isinstance(lr, torch.Tensor) else None
    lr_host = 0.0 if lr_dev is not None else float(lr)
    nxt = ws.next_for(b * t, weight.device)
    # algorithmic: grad row read + table row read-modify-write + row id
    C.annotate(bytes=float(b) * t * (ws.dim * grad.element_size() + 2 * ws.dim * 4 + 8))
    oh = ws.scratch_for(b, weight.device) if grad.dtype in (torch.float16, torch.bfloat16) else None
    C.call("dle_emb_sgd_dedup_ws", C.ptr(weight), C.ptr(rows), C.ptr(grad), C.ptr(ws.head), C.ptr(nxt),
           C.ptr(ws.is_small), ws.offsets_host.ctypes.data_as(ctypes.c_void_p), C.ptr(lr_dev), lr_host,
           C.ptr(scale), C.ptr(skip_flag), b, t, ws.dim, grad_batch_stride, C.dt(grad), C.ptr(oh),
           oh.numel() * 4 if oh is not None else 0, C.stream())
    return weight


def emb_adam_dedup_(weight, exp_avg, exp_avg_sq, rows, grad, ws, lr, step, grad_mul=None, skip_flag=None, betas=(0.9, 0.999),
                    eps=1e-8, grad_batch_stride=0, touched_rows=None):
    """torch.optim.SparseAdam on the rows `rows` looks up, in place: duplicates of a row are summed (fp32) first, then every
    looked-up row -- one whose sum is 0 included -- takes one step with g = sum * grad_mul; other rows keep w / m / v bit for bit.
    weight / exp_avg / exp_avg_sq: contiguous fp32 [rows, dim]; rows int64 [B,T]; grad as for emb_sgd_dedup_; step: int32 device
    tensor [1] holding t of THIS update; lr: float or fp32 device tensor [1]; grad_mul / skip_flag: fp32 device tensors [1] or None.
    touched_rows (optional, host int): distinct rows of the batch, for the algorithmic byte count of a kernel timer (without it
    the count covers the gradient reads and row ids only)."""
    import ctypes
    C.require_cuda(weight, exp_avg, exp_avg_sq, rows, grad, step, grad_mul, skip_flag)
    for name, x in (("embedding table", weight), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("%s must be contiguous fp32" % name)
    if exp_avg.shape != weight.shape or exp_avg_sq.shape != weight.shape:
        raise ValueError("exp_avg / exp_avg_sq must have the table's shape %s" % (tuple(weight.shape),))
    if step.dtype != torch.int32 or step.numel() != 1:
        raise ValueError("step must be an int32 device tensor of one element")
    if grad.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError("gradient dtype %s: fp32, fp16 or bf16" % grad.dtype)
    rows = _i64(rows, "rows")
    b, t = rows.shape
    if t != ws.tables or weight.shape[1] != ws.dim:
        raise ValueError("workspace was built for %d tables x dim %d" % (ws.tables, ws.dim))
    lr_dev = lr if isinstance(lr, torch.Tensor) else None
    lr_host = 0.0 if lr_dev is not None else float(lr)
    nxt = ws.next_for(b * t, weight.device)
    scratch = ws.adam_scratch_for(b, weight.device)
    # algorithmic: gradient row + row id per lookup, plus w, m, v read + written per touched row when that count is given (without
    # it the count would need a host read-back: the annotation is then the lower, gradient-side bound)
    table_side = 0.0 if touched_rows is None else float(touched_rows) * 6 * ws.dim * 4
    C.annotate(bytes=table_side + float(b) * t * (ws.dim * grad.element_size() + 8))
    C.call("dle_emb_adam_dedup_ws", C.ptr(weight), C.ptr(exp_avg), C.ptr(exp_avg_sq), C.ptr(rows), C.ptr(grad), C.ptr(ws.head),
           C.ptr(nxt), ws.offsets_host.ctypes.data_as(ctypes.c_void_p), C.ptr(lr_dev), lr_host, C.ptr(grad_mul), C.ptr(skip_flag),
           C.ptr(step), 1.0 - float(betas[0]), 1.0 - float(betas[1]), float(eps), b, t, ws.dim, grad_batch_stride, C.dt(grad), C.ptr(scratch),
           scratch.numel() * 4, C.stream())
    return weight


# ------------------------------------------------------------------ small train-step kernels
def cast_rows(x, out_dtype, cols_out=None, out=None):
    """2-D cast with optional zero padding of the trailing columns (K padded to a multiple of 8/16)."""
    C.require_cuda(x, out)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("cast_rows expects a 2-D tensor with unit inner stride")
    r, c = x.shape
    co = c if cols_out is None else cols_out
    if out is None:
        out = torch.empty((r, co), dtype=out_dtype, device=x.device)
    C.call("dle_cast_rows", C.ptr(x), C.ptr(out), r, c, co, x.stride(0), out.stride(0), C.dt(x), C.dt(out),
           C.stream())
    return out


def a2a_blocks(blocks, x, rows, widths, pack):
    """blocks: flat concatenation over ranks of [rows, widths[s]] matrices; x: [rows, sum(widths)] contiguous.  pack=False:
    x <- blocks (after the forward all-to-all); pack=True: blocks <- x (before the backward one).  One launch."""
    import ctypes
    C.require_cuda(blocks, x)
    if not (blocks.is_contiguous() and x.is_contiguous()) or blocks.dtype != x.dtype or blocks.numel() != x.numel():
        raise ValueError("a2a_blocks: contiguous buffers of one dtype and size")
    if x.numel() != rows * sum(widths):
        raise ValueError("a2a_blocks: x must hold rows x sum(widths) elements")
    w = (ctypes.c_int * len(widths))(*[int(v) for v in widths])
    C.call("dle_a2a_blocks", C.ptr(blocks), C.ptr(x), int(rows), len(widths), ctypes.cast(w, ctypes.c_void_p), x.element_size(),
           int(bool(pack)), C.stream())
    return blocks if pack else x


def transpose_cast(x, out_dtype, out=None):
    """out[c, r] = (out_dtype) x[r, c] for a 2-D fp32 / 16-bit matrix with unit inner stride: the transposed 16-bit working copy."""
    C.require_cuda(x, out)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("transpose_cast: 2-D input with unit inner stride")
    r, c = x.shape
    if out is None:
        out = torch.empty((c, r), dtype=out_dtype, device=x.device)
    if out.shape != (c, r) or out.stride(1) != 1 or out.dtype != out_dtype:
        raise ValueError("transpose_cast: output must be [cols, rows] of the requested dtype")
    C.call("dle_transpose_cast", C.ptr(x), C.ptr(out), r, c, x.stride(0), out.stride(0), C.dt(x), C.dt(out), C.stream())
    return out


def cast(x, out_dtype, out=None):
    """Flat dtype cast of a contiguous tensor."""
    C.require_cuda(x, out)
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    n = x.numel()
    C.call("dle_cast_rows", C.ptr(x), C.ptr(out), 1, n, n, n, n, C.dt(x), C.dt(out), C.stream())
    return out


def bce_with_logits(logits, target, grad_scale=None, want_grad=True, ld_logits=1):
    """-> (loss fp32 [1], dlogits or None).  dlogits = d(mean BCE)/dlogits * grad_scale."""
    C.require_cuda(logits, target, grad_scale)
    if target.dtype != torch.float32:
        raise ValueError("BCE targets must be fp32")
    n = target.numel()
    loss = torch.empty(1, dtype=torch.float32, device=target.device)
    dl = torch.empty(n, dtype=logits.dtype, device=logits.device) if want_grad else None
    C.call("dle_bce_logits", C.ptr(logits), C.ptr(target), C.ptr(loss), C.ptr(dl), C.ptr(grad_scale), n,
           ld_logits, C.dt(logits), C.stream())
    return loss, dl


class HeadWorkspace:
    """Scratch of head_bce_fwd_bwd for one (batch, K): one partial row per workgroup."""

    def __init__(self, m, k, device):
        self.m, self.k = int(m), int(k)
        nbytes = int(C.lib().dle_head_bce_workspace_bytes(self.m, self.k))
        self.buf = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def head_bce_fwd_bwd(h, w16, bias, target, grad_scale, gw, gb, ws, gprev_bias=None, dh=None, want_logits=False):
    """Last linear layer (out_features = 1) + BCEWithLogitsLoss(mean) + the backward of both in one pass over h [M, K] (16-bit):
    -> (loss fp32 [1], dh [M, K] masked by the ReLU of h, logits [M] or None); gw [K], gb [1] and (optional) gprev_bias [K] =
    column sums of dh are written in place (fp32)."""
    C.require_cuda(h, w16, bias, target, grad_scale, gw, gb, gprev_bias, dh)
    if h.dim() != 2 or h.stride(1) != 1 or target.dtype != torch.float32 or h.dtype != w16.dtype:
        raise ValueError("head_bce_fwd_bwd: h [M, K] 16-bit with unit inner stride, w16 of the same dtype, fp32 targets")
    m, k = h.shape
    if target.numel() != m or w16.numel() != k or gw.numel() != k or ws.m != m or ws.k != k:
        raise ValueError("head_bce_fwd_bwd: shape mismatch")
    for t in (gw, gb, gprev_bias):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise ValueError("head_bce_fwd_bwd: gradients are contiguous fp32 buffers")
    if dh is None:
        dh = torch.empty((m, k), dtype=h.dtype, device=h.device)
    loss = torch.empty(1, dtype=torch.float32, device=h.device)
    logits = torch.empty(m, dtype=h.dtype, device=h.device) if want_logits else None
    C.annotate(bytes=2.0 * m * k * h.element_size() + 6.0 * m, tag="%dx%d" % (m, k))
    C.call("dle_head_bce_fwd_bwd", C.ptr(h), C.ptr(w16), C.ptr(bias), C.ptr(target), C.ptr(grad_scale), C.ptr(loss),
           C.ptr(logits), C.ptr(dh), C.ptr(gw), C.ptr(gb), C.ptr(gprev_bias), C.ptr(ws.buf), ws.buf.numel() * 4, m, k,
           h.stride(0), dh.stride(0), C.dt(h), C.stream())
    return loss, dh, logits


def amp_update_scale_(scale, growth_tracker, found_inf, inv_scale=None, growth_factor=2.0, backoff_factor=0.5,
                      growth_interval=2000, clear_found_inf=True):
    C.require_cuda(scale, growth_tracker, found_inf, inv_scale)
    C.call("dle_amp_update_scale", C.ptr(scale), C.ptr(growth_tracker), C.ptr(found_inf), C.ptr(inv_scale),
           float(growth_factor), float(backoff_factor), int(growth_interval), int(clear_found_inf), C.stream())


def axpby_(x, y, out, a=1.0, b=1.0):
    """out = a * x + b * y on flat fp32 tensors (out may be x or y; y may be None when b == 0)."""
    C.require_cuda(x, y, out)
    if x.dtype != torch.float32 or out.dtype != torch.float32 or not (x.is_contiguous() and out.is_contiguous()):
        raise ValueError("axpby_ expects contiguous fp32 tensors")
    if out.numel() != x.numel() or (y is not None and y.numel() != x.numel()):
        raise ValueError("axpby_: size mismatch")
    C.call("dle_axpby_f32", C.ptr(x), C.ptr(y), C.ptr(out), float(a), float(b if y is not None else 0.0), x.numel(), C.stream())
    return out


def check_nonfinite_(x, found_inf):
    C.require_cuda(x, found_inf)
    C.call("dle_check_nonfinite", C.ptr(x), C.ptr(found_inf), x.numel(), C.dt(x), C.stream())


# ------------------------------------------------------------------ GEMM
def gemm(a, b, m, n, k, a_kc, b_kc, out=None, out_dtype=None, bias=None, act=C.ACT_NONE, aux=None,
         mask_src=None, splitk=1, accumulate=False, alpha=1.0, lda=None, ldb=None):
    """C[m,n] = act(alpha * A(m,k) B(n,k) + bias).  a/b are 2-D 16-bit tensors, row-major with
    arbitrary leading dimension; a_kc/b_kc say whether the contraction dim is the contiguous one."""
    C.require_cuda(a, b, out, bias, aux, mask_src)
    if a.dtype != b.dtype or a.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("gemm inputs must both be f16 or both bf16 (got %s, %s)" % (a.dtype, b.dtype))
    def _ld(t):
        if t.shape[-1] != 1 and t.stride(-1) != 1:
            raise ValueError("gemm operands must have unit inner stride")
        return t.stride(0) if (t.shape[0] > 1 and t.stride(0) >= t.shape[-1]) else t.shape[-1]
    lda = _ld(a) if lda is None else lda
    ldb = _ld(b) if ldb is None else ldb
    if out is None:
        out = torch.empty((m, n), dtype=out_dtype or a.dtype, device=a.device)
    if out.stride(-1) != 1:
        raise ValueError("gemm output must have unit inner stride")
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != n):
        raise ValueError("gemm bias must be fp32 [n]")
    if mask_src is not None and m > 1 and mask_src.dim() == 2 and out.dim() == 2 and mask_src.stride(0) != out.stride(0):
        # (the epilogues address the source tensor with the output's row pitch: another pitch would read other elements, and past
        #  the end of a dense source behind a row-strided output)
        raise ValueError("gemm mask_src must have the row pitch of the output (%d, got %d)" % (out.stride(0), mask_src.stride(0)))
    extra = (float(m * n) * mask_src.element_size() if mask_src is not None else 0.0) + \
            (float(aux.numel()) * aux.element_size() if aux is not None else 0.0)
    C.annotate(flops=2.0 * m * n * k,
               bytes=float(m * k + n * k) * a.element_size() + float(m * n) * out.element_size() + extra,
               tag="%dx%dx%d%s%s" % (m, n, k, "+src" if mask_src is not None else "", "+aux" if aux is not None else ""),
               replay=not accumulate)
    ws = splitk_workspace(a.device, splitk * m * n * 4) if splitk > 1 else None
    C.call("dle_gemm", C.ptr(a), C.ptr(b), C.ptr(out), C.ptr(aux), C.ptr(bias), C.ptr(mask_src), m, n, k,
           lda, ldb, out.stride(0) if out.dim() == 2 else n, int(a_kc), int(b_kc), C.dt(a), C.dt(out), act,
           splitk, int(accumulate), float(alpha), C.ptr(ws), ws.numel() * 4 if ws is not None else 0, C.stream())
    return out


_splitk_ws = {}


def splitk_workspace(device, nbytes):
    """fp32 scratch for split-K partial slabs, reduction partials and the like: one buffer per (device, CURRENT STREAM), grown on
    demand -- launches of one stream use it one after the other; two streams running kernels side by side (the weight-gradient
    stream of the ResNet engine) must not share it."""
    key = (device, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    w = _splitk_ws.get(key)
    if w is None or w.numel() * 4 < nbytes:
        w = torch.empty(max(nbytes // 4, 1 << 22), dtype=torch.float32, device=device)
        _splitk_ws[key] = w
    return w


def gemm_colsum(g, w, m, n, k, src, colsum_out, act=C.ACT_RELU_BWD, accumulate=False):
    """dX [m, n] = f(g [m, k] w [k, n], src [m, n]) and colsum_out [n] (fp32) (+)= column sums of the rounded dX: the data gradient
    of a linear layer through the activation derivative of the layer below + that layer's bias gradient in one launch (+ a small
    fold).  act = ACT_RELU_BWD (dX = product where src > 0) or ACT_MUL (dX = product * src).  -> dX, or None outside the kernel's
    envelope (the caller runs gemm + colsum)."""
    C.require_cuda(g, w, src, colsum_out)
    if (g.dtype not in (torch.float16, torch.bfloat16) or w.dtype != g.dtype or src.dtype != g.dtype
            or g.stride(1) != 1 or w.stride(1) != 1 or src.stride(1) != 1 or act not in (C.ACT_RELU_BWD, C.ACT_MUL)
            or colsum_out.dtype != torch.float32 or not colsum_out.is_contiguous() or colsum_out.numel() != n):
        return None
    out = torch.empty((m, n), dtype=g.dtype, device=g.device)
    if src.stride(0) != out.stride(0):
        return None
    ws = splitk_workspace(g.device, ((m + 127) // 128) * n * 4)
    by = float(m) * (k + 2 * n) * g.element_size() + float(k) * n * w.element_size()
    C.annotate(bytes=by, flops=2.0 * m * n * k, tag="%dx%dx%d+src+colsum" % (m, n, k))
    # (recorded in the family of the GEMM it replaces)
    rc = _timed_optional("dle_gemm", C.lib().dle_gemm_colsum,
                         (C.ptr(g), C.ptr(w), C.ptr(out), C.ptr(src), C.ptr(colsum_out), m, n, k, g.stride(0), w.stride(0),
                          out.stride(0), C.dt(g), int(act), int(accumulate), C.ptr(ws), ws.numel() * 4, C.stream()),
                         replayable=not accumulate)
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_gemm_colsum")
    return out if rc == 1 else None


def gemm_relu_bits(x, w, m, n, k, bias):
    """y [m, n] = relu(x [m, k] w [n, k]^T + bias) together with the KEEP BITS of y (uint8 [m n / 8]: bit (i n + j) & 7 of byte
    (i n + j) >> 3 = y[i, j] > 0) -- one (Linear + ReLU) layer whose backward reads 1 bit per element instead of y
    (csrc/gemm8_kernel.h ACT_RELU_BITS; dlrm/nn/mlps.py:38-43).  -> (y, bits), or None outside the ping-pong kernel's envelope
    (the caller runs gemm(act=ACT_RELU) and keeps y as the mask source).  y is bit-identical to gemm(act=ACT_RELU)."""
    C.require_cuda(x, w, bias)
    if (x.dtype not in (torch.float16, torch.bfloat16) or w.dtype != x.dtype or x.stride(1) != 1 or w.stride(1) != 1
            or n % 16 != 0 or bias is None or bias.dtype != torch.float32):
        return None
    y = torch.empty((m, n), dtype=x.dtype, device=x.device)
    bits = torch.empty(m * n // 8, dtype=torch.uint8, device=x.device)
    C.annotate(bytes=float(m) * (k + n) * x.element_size() + float(k) * n * w.element_size() + bits.numel(), flops=2.0 * m * n * k,
               tag="%dx%dx%d+bits" % (m, n, k))
    rc = _timed_optional("dle_gemm", C.lib().dle_gemm8_relu_bits_try,
                         (C.ptr(x), C.ptr(w), C.ptr(y), C.ptr(bits), C.ptr(bias), m, n, k, x.stride(0), w.stride(0), C.dt(x), C.stream()))
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_gemm8_relu_bits_try")
    return (y, bits) if rc == 1 else None


def gemm_colsum_bits(g, w, m, n, k, bits, colsum_out, accumulate=False):
    """gemm_colsum(act=ACT_RELU_BWD) with the mask given as the keep bits gemm_relu_bits left (1 bit per element) instead of the
    16-bit activation: dX [m, n] = (g [m, k] w [k, n]) where the bit is set, colsum_out [n] (+)= column sums of the rounded dX.
    -> dX, or None outside the envelope (the caller uses gemm_colsum with the activation)."""
    C.require_cuda(g, w, bits, colsum_out)
    if (g.dtype not in (torch.float16, torch.bfloat16) or w.dtype != g.dtype or g.stride(1) != 1 or w.stride(1) != 1
            or bits.dtype != torch.uint8 or bits.numel() != m * n // 8 or n % 16 != 0 or m % 256 != 0
            or colsum_out.dtype != torch.float32 or not colsum_out.is_contiguous() or colsum_out.numel() != n):
        return None
    out = torch.empty((m, n), dtype=g.dtype, device=g.device)
    ws = splitk_workspace(g.device, ((m + 127) // 128) * n * 4)
    by = float(m) * (k + n) * g.element_size() + float(k) * n * w.element_size() + bits.numel()
    C.annotate(bytes=by, flops=2.0 * m * n * k, tag="%dx%dx%d+bits+colsum" % (m, n, k))
    rc = _timed_optional("dle_gemm", C.lib().dle_gemm_colsum_bits,
                         (C.ptr(g), C.ptr(w), C.ptr(out), C.ptr(bits), C.ptr(colsum_out), m, n, k, g.stride(0), w.stride(0), C.dt(g),
                          int(accumulate), C.ptr(ws), ws.numel() * 4, C.stream()), replayable=not accumulate)
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_gemm_colsum_bits")
    return out if rc == 1 else None


def colsum(x, out=None, accumulate=False):
    """fp32 column sums of a 2-D tensor (bias gradient)."""
    C.require_cuda(x, out)
    if x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("colsum expects a 2-D tensor with unit inner stride")
    m, n = x.shape
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=x.device)
        accumulate = False
    ws = splitk_workspace(x.device, 2048 * n * 4)
    C.annotate(bytes=float(m) * n * x.element_size(), tag="%dx%d" % (m, n))
    C.call("dle_colsum", C.ptr(x), C.ptr(out), m, n, x.stride(0) if m > 1 else n, C.dt(x), int(accumulate),
           C.ptr(ws), ws.numel() * 4, C.stream())
    return out


class ColsumTable:
    """Device table of (matrix, fp32 destination) pairs for colsum_batched; the tensors are kept alive here (their ADDRESSES are
    in the table: they must be persistent buffers)."""

    def __init__(self, entries):
        self.entries = list(entries)
        src0 = self.entries[0][0]
        for x, out in self.entries:
            C.require_cuda(x, out)
            if x.shape != src0.shape or x.dtype != src0.dtype or not x.is_contiguous() or x.dim() != 2:
                raise ValueError("ColsumTable: contiguous 2-D matrices of one shape and dtype")
            if out.dtype != torch.float32 or out.numel() != x.shape[1] or not out.is_contiguous():
                raise ValueError("ColsumTable: fp32 destinations of N elements")
        self.n = len(self.entries)
        self.dev = torch.tensor([[x.data_ptr(), o.data_ptr()] for x, o in self.entries], dtype=torch.int64).to(src0.device)


def colsum_batched(table, m, n, ld, dtype):
    """fp32 column sums of every matrix of a ColsumTable ([m, n], row pitch ld) into its destination: one launch pair."""
    need = int(C.lib().dle_colsum_batched_workspace_bytes(table.n, m, n))
    ws = splitk_workspace(table.dev.device, need)
    C.annotate(bytes=float(table.n) * m * n * 2, tag="b%dx%dx%d" % (table.n, m, n))
    C.call("dle_colsum_batched", C.ptr(table.dev), table.n, m, n, ld, C.dt(dtype), C.ptr(ws), ws.numel() * 4, C.stream())


def pick_splitk(m_out, n_out, k, target_blocks=512):
    """Split the contraction so that a skinny wgrad still fills 256 CUs (K tiles of 64).  Outputs of at least 256x256
    run on the 256x256 tile (gemm_dma.hip launch_gemm): ONE slice per CU (256 // tiles, each >= 4 K tiles deep) -- the big
    tile issues half the LDS-DMA pieces per MFMA of the 128x128 one, which is what bounds the split weight gradients."""
    ktiles = (k + 63) // 64
    if m_out >= 256 and n_out >= 256 and "DLE_SPLITK_TARGET" not in os.environ:
        tiles_big = ((m_out + 255) // 256) * ((n_out + 255) // 256)
        if tiles_big >= 160:
            return 1
        s = min(ktiles // 4, max(256 // tiles_big, 1))
        if tiles_big <= 2:
            s = min(s, 64)      # (256x512x65536: 46 us at 64 slices, 56 at 128 -- each slice writes a whole fp32 slab of the output)
        if s >= 2 and tiles_big * s >= 128:
            return s
    target_blocks = int(os.environ.get("DLE_SPLITK_TARGET", target_blocks))      # tuning knob (tools/, not the product default)
    tiles = ((m_out + 127) // 128) * ((n_out + 127) // 128)
    s = max(1, min(ktiles, target_blocks // max(tiles, 1)))
    return s


def linear_fwd(x, w, bias=None, act=C.ACT_NONE, want_pre=False):
    """y = act(x @ w.T + bias); x [M,K], w [N,K] (both 16-bit).  Returns (y, pre or None)."""
    m, k = x.shape
    n = w.shape[0]
    pre = torch.empty((m, n), dtype=x.dtype, device=x.device) if want_pre else None
    y = gemm(x, w, m, n, k, True, True, bias=bias, act=act, aux=pre)
    return y, pre


def linear_dgrad(gy, w, mask_src=None):
    """dx[M,K] = gy[M,N] @ w[N,K]  (optionally * (mask_src > 0))."""
    m, n = gy.shape
    k = w.shape[1]
    return gemm(gy, w, m, k, n, True, False, act=C.ACT_RELU_BWD if mask_src is not None else C.ACT_NONE,
                mask_src=mask_src)


def linear_wgrad(gy, x, out=None, accumulate=False):
    """dw[N,K] (fp32) = gy[M,N].T @ x[M,K]."""
    m, n = gy.shape
    k = x.shape[1]
    sk = pick_splitk(n, k, m)
    if out is None:
        out = torch.empty((n, k), dtype=torch.float32, device=x.device)
        accumulate = False
    return gemm(gy, x, n, k, m, False, False, out=out, splitk=sk, accumulate=accumulate)


def relu_bwd(g, y, out=None):
    """g * (y > 0) for 16-bit 2-D (possibly row-strided) views."""
    C.require_cuda(g, y, out)
    if g.dim() != 2 or g.shape != y.shape or g.stride(1) != 1 or y.stride(1) != 1:
        raise ValueError("relu_bwd expects matching 2-D views with unit inner stride")
    r, c = g.shape
    if out is None:
        out = torch.empty((r, c), dtype=g.dtype, device=g.device)
    C.call("dle_relu_bwd", C.ptr(g), C.ptr(y), C.ptr(out), r, c, g.stride(0), y.stride(0), out.stride(0), C.dt(g),
           C.stream())
    return out


def copy_rows(src, dst):
    """dst[r, :] = src[r, :] for 2-D views with unit inner stride (row strides may differ)."""
    C.require_cuda(src, dst)
    if src.shape != dst.shape or src.dtype != dst.dtype:
        raise ValueError("copy_rows: shape/dtype mismatch")
    r, c = src.shape
    C.call("dle_cast_rows", C.ptr(src), C.ptr(dst), r, c, c, src.stride(0), dst.stride(0), C.dt(src), C.dt(dst),
           C.stream())
    return dst


# ------------------------------------------------------------------ convolutions (NHWC / KRSC, implicit GEMM)
def _conv_out(h, w, r, s, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - s) // stride + 1


def conv2d_fwd(x, w, stride=1, pad=0, bias=None, act=C.ACT_NONE, out=None, out_dtype=None):
    """x [N,H,W,C], w [Ko,R,S,C] (both 16-bit, contiguous) -> y [N,P,Q,Ko]."""
    C.require_cuda(x, w, bias, out)
    n, h, wd, c = x.shape
    ko, r, s, c2 = w.shape
    if c2 != c or not x.is_contiguous() or not w.is_contiguous() or x.dtype != w.dtype:
        raise ValueError("conv2d_fwd: x must be NHWC-contiguous and w KRSC-contiguous with matching C/dtype")
    p, q = _conv_out(h, wd, r, s, stride, pad)
    if out is None:
        out = torch.empty((n, p, q, ko), dtype=out_dtype or x.dtype, device=x.device)
    C.annotate(flops=2.0 * n * p * q * ko * r * s * c, tag="fwd %dx%dx%dx%d k%d %dx%d s%d" % (n, h, wd, c, ko, r, s, stride),
               bytes=float(x.numel() + w.numel() + out.numel()) * 2)
    C.call("dle_conv2d_fwd", C.ptr(x), C.ptr(w), C.ptr(out), C.ptr(bias), n, h, wd, c, ko, r, s, stride, pad,
           C.dt(x), C.dt(out), act, C.stream())
    return out


def conv2d_fwd_affine(x, w, scale, shift, stride=1, pad=0, residual=None, relu=True, out=None):
    """Inference unit in one launch: y = relu?(scale[ko] * conv(x, w) + shift[ko] (+ residual)) on the fp32 accumulator, rounded
    once.  x [N,H,W,C], w [Ko,R,S,C] (16-bit, contiguous), scale / shift fp32 [Ko], residual [N,P,Q,Ko] or None -> y [N,P,Q,Ko]."""
    C.require_cuda(x, w, scale, shift, residual, out)
    n, h, wd, c = x.shape
    ko, r, s, c2 = w.shape
    p, q = _conv_out(h, wd, r, s, stride, pad)
    if c2 != c or not x.is_contiguous() or not w.is_contiguous() or x.dtype != w.dtype:
        raise ValueError("conv2d_fwd_affine: x must be NHWC-contiguous and w KRSC-contiguous with matching C/dtype")
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.numel() != ko or not t.is_contiguous():
            raise ValueError("conv2d_fwd_affine: scale / shift must be contiguous fp32 [Ko]")
    if residual is not None and (tuple(residual.shape) != (n, p, q, ko) or residual.dtype != x.dtype or not residual.is_contiguous()):
        raise ValueError("conv2d_fwd_affine: residual must be a contiguous [N,P,Q,Ko] tensor of x's dtype")
    if out is None:
        out = torch.empty((n, p, q, ko), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (n, p, q, ko) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("conv2d_fwd_affine: out must be a contiguous [N,P,Q,Ko] tensor of x's dtype")
    C.annotate(flops=2.0 * n * p * q * ko * r * s * c, tag="affine %dx%dx%dx%d k%d %dx%d s%d%s" % (n, h, wd, c, ko, r, s, stride,
                                                                                                "+res" if residual is not None else ""),
               bytes=float(x.numel() + w.numel() + out.numel() * (2 if residual is not None else 1)) * 2)
    C.call("dle_conv2d_fwd_affine", C.ptr(x), C.ptr(w), C.ptr(out), C.ptr(scale), C.ptr(shift), C.ptr(residual), n, h, wd, c, ko,
           r, s, stride, pad, C.dt(x), int(bool(relu)), C.stream())
    return out


def pack_grouped_weight(w, dtype):
    """torch's grouped OIHW weight [Ko, Cg, 3, 3] (any device / float dtype / memory format) -> the [Ko, 3, 3, Cg] 16-bit tensor
    conv2d_grouped_fwd_affine reads (one rounding per element)."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError("pack_grouped_weight: expected a [Ko, Cg, 3, 3] weight (got %s)" % (tuple(w.shape),))
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("pack_grouped_weight: dtype must be torch.float16 or torch.bfloat16")
    return w.detach().permute(0, 2, 3, 1).to(dtype).contiguous()


def conv2d_grouped_fwd_affine(x, w, scale, shift, groups, stride=1, relu=True, out=None):
    """Grouped 3x3 / pad 1 inference unit in one launch: y = relu?(scale[ko] * conv_g(x, w) + shift[ko]) on the fp32 accumulator,
    rounded once.  x [N,H,W,C], w [Ko,3,3,C/groups] (pack_grouped_weight; 16-bit, contiguous), scale / shift fp32 [Ko]
    -> y [N,P,Q,Ko].  C == Ko, C % 64 == 0, C / groups in {4, 8, 16, 32}, stride 1 or 2: anything else raises ValueError."""
    C.require_cuda(x, w, scale, shift, out)
    if x.dim() != 4 or w.dim() != 4:
        raise ValueError("conv2d_grouped_fwd_affine: x must be [N,H,W,C] and w [Ko,3,3,Cg]")
    n, h, wd, c = x.shape
    ko, r, s, cg = w.shape
    if x.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("conv2d_grouped_fwd_affine: 16-bit activations and weights only (got %s)" % x.dtype)
    if (r, s) != (3, 3) or groups < 1 or cg * groups != c or not x.is_contiguous() or not w.is_contiguous() or x.dtype != w.dtype:
        raise ValueError("conv2d_grouped_fwd_affine: x must be NHWC-contiguous and w [Ko,3,3,C/groups]-contiguous of x's dtype")
    if stride < 1:
        raise ValueError("conv2d_grouped_fwd_affine: stride 1 or 2")
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.numel() != ko or not t.is_contiguous():
            raise ValueError("conv2d_grouped_fwd_affine: scale / shift must be contiguous fp32 [Ko]")
    p, q = _conv_out(h, wd, 3, 3, stride, 1)
    if out is None:
        out = torch.empty((n, p, q, ko), dtype=x.dtype, device=x.device)
    elif tuple(out.shape) != (n, p, q, ko) or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError("conv2d_grouped_fwd_affine: out must be a contiguous [N,P,Q,Ko] tensor of x's dtype")
    C.annotate(flops=2.0 * n * p * q * ko * 9 * cg, tag="grouped %dx%dx%dx%d g%d s%d" % (n, h, wd, c, groups, stride),
               bytes=float(x.numel() + w.numel() + out.numel()) * 2)
    C.call("dle_conv2d_grouped_fwd_affine", C.ptr(x), C.ptr(w), C.ptr(out), C.ptr(scale), C.ptr(shift), n, h, wd, c, ko, groups,
           stride, C.dt(x), int(bool(relu)), C.stream())
    return out


def se_gate(t, w1, b1, w2, b2, out=None):
    """Squeeze-and-excitation gate: sigmoid(w2 @ relu(w1 @ mean_hw(t) + b1) + b2) per image, in fp32.  t [N,H,W,C] or [N,HW,C]
    16-bit contiguous; w1 [S,C], b1 [S], w2 [C,S], b2 [C] contiguous fp32 (S <= 64) -> gate [N,C] fp32."""
    C.require_cuda(t, w1, b1, w2, b2, out)
    if t.dim() not in (3, 4) or not t.is_contiguous() or t.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("se_gate: t must be a contiguous 16-bit [N,H,W,C] or [N,HW,C] tensor")
    n, c = t.shape[0], t.shape[-1]
    hw = t.numel() // max(n * c, 1)
    s = w1.shape[0]
    for v, shape in ((w1, (s, c)), (b1, (s,)), (w2, (c, s)), (b2, (c,))):
        if v.dtype != torch.float32 or tuple(v.shape) != shape or not v.is_contiguous():
            raise ValueError("se_gate: weights must be contiguous fp32 w1 [S,C], b1 [S], w2 [C,S], b2 [C]")
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=t.device)
    elif tuple(out.shape) != (n, c) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("se_gate: out must be a contiguous fp32 [N,C] tensor")
    C.call("dle_se_gate", C.ptr(t), C.ptr(w1), C.ptr(b1), C.ptr(w2), C.ptr(b2), C.ptr(out), n, hw, c, s, C.dt(t), C.stream())
    return out


def se_apply(t, gate, residual=None, relu=True, out=None):
    """y = relu?(t * gate[n, c] + residual) in fp32, rounded once.  t, residual (or None) 16-bit contiguous [N,H,W,C] / [N,HW,C],
    gate fp32 [N,C] -> y of t's shape and dtype."""
    C.require_cuda(t, gate, residual, out)
    if t.dim() not in (3, 4) or not t.is_contiguous() or t.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError("se_apply: t must be a contiguous 16-bit [N,H,W,C] or [N,HW,C] tensor")
    n, c = t.shape[0], t.shape[-1]
    hw = t.numel() // max(n * c, 1)
    if gate.dtype != torch.float32 or tuple(gate.shape) != (n, c) or not gate.is_contiguous():
        raise ValueError("se_apply: gate must be a contiguous fp32 [N,C] tensor")
    if residual is not None and (residual.shape != t.shape or residual.dtype != t.dtype or not residual.is_contiguous()):
        raise ValueError("se_apply: residual must be a contiguous tensor of t's shape and dtype")
    if out is None:
        out = torch.empty_like(t)
    elif out.shape != t.shape or out.dtype != t.dtype or not out.is_contiguous():
        raise ValueError("se_apply: out must be a contiguous tensor of t's shape and dtype")
    C.annotate(tag="se_apply %dx%dx%d" % (n, hw, c), bytes=float(t.numel() * (3 if residual is not None else 2)) * 2)
    C.call("dle_se_apply", C.ptr(t), C.ptr(gate), C.ptr(residual), C.ptr(out), n, hw, c, C.dt(t), int(bool(relu)), C.stream())
    return out


# ------------------------------------------------------------------ EfficientNet's MBConv block (csrc/efficientnet.hip)
def dwconv2d_pool_bands(h, w, c, ksize, stride):
    """G of dwconv2d_act_fwd's pool [N, G, C] for an [N, h, w, c] input (host only)."""
    g = C.lib().dle_dwconv2d_pool_bands(int(h), int(w), int(c), int(ksize), int(stride))
    if g < 0:
        raise ValueError("dwconv2d_pool_bands: %s" % C.lib().dle_last_error().decode("utf-8", "replace"))
    return g


def dwconv2d_act_fwd(x, w, scale, shift, stride=1, in_act=False, out_act=False, pool=False, out=None):
    """Depthwise k x k (k 3 or 5, pad k // 2, stride 1 or 2) inference unit in one launch:
        y = round16(silu?(scale[c] * dwconv(a, w) + shift[c])),  a = round16(silu(x)) with in_act, x without.
    x [N,H,W,C] 16-bit contiguous (C % 8 == 0), w [k,k,C] of x's dtype (pack_depthwise_weight), scale / shift fp32 [C].
    pool: False -> returns y [N,P,Q,C]; True or a contiguous fp32 [N,G,C] tensor (G = dwconv2d_pool_bands) -> returns (y, pool), pool
    holding the per-tile fp32 sums of the rounded y that se_gate_act folds.  Anything outside the envelope raises ValueError."""
    name = "dwconv2d_act_fwd"
    if x.dim() != 4 or w.dim() != 3:
        raise ValueError("%s: x must be [N,H,W,C] and w [k,k,C]" % name)
    n, h, wd, c = x.shape
    k = w.shape[0]
    if x.dtype not in _FP16:
        raise ValueError("%s: 16-bit activations and weights only (got %s)" % (name, x.dtype))
    if c < 8 or c % 8:
        raise ValueError("%s: C must be a multiple of 8 (got %d)" % (name, c))
    if k not in (3, 5) or tuple(w.shape) != (k, k, c):
        raise ValueError("%s: w must be [k,k,C] with k 3 or 5 (got %s)" % (name, tuple(w.shape)))
    if stride not in (1, 2):
        raise ValueError("%s: stride 1 or 2 (got %s)" % (name, stride))
    if w.dtype != x.dtype or not x.is_contiguous() or not w.is_contiguous() or h < 1 or wd < 1:
        raise ValueError("%s: x must be NHWC-contiguous and w [k,k,C]-contiguous of x's dtype" % name)
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.numel() != c or not t.is_contiguous():
            raise ValueError("%s: scale / shift must be contiguous fp32 [C]" % name)
    for t, what in ((x, "x"), (w, "w"), (scale, "scale"), (shift, "shift")):
        if t.data_ptr() % 16:
            raise ValueError("%s: %s must be 16-byte aligned" % (name, what))
    p, q = _conv_out(h, wd, k, k, stride, k // 2)
    if out is not None and (tuple(out.shape) != (n, p, q, c) or out.dtype != x.dtype or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("%s: out must be a contiguous, 16-byte aligned [N,P,Q,C] tensor of x's dtype" % name)
    g = dwconv2d_pool_bands(h, wd, c, k, stride)
    want_pool = pool is not False and pool is not None
    if isinstance(pool, torch.Tensor) and (tuple(pool.shape) != (n, g, c) or pool.dtype != torch.float32 or not pool.is_contiguous()
                                           or pool.data_ptr() % 16):
        raise ValueError("%s: pool must be a contiguous, 16-byte aligned fp32 [N,G,C] = %s tensor (got %s %s)"
                         % (name, (n, g, c), pool.dtype, tuple(pool.shape)))
    C.require_cuda(x, w, scale, shift, out, pool if isinstance(pool, torch.Tensor) else None)
    if out is None:
        out = torch.empty((n, p, q, c), dtype=x.dtype, device=x.device)
    if want_pool and not isinstance(pool, torch.Tensor):
        pool = torch.empty((n, g, c), dtype=torch.float32, device=x.device)
    pt = pool if want_pool else None
    C.annotate(flops=2.0 * n * p * q * c * k * k, tag="dwconv %dx%dx%dx%d k%d s%d" % (n, h, wd, c, k, stride),
               bytes=float(x.numel() + w.numel() + out.numel()) * 2 + (pt.numel() * 4 if want_pool else 0))
    C.call("dle_dwconv2d_act_fwd", C.ptr(x), C.ptr(w), C.ptr(out), C.ptr(scale), C.ptr(shift), C.ptr(pt),
           pt.numel() * 4 if want_pool else 0, n, h, wd, c, k, stride, int(bool(in_act)), int(bool(out_act)), C.dt(x), C.stream())
    return (out, pt) if want_pool else out


SE_GATE_ACT_MAX_C_PLUS_S = 16384          # DLE_SE_GATE_ACT_MAX_C_PLUS_S


def se_gate_act(pool, inv_hw, w1, b1, w2, b2, act="silu", out=None):
    """Squeeze-and-excitation gate from pool partials: sigmoid(w2 @ f(w1 @ (inv_hw * sum_g pool[:, g]) + b1) + b2), f = SiLU
    (act "silu") or ReLU ("relu"), all in fp32.  pool [N,G,C] (dwconv2d_act_fwd) or [N,C]; w1 [S,C], b1 [S], w2 [C,S], b2 [C]
    contiguous fp32, any S >= 1 with C + S <= 16384 -> gate [N,C] fp32."""
    name = "se_gate_act"
    if act not in ("silu", "relu"):
        raise ValueError("%s: act must be 'silu' or 'relu' (got %r)" % (name, act))
    if pool.dim() not in (2, 3) or pool.dtype != torch.float32 or not pool.is_contiguous():
        raise ValueError("%s: pool must be a contiguous fp32 [N,G,C] or [N,C] tensor" % name)
    n, c = pool.shape[0], pool.shape[-1]
    g = pool.shape[1] if pool.dim() == 3 else 1
    if c < 8 or c % 8 or g < 1:
        raise ValueError("%s: C must be a multiple of 8 and G >= 1 (got C %d, G %d)" % (name, c, g))
    s = w1.shape[0] if w1.dim() == 2 else 0
    for v, shape in ((w1, (s, c)), (b1, (s,)), (w2, (c, s)), (b2, (c,))):
        if v.dtype != torch.float32 or tuple(v.shape) != shape or not v.is_contiguous() or s < 1:
            raise ValueError("%s: weights must be contiguous fp32 w1 [S,C], b1 [S], w2 [C,S], b2 [C]" % name)
    if c + s > SE_GATE_ACT_MAX_C_PLUS_S:
        raise ValueError("%s: C + S = %d: the mean and the hidden vector live in LDS, C + S <= %d" % (name, c + s, SE_GATE_ACT_MAX_C_PLUS_S))
    if out is not None and (tuple(out.shape) != (n, c) or out.dtype != torch.float32 or not out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous fp32 [N,C] tensor" % name)
    C.require_cuda(pool, w1, b1, w2, b2, out)
    if out is None:
        out = torch.empty((n, c), dtype=torch.float32, device=pool.device)
    C.call("dle_se_gate_act", C.ptr(pool), g, float(inv_hw), C.ptr(w1), C.ptr(b1), C.ptr(w2), C.ptr(b2), C.ptr(out), n, c, s,
           1 if act == "silu" else 0, C.stream())
    return out


def silu_avgpool_fwd(x, out=None):
    """y[n,c] = round16(mean_hw round16(silu(x[n,hw,c]))), the fp32 sum in a fixed order.  x [N,H,W,C] or [N,HW,C] 16-bit contiguous
    (C % 8 == 0) -> y [N,C] of x's dtype."""
    name = "silu_avgpool_fwd"
    if x.dim() not in (3, 4) or not x.is_contiguous() or x.dtype not in _FP16:
        raise ValueError("%s: x must be a contiguous 16-bit [N,H,W,C] or [N,HW,C] tensor" % name)
    n, c = x.shape[0], x.shape[-1]
    if c < 8 or c % 8:
        raise ValueError("%s: C must be a multiple of 8 (got %d)" % (name, c))
    hw = x.numel() // max(n * c, 1)
    if hw < 1 or x.data_ptr() % 16:
        raise ValueError("%s: x must hold at least one pixel and be 16-byte aligned" % name)
    if out is not None and (tuple(out.shape) != (n, c) or out.dtype != x.dtype or not out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous [N,C] tensor of x's dtype" % name)
    C.require_cuda(x, out)
    if out is None:
        out = torch.empty((n, c), dtype=x.dtype, device=x.device)
    C.call("dle_silu_avgpool_fwd", C.ptr(x), C.ptr(out), n, hw, c, C.dt(x), C.stream())
    return out


# ------------------------------------------------------------------ SSD300 detection post-processing (csrc/ssd.hip)
SSD_MAX_MAPS, SSD_MAX_KEEP, SSD_MAX_BOXES = 8, 256, 16384          # DLE_SSD_MAX_MAPS / _KEEP / _BOXES


def ssd_decode(heads, geom, dboxes_xywh, num_labels, scale_xy=0.1, scale_wh=0.2):
    """Head outputs -> (boxes [N,B,4] fp32 ltrb, probs [N,L,B] fp32 softmax, class-major).  heads: one contiguous 16-bit NHWC tensor
    [N, fs, fs, pitch] per feature map; geom: per map (nd, loc, conf) -- channels [loc, loc + 4 nd) are the location part and
    [conf, conf + L nd) the confidence part, laid out as the reference's NCHW heads (channel c = coordinate or label c // nd of
    anchor c % nd; box index a*fs*fs + h*fs + w inside the map).  dboxes_xywh: contiguous fp32 [B,4]."""
    name = "ssd_decode"
    if not 1 <= len(heads) <= SSD_MAX_MAPS or len(geom) != len(heads):
        raise ValueError("%s: 1..%d feature maps with one (nd, loc, conf) each" % (name, SSD_MAX_MAPS))
    h0 = heads[0]
    if h0.dtype not in _FP16:
        raise ValueError("%s: 16-bit head outputs only (got %s)" % (name, h0.dtype))
    n, table, b = h0.shape[0], [], 0
    for t, (nd, loc, conf) in zip(heads, geom):
        if t.dim() != 4 or t.shape[0] != n or t.shape[1] != t.shape[2] or t.dtype != h0.dtype or not t.is_contiguous():
            raise ValueError("%s: every head must be a contiguous [N, fs, fs, pitch] tensor of one dtype" % name)
        table += [int(t.shape[1]), int(nd), int(t.shape[3]), int(loc), int(conf)]
        b += int(nd) * int(t.shape[1]) ** 2
    if dboxes_xywh.dtype != torch.float32 or tuple(dboxes_xywh.shape) != (b, 4) or not dboxes_xywh.is_contiguous():
        raise ValueError("%s: dboxes_xywh must be a contiguous fp32 [B,4] = [%d,4] tensor" % (name, b))
    C.require_cuda(dboxes_xywh, *heads)
    boxes = torch.empty((n, b, 4), dtype=torch.float32, device=h0.device)
    probs = torch.empty((n, int(num_labels), b), dtype=torch.float32, device=h0.device)
    ptrs = (ctypes.c_void_p * len(heads))(*[t.data_ptr() for t in heads])
    g = (ctypes.c_int * len(table))(*table)
    C.call("dle_ssd_decode_fwd", ptrs, g, len(heads), C.ptr(dboxes_xywh), C.ptr(boxes), C.ptr(probs), n, b, int(num_labels),
           float(scale_xy), float(scale_wh), C.dt(h0), C.stream())
    return boxes, probs


def _ssd_boxes_probs(name, boxes, probs):
    if boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise ValueError("%s: boxes must be a contiguous fp32 [N,B,4] tensor" % name)
    if probs is not None and (probs.dim() != 3 or probs.dtype != torch.float32 or not probs.is_contiguous()
                              or probs.shape[0] != boxes.shape[0] or probs.shape[2] != boxes.shape[1]):
        raise ValueError("%s: probs must be a contiguous fp32 [N,L,B] tensor" % name)


def ssd_nms(boxes, probs, criteria=0.5, threshold=0.05, max_num=200):
    """Greedy per-class non-maximum suppression, one workgroup per (image, label >= 1).  boxes [N,B,4] fp32 ltrb, probs [N,L,B] fp32
    -> (kept_idx [N,L-1,max_num] int32, best first, -1 past the count; kept_score [N,L-1,max_num] fp32; kept_count [N,L-1] int32).
    Candidates: prob > threshold, the max_num best (ties: lower box index first); a candidate survives a kept one only if
    iou < criteria (a NaN suppresses)."""
    name = "ssd_nms"
    _ssd_boxes_probs(name, boxes, probs)
    n, l, b = probs.shape
    C.require_cuda(boxes, probs)
    max_num = int(max_num)
    m = max(max_num, 1)
    kept_idx = torch.empty((n, max(l - 1, 0), m), dtype=torch.int32, device=boxes.device)
    kept_score = torch.empty((n, max(l - 1, 0), m), dtype=torch.float32, device=boxes.device)
    kept_count = torch.empty((n, max(l - 1, 0)), dtype=torch.int32, device=boxes.device)
    C.call("dle_ssd_nms_fwd", C.ptr(boxes), C.ptr(probs), C.ptr(kept_idx), C.ptr(kept_score), C.ptr(kept_count), n, b, l,
           float(threshold), float(criteria), max_num, C.stream())
    return kept_idx, kept_score, kept_count


def ssd_select(boxes, kept_idx, kept_score, kept_count, max_output=200):
    """The max_output best of an image's kept candidates, best first (ties: lower label, then lower box index)
    -> (det_boxes [N,max_output,4] fp32, det_label [N,max_output] int32 (1..L-1), det_score fp32, det_idx int32 (the default-box
    index), det_count [N] int32); rows past the count are zero."""
    name = "ssd_select"
    _ssd_boxes_probs(name, boxes, None)
    n, b = boxes.shape[:2]
    if (kept_idx.dim() != 3 or kept_idx.dtype != torch.int32 or kept_score.dtype != torch.float32 or kept_idx.shape != kept_score.shape
            or kept_count.dtype != torch.int32 or tuple(kept_count.shape) != tuple(kept_idx.shape[:2]) or kept_idx.shape[0] != n
            or not (kept_idx.is_contiguous() and kept_score.is_contiguous() and kept_count.is_contiguous())):
        raise ValueError("%s: kept_idx int32 / kept_score fp32 [N,L-1,max_num] and kept_count int32 [N,L-1], contiguous (ssd_nms)" % name)
    C.require_cuda(boxes, kept_idx, kept_score, kept_count)
    lm1, max_num = kept_idx.shape[1:]
    max_output = int(max_output)
    m = max(max_output, 1)
    dev = boxes.device
    det_boxes = torch.empty((n, m, 4), dtype=torch.float32, device=dev)
    det_label = torch.empty((n, m), dtype=torch.int32, device=dev)
    det_score = torch.empty((n, m), dtype=torch.float32, device=dev)
    det_idx = torch.empty((n, m), dtype=torch.int32, device=dev)
    det_count = torch.empty((n,), dtype=torch.int32, device=dev)
    C.call("dle_ssd_select_fwd", C.ptr(boxes), C.ptr(kept_idx), C.ptr(kept_score), C.ptr(kept_count), C.ptr(det_boxes),
           C.ptr(det_label), C.ptr(det_score), C.ptr(det_idx), C.ptr(det_count), n, b, lm1 + 1, max_num, max_output, C.stream())
    return det_boxes, det_label, det_score, det_idx, det_count


def conv2d_dgrad(dy, w, in_hw, stride=1, pad=0, addend=None, out=None):
    """dy [N,P,Q,Ko], w [Ko,R,S,C] -> dx [N,H,W,C] (+ addend)."""
    C.require_cuda(dy, w, addend, out)
    n, p, q, ko = dy.shape
    ko2, r, s, c = w.shape
    h, wd = in_hw
    if ko2 != ko or not dy.is_contiguous() or not w.is_contiguous() or (p, q) != _conv_out(h, wd, r, s, stride, pad):
        raise ValueError("conv2d_dgrad: shape mismatch")
    if out is None:
        out = torch.empty((n, h, wd, c), dtype=dy.dtype, device=dy.device)
    if addend is not None and (addend.shape != out.shape or not addend.is_contiguous() or addend.dtype != dy.dtype):
        raise ValueError("conv2d_dgrad: addend must match dx")
    if r == 1 and s == 1 and pad == 0 and stride > 1 and addend is None and c % 8 == 0:
        # 1x1 stride-s (downsample branch): plain GEMM on the P x Q grid, then zero-stuffing -- the gather form would
        # run 1 - 1/s^2 of its tiles on rows that are identically zero
        m = n * p * q
        compact = gemm(dy.view(m, ko), w.view(ko, c), m, c, ko, True, False)
        C.annotate(bytes=float(out.numel() + compact.numel()) * 2, tag="N%dx%dx%dxC%d s%d" % (n, h, wd, c, stride))
        C.call("dle_upsample_zero", C.ptr(compact), C.ptr(out), n, p, q, h, wd, c, stride, C.dt(dy), C.stream())
        return out
    C.annotate(flops=2.0 * n * p * q * ko * r * s * c, tag="dgrad %dx%dx%dx%d k%d %dx%d s%d" % (n, h, wd, c, ko, r, s, stride),
               bytes=float(dy.numel() + w.numel() + out.numel()) * 2)
    if (r == 3 and s == 3 and stride == 2 and pad == 1 and addend is None and h % 2 == 0 and wd % 2 == 0
            and ko % 64 == 0 and c % 8 == 0):
        # four parity-class correlations with 1 + 2 + 2 + 4 taps instead of 9 taps over 3/4 zeros
        ws = splitk_workspace(dy.device, 9 * ko * c * 2)
        C.call("dle_conv2d_dgrad_s2", C.ptr(dy), C.ptr(w), C.ptr(out), n, h, wd, c, ko, C.ptr(ws), ws.numel() * 4,
               C.dt(dy), C.stream())
        return out
    C.call("dle_conv2d_dgrad", C.ptr(dy), C.ptr(w), C.ptr(out), C.ptr(addend), n, h, wd, c, ko, r, s, stride, pad,
           C.dt(dy), C.stream())
    return out


def upsample_zero(compact, in_hw, stride):
    """compact [N,P,Q,C] -> [N,H,W,C] with compact at the pixels (stride * i, stride * j) and zeros elsewhere."""
    C.require_cuda(compact)
    n, p, q, c = compact.shape
    h, wd = in_hw
    out = torch.empty((n, h, wd, c), dtype=compact.dtype, device=compact.device)
    C.annotate(bytes=float(out.numel() + compact.numel()) * 2, tag="N%dx%dx%dxC%d s%d" % (n, h, wd, c, stride))
    C.call("dle_upsample_zero", C.ptr(compact), C.ptr(out), n, p, q, h, wd, c, stride, C.dt(compact), C.stream())
    return out


def _timed_optional(name, fn, args, replayable=True):
    """A C-ABI call that may DECLINE (return 0) cannot go through C.call (which raises on non-zero): run it, and when bench.py's
    kernel timer is installed record it like C.call does (event pair on the launch stream, replayable) if it launched.  -> rc
    replayable=False: the launch ADDS into a live buffer (an accumulating bias-gradient / weight-gradient epilogue): it is
    timed, but KernelTimer.replay must never re-launch it."""
    tm = C._timer
    if tm is None:
        return fn(*args)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn(*args)
    e.record()
    meta, tm.meta = tm.meta, None
    if rc == 1:
        tm.records.append((name, s, e, meta))
        if replayable:
            tm.last[(name, meta.get("tag") if meta else None)] = (fn, args, torch.cuda.current_stream())
    return rc


def conv1x1_s2_dgrad_compact(dy, w):
    """The data gradient of a 1x1 stride-2 convolution ON ITS OWN GRID: dy [N,P,Q,Ko], w [Ko,1,1,C] -> [N,P,Q,C] (the non-zero
    pixels of dx; conv2d_dgrad zero-stuffs it to [N,2P,2Q,C], gemm_add_upsampled2 adds it without materialising that)."""
    n, p, q, ko = dy.shape
    c = w.shape[-1]
    m = n * p * q
    return gemm(dy.view(m, ko), w.view(ko, c), m, c, ko, True, False).view(n, p, q, c)


def gemm_add_upsampled2(a, b, compact, hw):
    """out [M, N] = a [M, K] @ b [K, N] + zero_stuffed(compact [n, H/2, W/2, N]) for M = n*H*W rows (the bottleneck's conv1 data
    gradient + the stride-2 downsample branch's, csrc/gemm_expand.hip).  Returns None when the shape is outside the streaming
    kernel's envelope (the caller materialises the zero-stuffed tensor instead)."""
    C.require_cuda(a, b, compact)
    m, k = a.shape
    k2, nn = b.shape
    h, wd = hw
    if k2 != k or a.stride(1) != 1 or b.stride(1) != 1 or not compact.is_contiguous() or compact.shape[-1] != nn or \
            a.dtype != b.dtype or compact.dtype != a.dtype:
        raise ValueError("gemm_add_upsampled2: shape / layout mismatch")
    out = torch.empty((m, nn), dtype=a.dtype, device=a.device)
    C.annotate(flops=2.0 * m * nn * k, tag="%dx%dx%d+up2" % (m, nn, k), bytes=float(a.numel() + b.numel() + out.numel() + compact.numel()) * 2)
    rc = _timed_optional("dle_gemm", C.lib().dle_gemm_expand_add_up2,
                         (C.ptr(a), C.ptr(b), C.ptr(out), C.ptr(compact), m, nn, k, a.stride(0), b.stride(0), nn, nn, 0, h, wd, C.dt(a),
                          C.stream()))
    if rc == 0:
        return None
    if rc != 1:
        C.check(rc - 1000 if rc > 1000 else rc, "dle_gemm_expand_add_up2")
    return out


def wgrad1x1(dy2d, x2d, out, accumulate=False):
    """out [Ko, C] fp32 (+)= dy2d [M, Ko]^T x2d [M, C] on the streaming weight-gradient kernel (csrc/wgrad1x1.hip).  Returns False
    when the shape is outside its envelope (the caller then uses gemm() with split-K)."""
    C.require_cuda(dy2d, x2d, out)
    m, ko = dy2d.shape
    c = x2d.shape[1]
    if x2d.shape[0] != m or not dy2d.is_contiguous() or not x2d.is_contiguous() or not out.is_contiguous() or \
            out.numel() != ko * c or out.dtype != torch.float32 or dy2d.dtype != x2d.dtype:
        return False
    need = int(C.lib().dle_wgrad1x1_workspace_for(m, ko, c))     # 0: outside the envelope -- no 64 MB scratch for a declined shape
    if need == 0:
        return False
    ws = splitk_workspace(dy2d.device, need)
    C.annotate(flops=2.0 * m * ko * c, tag="%dx%dx%d" % (ko, c, m), bytes=float(dy2d.numel() + x2d.numel()) * 2 + out.numel() * 4.0)
    # (recorded in the family of the split-K GEMM it replaces: the 1x1 gradients)
    rc = _timed_optional("dle_gemm", C.lib().dle_wgrad1x1_try,
                         (C.ptr(dy2d), C.ptr(x2d), C.ptr(out), m, ko, c, C.dt(dy2d), int(accumulate), C.ptr(ws), ws.numel() * 4, C.stream()),
                         replayable=not accumulate)
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_wgrad1x1_try")
    return rc == 1


def conv2d_wgrad(dy, x, rs, stride=1, pad=0, out=None, accumulate=False, splitk=None):
    """dy [N,P,Q,Ko], x [N,H,W,C] -> dw [Ko,R,S,C] fp32."""
    C.require_cuda(dy, x, out)
    n, p, q, ko = dy.shape
    n2, h, wd, c = x.shape
    r, s = rs
    if n2 != n or not dy.is_contiguous() or not x.is_contiguous() or (p, q) != _conv_out(h, wd, r, s, stride, pad):
        raise ValueError("conv2d_wgrad: shape mismatch")
    if out is None:
        out = torch.empty((ko, r, s, c), dtype=torch.float32, device=x.device)
        accumulate = False
    m_out, n_out, k = ko, r * s * c, n * p * q
    if splitk is None:
        splitk = pick_splitk(m_out, n_out, k, target_blocks=1024)
    need = splitk * m_out * n_out * 4 if splitk > 1 else 0
    if (r, s, stride, pad) == (3, 3, 1, 1):                 # the halo-tile kernel's partial blocks (csrc/conv3x3_wgrad.hip)
        need = max(need, int(C.lib().dle_conv3x3_wgrad_workspace()))
    ws = splitk_workspace(x.device, need) if need else None
    C.annotate(flops=2.0 * n * p * q * ko * r * s * c, tag="wgrad %dx%dx%dx%d k%d %dx%d s%d" % (n, h, wd, c, ko, r, s, stride),
               bytes=float(dy.numel() + x.numel()) * 2 + out.numel() * 4.0)
    C.call("dle_conv2d_wgrad", C.ptr(dy), C.ptr(x), C.ptr(out), n, h, wd, c, ko, r, s, stride, pad, C.dt(x), splitk,
           int(accumulate), C.ptr(ws), ws.numel() * 4 if ws is not None else 0, C.stream())
    return out


# ------------------------------------------------------------------ ResNet HBM-bound ops (NHWC, 16-bit)
def nchw_to_nhwc(x, out_dtype, c_padded=None):
    """fp32 [N,C,H,W] -> 16-bit [N,H,W,Cp] with zero-filled padding channels."""
    C.require_cuda(x)
    if x.dtype != torch.float32 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError("nchw_to_nhwc expects a contiguous fp32 NCHW tensor")
    n, c, h, w = x.shape
    cp = c_padded or (c + 7) // 8 * 8
    y = torch.empty((n, h, w, cp), dtype=out_dtype, device=x.device)
    C.call("dle_nchw_to_nhwc", C.ptr(x), C.ptr(y), n, c, h * w, cp, C.dt(y), C.stream())
    return y


def u8_nchw_normalize_nhwc(x, mean, std, out_dtype, c_padded=None):
    """uint8 [N,C,H,W] -> ((x - mean[c]) / std[c]) as 16-bit [N,H,W,Cp] (PrefetchedWrapper's normalisation + layout)."""
    C.require_cuda(x, mean, std)
    if x.dtype != torch.uint8 or x.dim() != 4 or not x.is_contiguous():
        raise ValueError("u8_nchw_normalize_nhwc expects a contiguous uint8 NCHW tensor")
    n, c, h, w = x.shape
    cp = c_padded or (c + 7) // 8 * 8
    y = torch.empty((n, h, w, cp), dtype=out_dtype, device=x.device)
    C.call("dle_u8_nchw_normalize_nhwc", C.ptr(x), C.ptr(y), C.ptr(mean), C.ptr(std), n, c, h * w, cp, C.dt(y), C.stream())
    return y


def _bn_ws(x2d):
    m, c = x2d.shape
    nbytes = C.lib().dle_bn_workspace_bytes(m, c)
    return splitk_workspace(x2d.device, nbytes)


def bn_fwd(x, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, residual=None, relu=True,
           out=None, want_mask=False):
    """Training-mode BatchNorm over the leading dims of NHWC x (+ residual, + ReLU).  -> (y, mean, rstd) or, with
    want_mask (and relu), (y, mean, rstd, relu_mask): the bit-packed y > 0 mask the backward pass reads instead of y."""
    C.require_cuda(x, gamma, beta, running_mean, running_var, residual, out)
    c = x.shape[-1]
    m = x.numel() // c
    x2 = x.reshape(m, c)
    mean = torch.empty(c, dtype=torch.float32, device=x.device)
    rstd = torch.empty(c, dtype=torch.float32, device=x.device)
    ws = _bn_ws(x2)
    C.annotate(bytes=float(x.numel()) * 2, tag="M%dxC%d" % (x.numel() // c, c))
    C.call("dle_bn_fwd_stats", C.ptr(x), m, c, eps, momentum, C.ptr(mean), C.ptr(rstd), C.ptr(running_mean),
           C.ptr(running_var), C.ptr(ws), ws.numel() * 4, C.dt(x), C.stream())
    y = torch.empty_like(x) if out is None else out
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) if (want_mask and relu) else None
    C.annotate(bytes=float(x.numel()) * (2 * (3 if residual is not None else 2) + (0.125 if mask is not None else 0)),
               tag="M%dxC%d%s" % (x.numel() // c, c, "+res" if residual is not None else ""))
    C.call("dle_bn_fwd_apply", C.ptr(x), C.ptr(residual), C.ptr(y), C.ptr(mask), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
           C.ptr(beta), m, c, int(relu), C.dt(x), C.stream())
    if want_mask:
        return y, mean, rstd, mask
    return y, mean, rstd


def conv2d_fwd_bnstats(x, w, stride=1, pad=0, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """conv (no bias / activation) + the training-mode BatchNorm statistics of its output in ONE pass over the
    activation: the convolution epilogue leaves per-tile column sums, a tiny deterministic fold turns them into
    mean / rstd / running stats.  x [N,H,W,C], w [Ko,R,S,C] -> (y [N,P,Q,Ko], mean [Ko], rstd [Ko])."""
    C.require_cuda(x, w, running_mean, running_var)
    n, h, wd, c = x.shape
    ko, r, s, c2 = w.shape
    if c2 != c or not x.is_contiguous() or not w.is_contiguous() or x.dtype != w.dtype:
        raise ValueError("conv2d_fwd_bnstats: x must be NHWC-contiguous and w KRSC-contiguous with matching C/dtype")
    p, q = _conv_out(h, wd, r, s, stride, pad)
    m = n * p * q
    y = torch.empty((n, p, q, ko), dtype=x.dtype, device=x.device)
    # partial rows: one per 128-row tile, or one per workgroup group of the streaming 1x1 kernel (gemm_expand.hip: at most
    # 1032, at most one per 64 rows rounded up to a multiple of 8); the call reports how many it wrote
    groups = max((m + 127) // 128, min(1032, (m + 63) // 64 + 8))
    ws = splitk_workspace(x.device, (groups + 32) * 2 * ko * 4)
    part, fold = ws[:groups * 2 * ko], ws[groups * 2 * ko:(groups + 32) * 2 * ko]
    import ctypes
    g_out = ctypes.c_int(0)
    C.annotate(flops=2.0 * m * ko * r * s * c, tag="fwd+stats %dx%dx%dx%d k%d %dx%d s%d" % (n, h, wd, c, ko, r, s, stride),
               bytes=float(x.numel() + w.numel() + y.numel()) * 2)
    C.call("dle_conv2d_fwd_colstats", C.ptr(x), C.ptr(w), C.ptr(y), n, h, wd, c, ko, r, s, stride, pad, C.dt(x),
           C.ptr(part), part.numel() * 4, ctypes.byref(g_out), C.stream())
    mean = torch.empty(ko, dtype=torch.float32, device=x.device)
    rstd = torch.empty(ko, dtype=torch.float32, device=x.device)
    C.call("dle_bn_stats_from_partials", C.ptr(part), g_out.value, m, ko, float(eps), float(momentum), C.ptr(mean),
           C.ptr(rstd), C.ptr(running_mean), C.ptr(running_var), C.ptr(fold), fold.numel() * 4, C.stream())
    return y, mean, rstd


def conv1x1_bnload_fwd(t, res, w, mean, rstd, gamma, beta, running_mean=None, running_var=None, eps=1e-5, momentum=0.1, res_bn=None):
    """The producer's BatchNorm-apply (+ residual) + ReLU on the operand load of a 1x1 convolution (csrc/conv_bnload.hip).
    t [.., K] pre-BatchNorm activations, res like t or None, w [N, 1, 1, K]; mean / rstd / gamma / beta: the PRODUCER's BatchNorm;
    running_mean / running_var / eps / momentum: THIS convolution's BatchNorm (its batch statistics come out of the epilogue).
    res_bn = (mean_r, rstd_r, gamma_r, beta_r): `res` is the downsample branch's CONVOLUTION output and its BatchNorm is applied on
    the residual's load (bit-identical to bn_fwd_apply(res, relu=False) in front).
    -> (out [.., N], y [.., K], bits, mean_out, rstd_out), or None when the shape is outside the kernel's envelope."""
    C.require_cuda(t, res, w, mean, rstd, gamma, beta, running_mean, running_var, *(res_bn or ()))
    k = t.shape[-1]
    n = w.shape[0]
    m = t.numel() // k
    if not t.is_contiguous() or not w.is_contiguous() or w.numel() != n * k or w.dtype != t.dtype or \
            (res is not None and (res.shape != t.shape or not res.is_contiguous() or res.dtype != t.dtype)):
        raise ValueError("conv1x1_bnload_fwd: dense operands of one 16-bit dtype expected")
    groups = C.lib().dle_conv1x1_bnload_groups(m, n, k)
    if groups == 0:
        return None
    out = torch.empty(t.shape[:-1] + (n,), dtype=t.dtype, device=t.device)
    y = torch.empty_like(t)
    bits = torch.empty(t.numel() // 8, dtype=torch.uint8, device=t.device)
    ws = splitk_workspace(t.device, (groups + 32) * 2 * n * 4)
    part, fold = ws[:groups * 2 * n], ws[groups * 2 * n:(groups + 32) * 2 * n]
    C.annotate(flops=2.0 * m * n * k, tag="bn+conv %dx%dx%d%s" % (m, n, k, "+res" if res is not None else ""),
               bytes=float(t.numel() * (3 if res is not None else 2) + out.numel() + w.numel()) * 2 + bits.numel())
    if res_bn is not None:
        if res is None:
            raise ValueError("conv1x1_bnload_fwd: res_bn without a residual")
        C.annotate(flops=2.0 * m * n * k, tag="bn+conv %dx%dx%d+bnres" % (m, n, k),
                   bytes=float(t.numel() * 3 + out.numel() + w.numel()) * 2 + bits.numel())
        rc = _timed_optional("dle_conv1x1_bnload_fwd", C.lib().dle_conv1x1_bnload_fwd2,
                             (C.ptr(t), C.ptr(res), C.ptr(w), C.ptr(out), C.ptr(y), C.ptr(bits), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
                              C.ptr(beta), C.ptr(res_bn[0]), C.ptr(res_bn[1]), C.ptr(res_bn[2]), C.ptr(res_bn[3]),
                              C.ptr(part), part.numel() * 4, m, n, k, C.dt(t), C.stream()))
    else:
        rc = _timed_optional("dle_conv1x1_bnload_fwd", C.lib().dle_conv1x1_bnload_fwd,
                             (C.ptr(t), C.ptr(res), C.ptr(w), C.ptr(out), C.ptr(y), C.ptr(bits), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
                              C.ptr(beta), C.ptr(part), part.numel() * 4, m, n, k, C.dt(t), C.stream()))
    if rc == 0:
        return None
    if rc != 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_conv1x1_bnload_fwd")
    mean_o = torch.empty(n, dtype=torch.float32, device=t.device)
    rstd_o = torch.empty(n, dtype=torch.float32, device=t.device)
    C.call("dle_bn_stats_from_partials", C.ptr(part), groups, m, n, float(eps), float(momentum), C.ptr(mean_o), C.ptr(rstd_o),
           C.ptr(running_mean), C.ptr(running_var), C.ptr(fold), fold.numel() * 4, C.stream())
    return out, y, bits, mean_o, rstd_o


# ---- the ResNet stem on its own kernels (csrc/stem.hip): 4-channel image, packed weights
def stem_pack_weight(w_master, out_dtype, out=None):
    """fp32 master of the stem convolution, a channels_last [64, 3, 7, 7] parameter (memory order [64][7][7][3]) -> the packed
    16-bit [64, 7, 8, 4] operand of the stem kernels (tap 7 / channel 3 zero)."""
    C.require_cuda(w_master, out)
    ko, ci, r, s = w_master.shape
    phys = w_master.permute(0, 2, 3, 1)
    if (ko, ci, r, s) != (64, 3, 7, 7) or not phys.is_contiguous() or w_master.dtype != torch.float32:
        raise ValueError("stem_pack_weight expects a channels_last fp32 [64, 3, 7, 7] weight")
    if out is None:
        out = torch.empty((64, 7, 8, 4), dtype=out_dtype, device=w_master.device)
    C.call("dle_stem_pack_weight", C.ptr(w_master), C.ptr(out), C.dt(out), C.stream())
    return out


def stem_conv_fwd(x4, w2, want_stats=True):
    """x4 [N, H, W, 4] 16-bit, w2 packed [64, 7, 8, 4] -> (y [N, P, Q, 64], partial [groups, 2, 64] fp32 or None)."""
    C.require_cuda(x4, w2)
    n, h, wd, c = x4.shape
    if c != 4 or not x4.is_contiguous() or tuple(w2.shape) != (64, 7, 8, 4) or w2.dtype != x4.dtype or not w2.is_contiguous():
        raise ValueError("stem_conv_fwd: x4 must be [N, H, W, 4] and w2 the packed [64, 7, 8, 4] weight of the same dtype")
    p, q = (h - 1) // 2 + 1, (wd - 1) // 2 + 1
    y = torch.empty((n, p, q, 64), dtype=x4.dtype, device=x4.device)
    part = None
    if want_stats:
        groups = C.lib().dle_stem_conv7_groups(n, h)
        part = splitk_workspace(x4.device, (groups + 32) * 2 * 64 * 4)[:(groups + 32) * 2 * 64]
    C.annotate(flops=2.0 * n * p * q * 64 * 147, tag="stem fwd%s %dx%dx%d" % ("+stats" if want_stats else "", n, h, wd),
               bytes=float(x4.numel() + y.numel()) * 2)
    C.call("dle_stem_conv7_fwd", C.ptr(x4), C.ptr(w2), C.ptr(y), C.ptr(part), part.numel() * 4 if part is not None else 0, n, h, wd,
           C.dt(x4), C.stream())
    return y, part


def stem_conv_fwd_bnstats(x4, w2, running_mean=None, running_var=None, eps=1e-5, momentum=0.1):
    """Stem convolution + the training-mode BatchNorm statistics of its output (the contract of conv2d_fwd_bnstats)."""
    y, part = stem_conv_fwd(x4, w2, want_stats=True)
    n, p, q, ko = y.shape
    groups = C.lib().dle_stem_conv7_groups(n, x4.shape[1])
    mean = torch.empty(ko, dtype=torch.float32, device=y.device)
    rstd = torch.empty(ko, dtype=torch.float32, device=y.device)
    fold = part[groups * 2 * ko:]
    C.call("dle_bn_stats_from_partials", C.ptr(part), groups, n * p * q, ko, float(eps), float(momentum), C.ptr(mean),
           C.ptr(rstd), C.ptr(running_mean), C.ptr(running_var), C.ptr(fold), fold.numel() * 4, C.stream())
    return y, mean, rstd


def stem_conv_wgrad(dy, x4, out, accumulate=False):
    """dy [N, P, Q, 64], x4 [N, H, W, 4] -> out: fp32 [64 * 7 * 7 * 3] in the master's KRSC memory order (the flat gradient view of
    the channels_last [64, 3, 7, 7] parameter)."""
    C.require_cuda(dy, x4, out)
    n, h, wd, c = x4.shape
    if c != 4 or not x4.is_contiguous() or not dy.is_contiguous() or dy.shape[0] != n or dy.shape[3] != 64 or \
            out.numel() != 64 * 147 or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("stem_conv_wgrad: shape mismatch")
    ws = splitk_workspace(x4.device, int(C.lib().dle_stem_conv7_wgrad_workspace(n, h)))
    C.annotate(flops=2.0 * dy.numel() * 147, tag="stem wgrad %dx%dx%d" % (n, h, wd), bytes=float(dy.numel() + x4.numel()) * 2)
    C.call("dle_stem_conv7_wgrad", C.ptr(dy), C.ptr(x4), C.ptr(out), C.ptr(ws), ws.numel() * 4, n, h, wd, C.dt(x4), int(accumulate),
           C.stream())
    return out


def bn_fwd_apply(x, mean, rstd, gamma, beta, residual=None, relu=True, want_mask=False, residual_bn=None):
    """y = act((x - mean) * rstd * gamma + beta (+ residual)) with given statistics -> (y, relu_mask or None).
    residual_bn = (mean_r, rstd_r, gamma_r, beta_r): `residual` is the downsample branch's convolution output, its BatchNorm (no
    ReLU) is applied on load (csrc/convnet.hip bn_apply2_pf_kernel; needs relu and want_mask)."""
    C.require_cuda(x, mean, rstd, gamma, beta, residual, *(residual_bn or ()))
    c = x.shape[-1]
    m = x.numel() // c
    y = torch.empty_like(x)
    if residual_bn is not None:
        if residual is None or not relu or not want_mask or residual.shape != x.shape or residual.dtype != x.dtype \
                or not (x.is_contiguous() and residual.is_contiguous()):
            raise ValueError("bn_fwd_apply: residual_bn needs a dense residual of x's shape / dtype, relu and want_mask")
        mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device)
        C.annotate(bytes=float(x.numel()) * (6 + 0.125), tag="M%dxC%d+bnres" % (m, c))
        C.call("dle_bn_fwd_apply2", C.ptr(x), C.ptr(residual), C.ptr(y), C.ptr(mask), C.ptr(mean), C.ptr(rstd), C.ptr(gamma), C.ptr(beta),
               C.ptr(residual_bn[0]), C.ptr(residual_bn[1]), C.ptr(residual_bn[2]), C.ptr(residual_bn[3]), m, c, C.dt(x), C.stream())
        return y, mask
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device) if (want_mask and relu) else None
    C.annotate(bytes=float(x.numel()) * (2 * (3 if residual is not None else 2) + (0.125 if mask is not None else 0)),
               tag="M%dxC%d%s" % (m, c, "+res" if residual is not None else ""))
    C.call("dle_bn_fwd_apply", C.ptr(x), C.ptr(residual), C.ptr(y), C.ptr(mask), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
           C.ptr(beta), m, c, int(relu), C.dt(x), C.stream())
    return y, mask


def bn_relu_maxpool_fwd(t, mean, rstd, gamma, beta):
    """maxpool3x3/2/pad1(relu(bn(t))) in one pass (the ResNet stem) -> (pooled [N,H/2,W/2,C], argmax uint8, relu_mask of the
    never-materialised activation); bit-identical to bn_fwd_apply + maxpool_fwd.  H, W even."""
    C.require_cuda(t, mean, rstd, gamma, beta)
    n, h, w, c = t.shape
    if h % 2 or w % 2 or not t.is_contiguous():
        raise ValueError("bn_relu_maxpool_fwd: contiguous NHWC input with even H, W expected")
    y = torch.empty((n, h // 2, w // 2, c), dtype=t.dtype, device=t.device)
    am = torch.empty((n, h // 2, w // 2, c), dtype=torch.uint8, device=t.device)
    mask = torch.empty(t.numel() // 8, dtype=torch.uint8, device=t.device)
    C.annotate(bytes=float(t.numel() + y.numel()) * 2 + am.numel() + mask.numel(), tag="N%dx%dx%dxC%d" % (n, h, w, c))
    C.call("dle_bn_relu_maxpool_fwd", C.ptr(t), C.ptr(y), C.ptr(am), C.ptr(mask), C.ptr(mean), C.ptr(rstd), C.ptr(gamma), C.ptr(beta),
           n, h, w, c, C.dt(t), C.stream())
    return y, am, mask


def bn_bwd(dy, y, x, mean, rstd, gamma, dgamma, dbeta, want_skip_grad=False, dx_out=None, relu_mask=None, reduce_done=False):
    """-> (dx, g) ; y = saved post-ReLU output or relu_mask = its bit-packed y > 0 mask (both None when the BN had no
    ReLU); g = dy*(y>0) if requested."""
    C.require_cuda(dy, y, x, mean, rstd, gamma, dgamma, dbeta, relu_mask)
    c = x.shape[-1]
    m = x.numel() // c
    ws = _bn_ws(x.reshape(m, c))
    if relu_mask is not None:
        y = None
    act_bytes = 0.125 if relu_mask is not None else (2.0 if y is not None else 0.0)
    relu_tag = "+relu" if (y is not None or relu_mask is not None) else ""
    if not reduce_done:                      # (reduce_done: the producer of dy already left dgamma / dbeta: gemm_masked_add_bnred)
        C.annotate(bytes=float(x.numel()) * (4 + act_bytes), tag="M%dxC%d%s" % (x.numel() // c, c, relu_tag))
        C.call("dle_bn_bwd_reduce", C.ptr(dy), C.ptr(y), C.ptr(relu_mask), C.ptr(x), C.ptr(mean), C.ptr(rstd), C.ptr(dgamma),
               C.ptr(dbeta), m, c, 0, C.ptr(ws), ws.numel() * 4, C.dt(x), C.stream())
    dx = torch.empty_like(x) if dx_out is None else dx_out
    g = torch.empty_like(x) if want_skip_grad else None
    C.annotate(bytes=float(x.numel()) * (6 + act_bytes + 2 * int(want_skip_grad)),
               tag="M%dxC%d%s%s" % (x.numel() // c, c, relu_tag, "+skip" if want_skip_grad else ""))
    C.call("dle_bn_bwd_apply", C.ptr(dy), C.ptr(y), C.ptr(relu_mask), C.ptr(x), C.ptr(dx), C.ptr(g), C.ptr(mean),
           C.ptr(rstd), C.ptr(gamma), C.ptr(dgamma), C.ptr(dbeta), m, c, C.dt(x), C.stream())
    return dx, g


def bn_bwd_reduce2(dy, relu_mask, x1, mean1, rstd1, dgamma1, dbeta1, x2, mean2, rstd2, dgamma2, dbeta2):
    """The backward reduction (dgamma, dbeta) of TWO BatchNorms fed by the same gradient dy under the same keep bits -- bn3 and the
    downsample branch's BatchNorm of a bottleneck's first block -- in one pass over dy and the mask (csrc/convnet.hip
    bn_reduce2_kernel); bit-identical to two bn_bwd reductions.  The callers then run their apply passes with reduce_done=True."""
    C.require_cuda(dy, relu_mask, x1, mean1, rstd1, dgamma1, dbeta1, x2, mean2, rstd2, dgamma2, dbeta2)
    c = x1.shape[-1]
    m = x1.numel() // c
    if x2.shape != x1.shape or dy.shape != x1.shape or not (dy.is_contiguous() and x1.is_contiguous() and x2.is_contiguous()) \
            or x1.dtype != dy.dtype or x2.dtype != dy.dtype:
        raise ValueError("bn_bwd_reduce2: dy, x1, x2 must be dense tensors of one shape / dtype")
    ws = splitk_workspace(x1.device, 2 * int(C.lib().dle_bn_workspace_bytes(m, c)))
    C.annotate(bytes=float(x1.numel()) * (6 + 0.125), tag="M%dxC%d+relu x2" % (m, c))
    C.call("dle_bn_bwd_reduce2", C.ptr(dy), C.ptr(relu_mask), C.ptr(x1), C.ptr(mean1), C.ptr(rstd1), C.ptr(dgamma1), C.ptr(dbeta1),
           C.ptr(x2), C.ptr(mean2), C.ptr(rstd2), C.ptr(dgamma2), C.ptr(dbeta2), m, c, C.ptr(ws), ws.numel() * 4, C.dt(x1), C.stream())


def gemm_masked_add_bnred(g2, w, m, n, k, addend, bits, t2, bits2, mean2, rstd2, dgamma2, dbeta2):
    """dx [m, n] = g2 [m, k] w [k, n] + addend under `bits` (the masked residual gradient, as gemm(act=ACT_ADD_MASKED)) AND the
    backward reduction of the BatchNorm that dx flows into: dgamma2 / dbeta2 (fp32 [n], overwritten) from g = dx under bits2 and
    xhat = (t2 - mean2) rstd2 -- what bn_bwd's first pass computes from a re-read of dx, t2 and the mask.  -> dx, or None outside
    the streaming kernel's envelope (nothing launched: run gemm and let the unit reduce for itself)."""
    C.require_cuda(g2, w, addend, bits, t2, bits2, mean2, rstd2, dgamma2, dbeta2)
    if (g2.dtype not in (torch.float16, torch.bfloat16) or m < 4096 or k not in (64, 128, 256) or n % 128 != 0 or n < 2 * k
            or (k == 256 and os.environ.get("DLE_GEMM_BNRED_K256", "0") != "1")
            or not (g2.is_contiguous() and w.is_contiguous() and addend.is_contiguous() and t2.is_contiguous())
            or t2.numel() != m * n or os.environ.get("DLE_RN50_FUSE_BNRED", "1") == "0"):
        return None
    groups = int(C.lib().dle_gemm_expand_groups(m, n, k))
    if groups <= 0:
        return None
    ws = splitk_workspace(g2.device, groups * 2 * n * 4)
    out = torch.empty((m, n), dtype=g2.dtype, device=g2.device)
    by = float(m) * (k + 3 * n) * g2.element_size() + float(m) * n * 0.25 + float(k) * n * 2
    C.annotate(bytes=by, flops=2.0 * m * n * k, tag="%dx%dx%d+src+aux+bnred" % (m, n, k))
    rc = _timed_optional("dle_gemm", C.lib().dle_gemm_expand_masked_bnred,
                         (C.ptr(g2), C.ptr(w), C.ptr(out), C.ptr(addend), C.ptr(bits), C.ptr(t2), C.ptr(bits2), C.ptr(mean2),
                          C.ptr(rstd2), C.ptr(ws), ws.numel() * 4, m, n, k, g2.stride(0), w.stride(0), out.stride(0), 0, C.dt(g2),
                          C.stream()))
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, "dle_gemm_expand_masked_bnred")
    if rc != 1:
        return None
    C.call("dle_bn_bwd_finish", C.ptr(ws), groups, n, C.ptr(dgamma2), C.ptr(dbeta2), 0, C.stream())
    return out


def _bn_bwd_conv1x1(dy, x, mean, rstd, gamma, dgamma, dbeta, w, relu_mask, reduce_done, bnred, xin=None, gw=None):
    """bn_bwd_conv1x1_dgrad (xin is None) and bn_bwd_conv1x1_dgrad_wgrad (xin, gw given) in one body: they differ in the workspace
    split, the C entry and the unfused continuation.  -> (dt, dx, bnred taken), dt = None in the wgrad form, or None outside the
    kernel's envelope (nothing has been launched then)."""
    wg = xin is not None
    more = (xin, gw) if wg else ()
    C.require_cuda(dy, x, mean, rstd, gamma, dgamma, dbeta, w, relu_mask, *more)
    k = x.shape[-1]
    m = x.numel() // k
    n = w.shape[-1]
    if (m < 4096 or k != 256 or n != 64 or w.numel() != k * n or not all(t.is_contiguous() for t in (dy, x, w) + more)
            or x.dtype not in (torch.float16, torch.bfloat16) or dy.dtype != x.dtype or w.dtype != x.dtype
            or (wg and (xin.numel() != m * n or gw.numel() != k * n or gw.dtype != torch.float32 or xin.dtype != x.dtype))
            or os.environ.get("DLE_CONV_BNBWD", "1") == "0"
            or any(t is not None and t.data_ptr() % 16 for t in (dy, x, w, relu_mask) + more)):   # (a view with a storage offset)
        return None
    ws = _bn_ws(x.reshape(m, k))
    act_bytes = 0.125 if relu_mask is not None else 0.0
    relu_tag = "+relu" if relu_mask is not None else ""
    if not reduce_done:                      # (reduce_done: the producer of dy already left dgamma / dbeta: gemm_masked_add_bnred)
        C.annotate(bytes=float(x.numel()) * (4 + act_bytes), tag="M%dxC%d%s" % (m, k, relu_tag))
        C.call("dle_bn_bwd_reduce", C.ptr(dy), None, C.ptr(relu_mask), C.ptr(x), C.ptr(mean), C.ptr(rstd), C.ptr(dgamma),
               C.ptr(dbeta), m, k, 0, C.ptr(ws), ws.numel() * 4, C.dt(x), C.stream())
    dt = None if wg else torch.empty_like(x)
    dx = torch.empty((m, n), dtype=x.dtype, device=x.device)
    t2 = bits2 = mean2 = rstd2 = part = None
    if bnred is not None and bnred[0].numel() == m * n and bnred[0].is_contiguous() and bnred[1] is not None \
            and os.environ.get("DLE_RN50_FUSE_BNRED", "1") != "0" and os.environ.get("DLE_RN50_FUSE_BNRED2", "1") != "0":
        t2, bits2, mean2, rstd2 = bnred[:4]
    groups = int(C.lib().dle_conv1x1_bnbwd_groups(m)) if wg or t2 is not None else 0
    bnred_tag = "+bnred" if t2 is not None else ""
    if wg:
        name = "dle_conv1x1_bnbwd_dgrad_wgrad"
        wg_bytes = int(C.lib().dle_conv1x1_bnbwd_wgrad_workspace(m, int(t2 is not None)))
        part_bytes = (groups * 2 * n * 4 + 15) // 16 * 16 if t2 is not None else 0
        # ONE request for both: two requests on one stream return the same buffer, and the kernel writes both in one launch
        buf = splitk_workspace(x.device, part_bytes + wg_bytes)
        part = buf[:part_bytes // 4] if t2 is not None else None
        wpart = buf[part_bytes // 4:]
        C.annotate(bytes=float(x.numel()) * (4 + act_bytes) + (dx.numel() + xin.numel()) * 2.0
                   + dx.numel() * (2.125 if t2 is not None else 0.0),
                   flops=4.0 * m * n * k, tag="bn_bwd+dgrad+wgrad %dx%dx%d%s%s" % (m, n, k, relu_tag, bnred_tag))
        args = (C.ptr(dy), C.ptr(x), C.ptr(relu_mask), C.ptr(w), C.ptr(dx), C.ptr(mean), C.ptr(rstd), C.ptr(gamma), C.ptr(dgamma),
                C.ptr(dbeta), C.ptr(t2), C.ptr(bits2), C.ptr(mean2), C.ptr(rstd2), C.ptr(part), part_bytes, C.ptr(xin), C.ptr(gw),
                C.ptr(wpart), wpart.numel() * 4, m, n, k, C.dt(x), C.stream())
    else:
        name = "dle_conv1x1_bnbwd_dgrad"
        if t2 is not None:
            part = splitk_workspace(x.device, groups * 2 * n * 4)
        C.annotate(bytes=float(x.numel()) * (6 + act_bytes) + dx.numel() * (2.0 + (2.125 if t2 is not None else 0.0)),
                   flops=2.0 * m * n * k, tag="bn_bwd+dgrad %dx%dx%d%s%s" % (m, n, k, relu_tag, bnred_tag))
        args = (C.ptr(dy), C.ptr(x), C.ptr(relu_mask), C.ptr(w), C.ptr(dt), C.ptr(dx), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
                C.ptr(dgamma), C.ptr(dbeta), C.ptr(t2), C.ptr(bits2), C.ptr(mean2), C.ptr(rstd2), C.ptr(part),
                part.numel() * 4 if part is not None else 0, m, n, k, C.dt(x), C.stream())
    rc = _timed_optional(name, getattr(C.lib(), name), args)
    if rc > 1:
        C.check(rc - 1000 if rc > 1000 else -1, name)
    if rc != 1:
        # the C side declined (a condition the envelope above cannot see, e.g. its statically cached DLE_CONV_BNBWD pin): the
        # reduction has been launched and dgamma / dbeta are final -- continue HERE with the unfused apply + GEMM (+ weight
        # gradient), so that a caller only ever sees None (nothing launched) or the outputs with taken = False
        dt, _ = bn_bwd(dy, None, x, mean, rstd, gamma, dgamma, dbeta, relu_mask=relu_mask, reduce_done=True, dx_out=dt)
        gemm(dt.view(m, k), w, m, n, k, True, False, out=dx)
        if wg and not wgrad1x1(dt.view(m, k), xin.view(m, n), gw.view(k, n)):
            gemm(dt.view(m, k), xin.view(m, n), k, n, m, False, False, out=gw.view(k, n),
                 splitk=pick_splitk(k, n, m, target_blocks=1024))
        return (None if wg else dt), dx, False
    if t2 is not None:
        C.call("dle_bn_bwd_finish", C.ptr(part), groups, n, C.ptr(bnred[4]), C.ptr(bnred[5]), 0, C.stream())
    return dt, dx, t2 is not None


def bn_bwd_conv1x1_dgrad(dy, x, mean, rstd, gamma, dgamma, dbeta, w, relu_mask=None, reduce_done=False, bnred=None):
    """BatchNorm backward of a conv + BN unit whose convolution is 1x1 / stride 1, with the unit's data gradient in the same
    pass: the reduction (dgamma, dbeta) as in bn_bwd, then ONE kernel that applies the backward on the operand load of
    dx = dt W (csrc/conv_bnbwd.hip).  x: the convolution output [.., K]; w: the 16-bit weight [K, N] (n contiguous).
    bnred = (t2 [.., N], bits2, mean2, rstd2, dgamma2, dbeta2): dx is the gradient that enters a second BatchNorm (bn2 of the
    bottleneck, behind a ReLU with keep bits bits2); its backward reduction is taken from dx in the same kernel and left in
    dgamma2 / dbeta2 (the caller's second unit then skips its own first pass).
    -> (dt, dx [m, N], bnred taken) or None outside the kernel's envelope (nothing has been launched then: run bn_bwd + gemm).
    (When the C side declines AFTER the reduction was launched the unfused apply + GEMM run here: same triple, taken = False.)"""
    return _bn_bwd_conv1x1(dy, x, mean, rstd, gamma, dgamma, dbeta, w, relu_mask, reduce_done, bnred)


def bn_bwd_conv1x1_dgrad_wgrad(dy, x, mean, rstd, gamma, dgamma, dbeta, w, xin, gw, relu_mask=None, reduce_done=False, bnred=None):
    """bn_bwd_conv1x1_dgrad with the convolution's weight gradient in the same kernel and WITHOUT dt: gw [K, N] (fp32, written)
    = dt^T xin, xin [.., N] the unit's saved input.  dt is never written or read back (csrc/conv_bnbwd.hip, WG form); gw and
    bnred's sums are accumulated in the order of wgrad1x1 / bn_bwd_conv1x1_dgrad: the same bits.  Other arguments as
    bn_bwd_conv1x1_dgrad.
    -> (dx [m, N], bnred taken) or None outside the kernel's envelope (nothing has been launched then).
    (When the C side declines AFTER the reduction was launched the unfused apply + GEMM + weight gradient run here: same pair,
    taken = False.)"""
    out = _bn_bwd_conv1x1(dy, x, mean, rstd, gamma, dgamma, dbeta, w, relu_mask, reduce_done, bnred, xin, gw)
    return out and out[1:]


def maxpool_fwd(x, ksize=3, stride=2, pad=1):
    C.require_cuda(x)
    n, h, w, c = x.shape
    p, q = (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1
    y = torch.empty((n, p, q, c), dtype=x.dtype, device=x.device)
    am = torch.empty((n, p, q, c), dtype=torch.uint8, device=x.device)
    C.annotate(bytes=float(x.numel() + y.numel()) * 2 + am.numel())
    C.call("dle_maxpool_fwd", C.ptr(x), C.ptr(y), C.ptr(am), n, h, w, c, ksize, stride, pad, C.dt(x), C.stream())
    return y, am


def maxpool_bwd(dy, argmax, in_hw, ksize=3, stride=2, pad=1):
    C.require_cuda(dy, argmax)
    n, p, q, c = dy.shape
    h, w = in_hw
    dx = torch.empty((n, h, w, c), dtype=dy.dtype, device=dy.device)
    C.annotate(bytes=float(dx.numel() + dy.numel()) * 2 + argmax.numel())
    C.call("dle_maxpool_bwd", C.ptr(dy), C.ptr(argmax), C.ptr(dx), n, h, w, c, ksize, stride, pad, C.dt(dy), C.stream())
    return dx


def pool_bn_bwd(dy, argmax, x, mean, rstd, gamma, dgamma, dbeta, relu_mask):
    """The stem's backward chain MaxPool2d(3, 2, 1) -> ReLU -> BatchNorm in two passes that gather the pooling gradient from dy
    [N, H/2, W/2, C] + argmax themselves (csrc/convnet.hip pool_bn_bwd_kernel): the full-resolution pooling gradient is never
    written.  x [N, H, W, C]: the BatchNorm's input; dgamma / dbeta are written.  -> dz, or None outside the envelope (nothing
    launched: maxpool_bwd + bn_bwd)."""
    C.require_cuda(dy, argmax, x, mean, rstd, gamma, dgamma, dbeta, relu_mask)
    n, h, w, c = x.shape
    if relu_mask is None or dy.shape != (n, h // 2, w // 2, c) or not (dy.is_contiguous() and x.is_contiguous()) or dy.dtype != x.dtype:
        return None
    nbytes = int(C.lib().dle_pool_bn_bwd_workspace_bytes(n, h, w, c))
    if nbytes == 0:
        return None
    ws = splitk_workspace(x.device, nbytes)
    dz = torch.empty_like(x)
    # two passes: (pooled gradient + argmax + x + keep bits) twice, dz once
    C.annotate(bytes=2.0 * (dy.numel() * 3 + x.numel() * 2.125) + x.numel() * 2.0, tag="N%dx%dx%dxC%d" % (n, h, w, c))
    C.call("dle_pool_bn_bwd", C.ptr(dy), C.ptr(argmax), C.ptr(relu_mask), C.ptr(x), C.ptr(dz), C.ptr(mean), C.ptr(rstd), C.ptr(gamma),
           C.ptr(dgamma), C.ptr(dbeta), n, h, w, c, C.ptr(ws), ws.numel() * 4, C.dt(x), C.stream())
    return dz


def avgpool_fwd(x):
    C.require_cuda(x)
    n, h, w, c = x.shape
    y = torch.empty((n, c), dtype=x.dtype, device=x.device)
    C.call("dle_avgpool_fwd", C.ptr(x), C.ptr(y), n, h * w, c, C.dt(x), C.stream())
    return y


def avgpool_bwd(dy, hw):
    C.require_cuda(dy)
    n, c = dy.shape
    h, w = hw
    dx = torch.empty((n, h, w, c), dtype=dy.dtype, device=dy.device)
    C.call("dle_avgpool_bwd", C.ptr(dy), C.ptr(dx), n, h * w, c, C.dt(dy), C.stream())
    return dx


def softmax_xent(logits, target, smoothing=0.0, ignore_index=-100, grad_scale=None, grad_dtype=None, ld_out=None):
    """logits fp32 [rows, classes(+pad)], target int64 [rows] -> (mean loss [1], dlogits or None)."""
    C.require_cuda(logits, target, grad_scale)
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or target.dtype != torch.int64:
        raise ValueError("softmax_xent expects fp32 [rows, classes] logits and int64 targets")
    rows, classes = logits.shape
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    scratch = torch.empty(1, dtype=torch.int32, device=logits.device)
    dl = None
    ldo = ld_out or classes
    if grad_dtype is not None:
        dl = torch.empty((rows, ldo), dtype=grad_dtype, device=logits.device)
    C.call("dle_softmax_xent", C.ptr(logits), C.ptr(target), C.ptr(loss), C.ptr(dl), C.ptr(grad_scale), C.ptr(scratch),
           rows, classes, logits.stride(0), ldo, float(smoothing), int(ignore_index),
           C.dt(grad_dtype) if grad_dtype is not None else 0, C.stream())
    return loss, dl


# ------------------------------------------------------------------ BERT ops (hidden states [tokens, H], 16-bit)
def gemm_batched(a, b, c, m, n, k, lda, ldb, ldc, a_kc, b_kc, batch, batch_inner, sa, sb, sc, alpha=1.0):
    """C[z] = alpha * A[z](m,k) B[z](n,k) for z = (zo, zi); sa/sb/sc = (outer, inner) element strides."""
    C.require_cuda(a, b, c)
    C.annotate(flops=2.0 * m * n * k * batch, tag="b%dx%dx%dx%d" % (batch, m, n, k),
               bytes=float(batch) * (m * k + n * k + m * n) * 2)
    C.call("dle_gemm_batched", C.ptr(a), C.ptr(b), C.ptr(c), m, n, k, lda, ldb, ldc, int(a_kc), int(b_kc), C.dt(a),
           C.dt(c), float(alpha), batch, batch_inner, sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], C.stream())
    return c


def layernorm_fwd(x, gamma, beta, residual=None, eps=1e-12, write_z=True):
    """y = LN(x + residual).  -> (y, z, mean, rstd); z is x itself when there is no residual."""
    C.require_cuda(x, gamma, beta, residual)
    rows, h = x.shape
    y = torch.empty_like(x)
    z = torch.empty_like(x) if (residual is not None and write_z) else None
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    C.annotate(bytes=float(x.numel()) * 2 * (4 if residual is not None else 2), tag="R%dxH%d" % (x.numel() // h, h))
    C.call("dle_layernorm_fwd", C.ptr(x), C.ptr(residual), C.ptr(z), C.ptr(y), C.ptr(gamma), C.ptr(beta), C.ptr(mean),
           C.ptr(rstd), rows, h, float(eps), C.dt(x), C.stream())
    return y, (z if z is not None else x), mean, rstd


def layernorm_bwd(dy, z, mean, rstd, gamma, dgamma, dbeta, accumulate=False):
    C.require_cuda(dy, z, mean, rstd, gamma, dgamma, dbeta)
    rows, h = z.shape
    dz = torch.empty_like(z)
    ws = splitk_workspace(z.device, C.lib().dle_layernorm_workspace_bytes(h))
    C.annotate(bytes=float(z.numel()) * 2 * 3, tag="R%dxH%d" % (rows, h))
    C.call("dle_layernorm_bwd", C.ptr(dy), C.ptr(z), C.ptr(mean), C.ptr(rstd), C.ptr(gamma), C.ptr(dz), C.ptr(dgamma),
           C.ptr(dbeta), rows, h, int(accumulate), C.ptr(ws), ws.numel() * 4, C.dt(z), C.stream())
    return dz


def dropout_add_layernorm_bwd(dy, z, mean, rstd, gamma, mask, p, dgamma, dbeta, dbias=None, accumulate=False):
    """Backward of dropout_add_layernorm_fwd in one pass -> (dz, dx): dz feeds the residual branch, dx = dz * keep / (1 - p)
    the dense layer; dbias (+)= column sums of dx."""
    C.require_cuda(dy, z, mean, rstd, gamma, mask, dgamma, dbeta, dbias)
    rows, h = z.shape
    dz, dx = torch.empty_like(z), torch.empty_like(z)
    ws = splitk_workspace(z.device, C.lib().dle_layernorm_workspace_bytes(h))
    C.annotate(bytes=float(z.numel()) * 2 * 4 + z.numel() / 8, tag="R%dxH%d+drop" % (rows, h))
    C.call("dle_dropout_add_layernorm_bwd", C.ptr(dy), C.ptr(z), C.ptr(mean), C.ptr(rstd), C.ptr(gamma), C.ptr(mask), float(p),
           C.ptr(dz), C.ptr(dx), C.ptr(dgamma), C.ptr(dbeta), C.ptr(dbias), rows, h, int(accumulate), C.ptr(ws),
           ws.numel() * 4, C.dt(z), C.stream())
    return dz, dx


def embed_sum(word, pos, typ, ids, token_type, seq_len, out_dtype):
    C.require_cuda(word, pos, typ, ids, token_type)
    t = ids.numel()
    h = word.shape[1]
    z = torch.empty((t, h), dtype=out_dtype, device=word.device)
    C.call("dle_embed_sum", C.ptr(word), C.ptr(pos), C.ptr(typ), C.ptr(ids), C.ptr(token_type), C.ptr(z), t, seq_len, h,
           C.dt(z), C.stream())
    return z


def embed_sum_packed(word, pos, typ, ids, token_type, position_ids, out_dtype):
    """embed_sum for a packed batch: row t takes position row position_ids[t] (int32 [T]) instead of t mod seq_len."""
    C.require_cuda(word, pos, typ, ids, token_type, position_ids)
    t = ids.numel()
    h = word.shape[1]
    if position_ids.dtype != torch.int32 or position_ids.numel() != t or not position_ids.is_contiguous():
        raise ValueError("embed_sum_packed: position_ids must be a contiguous int32 tensor with one entry per token")
    z = torch.empty((t, h), dtype=out_dtype, device=word.device)
    C.annotate(bytes=float(t) * h * (3 * 4 + 2), tag="T%dxH%d" % (t, h))
    C.call("dle_embed_sum_packed", C.ptr(word), C.ptr(pos), C.ptr(typ), C.ptr(ids), C.ptr(token_type), C.ptr(position_ids),
           C.ptr(z), t, h, C.dt(z), C.stream())
    return z


def embed_scatter_add_(grad_word, dz, ids):
    C.require_cuda(grad_word, dz, ids)
    C.call("dle_embed_scatter_add", C.ptr(dz), C.ptr(ids), C.ptr(grad_word), ids.numel(), dz.shape[1], C.dt(dz), C.stream())


def rows_select_sum(x, sel, k, out, accumulate=False):
    C.require_cuda(x, sel, out)
    rows, h = x.shape
    ws = splitk_workspace(x.device, 128 * k * h * 4)
    C.call("dle_rows_select_sum", C.ptr(x), C.ptr(sel), C.ptr(out), rows, h, k, int(accumulate), C.ptr(ws),
           ws.numel() * 4, C.dt(x), C.stream())
    return out


def rows_gather(src, idx):
    C.require_cuda(src, idx)
    dst = torch.empty((idx.numel(), src.shape[1]), dtype=src.dtype, device=src.device)
    C.call("dle_rows_gather", C.ptr(src), C.ptr(idx), C.ptr(dst), idx.numel(), src.shape[1], C.dt(src), C.stream())
    return dst


def rows_scatter_(dst, src, idx, accumulate=False):
    C.require_cuda(dst, src, idx)
    C.call("dle_rows_scatter", C.ptr(src), C.ptr(idx), C.ptr(dst), idx.numel(), src.shape[1], int(accumulate), C.dt(src),
           C.stream())
    return dst


def softmax_fwd_(scores, mask_add, rows_per_batch, scale):
    """In place over scores [..., L]."""
    C.require_cuda(scores, mask_add)
    l = scores.shape[-1]
    rows = scores.numel() // l
    C.annotate(bytes=float(scores.numel()) * 4, tag="R%dxL%d" % (rows, l))
    C.call("dle_softmax_fwd", C.ptr(scores), C.ptr(mask_add), rows, l, rows_per_batch, float(scale), C.dt(scores), C.stream())
    return scores


def softmax_bwd_(probs, dprobs, scale):
    C.require_cuda(probs, dprobs)
    l = probs.shape[-1]
    rows = probs.numel() // l
    C.annotate(bytes=float(probs.numel()) * 6, tag="R%dxL%d" % (rows, l))
    C.call("dle_softmax_bwd", C.ptr(probs), C.ptr(dprobs), rows, l, float(scale), C.dt(probs), C.stream())
    return dprobs


def act_bwd(g, src, act):
    """g * act'(src): act = C.ACT_GELU_BWD (src = pre-activation) or C.ACT_TANH_BWD (src = tanh output)."""
    C.require_cuda(g, src)
    out = torch.empty_like(g)
    C.call("dle_act_bwd", C.ptr(g), C.ptr(src), C.ptr(out), g.numel(), act, C.dt(g), C.stream())
    return out


# ------------------------------------------------------------------ dropout (BERT training mode)
def dropout_fwd(x, p, seed, offset, offset_base=None):
    """y = dropout(x) with the C-ABI's counter-based RNG.  Returns (y, mask) -- mask is bit-packed uint8 [numel/8].
    offset_base (all dropout wrappers): optional int64 DEVICE tensor [1] added to `offset` by the kernel -- the RNG
    advance of a HIP-graph-captured step lives in device memory."""
    C.require_cuda(x)
    n = x.numel()
    y = torch.empty_like(x)
    mask = torch.empty(n // 8, dtype=torch.uint8, device=x.device)
    C.annotate(bytes=float(n) * 2 * 2 + n / 8, tag="N%d" % n)
    C.call("dle_dropout_fwd", C.ptr(x), C.ptr(y), C.ptr(mask), n, float(p), int(seed), int(offset), C.ptr(offset_base),
           C.dt(x), C.stream())
    return y, mask


def dropout_bwd(dy, mask, p):
    C.require_cuda(dy, mask)
    dx = torch.empty_like(dy)
    n = dy.numel()
    C.annotate(bytes=float(n) * 2 * 2 + n / 8, tag="N%d" % n)
    C.call("dle_dropout_bwd", C.ptr(dy), C.ptr(mask), C.ptr(dx), n, float(p), C.dt(dy), C.stream())
    return dx


def dropout_add_layernorm_fwd(x, gamma, beta, residual, p, seed, offset, eps=1e-12, offset_base=None):
    """y = LayerNorm(dropout(x) + residual).  Returns (y, z, mean, rstd, mask)."""
    C.require_cuda(x, gamma, beta, residual)
    rows, h = x.shape
    y = torch.empty_like(x)
    z = torch.empty_like(x)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    mask = torch.empty(x.numel() // 8, dtype=torch.uint8, device=x.device)
    C.annotate(bytes=float(x.numel()) * 2 * 4 + x.numel() / 8, tag="R%dxH%d+drop" % (rows, h))
    C.call("dle_dropout_add_layernorm_fwd", C.ptr(x), C.ptr(residual), C.ptr(z), C.ptr(y), C.ptr(mask), C.ptr(gamma),
           C.ptr(beta), C.ptr(mean), C.ptr(rstd), rows, h, float(eps), float(p), int(seed), int(offset),
           C.ptr(offset_base), C.dt(x), C.stream())
    return y, z, mean, rstd, mask


def softmax_dropout_fwd_(scores, mask_add, rows_per_batch, scale, p, seed, offset, offset_base=None):
    """scores -> probs in place; returns (dropped = dropout(probs), mask)."""
    C.require_cuda(scores, mask_add)
    l = scores.shape[-1]
    rows = scores.numel() // l
    dropped = torch.empty_like(scores)
    mask = torch.empty(scores.numel() // 8, dtype=torch.uint8, device=scores.device)
    C.annotate(bytes=float(scores.numel()) * 6 + scores.numel() / 8, tag="R%dxL%d+drop" % (rows, l))
    C.call("dle_softmax_dropout_fwd", C.ptr(scores), C.ptr(dropped), C.ptr(mask), C.ptr(mask_add), rows, l,
           rows_per_batch, float(scale), float(p), int(seed), int(offset), C.ptr(offset_base), C.dt(scores), C.stream())
    return dropped, mask


def softmax_dropout_bwd_(probs, dprobs, mask, scale, p):
    C.require_cuda(probs, dprobs, mask)
    l = probs.shape[-1]
    rows = probs.numel() // l
    C.annotate(bytes=float(probs.numel()) * 6 + probs.numel() / 8, tag="R%dxL%d+drop" % (rows, l))
    C.call("dle_softmax_dropout_bwd", C.ptr(probs), C.ptr(dprobs), C.ptr(mask), rows, l, float(scale), float(p),
           C.dt(probs), C.stream())
    return dprobs


def attention_supported(seq_len, head_dim):
    """True when the fused attention kernels cover (seq_len, head_dim); otherwise use the batched-GEMM path."""
    return bool(C.lib().dle_attention_supported(int(seq_len), int(head_dim)))


def attention_fwd(qkv, mask_add, batch, seq_len, heads, scale, p=0.0, seed=0, offset=0, want_mask=False,
                  offset_base=None):
    """context = dropout(softmax(q k^T * scale + mask_add)) v for every (sequence, head) of qkv [T, 3H] in ONE kernel
    (BertSelfAttention.forward, modeling.py:340-384).  -> (ctx [T, H], stats [B*heads, S, 2 or 4] fp32, keep mask or None).
    seq_len 128, or a multiple of 128 up to 1024 (K / V then stream through LDS in 128-key blocks: csrc/attention.hip)."""
    C.require_cuda(qkv, mask_add)
    t, h3 = qkv.shape
    h = h3 // 3
    d = h // heads
    if not qkv.is_contiguous() or t != batch * seq_len or heads * d * 3 != h3:
        raise ValueError("attention_fwd: qkv must be a contiguous [batch * seq_len, 3 * heads * head_dim] tensor")
    ctx = torch.empty((t, h), dtype=qkv.dtype, device=qkv.device)
    stats = torch.empty((batch * heads, seq_len, int(C.lib().dle_attention_stats_floats(int(seq_len)))), dtype=torch.float32,
                        device=qkv.device)
    mask = torch.empty(batch * heads * seq_len * seq_len // 8, dtype=torch.uint8, device=qkv.device) \
        if (want_mask and p > 0) else None
    bh = batch * heads
    C.annotate(flops=4.0 * bh * seq_len * seq_len * d, bytes=float(t) * h * 2 * 4 + stats.numel() * 4,
               tag="B%dxh%dxS%dxd%d" % (batch, heads, seq_len, d))
    C.call("dle_attention_fwd", C.ptr(qkv), C.ptr(mask_add), C.ptr(ctx), C.ptr(stats), C.ptr(mask), batch, seq_len,
           heads, d, float(scale), float(p), int(seed), int(offset), C.ptr(offset_base), C.dt(qkv), C.stream())
    return ctx, stats, mask


def attention_varlen_supported(max_seqlen, head_dim):
    """True when the packed forward attention kernel covers (max_seqlen, head_dim): 64-wide heads, 1 <= max_seqlen <= 1024."""
    return bool(C.lib().dle_attention_varlen_supported(int(max_seqlen), int(head_dim)))


def attention_varlen_launch_count():
    """Launches of the packed attention kernel by this process so far."""
    return int(C.lib().dle_attention_varlen_launch_count())


def attention_fwd_varlen(qkv, cu_seqlens, max_seqlen, heads, scale, out=None):
    """context = softmax(q k^T * scale) v per (sequence, head) of a PACKED qkv [T, 3H]: sequence b owns rows
    cu_seqlens[b] .. cu_seqlens[b + 1] - 1 (int32 device tensor [B + 1], starting at 0; no sequence longer than max_seqlen).
    Inference only: no dropout, no statistics, the length is the mask.  -> ctx [T, H] (`out` when given)."""
    C.require_cuda(qkv, cu_seqlens, out)
    t, h3 = qkv.shape
    h = h3 // 3
    d = h // heads
    if not qkv.is_contiguous() or heads * d * 3 != h3:
        raise ValueError("attention_fwd_varlen: qkv must be a contiguous [T, 3 * heads * head_dim] tensor")
    if cu_seqlens.dtype != torch.int32 or cu_seqlens.dim() != 1 or cu_seqlens.numel() < 2 or not cu_seqlens.is_contiguous():
        raise ValueError("attention_fwd_varlen: cu_seqlens must be a contiguous int32 tensor [B + 1]")
    if out is None:
        out = torch.empty((t, h), dtype=qkv.dtype, device=qkv.device)
    elif out.shape != (t, h) or out.dtype != qkv.dtype or not out.is_contiguous():
        raise ValueError("attention_fwd_varlen: out must be a contiguous [T, H] tensor of qkv's dtype")
    b = cu_seqlens.numel() - 1
    # (upper bound of the work: every sequence at max_seqlen; the real figure needs the lengths on the host)
    C.annotate(flops=6.0 * t * max_seqlen * h, bytes=float(t) * h * 2 * 4, tag="T%dxB%dxh%dxS%dxd%d" % (t, b, heads, max_seqlen, d))
    C.call("dle_attention_fwd_varlen", C.ptr(qkv), C.ptr(cu_seqlens), C.ptr(out), b, int(max_seqlen), t, heads, d, float(scale),
           C.dt(qkv), C.stream())
    return out


def attention_bwd(qkv, dctx, mask_add, stats, batch, seq_len, heads, scale, p=0.0, seed=0, offset=0, offset_base=None,
                  colsum_partial=None, keep_mask=None):
    """dqkv [T, 3H] from dctx [T, H]: probabilities and dropout mask are recomputed from (qkv, stats, seed, offset).
    colsum_partial (optional fp32 [batch * seq_len / 128, 3H]) receives the column sums of dqkv per (sequence, 128-row block): the
    QKV bias gradient partials."""
    C.require_cuda(qkv, dctx, mask_add, stats)
    t, h3 = qkv.shape
    h = h3 // 3
    d = h // heads
    if not qkv.is_contiguous() or not dctx.is_contiguous() or dctx.shape != (t, h):
        raise ValueError("attention_bwd: qkv [T, 3H] and dctx [T, H] must be contiguous")
    dqkv = torch.empty_like(qkv)
    bh = batch * heads
    if colsum_partial is not None and (colsum_partial.numel() != batch * (seq_len // 128) * h3 or colsum_partial.dtype != torch.float32
                                       or not colsum_partial.is_contiguous()):
        raise ValueError("attention_bwd: colsum_partial must be fp32 [batch * seq_len / 128, 3H]")
    C.annotate(flops=10.0 * bh * seq_len * seq_len * d, bytes=float(t) * h * 2 * 7 + stats.numel() * 4,
               tag="B%dxh%dxS%dxd%d" % (batch, heads, seq_len, d))
    C.require_cuda(colsum_partial, keep_mask)
    if keep_mask is not None:
        # the keep mask attention_fwd(want_mask=True) returned: read by the S = 128 kernel instead of re-drawing it (same bits)
        C.call("dle_attention_bwd_keep", C.ptr(qkv), C.ptr(dctx), C.ptr(mask_add), C.ptr(stats), C.ptr(keep_mask), C.ptr(dqkv),
               C.ptr(colsum_partial), batch, seq_len, heads, d, float(scale), float(p), int(seed), int(offset), C.ptr(offset_base),
               C.dt(qkv), C.stream())
        return dqkv
    C.call("dle_attention_bwd", C.ptr(qkv), C.ptr(dctx), C.ptr(mask_add), C.ptr(stats), C.ptr(dqkv), C.ptr(colsum_partial),
           batch, seq_len,
           heads, d, float(scale), float(p), int(seed), int(offset), C.ptr(offset_base), C.dt(qkv), C.stream())
    return dqkv


def unpack_dropout_mask(mask, shape):
    """Bit-packed keep mask -> bool tensor of `shape` (bit k of byte i <-> flat element 8 i + k)."""
    bits = (mask.to(torch.int32).unsqueeze(1) >> torch.arange(8, device=mask.device, dtype=torch.int32)) & 1
    return bits.reshape(shape).bool()


# ------------------------------------------------------------------ HiFi-GAN generator (csrc/hifigan.hip)
def fold_weight_norm(v, g):
    """torch.nn.utils.weight_norm (dim = 0) folded: w = g * v / ||v|| in fp32, the norm over every dimension but 0 (the output
    channel of a Conv1d, the INPUT channel of a ConvTranspose1d).  Host packing: any device, exact fp32 arithmetic of torch."""
    v, g = v.detach().float(), g.detach().float()
    if v.dim() < 2 or g.shape[0] != v.shape[0] or g.numel() != v.shape[0]:
        raise ValueError("fold_weight_norm: v [O, ...] and g [O, 1, ...] expected (got %s, %s)" % (tuple(v.shape), tuple(g.shape)))
    # torch._weight_norm is the function behind torch.nn.utils.weight_norm / remove_weight_norm: v * (g / ||v||), the norm as
    # torch sums it -- a fold written out here differs from a checkpoint saved after remove_weight_norm in the last bit
    return torch._weight_norm(v.contiguous(), g.reshape((v.shape[0],) + (1,) * (v.dim() - 1)).contiguous(), 0)


def pack_conv1d_weight(w, dtype):
    """torch's Conv1d weight [Ko, C, ksize] -> the [Ko, ksize, C] 16-bit tensor conv1d_lrelu_fwd reads (one rounding per element)."""
    if w.dim() != 3:
        raise ValueError("pack_conv1d_weight: expected a [Ko, C, ksize] weight (got %s)" % (tuple(w.shape),))
    if dtype not in (torch.float16, torch.bfloat16, torch.float64):
        raise ValueError("pack_conv1d_weight: dtype must be torch.float16 or torch.bfloat16")
    return w.detach().permute(0, 2, 1).to(dtype).contiguous()


def pack_upsample_weight(w, stride, dtype):
    """ConvTranspose1d(Cin, Cout, k, stride u, padding (k - u) // 2) weight [Cin, Cout, k] -> the [u * Cout, 3, Cin] weight of the
    3-tap, dilation-1 "same" Conv1d that computes it:  packed[p * Cout + ko, j, c] = w[c, ko, (1 - j) * u + p + (k - u) // 2]
    where that index lies in [0, k), 0 elsewhere.  The convolution's [B, T, u * Cout] output is, as it lies in memory, the
    [B, T * u, Cout] tensor of the transposed convolution; its bias is the layer's repeated u times.  k - u even, k <= 2 u.
    dtype torch.float64 keeps the values unrounded (tests)."""
    if w.dim() != 3:
        raise ValueError("pack_upsample_weight: expected a [Cin, Cout, k] weight (got %s)" % (tuple(w.shape),))
    cin, cout, k = w.shape
    u = int(stride)
    if u < 1 or (k - u) % 2 or k > 2 * u or k < u:
        raise ValueError("pack_upsample_weight: needs k - stride even and stride <= k <= 2 stride (got k = %d, stride = %d)" % (k, u))
    if dtype not in (torch.float16, torch.bfloat16, torch.float64):
        raise ValueError("pack_upsample_weight: dtype must be torch.float16 or torch.bfloat16")
    pad = (k - u) // 2
    src = w.detach().to(torch.float64 if dtype == torch.float64 else torch.float32)
    packed = torch.zeros((u, cout, 3, cin), dtype=src.dtype, device=w.device)
    for j in range(3):
        for p in range(u):
            i = (1 - j) * u + p + pad
            if 0 <= i < k:
                packed[p, :, j, :] = src[:, :, i].t()
    return packed.reshape(u * cout, 3, cin).to(dtype).contiguous()


def conv1d_lrelu_fwd(x, w, bias, dilation=1, slope=1.0, alpha=1.0, add1=None, add2=None, out=None):
    """y = ((conv1d_same(leaky_relu(x, slope), w, dilation) + bias (+ add1) (+ add2)) * alpha) in ONE launch, rounded once.
    x [B, T, C] 16-bit channels-last, w [Ko, ksize, C] (pack_conv1d_weight / pack_upsample_weight), bias fp32 [Ko], add1 / add2
    [B, T, Ko] -> y [B, T, Ko].  slope = 1: no activation.  `out` may be add1 or add2 itself, never x.  Anything outside the
    kernel's envelope (include/dle_mi355x.h) raises ValueError."""
    C.require_cuda(x, w, bias, add1, add2, out)
    if x.dtype not in _FP16:
        raise ValueError("conv1d_lrelu_fwd: 16-bit activations and weights only (got %s)" % x.dtype)
    if x.dim() != 3 or w.dim() != 3 or not x.is_contiguous() or not w.is_contiguous() or w.dtype != x.dtype or w.shape[2] != x.shape[2]:
        raise ValueError("conv1d_lrelu_fwd: x must be contiguous [B,T,C] and w contiguous [Ko,ksize,C] of x's dtype")
    b, t, c = x.shape
    ko, ks, _ = w.shape
    if bias.dtype != torch.float32 or bias.numel() != ko or not bias.is_contiguous():
        raise ValueError("conv1d_lrelu_fwd: bias must be contiguous fp32 [Ko]")
    for a in (add1, add2):
        if a is not None and (tuple(a.shape) != (b, t, ko) or a.dtype != x.dtype or not a.is_contiguous()):
            raise ValueError("conv1d_lrelu_fwd: an addend must be a contiguous [B,T,Ko] tensor of x's dtype")
    out = _out_tensor("conv1d_lrelu_fwd", out, (b, t, ko), x.dtype, x.device,
                      text="out must be a contiguous [B,T,Ko] tensor of x's dtype")
    n_add = (add1 is not None) + (add2 is not None)
    C.annotate(flops=2.0 * b * t * ko * ks * c, tag="conv1d %dx%dx%d k%d ks%d d%d +%d" % (b, t, c, ko, ks, dilation, n_add),
               bytes=float(x.numel() + w.numel() + out.numel() * (1 + n_add)) * 2)
    C.call("dle_conv1d_lrelu_fwd", C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(add1), C.ptr(add2), C.ptr(out), b, t, c, ko, ks,
           int(dilation), float(slope), float(alpha), C.dt(x), C.stream())
    return out


def hfg_post_fwd(x, w, bias, slope=0.01, out=None):
    """audio [B, T] fp32 = tanh(conv1d_same(leaky_relu(x, slope), w) + bias): the one-channel output convolution of the HiFi-GAN
    generator.  x [B, T, C] 16-bit (C % 8 == 0, C <= 64), w [ksize, C] of x's dtype, bias fp32 [1]."""
    C.require_cuda(x, w, bias, out)
    if x.dtype not in _FP16:
        raise ValueError("hfg_post_fwd: 16-bit activations and weights only (got %s)" % x.dtype)
    if x.dim() != 3 or w.dim() != 2 or not x.is_contiguous() or not w.is_contiguous() or w.dtype != x.dtype or w.shape[1] != x.shape[2]:
        raise ValueError("hfg_post_fwd: x must be contiguous [B,T,C] and w contiguous [ksize,C] of x's dtype")
    if bias.dtype != torch.float32 or bias.numel() != 1:
        raise ValueError("hfg_post_fwd: bias must be fp32 [1]")
    b, t, c = x.shape
    out = _out_tensor("hfg_post_fwd", out, (b, t), torch.float32, x.device, text="out must be a contiguous fp32 [B,T] tensor")
    C.annotate(flops=2.0 * b * t * w.numel(), tag="hfg_post %dx%dx%d ks%d" % (b, t, c, w.shape[0]),
               bytes=float(x.numel()) * 2 + out.numel() * 4)
    C.call("dle_hfg_post_fwd", C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(out), b, t, c, w.shape[0], float(slope), C.dt(x), C.stream())
    return out


# ------------------------------------------------------------------ packed utterances: the validators every wrapper below shares
_FP16 = (torch.float16, torch.bfloat16)


def _cu_table(name, cu, what="cu_seqlens"):
    if cu is None or cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 2 or not cu.is_contiguous():
        raise ValueError("%s: %s must be a contiguous int32 tensor [B + 1]" % (name, what))
    return cu.numel() - 1


def _f32_tensor(name, t, shape, what):
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s: %s must be contiguous fp32 %s" % (name, what, list(shape)))


def _out_tensor(name, out, shape, dtype, device, what="out", text=None):
    """`text`: the wrapper's own wording of the complaint (the HiFi-GAN wrappers name shapes by letter)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or not out.is_contiguous():
        raise ValueError("%s: %s" % (name, text or "%s must be a contiguous %s tensor %s" % (what, dtype, list(shape))))
    return out


# ------------------------------------------------------------------ FastPitch on packed utterances (csrc/fastpitch.hip)
def conv1d_packed_fwd(x, w, bias, cu_seqlens, max_len, slope=1.0, add1=None, out=None):
    """y = conv1d_same(act(x), w) + bias (+ add1) per SEQUENCE of a packed x [total, C] (16-bit, channels-last; sequence b owns rows
    cu_seqlens[b] .. cu_seqlens[b + 1] - 1; rows outside a row's own sequence read as zero), one launch, one rounding.  w [Ko, ksize, C]
    (pack_conv1d_weight), bias fp32 [Ko], add1 [total, Ko] or None.  slope 1: no activation; slope 0: ReLU on the input.  `out` may
    be add1 itself, never x.  Anything outside the kernel's envelope (include/dle_mi355x.h) raises ValueError."""
    C.require_cuda(x, w, bias, cu_seqlens, add1, out)
    name = "conv1d_packed_fwd"
    if x.dtype not in _FP16:
        raise ValueError("%s: 16-bit activations and weights only (got %s)" % (name, x.dtype))
    if x.dim() != 2 or w.dim() != 3 or not x.is_contiguous() or not w.is_contiguous() or w.dtype != x.dtype or w.shape[2] != x.shape[1]:
        raise ValueError("%s: x must be contiguous [total,C] and w contiguous [Ko,ksize,C] of x's dtype" % name)
    total, c = x.shape
    ko, ks, _ = w.shape
    b = _cu_table(name, cu_seqlens)
    _f32_tensor(name, bias, (ko,), "bias")
    if add1 is not None and (tuple(add1.shape) != (total, ko) or add1.dtype != x.dtype or not add1.is_contiguous()):
        raise ValueError("%s: add1 must be a contiguous [total,Ko] tensor of x's dtype" % name)
    out = _out_tensor(name, out, (total, ko), x.dtype, x.device)
    C.annotate(flops=2.0 * total * ko * ks * c, tag="conv1d_packed %dx%d k%d ks%d B%d" % (total, c, ko, ks, b),
               bytes=float(x.numel() + w.numel() + out.numel() * (2 if add1 is not None else 1)) * 2)
    C.call("dle_conv1d_packed_fwd", C.ptr(x), C.ptr(w), C.ptr(bias), C.ptr(add1), C.ptr(out), C.ptr(cu_seqlens), b, int(max_len),
           total, c, ko, ks, float(slope), C.dt(x), C.stream())
    return out


def fp_relu_layernorm_fwd(x, gamma, beta, eps=1e-5, fc_w=None, fc_b=None, want_y=True, out=None, pred_out=None):
    """y = LayerNorm(relu(x)) * gamma + beta on rows of x [rows, H] (16-bit), and -- with fc_w fp32 [n_pred, H], fc_b fp32 [n_pred] --
    pred = y_rounded @ fc_w^T + fc_b as fp32 [rows, n_pred].  -> (y or None when want_y is False, pred or None)."""
    C.require_cuda(x, gamma, beta, fc_w, fc_b, out, pred_out)
    name = "fp_relu_layernorm_fwd"
    if x.dtype not in _FP16 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("%s: x must be a contiguous 16-bit [rows, H] tensor" % name)
    rows, h = x.shape
    _f32_tensor(name, gamma, (h,), "gamma")
    _f32_tensor(name, beta, (h,), "beta")
    n_pred = 0
    if (fc_w is None) != (fc_b is None):
        raise ValueError("%s: fc_w and fc_b come together" % name)
    if fc_w is not None:
        if fc_w.dim() != 2:
            raise ValueError("%s: fc_w must be fp32 [n_pred, H]" % name)
        n_pred = fc_w.shape[0]
        _f32_tensor(name, fc_w, (n_pred, h), "fc_w")
        _f32_tensor(name, fc_b, (n_pred,), "fc_b")
    if not want_y and not n_pred:
        raise ValueError("%s: neither y nor pred is wanted" % name)
    y = _out_tensor(name, out, (rows, h), x.dtype, x.device) if want_y else None
    pred = _out_tensor(name, pred_out, (rows, n_pred), torch.float32, x.device, "pred_out") if n_pred else None
    C.annotate(bytes=float(x.numel()) * 2 * (2 if want_y else 1), tag="relu_ln R%dxH%d p%d" % (rows, h, n_pred))
    C.call("dle_fp_relu_layernorm_fwd", C.ptr(x), C.ptr(y), C.ptr(gamma), C.ptr(beta), C.ptr(fc_w), C.ptr(fc_b), C.ptr(pred), rows, h,
           n_pred, float(eps), C.dt(x), C.stream())
    return y, pred


def fp_embed(ids, word, pos, cu_seqlens, max_len, dtype, spk=None, out=None):
    """y[r] = round16(word[ids[r]] + pos[position of r in its sequence] (+ spk)): ids int64 [total] packed, word fp32 [n_symbols, D],
    pos fp32 [n_pos >= max_len, D], spk fp32 [D] or None -> [total, D] of `dtype`."""
    C.require_cuda(ids, word, pos, cu_seqlens, spk, out)
    name = "fp_embed"
    if dtype not in _FP16:
        raise ValueError("%s: 16-bit output only (got %s)" % (name, dtype))
    if ids.dtype != torch.int64 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("%s: ids must be a contiguous int64 tensor [total]" % name)
    if word.dim() != 2 or pos.dim() != 2:
        raise ValueError("%s: word and pos must be fp32 [rows, D]" % name)
    d = word.shape[1]
    _f32_tensor(name, word, (word.shape[0], d), "word")
    _f32_tensor(name, pos, (pos.shape[0], d), "pos")
    if spk is not None:
        _f32_tensor(name, spk, (d,), "spk")
    b = _cu_table(name, cu_seqlens)
    total = ids.numel()
    out = _out_tensor(name, out, (total, d), dtype, ids.device)
    C.call("dle_fp_embed", C.ptr(ids), C.ptr(word), C.ptr(pos), C.ptr(spk), C.ptr(out), C.ptr(cu_seqlens), b, int(max_len), total,
           word.shape[0], pos.shape[0], d, C.dt(dtype), C.stream())
    return out


def fp_scalar_conv_add_(enc, v, w, bias, cu_seqlens, max_len):
    """enc[r, c] += bias[c] + sum_k w[c, k] v[r + k - (ksize - 1) / 2] in place (v zero outside the sequence): the Conv1d(1 -> D, k) of
    pitch_emb / energy_emb.  enc [total, D] 16-bit, v fp32 [total], w fp32 [D, ksize], bias fp32 [D]."""
    C.require_cuda(enc, v, w, bias, cu_seqlens)
    name = "fp_scalar_conv_add"
    if enc.dtype not in _FP16 or enc.dim() != 2 or not enc.is_contiguous():
        raise ValueError("%s: enc must be a contiguous 16-bit [total, D] tensor" % name)
    total, d = enc.shape
    _f32_tensor(name, v, (total,), "v")
    if w.dim() != 2:
        raise ValueError("%s: w must be fp32 [D, ksize]" % name)
    _f32_tensor(name, w, (d, w.shape[1]), "w")
    _f32_tensor(name, bias, (d,), "bias")
    b = _cu_table(name, cu_seqlens)
    C.annotate(bytes=float(enc.numel()) * 4, tag="scalar_conv R%dxD%d" % (total, d), replay=False)       # (adds into enc)
    C.call("dle_fp_scalar_conv_add", C.ptr(enc), C.ptr(v), C.ptr(w), C.ptr(bias), C.ptr(cu_seqlens), b, int(max_len), total, d,
           w.shape[1], C.dt(enc), C.stream())
    return enc


def fp_durations(src, cu_seqlens, max_len, pace=1.0, max_duration=75.0, from_log=True, max_out=1024):
    """Durations -> repetitions and the output sequence table (one workgroup).  src fp32 [total]: log durations (from_log: dur =
    clamp(exp(src) - 1, 0, max_duration)) or durations.  reps = (int)(dur / pace + 0.5f).
    -> (dur_pred fp32 [total] or None, reps int32 [total], tok_start int32 [total], cu_out int32 [B + 1])."""
    C.require_cuda(src, cu_seqlens)
    name = "fp_durations"
    if src.dim() != 1:
        raise ValueError("%s: src must be fp32 [total]" % name)
    total = src.numel()
    _f32_tensor(name, src, (total,), "src")
    b = _cu_table(name, cu_seqlens)
    if not (float(pace) > 0.0):
        raise ValueError("%s: pace must be positive (got %r)" % (name, pace))
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=src.device)
    dur = torch.empty(total, dtype=torch.float32, device=src.device) if from_log else None
    reps, tok_start, cu_out = i32(total), i32(total), i32(b + 1)
    C.call("dle_fp_durations", C.ptr(src), int(bool(from_log)), C.ptr(dur), C.ptr(reps), C.ptr(tok_start), C.ptr(cu_out),
           C.ptr(cu_seqlens), b, int(max_len), total, float(pace), float(max_duration), int(max_out), C.stream())
    return dur, reps, tok_start, cu_out


def fp_expand(enc, pos, reps, tok_start, cu_in, cu_out, max_in, max_out, total_out, out=None):
    """The length regulator as a gather + the decoder's positional embedding: y[cu_out[b] + p] = round16(enc[j] + pos[p]), j the token
    of sequence b that covers frame p.  enc [total_in, D] 16-bit, pos fp32 [n_pos >= max_out, D] -> [total_out, D]."""
    C.require_cuda(enc, pos, reps, tok_start, cu_in, cu_out, out)
    name = "fp_expand"
    if enc.dtype not in _FP16 or enc.dim() != 2 or not enc.is_contiguous():
        raise ValueError("%s: enc must be a contiguous 16-bit [total_in, D] tensor" % name)
    total_in, d = enc.shape
    if pos.dim() != 2:
        raise ValueError("%s: pos must be fp32 [n_pos, D]" % name)
    _f32_tensor(name, pos, (pos.shape[0], d), "pos")
    for t, what in ((reps, "reps"), (tok_start, "tok_start")):
        if t.dtype != torch.int32 or tuple(t.shape) != (total_in,) or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous int32 tensor [total_in]" % (name, what))
    b = _cu_table(name, cu_in, "cu_in")
    if _cu_table(name, cu_out, "cu_out") != b:
        raise ValueError("%s: cu_in and cu_out differ in length" % name)
    out = _out_tensor(name, out, (int(total_out), d), enc.dtype, enc.device)
    C.call("dle_fp_expand", C.ptr(enc), C.ptr(pos), C.ptr(reps), C.ptr(tok_start), C.ptr(cu_in), C.ptr(cu_out), C.ptr(out), b,
           int(max_in), total_in, int(max_out), int(total_out), pos.shape[0], d, C.dt(enc), C.stream())
    return out


def fp_unpack_mel(x, bias, cu_seqlens, t_pad, out=None):
    """Packed [total, n_mel] 16-bit -> fp32 [B, n_mel, t_pad]; the frames behind a sequence's length hold bias (fp32 [n_mel])."""
    C.require_cuda(x, bias, cu_seqlens, out)
    name = "fp_unpack_mel"
    if x.dtype not in _FP16 or x.dim() != 2 or not x.is_contiguous():
        raise ValueError("%s: x must be a contiguous 16-bit [total, n_mel] tensor" % name)
    total, n_mel = x.shape
    _f32_tensor(name, bias, (n_mel,), "bias")
    b = _cu_table(name, cu_seqlens)
    out = _out_tensor(name, out, (b, n_mel, int(t_pad)), torch.float32, x.device)
    C.call("dle_fp_unpack_mel", C.ptr(x), C.ptr(bias), C.ptr(out), C.ptr(cu_seqlens), b, total, n_mel, int(t_pad), C.dt(x), C.stream())
    return out


# ------------------------------------------------------------------ QuartzNet on packed utterances (csrc/quartznet.hip)
def pack_depthwise_weight(w, dtype):
    """torch's depthwise Conv1d weight [C, 1, ksize] (any device / float dtype) -> the [ksize, C] 16-bit tensor tcs_conv1d_packed_fwd
    reads: a tap's channels are contiguous (one rounding per element).  A depthwise Conv2d weight [C, 1, k, k] -> the [k, k, C]
    tensor dwconv2d_act_fwd reads, likewise."""
    if w.dim() == 4 and w.shape[1] == 1 and w.shape[2] == w.shape[3]:
        if dtype not in _FP16:
            raise ValueError("pack_depthwise_weight: dtype must be torch.float16 or torch.bfloat16")
        return w.detach()[:, 0].permute(1, 2, 0).to(dtype).contiguous()
    if w.dim() != 3 or w.shape[1] != 1:
        raise ValueError("pack_depthwise_weight: expected a [C, 1, ksize] weight (got %s)" % (tuple(w.shape),))
    if dtype not in _FP16:
        raise ValueError("pack_depthwise_weight: dtype must be torch.float16 or torch.bfloat16")
    return w.detach()[:, 0, :].t().to(dtype).contiguous()


def pad_ctc_decoder(weight, bias, dtype, rows=32):
    """The decoder's Conv1d(k = 1) weight [n_classes, C] (or [n_classes, C, 1]) and bias [n_classes] -> (16-bit [rows, C], fp32
    [rows]) with zero rows behind the classes: gemm then writes fp32 logits [total, rows] with 16-byte rows, and ctc_greedy_packed is
    told n_classes and ld = rows, so the padding columns never count."""
    if dtype not in _FP16:
        raise ValueError("pad_ctc_decoder: dtype must be torch.float16 or torch.bfloat16")
    w = weight.detach().reshape(weight.shape[0], -1)
    n, c = w.shape
    if bias.numel() != n or n > rows:
        raise ValueError("pad_ctc_decoder: weight [%d, %d], bias %d, rows %d do not fit" % (n, c, bias.numel(), rows))
    wp = torch.zeros((rows, c), dtype=dtype, device=w.device)
    wp[:n] = w.to(dtype)
    bp = torch.zeros((rows,), dtype=torch.float32, device=w.device)
    bp[:n] = bias.detach().float()
    return wp.contiguous(), bp.contiguous()


def _packed_conv_operands(name, x, ko, scale, shift, cu_in, cu_out, total_out, stride, residual, out):
    """What tcs_conv1d_packed_fwd and conv1d_bn_packed_fwd share behind their weight checks: the two tables (stride 1: cu_out
    defaults to cu_in and total_out to total_in), scale / shift / residual, and the output.  -> (B, cu_out, total_out, out)."""
    b = _cu_table(name, cu_in, "cu_in")
    if cu_out is None:
        if stride != 1:
            raise ValueError("%s: stride %d needs cu_out and total_out" % (name, stride))
        cu_out = cu_in
    elif _cu_table(name, cu_out, "cu_out") != b:
        raise ValueError("%s: cu_in and cu_out must describe the same batch" % name)
    if total_out is None:
        if stride != 1:
            raise ValueError("%s: stride %d needs cu_out and total_out" % (name, stride))
        total_out = x.shape[0]
    total_out = int(total_out)
    _f32_tensor(name, scale, (ko,), "scale")
    _f32_tensor(name, shift, (ko,), "shift")
    if residual is not None and (tuple(residual.shape) != (total_out, ko) or residual.dtype != x.dtype or not residual.is_contiguous()):
        raise ValueError("%s: residual must be a contiguous [total_out,Ko] tensor of x's dtype" % name)
    return b, cu_out, total_out, _out_tensor(name, out, (total_out, ko), x.dtype, x.device)


def tcs_conv1d_packed_fwd(x, dw, pw, scale, shift, cu_in, cu_out=None, total_out=None, stride=1, dilation=1, residual=None,
                          relu=True, out=None, d_out=None):
    """One time-channel separable unit in one launch, per SEQUENCE of a packed x [total_in, C] (16-bit, channels-last):
    d = round16(depthwise(x, dw)), y = round16(relu?(scale * (pw @ d) + shift (+ residual))).  dw [ksize, C] (pack_depthwise_weight),
    pw [Ko, C], scale / shift fp32 [Ko], residual [total_out, Ko] or None, d_out [total_out, C] or None (receives d).  cu_in / cu_out
    are device int32 [B + 1]; stride 1: cu_out defaults to cu_in and total_out to total_in; stride 2 needs both.  Anything outside the
    kernel's envelope (include/dle_mi355x.h) raises ValueError."""
    C.require_cuda(x, dw, pw, scale, shift, cu_in, cu_out, residual, out, d_out)
    name = "tcs_conv1d_packed_fwd"
    if x.dtype not in _FP16:
        raise ValueError("%s: 16-bit activations and weights only (got %s)" % (name, x.dtype))
    if x.dim() != 2 or dw.dim() != 2 or pw.dim() != 2 or not (x.is_contiguous() and dw.is_contiguous() and pw.is_contiguous()) or \
            dw.dtype != x.dtype or pw.dtype != x.dtype or dw.shape[1] != x.shape[1] or pw.shape[1] != x.shape[1]:
        raise ValueError("%s: x must be contiguous [total,C], dw contiguous [ksize,C] and pw contiguous [Ko,C] of x's dtype" % name)
    total_in, c = x.shape
    ks, ko = dw.shape[0], pw.shape[0]
    b, cu_out, total_out, out = _packed_conv_operands(name, x, ko, scale, shift, cu_in, cu_out, total_out, stride, residual, out)
    if d_out is not None:
        d_out = _out_tensor(name, d_out, (total_out, c), x.dtype, x.device, "d_out")
    C.annotate(flops=2.0 * total_out * c * (ko + ks), tag="tcs %dx%d k%d ks%d s%d d%d B%d" % (total_in, c, ko, ks, stride, dilation, b),
               bytes=float(x.numel() + dw.numel() + pw.numel() + out.numel() * (2 if residual is not None else 1)) * 2)
    C.call("dle_tcs_conv1d_packed_fwd", C.ptr(x), C.ptr(dw), C.ptr(pw), C.ptr(scale), C.ptr(shift), C.ptr(residual), C.ptr(out),
           C.ptr(d_out), C.ptr(cu_in), C.ptr(cu_out), b, total_in, total_out, c, ko, ks, int(stride), int(dilation), int(bool(relu)),
           C.dt(x), C.stream())
    return out


def tcs_prefetch_mode(mode=-1):
    """Which form of the fused separable kernel's chunk loop runs: 0 without the register prefetch of the next chunk, 1 with it, 2 by
    grid size (the default); -1 only asks.  Returns the previous setting.  Both forms give the same bits (tests, A/B timing)."""
    return int(C.lib().dle_tcs_prefetch_mode(int(mode)))


def _qn_normalize_pack(name, x, cu_seqlens, total, dtype, lead, out):
    """lead None: the entry without a lead (dle_qn_normalize_pack); otherwise dle_qn_normalize_pack_lead."""
    C.require_cuda(x, cu_seqlens, out)
    if dtype not in _FP16:
        raise ValueError("%s: 16-bit output only (got %s)" % (name, dtype))
    if x.dtype != torch.float32 or x.dim() != 3 or not x.is_contiguous():
        raise ValueError("%s: x must be a contiguous fp32 [B, F, T_pad] tensor" % name)
    b, f, t_pad = x.shape
    if _cu_table(name, cu_seqlens) != b:
        raise ValueError("%s: cu_seqlens must have B + 1 = %d entries" % (name, b + 1))
    out = _out_tensor(name, out, (int(total), f), dtype, x.device)
    C.annotate(bytes=float(x.numel()) * 4 + float(out.numel()) * 2,
               tag="qn_normalize %dx%dx%d" % (b, f, t_pad) + ("" if lead is None else " lead %d" % lead))
    if lead is None:
        C.call("dle_qn_normalize_pack", C.ptr(x), C.ptr(out), C.ptr(cu_seqlens), b, f, t_pad, int(total), C.dt(dtype), C.stream())
    else:
        C.call("dle_qn_normalize_pack_lead", C.ptr(x), C.ptr(out), C.ptr(cu_seqlens), b, f, t_pad, int(lead), int(total), C.dt(dtype),
               C.stream())
    return out


def qn_normalize_pack(x, cu_seqlens, total, dtype, out=None):
    """Per-feature normalisation over each utterance's own frames (unbiased std + 1e-5), the mask, the transpose and the 16-bit cast
    in one launch: x fp32 [B, F, T_pad] -> packed [total, F] of `dtype`."""
    return _qn_normalize_pack("qn_normalize_pack", x, cu_seqlens, total, dtype, None, out)


def qn_normalize_pack_lead(x, cu_seqlens, total, dtype, lead, out=None):
    """qn_normalize_pack with `lead` zero rows in front of every utterance (Jasper's --pad_leading, applied to the normalised
    features): cu_seqlens describes the OUTPUT rows, len_b + lead per sequence; the statistics run over the len_b real frames."""
    return _qn_normalize_pack("qn_normalize_pack_lead", x, cu_seqlens, total, dtype, lead, out)


def ctc_greedy_packed(logits, cu_seqlens, n_classes, want_logp=True, logp_out=None, ids_out=None, tokens_out=None, n_tokens_out=None):
    """log_softmax, the first-maximum argmax and the CTC collapse (drop repeats, then blanks; blank = n_classes - 1) of packed fp32
    logits [total, ld >= n_classes] in one launch -> (logp fp32 [total, n_classes] or None, ids int32 [total], tokens int32 [total]
    packed per sequence at cu_seqlens[b], n_tokens int32 [B])."""
    C.require_cuda(logits, cu_seqlens, logp_out, ids_out, tokens_out, n_tokens_out)
    name = "ctc_greedy_packed"
    if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous():
        raise ValueError("%s: logits must be a contiguous fp32 [total, ld] tensor" % name)
    total, ld = logits.shape
    b = _cu_table(name, cu_seqlens)
    dev = logits.device
    logp = _out_tensor(name, logp_out, (total, int(n_classes)), torch.float32, dev, "logp") if (want_logp or logp_out is not None) else None
    ids = _out_tensor(name, ids_out, (total,), torch.int32, dev, "ids")
    tokens = _out_tensor(name, tokens_out, (total,), torch.int32, dev, "tokens")
    n_tokens = _out_tensor(name, n_tokens_out, (b,), torch.int32, dev, "n_tokens")
    C.annotate(bytes=float(logits.numel()) * 4 + (float(logp.numel()) * 4 if logp is not None else 0.0) + float(total) * 8,
               tag="ctc_greedy %dx%d B%d" % (total, n_classes, b))
    C.call("dle_ctc_greedy_packed", C.ptr(logits), C.ptr(logp), C.ptr(ids), C.ptr(tokens), C.ptr(n_tokens), C.ptr(cu_seqlens), b, total,
           int(n_classes), ld, C.stream())
    return logp, ids, tokens, n_tokens


# ------------------------------------------------------------------ Jasper on packed utterances (csrc/jasper.hip)
def conv1d_bn_packed_fwd(x, w, scale, shift, cu_in, cu_out=None, total_out=None, stride=1, dilation=1, residual=None, relu=True,
                         out=None):
    """One Jasper sub-block in one launch, per SEQUENCE of a packed x [total_in, C] (16-bit, channels-last):
    y = round16(relu?(scale * conv1d(x, w) + shift (+ residual))), 'same' padding, rows outside the sequence read as zero.
    w [Ko, ksize, C] (pack_conv1d_weight, the layout of conv1d_lrelu_fwd), scale / shift fp32 [Ko], residual [total_out, Ko] or None.  cu_in / cu_out are device
    int32 [B + 1]; stride 1: cu_out defaults to cu_in and total_out to total_in; stride 2 needs both.  Anything outside the
    kernel's envelope (include/dle_mi355x.h) raises ValueError."""
    C.require_cuda(x, w, scale, shift, cu_in, cu_out, residual, out)
    name = "conv1d_bn_packed_fwd"
    if x.dtype not in _FP16:
        raise ValueError("%s: 16-bit activations and weights only (got %s)" % (name, x.dtype))
    if x.dim() != 2 or w.dim() != 3 or not (x.is_contiguous() and w.is_contiguous()) or w.dtype != x.dtype or \
            w.shape[2] != x.shape[1]:
        raise ValueError("%s: x must be contiguous [total,C] and w contiguous [Ko,ksize,C] of x's dtype" % name)
    total_in, c = x.shape
    ko, ks = w.shape[0], w.shape[1]
    b, cu_out, total_out, out = _packed_conv_operands(name, x, ko, scale, shift, cu_in, cu_out, total_out, stride, residual, out)
    C.annotate(flops=2.0 * total_out * c * ko * ks, tag="conv1d_bn %dx%d k%d ks%d s%d d%d B%d" % (total_in, c, ko, ks, stride, dilation, b),
               bytes=float(x.numel() + w.numel() + out.numel() * (2 if residual is not None else 1)) * 2)
    C.call("dle_conv1d_bn_packed_fwd", C.ptr(x), C.ptr(w), C.ptr(scale), C.ptr(shift), C.ptr(residual), C.ptr(out), C.ptr(cu_in),
           C.ptr(cu_out), b, total_in, total_out, c, ko, ks, int(stride), int(dilation), int(bool(relu)), C.dt(x), C.stream())
    return out


# ------------------------------------------------------------------ Transformer-XL evaluation (csrc/transformer_xl.hip)
def txl_attention_supported(qlen, klen, head_dim):
    return bool(C.lib().dle_txl_attention_supported(int(qlen), int(klen), int(head_dim)))


def txl_attention_launch_count():
    """Launches of the relative attention kernel by this process so far."""
    return int(C.lib().dle_txl_attention_launch_count())


def _txl_i32(name, t, what, n=None):
    if t is None:
        return
    if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or (n is not None and t.numel() != n):
        raise ValueError("%s: %s must be a contiguous int32 vector%s" % (name, what, "" if n is None else " of %d" % n))


def txl_rel_attention_fwd(q, u, v, kv, r, heads, qlen, mlen, start, shift, scale, out=None):
    """Relative attention of one Transformer-XL layer and segment over the K / V ring: q [B*qlen, >= H] (a column slice of the
    [.., 3H] projection is fine), u / v [heads, 64] (r_w_bias, r_r_bias), kv [B, cap, 2H] ring whose logical key j sits at row
    (start + j) % cap, r [n_dist, H] by distance, allowed(i, j) = (i - shift < j) and (j <= i + mlen) -> ctx [B*qlen, H]."""
    C.require_cuda(q, u, v, kv, r, out)
    name = "txl_rel_attention_fwd"
    heads, qlen, mlen, start, shift = int(heads), int(qlen), int(mlen), int(start), int(shift)
    if q.dtype not in _FP16 or any(t.dtype != q.dtype for t in (u, v, kv, r)):
        raise ValueError("%s: 16-bit operands of one dtype only" % name)
    if kv.dim() != 3 or not kv.is_contiguous() or heads < 1 or kv.shape[2] != 2 * heads * 64:
        raise ValueError("%s: kv must be a contiguous ring [B, cap, 2 * heads * 64]" % name)
    b, cap, h = kv.shape[0], kv.shape[1], heads * 64
    if tuple(u.shape) != (heads, 64) or tuple(v.shape) != (heads, 64) or not (u.is_contiguous() and v.is_contiguous()):
        raise ValueError("%s: u and v must be contiguous [heads, 64]" % name)
    if qlen < 1 or mlen < 0 or not txl_attention_supported(qlen, mlen + qlen, 64):
        raise ValueError("%s: outside the kernel's envelope: qlen %d, mlen %d (1 <= qlen <= 512, klen <= 4096)" % (name, qlen, mlen))
    klen = mlen + qlen
    if not (klen <= cap <= 4096) or not (0 <= start < cap) or shift < 1:
        raise ValueError("%s: needs klen <= cap <= 4096, 0 <= start < cap, shift >= 1 (got klen %d, cap %d, start %d, shift %d)"
                         % (name, klen, cap, start, shift))
    if q.dim() != 2 or q.shape[0] != b * qlen or q.shape[1] != h or q.stride(1) != 1 or q.stride(0) < h or q.stride(0) % 8:
        raise ValueError("%s: q must be [B*qlen, H] with unit inner stride and a row pitch that is a multiple of 8" % name)
    if r.dim() != 2 or r.shape[1] != h or r.shape[0] < klen or not r.is_contiguous():
        raise ValueError("%s: r must be a contiguous [n_dist >= klen, H] table" % name)
    out = _out_tensor(name, out, (b * qlen, h), q.dtype, q.device)
    C.annotate(flops=2.0 * b * heads * qlen * klen * 64 * 3, bytes=float(b) * (klen * 2 * h + 2 * qlen * h) * 2 + float(klen) * h * 2,
               tag="txl_attn B%d h%d q%d m%d" % (b, heads, qlen, mlen))
    C.call("dle_txl_rel_attention_fwd", C.ptr(q), q.stride(0), C.ptr(u), C.ptr(v), C.ptr(kv), C.ptr(r), C.ptr(out), b, heads, 64,
           qlen, mlen, cap, start, r.shape[0], min(shift, 1 << 30), float(scale), C.dt(q), C.stream())
    return out


def txl_kv_append(qkv, kv, qlen, mlen, start):
    """K and V thirds of the segment's projection qkv [B*qlen, 3H] -> rows (start + mlen + t) % cap of the ring kv [B, cap, 2H]."""
    C.require_cuda(qkv, kv)
    name = "txl_kv_append"
    qlen, mlen, start = int(qlen), int(mlen), int(start)
    if qkv.dtype not in _FP16 or kv.dtype != qkv.dtype:
        raise ValueError("%s: 16-bit operands of one dtype only" % name)
    if kv.dim() != 3 or not kv.is_contiguous() or kv.shape[2] % 16:
        raise ValueError("%s: kv must be a contiguous ring [B, cap, 2H]" % name)
    b, cap, h = kv.shape[0], kv.shape[1], kv.shape[2] // 2
    if qkv.dim() != 2 or not qkv.is_contiguous() or tuple(qkv.shape) != (b * qlen, 3 * h):
        raise ValueError("%s: qkv must be a contiguous [B*qlen, 3H] tensor" % name)
    if qlen < 1 or mlen < 0 or mlen + qlen > cap or cap > 4096 or not (0 <= start < cap):
        raise ValueError("%s: needs mlen + qlen <= cap <= 4096 and 0 <= start < cap (got %d, %d, %d, %d)" % (name, mlen, qlen, cap, start))
    C.annotate(bytes=float(b) * qlen * 2 * h * 2 * 2, tag="txl_kv_append B%d q%d" % (b, qlen))
    C.call("dle_txl_kv_append", C.ptr(qkv), qkv.stride(0), C.ptr(kv), b, h, qlen, mlen, cap, start, C.dt(qkv), C.stream())
    return kv


def rows_gather_scale(src, dst, rows, src_idx=None, dst_idx=None, scale=1.0):
    """dst[dst_idx[r], :] = round16(scale * float(src[src_idx[r], :])) for r < rows; either int32 index list may be None (= r).
    Rows whose index falls outside its tensor are skipped; destination rows must be distinct."""
    C.require_cuda(src, dst, src_idx, dst_idx)
    name = "rows_gather_scale"
    rows = int(rows)
    if src.dtype not in _FP16 or dst.dtype != src.dtype:
        raise ValueError("%s: 16-bit operands of one dtype only" % name)
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1] or src.shape[1] % 8 or src.shape[1] == 0:
        raise ValueError("%s: src and dst must be 2-D with one width, a multiple of 8" % name)
    for t in (src, dst):
        if t.stride(1) != 1 or t.stride(0) < t.shape[1] or t.stride(0) % 8:
            raise ValueError("%s: unit inner stride and a row pitch that is a multiple of 8" % name)
    _txl_i32(name, src_idx, "src_idx", rows)
    _txl_i32(name, dst_idx, "dst_idx", rows)
    if rows < 0 or (src_idx is None and rows > src.shape[0]) or (dst_idx is None and rows > dst.shape[0]):
        raise ValueError("%s: %d rows do not fit src %d / dst %d" % (name, rows, src.shape[0], dst.shape[0]))
    if src.shape[0] == 0 or dst.shape[0] == 0:
        raise ValueError("%s: empty source or destination" % name)
    C.annotate(bytes=float(rows) * src.shape[1] * 4, tag="rows_gather_scale %dx%d" % (rows, src.shape[1]))
    C.call("dle_rows_gather_scale", C.ptr(src), C.ptr(src_idx), C.ptr(dst), C.ptr(dst_idx), rows, src.shape[1], src.stride(0),
           dst.stride(0), src.shape[0], dst.shape[0], float(scale), C.dt(src), C.stream())
    return dst


def row_nll(logits, target, nll, pos=None, n_classes=None, accumulate=False):
    """nll[pos[r]] (+)= logsumexp(logits[r, :n_classes]) - logits[r, target[r]] on fp32 logits [rows, ld]; target / pos int32
    [rows] (pos None = r; the positions of one call must be distinct); nll fp32 vector."""
    C.require_cuda(logits, target, nll, pos)
    name = "row_nll"
    if logits.dtype != torch.float32 or logits.dim() != 2 or logits.stride(1) != 1 or logits.stride(0) < logits.shape[1]:
        raise ValueError("%s: logits must be an fp32 [rows, ld] tensor with unit inner stride" % name)
    rows = logits.shape[0]
    n_classes = logits.shape[1] if n_classes is None else int(n_classes)
    if not (1 <= n_classes <= 160003) or n_classes > logits.shape[1]:
        raise ValueError("%s: 1 <= n_classes <= min(160003, ld) (got %d, ld %d)" % (name, n_classes, logits.shape[1]))
    _txl_i32(name, target, "target", rows)
    _txl_i32(name, pos, "pos", rows)
    if target is None:
        raise ValueError("%s: target is required" % name)
    if nll.dtype != torch.float32 or nll.dim() != 1 or not nll.is_contiguous() or nll.numel() == 0 or \
            (pos is None and rows > nll.numel()):
        raise ValueError("%s: nll must be a contiguous fp32 vector with room for the rows" % name)
    C.annotate(bytes=float(rows) * n_classes * 4, tag="row_nll %dx%d" % (rows, n_classes), replay=not accumulate)
    C.call("dle_row_nll", C.ptr(logits), logits.stride(0), C.ptr(target), C.ptr(pos), C.ptr(nll), rows, n_classes, nll.numel(),
           int(bool(accumulate)), C.stream())
    return nll


# ---- Temporal Fusion Transformer inference (csrc/tft.hip) ---------------------------------------------------------------------
TFT_HIDDEN = 128
TFT_MAX_VARS = 8
TFT_ROW_TILE = 32            # rows per workgroup of the GRN / VSN kernels, batch rows per workgroup of the LSTM


def _tft_rows16(name, t, what):
    if t.dtype not in _FP16 or t.dim() != 2 or t.shape[1] != TFT_HIDDEN or t.stride(1) != 1 or t.stride(0) % 8 or \
            (t.shape[0] > 1 and t.stride(0) < TFT_HIDDEN):
        raise ValueError("%s: %s must be 16-bit [rows, 128] with unit inner stride and a row pitch that is a multiple of 8" % (name, what))


def _tft_w16(name, t, shape, dtype, what):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor %s" % (name, what, dtype, list(shape)))


def tft_grn_pack(grn, dtype, device):
    """The parameters of one reference GRN (or of a GLU + LayerNorm pair given as {'glu': .., 'ln': ..}) as the kernel takes them:
    16-bit weights [out][in], fp32 biases and LayerNorm parameters.  `grn` maps the reference's parameter names to tensors."""
    def w(k):
        return grn[k].detach().to(device=device, dtype=dtype).contiguous()

    def f(k):
        return grn[k].detach().to(device=device, dtype=torch.float32).contiguous()
    p = {"wg": w("glu.lin.weight"), "bg": f("glu.lin.bias"), "gamma": f("layer_norm.ln.weight"), "beta": f("layer_norm.ln.bias")}
    if "lin_a.weight" in grn:
        p.update(wa=w("lin_a.weight"), ba=f("lin_a.bias"), wi=w("lin_i.weight"), bi=f("lin_i.bias"))
        if "lin_c.weight" in grn:
            p["wc"] = w("lin_c.weight")
    return p


def tft_grn_fwd(x, p, ctx=None, rows_per_ctx=1, res=None, res_rows_per_batch=0, x_index=None, wq=None, bq=None, eps=1e-3,
                want_out=True, out=None):
    """One gated residual network on x [rows, 128] (or on the rows x[x_index]), parameters from tft_grn_pack.  ctx [batch, 128]
    with rows_per_ctx rows of x per context row.  Without 'wa' in p: gate mode, GLU(x) + res -> LayerNorm; res is [rows, 128] or,
    with res_rows_per_batch, a [batch, steps, 128] tensor whose LAST res_rows_per_batch steps of every batch element are the rows.
    wq [Q, 128] / bq [Q] fp32: also returns the fp32 [rows, Q] projection of the unrounded output.  Returns out, (out, q) or q."""
    name = "tft_grn_fwd"
    C.require_cuda(x, ctx, res, x_index, wq, bq, out)
    _tft_rows16(name, x, "x")
    dtype = x.dtype
    gate = "wa" not in p
    rows = x.shape[0] if x_index is None else x_index.numel()
    if x_index is not None and (x_index.dtype != torch.int32 or x_index.dim() != 1 or not x_index.is_contiguous()):
        raise ValueError("%s: x_index must be a contiguous int32 vector" % name)
    _tft_w16(name, p["wg"], (2 * TFT_HIDDEN, TFT_HIDDEN), dtype, "wg")
    _f32_tensor(name, p["bg"], (2 * TFT_HIDDEN,), "bg")
    _f32_tensor(name, p["gamma"], (TFT_HIDDEN,), "gamma")
    _f32_tensor(name, p["beta"], (TFT_HIDDEN,), "beta")
    res_ptr, ldr, res_bs = 0, 0, 0
    if gate:
        if res is None or ctx is not None:
            raise ValueError("%s: gate mode takes a residual and no context" % name)
        if res_rows_per_batch:
            if res.dtype != dtype or res.dim() != 3 or res.shape[2] != TFT_HIDDEN or not res.is_contiguous() or \
                    res.shape[1] < res_rows_per_batch or res.shape[0] * res_rows_per_batch != rows:
                raise ValueError("%s: res must be a contiguous [rows / %d, steps >= %d, 128] tensor" % (name, res_rows_per_batch, res_rows_per_batch))
            res_ptr = res.data_ptr() + (res.shape[1] - res_rows_per_batch) * TFT_HIDDEN * res.element_size()
            ldr, res_bs = TFT_HIDDEN, res.shape[1] * TFT_HIDDEN
        else:
            _tft_rows16(name, res, "res")
            if res.dtype != dtype or res.shape[0] != rows:
                raise ValueError("%s: res must have the rows and the type of x" % name)
            res_ptr, ldr = res.data_ptr(), res.stride(0) if rows > 1 else TFT_HIDDEN
    else:
        if res is not None:
            raise ValueError("%s: the residual of the full network is its input" % name)
        for k in ("wa", "wi"):
            _tft_w16(name, p[k], (TFT_HIDDEN, TFT_HIDDEN), dtype, k)
        _f32_tensor(name, p["ba"], (TFT_HIDDEN,), "ba")
        _f32_tensor(name, p["bi"], (TFT_HIDDEN,), "bi")
        if ctx is not None:
            if "wc" not in p:
                raise ValueError("%s: this network has no lin_c" % name)
            _tft_w16(name, p["wc"], (TFT_HIDDEN, TFT_HIDDEN), dtype, "wc")
            _tft_rows16(name, ctx, "ctx")
            if ctx.dtype != dtype or rows_per_ctx < 1 or ctx.shape[0] * rows_per_ctx < rows:
                raise ValueError("%s: ctx has %d rows for %d rows of x at %d rows per context" % (name, ctx.shape[0], rows, rows_per_ctx))
    q = None
    if wq is not None:
        nq = wq.shape[0]
        if not 1 <= nq <= 8:
            raise ValueError("%s: 1 to 8 quantiles (got %d)" % (name, nq))
        _f32_tensor(name, wq, (nq, TFT_HIDDEN), "wq")
        _f32_tensor(name, bq, (nq,), "bq")
        q = torch.empty((rows, nq), dtype=torch.float32, device=x.device)
    if want_out or q is None:
        out = _out_tensor(name, out, (rows, TFT_HIDDEN), dtype, x.device)
    else:
        out = None
    C.annotate(flops=2.0 * rows * TFT_HIDDEN * TFT_HIDDEN * (2 if gate else 4 + (ctx is not None)), tag="tft_grn %d%s" % (rows, " gate" if gate else ""))
    C.call("dle_tft_grn_fwd", C.ptr(x), x.stride(0) if x.shape[0] > 1 else TFT_HIDDEN, C.ptr(x_index), x.shape[0] if x_index is not None else 0,
           C.ptr(ctx), (ctx.stride(0) if ctx.shape[0] > 1 else TFT_HIDDEN) if ctx is not None else 0, int(rows_per_ctx),
           res_ptr, ldr, int(res_rows_per_batch), res_bs,
           C.ptr(p.get("wa")), C.ptr(p.get("ba")), C.ptr(p.get("wc")) if ctx is not None else 0, C.ptr(p.get("wi")), C.ptr(p.get("bi")),
           C.ptr(p["wg"]), C.ptr(p["bg"]), C.ptr(p["gamma"]), C.ptr(p["beta"]), float(eps), C.ptr(out), TFT_HIDDEN,
           C.ptr(wq), C.ptr(bq), C.ptr(q), q.shape[1] if q is not None else 0, rows, TFT_HIDDEN, C.dt(dtype), C.stream())
    if q is None:
        return out
    return (out, q) if out is not None else q


def tft_vsn_pack(vsn, emb_vectors, emb_bias, dtype, device):
    """Parameter blocks of dle_tft_vsn_fwd for a selection network over F continuous variables.  `vsn` maps the reference's names
    (joint_grn.*, var_grns.N.*) to tensors; emb_vectors / emb_bias [F, 128] are the embedding of the variables in the network's
    column order.  The first linear of every network acts on x_f a_f + b_f, so it is folded here, in float64, into
    x_f (W a_f) + (W b_f + bias); so is the out_proj of the joint network."""
    H = TFT_HIDDEN
    d = {k: v.detach().double().cpu() for k, v in vsn.items()}
    a, b = emb_vectors.detach().double().cpu(), emb_bias.detach().double().cpu()
    F = a.shape[0]
    if not 1 <= F <= TFT_MAX_VARS or tuple(a.shape) != (F, H) or tuple(b.shape) != (F, H):
        raise ValueError("tft_vsn_pack: 1 to 8 variables with [F, 128] embeddings (got %s)" % (list(a.shape),))
    wa = d["joint_grn.lin_a.weight"].reshape(H, F, H)
    ju = torch.einsum("nfh,fh->fn", wa, a)
    jv = torch.einsum("nfh,fh->n", wa, b) + d["joint_grn.lin_a.bias"]
    wo = d["joint_grn.out_proj.weight"].reshape(F, F, H)                      # [f_out, f_in, h]
    jo = torch.zeros(F, 8, dtype=torch.float64)
    jo[:, :F] = torch.einsum("ofh,fh->fo", wo, a)
    jov = torch.zeros(8, dtype=torch.float64)
    jov[:F] = torch.einsum("ofh,fh->o", wo, b) + d["joint_grn.out_proj.bias"]
    wg = torch.zeros(32, H, dtype=torch.float64)
    bg = torch.zeros(32, dtype=torch.float64)
    wg[:F], wg[8:8 + F] = d["joint_grn.glu.lin.weight"][:F], d["joint_grn.glu.lin.weight"][F:]
    bg[:F], bg[8:8 + F] = d["joint_grn.glu.lin.bias"][:F], d["joint_grn.glu.lin.bias"][F:]
    gam, bet = torch.ones(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64)
    if F > 1:
        gam[:F], bet[:F] = d["joint_grn.layer_norm.ln.weight"], d["joint_grn.layer_norm.ln.bias"]
    has_ctx = "joint_grn.lin_c.weight" in d
    w16 = [d["joint_grn.lin_c.weight"] if has_ctx else torch.zeros(H, H, dtype=torch.float64), d["joint_grn.lin_i.weight"], wg]
    p32 = [ju, jv, d["joint_grn.lin_i.bias"], bg, jo, jov, gam, bet]
    for f in range(F):
        g = "var_grns.%d." % f
        w = d[g + "lin_a.weight"]
        p32 += [w @ a[f], w @ b[f] + d[g + "lin_a.bias"], a[f], b[f], d[g + "lin_i.bias"], d[g + "glu.lin.bias"],
                d[g + "layer_norm.ln.weight"], d[g + "layer_norm.ln.bias"]]
        w16 += [d[g + "lin_i.weight"], d[g + "glu.lin.weight"]]
    w16 = torch.cat([t.reshape(-1) for t in w16]).to(device=device, dtype=dtype)
    p32 = torch.cat([t.reshape(-1) for t in p32]).to(device=device, dtype=torch.float32)
    assert w16.numel() == 2 * H * H + 32 * H + F * 3 * H * H and p32.numel() == F * H + 2 * H + 32 + F * 8 + 24 + F * 9 * H
    return {"w16": w16, "p32": p32, "F": F, "has_ctx": has_ctx}


def tft_vsn_fwd(groups, p, dtype, steps, t0=0, ctx=None, out=None, out_t0=0, want_weights=False, eps=1e-3):
    """Embedding + variable selection in one launch.  groups: up to three fp32 tensors [B, T, n_g] (contiguous) whose columns,
    in order, are the F variables of the pack p; rows are steps t0 .. t0 + steps - 1 of every batch element; ctx [B, 128] or None.
    out: [B, out_T, 128] (allocated as [B, steps, 128] when None), written at steps out_t0 .. out_t0 + steps - 1.
    Returns out or (out, weights [B, steps, F] fp32)."""
    name = "tft_vsn_fwd"
    groups = [g for g in groups if g is not None]
    C.require_cuda(*groups, ctx, out)
    if not 1 <= len(groups) <= 3:
        raise ValueError("%s: one to three variable groups" % name)
    B, T = groups[0].shape[0], groups[0].shape[1]
    for g in groups:
        if g.dtype != torch.float32 or g.dim() != 3 or g.shape[0] != B or g.shape[1] != T or not g.is_contiguous():
            raise ValueError("%s: every group must be a contiguous fp32 [B, T, n] tensor of one B and T" % name)
    if sum(g.shape[2] for g in groups) != p["F"]:
        raise ValueError("%s: %d columns for a network of %d variables" % (name, sum(g.shape[2] for g in groups), p["F"]))
    if dtype not in _FP16 or p["w16"].dtype != dtype:
        raise ValueError("%s: the pack is %s, the call %s" % (name, p["w16"].dtype, dtype))
    steps, t0, out_t0 = int(steps), int(t0), int(out_t0)
    if steps < 1 or t0 < 0 or t0 + steps > T:
        raise ValueError("%s: steps %d .. %d of %d" % (name, t0, t0 + steps, T))
    if (ctx is not None) != p["has_ctx"]:
        raise ValueError("%s: the context and the network's lin_c go together" % name)
    if ctx is not None:
        _tft_rows16(name, ctx, "ctx")
        if ctx.dtype != dtype or ctx.shape[0] != B:
            raise ValueError("%s: ctx must be [B, 128] of the operand type" % name)
    if out is None:
        out = torch.empty((B, steps, TFT_HIDDEN), dtype=dtype, device=groups[0].device)
    if out.dtype != dtype or out.dim() != 3 or out.shape[0] != B or out.shape[2] != TFT_HIDDEN or not out.is_contiguous() or \
            out_t0 < 0 or out_t0 + steps > out.shape[1]:
        raise ValueError("%s: out must be a contiguous [B, >= out_t0 + steps, 128] tensor of the operand type" % name)
    weights = torch.empty((B, steps, p["F"]), dtype=torch.float32, device=out.device) if want_weights else None
    seg = []
    for i in range(3):
        g = groups[i] if i < len(groups) else None
        seg += [C.ptr(g), g.shape[2] if g is not None else 0, g.shape[2] if g is not None else 0]
    C.annotate(flops=2.0 * B * steps * TFT_HIDDEN * TFT_HIDDEN * (2 + 3 * p["F"]), tag="tft_vsn %dx%d F%d" % (B, steps, p["F"]))
    C.call("dle_tft_vsn_fwd", *seg, steps, T, t0, C.ptr(ctx), (ctx.stride(0) if B > 1 else TFT_HIDDEN) if ctx is not None else 0,
           C.ptr(p["w16"]), C.ptr(p["p32"]), C.ptr(out), TFT_HIDDEN, out.shape[1], out_t0, C.ptr(weights), B * steps, TFT_HIDDEN,
           float(eps), C.dt(dtype), C.stream())
    return (out, weights) if want_weights else out


def tft_lstm_fwd(xproj, whh, h0, c0, out=None, want_out=True):
    """A whole LSTM layer in one launch.  xproj [B, T, 512] fp32 = W_ih x + b_ih + b_hh (any batch / step strides that are
    multiples of 4, unit inner stride), whh [512, 128] 16-bit, h0 [B, 128] 16-bit, c0 [B, 128] fp32 or 16-bit.  out [B, T, 128]
    (a step-slice of a larger contiguous tensor is fine).  Returns out, hn (16-bit), cn (fp32)."""
    name = "tft_lstm_fwd"
    C.require_cuda(xproj, whh, h0, c0, out)
    if xproj.dtype != torch.float32 or xproj.dim() != 3 or xproj.shape[2] != 4 * TFT_HIDDEN or xproj.stride(2) != 1:
        raise ValueError("%s: xproj must be fp32 [B, T, 512] with unit inner stride" % name)
    B, T = xproj.shape[0], xproj.shape[1]
    dtype = whh.dtype
    if dtype not in _FP16:
        raise ValueError("%s: 16-bit weights only" % name)
    _tft_w16(name, whh, (4 * TFT_HIDDEN, TFT_HIDDEN), dtype, "whh")
    _tft_w16(name, h0, (B, TFT_HIDDEN), dtype, "h0")
    if c0.dtype not in (torch.float32, dtype) or tuple(c0.shape) != (B, TFT_HIDDEN) or not c0.is_contiguous():
        raise ValueError("%s: c0 must be a contiguous [B, 128] tensor, fp32 or of the operand type" % name)
    if T < 1 or B < 1:
        raise ValueError("%s: empty batch or sequence" % name)
    if want_out:
        if out is None:
            out = torch.empty((B, T, TFT_HIDDEN), dtype=dtype, device=xproj.device)
        if out.dtype != dtype or tuple(out.shape) != (B, T, TFT_HIDDEN) or out.stride(2) != 1:
            raise ValueError("%s: out must be [B, T, 128] of the operand type with unit inner stride" % name)
    else:
        out = None
    hn = torch.empty((B, TFT_HIDDEN), dtype=dtype, device=xproj.device)
    cn = torch.empty((B, TFT_HIDDEN), dtype=torch.float32, device=xproj.device)
    C.annotate(flops=2.0 * B * T * 4 * TFT_HIDDEN * TFT_HIDDEN, tag="tft_lstm %dx%d" % (B, T))
    C.call("dle_tft_lstm_fwd", C.ptr(xproj), xproj.stride(0) if B > 1 else T * xproj.stride(1), xproj.stride(1) if T > 1 else 4 * TFT_HIDDEN,
           C.ptr(whh), C.ptr(h0), C.ptr(c0), C.dt(c0), C.ptr(out),
           (out.stride(0) if B > 1 else T * out.stride(1)) if out is not None else 0,
           (out.stride(1) if T > 1 else TFT_HIDDEN) if out is not None else 0, C.ptr(hn), C.ptr(cn), B, T, TFT_HIDDEN, C.dt(dtype), C.stream())
    return out, hn, cn


def tft_attention_fwd(qkv, wo, B, T, encoder_length, heads=4, want_probs=False):
    """Interpretable multi-head attention for positions encoder_length .. T - 1: qkv [B * T, 288] 16-bit (q | k | shared v),
    wo [128, 32].  Returns out [B, T - encoder_length, 128], or (out, mean probabilities [B, T - encoder_length, T] fp32)."""
    name = "tft_attention_fwd"
    C.require_cuda(qkv, wo)
    B, T, enc, heads = int(B), int(T), int(encoder_length), int(heads)
    if heads != 4:
        raise ValueError("%s: built for 4 heads of 32 (got %d heads)" % (name, heads))
    if qkv.dtype not in _FP16 or qkv.dim() != 2 or qkv.shape[1] != 288 or qkv.stride(1) != 1 or qkv.stride(0) % 8 or qkv.shape[0] != B * T:
        raise ValueError("%s: qkv must be 16-bit [B * T, 288] with unit inner stride and a row pitch that is a multiple of 8" % name)
    _tft_w16(name, wo, (TFT_HIDDEN, 32), qkv.dtype, "wo")
    if not (2 <= T <= 192) or not (1 <= enc < T) or B < 1:
        raise ValueError("%s: needs 2 <= T <= 192 and 1 <= encoder_length < T (got T %d, encoder_length %d)" % (name, T, enc))
    out = torch.empty((B, T - enc, TFT_HIDDEN), dtype=qkv.dtype, device=qkv.device)
    probs = torch.empty((B, T - enc, T), dtype=torch.float32, device=qkv.device) if want_probs else None
    C.annotate(flops=2.0 * B * (T - enc) * T * 32 * 5, tag="tft_attn %dx%d/%d" % (B, T, enc))
    C.call("dle_tft_attention_fwd", C.ptr(qkv), qkv.stride(0) if B * T > 1 else 288, C.ptr(wo), C.ptr(out), C.ptr(probs), B, T, enc, heads, 32,
           C.dt(qkv), C.stream())
    return (out, probs) if want_probs else out


# ------------------------------------------------------------------ NCF (csrc/ncf.hip)
def ncf_score_supported(factors, layers):
    """Whether dle_ncf_score_fwd is built for this architecture (host only, no launch): --factors 64 --layers 256 256 128 64."""
    layers = [int(n) for n in layers]
    return len(layers) == 4 and bool(C.lib().dle_ncf_score_supported(int(factors), *layers))


def ncf_score_fwd(mf_user, mf_item, mlp_user, mlp_item, weights, biases, wf, bf, user, item, label=None, want_prob=False,
                  max_workgroups=0, logit_out=None, prob_out=None):
    """NeuMF.forward of `user` / `item` (int32 or int64 [B]) in one persistent launch.  Tables and weights = (W1, W2, W3) 16-bit,
    biases = (b1, b2, b3), wf [factors + l3] and bf [1] fp32.  Returns (logit fp32 [B], prob fp32 [B] or None, loss partials fp32
    or None): with label (fp32 [B]) the partials hold one binary cross-entropy sum per workgroup, zeros behind the grid; their
    sum is the batch's loss sum.  A sample with an index outside its table gets NaN and adds nothing to the loss."""
    name = "ncf_score_fwd"
    tables = (mf_user, mf_item, mlp_user, mlp_item)
    C.require_cuda(*tables, *weights, *biases, wf, bf, user, item, label, logit_out, prob_out)
    dtype = mf_user.dtype
    if dtype not in _FP16:
        raise ValueError("%s: 16-bit tables and weights only (got %s)" % (name, dtype))
    for t in tables + tuple(weights):
        if t.dtype != dtype or t.dim() != 2 or not t.is_contiguous():
            raise ValueError("%s: tables and weights must be contiguous 2-D tensors of one 16-bit type" % name)
    if len(weights) != 3 or len(biases) != 3:
        raise ValueError("%s: three MLP layers (got %d weights, %d biases)" % (name, len(weights), len(biases)))
    factors, l0 = mf_user.shape[1], 2 * mlp_user.shape[1]
    l1, l2, l3 = (w.shape[0] for w in weights)
    if mf_item.shape[1] != factors or mlp_item.shape[1] * 2 != l0 or mf_user.shape[0] != mlp_user.shape[0] or \
            mf_item.shape[0] != mlp_item.shape[0]:
        raise ValueError("%s: the user tables and the item tables must agree in rows, the GMF and MLP pairs in width" % name)
    if [w.shape[1] for w in weights] != [l0, l1, l2]:
        raise ValueError("%s: weight shapes do not chain: %s" % (name, [tuple(w.shape) for w in weights]))
    for b, n in zip(tuple(biases) + (wf, bf), (l1, l2, l3, factors + l3, 1)):
        if b.dtype != torch.float32 or b.numel() != n or not b.is_contiguous():
            raise ValueError("%s: biases and the final layer are contiguous fp32 tensors of %d elements" % (name, n))
    if user.dtype != item.dtype or user.dtype not in (torch.int32, torch.int64) or user.dim() != 1 or user.shape != item.shape or \
            not user.is_contiguous() or not item.is_contiguous():
        raise ValueError("%s: user and item must be contiguous int32 or int64 vectors of one length" % name)
    B, dev = user.numel(), mf_user.device
    if label is not None and (label.dtype != torch.float32 or label.numel() != B or not label.is_contiguous()):
        raise ValueError("%s: label must be a contiguous fp32 vector of the batch's length" % name)
    if max_workgroups < 0:
        raise ValueError("%s: max_workgroups must be 0 (the device's CU count) or positive" % name)
    logit = torch.empty(B, dtype=torch.float32, device=dev) if logit_out is None else logit_out
    prob = (torch.empty(B, dtype=torch.float32, device=dev) if prob_out is None else prob_out) if want_prob or prob_out is not None else None
    for t in (logit, prob):
        if t is not None and (t.dtype != torch.float32 or t.numel() != B or not t.is_contiguous()):
            raise ValueError("%s: outputs are contiguous fp32 vectors of the batch's length" % name)
    partials = None
    if label is not None:
        n = int(max_workgroups) or torch.cuda.get_device_properties(dev).multi_processor_count
        partials = torch.empty(n, dtype=torch.float32, device=dev)
    if B == 0:                                        # nothing to launch (and no pointer to hand over)
        return logit, prob, (partials.zero_() if partials is not None else None)
    C.annotate(flops=2.0 * B * (l0 * l1 + l1 * l2 + l2 * l3 + factors + l3), bytes=float(B) * (2 * (factors + l0 // 2) * 2 + 4),
               tag="ncf_score %d" % B)
    C.call("dle_ncf_score_fwd", C.ptr(mf_user), C.ptr(mf_item), C.ptr(mlp_user), C.ptr(mlp_item), mf_user.shape[0], mf_item.shape[0],
           C.ptr(weights[0]), C.ptr(biases[0]), C.ptr(weights[1]), C.ptr(biases[1]), C.ptr(weights[2]), C.ptr(biases[2]), C.ptr(wf),
           C.ptr(bf), C.ptr(user), C.ptr(item), 64 if user.dtype == torch.int64 else 32, C.ptr(label), C.ptr(logit), C.ptr(prob),
           C.ptr(partials), partials.numel() if partials is not None else 0, B, factors, l0, l1, l2, l3, int(max_workgroups),
           C.dt(dtype), C.stream())
    return logit, prob, partials


def ncf_rank_fwd(rating, label, ignore, samples_per_series, k):
    """hits (int32) and dcg (fp32) per series of `samples_per_series` elements by the stated rank rule of dle_ncf_rank_fwd:
    rating, label fp32 [n_series * S], ignore bool / uint8 of that length or None."""
    name = "ncf_rank_fwd"
    C.require_cuda(rating, label, ignore)
    S, k = int(samples_per_series), int(k)
    if rating.dtype != torch.float32 or label.dtype != torch.float32 or not rating.is_contiguous() or not label.is_contiguous() or \
            rating.numel() != label.numel():
        raise ValueError("%s: rating and label must be contiguous fp32 tensors of one length" % name)
    if S < 1 or rating.numel() % S:
        raise ValueError("%s: %d elements are not whole series of %d" % (name, rating.numel(), S))
    if ignore is not None:
        if ignore.dtype == torch.bool:
            ignore = ignore.view(torch.uint8)
        if ignore.dtype != torch.uint8 or ignore.numel() != rating.numel() or not ignore.is_contiguous():
            raise ValueError("%s: ignore must be a contiguous bool or uint8 tensor of the ratings' length" % name)
    n = rating.numel() // S
    hits = torch.empty(n, dtype=torch.int32, device=rating.device)
    dcg = torch.empty(n, dtype=torch.float32, device=rating.device)
    C.call("dle_ncf_rank_fwd", C.ptr(rating), C.ptr(label), C.ptr(ignore), C.ptr(hits), C.ptr(dcg), n, S, k, C.stream())
    return hits, dcg


# ------------------------------------------------------------------ MoFlow (csrc/moflow.hip)
def _mf_f32(name, t, numel, what):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
        raise ValueError("%s: %s must be a contiguous fp32 tensor of %d elements" % (name, what, numel))
    return t


def _mf_rows(name, z, width, what):
    """Row pitch of a 2-D fp32 [B, width] view with unit inner stride (a column slice of the latent vector)."""
    if z.dtype != torch.float32 or z.dim() != 2 or z.shape[1] != width or (width > 1 and z.stride(1) != 1):
        raise ValueError("%s: %s must be fp32 [batch, %d] with unit inner stride" % (name, what, width))
    return z.stride(0) if z.shape[0] > 1 else max(z.stride(0), width)


def mf_squeeze_fwd(z_adj, n_node, fold, img_half, dtype, state=None, img=None):
    """z_adj fp32 [B, 4 N N] (rows may be a slice of the latent vector) -> (state fp32 [B, P, C], 16-bit image [B, P, C/2] of half
    img_half): Block._squeeze with channels innermost."""
    name = "mf_squeeze_fwd"
    C.require_cuda(z_adj, state, img)
    if dtype not in _FP16:
        raise ValueError("%s: the image is 16-bit (got %s)" % (name, dtype))
    n, fold = int(n_node), int(fold)
    if fold < 1 or n < 1 or n % fold:
        raise ValueError("%s: n_node %d is not a multiple of the fold %d" % (name, n, fold))
    ldz = _mf_rows(name, z_adj, 4 * n * n, "z_adj")
    b, p, c = z_adj.shape[0], (n // fold) ** 2, 4 * fold * fold
    state = torch.empty((b, p, c), dtype=torch.float32, device=z_adj.device) if state is None else _mf_f32(name, state, b * p * c, "state")
    if img is None:
        img = torch.empty((b, p, c // 2), dtype=dtype, device=z_adj.device)
    elif img.dtype != dtype or not img.is_contiguous() or img.numel() != b * p * c // 2:
        raise ValueError("%s: img must be a contiguous %s tensor of %d elements" % (name, dtype, b * p * c // 2))
    if b:
        C.call("dle_mf_squeeze_fwd", C.ptr(z_adj), ldz, C.ptr(state), C.ptr(img), b, n, fold, int(img_half), C.dt(dtype), C.stream())
    return state, img


def mf_couple_fwd(h2, w3, b3, scale, loc, state, positions, mask_swap, img_half=None, state_out=None, img=None):
    """The third convolution of a bond coupling as the folded dense product + the rest of Flow.reverse (contract: dle_mi355x.h).
    h2 16-bit [B, K], w3 16-bit [2 M, K], b3 fp32 [2 M], scale / loc fp32 [C], state fp32 [B, P, C] -> (new state, 16-bit image of
    half img_half or None)."""
    name = "mf_couple_fwd"
    C.require_cuda(h2, w3, b3, scale, loc, state, state_out, img)
    dtype = h2.dtype
    if dtype not in _FP16 or w3.dtype != dtype:
        raise ValueError("%s: 16-bit operands of one type (got %s, %s)" % (name, h2.dtype, w3.dtype))
    if h2.dim() != 2 or w3.dim() != 2 or h2.stride(1) != 1 or not w3.is_contiguous() or w3.shape[1] != h2.shape[1] or w3.shape[0] % 2:
        raise ValueError("%s: h2 [batch, K] and a contiguous w3 [2 M, K]" % name)
    b, k, m, p = h2.shape[0], h2.shape[1], w3.shape[0] // 2, int(positions)
    if p < 1 or m % p:
        raise ValueError("%s: %d elements are not %d positions of whole channels" % (name, m, p))
    ch = m // p
    _mf_f32(name, b3, 2 * m, "b3"), _mf_f32(name, scale, 2 * ch, "scale"), _mf_f32(name, loc, 2 * ch, "loc")
    _mf_f32(name, state, b * 2 * m, "state")
    state_out = torch.empty_like(state) if state_out is None else _mf_f32(name, state_out, b * 2 * m, "state_out")
    if img_half is not None and img is None:
        img = torch.empty((b, p, ch), dtype=dtype, device=h2.device)
    if img is not None and (img.dtype != dtype or not img.is_contiguous() or img.numel() != b * m or img_half is None):
        raise ValueError("%s: img must be a contiguous %s tensor of %d elements, with img_half" % (name, dtype, b * m))
    C.annotate(flops=4.0 * b * m * k, bytes=2.0 * (2 * m * k + b * k) + 16.0 * b * m + (2.0 * b * m if img is not None else 0.0),
               tag="mf_couple %dx%dx%d" % (b, 2 * m, k))
    C.call("dle_mf_couple_fwd", C.ptr(h2), h2.stride(0) if b > 1 else max(h2.stride(0), k), C.ptr(w3), C.ptr(b3), C.ptr(scale), C.ptr(loc),
           C.ptr(state), C.ptr(state_out), C.ptr(img), b, p, ch, k, int(bool(mask_swap)), int(img_half or 0), C.dt(dtype), C.stream())
    return state_out, img


def mf_bond_decide_fwd(state, n_node, fold, unshift, want_adj=False, want_h=False, mask=None, code=None, adj01=None, h_adj=None):
    """The tail of MoFlow.reverse's bond half by the stated rule of dle_mf_bond_decide_fwd: state fp32 [B, P, C] -> (mask uint8
    [B, N, N], code uint8 [B, N, N], adj01 fp32 [B, 4, N, N] or None, h_adj fp32 [B, 4, N, N] or None)."""
    name = "mf_bond_decide_fwd"
    C.require_cuda(state, mask, code, adj01, h_adj)
    n, fold = int(n_node), int(fold)
    if fold < 1 or n < 1 or n % fold:
        raise ValueError("%s: n_node %d is not a multiple of the fold %d" % (name, n, fold))
    if state.dtype != torch.float32 or not state.is_contiguous() or state.numel() % (4 * n * n):
        raise ValueError("%s: state must be a contiguous fp32 tensor of whole [4, %d, %d] samples" % (name, n, n))
    b, dev = state.numel() // (4 * n * n), state.device
    mask = torch.empty((b, n, n), dtype=torch.uint8, device=dev) if mask is None else mask
    code = torch.empty((b, n, n), dtype=torch.uint8, device=dev) if code is None else code
    for t in (mask, code):
        if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != b * n * n:
            raise ValueError("%s: mask and code are contiguous uint8 [batch, %d, %d]" % (name, n, n))
    if want_adj and adj01 is None:
        adj01 = torch.empty((b, 4, n, n), dtype=torch.float32, device=dev)
    if want_h and h_adj is None:
        h_adj = torch.empty((b, 4, n, n), dtype=torch.float32, device=dev)
    for t in (adj01, h_adj):
        if t is not None:
            _mf_f32(name, t, b * 4 * n * n, "adj01 / h_adj")
    if b:
        C.call("dle_mf_bond_decide_fwd", C.ptr(state), C.ptr(mask), C.ptr(code), C.ptr(adj01), C.ptr(h_adj), b, n, fold, int(bool(unshift)),
               C.stream())
    return mask, code, adj01, h_adj


def mf_atom_supported(n_node, n_type, hidden_gnn, hidden_lin, n_flow, n_block=1, mask_row_size=1):
    """Whether dle_mf_atom_reverse_fwd is built for this atom flow (host only, no launch)."""
    g, l = [int(v) for v in hidden_gnn], [int(v) for v in hidden_lin]
    return bool(C.lib().dle_mf_atom_supported(int(n_node), int(n_type), int(n_block), len(g), g[0] if g else 0, len(l), l[0] if l else 0,
                                              l[1] if len(l) > 1 else 0, int(n_flow), int(mask_row_size)))


def mf_atom_reverse_fwd(z_x, mask, w16, p32, n_node, n_type, hidden_gnn, hidden_lin, row_stride, unshift, tile=32, max_workgroups=0,
                        out=None):
    """GlowOnGraph.reverse in one launch: z_x fp32 [B, N T] (rows may be a slice of the latent vector), mask uint8 [B, N, N] (the bits
    of mf_bond_decide_fwd), w16 16-bit [n_flow, w_stride] / p32 fp32 [n_flow, p_stride] as moflow.model.pack_atom_flows lays them
    out -> x fp32 [B, N, T]."""
    name = "mf_atom_reverse_fwd"
    C.require_cuda(z_x, mask, w16, p32, out)
    n, t = int(n_node), int(n_type)
    if w16.dtype not in _FP16 or w16.dim() != 2 or not w16.is_contiguous() or p32.dtype != torch.float32 or p32.dim() != 2 or \
            not p32.is_contiguous() or p32.shape[0] != w16.shape[0]:
        raise ValueError("%s: w16 [n_flow, pitch] 16-bit and p32 [n_flow, pitch] fp32, contiguous" % name)
    ldz = _mf_rows(name, z_x, n * t, "z_x")
    b = z_x.shape[0]
    if mask.dtype != torch.uint8 or not mask.is_contiguous() or mask.numel() != b * n * n:
        raise ValueError("%s: mask must be a contiguous uint8 [batch, %d, %d]" % (name, n, n))
    if len(hidden_gnn) != 1 or len(hidden_lin) != 2:
        raise ValueError("%s: built for one graph-convolution layer and two linear blocks (got %s, %s)" % (name, list(hidden_gnn), list(hidden_lin)))
    if max_workgroups < 0:
        raise ValueError("%s: max_workgroups must be 0 (the device's CU count) or positive" % name)
    out = torch.empty((b, n, t), dtype=torch.float32, device=z_x.device) if out is None else _mf_f32(name, out, b * n * t, "out")
    n_flow = w16.shape[0]
    per = sum(a * c for a, c in zip([4 * t + 4, hidden_gnn[0], hidden_lin[0], hidden_lin[1]], [hidden_gnn[0], hidden_lin[0], hidden_lin[1], 2 * t]))
    C.annotate(flops=2.0 * b * n_flow * per, bytes=float(w16.numel()) * 2 + b * (8.0 * n * t + n * n), tag="mf_atom %d" % b)
    C.call("dle_mf_atom_reverse_fwd", C.ptr(z_x), ldz, C.ptr(mask), C.ptr(w16), w16.stride(0), C.ptr(p32), p32.stride(0), C.ptr(out), b, n, t,
           int(hidden_gnn[0]), int(hidden_lin[0]), int(hidden_lin[1]), n_flow, int(row_stride), int(bool(unshift)), int(tile),
           int(max_workgroups), C.dt(w16.dtype), C.stream())
    return out


# ------------------------------------------------------------------ nnU-Net (csrc/nnunet.hip)
def _nu_volume(t, name):
    """(N, D, H, W, ld) of a contiguous channels-last 16-bit volume [N, D, H, W, ld]."""
    if t.dim() != 5 or not t.is_contiguous() or t.dtype not in _FP16:
        raise ValueError("%s: volumes are contiguous 16-bit [N, D, H, W, ld] tensors (got %s %s)" % (name, t.dtype, tuple(t.shape)))
    return tuple(int(s) for s in t.shape)


def conv3d_in_bands(D, H, W, stride):
    """Statistic bands per sample of conv3d_in_fwd's output for a [D, H, W] input (host only)."""
    g = int(C.lib().dle_conv3d_in_bands(int(D), int(H), int(W), int(stride)))
    if g < 1:
        raise ValueError("conv3d_in_bands: extents >= 1 and stride 1 or 2 (got %s, stride %s)" % ((D, H, W), stride))
    return g


def conv3d_in_fwd(x, weight, y, C_in=None, x_off=0, y_off=0, scale=None, shift=None, stride=1, relu_in=False, relu_out=True, part=None):
    """3x3x3 pad-1 convolution of channels [x_off, x_off + C_in) of x [N, D, H, W, ldx] into channels [y_off, y_off + Ko) of
    y [N, P, Q, R, ldy], with a = round16(relu_in?(scale[n, c] * x + shift[n, c])) applied on the operand load (scale None: a = x).
    weight [Ko, 3, 3, 3, C_in] 16-bit; scale, shift fp32 [N, C_in]; part None or fp32 [N, G, Ko, 3] receives (count, sum, M2) of the
    stored output per band.  Returns y."""
    name = "conv3d_in_fwd"
    C.require_cuda(x, weight, y, scale, shift, part)
    N, D, H, W, ldx = _nu_volume(x, name)
    Ny, P, Q, R, ldy = _nu_volume(y, name)
    if weight.dim() != 5 or tuple(weight.shape[1:4]) != (3, 3, 3) or weight.dtype != x.dtype or y.dtype != x.dtype or not weight.is_contiguous():
        raise ValueError("%s: weight is a contiguous [Ko, 3, 3, 3, C] tensor of the volumes' type (got %s %s)" % (name, weight.dtype, tuple(weight.shape)))
    Ko, Cw = int(weight.shape[0]), int(weight.shape[4])
    C_in = Cw if C_in is None else int(C_in)
    stride = int(stride)
    if C_in != Cw:
        raise ValueError("%s: the weight has %d input channels, the call names %d" % (name, Cw, C_in))
    if stride not in (1, 2) or (Ny, P, Q, R) != (N, (D - 1) // stride + 1, (H - 1) // stride + 1, (W - 1) // stride + 1):
        raise ValueError("%s: output %s does not belong to input %s at stride %s" % (name, (Ny, P, Q, R), (N, D, H, W), stride))
    if (scale is None) != (shift is None):
        raise ValueError("%s: scale and shift go together" % name)
    for t in (scale, shift):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (N, C_in) or not t.is_contiguous()):
            raise ValueError("%s: scale and shift are contiguous fp32 [N, C] = [%d, %d] tensors" % (name, N, C_in))
    if part is not None:
        G = conv3d_in_bands(D, H, W, stride)
        if part.dtype != torch.float32 or tuple(part.shape) != (N, G, Ko, 3) or not part.is_contiguous():
            raise ValueError("%s: part is a contiguous fp32 [N, G, Ko, 3] = [%d, %d, %d, 3] tensor" % (name, N, G, Ko))
    C.annotate(flops=2.0 * N * P * Q * R * 27 * C_in * Ko, bytes=2.0 * (N * D * H * W * C_in + N * P * Q * R * Ko + 27 * C_in * Ko),
               tag="conv3d_in %dx%dx%dx%d c%d k%d s%d" % (N, D, H, W, C_in, Ko, stride))
    C.call("dle_conv3d_in_fwd", C.ptr(x), ldx, int(x_off), C.ptr(scale), C.ptr(shift), C.ptr(weight), C.ptr(y), ldy, int(y_off), C.ptr(part),
           N, D, H, W, C_in, Ko, stride, int(bool(relu_in)), int(bool(relu_out)), C.dt(x), C.stream())
    return y


def instnorm_fold(part, gamma, beta, eps, scale, shift, out_off=0):
    """part fp32 [N, G, C, 3] -> scale = gamma / sqrt(var + eps), shift = beta - mean * scale (biased variance, Chan's merge in band
    order) into channels [out_off, out_off + C) of scale, shift fp32 [N, ld]."""
    name = "instnorm_fold"
    C.require_cuda(part, gamma, beta, scale, shift)
    if part.dtype != torch.float32 or part.dim() != 4 or part.shape[3] != 3 or not part.is_contiguous():
        raise ValueError("%s: part is a contiguous fp32 [N, G, C, 3] tensor" % name)
    N, G, Cn = (int(s) for s in part.shape[:3])
    for t in (gamma, beta):
        if t.dtype != torch.float32 or t.numel() != Cn or not t.is_contiguous():
            raise ValueError("%s: gamma and beta are contiguous fp32 vectors of %d elements" % (name, Cn))
    for t in (scale, shift):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != N or not t.is_contiguous() or t.shape != scale.shape:
            raise ValueError("%s: scale and shift are contiguous fp32 [N, ld] tensors of one shape" % name)
    C.call("dle_instnorm_fold", C.ptr(part), G, Cn, C.ptr(gamma), C.ptr(beta), float(eps), C.ptr(scale), C.ptr(shift), int(scale.shape[1]),
           int(out_off), N, C.stream())
    return scale, shift


def upsample3d_x2_bands(D, H, W):
    g = int(C.lib().dle_upsample3d_x2_bands(int(D), int(H), int(W)))
    if g < 1:
        raise ValueError("upsample3d_x2_bands: extents >= 1 (got %s)" % ((D, H, W),))
    return g


def upsample3d_x2_fwd(x, y, channels=None, x_off=0, y_off=0, part=None):
    """Trilinear x2 upsample (align_corners=True) of channels [x_off, x_off + channels) of x [N, D, H, W, ldx] into channels
    [y_off, ...) of y [N, 2D, 2H, 2W, ldy]; part None or fp32 [N, G, channels, 3].  Returns y."""
    name = "upsample3d_x2_fwd"
    C.require_cuda(x, y, part)
    N, D, H, W, ldx = _nu_volume(x, name)
    Ny, P, Q, R, ldy = _nu_volume(y, name)
    Cn = ldx if channels is None else int(channels)
    if (Ny, P, Q, R) != (N, 2 * D, 2 * H, 2 * W) or y.dtype != x.dtype:
        raise ValueError("%s: output %s is not twice the input %s" % (name, (Ny, P, Q, R), (N, D, H, W)))
    if part is not None:
        G = upsample3d_x2_bands(D, H, W)
        if part.dtype != torch.float32 or tuple(part.shape) != (N, G, Cn, 3) or not part.is_contiguous():
            raise ValueError("%s: part is a contiguous fp32 [N, G, C, 3] = [%d, %d, %d, 3] tensor" % (name, N, G, Cn))
    C.annotate(bytes=2.0 * N * D * H * W * Cn * 9, tag="upsample3d %dx%dx%dx%d c%d" % (N, D, H, W, Cn))
    C.call("dle_upsample3d_x2_fwd", C.ptr(x), ldx, int(x_off), C.ptr(y), ldy, int(y_off), C.ptr(part), N, D, H, W, Cn, C.dt(x), C.stream())
    return y


def nnunet_head_blend_fwd(x, weight, bias, imp, out, origin):
    """out[k, d0 + d, h0 + h, w0 + w] += imp[d, h, w] * (bias[k] + sum_c weight[k, c] * x[d, h, w, c]) for ONE window x [Dp, Hp, Wp, ld]
    (16-bit, channels last); weight 16-bit [K, C], bias fp32 [K], imp fp32 [Dp, Hp, Wp], out fp32 [K, Dv, Hv, Wv], origin (d0, h0, w0)."""
    name = "nnunet_head_blend_fwd"
    C.require_cuda(x, weight, bias, imp, out)
    if x.dim() != 4 or x.dtype not in _FP16 or not x.is_contiguous():
        raise ValueError("%s: the window is a contiguous 16-bit [Dp, Hp, Wp, ld] tensor" % name)
    Dp, Hp, Wp, ld = (int(s) for s in x.shape)
    if weight.dim() != 2 or weight.dtype != x.dtype or not weight.is_contiguous():
        raise ValueError("%s: weight is a contiguous [K, C] tensor of the window's type" % name)
    K, Cn = (int(s) for s in weight.shape)
    if bias.dtype != torch.float32 or bias.numel() != K or not bias.is_contiguous():
        raise ValueError("%s: bias is a contiguous fp32 vector of %d elements" % (name, K))
    if imp.dtype != torch.float32 or tuple(imp.shape) != (Dp, Hp, Wp) or not imp.is_contiguous():
        raise ValueError("%s: imp is a contiguous fp32 [%d, %d, %d] tensor" % (name, Dp, Hp, Wp))
    if out.dtype != torch.float32 or out.dim() != 4 or out.shape[0] != K or not out.is_contiguous():
        raise ValueError("%s: out is a contiguous fp32 [K, Dv, Hv, Wv] tensor" % name)
    d0, h0, w0 = (int(v) for v in origin)
    C.call("dle_nnunet_head_blend_fwd", C.ptr(x), ld, C.ptr(weight), C.ptr(bias), C.ptr(imp), C.ptr(out), K, Cn, Dp, Hp, Wp, int(out.shape[1]),
           int(out.shape[2]), int(out.shape[3]), d0, h0, w0, C.dt(x), C.stream())
    return out
