"""BraTS22 UNet3D inference on the gfx950 library (reference: nnunet/brats22_model.py UNet3D.forward under eval(), nn_unet.py
NNUnet.forward / tta_inference / sliding_window_inference).

Per patch batch the launch list is fixed: one dle_conv3d_in_fwd per convolution (22 at six levels), one dle_upsample3d_x2_fwd per
decoder level, one dle_instnorm_fold per normalised operand (two for a concat buffer: its halves come from different producers) and
one dle_nnunet_head_blend_fwd per sample.  An encoder output is written straight into its slot of the decoder's concat buffer and
the next downsampling convolution reads it from there; the normalised activations never exist in memory.

Sliding window (MONAI's sliding_window_inference is not part of the reference's text and cannot be run next to this project: the
rule below is the project's own statement of MONAI's documented behaviour, unverified against MONAI): a volume smaller than the
patch is zero-padded, half of the difference in front; the scan interval of an axis is int(patch * (1 - overlap)), at least 1, or the
patch where the axis is exactly one patch long; windows start at multiples of the interval and the last is clamped to the border;
blend "constant" weights every voxel 1, "gaussian" exp(-x^2 / (2 sigma^2)) per axis with sigma = 0.125 patch, normalised to a maximum
of 1 with zeros raised to the smallest positive value.  All of it is host work in float64, done once per volume geometry.
"""
import itertools
import math

import numpy as np
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import GraphCache, gpu_device, require_16bit
from . import model as M

TTA_FLIPS = ((), (2,), (3,), (4,), (2, 3), (2, 4), (3, 4), (2, 3, 4))          # nn_unet.py:55, the identity first


# ---------------------------------------------------------------------------------------------- host geometry (float64)
def scan_interval(image, patch, overlap):
    return tuple(p if i == p else max(int(p * (1.0 - overlap)), 1) for i, p in zip(image, patch))


def window_starts(image, patch, overlap):
    """Window origins (d, h, w) in scan order (w fastest) of a volume at least as large as the patch."""
    axes = []
    for size, p, step in zip(image, patch, scan_interval(image, patch, overlap)):
        if size < p:
            raise ValueError("window_starts: pad the volume to the patch first (%s < %s)" % (size, p))
        num = int(math.ceil(float(size) / step))
        n = next((d for d in range(num) if d * step + p >= size), None)
        n = 1 if n is None else n + 1
        axes.append([d * step - max(d * step + p - size, 0) for d in range(n)])
    return list(itertools.product(*axes))


def importance_map(patch, blend):
    """float64 [Dp, Hp, Wp]."""
    if blend == "constant":
        return np.ones(tuple(patch), dtype=np.float64)
    if blend != "gaussian":
        raise ValueError("blend must be 'constant' or 'gaussian' (got %r)" % (blend,))
    m = np.ones((), dtype=np.float64)
    for p in patch:
        x = np.arange(p, dtype=np.float64) - (p - 1) / 2.0
        m = np.multiply.outer(m, np.exp(-0.5 * (x / (0.125 * p)) ** 2))
    m = m / m.max()
    m[m == 0] = m[m > 0].min()
    return m


def pad_amounts(image, patch):
    """[(front, back)] per axis so that the padded volume holds one patch."""
    out = []
    for size, p in zip(image, patch):
        diff = max(p - size, 0)
        out.append((diff // 2, diff - diff // 2))
    return out


class BratsSegmenter:
    def __init__(self, state, dtype=torch.float16, device=None, graphs=False, patch_size=(128, 128, 128), val_batch_size=1):
        require_16bit(dtype, "BratsSegmenter")
        self.levels = M.levels_of(state)
        self.dev = dev = gpu_device(device, "BratsSegmenter")
        self.dtype, self.patch, self.batch = dtype, tuple(int(p) for p in patch_size), int(val_batch_size)
        if len(self.patch) != 3 or min(self.patch) < 1 or self.batch < 1:
            raise ValueError("BratsSegmenter: a 3-D patch size and a positive batch size")
        self.f = M.FILTERS[:self.levels]
        self.convs = M.conv_names(self.levels)
        self.w = {k: M.pack_conv_weight(state[k], dtype, dev) for k, *_ in self.convs}
        self.norm = {n: (state[n + ".weight"].to(dev, torch.float32).contiguous(), state[n + ".bias"].to(dev, torch.float32).contiguous())
                     for _, n, *_ in self.convs if n is not None}
        self.head_w = state["output_block.conv.weight"].to(dev, torch.float32).reshape(M.N_CLASS, self.f[0]).to(dtype).contiguous()
        self.head_b = state["output_block.conv.bias"].to(dev, torch.float32).contiguous()
        self._plans, self._geom, self._ones = {}, {}, {}
        self._graphs = GraphCache(graphs)

    # ------------------------------------------------------------------ the plan of one patch shape
    def _plan(self, N, D, H, W):
        """Buffers (allocated once per patch shape) and the launch list of UNet3D.forward for x [N, D, H, W, 8]."""
        key = (N, D, H, W)
        if key in self._plans:
            return self._plans[key]
        L, f, dev, dt = self.levels, self.f, self.dev, self.dtype
        dims = [(D, H, W)]
        for _ in range(1, L):
            dims.append(tuple((e - 1) // 2 + 1 for e in dims[-1]))
        for l in range(L - 1):
            if tuple(2 * e for e in dims[l + 1]) != dims[l]:
                raise ValueError("BratsSegmenter: patch %s does not halve evenly over %d levels (the reference's torch.cat fails too)" % ((D, H, W), L))

        def vol(l, c):
            return torch.empty((N,) + dims[l] + (c,), dtype=dt, device=dev)

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=dev)

        ops = []                                        # (kind, kwargs)
        xin = torch.zeros((N, D, H, W, M.STEM_CHANNELS), dtype=dt, device=dev)
        cat = [vol(l, f[l + 1] + f[l]) for l in range(L - 1)]       # [upsampled f[l+1] | skip f[l]]
        wkey = iter(self.convs)

        def conv(x, cin, x_off, y, y_off, l_in, stride, table, relu_in, relu_out, want_part):
            k, n, s, ci, co = next(wkey)
            assert s == stride and (ci == cin or cin == M.STEM_CHANNELS), (k, s, stride, ci, cin)
            part = f32(N, F.conv3d_in_bands(*dims[l_in], stride), co, 3) if want_part else None
            ops.append(("conv", dict(x=x, weight=self.w[k], y=y, C_in=cin, x_off=x_off, y_off=y_off, scale=table[0] if table else None,
                                     shift=table[1] if table else None, stride=stride, relu_in=relu_in, relu_out=relu_out, part=part)))
            return part, n

        def fold(part, norm, table, off):
            g, b = self.norm[norm]
            c = part.shape[2]
            ops.append(("fold", dict(part=part, gamma=g[off:off + c], beta=b[off:off + c], eps=M.EPS, scale=table[0], shift=table[1], out_off=off)))

        # InputBlock: conv1 -> norm -> ReLU -> conv2 -> ReLU; its output is the skip half of cat[0]
        t0 = vol(0, f[0])
        p, _ = conv(xin, M.STEM_CHANNELS, 0, t0, 0, 0, 1, None, False, False, True)
        tab = (f32(N, f[0]), f32(N, f[0]))
        fold(p, "input_block.norm", tab, 0)
        skip_part = [None] * (L - 1)
        skip_part[0], _ = conv(t0, f[0], 0, cat[0], f[1], 0, 1, tab, True, True, True)
        # encoder: level l reads the skip half of cat[l-1]
        bott = None
        for l in range(1, L):
            name = self.convs[2 * l][1]                 # "<block>.conv1.norm"
            tab = (f32(N, f[l - 1]), f32(N, f[l - 1]))
            fold(skip_part[l - 1], name, tab, 0)
            mid = vol(l, f[l])
            p, _ = conv(cat[l - 1], f[l - 1], f[l], mid, 0, l - 1, 2, tab, False, True, True)
            tab = (f32(N, f[l]), f32(N, f[l]))
            fold(p, name.replace("conv1", "conv2"), tab, 0)
            if l < L - 1:
                skip_part[l], _ = conv(mid, f[l], 0, cat[l], f[l + 1], l, 1, tab, False, True, True)
            else:
                bott = vol(l, f[l])
                conv(mid, f[l], 0, bott, 0, l, 1, tab, False, True, False)
        # decoder: level l = L-2 .. 0
        cur, cur_c = bott, f[L - 1]
        for l in range(L - 2, -1, -1):
            up_part = f32(N, F.upsample3d_x2_bands(*dims[l + 1]), cur_c, 3)
            ops.append(("upsample", dict(x=cur, y=cat[l], channels=cur_c, x_off=0, y_off=0, part=up_part)))
            name = "upsamples.%d.conv_block.conv1.norm" % (L - 2 - l)
            cc = f[l + 1] + f[l]
            tab = (f32(N, cc), f32(N, cc))
            fold(up_part, name, tab, 0)
            fold(skip_part[l], name, tab, f[l + 1])
            mid = vol(l, f[l])
            p, _ = conv(cat[l], cc, 0, mid, 0, l, 1, tab, False, True, True)
            tab = (f32(N, f[l]), f32(N, f[l]))
            fold(p, name.replace("conv1", "conv2"), tab, 0)
            cur, cur_c = vol(l, f[l]), f[l]
            conv(mid, f[l], 0, cur, 0, l, 1, tab, False, True, False)
        assert next(wkey, None) is None
        plan = self._plans[key] = {"xin": xin, "ops": ops, "last": cur, "logits": f32(N, M.N_CLASS, D, H, W)}
        return plan

    def launch_list(self, N, D, H, W):
        """Kernel names of one patch batch, in order."""
        names = {"conv": "dle_conv3d_in_fwd", "fold": "dle_instnorm_fold", "upsample": "dle_upsample3d_x2_fwd"}
        return [names[k] for k, _ in self._plan(N, D, H, W)["ops"]] + ["dle_nnunet_head_blend_fwd"] * N

    def _features(self, x):
        """x [N, 5, D, H, W] on the device -> the last ReLU output [N, D, H, W, 64] (a buffer of the plan)."""
        N, c, D, H, W = x.shape
        plan = self._plan(N, D, H, W)
        plan["xin"][..., :M.IN_CHANNELS].copy_(x.permute(0, 2, 3, 4, 1))          # the NCDHW -> NDHWC pack, one rounding
        for kind, kw in plan["ops"]:
            if kind == "conv":
                F.conv3d_in_fwd(**kw)
            elif kind == "fold":
                F.instnorm_fold(**kw)
            else:
                F.upsample3d_x2_fwd(**kw)
        return plan["last"]

    def _check_patch(self, x):
        C.require_cuda(x)
        if x.dim() != 5 or x.shape[1] != M.IN_CHANNELS:
            raise ValueError("BratsSegmenter: input is [N, %d, D, H, W] (got %s)" % (M.IN_CHANNELS, tuple(x.shape)))
        return x.to(torch.float32)

    def _logits(self, x):
        feat = self._features(x)
        out = self._plans[(x.shape[0],) + tuple(x.shape[2:])]["logits"].zero_()
        ones = self._ones.get(tuple(x.shape[2:]))
        if ones is None:
            ones = self._ones[tuple(x.shape[2:])] = torch.ones(tuple(x.shape[2:]), dtype=torch.float32, device=self.dev)
        for n in range(x.shape[0]):
            F.nnunet_head_blend_fwd(feat[n], self.head_w, self.head_b, ones, out[n], (0, 0, 0))
        return out

    @torch.no_grad()
    def logits_patch(self, x):
        """UNet3D.forward under eval(): x [N, 5, D, H, W] -> fp32 [N, 3, D, H, W].  The result is the segmenter's buffer for this
        patch shape (allocated once, like every other buffer of the plan; with graphs=True the captured graph writes it): the next
        call with the same shape overwrites it, so copy what must outlive that."""
        x = self._check_patch(x)
        return self._graphs.run(("logits",) + tuple(x.shape[:1]) + tuple(x.shape[2:]), self._logits, x)

    @torch.no_grad()
    def forward(self, img):
        """NNUnet.forward (nn_unet.py:60-61): the class index per voxel."""
        return torch.argmax(self.logits_patch(img), 1)

    __call__ = forward

    # ------------------------------------------------------------------ sliding window
    def _geometry(self, shape, overlap, blend):
        key = (tuple(shape), float(overlap), blend)
        g = self._geom.get(key)
        if g is None:
            pads = pad_amounts(shape, self.patch)
            padded = tuple(s + a + b for s, (a, b) in zip(shape, pads))
            starts = window_starts(padded, self.patch, overlap)
            imp = importance_map(self.patch, blend)
            total = np.zeros(padded, dtype=np.float64)
            for d, h, w in starts:
                total[d:d + self.patch[0], h:h + self.patch[1], w:w + self.patch[2]] += imp
            g = self._geom[key] = {
                "pads": pads, "padded": padded, "starts": starts,
                "imp": torch.from_numpy(imp.astype(np.float32)).to(self.dev).contiguous(),
                "recip": torch.from_numpy((1.0 / total).astype(np.float32)).to(self.dev),
                "acc": torch.empty((M.N_CLASS,) + padded, dtype=torch.float32, device=self.dev),
                "win": {},
            }
        return g

    def _window_batch(self, g, vol, starts):
        """One patch batch: the windows' features, then one head launch per window into the accumulator (stream order)."""
        pd, ph, pw = self.patch
        n = len(starts)
        win = g["win"].get(n)
        if win is None:
            win = g["win"][n] = torch.empty((n, M.IN_CHANNELS, pd, ph, pw), dtype=torch.float32, device=self.dev)
        for i, (d, h, w) in enumerate(starts):
            win[i].copy_(vol[:, d:d + pd, h:h + ph, w:w + pw])

        def run(win):
            return self._features(win)
        feat = self._graphs.run(("features", n, pd, ph, pw), run, win)
        for i, origin in enumerate(starts):
            F.nnunet_head_blend_fwd(feat[i], self.head_w, self.head_b, g["imp"], g["acc"], origin)

    def _segment_once(self, vol, overlap, blend):
        g = self._geometry(tuple(vol.shape[1:]), overlap, blend)
        (a0, b0), (a1, b1), (a2, b2) = g["pads"]
        if any(a or b for a, b in g["pads"]):
            vol = torch.nn.functional.pad(vol, (a2, b2, a1, b1, a0, b0))
        g["acc"].zero_()
        for i in range(0, len(g["starts"]), self.batch):
            self._window_batch(g, vol, g["starts"][i:i + self.batch])
        out = g["acc"] * g["recip"]
        D, H, W = g["padded"]
        return out[:, a0:D - b0, a1:H - b1, a2:W - b2]

    @torch.no_grad()
    def segment(self, volume, overlap=0.25, blend="constant", tta=False):
        """do_inference / tta_inference of nn_unet.py:203-217 for one volume [5, Dv, Hv, Wv] -> fp32 logits [3, Dv, Hv, Wv]."""
        C.require_cuda(volume)
        if volume.dim() != 4 or volume.shape[0] != M.IN_CHANNELS:
            raise ValueError("BratsSegmenter.segment: volume is [%d, Dv, Hv, Wv] (got %s)" % (M.IN_CHANNELS, tuple(volume.shape)))
        if not 0.0 <= overlap < 1.0:
            raise ValueError("BratsSegmenter.segment: 0 <= overlap < 1")
        volume = volume.to(torch.float32)
        if not tta:
            return self._segment_once(volume, overlap, blend).clone()
        total = None
        for dims in TTA_FLIPS:                          # volume axes are the batch's axes minus one
            ax = [d - 1 for d in dims]
            pred = self._segment_once(torch.flip(volume, ax) if ax else volume, overlap, blend)
            pred = torch.flip(pred, ax) if ax else pred.clone()
            total = pred if total is None else total.add_(pred)
        return total.div_(len(TTA_FLIPS))
