"""MoFlowGenerator: MoFlow.reverse (model.py:205-236) and generate.py's infer() on the kernels of csrc/moflow.hip.

A reverse pass is 3 n_flow + 3 launches and no host read: dle_mf_squeeze_fwd, per bond flow (last to first) two dle_gemm (the folded
layers 1 and 2, bias + ReLU) and dle_mf_couple_fwd, then dle_mf_bond_decide_fwd and dle_mf_atom_reverse_fwd.  Rounding points: the
weights once (BatchNorm folded in fp32 first); the coupling's input half, the two hidden activations of a bond coupling, the atom
flow's aggregate and its three hidden activations once each; the flow states, s, t, exp and ActNorm stay fp32.
"""
import numpy as np
import torch

from .. import _cabi as C
from .. import functional as F
from ..utils.frontend import GraphCache, gpu_device, require_16bit
from . import model as M
from .mols import decode_predictions


class MoFlowGenerator:
    def __init__(self, model, dtype, graphs=False, device=None, max_workgroups=0, tile=32):
        require_16bit(dtype, "MoFlowGenerator")
        cfg = model.config
        M.check_bond_envelope(cfg)
        M.check_atom_envelope(cfg)
        dev = gpu_device(device, "MoFlowGenerator")
        a, b = cfg.model_config.atom_config, cfg.model_config.bond_config
        self.n, self.t, self.fold = cfg.max_num_nodes, cfg.num_node_features, b.n_squeeze
        if not F.mf_atom_supported(self.n, self.t, a.hidden_gnn, a.hidden_lin, a.n_flow, a.n_block, a.mask_row_size_list[0]):
            raise ValueError("the atom flow is outside dle_mf_atom_reverse_fwd's envelope (N %d, T %d, gnn %s, lin %s)" %
                             (self.n, self.t, list(a.hidden_gnn), list(a.hidden_lin)))
        self.config, self.dtype, self.device = cfg, dtype, dev
        self.positions = (self.n // self.fold) ** 2
        self.a_size, self.z_dim = self.n * self.t, cfg.z_dim
        self.unshift = cfg.model_config.noise_scale == 0
        self.hidden_gnn, self.hidden_lin, self.row_stride = list(a.hidden_gnn), list(a.hidden_lin), a.mask_row_stride_list[0]
        self.max_workgroups, self.tile = int(max_workgroups), int(tile)
        self.bond = []
        for f in M.folded_bond_flows(model):
            rec = {k: f[k].to(dev, dtype).contiguous() for k in ("w1", "w2", "w3")}
            rec.update({k: f[k].to(dev).contiguous() for k in ("b1", "b2", "b3", "scale", "loc")})
            rec["swap"] = f["swap"]
            self.bond.append(rec)
        w16, p32 = M.pack_atom_flows(model, dtype)
        self.w16, self.p32 = w16.to(dev), p32.to(dev)
        self._graphs = GraphCache(graphs)

    # the half a flow's first layer reads: the first half, the second when its halves swap
    @staticmethod
    def _a_half(flow):
        return 1 if flow["swap"] else 0

    def _reverse(self, z, want_h=False):
        b = z.shape[0]
        state, img = F.mf_squeeze_fwd(z[:, self.a_size:], self.n, self.fold, self._a_half(self.bond[-1]), self.dtype)
        for i in range(len(self.bond) - 1, -1, -1):
            f = self.bond[i]
            x = img.view(b, -1)
            h1 = F.gemm(x, f["w1"], b, f["w1"].shape[0], x.shape[1], True, True, bias=f["b1"], act=C.ACT_RELU)
            h2 = F.gemm(h1, f["w2"], b, f["w2"].shape[0], h1.shape[1], True, True, bias=f["b2"], act=C.ACT_RELU)
            nxt = self._a_half(self.bond[i - 1]) if i else None
            state, img = F.mf_couple_fwd(h2, f["w3"], f["b3"], f["scale"], f["loc"], state, self.positions, f["swap"], img_half=nxt,
                                         state_out=state)
        mask, code, adj, h_adj = F.mf_bond_decide_fwd(state, self.n, self.fold, self.unshift, want_adj=True, want_h=want_h)
        x = F.mf_atom_reverse_fwd(z[:, :self.a_size], mask, self.w16, self.p32, self.n, self.t, self.hidden_gnn, self.hidden_lin,
                                  self.row_stride, self.unshift, tile=self.tile, max_workgroups=self.max_workgroups)
        return (adj, x, mask, code) + ((h_adj,) if want_h else ())

    def _check_z(self, z):
        C.require_cuda(z)
        if z.dim() != 2 or z.shape[1] != self.z_dim or z.dtype != torch.float32 or not z.is_contiguous():
            raise ValueError("z must be a contiguous fp32 [batch, %d] tensor (got %s %s)" % (self.z_dim, z.dtype, tuple(z.shape)))

    def reverse_all(self, z, want_h=False):
        """-> (adj fp32 [B, 4, N, N] of 0 / 1, x fp32 [B, N, T], bit mask uint8 [B, N, N], bond code uint8 [B, N, N][, h_adj]).  With
        graphs the tensors live in buffers the captured graph owns: copy them before the next call of that batch size."""
        self._check_z(z)
        if z.shape[0] == 0:
            e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=z.device)
            out = (e(0, 4, self.n, self.n), e(0, self.n, self.t), e(0, self.n, self.n, dt=torch.uint8), e(0, self.n, self.n, dt=torch.uint8))
            return out + ((e(0, 4, self.n, self.n),) if want_h else ())
        return self._graphs.run(("reverse", z.shape[0], bool(want_h)), lambda zz: self._reverse(zz, want_h), z)

    def reverse(self, z):
        """MoFlow.reverse: z fp32 [B, z_dim] on the device -> (adj [B, 4, N, N], x [B, N, T]) as the reference returns them."""
        return self.reverse_all(z)[:2]

    def sample(self, batch_size, temperature=0.6, ln_var=0.0, generator=None):
        """generate.py's infer() up to the post-processing: z ~ N(0, sigma^2), sigma = temperature sqrt(exp(ln_var)), drawn on the
        device (from `generator`, a device generator, when given) -> (z, adj, x, bond code)."""
        sigma = float(temperature) * float(np.sqrt(np.exp(float(ln_var))))
        z = torch.randn((int(batch_size), self.z_dim), dtype=torch.float32, device=self.device, generator=generator) * sigma
        adj, x, _, code = self.reverse_all(z)
        return z, adj, x, code

    def decode(self, code, x):
        """postprocess_predictions (utils.py:47-63) on the device with one host read: bond code uint8 [B, N, N] (the argmax over the
        bond types) and x [B, N, T] -> (atomic numbers int64 [B, n], bond codes int64 [B, n, n]) as numpy, n = max_num_atoms."""
        return decode_predictions(code, x, self.config)
