"""MoFlow (reference: PyTorch/DrugDiscovery/MoFlow/moflow/model/{model,glow,coupling,basic}.py) as an nn.Module with the
reference's state-dict names and shapes, reverse direction only: what a checkpoint loads into, the perf baseline and the statement the
host tests hold the kernels' regroupings against.  It runs in whatever dtype its parameters have (float64 in the tests).

The second half is the weight packing of the generator (infer.py):
  * a 3x3 / pad 1 convolution on a G x G image, G <= 3, as the dense map [P Cin] -> [P Cout] of its live taps (fold_conv);
  * evaluation-mode BatchNorm folded into weight and bias IN FP32, before the one rounding of the weight to 16 bits;
  * the atom flow's row-only, aggregate-first form (folded_atom_flows): flow i touches row r = (i stride) % N only, and the graph
    convolution of that row is one [4 T + 4] -> gnn product of the masked aggregate and the per-type degrees.
"""
import torch
import torch.nn as nn

from .config import Config


class ActNorm(nn.Module):
    def __init__(self, num_channels, num_dims):
        super().__init__()
        shape = [1] * num_dims
        shape[1] = num_channels
        self.loc = nn.Parameter(torch.zeros(*shape))
        self.scale = nn.Parameter(torch.ones(*shape))
        self.register_buffer("initialized", torch.tensor(0, dtype=torch.uint8))
        self.register_buffer("num_elements", torch.tensor(0, dtype=torch.uint8))

    def reverse(self, y):
        return y / self.scale - self.loc


class AffineCoupling(nn.Module):
    def __init__(self, in_channel, hidden_channels, mask_swap):
        super().__init__()
        self.mask_swap = bool(mask_swap)
        layers, last = [], in_channel // 2
        for h in hidden_channels:
            layers += [nn.Conv2d(last, h, 3, padding=1), nn.BatchNorm2d(h), nn.ReLU()]
            last = h
        layers.append(nn.Conv2d(last, in_channel, 3, padding=1))
        self.layers = nn.Sequential(*layers)

    def reverse(self, y):
        a, b = y.chunk(2, 1)
        if self.mask_swap:
            a, b = b, a
        s, t = self.layers(a).chunk(2, 1)
        b = b * (1 + torch.exp(-s)) - t
        return torch.cat([b, a] if self.mask_swap else [a, b], 1)


class Flow(nn.Module):
    def __init__(self, in_channel, hidden_channels, conv_lu, mask_swap):
        super().__init__()
        if conv_lu != 2:
            raise ValueError("conv_lu %r is not built: only 2 (no invertible 1x1 convolution, the coupling halves swap)" % (conv_lu,))
        self.actnorm = ActNorm(in_channel, 4)
        self.coupling = AffineCoupling(in_channel, hidden_channels, mask_swap)

    def reverse(self, y):
        return self.actnorm.reverse(self.coupling.reverse(y))


def squeeze(x, fold):
    b, c, h, w = x.shape
    x = x.reshape(b, c, h // fold, fold, w // fold, fold).permute(0, 1, 3, 5, 2, 4)
    return x.reshape(b, c * fold * fold, h // fold, w // fold)


def unsqueeze(x, fold):
    b, c, h, w = x.shape
    x = x.reshape(b, c // (fold * fold), fold, fold, h, w).permute(0, 1, 4, 2, 5, 3)
    return x.reshape(b, c // (fold * fold), h * fold, w * fold)


class Block(nn.Module):
    def __init__(self, in_channel, n_flow, squeeze_fold, hidden_channels, conv_lu):
        super().__init__()
        self.squeeze_fold = squeeze_fold
        self.flows = nn.ModuleList(Flow(in_channel * squeeze_fold ** 2, hidden_channels, conv_lu, bool(i % 2)) for i in range(n_flow))

    def reverse(self, y):
        h = squeeze(y, self.squeeze_fold)
        for flow in reversed(self.flows):
            h = flow.reverse(h)
        return unsqueeze(h, self.squeeze_fold)


class Glow(nn.Module):
    def __init__(self, in_channel, n_flow, n_block, squeeze_fold, hidden_channel, conv_lu):
        super().__init__()
        self.blocks = nn.ModuleList(Block(in_channel, n_flow, squeeze_fold, hidden_channel, conv_lu) for _ in range(n_block))

    def reverse(self, z):
        for block in reversed(self.blocks):
            z = block.reverse(z)
        return z


class GraphConv(nn.Module):
    def __init__(self, in_channels, out_channels, num_atoms, num_edge_type=4):
        super().__init__()
        self.graph_linear_self = nn.Linear(in_channels, out_channels)
        self.graph_linear_edge = nn.Linear(in_channels, out_channels * num_edge_type)
        self.num_edge_type, self.out_ch, self.num_atoms = num_edge_type, out_channels, num_atoms

    def forward(self, adj, nodes):                     # nodes [B, N, 1, in]
        hs = self.graph_linear_self(nodes)
        m = self.graph_linear_edge(nodes).reshape(-1, self.num_atoms, self.out_ch, self.num_edge_type)
        return hs + torch.einsum("bemn,bnce->bmc", adj, m).unsqueeze(2)


class ConvCouplingBlock(nn.Module):
    def __init__(self, in_dim, out_dim, n_node):
        super().__init__()
        self.graph_conv = GraphConv(in_dim, out_dim, n_node)
        self.bn = nn.BatchNorm2d(n_node)
        self.relu = nn.ReLU()

    def forward(self, adj, h):
        return self.relu(self.bn(self.graph_conv(adj, h)))


class LinCouplingBlock(nn.Module):
    def __init__(self, in_dim, out_dim, n_node):
        super().__init__()
        self.lin = nn.Linear(in_dim, out_dim)
        self.bn = nn.BatchNorm2d(n_node)
        self.relu = nn.ReLU()

    def forward(self, h):
        return self.relu(self.bn(self.lin(h)))


class GraphAffineCoupling(nn.Module):
    def __init__(self, n_node, in_dim, hidden_gnn, hidden_lin, masked_row):
        super().__init__()
        self.masked_row = list(masked_row)
        conv, last = [], in_dim
        for d in hidden_gnn:
            conv.append(ConvCouplingBlock(last, d, n_node))
            last = d
        self.net_conv = nn.ModuleList(conv)
        lin = []
        for d in hidden_lin:
            lin.append(LinCouplingBlock(last, d, n_node))
            last = d
        lin.append(nn.Linear(last, in_dim * 2))
        self.net_lin = nn.Sequential(*lin)
        mask = torch.ones(n_node, in_dim)
        mask[self.masked_row, :] = 0
        self.register_buffer("mask", mask)

    def reverse(self, adj, y):
        masked = self.mask * y
        h = masked.unsqueeze(2)
        for layer in self.net_conv:
            h = layer(adj, h)
        s, t = self.net_lin(h).squeeze(2).chunk(2, dim=-1)
        return masked + (1 - self.mask) * (y * (1 + torch.exp(-s)) - t)


class FlowOnGraph(nn.Module):
    def __init__(self, n_node, in_dim, hidden_gnn, hidden_lin, masked_row):
        super().__init__()
        self.actnorm = ActNorm(n_node, 3)
        self.coupling = GraphAffineCoupling(n_node, in_dim, hidden_gnn, hidden_lin, masked_row)

    def reverse(self, adj, y):
        return self.actnorm.reverse(self.coupling.reverse(adj, y))


class BlockOnGraph(nn.Module):
    def __init__(self, n_node, in_dim, hidden_gnn, hidden_lin, n_flow, mask_row_size, mask_row_stride):
        super().__init__()
        if not 0 < mask_row_size < n_node:
            raise ValueError("mask_row_size must lie in (0, n_node)")
        self.flows = nn.ModuleList(
            FlowOnGraph(n_node, in_dim, hidden_gnn, hidden_lin,
                        [r % n_node for r in range(i * mask_row_stride, i * mask_row_stride + mask_row_size)]) for i in range(n_flow))

    def reverse(self, adj, y):
        for flow in reversed(self.flows):
            y = flow.reverse(adj, y)
        return y


def _per_block(values, n_block):
    values = list(values)
    if len(values) not in (1, n_block):
        raise ValueError("one value, or one per block")
    return values * n_block if len(values) == 1 else values


class GlowOnGraph(nn.Module):
    def __init__(self, n_node, in_dim, hidden_gnn, hidden_lin, n_flow, n_block, mask_row_size_list, mask_row_stride_list):
        super().__init__()
        sizes, strides = _per_block(mask_row_size_list, n_block), _per_block(mask_row_stride_list, n_block)
        self.blocks = nn.ModuleList(BlockOnGraph(n_node, in_dim, hidden_gnn, hidden_lin, n_flow, sizes[i], strides[i]) for i in range(n_block))

    def reverse(self, adj, z):
        for block in reversed(self.blocks):
            z = block.reverse(adj, z)
        return z


class MoFlowModel(nn.Module):
    def __init__(self, config: Config):
        super().__init__()
        self.config = config
        mc = config.model_config
        self.b_n_type, self.a_n_node, self.a_n_type = config.num_edge_features, config.max_num_nodes, config.num_node_features
        self.b_size = self.a_n_node ** 2 * self.b_n_type
        self.a_size = self.a_n_node * self.a_n_type
        self.noise_scale = mc.noise_scale
        b, a = mc.bond_config, mc.atom_config
        self.bond_model = Glow(self.b_n_type, b.n_flow, b.n_block, b.n_squeeze, b.hidden_ch, b.conv_lu)
        self.atom_model = GlowOnGraph(self.a_n_node, self.a_n_type, a.hidden_gnn, a.hidden_lin, a.n_flow, a.n_block,
                                      a.mask_row_size_list, a.mask_row_stride_list)

    def bond_reverse(self, z):
        """-> the bond model's output h_adj [B, 4, N, N], before the un-shift and the discretisation."""
        n = self.a_n_node
        return self.bond_model.reverse(z[:, self.a_size:].reshape(z.shape[0], self.b_n_type, n, n))

    def discretise(self, h_adj):
        if self.noise_scale == 0:
            h_adj = (h_adj + 0.5) * 2
        adj = ((h_adj + h_adj.permute(0, 1, 3, 2)) / 2).softmax(dim=1)
        return torch.floor(adj / adj.max(dim=1, keepdim=True).values)

    def atom_reverse(self, adj, z):
        h = self.atom_model.reverse(adj, z[:, :self.a_size].reshape(z.shape[0], self.a_n_node, self.a_n_type))
        return (h + 0.5) * 2 if self.noise_scale == 0 else h

    def reverse(self, z):
        """MoFlow.reverse (model.py:205-236): z [B, N T + 4 N N] -> (adj [B, 4, N, N] of 0 / 1, x [B, N, T])."""
        adj = self.discretise(self.bond_reverse(z))
        return adj, self.atom_reverse(adj, z)


# ---- packing ------------------------------------------------------------------------------------------------------------------------
def fold_conv(weight, grid):
    """Conv2d(3x3, padding 1) weight [O, I, 3, 3] on a grid x grid image -> the dense map [P, O, P, I] (output position, output channel,
    input position, input channel) of its live taps; zero where a tap does not reach."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError("fold_conv: a 3x3 convolution weight")
    if not 1 <= grid <= 3:
        raise ValueError("the folded bond convolution is built for a squeezed image of at most 3 x 3 positions (got %d x %d)" % (grid, grid))
    o, i = weight.shape[:2]
    dense = weight.new_zeros(grid * grid, o, grid * grid, i)
    for qy in range(grid):
        for qx in range(grid):
            for py in range(grid):
                for px in range(grid):
                    dy, dx = py - qy + 1, px - qx + 1
                    if 0 <= dy <= 2 and 0 <= dx <= 2:
                        dense[qy * grid + qx, :, py * grid + px, :] = weight[:, :, dy, dx]
    return dense


def _bn_affine(bn, dt):
    a = bn.weight.detach().to(dt) / torch.sqrt(bn.running_var.detach().to(dt) + bn.eps)
    return a, bn.bias.detach().to(dt) - bn.running_mean.detach().to(dt) * a


def check_bond_envelope(config):
    b = config.model_config.bond_config
    if b.conv_lu != 2:
        raise ValueError("conv_lu %r is not built: only 2" % (b.conv_lu,))
    if b.n_block != 1 or len(b.hidden_ch) != 2:
        raise ValueError("the bond flow is built for one block and two hidden convolutions (got %d, %s)" % (b.n_block, list(b.hidden_ch)))
    n = config.max_num_nodes
    if n % b.n_squeeze or (n // b.n_squeeze) ** 2 > 9:
        raise ValueError("the folded bond convolution needs (N / n_squeeze)^2 <= 9 positions (got N %d, n_squeeze %d)" % (n, b.n_squeeze))


def folded_bond_flows(model, dt=torch.float32):
    """Per bond flow, folded in `dt` (fp32 is what the generator rounds; float64 for the host tests):w1 [P h1, P C/2], b1, w2 [P h2, P h1], b2 (BatchNorm folded), w3 [2 M, P h2] (s rows, then t rows), b3 [2 M],
    scale / loc [C], swap."""
    check_bond_envelope(model.config)
    b = model.config.model_config.bond_config
    grid = model.a_n_node // b.n_squeeze
    p = grid * grid
    out = []
    for flow in model.bond_model.blocks[0].flows:
        L = flow.coupling.layers
        rec = {"swap": flow.coupling.mask_swap}
        for k, (ci, bi) in enumerate(((0, 1), (3, 4)), 1):
            a, c = _bn_affine(L[bi], dt)
            w = fold_conv(L[ci].weight.detach().to(dt) * a.view(-1, 1, 1, 1), grid)
            rec["w%d" % k] = w.reshape(p * w.shape[1], p * w.shape[3]).contiguous()
            rec["b%d" % k] = (L[ci].bias.detach().to(dt) * a + c).repeat(p)
        w = fold_conv(L[6].weight.detach().to(dt), grid)           # [P, C, P, h2]
        ch = w.shape[1] // 2
        rec["w3"] = torch.cat([w[:, :ch].reshape(p * ch, -1), w[:, ch:].reshape(p * ch, -1)]).contiguous()
        bias = L[6].bias.detach().to(dt)
        rec["b3"] = torch.cat([bias[:ch].repeat(p), bias[ch:].repeat(p)])
        rec["scale"] = flow.actnorm.scale.detach().to(dt).reshape(-1)
        rec["loc"] = flow.actnorm.loc.detach().to(dt).reshape(-1)
        out.append(rec)
    return out


def check_atom_envelope(config):
    a = config.model_config.atom_config
    if a.n_block != 1 or len(a.hidden_gnn) != 1 or len(a.hidden_lin) != 2 or list(a.mask_row_size_list) != [1]:
        raise ValueError("the atom flow is built for one block, one graph-convolution layer, two linear blocks and mask_row_size 1 "
                         "(got %d, %s, %s, %s)" % (a.n_block, list(a.hidden_gnn), list(a.hidden_lin), list(a.mask_row_size_list)))


def folded_atom_flows(model, dt=torch.float32):
    """Per atom flow, folded in `dt`, row-only and aggregate-first: row, wg [gnn, 4 T + 4] (column e T + t: edge type e, feature t; column
    4 T + e: the edge bias, multiplied by the degree), bg, w1, b1, w2, b2 (row r's BatchNorm affine folded), w3 [2 T, lin1], b3, scale
    / loc [N]."""
    check_atom_envelope(model.config)
    return fold_atom_model(model.atom_model, model.a_n_type, dt)


def fold_atom_model(atom_model, t, dt=torch.float32):
    """folded_atom_flows of a GlowOnGraph with one block, one graph-convolution layer, two linear blocks and mask_row_size 1."""
    out = []
    for flow in atom_model.blocks[0].flows:
        cp = flow.coupling
        r = cp.masked_row[0]
        gc = cp.net_conv[0].graph_conv
        d = gc.out_ch
        we = gc.graph_linear_edge.weight.detach().to(dt).reshape(d, 4, t)        # row c * 4 + e of the Linear
        be = gc.graph_linear_edge.bias.detach().to(dt).reshape(d, 4)
        a, c = _bn_affine(cp.net_conv[0].bn, dt)
        rec = {"row": r, "wg": torch.cat([we.reshape(d, 4 * t), be], 1) * a[r],
               "bg": gc.graph_linear_self.bias.detach().to(dt) * a[r] + c[r]}
        for k in (0, 1):
            a, c = _bn_affine(cp.net_lin[k].bn, dt)
            rec["w%d" % (k + 1)] = cp.net_lin[k].lin.weight.detach().to(dt) * a[r]
            rec["b%d" % (k + 1)] = cp.net_lin[k].lin.bias.detach().to(dt) * a[r] + c[r]
        rec["w3"] = cp.net_lin[2].weight.detach().to(dt)
        rec["b3"] = cp.net_lin[2].bias.detach().to(dt)
        rec["scale"] = flow.actnorm.scale.detach().to(dt).reshape(-1)
        rec["loc"] = flow.actnorm.loc.detach().to(dt).reshape(-1)
        out.append(rec)
    return out


def _up(v, m):
    return (v + m - 1) // m * m


def _fragment_order(w, rows, cols, dtype):
    """[r, c] fp32 -> zero padded to [rows, cols], rounded once, in MFMA fragment order [rows / 32][cols / 16][2][32][8]."""
    p = torch.zeros(rows, cols, dtype=torch.float32)
    p[:w.shape[0], :w.shape[1]] = w
    return p.to(dtype).reshape(rows // 32, 32, cols // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(-1)


def pack_atom_flows(model, dtype):
    """-> (w16 [n_flow, w_stride] in `dtype`, p32 [n_flow, p_stride] fp32) on the host, laid out as dle_mf_atom_reverse_fwd reads them."""
    return pack_folded_atom_flows(folded_atom_flows(model), dtype)


def pack_folded_atom_flows(flows, dtype):
    """The packing of folded_atom_flows' records (weights are rounded to `dtype` here, once)."""
    n, t = flows[0]["scale"].numel(), flows[0]["w3"].shape[0] // 2
    kg, d1, d2, d3 = _up(4 * t + 4, 16), _up(flows[0]["wg"].shape[0], 32), _up(flows[0]["w1"].shape[0], 32), _up(flows[0]["w2"].shape[0], 32)
    w16, p32 = [], []
    for f in flows:
        w3 = torch.zeros(32, f["w3"].shape[1])
        w3[:t], w3[16:16 + t] = f["w3"][:t], f["w3"][t:]
        b3 = torch.zeros(32)
        b3[:t], b3[16:16 + t] = f["b3"][:t], f["b3"][t:]
        w16.append(torch.cat([_fragment_order(f["wg"], d1, kg, dtype), _fragment_order(f["w1"], d2, d1, dtype),
                              _fragment_order(f["w2"], d3, d2, dtype), _fragment_order(w3, 32, d3, dtype)]))
        p = torch.zeros(_up(d1 + d2 + d3 + 32 + 2 * n, 4))
        for off, v in ((0, f["bg"]), (d1, f["b1"]), (d1 + d2, f["b2"]), (d1 + d2 + d3, b3), (d1 + d2 + d3 + 32, f["scale"]),
                       (d1 + d2 + d3 + 32 + n, f["loc"])):
            p[off:off + v.numel()] = v
        p32.append(p)
    return torch.stack(w16), torch.stack(p32)
