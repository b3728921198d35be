"""TEST DOUBLES (tests/ only) for WaveGlow inference: plain-torch statements of
  * `flow_inv` / `flow_inv_first`: what dle_wg_flow_inv(_first) compute on the [M, 8] flow state (csrc/waveglow.hip), and
  * `infer`: WaveGlow.infer / infer_onnx (waveglow/model.py:234-315) in the reference's own [B, C, T] layout with explicit noise,
    `forward_z`: the forward flow (model.py:189-232) over the same WN statement, for round trips.
`work` is the arithmetic dtype (torch.float64 accumulates every contraction in fp64), `store` an optional 16-bit dtype applied at
exactly the points where the engine keeps 16 bits: GEMM weight operands, the mel, the upsampled spectrogram, the cond / in-layer
pre-activations, the gate output, both res_skip halves and the `start` operand a0.  The flow state, `end`'s output (b | log_s),
biases and W^-1 stay fp32 in the engine and are not rounded here.  The product never imports this file.
"""
import torch
import torch.nn.functional as TF


def flow_inv_first(noise, c, sigma, dtype):
    out = torch.zeros_like(noise)
    out[:, 8 - c:] = sigma * noise[:, :c]
    a0 = torch.zeros((noise.shape[0], 8), dtype=dtype)
    a0[:, :c // 2] = out[:, 8 - c:8 - c + c // 2].to(dtype)
    return out, a0


def flow_inv(state, o, winv_t, c, next_c=0, early=0, noise=None, z_col=0, sigma=1.0, dtype=torch.float16):
    """-> (new state, a0 or None); state / o / noise [M, 8] of one floating dtype, winv_t = (W^-1)^T flattened (c*c values)."""
    off, nh = 8 - c, c // 2
    a = state[:, off:].clone()
    a[:, nh:] = (a[:, nh:] - o[:, :nh]) * torch.exp(-o[:, nh:2 * nh])
    out = state.clone()
    out[:, off:] = a @ winv_t.reshape(-1)[:c * c].view(c, c).to(state.dtype)        # new[:, j] = sum_i a[:, i] W^-1[j, i]
    if early:
        out[:, off - early:off] = sigma * noise[:, z_col:z_col + early]
    a0 = None
    if next_c:
        a0 = torch.zeros((state.shape[0], 8), dtype=dtype)
        a0[:, :next_c // 2] = out[:, 8 - next_c:8 - next_c + next_c // 2].to(dtype)
    return out, a0


# ---------------------------------------------------------------- the whole network, reference layout
def _q(t, store, work):
    return (t.to(store) if store is not None else t).to(work)


def _wn_weight(p, name):
    v, g = p[name + ".weight_v"].float(), p[name + ".weight_g"].float()
    return v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1))            # fp32, as dle_wg_weight_norm_fwd forms it


def wn(p, pre, a0, spect, cfg, store, work):
    """WN.forward (model.py:138-157): a0 [B, n_half, T'] (already rounded to `store`), spect [B, 640, T'] -> (b | log_s)."""
    w, nc, ks = cfg["WN_config"], cfg["WN_config"]["n_channels"], cfg["WN_config"]["kernel_size"]
    q = lambda t: _q(t, store, work)
    wt = lambda name: q(_wn_weight(p, pre + name))
    bias = lambda name: p[pre + name + ".bias"].to(work)
    x = q(TF.conv1d(a0, wt("start"), bias("start")))
    skip = None
    for i in range(w["n_layers"]):
        d = 2 ** i
        cond = q(TF.conv1d(spect, wt("cond_layers.%d" % i), bias("cond_layers.%d" % i)))
        s = q(TF.conv1d(x, wt("in_layers.%d" % i), bias("in_layers.%d" % i), dilation=d, padding=(ks * d - d) // 2) + cond)
        acts = q(torch.tanh(s[:, :nc]) * torch.sigmoid(s[:, nc:]))
        rs = TF.conv1d(acts, wt("res_skip_layers.%d" % i), bias("res_skip_layers.%d" % i))
        if i < w["n_layers"] - 1:
            x = q(rs[:, :nc] + x)
            rs = rs[:, nc:]
        skip = q(rs if skip is None else rs + skip)
    return TF.conv1d(skip, q(p[pre + "end.weight"].float()), bias("end"))


def _spect(p, cfg, mel, samples, store, work):
    """Upsampling + grouping (model.py:236-243): -> [B, 640, samples / 8] with channel = mel * 8 + g."""
    q = lambda t: _q(t, store, work)
    ng = cfg["n_group"]
    up = TF.conv_transpose1d(q(mel), q(p["upsample.weight"].float()), p["upsample.bias"].to(work), stride=256)
    up = q(up[:, :, :samples])
    up = up.unfold(2, ng, ng).permute(0, 2, 1, 3)
    return up.contiguous().view(up.size(0), up.size(1), -1).permute(0, 2, 1)


def _winv(p, k, work):
    w = p["convinv.%d.conv.weight" % k].squeeze(-1)
    return torch.linalg.inv(w.double()).float().to(work)                 # fp64 Gauss-Jordan, kept in fp32 (dle_wg_logdet_inv)


def n_remaining(cfg):
    return cfg["n_group"] - cfg["n_early_size"] * len([k for k in range(1, cfg["n_flows"]) if k % cfg["n_early_every"] == 0])


def infer(p, cfg, mel, z, sigma, store=None, work=torch.float64):
    """mel [B, 80, frames], z [B, 8, frames*32] (infer_onnx's layout) -> audio [B, frames*256] in `work`."""
    spect = _spect(p, cfg, mel, mel.shape[2] * 256, store, work)
    n_rem, es = n_remaining(cfg), cfg["n_early_size"]
    z = z.to(work)
    audio, rest = sigma * z[:, :n_rem], z[:, n_rem:]
    for k in reversed(range(cfg["n_flows"])):
        nh = audio.size(1) // 2
        a0, a1 = audio[:, :nh], audio[:, nh:]
        o = wn(p, "WN.%d." % k, _q(a0, store, work), spect, cfg, store, work)
        a1 = (a1 - o[:, :nh]) * torch.exp(-o[:, nh:])
        audio = TF.conv1d(torch.cat([a0, a1], 1), _winv(p, k, work).unsqueeze(-1))
        if k % cfg["n_early_every"] == 0 and k > 0:
            audio = torch.cat((sigma * rest[:, :es], audio), 1)
            rest = rest[:, es:]
    return audio.permute(0, 2, 1).contiguous().view(audio.size(0), -1)


def forward_z(p, cfg, mel, audio, store=None, work=torch.float64):
    """The forward flow (model.py:189-232): -> z [B, 8, T/8] in the FORWARD's channel order (early outputs first)."""
    ng = cfg["n_group"]
    spect = _spect(p, cfg, mel, audio.shape[1], store, work)
    a = audio.to(work).unfold(1, ng, ng).permute(0, 2, 1)
    outs = []
    for k in range(cfg["n_flows"]):
        if k % cfg["n_early_every"] == 0 and k > 0:
            outs.append(a[:, :cfg["n_early_size"]])
            a = a[:, cfg["n_early_size"]:]
        a = TF.conv1d(a, p["convinv.%d.conv.weight" % k].to(work))
        nh = a.size(1) // 2
        a0, a1 = a[:, :nh], a[:, nh:]
        o = wn(p, "WN.%d." % k, _q(a0, store, work), spect, cfg, store, work)
        a = torch.cat([a0, torch.exp(o[:, nh:]) * a1 + o[:, :nh]], 1)
    outs.append(a)
    return torch.cat(outs, 1)


def noise_in_forward_order(z, cfg, sigma):
    """infer's z [B, 8, T'] (initial channels, then the early draws in the order the REVERSE loop uses them) -> sigma * z with the
    channels where the forward flow emits them: the early output of the smallest k first, the final channels last."""
    n_rem, es = n_remaining(cfg), cfg["n_early_size"]
    parts, col = [z[:, :n_rem]], n_rem
    while col < cfg["n_group"]:
        parts.insert(0, z[:, col:col + es])
        col += es
    return sigma * torch.cat(parts, 1)
