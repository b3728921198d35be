"""TEST DOUBLES (tests/ only) for Tacotron2 inference, on top of tests/_tacotron2_doubles.py:
  * `prenet_infer` / `frame_infer`: plain-torch statements of dle_t2_prenet_infer / dle_t2_frame_infer (csrc/tacotron2.hip), with
    the device step words emulated on CPU tensors;
  * `infer`: Tacotron2.infer (tacotron2/model.py:678-691; Decoder.infer :515-595) in plain torch with the prenet masks of the RNG
    contract (include/dle_mi355x.h): step t, layer l -> oracle.philox_oracle.keep_mask(B * P, 0.5, seed, 1 + 2 t + l).
`work` is the arithmetic dtype, `store` an optional 16-bit dtype applied at exactly the points where the engine keeps 16 bits:
GEMM weight operands, embedding rows, every convolution / BatchNorm / tanh output, the LSTM gate pre-activations and hidden states,
the encoder memory and processed memory, the decoder input frame, both prenet layers, the tanh inside the attention, the (previous,
cumulative) attention weights, the context, and the postnet's input.  Cell states, the query, energies, attention weights, the mel
frame and the gate logit stay fp32 in the engine and are not rounded here.  The product never imports this file.
"""
import numpy as np
import torch
import torch.nn.functional as TF

from oracle import philox_oracle as PO
from tests import _tacotron2_doubles as D


def keep_mask(b, p_dim, seed, t, layer):
    return torch.from_numpy(PO.keep_mask(b * p_dim, 0.5, seed, 1 + 2 * t + layer)).view(b, p_dim)


# ---------------------------------------------------------------- the two new C-ABI calls
def prenet_infer(frame, w0, w1, dst, seed, step_word, mask0=None, mask1=None):
    b, p = dst.shape
    t = int(step_word.reshape(-1)[0])
    dt = dst.dtype
    x = torch.zeros(b, w0.shape[1], dtype=dt) if frame is None else frame.to(dt)
    out = x
    for layer, (w, m_out) in enumerate(((w0, mask0), (w1, mask1))):
        keep = keep_mask(b, p, seed, t, layer)
        y = torch.relu((out.double() @ w.double().t()).float()).to(dt)
        out = (y.float() * keep * float(PO.inv_keep(0.5))).to(dt)
        if m_out is not None:
            m_out.copy_(D._pack(keep))
    dst.copy_(out)


def frame_infer(hc, w, bias, mel_out, gate_out, frame_next, not_finished, mel_lengths, state, parity, gate_threshold, max_steps,
                prenet=None, seed=0):
    b, steps, nm = mel_out.shape
    t = int(state[parity])
    out = (hc.double() @ w.double()[:nm + 1].t()).float() + bias[:nm + 1]
    frame_next.copy_(out[:, :nm])
    if 0 <= t < max_steps and t < steps:
        mel_out[:, t].copy_(out[:, :nm])
        gate_out[:, t].copy_(out[:, nm])
        dec = (torch.sigmoid(out[:, nm]) <= gate_threshold).to(torch.int32)
        not_finished.mul_(dec)
        mel_lengths.add_(not_finished)
        if int(state[3]) == 0:
            state[2] = t + 1
            if int(not_finished.sum()) == 0:
                state[3] = 1
    state[1 - parity] = t + 1
    if prenet is not None:
        w0, w1, dst = prenet
        prenet_infer(frame_next, w0, w1, dst, seed, state[1 - parity:])


def install(monkeypatch):
    """The doubles for every C-ABI call Tacotron2Synthesizer makes."""
    from deeplearningexamples_amd.tacotron2 import ops
    D.install(monkeypatch)
    monkeypatch.setattr(ops, "prenet_infer", prenet_infer)
    monkeypatch.setattr(ops, "frame_infer", frame_infer)


# ---------------------------------------------------------------- the whole network, reference layout
def _q(t, store, work):
    return (t.to(store) if store is not None else t).to(work)


def _bn_eval(x, p, name, work):
    rstd = torch.rsqrt(p[name + ".running_var"].float() + 1e-5).to(work).view(1, -1, 1)
    return ((x - p[name + ".running_mean"].to(work).view(1, -1, 1)) * rstd * p[name + ".weight"].to(work).view(1, -1, 1)
            + p[name + ".bias"].to(work).view(1, -1, 1))


def _cell(g, c):
    i, f, gg, o = g.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def _lstm_dir(x, lengths, p, reverse, q, work):
    sfx = "_reverse" if reverse else ""
    w_ih, w_hh = q(p["encoder.lstm.weight_ih_l0" + sfx].float()), q(p["encoder.lstm.weight_hh_l0" + sfx].float())
    bias = (p["encoder.lstm.bias_ih_l0" + sfx].float() + p["encoder.lstm.bias_hh_l0" + sfx].float()).to(work)
    b, t, _ = x.shape
    hd = w_hh.shape[1]
    gx = q(x @ w_ih.t() + bias)
    h, c = torch.zeros(b, hd, dtype=work), torch.zeros(b, hd, dtype=work)
    outs = [None] * t
    for step in (range(t - 1, -1, -1) if reverse else range(t)):
        h2, c2 = _cell(q(h @ w_hh.t() + gx[:, step]), c)
        h2 = q(h2)
        live = (step < lengths).to(work).unsqueeze(1)
        h, c = live * h2 + (1 - live) * h, live * c2 + (1 - live) * c
        outs[step] = live * h2
    return torch.stack(outs, dim=1)


def encoder(p, cfg, text, lengths, store=None, work=torch.float32):
    q = lambda t: _q(t, store, work)
    x = q(TF.embedding(text, p["embedding.weight"].float())).transpose(1, 2)
    for i in range(cfg["encoder_n_convolutions"]):
        pre = "encoder.convolutions.%d." % i
        k = p[pre + "0.conv.weight"].shape[2]
        x = q(TF.conv1d(x, q(p[pre + "0.conv.weight"].float()), p[pre + "0.conv.bias"].to(work), padding=(k - 1) // 2))
        x = q(torch.relu(_bn_eval(x, p, pre + "1", work)))
    x = x.transpose(1, 2)
    return torch.cat([_lstm_dir(x, lengths, p, False, q, work), _lstm_dir(x, lengths, p, True, q, work)], dim=2)


def location_matrix(p, q):
    """Location conv [F, 2, KL] and dense [A, F] pre-multiplied into one [A, 2, KL] kernel, as the engine's `loc2` operand."""
    att = "decoder.attention_layer."
    wc = q(p[att + "location_layer.location_conv.conv.weight"].float())
    wd = q(p[att + "location_layer.location_dense.linear_layer.weight"].float())
    return q(torch.einsum("af,fck->ack", wd, wc))


def decoder(p, cfg, memory, lengths, seed, max_decoder_steps=2000, gate_threshold=0.5, early_stopping=True, store=None,
            work=torch.float32, trace=None):
    """Decoder.infer.  -> (mel [B, T, n_mel], gate [B, T], alignments [B, T, Ti], mel_lengths int32 [B]).  trace (list): receives
    [decoder_hidden | context] of every step (the gate layer's input)."""
    q = lambda t: _q(t, store, work)
    b, ti, _ = memory.shape
    P, nm = cfg["prenet_dim"], cfg["n_mel_channels"]
    att = "decoder.attention_layer."
    W = lambda name: q(p[name].float())
    pre0, pre1 = W("decoder.prenet.layers.0.linear_layer.weight"), W("decoder.prenet.layers.1.linear_layer.weight")
    wa = torch.cat([W("decoder.attention_rnn.weight_ih"), W("decoder.attention_rnn.weight_hh")], dim=1)
    ba = (p["decoder.attention_rnn.bias_ih"].float() + p["decoder.attention_rnn.bias_hh"].float()).to(work)
    wd = torch.cat([W("decoder.decoder_rnn.weight_ih"), W("decoder.decoder_rnn.weight_hh")], dim=1)
    bd = (p["decoder.decoder_rnn.bias_ih"].float() + p["decoder.decoder_rnn.bias_hh"].float()).to(work)
    wq, v = W(att + "query_layer.linear_layer.weight"), p[att + "v.linear_layer.weight"].to(work).view(-1)
    pm = q(memory @ W(att + "memory_layer.linear_layer.weight").t())
    wloc = location_matrix(p, q)
    kl = wloc.shape[2]
    wp = torch.cat([W("decoder.linear_projection.linear_layer.weight"), W("decoder.gate_layer.linear_layer.weight")], dim=0)
    bp = torch.cat([p["decoder.linear_projection.linear_layer.bias"], p["decoder.gate_layer.linear_layer.bias"]]).to(work)
    pad = torch.arange(ti)[None, :] >= lengths[:, None]
    ah, ac = torch.zeros(b, cfg["attention_rnn_dim"], dtype=work), torch.zeros(b, cfg["attention_rnn_dim"], dtype=work)
    dh, dc = torch.zeros(b, cfg["decoder_rnn_dim"], dtype=work), torch.zeros(b, cfg["decoder_rnn_dim"], dtype=work)
    aw16 = cum16 = torch.zeros(b, ti, dtype=work)
    ctx = torch.zeros(b, memory.shape[2], dtype=work)
    frame = torch.zeros(b, nm, dtype=work)
    not_finished, mel_lengths = torch.ones(b, dtype=torch.int32), torch.zeros(b, dtype=torch.int32)
    scale = float(PO.inv_keep(0.5))
    mels, gates, aligns = [], [], []
    while True:
        t = len(mels)
        x = q(frame)
        for layer, w in enumerate((pre0, pre1)):
            x = q(torch.relu(x @ w.t()))
            x = q(x * keep_mask(b, P, seed, t, layer).to(work) * scale)
        ah, ac = _cell(q(torch.cat([x, ctx, ah], dim=1) @ wa.t() + ba), ac)
        ah = q(ah)
        loc = TF.conv1d(torch.stack([aw16, cum16], dim=1), wloc, padding=(kl - 1) // 2).transpose(1, 2)
        th = q(torch.tanh((ah @ wq.t()).unsqueeze(1) + pm + loc))
        aw = torch.softmax((th @ v).masked_fill(pad, -float("inf")), dim=1)
        ctx = q(torch.bmm(aw.unsqueeze(1), memory).squeeze(1))
        aw16, cum16 = q(aw), q(cum16 + aw)
        dh, dc = _cell(q(torch.cat([ah, ctx, dh], dim=1) @ wd.t() + bd), dc)
        dh = q(dh)
        hc = torch.cat([dh, ctx], dim=1)
        if trace is not None:
            trace.append(hc)
        out = hc @ wp.t() + bp
        frame = out[:, :nm]
        mels.append(frame)
        gates.append(out[:, nm])
        aligns.append(aw)
        dec = (torch.sigmoid(out[:, nm].float()) <= gate_threshold).to(torch.int32)
        not_finished = not_finished * dec
        mel_lengths = mel_lengths + not_finished
        if early_stopping and int(not_finished.sum()) == 0:
            break
        if len(mels) == max_decoder_steps:
            break
    return torch.stack(mels, dim=1), torch.stack(gates, dim=1), torch.stack(aligns, dim=1), mel_lengths


def postnet(p, cfg, mel, store=None, work=torch.float32):
    """mel [B, T, n_mel] -> mel + postnet(mel), [B, n_mel, T]."""
    q = lambda t: _q(t, store, work)
    npc = cfg["postnet_n_convolutions"]
    y = q(mel).transpose(1, 2)
    for i in range(npc):
        pre = "postnet.convolutions.%d." % i
        k = p[pre + "0.conv.weight"].shape[2]
        y = q(TF.conv1d(y, q(p[pre + "0.conv.weight"].float()), p[pre + "0.conv.bias"].to(work), padding=(k - 1) // 2))
        y = q(_bn_eval(y, p, pre + "1", work))
        if i < npc - 1:
            y = q(torch.tanh(y))
    return mel.transpose(1, 2) + y


def infer(p, cfg, text, lengths, seed, max_decoder_steps=2000, gate_threshold=0.5, early_stopping=True, store=None,
          work=torch.float32, trace=None):
    """-> (mel_outputs_postnet [B, n_mel, T], mel_lengths int32 [B], alignments [B, T, Ti], gate logits [B, T]) in `work`."""
    with torch.no_grad():
        memory = encoder(p, cfg, text, lengths, store, work)
        mel, gate, aligns, mel_lengths = decoder(p, cfg, memory, lengths, seed, max_decoder_steps, gate_threshold, early_stopping,
                                                 store, work, trace)
        return postnet(p, cfg, mel, store, work), mel_lengths, aligns, gate


def full_state(cfg, seed, gate_seed=None, gate_scale=1.0, gate_bias=None):
    """oracle seeded_state + seeded_running_stats; gate_seed: the gate layer's weight redrawn from its own stream (N(0, 1) / sqrt(fan
    in) x gate_scale) and its bias set to gate_bias -- what tools/make_tacotron2_infer_golden.py searched over."""
    from oracle import tacotron2_oracle as TO
    st = dict(TO.seeded_state(cfg, seed))
    st.update(TO.seeded_running_stats(cfg, seed))
    if gate_seed is not None:
        name = "decoder.gate_layer.linear_layer."
        shape = st[name + "weight"].shape
        w = np.random.default_rng(int(gate_seed)).standard_normal(shape) / np.sqrt(shape[1]) * gate_scale
        st[name + "weight"] = torch.from_numpy(w.astype(np.float32))
        st[name + "bias"] = torch.full((1,), float(gate_bias), dtype=torch.float32)
    return st
