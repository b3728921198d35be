"""Writes tests/golden/tacotron2_infer.npz from the REFERENCE's own Tacotron2.infer (CPU, fp32, eval mode).  Needs the reference
tree (oracle/_ref_import.py, DLE_REFERENCE); run once where it is mounted:

    python tools/make_tacotron2_infer_golden.py

Model: oracle.tacotron2_oracle.TACOTRON2_SMALL with seeded_state + seeded_running_stats (the first seed of MODEL_SEEDS that admits the margin below).  For the duration of the call
F.dropout as the reference's prenet sees it is replaced by a function that applies the masks of the RNG contract
(include/dle_mi355x.h): call 2 t + l of the run -> philox_oracle.keep_mask(B * P, 0.5, SEED, 1 + 2 t + l), kept values x 2.
  (a) batch 3, text lengths 23 / 19 / 12, early stopping: the three samples stop at three different steps, the last below 40;
  (b) the same model with a max_decoder_steps that cuts the run before any gate fires.
Free-running decoding amplifies rounding, and a gate logit near the threshold would make the stop step arbitrary.  The decoder's
trajectory does not depend on the gate layer (only the mel frame is fed back), so the tool runs it once in fp32 and once with the
operands rounded to bf16 at the engine's storage points (tests/_tacotron2_infer_doubles.py), both for 40 steps, and searches the
gate layer's seed, scale and bias for the draw with the best margin: at every (step, sample) up to the sample's stop,
|logit - logit(threshold)| >= 10 x the largest gate-logit deviation of the bf16 run over the same positions.  It asserts that
margin and stores it.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _ref_import as R                                      # noqa: E402
from oracle import philox_oracle as PO                                   # noqa: E402
from oracle import tacotron2_oracle as TO                                # noqa: E402
from tests import _tacotron2_infer_doubles as DI                         # noqa: E402

MODEL_SEEDS, RNG_SEED, TEXT_LENGTHS, HORIZON, MARGIN = range(17, 33), 1234, [23, 19, 12], 40, 10.0
GATE_SEEDS, GATE_SCALE = 20000, 8.0


def case_text(cfg):
    rng = np.random.default_rng(217)
    text = np.zeros((len(TEXT_LENGTHS), max(TEXT_LENGTHS)), np.int64)
    for i, n in enumerate(TEXT_LENGTHS):
        text[i, :n] = rng.integers(1, cfg["n_symbols"], n)
    return torch.from_numpy(text), torch.tensor(TEXT_LENGTHS, dtype=torch.int64)


def search_gate(cfg, text, lengths, model_seed):
    """-> (gate_seed, scale, bias, margin, deviation, stops) of the best draw."""
    p = DI.full_state(cfg, model_seed)
    t32, t16 = [], []
    DI.infer(p, cfg, text, lengths, RNG_SEED, max_decoder_steps=HORIZON, early_stopping=False, trace=t32)
    DI.infer(p, cfg, text, lengths, RNG_SEED, max_decoder_steps=HORIZON, early_stopping=False, store=torch.bfloat16, trace=t16)
    h32, h16 = torch.stack(t32).double(), torch.stack(t16).double()      # [T, B, Hd + E]
    best = None
    t_idx = torch.arange(h32.shape[0])[None, :, None]
    for gs in range(GATE_SEEDS):
        w = np.random.default_rng(gs).standard_normal((1, h32.shape[2])) / np.sqrt(h32.shape[2]) * GATE_SCALE
        w32 = torch.from_numpy(w.astype(np.float32))
        l32 = (h32 @ w32.double().t()).squeeze(2)                        # [T, B]
        dl = ((h16 @ w32.bfloat16().double().t()).squeeze(2) - l32).abs()
        biases = torch.linspace(-float(l32.max()), -float(l32.min()), 400, dtype=torch.float64).view(-1, 1, 1)
        lb = l32[None] + biases                                          # [n_bias, T, B]
        fire = lb > 0                                                    # sigmoid(x) <= 0.5  <=>  x <= 0
        stops = fire.to(torch.int8).argmax(1)                            # first firing step of every sample, [n_bias, B]
        ok = fire.any(1).all(1) & (stops.min(1).values >= 6) & (stops.max(1).values + 1 < HORIZON)
        srt = stops.sort(1).values
        ok &= (srt[:, 1:] != srt[:, :-1]).all(1)
        if not bool(ok.any()):
            continue
        live = t_idx <= stops[:, None, :]
        margin = lb.abs().masked_fill(~live, float("inf")).amin((1, 2))
        dev = (dl[None] * live).amax((1, 2))
        ratio = (margin / dev).masked_fill(~ok, 0.0)
        i = int(ratio.argmax())
        if best is None or float(ratio[i]) > best[3] / best[4]:
            # the bias as the fp32 value the model holds: margin and stops are re-derived from it below
            best = (gs, GATE_SCALE, float(np.float32(biases[i].item())), float(margin[i]), float(dev[i]), stops[i].tolist())
    return best


def reference_infer(model, text, lengths, cfg):
    import torch.nn.functional as TF
    calls = [0]
    b, pdim = text.shape[0], cfg["prenet_dim"]

    def dropout(x, p=0.5, training=True, inplace=False):
        if not training:
            return x
        t, layer = divmod(calls[0], 2)
        calls[0] += 1
        assert p == 0.5 and tuple(x.shape) == (b, pdim)
        return x * DI.keep_mask(b, pdim, RNG_SEED, t, layer) * float(PO.inv_keep(0.5))
    real, dec_infer, gates = TF.dropout, model.decoder.infer, []

    def keep_gates(*a, **kw):                                            # Tacotron2.infer drops Decoder.infer's gate energies
        out = dec_infer(*a, **kw)
        gates.append(out[1])
        return out
    TF.dropout, model.decoder.infer = dropout, keep_gates
    try:
        with torch.no_grad():
            post, mel_lengths, aligns = model.infer(text, lengths)
    finally:
        TF.dropout, model.decoder.infer = real, dec_infer
    assert calls[0] == 2 * post.shape[2], (calls[0], post.shape)
    return post, mel_lengths, aligns, gates[0].reshape(post.shape[2], b).t().contiguous()


def main():
    if not R.have_reference():
        raise SystemExit("the reference tree is not mounted (DLE_REFERENCE)")
    ref = R.import_tacotron2()
    cfg = TO.TACOTRON2_SMALL
    text, lengths = case_text(cfg)
    for model_seed in MODEL_SEEDS:                                       # the first model seed whose best gate draw has the margin
        gs, scale, bias, margin, dev, stops = search_gate(cfg, text, lengths, model_seed)
        print("model seed %d, gate seed %d scale %.1f bias %.4f: stops %s, margin %.4f, bf16 deviation %.5f, ratio %.1f" % (
            model_seed, gs, scale, bias, stops, margin, dev, margin / dev), flush=True)
        if margin >= MARGIN * dev:
            break
    assert margin >= MARGIN * dev, (margin, dev)
    p = DI.full_state(cfg, model_seed, gs, scale, bias)
    cut = min(stops) - 1                                                # case (b): steps 0 .. cut - 1, no gate has fired
    arrs = dict(text=text.numpy(), text_lengths=lengths.numpy(), seed=np.asarray([RNG_SEED], np.int64),
                model_seed=np.asarray([model_seed], np.int64), gate_seed=np.asarray([gs], np.int64),
                gate_scale=np.asarray([scale], np.float64), gate_bias=np.asarray([bias], np.float64),
                margin=np.asarray([margin], np.float64), bf16_deviation=np.asarray([dev], np.float64),
                b_max_decoder_steps=np.asarray([cut], np.int64))
    for tag, max_steps in (("a", 2000), ("b", cut)):
        model = ref.model.Tacotron2(mask_padding=False, max_decoder_steps=max_steps, gate_threshold=0.5,
                                    decoder_no_early_stopping=False, **cfg)
        model.load_state_dict(p, strict=False)
        model.eval()
        post, ml, al, gate = reference_infer(model, text, lengths, cfg)
        got = DI.infer(p, cfg, text, lengths, RNG_SEED, max_decoder_steps=max_steps)
        assert post.shape == got[0].shape and torch.equal(ml, got[1]), (post.shape, got[0].shape, ml, got[1])
        print("case %s: T %d, mel_lengths %s; statement vs reference: mel max abs %.3e, alignments max abs %.3e" % (
            tag, post.shape[2], ml.tolist(), float((got[0] - post).abs().max()), float((got[2] - al).abs().max())),
              "gate max abs %.3e" % float((got[3] - gate).abs().max()))
        arrs.update({tag + "_mel_post": post.numpy(), tag + "_mel_lengths": ml.numpy(), tag + "_alignments": al.numpy(),
                     tag + "_gate": gate.numpy()})
    assert arrs["a_mel_lengths"].tolist() == [s for s in stops] and arrs["a_mel_post"].shape[2] == max(stops) + 1
    path = os.path.join(ROOT, "tests", "golden", "tacotron2_infer.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, {k: v.shape for k, v in arrs.items()}, "%d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
