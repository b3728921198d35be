"""Entry point mirroring SpeechSynthesis/Tacotron2/inference.py: text -> mel spectrogram -> audio files.

    python -m deeplearningexamples_amd.tacotron2.inference -i phrases.txt --tacotron2 checkpoint_Tacotron2_last.pt \
        --waveglow checkpoint_WaveGlow_last.pt -o audio/ --fp16

The flag names are the reference's (inference.py:46-77) plus --amp-dtype and --seed (the stream of the prenet's dropout masks,
which stay on at inference).  The phrases of the text file (one per line) go through text_to_sequence(english_cleaners), are
sorted by length and zero padded as prepare_input_sequence does (inference.py:141-172), then Tacotron2Synthesizer ->
WaveGlowVocoder -> Denoiser.  Writes audio_<n><suffix>.wav (16-bit PCM, trimmed to mel_lengths * hop, scaled to full range as the
reference does) and the reference's DLLogger records (tacotron2_items_per_sec, tacotron2_latency, waveglow_items_per_sec,
waveglow_latency, denoiser_latency, latency).  Without --waveglow the mel tensors are saved instead (mel_<n><suffix>.pt).  The
checkpoints are the files the train entry points write, or the reference's own.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from ..utils import dllogger as DLLogger
from ..waveglow.inference import load_model as load_waveglow
from ..waveglow.inference import write_wav
from .model import DEFAULT_CONFIG, Tacotron2
from .text import text_to_sequence


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Tacotron2 + WaveGlow inference on MI355X (text to speech)", allow_abbrev=False)
    p.add_argument("-i", "--input", type=str, required=True, help="full path to the input text (phrases separated by new line)")
    p.add_argument("-o", "--output", required=True, help="output folder to save audio (file per phrase)")
    p.add_argument("--suffix", type=str, default="", help="output filename suffix")
    p.add_argument("--tacotron2", type=str, default=None, help="full path to the Tacotron2 model checkpoint file")
    p.add_argument("--waveglow", type=str, default=None, help="full path to the WaveGlow model checkpoint file")
    p.add_argument("-s", "--sigma-infer", default=0.9, type=float)
    p.add_argument("-d", "--denoising-strength", default=0.01, type=float, help="0 skips the denoiser")
    p.add_argument("-sr", "--sampling-rate", default=22050, type=int, help="Sampling rate")
    mode = p.add_mutually_exclusive_group()
    mode.add_argument("--fp16", action="store_true", help="16-bit storage in fp16 (the default of this path)")
    mode.add_argument("--cpu", action="store_true", help="there is no CPU path")
    p.add_argument("--log-file", type=str, default="nvlog.json", help="Filename for logging")
    p.add_argument("--include-warmup", action="store_true", help="Include warmup")
    p.add_argument("--stft-hop-length", type=int, default=256, help="STFT hop length: samples per mel frame")
    x = p.add_argument_group("this port")
    x.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"], help="16-bit storage type")
    x.add_argument("--seed", default=1234, type=int, help="stream of the prenet's dropout masks (and of the vocoder's noise)")
    args, unknown = p.parse_known_args(argv)                             # as the reference does (inference.py:200)
    if unknown:
        print("warning: ignored command-line arguments: %s" % " ".join(unknown), file=sys.stderr)
    return args


def check_args(args):
    if args.cpu:
        raise SystemExit("--cpu: this path runs on the MI355X only")
    if args.fp16 and args.amp_dtype != "fp16":
        raise SystemExit("--fp16 and --amp-dtype bf16 contradict each other")
    if args.tacotron2 is None:
        raise SystemExit("--tacotron2 CHECKPOINT is required")
    if args.stft_hop_length != 256:
        raise SystemExit("--stft-hop-length: the vocoder upsamples by 256 samples per frame")


def load_model(path, device):
    """-> (Tacotron2 with the checkpoint's weights, the checkpoint's config or the reference's defaults)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in ckpt["state_dict"].items()}
    config = dict(ckpt.get("config") or DEFAULT_CONFIG)
    model = Tacotron2(device=device, **config)
    model.load_reference_state(state)
    return model, config


def read_phrases(path):
    try:
        with open(path, "r") as f:
            return [ln for ln in f.readlines() if ln.strip()]
    except OSError:
        raise SystemExit("Could not read file")


def prepare_input_sequence(texts):
    """inference.py:141-172: english_cleaners sequences, sorted by length (descending), right zero padded.
    -> (text int64 [B, Ti], lengths int64 [B]) on the CPU."""
    seqs = [torch.tensor(text_to_sequence(t, ["english_cleaners"]), dtype=torch.int64) for t in texts]
    lengths, order = torch.sort(torch.tensor([len(s) for s in seqs], dtype=torch.int64), dim=0, descending=True)
    padded = torch.zeros(len(seqs), int(lengths[0]), dtype=torch.int64)
    for i, j in enumerate(order.tolist()):
        padded[i, :seqs[j].numel()] = seqs[j]
    return padded, lengths


def main(argv=None):
    """-> (mel fp32 [B, n_mel, T], mel_lengths int32 [B], audio fp32 [B, T * hop] or None) on the device."""
    from ..waveglow.infer import Denoiser, WaveGlowVocoder
    from .infer import Tacotron2Synthesizer
    args = parse_args(argv)
    check_args(args)
    dev = torch.device("cuda", 0)
    os.makedirs(args.output, exist_ok=True)
    DLLogger.init(backends=[DLLogger.JSONStreamBackend(DLLogger.Verbosity.DEFAULT, os.path.join(args.output, args.log_file)),
                            DLLogger.StdOutBackend(DLLogger.Verbosity.VERBOSE)])
    for k, v in vars(args).items():
        DLLogger.log(step="PARAMETER", data={k: v})
    DLLogger.log(step="PARAMETER", data={"model_name": "Tacotron2_PyT"})
    dtype = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    model, config = load_model(args.tacotron2, dev)
    synth = Tacotron2Synthesizer(model, compute_dtype=dtype, max_decoder_steps=int(config.get("max_decoder_steps", 2000)),
                                 gate_threshold=float(config.get("gate_threshold", 0.5)),
                                 early_stopping=not config.get("decoder_no_early_stopping", False), seed=args.seed)
    vocoder = denoiser = None
    if args.waveglow is not None:
        wg = load_waveglow(args.waveglow, dev)
        vocoder = WaveGlowVocoder(wg, compute_dtype=dtype)
        if args.denoising_strength > 0:
            denoiser = Denoiser(vocoder, n_mel_channels=wg.cfg["n_mel_channels"])
    text, lengths = prepare_input_sequence(read_phrases(args.input))
    text, lengths = text.to(dev), lengths.to(dev)
    if args.include_warmup:
        for _ in range(3):
            mel, _, _ = synth.infer(text, lengths)
            if vocoder is not None:
                vocoder.infer(mel, sigma=args.sigma_infer)
    torch.manual_seed(args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    mel, mel_lengths, _ = synth.infer(text, lengths)
    torch.cuda.synchronize()
    t_t2 = time.perf_counter() - t0
    print("Stopping after", mel.size(2), "decoder steps")
    DLLogger.log(step=0, data={"tacotron2_items_per_sec": mel.size(0) * mel.size(2) / t_t2})
    DLLogger.log(step=0, data={"tacotron2_latency": t_t2})
    audio = None
    if vocoder is None:
        for i in range(mel.size(0)):
            torch.save(mel[i, :, :int(mel_lengths[i])].cpu(), os.path.join(args.output, "mel_%d%s.pt" % (i, args.suffix)))
        DLLogger.log(step=0, data={"latency": t_t2})
    else:
        t0 = time.perf_counter()
        audio = vocoder.infer(mel, sigma=args.sigma_infer)
        torch.cuda.synchronize()
        t_wg = time.perf_counter() - t0
        t0 = time.perf_counter()
        audio = denoiser(audio, strength=args.denoising_strength).squeeze(1) if denoiser is not None else audio.clone()
        torch.cuda.synchronize()
        t_dn = time.perf_counter() - t0
        DLLogger.log(step=0, data={"waveglow_items_per_sec": audio.numel() / t_wg})
        DLLogger.log(step=0, data={"waveglow_latency": t_wg})
        DLLogger.log(step=0, data={"denoiser_latency": t_dn})
        DLLogger.log(step=0, data={"latency": t_t2 + t_wg + t_dn})
        host, lens = audio.float().cpu().numpy(), mel_lengths.cpu().tolist()
        for i, a in enumerate(host):
            a = a[:lens[i] * args.stft_hop_length]
            peak = float(np.abs(a).max()) if a.size else 0.0
            write_wav(os.path.join(args.output, "audio_%d%s.wav" % (i, args.suffix)), a / peak if peak > 0 else a, args.sampling_rate)
    DLLogger.flush()
    return mel, mel_lengths, audio


if __name__ == "__main__":
    main()
