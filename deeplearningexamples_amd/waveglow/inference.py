"""Entry point mirroring the WaveGlow half of SpeechSynthesis/Tacotron2/inference.py: mel spectrogram -> audio files.

    python -m deeplearningexamples_amd.waveglow.inference --waveglow out/checkpoint_WaveGlow_last.pt --mel mel.pt -o audio/
    python -m deeplearningexamples_amd.waveglow.inference --waveglow CKPT --synth-data -o audio/ --fp16

The flag names are the reference's (inference.py:46-77); --mel / --synth-data replace its text input: the text-to-mel half lives
in tacotron2/inference.py (text -> mel -> audio), and -i / --tacotron2 parse here only to exit pointing at it.  The checkpoint is the file
waveglow/train.py writes or the reference's own (`state_dict` + `config`, DistributedDataParallel's "module." prefix removed).
Writes audio_<n><suffix>.wav (16-bit PCM, each utterance scaled to full range as the reference does) and DLLogger records
(waveglow_latency, waveglow_items_per_sec, denoiser_latency, latency).
"""
import argparse
import os
import sys
import time
import wave

import numpy as np
import torch

from ..utils import dllogger as DLLogger
from .infer import Denoiser, WaveGlowVocoder
from .model import DEFAULT_CONFIG, WaveGlow


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="WaveGlow inference on MI355X (mel spectrogram to audio)", allow_abbrev=False)
    p.add_argument("-i", "--input", type=str, default=None, help="input text: see deeplearningexamples_amd.tacotron2.inference")
    p.add_argument("-o", "--output", required=True, help="output folder to save audio (file per utterance)")
    p.add_argument("--suffix", type=str, default="", help="output filename suffix")
    p.add_argument("--tacotron2", type=str, default=None, help="Tacotron2 checkpoint: see deeplearningexamples_amd.tacotron2.inference")
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
    src = x.add_mutually_exclusive_group()
    src.add_argument("--mel", type=str, default=None, help="torch file holding a mel spectrogram [80, frames] or [B, 80, frames]")
    src.add_argument("--synth-data", action="store_true", help="a normal(-5.62, 1.98) spectrogram instead of a file")
    x.add_argument("--synth-frames", default=895, type=int, help="--synth-data: mel frames per utterance")
    x.add_argument("-bs", "--batch-size", default=1, type=int, help="--synth-data: utterances")
    x.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"], help="16-bit storage type")
    x.add_argument("--seed", default=1234, type=int, help="seed of the noise (and of --synth-data)")
    args, unknown = p.parse_known_args(argv)                             # as the reference does (inference.py:200)
    if unknown:
        print("warning: ignored command-line arguments: %s" % " ".join(unknown), file=sys.stderr)
    return args


def _reject_unbuilt(args):
    if args.input is not None or args.tacotron2 is not None:
        raise SystemExit("-i / --tacotron2: text to speech (Tacotron2 + WaveGlow) is python -m deeplearningexamples_amd.tacotron2.inference; "
                         "this entry point takes a spectrogram: --mel FILE.pt or --synth-data")
    if args.cpu:
        raise SystemExit("--cpu: this path runs on the MI355X only")
    if args.fp16 and args.amp_dtype != "fp16":
        raise SystemExit("--fp16 and --amp-dtype bf16 contradict each other")
    if args.waveglow is None:
        raise SystemExit("--waveglow CHECKPOINT is required")
    if args.mel is None and not args.synth_data:
        raise SystemExit("pass a spectrogram with --mel FILE.pt or --synth-data")
    if args.stft_hop_length != 256:
        raise SystemExit("--stft-hop-length: the network upsamples by 256 samples per frame")


def load_model(path, device):
    """-> WaveGlow with the checkpoint's weights (config: the checkpoint's own, else the reference's defaults)."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    state = {(k[7:] if k.startswith("module.") else k): v for k, v in ckpt["state_dict"].items()}
    model = WaveGlow(**dict(ckpt.get("config") or DEFAULT_CONFIG), device=device)
    model.load_reference_state(state)
    return model


def synth_mel(batch, n_mel, frames, seed):
    """The --synth-data input of inference_perf.py: normal(-5.62, 1.98)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(batch, n_mel, frames, generator=g) * 1.98 - 5.62


def write_wav(path, audio, rate):
    """audio: 1-D float array in [-1, 1] -> 16-bit mono PCM."""
    pcm = np.clip(np.rint(np.asarray(audio, dtype=np.float64) * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(rate))
        f.writeframes(pcm.tobytes())


def main(argv=None):
    """-> the audio fp32 [B, T] on the device, as written (before each file's scaling to full range)."""
    args = parse_args(argv)
    _reject_unbuilt(args)
    dev = torch.device("cuda", 0)
    os.makedirs(args.output, exist_ok=True)
    DLLogger.init(backends=[DLLogger.JSONStreamBackend(DLLogger.Verbosity.DEFAULT, os.path.join(args.output, args.log_file)),
                            DLLogger.StdOutBackend(DLLogger.Verbosity.VERBOSE)])
    for k, v in vars(args).items():
        DLLogger.log(step="PARAMETER", data={k: v})
    DLLogger.log(step="PARAMETER", data={"model_name": "WaveGlow_PyT"})
    model = load_model(args.waveglow, dev)
    vocoder = WaveGlowVocoder(model, compute_dtype=torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16)
    if args.synth_data:
        mel = synth_mel(args.batch_size, model.cfg["n_mel_channels"], args.synth_frames, args.seed)
    else:
        mel = torch.load(args.mel, map_location="cpu", weights_only=False)
        mel = torch.as_tensor(mel, dtype=torch.float32)
        mel = mel[None] if mel.dim() == 2 else mel
    mel = mel.to(dev, torch.float32).contiguous()
    denoiser = Denoiser(vocoder, n_mel_channels=model.cfg["n_mel_channels"]) if args.denoising_strength > 0 else None
    if args.include_warmup:
        for _ in range(3):
            vocoder.infer(mel, sigma=args.sigma_infer)
    torch.manual_seed(args.seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    audio = vocoder.infer(mel, sigma=args.sigma_infer)
    torch.cuda.synchronize()
    t_wg = time.perf_counter() - t0
    t0 = time.perf_counter()
    if denoiser is not None:
        audio = denoiser(audio, strength=args.denoising_strength).squeeze(1)
    else:
        audio = audio.clone()
    torch.cuda.synchronize()
    t_dn = time.perf_counter() - t0
    DLLogger.log(step=0, data={"waveglow_items_per_sec": audio.numel() / t_wg})
    DLLogger.log(step=0, data={"waveglow_latency": t_wg})
    DLLogger.log(step=0, data={"denoiser_latency": t_dn})
    DLLogger.log(step=0, data={"latency": t_wg + t_dn})
    host = audio.float().cpu().numpy()
    for i, a in enumerate(host):
        peak = float(np.abs(a).max())
        write_wav(os.path.join(args.output, "audio_%d%s.wav" % (i, args.suffix)), a / peak if peak > 0 else a, args.sampling_rate)
    DLLogger.flush()
    return audio


if __name__ == "__main__":
    main()
