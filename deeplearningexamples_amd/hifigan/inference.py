"""Entry point mirroring SpeechSynthesis/HiFiGAN/inference.py for the vocoder-only case: saved mel spectrograms -> audio files.

    python -m deeplearningexamples_amd.hifigan.inference -i phrases/mels.tsv --dataset-path data/ --hifigan hifigan_gen_checkpoint.pt \
        -o audio/ --amp --cuda [-d 0.01] [--ema] [-bs 16] [--amp-dtype bf16]

The flag names are the reference's (inference.py:52-148) plus --amp-dtype; every other flag of its parser parses.  -i names a
.tsv whose header has a `mel` column (files under --dataset-path, each a torch tensor [80, frames]) and optionally an `output`
column (file names of the .wav files; audio_<n>.wav otherwise).  As the reference: utterances ordered by length, longest first,
zero padded to batches of -bs; audio scaled by --max_wav_value, cut to mel_len * hop_length samples, --fade-out frames faded,
scaled to its peak; .wav files written only when --repeats is 1.  DLLogger records hifigan_samples/s and hifigan_latency per
batch and their averages.  The checkpoint is the reference's ({'generator', 'gen_ema', 'config', 'train_setup'}); its
train_setup overrides --sampling-rate, --hop-length, --win-length and --max_wav_value as the reference does.

What this port does not build exits with one line: --fastpitch (and a text input, which needs it), --waveglow, --torchscript,
--torch-tensorrt, --checkpoint-format ts, --report-mel-loss.
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np
import torch

from ..utils import dllogger as DLLogger
from ..waveglow.inference import write_wav
from .infer import Denoiser, HifiGanVocoder

CHECKPOINT_SPECIFIC_ARGS = ["sampling_rate", "hop_length", "win_length", "max_wav_value"]


def build_parser():
    p = argparse.ArgumentParser(description="HiFi-GAN inference on MI355X (mel spectrogram to audio)", allow_abbrev=False)
    p.add_argument("-i", "--input", type=str, required=True, help="full path to the input .tsv (a `mel` column, optionally `output`)")
    p.add_argument("-o", "--output", default=None, help="output folder to save audio (file per phrase)")
    p.add_argument("--log-file", type=str, default=None, help="path to a DLLogger log file")
    p.add_argument("--save-mels", action="store_true", help="(spectrogram generator only)")
    p.add_argument("--cuda", action="store_true", help="accepted: this path always runs on the GPU")
    p.add_argument("--cudnn-benchmark", action="store_true", help="accepted and ignored")
    p.add_argument("--l2-promote", action="store_true", help="accepted and ignored")
    p.add_argument("--fastpitch", type=str, default=None, help="not built: see deeplearningexamples_amd.tacotron2.inference")
    p.add_argument("--waveglow", type=str, default=None, help="not built here: see deeplearningexamples_amd.waveglow.inference")
    p.add_argument("-s", "--waveglow-sigma-infer", default=0.9, type=float, help="(WaveGlow only)")
    p.add_argument("--hifigan", type=str, default=None, help="full path to a HiFi-GAN checkpoint file")
    p.add_argument("-d", "--denoising-strength", default=0.0, type=float, help="capture and subtract model bias to enhance audio")
    p.add_argument("--hop-length", type=int, default=256, help="STFT hop length for estimating audio length from mel size")
    p.add_argument("--win-length", type=int, default=1024, help="STFT win length for the denoiser")
    p.add_argument("-sr", "--sampling-rate", default=22050, type=int, choices=[22050, 44100], help="sampling rate")
    p.add_argument("--max_wav_value", default=32768.0, type=float, help="maximum audiowave value")
    p.add_argument("--amp", action="store_true", help="16-bit inference (the only mode of this path)")
    p.add_argument("-bs", "--batch-size", type=int, default=64)
    p.add_argument("--warmup-steps", type=int, default=0, help="warmup iterations before measuring performance")
    p.add_argument("--repeats", type=int, default=1, help="repeat inference for benchmarking")
    p.add_argument("--torchscript", action="store_true", help="not built")
    p.add_argument("--checkpoint-format", type=str, choices=["pyt", "ts"], default="pyt", help="input checkpoint format")
    p.add_argument("--torch-tensorrt", action="store_true", help="not built")
    p.add_argument("--report-mel-loss", action="store_true", help="not built")
    p.add_argument("--ema", action="store_true", help="use the EMA averaged model (if saved in the checkpoint)")
    p.add_argument("--dataset-path", type=str, help="path to the dataset (the `mel` column is relative to it)")
    p.add_argument("--speaker", type=int, default=0, help="(spectrogram generator only)")
    p.add_argument("--affinity", type=str, default="single",
                   choices=["socket", "single", "single_unique", "socket_unique_interleaved", "socket_unique_continuous", "disabled"],
                   help="accepted and ignored")
    t = p.add_argument_group("transform")
    t.add_argument("--fade-out", type=int, default=6, help="number of fadeout frames at the end")
    t.add_argument("--pace", type=float, default=1.0, help="(spectrogram generator only)")
    t.add_argument("--pitch-transform-flatten", action="store_true", help="(spectrogram generator only)")
    t.add_argument("--pitch-transform-invert", action="store_true", help="(spectrogram generator only)")
    t.add_argument("--pitch-transform-amplify", type=float, default=1.0, help="(spectrogram generator only)")
    t.add_argument("--pitch-transform-shift", type=float, default=0.0, help="(spectrogram generator only)")
    t.add_argument("--pitch-transform-custom", action="store_true", help="(spectrogram generator only)")
    x = p.add_argument_group("Text processing parameters")
    x.add_argument("--text-cleaners", type=str, nargs="*", default=["english_cleaners_v2"], help="(text input only)")
    x.add_argument("--symbol-set", type=str, default="english_basic", help="(text input only)")
    x.add_argument("--p-arpabet", type=float, default=0.0, help="(text input only)")
    x.add_argument("--heteronyms-path", type=str, default="data/cmudict/heteronyms", help="(text input only)")
    x.add_argument("--cmudict-path", type=str, default="data/cmudict/cmudict-0.7b", help="(text input only)")
    g = p.add_argument_group("this port")
    g.add_argument("--hifigan-config", type=str, default=None, help="a HiFi-GAN config .json (overrides the checkpoint's)")
    g.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"], help="16-bit storage type")
    g.add_argument("--graphs", action="store_true", help="replay one captured graph per batch shape")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def load_fields(fpath):
    """inference.py:151-159: a .tsv's columns by header name; any other file is a list of phrases."""
    lines = [l.strip() for l in open(fpath, encoding="utf-8")]
    if fpath.endswith(".tsv"):
        columns = lines[0].split("\t")
        fields = list(zip(*[t.split("\t") for t in lines[1:] if t]))
    else:
        columns, fields = ["text"], [lines]
    return {c: list(f) for c, f in zip(columns, fields)}


def _reject_unbuilt(args, fields):
    if args.fastpitch is not None:
        raise SystemExit("--fastpitch: this entry point reads saved spectrograms; text to speech with FastPitch is python -m deeplearningexamples_amd.fastpitch.inference")
    if args.waveglow is not None:
        raise SystemExit("--waveglow: the WaveGlow vocoder is python -m deeplearningexamples_amd.waveglow.inference")
    if args.torchscript:
        raise SystemExit("--torchscript: TorchScript inference is not built")
    if args.torch_tensorrt:
        raise SystemExit("--torch-tensorrt: Torch-TensorRT inference is not built")
    if args.checkpoint_format == "ts":
        raise SystemExit("--checkpoint-format ts: TorchScript checkpoints are not read; pass the reference's .pt checkpoint")
    if args.report_mel_loss:
        raise SystemExit("--report-mel-loss: the mel loss is not built")
    if "mel" not in fields:
        raise SystemExit("the input has no `mel` column: this entry point turns saved spectrograms into audio; text to speech is "
                         "python -m deeplearningexamples_amd.tacotron2.inference")
    if args.hifigan is None:
        raise SystemExit("--hifigan CHECKPOINT is required")
    if not args.amp:
        raise SystemExit("this path computes in 16 bits: pass --amp (the reference's fp32 / TF32 recipes are not built)")


def prepare_batches(fields, dataset_path, batch_size, device):
    """inference.py:162-209 for the vocoder-only case: load, order by length (longest first), cut into batches, zero pad.
    -> [dict(mel [B, 80, Tmax] fp32 on `device`, mel_lens [B] (host), output [names] or None)]."""
    mels = [torch.as_tensor(torch.load(os.path.join(dataset_path or "", f), map_location="cpu", weights_only=False)).float()
            for f in fields["mel"]]
    for f, m in zip(fields["mel"], mels):
        if m.dim() != 2 or m.shape[0] != 80:
            raise SystemExit("%s: expected a [80, frames] spectrogram, got %s" % (f, tuple(m.shape)))
    order = np.argsort([-m.shape[1] for m in mels])
    mels = [mels[i] for i in order]
    names = [fields["output"][i] for i in order] if "output" in fields else None
    batches = []
    for b in range(0, len(mels), batch_size):
        part = mels[b:b + batch_size]
        lens = torch.tensor([m.shape[1] for m in part], dtype=torch.long)
        mel = torch.zeros((len(part), 80, int(lens.max())), dtype=torch.float32)
        for i, m in enumerate(part):
            mel[i, :, :m.shape[1]] = m
        batches.append(dict(mel=mel.to(device), mel_lens=lens, output=names[b:b + batch_size] if names else None))
    return batches


def main(argv=None):
    """-> the audio of every utterance as written (1-D fp32 host arrays, in the order processed)."""
    args = parse_args(argv)
    fields = load_fields(args.input)
    _reject_unbuilt(args, fields)
    dev = torch.device("cuda", 0)
    if args.output is not None:
        os.makedirs(args.output, exist_ok=True)
    log_fpath = args.log_file or os.path.join(args.output or ".", "nvlog_infer.json")
    DLLogger.init(backends=[DLLogger.JSONStreamBackend(DLLogger.Verbosity.DEFAULT, log_fpath, append=True),
                            DLLogger.StdOutBackend(DLLogger.Verbosity.VERBOSE)])
    for k, v in vars(args).items():
        DLLogger.log(step="PARAMETER", data={k: v})
    ckpt = torch.load(args.hifigan, map_location="cpu", weights_only=False)
    config = json.load(open(args.hifigan_config)) if args.hifigan_config else None
    dtype = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    vocoder = HifiGanVocoder.from_checkpoint(ckpt, ema=args.ema, config=config, dtype=dtype, device=dev, graphs=args.graphs)
    for k in CHECKPOINT_SPECIFIC_ARGS:                                   # inference.py:399-412
        val = (ckpt.get("train_setup") or {}).get(k)
        if val and getattr(args, k) != val:
            print("Overwriting args.%s=%s with %s from vocoder checkpoint." % (k, getattr(args, k), val))
            setattr(args, k, val)
    denoiser = Denoiser(vocoder, win_length=args.win_length) if args.denoising_strength > 0.0 else None

    def generate_audio(mel):
        audios = vocoder.infer(mel.to(dtype))                            # --amp: the reference hands the vocoder a 16-bit spectrogram
        if denoiser is not None:
            audios = denoiser(audios, args.denoising_strength).squeeze(1)
        return audios * args.max_wav_value

    batches = prepare_batches(fields, args.dataset_path, args.batch_size, dev)
    cycle = itertools.cycle(batches)
    for _ in range(args.warmup_steps):
        generate_audio(next(cycle)["mel"])
    measures, written = [], []
    all_utterances = all_samples = 0
    log_enabled = args.repeats == 1
    for rep in range(args.repeats):
        for b in batches:
            torch.cuda.synchronize()
            t0 = time.time()
            audios = generate_audio(b["mel"])
            torch.cuda.synchronize()
            measures.append(time.time() - t0)
            if log_enabled:
                DLLogger.log(step=rep, data={"hifigan_samples/s": audios.size(0) * audios.size(1) / measures[-1]})
                DLLogger.log(step=rep, data={"hifigan_latency": measures[-1]})
            if args.output is not None and args.repeats == 1:
                for i, audio in enumerate(audios):
                    audio = audio[:int(b["mel_lens"][i]) * args.hop_length].clone()
                    if args.fade_out:
                        fade_len = min(args.fade_out * args.hop_length, audio.numel())
                        audio[audio.numel() - fade_len:] *= torch.linspace(1.0, 0.0, fade_len, device=audio.device)
                    peak = torch.max(torch.abs(audio))
                    audio = (audio / peak if float(peak) > 0 else audio).cpu().numpy()
                    fname = b["output"][i] if b["output"] else "audio_%d.wav" % (all_utterances + i)
                    write_wav(os.path.join(args.output, fname), audio, args.sampling_rate)
                    written.append(audio)
            all_utterances += b["mel"].size(0)
            all_samples += int(b["mel_lens"].sum()) * args.hop_length
    vm = np.sort(np.asarray(measures))
    DLLogger.log(step=(), data={"avg_hifigan_samples/s": all_samples / vm.sum()})
    DLLogger.log(step=(), data={"avg_hifigan_latency": vm.mean()})
    DLLogger.log(step=(), data={"avg_hifigan_RTF": all_samples / (all_utterances * vm.mean() * args.sampling_rate)})
    DLLogger.flush()
    return written


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
