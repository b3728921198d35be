"""Entry point mirroring SpeechSynthesis/FastPitch/inference.py: text -> mel spectrogram (FastPitch) -> audio (HiFi-GAN or WaveGlow).

    python -m deeplearningexamples_amd.fastpitch.inference -i phrases.txt --fastpitch FastPitch_checkpoint.pt \
        --hifigan hifigan_gen_checkpoint.pt -o audio/ --amp --cuda [--pace 0.9] [-bs 16] [--amp-dtype bf16]
    python -m deeplearningexamples_amd.fastpitch.inference -i phrases.tsv --fastpitch FastPitch_checkpoint.pt -o mels/ --amp --save-mels

The flag names are the reference's (inference.py:52-148) plus --amp-dtype and --hifigan-config; every flag of its parser parses.
-i names a text file (one phrase per line) or a .tsv with a `text` column and optionally an `output` column (file names).  As the
reference: phrases ordered by length, longest first, cut into batches of -bs; --pace, --speaker and the --pitch-transform-{flatten,
invert,amplify,shift} flags reach FastPitch.infer (the transform is a closure, not an eval'd string); audio is cut to mel_len *
hop_length samples, --fade-out frames are faded, the result scaled to its peak and written as 16-bit .wav when --repeats is 1;
--save-mels writes each spectrogram [frames, n_mel] as .npy.  DLLogger records fastpitch_frames/s, fastpitch_latency, the vocoder's
samples/s and latency per batch, and their averages.  Without --hifigan / --waveglow only --save-mels is possible.

Text.  The symbol table and cleaners are those of tacotron2/text.py (`english_basic`: the same 148 symbols).  `inflect` and
`unidecode` are not installed here, so `english_cleaners_v2` maps to text.py's `english_cleaners`: lowercase, the abbreviation
table, whitespace.  Missing against the reference's v2 pipeline: transliteration of non-ASCII text, the spelling out of numbers,
dates, times, currency and letter-number compounds ("2pm", "A4"), and the spelling of acronyms; text that holds digits or non-ASCII
characters raises and says so, and '/' becomes a space as in the reference.

What this port does not build exits with one line: --torchscript, --torch-tensorrt, --checkpoint-format ts, --report-mel-loss,
--pitch-transform-custom, --p-arpabet > 0, fp32 (no --amp).
"""
import argparse
import itertools
import os
import re
import sys
import time

import numpy as np
import torch

from ..hifigan.inference import CHECKPOINT_SPECIFIC_ARGS, load_fields
from ..tacotron2 import text as T
from ..utils import dllogger as DLLogger
from ..waveglow.inference import write_wav
from .infer import FastPitchSynthesizer

CLEANER_MAP = {"english_cleaners_v2": "english_cleaners"}


def build_parser():
    p = argparse.ArgumentParser(description="FastPitch inference on MI355X (text to mel spectrogram to audio)", allow_abbrev=False)
    p.add_argument("-i", "--input", type=str, required=True, help="full path to the input text (phrases separated by newlines) or .tsv")
    p.add_argument("-o", "--output", default=None, help="output folder to save audio (file per phrase)")
    p.add_argument("--log-file", type=str, default=None, help="path to a DLLogger log file")
    p.add_argument("--save-mels", action="store_true", help="save generator outputs to disk")
    p.add_argument("--cuda", action="store_true", help="accepted: this path always runs on the GPU")
    p.add_argument("--cudnn-benchmark", action="store_true", help="accepted and ignored")
    p.add_argument("--l2-promote", action="store_true", help="accepted and ignored")
    p.add_argument("--fastpitch", type=str, default=None, help="full path to the FastPitch checkpoint file (required)")
    p.add_argument("--waveglow", type=str, default=None, help="full path to a WaveGlow checkpoint file")
    p.add_argument("-s", "--waveglow-sigma-infer", default=0.9, type=float, help="WaveGlow sigma")
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
    p.add_argument("--ema", action="store_true", help="use the EMA averaged model (if saved in the checkpoints)")
    p.add_argument("--dataset-path", type=str, help="accepted (extra data fields are not read)")
    p.add_argument("--speaker", type=int, default=0, help="speaker id for a multi-speaker model")
    p.add_argument("--affinity", type=str, default="single",
                   choices=["socket", "single", "single_unique", "socket_unique_interleaved", "socket_unique_continuous", "disabled"],
                   help="accepted and ignored")
    t = p.add_argument_group("transform")
    t.add_argument("--fade-out", type=int, default=10, help="number of fadeout frames at the end")
    t.add_argument("--pace", type=float, default=1.0, help="adjust the pace of speech")
    t.add_argument("--pitch-transform-flatten", action="store_true", help="flatten the pitch")
    t.add_argument("--pitch-transform-invert", action="store_true", help="invert the pitch wrt mean value")
    t.add_argument("--pitch-transform-amplify", type=float, default=1.0, help="multiplicative amplification of pitch variability")
    t.add_argument("--pitch-transform-shift", type=float, default=0.0, help="raise/lower the pitch by <hz>")
    t.add_argument("--pitch-transform-custom", action="store_true", help="not built")
    x = p.add_argument_group("Text processing parameters")
    x.add_argument("--text-cleaners", type=str, nargs="*", default=["english_cleaners_v2"], help="type of text cleaners for input text")
    x.add_argument("--symbol-set", type=str, default="english_basic", help="symbol set for input text")
    x.add_argument("--p-arpabet", type=float, default=0.0, help="not built above 0")
    x.add_argument("--heteronyms-path", type=str, default="cmudict/heteronyms", help="(ARPAbet only)")
    x.add_argument("--cmudict-path", type=str, default="cmudict/cmudict-0.7b", help="(ARPAbet only)")
    g = p.add_argument_group("this port")
    g.add_argument("--hifigan-config", type=str, default=None, help="a HiFi-GAN config .json (overrides the checkpoint's)")
    g.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"], help="16-bit storage type")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def _reject_unbuilt(args):
    if args.torchscript:
        raise SystemExit("--torchscript: TorchScript inference is not built")
    if args.torch_tensorrt:
        raise SystemExit("--torch-tensorrt: Torch-TensorRT inference is not built")
    if args.checkpoint_format == "ts":
        raise SystemExit("--checkpoint-format ts: TorchScript checkpoints are not read; pass the reference's .pt checkpoint")
    if args.report_mel_loss:
        raise SystemExit("--report-mel-loss: the mel loss is not built")
    if args.pitch_transform_custom:
        raise SystemExit("--pitch-transform-custom: the custom transform of pitch_transform.py is not built")
    if args.p_arpabet > 0.0:
        raise SystemExit("--p-arpabet > 0: the CMUdict ARPAbet conversion is not built (write phonemes as {HH AW1 S} spans)")
    if args.symbol_set != "english_basic":
        raise SystemExit("--symbol-set %s: only english_basic is built" % args.symbol_set)
    if args.fastpitch is None:
        raise SystemExit("--fastpitch CHECKPOINT is required (saved spectrograms to audio is python -m deeplearningexamples_amd.hifigan.inference)")
    if args.waveglow is not None and args.hifigan is not None:
        raise SystemExit("--waveglow and --hifigan: specify a single vocoder model")
    if args.waveglow is None and args.hifigan is None and not args.save_mels:
        raise SystemExit("no vocoder (--hifigan or --waveglow): without one only --save-mels has anything to write")
    if args.save_mels and args.output is None:
        raise SystemExit("--save-mels needs an output folder (-o)")
    if not args.amp:
        raise SystemExit("this path computes in 16 bits: pass --amp (the reference's fp32 / TF32 recipes are not built)")


def build_pitch_transformation(args):
    """inference.py:211-233 as a closure: ((((pitch * 0) * -1) * amplify) + shift / std), each step only when its flag is set.
    -> None when no flag is set."""
    flatten, invert = args.pitch_transform_flatten, args.pitch_transform_invert
    amplify, shift = args.pitch_transform_amplify, args.pitch_transform_shift
    if not flatten and not invert and amplify == 1.0 and shift == 0.0:
        return None

    def transform(pitch, pitch_lens, mean, std):
        if flatten:
            pitch = pitch * 0.0
        if invert:
            pitch = pitch * -1.0
        if amplify != 1.0:
            pitch = pitch * amplify
        if shift != 0.0:
            pitch = pitch + shift / std
        return pitch
    return transform


def encode_text(text, cleaner_names):
    """text_processing.py:125-164 with p_arpabet = 0 -> list of symbol ids ({...} spans are ARPAbet)."""
    names = [CLEANER_MAP.get(n, n) for n in cleaner_names]
    ids = T.text_to_sequence(re.sub(r"/+", " ", text) if "english_cleaners_v2" in cleaner_names else text, names)
    if not ids:
        raise SystemExit("a phrase has no symbol of the table: %r" % (text,))
    return ids


def prepare_batches(fields, cleaner_names, batch_size):
    """inference.py:161-208: encode, order by length (longest first), cut into batches.
    -> [dict(text [id tensors], text_lens [B], output [names] or None)]."""
    texts = [torch.tensor(encode_text(t, cleaner_names), dtype=torch.int64) for t in fields["text"]]
    order = np.argsort([-t.numel() for t in texts], kind="stable")
    texts = [texts[i] for i in order]
    names = [fields["output"][i] for i in order] if "output" in fields else None
    for t in texts:
        print(T.sequence_to_text(t.numpy()))
    return [dict(text=texts[b:b + batch_size], text_lens=[t.numel() for t in texts[b:b + batch_size]],
                 output=names[b:b + batch_size] if names else None) for b in range(0, len(texts), batch_size)]


def finish_audio(audio, n_samples, fade_frames, hop_length):
    """One utterance as the reference writes it (inference.py:497-507): cut to its length, fade-out, scaled to its peak -> host
    array."""
    audio = audio[:n_samples].clone()
    if fade_frames:
        fade_len = min(fade_frames * hop_length, audio.numel())
        audio[audio.numel() - fade_len:] *= torch.linspace(1.0, 0.0, fade_len, device=audio.device)
    peak = torch.max(torch.abs(audio)) if audio.numel() else 0.0
    return (audio / peak if float(peak) > 0 else audio).cpu().numpy()


def load_vocoder(args, dtype, dev):
    """-> (name, generate_audio(mel fp32 [B, n_mel, T]) -> audio fp32 [B, T * hop] scaled as the reference's, train_setup)."""
    if args.hifigan is not None:
        import json

        from ..hifigan.infer import Denoiser, HifiGanVocoder
        ckpt = torch.load(args.hifigan, map_location="cpu", weights_only=False)
        config = json.load(open(args.hifigan_config)) if args.hifigan_config else None
        vocoder = HifiGanVocoder.from_checkpoint(ckpt, ema=args.ema, config=config, dtype=dtype, device=dev)
        denoiser = Denoiser(vocoder, win_length=args.win_length) if args.denoising_strength > 0.0 else None

        def generate_audio(mel):
            audios = vocoder.infer(mel)
            if denoiser is not None:
                audios = denoiser(audios, args.denoising_strength).squeeze(1)
            return audios * args.max_wav_value
        return "hifigan", generate_audio, ckpt.get("train_setup") or {}
    if args.waveglow is not None:
        from ..waveglow.infer import Denoiser, WaveGlowVocoder
        from ..waveglow.inference import load_model
        model = load_model(args.waveglow, dev)
        vocoder = WaveGlowVocoder(model, compute_dtype=dtype)
        denoiser = Denoiser(vocoder, win_length=args.win_length, n_mel_channels=model.cfg["n_mel_channels"]) \
            if args.denoising_strength > 0.0 else None

        def generate_audio(mel):
            audios = vocoder.infer(mel.float().contiguous(), sigma=args.waveglow_sigma_infer)
            if denoiser is not None:
                audios = denoiser(audios.float(), strength=args.denoising_strength).squeeze(1)
            return audios
        return "waveglow", generate_audio, {}
    return None, None, {}


def main(argv=None):
    """-> dict(mels=[host arrays [frames, n_mel]], audio=[1-D host arrays as written]) in the order processed."""
    args = parse_args(argv)
    _reject_unbuilt(args)
    fields = load_fields(args.input)
    if "text" not in fields:
        raise SystemExit("the input has no `text` column")
    dev = torch.device("cuda", 0)
    if args.output is not None:
        os.makedirs(args.output, exist_ok=True)
    log_fpath = args.log_file or os.path.join(args.output or ".", "nvlog_infer.json")
    DLLogger.init(backends=[DLLogger.JSONStreamBackend(DLLogger.Verbosity.DEFAULT, log_fpath, append=True),
                            DLLogger.StdOutBackend(DLLogger.Verbosity.VERBOSE)])
    for k, v in vars(args).items():
        DLLogger.log(step="PARAMETER", data={k: v})
    dtype = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    gen_ckpt = torch.load(args.fastpitch, map_location="cpu", weights_only=False)
    generator = FastPitchSynthesizer.from_checkpoint(gen_ckpt, ema=args.ema, dtype=dtype, device=dev)
    voc_name, generate_audio, voc_setup = load_vocoder(args, dtype, dev)
    gen_setup = gen_ckpt.get("train_setup") or {}
    for k in CHECKPOINT_SPECIFIC_ARGS:                                   # inference.py:399-412
        v1, v2 = gen_setup.get(k), voc_setup.get(k)
        if v1 is not None and v2 is not None and v1 != v2:
            raise SystemExit("%s mismatch in spectrogram generator and vocoder" % k)
        val = v1 or v2
        if val and getattr(args, k) != val:
            print("Overwriting args.%s=%s with %s from %s checkpoint." % (k, getattr(args, k), val, "generator" if v2 is None else "vocoder"))
            setattr(args, k, val)
    gen_kw = dict(pace=args.pace, speaker=args.speaker, pitch_tgt=None, pitch_transform=build_pitch_transformation(args))

    batches = prepare_batches(fields, args.text_cleaners, args.batch_size)
    cycle = itertools.cycle(batches)
    for _ in range(args.warmup_steps):
        mel = generator.infer(next(cycle)["text"])[0]
        if generate_audio is not None:
            generate_audio(mel)
    gen_measures, voc_measures, mels, written = [], [], [], []
    all_utterances = all_samples = all_letters = all_frames = 0
    log_enabled = args.repeats == 1
    log = (lambda s, d: DLLogger.log(step=s, data=d)) if log_enabled else (lambda s, d: None)
    for rep in range(args.repeats):
        for b in batches:
            torch.cuda.synchronize()
            t0 = time.time()
            mel, mel_lens = generator.infer(b["text"], **gen_kw)[:2]
            torch.cuda.synchronize()
            gen_measures.append(time.time() - t0)
            lens = mel_lens.tolist()
            all_letters += sum(b["text_lens"])
            all_frames += mel.size(0) * mel.size(2)
            log(rep, {"fastpitch_frames/s": mel.size(0) * mel.size(2) / gen_measures[-1]})
            log(rep, {"fastpitch_latency": gen_measures[-1]})
            if args.save_mels and args.repeats == 1:
                for i, n in enumerate(lens):
                    m = mel[i, :, :n].permute(1, 0).cpu().numpy()
                    fname = b["output"][i] if b["output"] else "mel_%d.npy" % (all_utterances + i)
                    np.save(os.path.join(args.output, os.path.splitext(os.path.basename(fname))[0] + ".npy"), m)
                    mels.append(m)
            if generate_audio is not None and mel.size(2) > 0:
                torch.cuda.synchronize()
                t0 = time.time()
                audios = generate_audio(mel)
                torch.cuda.synchronize()
                voc_measures.append(time.time() - t0)
                log(rep, {"%s_samples/s" % voc_name: audios.size(0) * audios.size(1) / voc_measures[-1]})
                log(rep, {"%s_latency" % voc_name: voc_measures[-1]})
                if args.output is not None and args.repeats == 1:
                    for i, audio in enumerate(audios):
                        host = finish_audio(audio.float(), lens[i] * args.hop_length, args.fade_out, args.hop_length)
                        fname = b["output"][i] if b["output"] else "audio_%d.wav" % (all_utterances + i)
                        write_wav(os.path.join(args.output, fname), host, args.sampling_rate)
                        written.append(host)
                all_samples += sum(lens) * args.hop_length
            all_utterances += len(lens)
    gm = np.asarray(gen_measures)
    DLLogger.log(step=(), data={"avg_fastpitch_tokens/s": all_letters / gm.sum()})
    DLLogger.log(step=(), data={"avg_fastpitch_frames/s": all_frames / gm.sum()})
    DLLogger.log(step=(), data={"avg_fastpitch_latency": gm.mean()})
    DLLogger.log(step=(), data={"avg_fastpitch_RTF": all_frames * args.hop_length / (gm.sum() * args.sampling_rate)})
    if voc_measures:
        vm = np.asarray(voc_measures)
        DLLogger.log(step=(), data={"avg_%s_samples/s" % voc_name: all_samples / vm.sum()})
        DLLogger.log(step=(), data={"avg_%s_latency" % voc_name: vm.mean()})
        DLLogger.log(step=(), data={"avg_latency": gm.mean() + vm.mean()})
    DLLogger.flush()
    return dict(mels=mels, audio=written)


if __name__ == "__main__":
    sys.exit(0 if main() is not None else 1)
