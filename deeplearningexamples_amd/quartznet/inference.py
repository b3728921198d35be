"""Entry point mirroring SpeechRecognition/QuartzNet/inference.py: .wav files (or a manifest) -> transcripts (and WER).

    python -m deeplearningexamples_amd.quartznet.inference --model_config quartznet15x5_speedp-online-1.15_speca.yaml \
        --ckpt QuartzNet_checkpoint.pt --ema --amp --transcribe_wav speech.wav [--amp-dtype bf16]
    python -m deeplearningexamples_amd.quartznet.inference --model_config CONFIG.yaml --ckpt CKPT.pt --amp --dataset_dir LibriSpeech \
        --val_manifests librispeech-dev-clean-wav.json --batch_size 16 --override_config input_val.audio_dataset.trim_silence=false

The flag names are the reference's (inference.py:43-93) plus --amp-dtype; every flag of its parser parses.  Built: --transcribe_wav,
--transcribe_filelist (one path per line; batch size 1, as the reference), --dataset_dir + --val_manifests (the reference's .json
manifests: `files[-1].fname`, `transcript`; batches of --batch_size in manifest order) with the word error rate of
common/metrics.py:15-59 restated, --model_config, --ckpt, --ema (falls back to the plain weights with the reference's warning when
the checkpoint has no averaged ones), --amp, --save_predictions, --save_logits, --override_config KEY=VALUE, --seed (the dither),
--steps / --warmup_steps with the latency percentiles of inference.py:96-114 (at least 20 measured steps, the first five dropped).
--save_logits writes a LIST of per-utterance [frames, n_classes] tensors: there is no padded batch here to save.
--dali_device other than none: for .wav input it is switched off with the reference's message; for a manifest it exits (DALI is
not built).  Wav files are read with tacotron2.audio.load_wav_to_torch; int16 samples are scaled by 2^-15 as the reference's
AudioSegment does.

What this port does not build exits with one line: --cpu, --torchscript, --torchscript_export, .nemo checkpoints, DALI on a
manifest, several GPUs (WORLD_SIZE > 1), a sampling rate other than 16 kHz, fp32 (no --amp), and a manifest run with
trim_silence: true (the trimming is librosa's, which is not installed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from ..tacotron2.audio import load_wav_to_torch
from ..utils import dllogger as DLLogger
from ..utils.state import load_config
from .infer import QuartzNetRecognizer
from .model import apply_overrides


def build_parser():
    p = argparse.ArgumentParser(description="QuartzNet inference on MI355X", allow_abbrev=False)
    p.add_argument("--batch_size", default=16, type=int, help="data batch size")
    p.add_argument("--steps", default=0, type=int, help="eval this many steps")
    p.add_argument("--warmup_steps", default=0, type=int, help="burn-in period before measuring latencies")
    p.add_argument("--model_config", type=str, required=True, help="model config path")
    p.add_argument("--dataset_dir", type=str, help="absolute path to dataset folder")
    p.add_argument("--val_manifests", type=str, nargs="+", help="relative path to evaluation dataset manifest files")
    p.add_argument("--ckpt", default=None, type=str, help="path to model checkpoint")
    p.add_argument("--amp", "--fp16", action="store_true", help="16-bit inference (the only mode of this path)")
    p.add_argument("--cudnn_benchmark", action="store_true", help="accepted and ignored")
    p.add_argument("--cpu", action="store_true", help="not built")
    p.add_argument("--seed", default=None, type=int, help="random seed (the dither)")
    p.add_argument("--local_rank", default=os.getenv("LOCAL_RANK", 0), type=int, help="accepted: one GPU only")
    io = p.add_argument_group("feature and checkpointing setup")
    io.add_argument("--dali_device", type=str, choices=["none", "cpu", "gpu"], default="gpu", help="DALI is not built")
    io.add_argument("--save_predictions", type=str, default=None, help="save predictions in text form at this location")
    io.add_argument("--save_logits", default=None, type=str, help="save the per-utterance log-probabilities under this path")
    io.add_argument("--transcribe_wav", type=str, help="path to a single .wav file (16 kHz)")
    io.add_argument("--transcribe_filelist", type=str, help="path to a filelist with one .wav path per line")
    io.add_argument("-o", "--output_dir", default="results/", help="output folder (the DLLogger file)")
    io.add_argument("--log_file", type=str, default=None, help="path to a DLLogger log file")
    io.add_argument("--ema", action="store_true", help="load averaged model weights")
    io.add_argument("--torchscript", action="store_true", help="not built")
    io.add_argument("--torchscript_export", action="store_true", help="not built")
    io.add_argument("--override_config", type=str, action="append", help="override a config value: nested.config.key=val")
    g = p.add_argument_group("this port")
    g.add_argument("--amp-dtype", default="fp16", choices=["fp16", "bf16"], help="16-bit storage type")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def reject_unbuilt(args, cfg=None):
    if args.cpu:
        raise SystemExit("--cpu: there is no CPU path")
    if args.torchscript or args.torchscript_export:
        raise SystemExit("--torchscript / --torchscript_export: TorchScript is not built")
    if args.ckpt is not None and args.ckpt.lower().endswith(".nemo"):
        raise SystemExit(".nemo checkpoints are not read: pass the reference's torch checkpoint")
    if int(os.environ.get("WORLD_SIZE", 1)) > 1:
        raise SystemExit("WORLD_SIZE > 1: inference on several GPUs is not built")
    if not args.amp:
        raise SystemExit("this path computes in 16 bits: pass --amp (the reference's fp32 / TF32 recipes are not built)")
    if args.transcribe_wav and args.transcribe_filelist:
        raise SystemExit("--transcribe_wav and --transcribe_filelist: pass one of them")
    wav_input = bool(args.transcribe_wav or args.transcribe_filelist)
    if not wav_input and not (args.dataset_dir and args.val_manifests):
        raise SystemExit("no input: --transcribe_wav, --transcribe_filelist, or --dataset_dir with --val_manifests")
    if not wav_input and args.dali_device != "none":
        raise SystemExit("--dali_device %s: DALI is not built; pass --dali_device none" % args.dali_device)
    if cfg is not None:
        sr = cfg["input_val"]["audio_dataset"].get("sample_rate", 16000)
        if int(sr) != 16000:
            raise SystemExit("sample_rate %s: only 16 kHz is built" % sr)
        if not wav_input and cfg["input_val"]["audio_dataset"].get("trim_silence", False):
            raise SystemExit("trim_silence: true needs librosa, which is not installed: pass "
                             "--override_config input_val.audio_dataset.trim_silence=false")


def read_wav(path):
    """-> fp32 samples in [-1, 1) (integer PCM scaled by 2^-(bits - 1), as common/audio.py's AudioSegment), 16 kHz mono only."""
    from scipy.io.wavfile import read
    kind = read(path, mmap=True)[1].dtype                               # the sample format, from the header
    data, sr = load_wav_to_torch(path)
    if int(sr) != 16000:
        raise SystemExit("%s: sampling rate %d; only 16 kHz is built" % (path, sr))
    if data.dim() != 1:
        raise SystemExit("%s: %d channels; only mono is built" % (path, data.shape[1]))
    if kind == np.int16:
        data = data * 2.0 ** -15
    elif kind == np.int32:
        data = data * 2.0 ** -31
    elif kind not in (np.float32, np.float64):
        raise SystemExit("%s: %s samples; only int16, int32 and float .wav files are built" % (path, kind))
    return data


def read_manifests(dataset_dir, manifests):
    """The reference's .json manifests (common/dataset.py:150-190) -> [(wav path, transcript)]."""
    out = []
    for m in manifests:
        for path in m.split(","):
            full = path if os.path.isabs(path) else os.path.join(dataset_dir, path)
            for s in json.load(open(full, "r", encoding="utf-8")):
                tr = s.get("transcript")
                if tr is None and s.get("text_filepath"):
                    tr = open(s["text_filepath"], "r", encoding="utf-8").read().replace("\n", "")
                if not isinstance(tr, str):
                    print("WARNING: Skipped sample (transcript not a str): %s." % (tr,))
                    continue
                out.append((os.path.join(dataset_dir, s["files"][-1]["fname"]), tr))
    return out


def normalize_transcript(s, labels):
    """Lower case and only the model's characters (the reference's normalize_string also spells out numbers with `inflect`, which is
    not installed: a transcript with digits keeps none of them)."""
    keep = set(labels)
    return " ".join("".join(c for c in s.lower() if c in keep).split())


def edit_distance(hyp, ref):
    """Fewest insertions, deletions and substitutions that turn the word list `hyp` into `ref` (the full table, by rows)."""
    rows, cols = len(hyp) + 1, len(ref) + 1
    table = np.zeros((rows, cols), dtype=np.int64)
    table[:, 0] = np.arange(rows)
    table[0, :] = np.arange(cols)
    for i in range(1, rows):
        for j in range(1, cols):
            same = hyp[i - 1] == ref[j - 1]
            table[i, j] = min(table[i - 1, j - 1] + (0 if same else 1), table[i - 1, j] + 1, table[i, j - 1] + 1)
    return int(table[-1, -1])


def word_error_rate(hypotheses, references):
    """What common/metrics.py:37-59 reports: word edits summed over the pairs, over the reference's words -> (wer, edits, words).
    Hypotheses beyond the references are ignored, fewer are an error, and no reference words at all give inf."""
    if len(hypotheses) < len(references):
        raise ValueError("%d hypotheses for %d references" % (len(hypotheses), len(references)))
    pairs = [(h.split(), r.split()) for h, r in zip(hypotheses, references)]
    edits = sum(edit_distance(h, r) for h, r in pairs)
    words = sum(len(r) for _, r in pairs)
    return (edits / words if words else float("inf")), edits, words


def latency_percentiles(seconds, ratios=(0.9, 0.95, 0.99), skip=5):
    """The figures inference.py:96-114 logs, in milliseconds, over the samples behind the first `skip`: for a ratio a the value at
    position int(n (1 - a)) of the samples in DESCENDING order (the slowest 1 - a of them lie above it), and the mean under 0.5."""
    ms = np.sort(np.asarray(seconds[skip:], dtype=np.float64) * 1000.0)[::-1]
    out = {a: float(ms[int(len(ms) * (1 - a))]) for a in ratios}
    out[0.5] = float(ms.mean())
    return out


def main(argv=None, parser=None, recognizer=None):
    """-> dict(preds=[str], wer=float or None, logits=[host tensors]).  parser / recognizer: another recipe's command line over
    the same modes (jasper/inference.py): its argparse parser and a function (ckpt, cfg, args, dtype, dev) -> recognizer."""
    args = (parser or build_parser()).parse_args(argv)
    reject_unbuilt(args)
    cfg = apply_overrides(load_config(args.model_config), args.override_config)
    reject_unbuilt(args, cfg)
    wav_input = bool(args.transcribe_wav or args.transcribe_filelist)
    if wav_input and args.dali_device != "none":
        print("DALI supported only with input .json files; disabling")
    os.makedirs(args.output_dir, exist_ok=True)
    log_fpath = args.log_file or os.path.join(args.output_dir, "nvlog_infer.json")
    DLLogger.init(backends=[DLLogger.JSONStreamBackend(DLLogger.Verbosity.DEFAULT, log_fpath, append=True),
                            DLLogger.StdOutBackend(DLLogger.Verbosity.VERBOSE)])
    for k, v in vars(args).items():
        DLLogger.log(step="PARAMETER", data={k: v})
    gen = None
    if args.seed is not None:
        torch.manual_seed(args.seed)
        gen = torch.Generator().manual_seed(args.seed)
    dtype = torch.float16 if args.amp_dtype == "fp16" else torch.bfloat16
    dev = torch.device("cuda", 0)
    if args.ckpt is None:
        raise SystemExit("--ckpt CHECKPOINT is required: a randomly initialised model transcribes nothing")
    ckpt = torch.load(args.ckpt, map_location="cpu", weights_only=False)
    if args.ema and isinstance(ckpt, dict) and "state_dict" in ckpt and "ema_state_dict" not in ckpt:
        print("WARNING: EMA weights are unavailable in %s." % args.ckpt)
    if recognizer is not None:
        rec = recognizer(ckpt, cfg, args, dtype, dev)
    else:
        rec = QuartzNetRecognizer.from_checkpoint(ckpt, cfg, ema=args.ema, dtype=dtype, device=dev)

    if args.transcribe_wav:
        items, bs = [(args.transcribe_wav, None)], 1
    elif args.transcribe_filelist:
        items, bs = [(l.strip(), None) for l in open(args.transcribe_filelist) if l.strip()], 1
    else:
        items, bs = read_manifests(args.dataset_dir, args.val_manifests), args.batch_size
        if cfg["input_val"]["audio_dataset"].get("normalize_transcripts", True):
            items = [(p, normalize_transcript(t, rec.labels)) for p, t in items]
    if not items:
        raise SystemExit("the input lists no utterances")
    batches = [items[i:i + bs] for i in range(0, len(items), bs)]
    measure = args.steps > 0
    steps = (args.steps + args.warmup_steps) or len(batches)
    preds, txts, logits = [], [], []
    dur = {"data": [], "dnn": [], "data+dnn": []}
    for it in range(steps):
        batch = batches[it % len(batches)]
        t0 = time.time()
        feats, lens = rec.features([read_wav(p) for p, _ in batch], gen)
        t1 = time.time()
        texts, _, logp = rec.decode(feats, lens, want_logp=bool(args.save_logits))
        torch.cuda.synchronize()
        t2 = time.time()
        if it >= 1 and (not measure or it >= args.warmup_steps):
            dur["data"].append(t1 - t0)
            dur["dnn"].append(t2 - t1)
            dur["data+dnn"].append(t2 - t0)
        preds += texts
        txts += [t for _, t in batch if t is not None]
        if logp is not None:
            logits += [l.cpu() for l in logp]
    wer = None
    if args.transcribe_wav:
        for i, p in enumerate(preds):
            print("Prediction %3d: %s" % (i + 1, p))
    elif not args.transcribe_filelist:
        wer = word_error_rate(preds, txts)[0]
        DLLogger.log(step=(), data={"eval_wer": 100 * wer})
    if args.save_predictions:
        with open(args.save_predictions, "w") as f:
            f.write("\n".join(preds))
    if args.save_logits:
        torch.save(logits, args.save_logits)
    if len(dur["data"]) >= 20:
        for stage in dur:
            lat = latency_percentiles(dur[stage])
            for k in (0.99, 0.95, 0.9, 0.5):
                DLLogger.log(step=(), data={"%s_latency_%s" % (stage, str(k).replace(".", "_")): lat[k]})
    else:
        print("Not enough samples to measure latencies.")
    DLLogger.flush()
    return dict(preds=preds, wer=wer, logits=logits)


if __name__ == "__main__":
    main(sys.argv[1:])
