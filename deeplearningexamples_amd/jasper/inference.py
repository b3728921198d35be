"""Entry point mirroring SpeechRecognition/Jasper/inference.py: .wav files (or a manifest) -> transcripts (and WER).

    python -m deeplearningexamples_amd.jasper.inference --model_config jasper10x5dr_speedp-online_speca.yaml \
        --ckpt Jasper_checkpoint.pt --ema --amp --transcribe_wav speech.wav [--amp-dtype bf16]
    python -m deeplearningexamples_amd.jasper.inference --model_config CONFIG.yaml --ckpt CKPT.pt --amp --dataset_dir LibriSpeech \
        --val_manifests librispeech-dev-clean-wav.json --dali_device none --batch_size 16 \
        --override_config input_val.audio_dataset.trim_silence=false

The flag names are the reference's (inference.py:45-98) plus --amp-dtype; every flag of its parser parses.  The modes, the WER,
the latency report and the one-line refusals (--cpu, --torchscript*, DALI on a manifest, .nemo, several GPUs, fp32) are those of
quartznet/inference.py, whose code this module runs; what Jasper adds is --pad_leading (default 16): that many zero frames in front
of every utterance's normalised features (inference.py:329-333), and the key names of the first release's checkpoints.
"""
import sys

from ..quartznet import inference as qn
from .infer import JasperRecognizer


def build_parser():
    p = qn.build_parser()
    p.description = "Jasper inference on MI355X"
    p.add_argument("--pad_leading", type=int, default=16,
                   help="pads every utterance with leading zero frames to counteract conv shifts of the field of view")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def _recognizer(ckpt, cfg, args, dtype, dev):
    if args.pad_leading < 0:
        raise SystemExit("--pad_leading %d: must not be negative" % args.pad_leading)
    return JasperRecognizer.from_checkpoint(ckpt, cfg, ema=args.ema, dtype=dtype, device=dev, pad_leading=args.pad_leading)


def main(argv=None):
    """-> dict(preds=[str], wer=float or None, logits=[host tensors])."""
    return qn.main(argv, parser=build_parser(), recognizer=_recognizer)


if __name__ == "__main__":
    main(sys.argv[1:])
