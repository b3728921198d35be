"""Command line of the SSD300 recipe (PyTorch/Detection/SSD/main.py:53-127): every flag of the reference parses.

    python -m deeplearningexamples_amd.ssd.main --data /coco --mode evaluation --checkpoint epoch_64.pt [--json-summary out.json]
    python -m deeplearningexamples_amd.ssd.main --data /coco --mode benchmark-inference --eval-batch-size 32

--mode evaluation runs SSDDetector over COCO val2017 (<data>/annotations/instances_val2017.json, <data>/val2017), writes the
detections in the reference's 7-column form (ssd/evaluate.py:62-67: image id, x, y, w, h in pixels, score, category id) as a
COCO-results JSON and, when pycocotools imports, prints the reference's `Model precision ... mAP` line.  --mode
benchmark-inference prints the reference's throughput line for the network alone (what the reference times) and for the network
with the detection.  Training is not built here.
"""
import json
import os
import sys
import time
from argparse import ArgumentParser

import numpy as np
import torch

from . import model as M

MODES = ("training", "evaluation", "benchmark-training", "benchmark-inference")


def make_parser():
    p = ArgumentParser(description="Single Shot MultiBox Detector on COCO: inference on the gfx950 library")
    p.add_argument("--data", "-d", type=str, default="/coco", required=True, help="path to the COCO files")
    p.add_argument("--epochs", "-e", type=int, default=65)
    p.add_argument("--batch-size", "--bs", type=int, default=32)
    p.add_argument("--eval-batch-size", "--ebs", type=int, default=32, help="images per evaluation batch")
    p.add_argument("--no-cuda", action="store_true")
    p.add_argument("--seed", "-s", type=int)
    p.add_argument("--checkpoint", type=str, default=None, help="the reference's checkpoint ({'model': ...}) or a state dict")
    p.add_argument("--torchvision-weights-version", type=str, default="IMAGENET1K_V2", choices=["IMAGENET1K_V1", "IMAGENET1K_V2", "DEFAULT"])
    p.add_argument("--save", type=str, default=None)
    p.add_argument("--mode", type=str, default="training", choices=list(MODES))
    p.add_argument("--evaluation", nargs="*", type=int, default=[21, 31, 37, 42, 48, 53, 59, 64])
    p.add_argument("--multistep", nargs="*", type=int, default=[43, 54])
    p.add_argument("--learning-rate", "--lr", type=float, default=2.6e-3)
    p.add_argument("--momentum", "-m", type=float, default=0.9)
    p.add_argument("--weight-decay", "--wd", type=float, default=0.0005)
    p.add_argument("--warmup", type=int, default=None)
    p.add_argument("--benchmark-iterations", type=int, default=20, metavar="N")
    p.add_argument("--benchmark-warmup", type=int, default=20, metavar="N")
    p.add_argument("--backbone", type=str, default="resnet50", choices=list(M.BACKBONES))
    p.add_argument("--backbone-path", type=str, default=None)
    p.add_argument("--num-workers", type=int, default=8)
    p.add_argument("--amp", dest="amp", action="store_true", help="16-bit inference (the only precision built)")
    p.add_argument("--no-amp", dest="amp", action="store_false")
    p.set_defaults(amp=True)
    p.add_argument("--allow-tf32", dest="allow_tf32", action="store_true")
    p.add_argument("--no-allow-tf32", dest="allow_tf32", action="store_false")
    p.set_defaults(allow_tf32=True)
    p.add_argument("--data-layout", default="channels_last", choices=["channels_first", "channels_last"])
    p.add_argument("--log-interval", type=int, default=20)
    p.add_argument("--json-summary", type=str, default=None, help="evaluation: where the COCO-results JSON goes")
    p.add_argument("--local_rank", default=os.getenv("LOCAL_RANK", 0), type=int)
    # this project's own
    p.add_argument("--dtype", choices=["bf16", "fp16"], default="fp16", help="16-bit type of the activations and weights")
    p.add_argument("--graphs", action="store_true", help="replay one captured graph per batch shape")
    p.add_argument("--width", type=int, default=1, help="channel divisor of a randomly initialised network (no --checkpoint)")
    return p


def reject(args):
    """The one-line rejections: -> the message, or None."""
    if args.mode in ("training", "benchmark-training"):
        return "--mode %s: training is not built here (inference only: --mode evaluation or benchmark-inference)" % args.mode
    if args.backbone != "resnet50":
        return "--backbone %s: only the resnet50 backbone is built" % args.backbone
    if not args.amp:
        return "--no-amp: this path computes in 16 bits (fp32 / TF32 inference is not built)"
    if args.no_cuda:
        return "--no-cuda: the kernels run on the GPU only"
    return None


class COCODetection:
    """The validation reader (ssd/utils.py:462-555 with the SSDTransformer of validation, :426-436): annotation JSON + PIL.
    Yields (uint8 image [3, 300, 300] resized as transforms.Resize((300, 300)) does (bilinear, antialiased), image id,
    (height, width)); the normalisation with the ImageNet mean / std happens on the device."""

    def __init__(self, img_folder, annotate_file, size=(300, 300)):
        with open(annotate_file) as f:
            data = json.load(f)
        self.img_folder, self.size = img_folder, size
        self.label_map, self.label_info = {}, {0: "background"}
        for cnt, cat in enumerate(data["categories"], 1):
            self.label_map[cat["id"]] = cnt
            self.label_info[cnt] = cat["name"]
        self.images = {}
        for img in data["images"]:
            if img["id"] in self.images:
                raise ValueError("duplicated image record %r" % (img["id"],))
            self.images[img["id"]] = (img["file_name"], (img["height"], img["width"]))
        annotated = {a["image_id"] for a in data.get("annotations", [])}
        self.img_keys = [k for k in self.images if k in annotated]        # the reference drops images without boxes

    def __len__(self):
        return len(self.img_keys)

    def __getitem__(self, idx):
        from PIL import Image
        img_id = self.img_keys[idx]
        name, (h, w) = self.images[img_id]
        img = Image.open(os.path.join(self.img_folder, name)).convert("RGB").resize((self.size[1], self.size[0]), Image.BILINEAR)
        return torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous(), img_id, (h, w)

    def batches(self, batch_size):
        for i in range(0, len(self), batch_size):
            items = [self[j] for j in range(i, min(i + batch_size, len(self)))]
            yield torch.stack([it[0] for it in items]), [it[1] for it in items], [it[2] for it in items]


def results_rows(decoded, img_ids, img_sizes, inv_map):
    """evaluate.py:59-67: the 7 columns per detection."""
    rows = []
    for (boxes, labels, scores), img_id, (htot, wtot) in zip(decoded, img_ids, img_sizes):
        for loc, label, prob in zip(boxes.tolist(), labels.tolist(), scores.tolist()):
            rows.append([img_id, loc[0] * wtot, loc[1] * htot, (loc[2] - loc[0]) * wtot, (loc[3] - loc[1]) * htot, prob, inv_map[label]])
    return rows


def write_results(rows, path):
    """COCO-results JSON of the 7-column rows."""
    out = [dict(image_id=int(r[0]), bbox=[float(np.float32(v)) for v in r[1:5]], score=float(np.float32(r[5])), category_id=int(r[6]))
           for r in rows]
    with open(path, "w") as f:
        json.dump(out, f)
    return len(out)


def coco_map(annotate_file, results_path):
    """The reference's COCOeval (evaluate.py:117-124) when pycocotools imports; None otherwise."""
    try:
        from pycocotools.coco import COCO
        from pycocotools.cocoeval import COCOeval
    except ImportError:
        return None
    gt = COCO(annotation_file=annotate_file)
    e = COCOeval(gt, gt.loadRes(results_path), iouType="bbox")
    e.evaluate()
    e.accumulate()
    e.summarize()
    return float(e.stats[0])


def build_detector(args):
    from .infer import SSDDetector
    dtype = torch.float16 if args.dtype == "fp16" else torch.bfloat16
    if args.checkpoint is not None:
        return SSDDetector.from_checkpoint(args.checkpoint, dtype=dtype, graphs=args.graphs)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    return SSDDetector(M.SSD300("resnet50", width=args.width).to("cuda").eval(), dtype=dtype, graphs=args.graphs)


def evaluate(det, args):
    annotate = os.path.join(args.data, "annotations", "instances_val2017.json")
    coco = COCODetection(os.path.join(args.data, "val2017"), annotate)
    inv_map = {v: k for k, v in coco.label_map.items()}
    rows, start = [], time.time()
    for images, ids, sizes in coco.batches(args.eval_batch_size):
        rows += results_rows(det.decode_batch(images, 0.50, 200), ids, sizes, inv_map)
    print("Predicting Ended, total time: {:.2f} s".format(time.time() - start))
    path = args.json_summary or os.path.join(args.save or ".", "ssd_detections.json")
    print("wrote %d detections of %d images to %s" % (write_results(rows, path), len(coco), path))
    acc = coco_map(annotate, path) if rows else None
    if acc is None:
        print("pycocotools is not installed (or nothing was detected): no mAP; score %s with COCOeval" % path)
    else:
        print("Model precision {} mAP".format(acc))
    return path


def benchmark_inference(det, args):
    n = args.eval_batch_size
    images = torch.randint(0, 256, (n, 3, 300, 300), dtype=torch.uint8, device="cuda")
    for what, fn in (("network", det.head_outputs), ("network + detection", det.detect)):
        times = []
        for i in range(args.benchmark_warmup + args.benchmark_iterations):
            torch.cuda.synchronize()
            t0 = time.time()
            fn(images)
            torch.cuda.synchronize()
            if i >= args.benchmark_warmup:
                times.append(time.time() - t0)
        total, ips = sum(times), n / np.asarray(times)
        print("{}: Done benchmarking. Total images: {}\ttotal time: {:.3f}\tAverage images/sec: {:.3f}\tMedian images/sec: {:.3f}".format(
            what, n * len(times), total, n * len(times) / total, float(np.median(ips))))


def main(argv=None):
    args = make_parser().parse_args(argv)
    msg = reject(args)
    if msg:
        print(msg)
        return 2
    det = build_detector(args)
    if args.mode == "evaluation":
        evaluate(det, args)
    else:
        benchmark_inference(det, args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
