"""ResNet-50 train step at the benched shape (batch 256, 224 x 224, bf16; bench.py's Rn50Workload) with and without the weight
average of --use-ema (csrc/multi_tensor.hip mt_ema): two trainers in ONE process on one box, blocks of steps alternating between
them, device events, medians.  Prints one JSON line with
  1. ms per step of the ema=None trainer and of the ema=0.9999 trainer (and their difference),
  2. dle_mt_ema's own event-pair time inside the step and its GB/s over 12 B / element,
  3. the GB/s of dle_mt_sgd over the 53-tensor table (22 B / element) in the same steps -- the sibling stream kernel,
and the launch lists of one step of each trainer (the ema=None step must be the ema step minus its last launch).
    python tools/rn50_ema_ab.py [batch] [steps per block] [rounds]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from deeplearningexamples_amd import _cabi as C
from deeplearningexamples_amd.convnets.engine import ResNetTrainer
from deeplearningexamples_amd.convnets.resnet import ResNet50

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
MU = 0.9999
dev = torch.device("cuda", 0)


def build(ema):
    torch.manual_seed(0)
    m = ResNet50(device=dev)
    return ResNetTrainer(m, lr=0.256 * batch / 256, momentum=0.875, weight_decay=3.0517578125e-05, label_smoothing=0.1,
                         compute_dtype=torch.bfloat16, static_loss_scale=128.0, ema=ema)


g = torch.Generator(device="cpu").manual_seed(1000)
x = torch.randn((batch, 3, 224, 224), generator=g).to(dev)
y = torch.randint(0, 1000, (batch,), generator=g).to(dev)
trainers = {"off": build(None), "on": build(MU)}
it = {"off": 0, "on": 0}


def run(name, n):
    tr = trainers[name]
    for _ in range(n):
        if name == "on":
            loss = tr.train_step(x, y, step=it[name])
        else:
            loss = tr.train_step(x, y)
        it[name] += 1
    return loss


def block_ms(name, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run(name, n)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n


out = {"batch": batch, "steps_per_block": steps, "rounds": rounds, "mu": MU}
for name in trainers:                      # warm-up: code objects, the allocator's pool, every shape of the step
    run(name, 5)
torch.cuda.synchronize()
ms = {"off": [], "on": []}
for r in range(rounds):
    for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
        ms[name].append(block_ms(name, steps))
for name in ms:
    out["step_ms_ema_" + name] = round(statistics.median(ms[name]), 4)
    out["step_ms_ema_%s_blocks" % name] = [round(v, 4) for v in ms[name]]
out["step_ms_difference"] = round(out["step_ms_ema_on"] - out["step_ms_ema_off"], 4)

# ---- per-launch event pairs (every kernel in line on one stream, as bench.py's per-kernel pass): the two stream kernels' own time
launches = {}
agg = {}
for name, tr in trainers.items():
    tr.set_side_streams(False)
    run(name, 2)
    timer = C.KernelTimer()
    C.set_timer(timer)
    run(name, 1)
    launches[name] = [(n, (m or {}).get("tag")) for n, _, _, m in timer.records]
    timer.records = []
    run(name, 10)
    C.set_timer(None)
    torch.cuda.synchronize()
    per = {}
    for n, s, e, m in timer.records:
        per.setdefault((n, (m or {}).get("tag")), []).append((s.elapsed_time(e), (m or {}).get("bytes", 0.0)))
    agg[name] = per
    tr.set_side_streams(True)


def kernel_figures(per, entry, pick):
    keys = [k for k in per if k[0] == entry]
    if not keys:
        return None
    k = pick(keys)
    t = statistics.median(v[0] for v in per[k])
    b = per[k][0][1]
    return {"tag": k[1], "median_ms": round(t, 4), "bytes": b, "GB_per_s": round(b / t / 1e6, 1), "calls": len(per[k])}


biggest = lambda keys: max(keys, key=lambda k: int(k[1].split(",")[1][:-1]))   # noqa: E731  ("53t,25493504e": by element count)
out["mt_ema_in_step"] = kernel_figures(agg["on"], "dle_mt_ema", biggest)
out["mt_sgd_in_step_ema_on"] = kernel_figures(agg["on"], "dle_mt_sgd", biggest)
out["mt_sgd_in_step_ema_off"] = kernel_figures(agg["off"], "dle_mt_sgd", biggest)
tab = trainers["on"].t_ema
out["mt_ema_table"] = {"tensors": tab.n, "elements": tab.total_elems, "chunk": tab.chunk, "workgroups": tab.total_chunks,
                       "tensors_under_2048": sum(1 for t in tab._keep[0] if t.numel() < 2048)}

# ---- the launch under the averaged update alone, back to back (one event pair around many launches: no per-call host gap; its
# 205 MB working set largely stays in the 256 MB Infinity Cache between launches, so this is NOT the in-step figure)
from deeplearningexamples_amd import multi_tensor as mt   # noqa: E402
tr = trainers["on"]
for _ in range(3):
    mt.ema(tr.t_ema, MU, coef=tr.ema_coef)
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
s.record()
for _ in range(50):
    mt.ema(tr.t_ema, MU, coef=tr.ema_coef)
e.record()
torch.cuda.synchronize()
t = s.elapsed_time(e) / 50
out["mt_ema_back_to_back"] = {"ms": round(t, 4), "GB_per_s": round(tab.total_elems * 12 / t / 1e6, 1)}

# ---- launch lists: a step without the average is the step with it minus the last launch
names_off = [n for n, _ in launches["off"]]
names_on = [n for n, _ in launches["on"]]
out["launches_per_step_ema_off"] = len(names_off)
out["launches_per_step_ema_on"] = len(names_on)
out["ema_on_extra_launches"] = names_on[len(names_off):] if names_on[:len(names_off)] == names_off else "launch lists differ before the end"
out["ema_is_last_launch"] = bool(names_on) and names_on[-1] == "dle_mt_ema"
out["device"] = torch.cuda.get_device_name(0)
print(json.dumps(out))
