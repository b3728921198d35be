"""Transformer-XL evaluation timing on the MI355X: the relative attention kernel against a torch composition of the reference's
tensor operations, and whole segments with the K/V cache against recomputing K and V of the whole window.

    python tools/txl_infer_perf.py [--reps 10] [--out profiles/txl_infer_perf.json]

(a) Kernel.  dle_txl_rel_attention_fwd at the base shape (batch 16, 8 heads, 64 queries, memory 0 / 64 / 320 / 640) and the large
shape (batch 16, 16 heads, 128 queries, memory 0 / 128 / 800 / 1600): the steady state and the warm-up lengths; fp16 everywhere
and bf16 at the two steady states; same_length off and on (the band then skips key tiles).
  `new`         one F.txl_rel_attention_fwd launch over a zero-start ring;
  `comparator`  the five tensor operations of RelPartialLearnableMultiHeadAttn.forward (mem_transformer.py:266-288) on the same
                device in the same 16-bit type, in the reference's layouts: the two einsums AC and BD, _rel_shift, (AC + BD) * scale
                with masked_fill and softmax, the einsum with V.  Its output is compared with the kernel's once, before timing.
Both run in one process, alternated sample by sample after 3 warm-up launches each; a sample is LAUNCHES launches between two
device events.  Reported: median, minimum, `spread_pct` (median of the even against the odd samples), `new_over_comparator`,
`loses` where that exceeds 1.05.  Bounds, from the shapes: `t_mfma_us` = the matrix-instruction work the KERNEL issues (per visited
32 x 32 tile pair 16 instructions of 32 x 32 x 16: 4 for AC, 8 for the 64-distance band, 4 for the context; masked-out tiles
are not visited) at 2500 TFLOP/s, beside `t_mfma_min_us`, the same at the algorithm's 3 x 2 x 64 flops per allowed (query, key)
pair; `t_kv_us` = the ring rows each (batch element, head) reads once (klen x 128 x 2 bytes for K and V) at 8000 GB/s.

(b) Segments.  TransformerXLEvaluator at the base (16 layers, d_model 512, div_val 1, tgt_len 64, mem_len 640) and large (18 layers,
d_model 1024, div_val 4, tgt_len 128, mem_len 1600) configurations of wt103_{base,large}.yaml with seeded random weights, in the
steady state (full memory), fp16 and bf16, batch 1 / 4 / 16 / 32, against `Recompute`, a variant kept in THIS FILE only: it
keeps the hidden states of the window per layer and projects all mem_len + tgt_len rows to Q, K and V in every segment, as the
reference does (mem_transformer.py:239-247), then runs the same attention kernel on the freshly written ring.  Token ids are
drawn log-uniformly over the vocabulary (79 % fall into the shortlist, as frequent words do in text; uniform ids would send
60 % of the rows to the 160,000-class tail).  A sample is one segment() between device events, host bucketing included;
alternated, after 3 warm-up segments each.  Reported: median ms per segment, tokens/s, `cache_over_recompute`.
Nothing here fixes a speed in advance.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS, MFMA_PEAK_TFLOPS = 8000.0, 2500.0
LAUNCHES = 10
BASE = dict(n_token=267735, n_layer=16, n_head=8, d_model=512, d_head=64, d_inner=2048, d_embed=512, div_val=1,
            tie_projs=[False, True, True, True], cutoffs=[19997, 39997, 199997], tgt_len=64, mem_len=640, clamp_len=400, same_length=True)
LARGE = dict(n_token=267735, n_layer=18, n_head=16, d_model=1024, d_head=64, d_inner=4096, d_embed=1024, div_val=4,
             tie_projs=[False, True, True, True], cutoffs=[19997, 39997, 199997], tgt_len=128, mem_len=1600, clamp_len=1000, same_length=True)


def summarise(ms):
    even, odd = statistics.median(ms[0::2]), statistics.median(ms[1::2])
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), spread_pct=100.0 * abs(even - odd) / min(even, odd))


def sample(call, launches=LAUNCHES):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(launches):
        call()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / launches


def tiles_visited(qlen, mlen, shift):
    n = 0
    klen = qlen + mlen
    for i0 in range(0, qlen, 32):
        ilast = min(i0 + 31, qlen - 1)
        jlo, jhi = max(0, i0 - shift + 1), min(klen - 1, ilast + mlen)
        n += jhi // 32 - jlo // 32 + 1
    return n


def kernel_leg(reps):
    import torch
    from deeplearningexamples_amd import functional as F
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    plan = [("base", 16, 8, 64, m, torch.float16) for m in (0, 64, 320, 640)] + [("base", 16, 8, 64, 640, torch.bfloat16)] + \
           [("large", 16, 16, 128, m, torch.float16) for m in (0, 128, 800, 1600)] + [("large", 16, 16, 128, 1600, torch.bfloat16)]
    for name, b, nh, qlen, mlen, dt in plan:
        mem_len = 640 if name == "base" else 1600
        for same in (False, True):
            klen, h = qlen + mlen, nh * 64
            mask_len = klen - mem_len - 1
            shift = (qlen - mask_len if mask_len > 0 else qlen) if same else qlen
            rnd = lambda *s: torch.randn(*s, generator=g, device=dev).to(dt)
            qkv, u, v, kv, r = rnd(b * qlen, 3 * h), 0.5 * rnd(nh, 64), 0.5 * rnd(nh, 64), rnd(b, klen, 2 * h), rnd(klen, h)
            ctx = torch.empty(b * qlen, h, dtype=dt, device=dev)
            scale = 0.125
            new = lambda: F.txl_rel_attention_fwd(qkv[:, :h], u, v, kv, r, nh, qlen, mlen, 0, shift, scale, out=ctx)
            # the reference's layouts: [len, bsz, n_head, d_head]; r_head_k [klen, n_head, d_head] for pos_seq = klen-1 .. 0
            wq = qkv[:, :h].reshape(b, qlen, nh, 64).permute(1, 0, 2, 3).contiguous()
            wk = kv[:, :, :h].reshape(b, klen, nh, 64).permute(1, 0, 2, 3).contiguous()
            wv = kv[:, :, h:].reshape(b, klen, nh, 64).permute(1, 0, 2, 3).contiguous()
            rk = r.flip(0).reshape(klen, nh, 64).contiguous()
            i, j = torch.arange(qlen, device=dev)[:, None], torch.arange(klen, device=dev)[None, :]
            mask = ~((i - shift < j) & (j <= i + mlen))

            def old():
                ac = torch.einsum("ibnd,jbnd->bnij", wq + u, wk)
                bd = torch.einsum("ibnd,jnd->bnij", wq + v, rk)
                zp = torch.zeros((b, nh, qlen, 1), device=dev, dtype=dt)
                bd = torch.cat([zp, bd], dim=3).view(b, nh, klen + 1, qlen).narrow(2, 1, klen).view(b, nh, qlen, klen)
                score = ((ac + bd) * scale).masked_fill_(mask[None, None], -float("inf"))
                prob = torch.softmax(score, dim=3)
                return torch.einsum("bnij,jbnd->ibnd", prob, wv)

            new()
            ref = old().permute(1, 0, 2, 3).reshape(b * qlen, h)
            torch.cuda.synchronize()
            diff = float((ref.float() - ctx.float()).abs().max())
            for _ in range(3):
                new()
                old()
            ms_new, ms_old = [], []
            for _ in range(reps):
                ms_new.append(sample(new))
                ms_old.append(sample(old))
            nt = tiles_visited(qlen, mlen, shift)
            issued = float(b * nh * nt) * 16 * 2 * 32 * 32 * 16
            allowed = float(((~mask).sum()).item())
            rec = dict(model=name, batch=b, heads=nh, qlen=qlen, mlen=mlen, dtype=str(dt), same_length=same, shift=shift,
                       new=summarise(ms_new), comparator=summarise(ms_old), max_abs_diff_against_comparator=diff,
                       tiles_visited=nt, t_mfma_us=issued / (MFMA_PEAK_TFLOPS * 1e6),
                       t_mfma_min_us=b * nh * allowed * 3 * 2 * 64 / (MFMA_PEAK_TFLOPS * 1e6),
                       t_kv_us=float(b) * klen * 2 * h * 2 / (HBM_PEAK_GBS * 1e3))
            t = rec["new"]["median_ms"] * 1e3
            rec.update(frac_of_mfma_bound=rec["t_mfma_us"] / t, frac_of_kv_bound=rec["t_kv_us"] / t,
                       new_over_comparator=rec["new"]["median_ms"] / rec["comparator"]["median_ms"])
            rec["loses"] = rec["new_over_comparator"] > 1.05
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def random_model(cfg, seed):
    import torch
    from deeplearningexamples_amd.transformer_xl.model import TransformerXLModel, check_config, state_shapes
    g = torch.Generator().manual_seed(seed)
    cfg = check_config(cfg)
    st = {}
    for k, shape in state_shapes(cfg).items():
        if k.startswith("crit.shared_out_projs.") or k == "pos_emb.inv_freq":
            continue
        if k.endswith("layer_norm.weight"):
            st[k] = torch.ones(shape)
        elif len(shape) == 1:
            st[k] = torch.zeros(shape)
        else:
            st[k] = torch.randn(shape, generator=g) * (0.02 if k.startswith("word_emb.emb_layers") else shape[-1] ** -0.5)
    return TransformerXLModel(cfg).load_state_dict(st)


def log_uniform_ids(n_token, shape, g):
    import torch
    return torch.exp(torch.rand(shape, generator=g) * math.log(n_token)).long().clamp(max=n_token - 1)


def make_recompute(base):
    """The tool-only variant: hidden-state memory, Q / K / V of the whole window projected in every segment."""
    import torch
    from deeplearningexamples_amd import _cabi as C
    from deeplearningexamples_amd import functional as F
    from deeplearningexamples_amd.transformer_xl.infer import LN_EPS

    class Recompute(base):
        def reset(self):
            self.mems = [torch.zeros((self.bsz, 0, self.d_model), dtype=self.dtype, device=self.dev) for _ in self.layers]
            self.start, self.mlen = 0, 0

        def segment(self, data, target):
            qlen, bsz = data.shape
            dev, dt, R, dm, H = self.dev, self.dtype, qlen * bsz, self.d_model, self.H
            host, plan = self.bucket(data, target)
            mlen = self.mlen
            klen = mlen + qlen
            mask_len = klen - self.mem_len - 1
            shift = (qlen - mask_len if mask_len > 0 else qlen) if self.cfg["same_length"] else qlen
            with torch.no_grad():
                idx = torch.from_numpy(host).to(dev, non_blocking=True)
                cut = lambda s: idx[s[0]:s[0] + s[1]]
                x = torch.empty((R, dm), dtype=dt, device=dev)
                for i, src, dst in plan["emb"]:
                    n, proj = src[1], self.emb_proj[i]
                    if proj is None:
                        F.rows_gather_scale(self.emb[i], x, n, src_idx=cut(src), dst_idx=None if dst is None else cut(dst), scale=self.emb_scale)
                    else:
                        e = torch.empty((n, self.emb[i].shape[1]), dtype=dt, device=dev)
                        F.rows_gather_scale(self.emb[i], e, n, src_idx=cut(src))
                        F.rows_gather_scale(F.gemm(e, proj, n, dm, e.shape[1], True, True), x, n, dst_idx=None if dst is None else cut(dst),
                                            scale=self.emb_scale)
                new_mems = []
                for L, mem in zip(self.layers, self.mems):
                    cat = torch.cat([mem, x.view(bsz, qlen, dm)], 1)                              # [bsz, klen, dm]
                    new_mems.append(cat[:, max(0, klen - self.mem_len):])
                    qkv = F.gemm(cat.view(bsz * klen, dm), L.qkv, bsz * klen, 3 * H, dm, True, True)
                    F.txl_kv_append(qkv, L.kv, klen, 0, 0)
                    q = qkv.view(bsz, klen, 3 * H)[:, mlen:, :H].reshape(R, H)
                    ctx = F.txl_rel_attention_fwd(q, self.u, self.v, L.kv, L.r, self.nh, qlen, mlen, 0, shift, self.scale)
                    ao = F.gemm(ctx, L.o, R, dm, H, True, True)
                    x = F.layernorm_fwd(ao, L.ln1[0], L.ln1[1], residual=x, eps=LN_EPS, write_z=False)[0]
                    h1 = F.gemm(x, L.ff1[0], R, L.ff1[0].shape[0], dm, True, True, bias=L.ff1[1], act=C.ACT_RELU)
                    h2 = F.gemm(h1, L.ff2[0], R, dm, h1.shape[1], True, True, bias=L.ff2[1])
                    x = F.layernorm_fwd(h2, L.ln2[0], L.ln2[1], residual=x, eps=LN_EPS, write_z=False)[0]
                self.mems = new_mems
                nll = torch.empty(R, dtype=torch.float32, device=dev)
                F.row_nll(self._logits(x, 0, R), cut(plan["head"][0]), nll, pos=cut(plan["head"][1]))
                for i, rows, tgt, pos in plan["tails"]:
                    n = rows[1]
                    hi = torch.empty((n, dm), dtype=dt, device=dev)
                    F.rows_gather_scale(x, hi, n, src_idx=cut(rows))
                    F.row_nll(self._logits(hi, i, n), cut(tgt), nll, pos=cut(pos), accumulate=True)
            self.mlen = min(self.mem_len, klen)
            return nll.view(qlen, bsz)

    return Recompute


def segment_leg(reps, batches):
    import torch
    from deeplearningexamples_amd.transformer_xl.infer import TransformerXLEvaluator
    Recompute = make_recompute(TransformerXLEvaluator)
    out = []
    for name, cfg in (("base", BASE), ("large", LARGE)):
        model = random_model(cfg, 3)
        tgt, mem = cfg["tgt_len"], cfg["mem_len"]
        fill = (mem + tgt - 1) // tgt
        for dt in (torch.float16, torch.bfloat16):
            for bsz in batches:
                g = torch.Generator().manual_seed(bsz)
                stream = [(log_uniform_ids(cfg["n_token"], (tgt, bsz), g), log_uniform_ids(cfg["n_token"], (tgt, bsz), g))
                          for _ in range(fill + 3 + reps)]
                evs = dict(cache=TransformerXLEvaluator(model, bsz, dtype=dt), recompute=Recompute(model, bsz, dtype=dt))
                for ev in evs.values():
                    ev.reset()
                    for d, t in stream[:fill + 3]:                        # fills the memory, then three warm-up segments
                        last = ev.segment(d, t)
                torch.cuda.synchronize()
                # the two variants compute the same thing: their losses agree to the 16-bit working precision
                a = evs["cache"].segment(*stream[fill + 2]).float()
                bb = evs["recompute"].segment(*stream[fill + 2]).float()
                diff = float((a - bb).abs().max())
                ms = dict(cache=[], recompute=[])
                for d, t in stream[fill + 3:]:
                    for k, ev in evs.items():
                        ms[k].append(sample(lambda: ev.segment(d, t), launches=1))
                rec = dict(model=name, dtype=str(dt), batch=bsz, tgt_len=tgt, mem_len=mem, max_abs_nll_diff=diff,
                           cache=summarise(ms["cache"]), recompute=summarise(ms["recompute"]))
                for k in ("cache", "recompute"):
                    rec[k]["tokens_per_s"] = bsz * tgt / (rec[k]["median_ms"] * 1e-3)
                rec["cache_over_recompute"] = rec["cache"]["median_ms"] / rec["recompute"]["median_ms"]
                print(json.dumps(rec), flush=True)
                out.append(rec)
                del evs
                torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4, 16, 32])
    ap.add_argument("--skip-segments", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "txl_infer_perf.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    result = dict(device=torch.cuda.get_device_name(0), reps=args.reps, launches_per_sample=LAUNCHES,
                  peaks=dict(hbm_gbs=HBM_PEAK_GBS, mfma_tflops=MFMA_PEAK_TFLOPS), kernel=kernel_leg(args.reps))
    if not args.skip_segments:
        result["segments"] = segment_leg(args.reps, args.batches)
    rows = result["kernel"] + sum(([r["cache"], r["recompute"]] for r in result.get("segments", [])), [])
    result["spread_pct_max"] = max(r["spread_pct"] if "spread_pct" in r else max(r["new"]["spread_pct"], r["comparator"]["spread_pct"])
                                   for r in rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
