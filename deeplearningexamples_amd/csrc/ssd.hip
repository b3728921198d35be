// SSD300 detection post-processing: box decode + softmax, per-class greedy non-maximum suppression, per-image selection.
//
// Replaces (PyTorch/Detection/SSD/ssd/):
//   model.py:108-115    SSD300.bbox_view (the NCHW reshape of the head outputs to [N, 4, B] / [N, L, B] and their concatenation)
//   utils.py:127-159    Encoder.scale_back_batch (scale, default-box transform, xywh -> ltrb, softmax over the labels)
//   utils.py:32-66      calc_iou_tensor
//   utils.py:172-221    Encoder.decode_single (the Python loop over 80 classes, one .item() and one IoU tensor per suppression step,
//                       and the final cut to max_output)
//
//  * ssd_decode_kernel: thread = (image, box).  Inside a map threads are ordered (pixel, anchor) so that a wavefront reads
//    neighbouring channels of neighbouring pixels; the box index it writes is anchor * H * W + pixel (the reference's reshape).
//    fp32 arithmetic in the reference's operation order, three passes over the L logits of the box (max, sum, quotient).
//  * ssd_nms_kernel: one 256-thread workgroup per (image, label >= 1).  It streams the probability row, compacts the candidates
//    (prob > threshold) in index order with wavefront ballots (no atomics), sorts their 64-bit keys (ordered score bits, then the
//    complemented box index: the lower index wins a tie) with a bitonic network in LDS, takes the best max_num, builds the
//    max_num x max_num suppression bits (bit (i, j), j > i: !(iou < criteria), so a NaN suppresses) with one ballot per (row,
//    wavefront), and wavefront 0 sweeps them serially 64 rows at a time (rows in registers, v_readlane per kept row).
//  * ssd_select_kernel: one workgroup per image: the first min(count, max_output) entries of every class list, compacted in
//    (label, rank) order, sorted by (score, lower label, lower box index), the best max_output written with their boxes.
//
// Contraction is off in this file: the IoU and the decode are sequences of separately rounded fp32 operations, as torch's.
#include "common.h"

#pragma clang fp contract(off)

#define SSD_THREADS 256
#define SSD_WAVES (SSD_THREADS / 64)
static_assert(DLE_SSD_MAX_KEEP == SSD_THREADS, "one thread per candidate of the suppression stage");

struct SsdMaps {
  const unsigned short* head[DLE_SSD_MAX_MAPS];
  int fs[DLE_SSD_MAX_MAPS], nd[DLE_SSD_MAX_MAPS], pitch[DLE_SSD_MAX_MAPS], loc[DLE_SSD_MAX_MAPS], conf[DLE_SSD_MAX_MAPS];
  int start[DLE_SSD_MAX_MAPS + 1];
  int n;
};

// ------------------------------------------------------------------------------------------------------------------ decode
template <int DT>
__global__ __launch_bounds__(SSD_THREADS) void ssd_decode_kernel(SsdMaps maps, const float* __restrict__ dboxes, float* __restrict__ boxes,
                                                                 float* __restrict__ probs, int N, int B, int L, float scale_xy,
                                                                 float scale_wh) {
  const long long gid = (long long)blockIdx.x * SSD_THREADS + threadIdx.x;
  if (gid >= (long long)N * B) return;
  const int n = (int)(gid / B), t = (int)(gid - (long long)n * B);
  int m = 0;
  while (m + 1 < maps.n && t >= maps.start[m + 1]) ++m;
  const int fs = maps.fs[m], nd = maps.nd[m], hw = fs * fs;
  const int local = t - maps.start[m];
  const int pix = local / nd, a = local - pix * nd;
  const int b = maps.start[m] + a * hw + pix;
  const unsigned short* px = maps.head[m] + ((long long)n * hw + pix) * maps.pitch[m];
  // ---- box: loc channel c is coordinate c / nd of anchor c % nd
  const unsigned short* pl = px + maps.loc[m] + a;
  const float lx = Elem<DT>::to_f32(pl[0]), ly = Elem<DT>::to_f32(pl[nd]);
  const float lw = Elem<DT>::to_f32(pl[2 * nd]), lh = Elem<DT>::to_f32(pl[3 * nd]);
  const float4_t d = *(const float4_t*)(dboxes + (long long)b * 4);
  const float x = (scale_xy * lx) * d[2] + d[0];
  const float y = (scale_xy * ly) * d[3] + d[1];
  const float w = expf(scale_wh * lw) * d[2];
  const float h = expf(scale_wh * lh) * d[3];
  float4_t o;
  o[0] = x - 0.5f * w;
  o[1] = y - 0.5f * h;
  o[2] = x + 0.5f * w;
  o[3] = y + 0.5f * h;
  *(float4_t*)(boxes + ((long long)n * B + b) * 4) = o;
  // ---- softmax over the labels: conf channel c is label c / nd of anchor c % nd
  const unsigned short* pc = px + maps.conf[m] + a;
  float mx = Elem<DT>::to_f32(pc[0]);
  for (int l = 1; l < L; ++l) mx = fmaxf(mx, Elem<DT>::to_f32(pc[l * nd]));
  float sum = 0.f;
  for (int l = 0; l < L; ++l) sum += expf(Elem<DT>::to_f32(pc[l * nd]) - mx);
  float* pp = probs + (long long)n * L * B + b;
  for (int l = 0; l < L; ++l) pp[(long long)l * B] = __fdiv_rn(expf(Elem<DT>::to_f32(pc[l * nd]) - mx), sum);
}

extern "C" int dle_ssd_decode_fwd(const void* const* heads, const int* geom, int nmaps, const float* dboxes_xywh, float* boxes,
                                  float* probs, int N, int B, int L, float scale_xy, float scale_wh, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "ssd_decode_fwd: 16-bit head outputs only");
  DLE_CHECK_ARG(heads && geom, "ssd_decode_fwd: null map table");
  DLE_CHECK_ARG(nmaps >= 1 && nmaps <= DLE_SSD_MAX_MAPS, "ssd_decode_fwd: 1..%d feature maps (got %d)", DLE_SSD_MAX_MAPS, nmaps);
  DLE_CHECK_ARG(N >= 0 && L >= 2 && B >= 1, "ssd_decode_fwd: bad shape (N >= 0, B >= 1, L >= 2; got N %d, B %d, L %d)", N, B, L);
  SsdMaps maps;
  long long total = 0;
  for (int m = 0; m < DLE_SSD_MAX_MAPS; ++m) {
    maps.head[m] = nullptr;
    maps.fs[m] = maps.nd[m] = maps.pitch[m] = maps.loc[m] = maps.conf[m] = 0;
  }
  for (int m = 0; m < nmaps; ++m) {
    const int fs = geom[5 * m], nd = geom[5 * m + 1], pitch = geom[5 * m + 2], loc = geom[5 * m + 3], conf = geom[5 * m + 4];
    DLE_CHECK_ARG(fs >= 1 && fs <= 4096 && nd >= 1 && nd <= 4096 && pitch >= 1, "ssd_decode_fwd: map %d: bad fs / nd / pitch", m);
    DLE_CHECK_ARG(loc >= 0 && (long long)loc + 4ll * nd <= pitch && conf >= 0 && (long long)conf + (long long)L * nd <= pitch,
                  "ssd_decode_fwd: map %d: loc [%d, +4 nd) or conf [%d, +L nd) outside the pitch %d", m, loc, conf, pitch);
    DLE_CHECK_ARG((long long)(N > 0 ? N : 1) * fs * fs * pitch < (1ll << 31), "ssd_decode_fwd: map %d: head tensor too large", m);
    DLE_CHECK_ARG(N == 0 || heads[m], "ssd_decode_fwd: map %d: null head pointer", m);
    maps.head[m] = (const unsigned short*)heads[m];
    maps.fs[m] = fs, maps.nd[m] = nd, maps.pitch[m] = pitch, maps.loc[m] = loc, maps.conf[m] = conf;
    maps.start[m] = (int)total;
    total += (long long)nd * fs * fs;
    DLE_CHECK_ARG(total < (1ll << 24), "ssd_decode_fwd: too many boxes");
  }
  for (int m = nmaps; m <= DLE_SSD_MAX_MAPS; ++m) maps.start[m] = (int)total;
  maps.n = nmaps;
  DLE_CHECK_ARG(total == B, "ssd_decode_fwd: the maps hold %lld boxes, B = %d", total, B);
  DLE_CHECK_ARG((long long)N * B * L < (1ll << 31), "ssd_decode_fwd: probs too large (below 2^31 elements)");
  if (N == 0) return 0;
  DLE_CHECK_ARG(dboxes_xywh && boxes && probs, "ssd_decode_fwd: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)dboxes_xywh) | ((uintptr_t)boxes)) & 15), "ssd_decode_fwd: dboxes_xywh and boxes must be 16-byte aligned");
  const unsigned grid = (unsigned)(((long long)N * B + SSD_THREADS - 1) / SSD_THREADS);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL(ssd_decode_kernel<DLE_F16>, dim3(grid), dim3(SSD_THREADS), 0, stream, maps, dboxes_xywh, boxes, probs, N, B, L, scale_xy, scale_wh);
  else
    hipLaunchKernelGGL(ssd_decode_kernel<DLE_BF16>, dim3(grid), dim3(SSD_THREADS), 0, stream, maps, dboxes_xywh, boxes, probs, N, B, L, scale_xy, scale_wh);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------- shared device parts
// fp32 bits -> unsigned with the same order (and back)
__device__ __forceinline__ unsigned ssd_ordered(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ssd_unordered(unsigned o) {
  const unsigned u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __builtin_bit_cast(float, u);
}

// Appends the keys of the threads with pred, in thread order, behind keys[total] (every thread of the block calls it; wcnt: 2 x
// SSD_WAVES ints, alternated by `phase` so that one barrier per call is enough).  Returns the new total.
__device__ __forceinline__ int ssd_append(unsigned long long* keys, int* wcnt, int phase, int total, bool pred, unsigned long long key) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long m = __ballot(pred);
  int* wc = wcnt + (phase & 1) * SSD_WAVES;
  if (lane == 0) wc[wave] = __popcll(m);
  __syncthreads();
  int off = total, all = 0;
#pragma unroll
  for (int w = 0; w < SSD_WAVES; ++w) {
    const int c = wc[w];
    off += w < wave ? c : 0;
    all += c;
  }
  if (pred) keys[off + __popcll(m & ((1ull << lane) - 1ull))] = key;
  return total + all;
}

// keys[0, P) (P a power of two) in descending order; every thread of the block calls it; starts and ends with a barrier
__device__ __forceinline__ void ssd_sort_desc(unsigned long long* keys, int P) {
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += SSD_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const unsigned long long a = keys[i], b = keys[l];
        const bool desc = (i & k) == 0;
        if ((a < b) == desc) { keys[i] = b, keys[l] = a; }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int ssd_pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// calc_iou_tensor's fp32 operations in its order (utils.py:47-65); the division is correctly rounded
__device__ __forceinline__ float ssd_iou(float4_t p, float4_t q) {
  const float l = fmaxf(p[0], q[0]), t = fmaxf(p[1], q[1]), r = fminf(p[2], q[2]), b = fminf(p[3], q[3]);
  float dx = r - l, dy = b - t;
  dx = dx < 0.f ? 0.f : dx;
  dy = dy < 0.f ? 0.f : dy;
  const float inter = dx * dy;
  const float a1 = (p[2] - p[0]) * (p[3] - p[1]);
  const float a2 = (q[2] - q[0]) * (q[3] - q[1]);
  return __fdiv_rn(inter, (a1 + a2) - inter);
}

// --------------------------------------------------------------------------------------------------------------------- NMS
// dynamic LDS: keys [P] u64 | box [256] float4 | mask [256][4] u64 | sidx [256] int | kept [256] int | wcnt [8] int
__host__ __device__ inline size_t ssd_tail_bytes() { return 256 * 16 + 256 * 4 * 8 + 256 * 4 + 256 * 4 + 8 * 4; }

__global__ __launch_bounds__(SSD_THREADS) void ssd_nms_kernel(const float* __restrict__ boxes, const float* __restrict__ probs,
                                                              int* __restrict__ kept_idx, float* __restrict__ kept_score,
                                                              int* __restrict__ kept_count, int B, int L, int cap, float threshold,
                                                              float criteria, int max_num) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ssd_lds[];
  unsigned long long* keys = (unsigned long long*)ssd_lds;
  float4_t* box = (float4_t*)(keys + cap);
  unsigned long long* mask = (unsigned long long*)(box + 256);
  int* sidx = (int*)(mask + 256 * 4);
  int* kept = sidx + 256;
  int* wcnt = kept + 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = blockIdx.x / (L - 1), lab = blockIdx.x - n * (L - 1);          // label lab + 1
  const float* row = probs + ((long long)n * L + lab + 1) * B;
  // ---- candidates, in index order
  int total = 0, phase = 0;
  for (int base = 0; base < B; base += SSD_THREADS, ++phase) {
    const int i = base + tid;
    const float s = i < B ? row[i] : 0.f;
    const bool pred = i < B && s > threshold;
    total = ssd_append(keys, wcnt, phase, total, pred, ((unsigned long long)ssd_ordered(s) << 32) | (unsigned)~i);
  }
  const int P = ssd_pow2_at_least(total);
  for (int i = total + tid; i < P; i += SSD_THREADS) keys[i] = 0ull;
  ssd_sort_desc(keys, P);
  const int K = total < max_num ? total : max_num;
  // ---- the best K with their boxes
  if (tid < K) {
    const int idx = (int)~(unsigned)keys[tid];
    box[tid] = *(const float4_t*)(boxes + ((long long)n * B + idx) * 4);
    sidx[tid] = idx;
  }
  __syncthreads();
  // ---- suppression bits: word (i, wave) holds, for j = 64 wave + lane > i, whether kept candidate i removes candidate j
  {
    const float4_t mine = tid < K ? box[tid] : float4_t{0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < K; ++i) {
      if (wave * 64 + 63 <= i) {
        if (lane == 0) mask[i * 4 + wave] = 0ull;
        continue;
      }
      const bool sup = tid > i && tid < K && !(ssd_iou(mine, box[i]) < criteria);
      const unsigned long long m = __ballot(sup);
      if (lane == 0) mask[i * 4 + wave] = m;
    }
  }
  __syncthreads();
  // ---- the serial sweep, wavefront 0
  if (wave == 0) {
    unsigned long long removed[4] = {0ull, 0ull, 0ull, 0ull};
    int count = 0;
    for (int c = 0; c * 64 < K; ++c) {
      const int r = c * 64 + lane;
      unsigned lo[4], hi[4];
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const unsigned long long v = r < K ? mask[r * 4 + w] : 0ull;
        lo[w] = (unsigned)v, hi[w] = (unsigned)(v >> 32);
      }
      const int rows = K - c * 64 < 64 ? K - c * 64 : 64;
      for (int l = 0; l < rows; ++l) {
        const unsigned long long cur = c == 0 ? removed[0] : c == 1 ? removed[1] : c == 2 ? removed[2] : removed[3];
        if ((cur >> l) & 1ull) continue;
        if (lane == 0) kept[count] = c * 64 + l;
        ++count;
#pragma unroll
        for (int w = 0; w < 4; ++w)
          removed[w] |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)hi[w], l) << 32) |
                        (unsigned)__builtin_amdgcn_readlane((int)lo[w], l);
      }
    }
    if (lane == 0) wcnt[0] = count;
  }
  __syncthreads();
  const int count = wcnt[0];
  const long long o = ((long long)n * (L - 1) + lab) * max_num;
  if (tid == 0) kept_count[(long long)n * (L - 1) + lab] = count;
  if (tid < max_num) {
    int ki = -1;
    float ks = 0.f;
    if (tid < count) {
      const int pos = kept[tid];
      ki = sidx[pos];
      ks = row[ki];
    }
    kept_idx[o + tid] = ki;
    kept_score[o + tid] = ks;
  }
}

extern "C" int dle_ssd_nms_fwd(const float* boxes, const float* probs, int* kept_idx, float* kept_score, int* kept_count, int N,
                               int B, int L, float threshold, float criteria, int max_num, hipStream_t stream) {
  DLE_CHECK_ARG(max_num >= 1 && max_num <= DLE_SSD_MAX_KEEP, "ssd_nms_fwd: 1 <= max_num <= %d (got %d)", DLE_SSD_MAX_KEEP, max_num);
  DLE_CHECK_ARG(L >= 2 && L <= 65536, "ssd_nms_fwd: 2 <= L <= 65536 (got %d)", L);
  DLE_CHECK_ARG(N >= 0 && B >= 1 && B <= DLE_SSD_MAX_BOXES, "ssd_nms_fwd: N >= 0 and 1 <= B <= %d (got N %d, B %d)", DLE_SSD_MAX_BOXES, N, B);
  DLE_CHECK_ARG((long long)N * L * B < (1ll << 31) && (long long)N * (L - 1) * max_num < (1ll << 31) && (long long)N * (L - 1) < (1ll << 31),
                "ssd_nms_fwd: tensor too large (below 2^31 elements)");
  if (N == 0) return 0;
  DLE_CHECK_ARG(boxes && probs && kept_idx && kept_score && kept_count, "ssd_nms_fwd: null pointer");
  DLE_CHECK_ARG(!(((uintptr_t)boxes) & 15), "ssd_nms_fwd: boxes must be 16-byte aligned");
  int cap = 2;                                            // (16 bytes at least: what follows the keys is 16-byte aligned)
  while (cap < B) cap <<= 1;
  const size_t lds = (size_t)cap * 8 + ssd_tail_bytes();
  DLE_LAUNCH_LDS(ssd_nms_kernel, dim3((unsigned)(N * (L - 1))), dim3(SSD_THREADS), lds, stream, boxes, probs, kept_idx, kept_score,
                 kept_count, B, L, cap, threshold, criteria, max_num);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------------------------ select
__global__ __launch_bounds__(SSD_THREADS) void ssd_select_kernel(const float* __restrict__ boxes, const int* __restrict__ kept_idx,
                                                                 const float* __restrict__ kept_score, const int* __restrict__ kept_count,
                                                                 float* __restrict__ det_boxes, int* __restrict__ det_label,
                                                                 float* __restrict__ det_score, int* __restrict__ det_idx,
                                                                 int* __restrict__ det_count, int B, int L, int cap, int max_num,
                                                                 int max_output) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ssd_lds[];
  unsigned long long* keys = (unsigned long long*)ssd_lds;
  int* wcnt = (int*)(keys + cap);
  const int tid = threadIdx.x, n = blockIdx.x;
  const int per = max_num < max_output ? max_num : max_output;      // only the first max_output of a class can be selected
  const int slots = (L - 1) * per;
  const long long cls0 = (long long)n * (L - 1);
  int total = 0, phase = 0;
  for (int base = 0; base < slots; base += SSD_THREADS, ++phase) {
    const int s = base + tid;
    bool pred = false;
    unsigned long long key = 0ull;
    if (s < slots) {
      const int lab = s / per, pos = s - lab * per;
      int c = kept_count[cls0 + lab];
      c = c < 0 ? 0 : (c > max_num ? max_num : c);
      if (pos < c) {
        const long long at = (cls0 + lab) * max_num + pos;
        const unsigned idx = (unsigned)kept_idx[at] & 0xffffu;
        pred = true;
        key = ((unsigned long long)ssd_ordered(kept_score[at]) << 32) | (unsigned)~(((unsigned)lab << 16) | idx);
      }
    }
    total = ssd_append(keys, wcnt, phase, total, pred, key);
  }
  const int P = ssd_pow2_at_least(total);
  for (int i = total + tid; i < P; i += SSD_THREADS) keys[i] = 0ull;
  ssd_sort_desc(keys, P);
  const int count = total < max_output ? total : max_output;
  if (tid == 0) det_count[n] = count;
  if (tid < max_output) {
    float4_t bx = {0.f, 0.f, 0.f, 0.f};
    int label = 0, idx = 0;
    float score = 0.f;
    if (tid < count) {
      const unsigned long long key = keys[tid];
      const unsigned low = ~(unsigned)key;
      label = (int)(low >> 16) + 1;
      idx = (int)(low & 0xffffu);
      idx = idx < B ? idx : B - 1;
      score = ssd_unordered((unsigned)(key >> 32));
      bx = *(const float4_t*)(boxes + ((long long)n * B + idx) * 4);
    }
    const long long o = (long long)n * max_output + tid;
    *(float4_t*)(det_boxes + o * 4) = bx;
    det_label[o] = label;
    det_score[o] = score;
    det_idx[o] = idx;
  }
}

extern "C" int dle_ssd_select_fwd(const float* boxes, const int* kept_idx, const float* kept_score, const int* kept_count,
                                  float* det_boxes, int* det_label, float* det_score, int* det_idx, int* det_count, int N, int B, int L,
                                  int max_num, int max_output, hipStream_t stream) {
  DLE_CHECK_ARG(max_num >= 1 && max_num <= DLE_SSD_MAX_KEEP, "ssd_select_fwd: 1 <= max_num <= %d (got %d)", DLE_SSD_MAX_KEEP, max_num);
  DLE_CHECK_ARG(max_output >= 1 && max_output <= DLE_SSD_MAX_KEEP, "ssd_select_fwd: 1 <= max_output <= %d (got %d)", DLE_SSD_MAX_KEEP, max_output);
  DLE_CHECK_ARG(L >= 2 && L <= 65536, "ssd_select_fwd: 2 <= L <= 65536 (got %d)", L);
  DLE_CHECK_ARG(N >= 0 && B >= 1 && B <= DLE_SSD_MAX_BOXES, "ssd_select_fwd: N >= 0 and 1 <= B <= %d (got N %d, B %d)", DLE_SSD_MAX_BOXES, N, B);
  const long long slots = (long long)(L - 1) * (max_num < max_output ? max_num : max_output);
  DLE_CHECK_ARG(slots <= DLE_SSD_MAX_BOXES, "ssd_select_fwd: (L - 1) * min(max_num, max_output) = %lld candidates per image; the sort holds %d in LDS",
                slots, DLE_SSD_MAX_BOXES);
  DLE_CHECK_ARG((long long)N * (L - 1) * max_num < (1ll << 31) && (long long)N * B < (1ll << 29), "ssd_select_fwd: tensor too large");
  if (N == 0) return 0;
  DLE_CHECK_ARG(boxes && kept_idx && kept_score && kept_count && det_boxes && det_label && det_score && det_idx && det_count,
                "ssd_select_fwd: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)boxes) | ((uintptr_t)det_boxes)) & 15), "ssd_select_fwd: boxes and det_boxes must be 16-byte aligned");
  int cap = 2;                                            // (16 bytes at least: what follows the keys is 16-byte aligned)
  while (cap < slots) cap <<= 1;
  const size_t lds = (size_t)cap * 8 + 8 * 4;
  DLE_LAUNCH_LDS(ssd_select_kernel, dim3((unsigned)N), dim3(SSD_THREADS), lds, stream, boxes, kept_idx, kept_score, kept_count, det_boxes,
                 det_label, det_score, det_idx, det_count, B, L, cap, max_num, max_output);
  DLE_LAUNCH_CHECK();
  return 0;
}
