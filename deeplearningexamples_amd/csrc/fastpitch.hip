// FastPitch, inference (SpeechSynthesis/FastPitch/fastpitch/model.py:327-385 FastPitch.infer, transformer.py:39-78
// PositionwiseConvFF, common/layers.py:76-88 ConvReLUNorm) on PACKED utterances: activations are 16-bit, channels-last
// [total_rows, C]; sequence b owns rows cu[b] .. cu[b + 1] - 1 of a device int32 table cu[B + 1].  There are no padding rows and no
// masks: every kernel reads rows outside the row's own sequence as zero, so an utterance gets what it gets alone, whatever shares
// its batch.  Lengths are clamped to [0, max_len] and rows to `total` inside every kernel (as dle_attention_fwd_varlen does): a
// wrong table gives wrong answers but reaches no memory outside the operands.
//
// dle_conv1d_packed_fwd -- the hot path: the two k = 3 convolutions of every FFT block (384 -> 1536 -> 384) and the convolutions
// of the temporal predictors.  The staging and MFMA scheme is that of hfg_conv1d_kernel (csrc/hifigan.hip), dilation 1:
//  * one workgroup of 4 wavefronts per (sequence, time tile of TT = 64 rows, channel block of CB = 128 output channels); a tile
//    never spans two sequences, and a workgroup whose tile starts at or behind its sequence's (clamped) length exits before any
//    barrier.  The grid is B * ceil(max_len / TT) x ceil(Ko / CB);
//  * per 64-channel chunk of C the rows [t0 - halo, t0 + TT + halo) of a = relu-or-not(x) are staged in LDS ONCE (16-byte loads,
//    zeros outside [0, len) of the OWN sequence and beyond C; pitch 72 elements: the 16 rows of a ds_read_b128 lane group cover the
//    64 banks exactly once); the ksize taps read shifted windows of that one image as the B operand of v_mfma_f32_32x32x16
//    (lane = time step), so HBM sees every activation once per channel block;
//  * the weights are the A operand (lane = output channel), one 16-byte global load per lane, tap and 16-channel step, each
//    fragment used for the wavefront's 2 time sub-tiles of 32 rows.  With few rows the kernel is bound by the latency of its
//    loads, not by their volume (6 workgroups walk C = 1536 at 128 rows), so both operands are software-pipelined one chunk
//    ahead: while chunk i is multiplied, the activations of chunk i + 1 are in flight to registers (stored to LDS after the
//    barrier) and, for ksize <= 3, so are the weight fragments of all its taps;
//  * epilogue on the accumulators: acc + bias (+ add1), one rounding, 8-byte stores; add1 is read by the lane that writes the
//    same element afterwards, so y may be add1.
// Tile sizes.  TT = 64, CB = 128 (every wavefront a 32-channel slice, all four sharing the staged tile): FastPitch's rows are few
// -- a batch of texts is some hundreds of rows, one spectrogram at most 1024 -- while Ko is 384 or 1536, so the parallelism has
// to come from the channel blocks: 64 x 128 gives 3 (Ko = 384) or 12 (Ko = 1536) workgroups per 64 rows, and at C = 1536 the
// staged tile (74 rows x 144 B = 10.4 KiB) leaves room for several workgroups per CU.  A longer tile would halve the workgroup
// count of an 800-frame utterance below the CU count at Ko = 1536; a 32-row tile would read every weight twice as often, and
// the weights (1536 x 3 x 384 x 2 B = 3.4 MiB per convolution) are already the larger operand.  The second sub-tile of a ragged
// last tile with <= 32 live rows is skipped (wave-uniform).
//
// The other kernels are bound by launch latency, not by bandwidth (rows x a few hundred channels): they are written for exactness
// of their contract, one rounding per output, fp32 arithmetic in a fixed order without contraction where a test compares bits.
#include "conv1d_family.h"
#include <math.h>

// every product and sum below is rounded on its own (no fused multiply-add unless written as one): the row kernels promise bits
#pragma clang fp contract(off)

#define FP_CC 64           // channels per staged chunk
#define FP_PITCH 72        // LDS row pitch in elements
#define FP_MAX_HALO 5      // ksize <= 11
#define FP_TT 64           // rows per time tile
#define FP_CB 128          // output channels per workgroup
#define FP_MAX_LEN 1024    // the envelope of dle_attention_fwd_varlen
#define FP_RT 16           // rows per workgroup of the row kernels (embed, scalar_conv_add, expand)
#define FP_UT 64           // frames per workgroup of unpack_mel

struct FpConvArgs {
  const unsigned short* x;     // [total, C]
  const unsigned short* w;     // [Ko, ksize, C]
  const float* bias;           // [Ko]
  const unsigned short* add1;  // [total, Ko] or null
  unsigned short* y;           // [total, Ko]
  const int32_t* cu;           // [B + 1]
  long long total;
  int max_len, C, Ko, ksize, halo, ttiles;
  float slope;
};

// K3: ksize <= 3 (every convolution of FastPitch): the weight fragments of ALL taps of a chunk are held in registers and those of
// the next chunk are loaded while this one is multiplied.  Otherwise (ksize 5 .. 11) one tap is loaded ahead, as hfg_conv1d_kernel
// does.  Both walk taps, 16-channel steps and sub-tiles in the same order, so the accumulator sees the same sequence of MFMAs.
template <int DT, bool K3>
__global__ __launch_bounds__(256) void fp_conv1d_packed_kernel(FpConvArgs p) {
  constexpr int NT = FP_TT / 32, WT = K3 ? 3 : 1;
  __shared__ __attribute__((aligned(16))) unsigned short lds[(FP_TT + 2 * FP_MAX_HALO) * FP_PITCH];
  const int b = blockIdx.x / p.ttiles, t0 = (blockIdx.x - b * p.ttiles) * FP_TT;
  long long start;
  int len;
  c1d_seq(p.cu, b, p.total, start, len, p.max_len);
  if (t0 >= len) return;                                             // workgroup-uniform: before any barrier or LDS write
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int kob = blockIdx.y * FP_CB + wave * 32;
  const int ko = kob + fr;
  const bool wave_on = kob < p.Ko;                                    // wave-uniform; an idle wave still stages and meets the barriers
  const bool ko_ok = ko < p.Ko;
  const int nts = len - t0 > 32 ? NT : 1;                             // live 32-row sub-tiles (workgroup-uniform)
  const unsigned short* xs = p.x + start * p.C;
  const unsigned short* wk0 = p.w + (long long)(ko_ok ? ko : 0) * p.ksize * p.C;
  const int rows = FP_TT + 2 * p.halo;

  float16_t acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nt][i] = 0.f;

  auto load_tap = [&](int c0, int tap, ushort8_t* f) { c1d_load_tap(f, wk0, tap, p.C, c0, fh, ko_ok); };
  auto load_taps = [&](int c0, ushort8_t (*f)[4]) {
#pragma unroll
    for (int tap = 0; tap < WT; ++tap)
      if (tap < p.ksize) load_tap(c0, tap, f[tap]);
  };
  auto mfma_tap = [&](int tap, int nks, const ushort8_t* wf) {
    const unsigned short* win = lds + (fr + tap) * FP_PITCH + fh * 8;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (ks < nks) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          if (nt < nts) {
            const ushort8_t fa = *(const ushort8_t*)(win + nt * 32 * FP_PITCH + ks * 16);
            acc[nt] = Mfma32x16<DT>::run(wf[ks], fa, acc[nt]);
          }
        }
      }
    }
  };

  ushort8_t sv[3], wcur[WT][4], wnxt[WT][4];
  c1d_stage_load<DT>(sv, xs, len, p.C, t0 - p.halo, rows, 0, p.slope);
  if (K3 && wave_on) load_taps(0, wcur);
  for (int c0 = 0; c0 < p.C; c0 += FP_CC) {
    const int cw = p.C - c0 < FP_CC ? p.C - c0 : FP_CC;
    const int nks = (cw + 15) >> 4;
    const bool more = c0 + FP_CC < p.C;
    if (c0) __syncthreads();                                          // every wave is done with the previous chunk's tile
    c1d_stage_store<3, FP_PITCH>(lds, sv, rows);
    if (more) {                                                       // the next chunk's operands: in flight during this chunk's MFMAs
      c1d_stage_load<DT>(sv, xs, len, p.C, t0 - p.halo, rows, c0 + FP_CC, p.slope);
      if (K3 && wave_on) load_taps(c0 + FP_CC, wnxt);
    }
    __syncthreads();
    if (!wave_on) continue;
    if (K3) {
#pragma unroll
      for (int tap = 0; tap < WT; ++tap)
        if (tap < p.ksize) mfma_tap(tap, nks, wcur[tap]);
      if (more) {
#pragma unroll
        for (int tap = 0; tap < WT; ++tap)
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) wcur[tap][ks] = wnxt[tap][ks];
      }
    } else {
      ushort8_t nxt[4];
      load_tap(c0, 0, nxt);
      for (int tap = 0; tap < p.ksize; ++tap) {
        ushort8_t wf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) wf[ks] = nxt[ks];
        if (tap + 1 < p.ksize) load_tap(c0, tap + 1, nxt);
        mfma_tap(tap, nks, wf);
      }
    }
  }
  if (!wave_on) return;

  // D: lane owns row fr of the sub-tile, channels kob + 8 (i >> 2) + 4 fh + (i & 3)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int t = t0 + nt * 32 + fr;
    if (t >= len) continue;
    const long long row = (start + t) * p.Ko;
    c1d_epilogue_bias<DT>(acc[nt], p.bias, p.add1, nullptr, p.y, row, kob, fh, p.Ko, 1.f);
  }
}

// the (B, max_len, total) envelope every packed kernel shares with dle_attention_fwd_varlen
#define FP_CHECK_TABLE(name, B, max_len, total)                                                                            \
  DLE_CHECK_ARG(c1d_batch_ok(B, total, total) && (total) > 0, name ": bad batch / total rows");                            \
  DLE_CHECK_ARG((max_len) >= 1 && (max_len) <= FP_MAX_LEN, name ": 1 <= max_len <= 1024 (got %d)", (int)(max_len))

extern "C" int dle_conv1d_packed_fwd(const void* x, const void* w, const float* bias, const void* add1, void* y,
                                     const int32_t* cu_seqlens, int B, int max_len, int64_t total, int C, int Ko, int ksize,
                                     float slope, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "conv1d_packed_fwd: 16-bit activations and weights only");
  FP_CHECK_TABLE("conv1d_packed_fwd", B, max_len, total);
  DLE_CHECK_ARG(C >= 8 && C <= 2048 && C % 8 == 0, "conv1d_packed_fwd: C must be a multiple of 8 in [8, 2048] (got %d)", C);
  DLE_CHECK_ARG(Ko >= 8 && Ko <= 2048 && Ko % 8 == 0, "conv1d_packed_fwd: Ko must be a multiple of 8 in [8, 2048] (got %d)", Ko);
  DLE_CHECK_ARG(ksize >= 1 && ksize <= 11 && (ksize & 1), "conv1d_packed_fwd: ksize must be odd in [1, 11] (got %d)", ksize);
  DLE_CHECK_ARG(x && w && bias && y && cu_seqlens, "conv1d_packed_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(x, w, bias, add1, y) && dle_aligned<4>(cu_seqlens),
                "conv1d_packed_fwd: x, w, bias, add1 and y must be 16-byte aligned");
  const long long xbytes = (long long)total * C * 2, ybytes = (long long)total * Ko * 2;
  DLE_CHECK_ARG(c1d_under_4gib(xbytes, ybytes), "conv1d_packed_fwd: each tensor must be smaller than 4 GiB");
  DLE_CHECK_ARG(!c1d_overlap(x, xbytes, y, ybytes), "conv1d_packed_fwd: y must not overlap x");
  DLE_CHECK_ARG(c1d_addend_ok(add1, y, ybytes), "conv1d_packed_fwd: y overlaps add1 without being it");
  FpConvArgs p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.bias = bias; p.add1 = (const unsigned short*)add1;
  p.y = (unsigned short*)y; p.cu = cu_seqlens; p.total = total; p.max_len = max_len; p.C = C; p.Ko = Ko; p.ksize = ksize;
  p.halo = (ksize - 1) / 2; p.ttiles = (max_len + FP_TT - 1) / FP_TT; p.slope = slope;
  const long long gx = (long long)B * p.ttiles;
  DLE_CHECK_ARG(gx <= 0x7FFFFFFFLL, "conv1d_packed_fwd: too many time tiles");
  const dim3 grid((unsigned)gx, (unsigned)((Ko + FP_CB - 1) / FP_CB)), block(256);
#define FP_GO(DT)                                                                                      \
  do {                                                                                                \
    if (ksize <= 3) hipLaunchKernelGGL((fp_conv1d_packed_kernel<DT, true>), grid, block, 0, stream, p); \
    else hipLaunchKernelGGL((fp_conv1d_packed_kernel<DT, false>), grid, block, 0, stream, p);          \
  } while (0)
  if (dtype == DLE_F16) FP_GO(DLE_F16); else FP_GO(DLE_BF16);
#undef FP_GO
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- relu + LayerNorm (+ the predictor's fc) -----------------------------------------------------------------------------------
// one wavefront per row, H <= 1024: at most 2 chunks of 8 channels per lane
#define FP_LN_CH 2
#define FP_LN_MAX_PRED 4
#define FP_LN_GRID_CAP 512

template <int DT>
__global__ __launch_bounds__(256) void fp_relu_ln_kernel(const unsigned short* x, unsigned short* y, const float* gamma,
                                                         const float* beta, const float* fc_w, const float* fc_b, float* pred,
                                                         long long rows, int H, int n_pred, float eps) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
  const int nch = H >> 3;
  for (long long r = wave; r < rows; r += nwaves) {
    float v[FP_LN_CH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < FP_LN_CH; ++i) {
      const int c = lane + i * 64;
      if (c < nch) {
        float xf[8];
        unpack8<DT>(*(const ushort8_t*)(x + r * H + c * 8), xf);
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[i][k] = xf[k] > 0.f ? xf[k] : 0.f; s += v[i][k]; }
      }
    }
    s = wave_sum(s);
    const float mu = s / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < FP_LN_CH; ++i)
      if (lane + i * 64 < nch)
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float d = v[i][k] - mu; q += d * d; }
    q = wave_sum(q);
    const float rs = rsqrtf(q / (float)H + eps);
    float dot[FP_LN_MAX_PRED] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < FP_LN_CH; ++i) {
      const int c = lane + i * 64;
      if (c < nch) {
        float of[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) of[k] = (v[i][k] - mu) * rs * gamma[c * 8 + k] + beta[c * 8 + k];
        const ushort8_t o = pack8<DT>(of);
        if (y) *(ushort8_t*)(y + r * H + c * 8) = o;
        if (n_pred) {
          unpack8<DT>(o, of);                                            // the fc reads the ROUNDED y, as the next layer would
#pragma unroll
          for (int j = 0; j < FP_LN_MAX_PRED; ++j)
            if (j < n_pred)
#pragma unroll
              for (int k = 0; k < 8; ++k) dot[j] = __builtin_fmaf(fc_w[(long long)j * H + c * 8 + k], of[k], dot[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < FP_LN_MAX_PRED; ++j) {
      if (j < n_pred) {
        const float d = wave_sum(dot[j]);
        if (lane == 0) pred[r * n_pred + j] = d + fc_b[j];
      }
    }
  }
}

extern "C" int dle_fp_relu_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, const float* fc_w,
                                         const float* fc_b, float* pred, int64_t rows, int H, int n_pred, float eps, int dtype,
                                         hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "fp_relu_layernorm_fwd: 16-bit activations only");
  DLE_CHECK_ARG(H >= 8 && H % 8 == 0 && H <= 64 * FP_LN_CH * 8, "fp_relu_layernorm_fwd: H must be a multiple of 8, <= 1024 (got %d)", H);
  DLE_CHECK_ARG(n_pred >= 0 && n_pred <= FP_LN_MAX_PRED, "fp_relu_layernorm_fwd: n_pred in [0, 4] (got %d)", n_pred);
  DLE_CHECK_ARG(rows >= 0 && rows < (1LL << 31), "fp_relu_layernorm_fwd: bad row count");
  DLE_CHECK_ARG(y || n_pred, "fp_relu_layernorm_fwd: neither y nor pred is wanted");
  if (rows == 0) return 0;
  DLE_CHECK_ARG(x && gamma && beta && (!n_pred || (fc_w && fc_b && pred)), "fp_relu_layernorm_fwd: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)x) | ((uintptr_t)y)) & 15) &&
                    !((((uintptr_t)gamma) | ((uintptr_t)beta) | ((uintptr_t)fc_w) | ((uintptr_t)fc_b) | ((uintptr_t)pred)) & 3),
                "fp_relu_layernorm_fwd: x and y must be 16-byte aligned");
  long long g = (rows + 3) / 4;
  if (g > FP_LN_GRID_CAP) g = FP_LN_GRID_CAP;
  const dim3 grid((unsigned)g), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((fp_relu_ln_kernel<DLE_F16>), grid, block, 0, stream, (const unsigned short*)x, (unsigned short*)y, gamma, beta,
                       fc_w, fc_b, pred, (long long)rows, H, n_pred, eps);
  else
    hipLaunchKernelGGL((fp_relu_ln_kernel<DLE_BF16>), grid, block, 0, stream, (const unsigned short*)x, (unsigned short*)y, gamma, beta,
                       fc_w, fc_b, pred, (long long)rows, H, n_pred, eps);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- embedding: word[ids] + pos[p] (+ spk) -------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void fp_embed_kernel(const int64_t* ids, const float* word, const float* pos, const float* spk,
                                                       unsigned short* y, const int32_t* cu, long long total, int max_len,
                                                       int n_symbols, int D, int rtiles) {
  const int b = blockIdx.x / rtiles, p0 = (blockIdx.x - b * rtiles) * FP_RT;
  long long start;
  int len;
  c1d_seq(cu, b, total, start, len, max_len);
  const int n = (len - p0 < FP_RT ? len - p0 : FP_RT) * D;              // <= 0: nothing to do
  for (int i = threadIdx.x; i < n; i += 256) {
    const int pr = p0 + i / D, c = i - (i / D) * D;
    const long long r = start + pr;
    long long id = ids[r];
    id = id < 0 ? 0 : (id >= n_symbols ? n_symbols - 1 : id);
    float v = word[id * D + c] + pos[(long long)pr * D + c];
    if (spk) v = v + spk[c];
    y[r * D + c] = Elem<DT>::from_f32(v);
  }
}

extern "C" int dle_fp_embed(const int64_t* ids, const float* word, const float* pos, const float* spk, void* y,
                            const int32_t* cu_seqlens, int B, int max_len, int64_t total, int n_symbols, int n_pos, int D, int dtype,
                            hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "fp_embed: 16-bit output only");
  FP_CHECK_TABLE("fp_embed", B, max_len, total);
  DLE_CHECK_ARG(D >= 1 && D <= 4096 && n_symbols >= 1, "fp_embed: bad table shape (D = %d, n_symbols = %d)", D, n_symbols);
  DLE_CHECK_ARG(n_pos >= max_len, "fp_embed: the positional table has %d rows, max_len is %d", n_pos, max_len);
  DLE_CHECK_ARG(ids && word && pos && y && cu_seqlens, "fp_embed: null pointer");
  DLE_CHECK_ARG((long long)total * D * 2 < 0xFFFFFFF0LL, "fp_embed: y must be smaller than 4 GiB");
  const int rtiles = (max_len + FP_RT - 1) / FP_RT;
  const dim3 grid((unsigned)((long long)B * rtiles)), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((fp_embed_kernel<DLE_F16>), grid, block, 0, stream, ids, word, pos, spk, (unsigned short*)y, cu_seqlens,
                       (long long)total, max_len, n_symbols, D, rtiles);
  else
    hipLaunchKernelGGL((fp_embed_kernel<DLE_BF16>), grid, block, 0, stream, ids, word, pos, spk, (unsigned short*)y, cu_seqlens,
                       (long long)total, max_len, n_symbols, D, rtiles);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- pitch_emb / energy_emb: Conv1d(1 -> D, k) of a per-token series, added in place -------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void fp_scalar_conv_add_kernel(unsigned short* enc, const float* v, const float* w, const float* bias,
                                                                 const int32_t* cu, long long total, int max_len, int D, int ksize,
                                                                 int rtiles) {
  const int b = blockIdx.x / rtiles, p0 = (blockIdx.x - b * rtiles) * FP_RT;
  long long start;
  int len;
  c1d_seq(cu, b, total, start, len, max_len);
  const int n = (len - p0 < FP_RT ? len - p0 : FP_RT) * D;
  const int halo = (ksize - 1) / 2;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int pr = p0 + i / D, c = i - (i / D) * D;
    float s = bias[c];
    for (int k = 0; k < ksize; ++k) {
      const int q = pr + k - halo;
      const float vv = (q >= 0 && q < len) ? v[start + q] : 0.f;
      s = s + w[c * ksize + k] * vv;                                  // (two roundings: contraction is off in this file)
    }
    const long long o = (start + pr) * D + c;
    enc[o] = Elem<DT>::from_f32(Elem<DT>::to_f32(enc[o]) + s);
  }
}

extern "C" int dle_fp_scalar_conv_add(void* enc, const float* v, const float* w, const float* bias, const int32_t* cu_seqlens, int B,
                                      int max_len, int64_t total, int D, int ksize, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "fp_scalar_conv_add: 16-bit activations only");
  FP_CHECK_TABLE("fp_scalar_conv_add", B, max_len, total);
  DLE_CHECK_ARG(D >= 1 && D <= 4096, "fp_scalar_conv_add: D in [1, 4096] (got %d)", D);
  DLE_CHECK_ARG(ksize >= 1 && ksize <= 11 && (ksize & 1), "fp_scalar_conv_add: ksize must be odd in [1, 11] (got %d)", ksize);
  DLE_CHECK_ARG(enc && v && w && bias && cu_seqlens, "fp_scalar_conv_add: null pointer");
  DLE_CHECK_ARG((long long)total * D * 2 < 0xFFFFFFF0LL, "fp_scalar_conv_add: enc must be smaller than 4 GiB");
  const int rtiles = (max_len + FP_RT - 1) / FP_RT;
  const dim3 grid((unsigned)((long long)B * rtiles)), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((fp_scalar_conv_add_kernel<DLE_F16>), grid, block, 0, stream, (unsigned short*)enc, v, w, bias, cu_seqlens,
                       (long long)total, max_len, D, ksize, rtiles);
  else
    hipLaunchKernelGGL((fp_scalar_conv_add_kernel<DLE_BF16>), grid, block, 0, stream, (unsigned short*)enc, v, w, bias, cu_seqlens,
                       (long long)total, max_len, D, ksize, rtiles);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- durations -> repetitions, per-sequence exclusive cumsum, output table (one workgroup: B * L is tiny) ----------------------
__global__ __launch_bounds__(256) void fp_durations_kernel(const float* src, int from_log, float* dur_pred, int32_t* reps,
                                                           int32_t* tok_start, int32_t* cu_out, const int32_t* cu_in, int B,
                                                           int max_len, long long total, float pace, float max_duration,
                                                           int max_out) {
  for (int b = threadIdx.x; b < B; b += 256) {
    long long start;
    int len;
    c1d_seq(cu_in, b, total, start, len, max_len);
    long long run = 0;
    for (int i = 0; i < len; ++i) {
      float d = src[start + i];
      if (from_log) {
        d = expf(d) - 1.f;
        d = d < 0.f ? 0.f : (d > max_duration ? max_duration : d);      // (NaN passes, as torch.clamp lets it)
        if (dur_pred) dur_pred[start + i] = d;
      }
      const float f = __fdiv_rn(d, pace) + 0.5f;                          // IEEE division, as torch divides on the host
      int rp = (f >= 0.f && f < 1.0e6f) ? (int)f : 0;                  // the cast truncates; NaN, negative and absurd values give 0
      if (run + rp > max_out) rp = (int)(max_out - run);              // a sequence never grows beyond max_out rows
      reps[start + i] = rp;
      tok_start[start + i] = (int)run;
      run += rp;
    }
    cu_out[b + 1] = (int)run;                                          // lengths first; the prefix sum follows
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long acc = 0;
    cu_out[0] = 0;
    for (int b = 0; b < B; ++b) {
      acc += cu_out[b + 1];
      cu_out[b + 1] = (int)(acc > 0x7FFFFFFFLL ? 0x7FFFFFFFLL : acc);
    }
  }
}

extern "C" int dle_fp_durations(const float* src, int from_log, float* dur_pred, int32_t* reps, int32_t* tok_start, int32_t* cu_out,
                                const int32_t* cu_in, int B, int max_len, int64_t total, float pace, float max_duration, int max_out,
                                hipStream_t stream) {
  FP_CHECK_TABLE("fp_durations", B, max_len, total);
  DLE_CHECK_ARG(B <= 65536, "fp_durations: at most 65536 sequences (got %d)", B);
  DLE_CHECK_ARG(pace > 0.f && max_duration >= 0.f && max_out >= 1, "fp_durations: pace > 0, max_duration >= 0, max_out >= 1");
  DLE_CHECK_ARG(src && reps && tok_start && cu_out && cu_in, "fp_durations: null pointer");
  hipLaunchKernelGGL(fp_durations_kernel, dim3(1), dim3(256), 0, stream, src, from_log, dur_pred, reps, tok_start, cu_out, cu_in, B,
                     max_len, (long long)total, pace, max_duration, max_out);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- the length regulator + the decoder's positional embedding ------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void fp_expand_kernel(const unsigned short* enc, const float* pos, const int32_t* reps,
                                                        const int32_t* tok_start, const int32_t* cu_in, const int32_t* cu_out,
                                                        unsigned short* y, int max_in, long long total_in, int max_out,
                                                        long long total_out, int D, int rtiles) {
  const int b = blockIdx.x / rtiles, p0 = (blockIdx.x - b * rtiles) * FP_RT;
  long long in0, out0;
  int in_len, out_len;
  c1d_seq(cu_in, b, total_in, in0, in_len, max_in);
  c1d_seq(cu_out, b, total_out, out0, out_len, max_out);
  if (p0 >= out_len) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int pr = p0 + wave; pr < p0 + FP_RT && pr < out_len; pr += 4) {
    // the last token whose first frame is at or before pr (tok_start is non-decreasing inside a sequence; tokens without
    // repetitions share their successor's start, so the last of a run of equal starts is the one that has frames)
    int lo = 0, hi = in_len;                                            // invariant: tok_start[lo'] <= pr for lo' < lo ... search on [lo, hi)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (tok_start[in0 + mid] <= pr) lo = mid + 1; else hi = mid;
    }
    const int j = lo - 1;
    bool ok = j >= 0;
    if (ok) {
      const int ts = tok_start[in0 + j];
      ok = pr - ts < reps[in0 + j];                                      // (a table that does not cover pr: the row gets pos alone)
    }
    const unsigned short* src = enc + (in0 + (ok ? j : 0)) * D;
    unsigned short* dst = y + (out0 + pr) * D;
    for (int c = lane; c < D; c += 64) {
      const float e = ok ? Elem<DT>::to_f32(src[c]) : 0.f;
      dst[c] = Elem<DT>::from_f32(e + pos[(long long)pr * D + c]);
    }
  }
}

extern "C" int dle_fp_expand(const void* enc, const float* pos, const int32_t* reps, const int32_t* tok_start, const int32_t* cu_in,
                             const int32_t* cu_out, void* y, int B, int max_in, int64_t total_in, int max_out, int64_t total_out,
                             int n_pos, int D, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "fp_expand: 16-bit activations only");
  FP_CHECK_TABLE("fp_expand", B, max_in, total_in);
  FP_CHECK_TABLE("fp_expand", B, max_out, total_out);
  DLE_CHECK_ARG(D >= 1 && D <= 4096, "fp_expand: D in [1, 4096] (got %d)", D);
  DLE_CHECK_ARG(n_pos >= max_out, "fp_expand: the positional table has %d rows, max_out is %d", n_pos, max_out);
  DLE_CHECK_ARG(enc && pos && reps && tok_start && cu_in && cu_out && y, "fp_expand: null pointer");
  DLE_CHECK_ARG((long long)total_in * D * 2 < 0xFFFFFFF0LL && (long long)total_out * D * 2 < 0xFFFFFFF0LL,
                "fp_expand: each tensor must be smaller than 4 GiB");
  const int rtiles = (max_out + FP_RT - 1) / FP_RT;
  const dim3 grid((unsigned)((long long)B * rtiles)), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((fp_expand_kernel<DLE_F16>), grid, block, 0, stream, (const unsigned short*)enc, pos, reps, tok_start, cu_in,
                       cu_out, (unsigned short*)y, max_in, (long long)total_in, max_out, (long long)total_out, D, rtiles);
  else
    hipLaunchKernelGGL((fp_expand_kernel<DLE_BF16>), grid, block, 0, stream, (const unsigned short*)enc, pos, reps, tok_start, cu_in,
                       cu_out, (unsigned short*)y, max_in, (long long)total_in, max_out, (long long)total_out, D, rtiles);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- packed [total_out, n_mel] 16-bit -> fp32 [B, n_mel, T_pad], padding frames = bias -----------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void fp_unpack_mel_kernel(const unsigned short* x, const float* bias, float* mel, const int32_t* cu,
                                                            long long total, int n_mel, int t_pad, int ttiles) {
  const int b = blockIdx.x / ttiles, t0 = (blockIdx.x - b * ttiles) * FP_UT;
  long long start;
  int len;
  c1d_seq(cu, b, total, start, len, t_pad);
  const int n = n_mel * FP_UT;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int m = i / FP_UT, t = t0 + (i - m * FP_UT);
    if (t >= t_pad) continue;
    mel[((long long)b * n_mel + m) * t_pad + t] = t < len ? Elem<DT>::to_f32(x[(start + t) * n_mel + m]) : bias[m];
  }
}

extern "C" int dle_fp_unpack_mel(const void* x, const float* bias, float* mel, const int32_t* cu_seqlens, int B, int64_t total, int n_mel,
                                 int t_pad, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "fp_unpack_mel: 16-bit input only");
  FP_CHECK_TABLE("fp_unpack_mel", B, t_pad, total);
  DLE_CHECK_ARG(n_mel >= 1 && n_mel <= 1024, "fp_unpack_mel: n_mel in [1, 1024] (got %d)", n_mel);
  DLE_CHECK_ARG(x && bias && mel && cu_seqlens, "fp_unpack_mel: null pointer");
  const int ttiles = (t_pad + FP_UT - 1) / FP_UT;
  const dim3 grid((unsigned)((long long)B * ttiles)), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((fp_unpack_mel_kernel<DLE_F16>), grid, block, 0, stream, (const unsigned short*)x, bias, mel, cu_seqlens,
                       (long long)total, n_mel, t_pad, ttiles);
  else
    hipLaunchKernelGGL((fp_unpack_mel_kernel<DLE_BF16>), grid, block, 0, stream, (const unsigned short*)x, bias, mel, cu_seqlens,
                       (long long)total, n_mel, t_pad, ttiles);
  DLE_LAUNCH_CHECK();
  return 0;
}
