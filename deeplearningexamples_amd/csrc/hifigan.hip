// HiFi-GAN generator, inference (SpeechSynthesis/HiFiGAN/hifigan/models.py:75-137 ResBlock1/2, 140-232 Generator): the dilated
// "same" Conv1d with everything that surrounds it in the network fused in, and the Ko = 1 output convolution with its tanh.
//
// dle_conv1d_lrelu_fwd.  Replaces  xt = F.leaky_relu(x, slope); xt = conv(xt); x = xt + x  (models.py:98-105, 128-133), the running
// `xs += resblock(x)` / `xs / num_kernels` of Generator.forward (models.py:211-217) and, on a packed weight
// (functional.pack_upsample_weight), the ConvTranspose1d of `ups` -- each as ONE launch:
//
//  * a workgroup of 4 wavefronts owns TT time steps of one image for a block of 32 WK output channels.  Per 64-channel chunk of
//    C it stages the rows [t0 - halo, t0 + TT + halo) of `a` = leaky_relu(x) in LDS ONCE (16-byte loads, the fp32 product and its
//    rounding applied there, zeros outside [0, T) and beyond C); all ksize taps then read shifted windows of that one image: the
//    window is the B operand of v_mfma_f32_32x32x16 (lane = time step, 8 channels), so HBM sees every activation once per
//    channel block instead of the ksize copies of a column matrix.  Rows are pitched 72 elements (144 B): the 16 rows of one
//    ds_read_b128 lane group start 36 dwords apart and cover the 64 banks exactly once;
//  * the weights are the A operand (lane = output channel), read from global memory as they are: one 16-byte load per lane,
//    tap and 16-channel step, the next tap's fragments in flight while this tap's MFMAs run, each fragment used for NT = 2
//    time sub-tiles.  WK = 1, 2, 4 wavefronts across the channels for Ko <= 32, <= 64, more: the narrow late stages give every
//    wavefront its own stretch of time (TT = 256) and the wide early ones share a short staged tile (TT = 64);
//  * epilogue on the accumulator registers: lane = time step, 4 runs of 4 consecutive channels:
//    (acc + bias (+ add1) (+ add2)) * alpha, one rounding, 8-byte stores.  An addend is read by the lane that writes the same
//    element afterwards, so y may be one of the addends.
//
// dle_hfg_post_fwd.  conv_post + tanh (models.py:218-221): one output channel, so a dot product per time step, bound by its one
// read of x: 256 time steps and their halo staged in LDS as above, the weights as fp32 in LDS (broadcast reads), one thread per
// sample, sequential fp32 fma, tanhf.
#include "conv1d_family.h"

#define HFG_CC 64          // channels per staged chunk
#define HFG_PITCH 72       // LDS row pitch in elements
#define HFG_MAX_HALO 36

struct HfgArgs {
  const unsigned short* x;     // [B, T, C]
  const unsigned short* w;     // [Ko, ksize, C]
  const float* bias;           // [Ko]
  const unsigned short* add1;  // [B, T, Ko] or null
  const unsigned short* add2;
  unsigned short* y;           // [B, T, Ko]
  int T, C, Ko, ksize, dil, halo, ttiles;
  float slope, alpha;
};

// rows [t0 - halo, t0 - halo + rows) x channels [c0, c0 + 8 npr) of image b -> lds[row][8 piece]; 256 threads
template <int DT>
__device__ __forceinline__ void hfg_stage(unsigned short* lds, const unsigned short* xb, int T, int C, int t0, int halo, int rows,
                                          int c0, int npr, float slope) {
  const int cc = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  if (cc >= npr) return;
  const int c = c0 + cc * 8;
  for (int r = r0; r < rows; r += 32) {
    const int t = t0 - halo + r;
    ushort8_t v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (t >= 0 && t < T && c < C) {
      v = *(const ushort8_t*)(xb + (long long)t * C + c);
      if (slope != 1.f) v = c1d_act8<DT>(v, slope);
    }
    *(ushort8_t*)(lds + r * HFG_PITCH + cc * 8) = v;
  }
}

template <int DT, int WK>
__global__ __launch_bounds__(256) void hfg_conv1d_kernel(HfgArgs p) {
  constexpr int NT = 2, WT = 4 / WK, TT = WT * NT * 32;
  __shared__ __attribute__((aligned(16))) unsigned short lds[(TT + 2 * HFG_MAX_HALO) * HFG_PITCH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int wk = wave % WK, wt = wave / WK;
  const int b = blockIdx.x / p.ttiles, t0 = (blockIdx.x - b * p.ttiles) * TT;
  const int kob = (blockIdx.y * WK + wk) * 32;
  const int ko = kob + fr;
  const bool wave_on = kob < p.Ko && t0 + wt * NT * 32 < p.T;          // wave-uniform; an idle wave still stages and meets the barriers
  const bool ko_ok = ko < p.Ko;
  const unsigned short* xb = p.x + (long long)b * p.T * p.C;
  const unsigned short* wk0 = p.w + (long long)(ko_ok ? ko : 0) * p.ksize * p.C;   // row of ko; the channel offset is added per load
  const int rows = TT + 2 * p.halo;

  float16_t acc[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[nt][i] = 0.f;

  for (int c0 = 0; c0 < p.C; c0 += HFG_CC) {
    const int cw = p.C - c0 < HFG_CC ? p.C - c0 : HFG_CC;
    const int nks = (cw + 15) >> 4;
    if (c0) __syncthreads();
    hfg_stage<DT>(lds, xb, p.T, p.C, t0, p.halo, rows, c0, nks * 2, p.slope);
    __syncthreads();
    if (!wave_on) continue;
    auto load_tap = [&](int tap, ushort8_t* f) { c1d_load_tap(f, wk0, tap, p.C, c0, fh, ko_ok); };   // the next tap's A fragments
    ushort8_t nxt[4];
    load_tap(0, nxt);
    for (int tap = 0; tap < p.ksize; ++tap) {
      ushort8_t wf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) wf[ks] = nxt[ks];
      if (tap + 1 < p.ksize) load_tap(tap + 1, nxt);
      const unsigned short* win = lds + (wt * NT * 32 + fr + tap * p.dil) * HFG_PITCH + fh * 8;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        if (ks < nks) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const ushort8_t fa = *(const ushort8_t*)(win + nt * 32 * HFG_PITCH + ks * 16);
            acc[nt] = Mfma32x16<DT>::run(wf[ks], fa, acc[nt]);
          }
        }
      }
    }
  }
  if (!wave_on) return;

  // D: lane owns time step fr of the sub-tile, channels kob + 8 (i >> 2) + 4 fh + (i & 3)
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int t = t0 + (wt * NT + nt) * 32 + fr;
    if (t >= p.T) continue;
    const long long row = ((long long)b * p.T + t) * p.Ko;
    c1d_epilogue_bias<DT>(acc[nt], p.bias, p.add1, p.add2, p.y, row, kob, fh, p.Ko, p.alpha);
  }
}

extern "C" int dle_conv1d_lrelu_fwd(const void* x, const void* w, const float* bias, const void* add1, const void* add2, void* y,
                                    int B, int T, int C, int Ko, int ksize, int dilation, float slope, float alpha, int dtype,
                                    hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "conv1d_lrelu_fwd: 16-bit activations and weights only");
  DLE_CHECK_ARG(B >= 0 && T >= 1, "conv1d_lrelu_fwd: bad shape (B = %d, T = %d)", B, T);
  DLE_CHECK_ARG(C >= 8 && C <= 2048 && C % 8 == 0, "conv1d_lrelu_fwd: C must be a multiple of 8 in [8, 2048] (got %d)", C);
  DLE_CHECK_ARG(Ko >= 8 && Ko <= 2048 && Ko % 8 == 0, "conv1d_lrelu_fwd: Ko must be a multiple of 8 in [8, 2048] (got %d)", Ko);
  DLE_CHECK_ARG(ksize >= 1 && ksize <= 11 && (ksize & 1), "conv1d_lrelu_fwd: ksize must be odd in [1, 11] (got %d)", ksize);
  DLE_CHECK_ARG(dilation >= 1 && (long long)(ksize - 1) / 2 * dilation <= HFG_MAX_HALO,
                "conv1d_lrelu_fwd: dilation >= 1 with (ksize - 1) / 2 * dilation <= %d (got ksize %d, dilation %d)", HFG_MAX_HALO,
                ksize, dilation);
  if (B == 0) return 0;
  DLE_CHECK_ARG(x && w && bias && y, "conv1d_lrelu_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(x, w, bias, add1, add2, y),
                "conv1d_lrelu_fwd: every operand must be 16-byte aligned");
  const long long xbytes = (long long)B * T * C * 2, ybytes = (long long)B * T * Ko * 2;
  DLE_CHECK_ARG(c1d_under_4gib(xbytes, ybytes), "conv1d_lrelu_fwd: each tensor must be smaller than 4 GiB");
  DLE_CHECK_ARG(!c1d_overlap(x, xbytes, y, ybytes), "conv1d_lrelu_fwd: y must not overlap x");
  DLE_CHECK_ARG(c1d_addend_ok(add1, y, ybytes), "conv1d_lrelu_fwd: y overlaps add1 without being it");
  DLE_CHECK_ARG(c1d_addend_ok(add2, y, ybytes), "conv1d_lrelu_fwd: y overlaps add2 without being it");
  const int WK = Ko <= 32 ? 1 : Ko <= 64 ? 2 : 4;
  const int TT = (4 / WK) * 64;
  HfgArgs p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.bias = bias;
  p.add1 = (const unsigned short*)add1; p.add2 = (const unsigned short*)add2; p.y = (unsigned short*)y;
  p.T = T; p.C = C; p.Ko = Ko; p.ksize = ksize; p.dil = dilation; p.halo = (ksize - 1) / 2 * dilation;
  p.ttiles = (T + TT - 1) / TT;
  p.slope = slope; p.alpha = alpha;
  const long long gx = (long long)B * p.ttiles;
  DLE_CHECK_ARG(gx <= 0x7FFFFFFFLL, "conv1d_lrelu_fwd: too many time tiles");
  const dim3 grid((unsigned)gx, (unsigned)((Ko + 32 * WK - 1) / (32 * WK))), block(256);
#define HFG_GO(DT, WKV) hipLaunchKernelGGL((hfg_conv1d_kernel<DT, WKV>), grid, block, 0, stream, p)
#define HFG_PICK(DT) do { if (WK == 1) HFG_GO(DT, 1); else if (WK == 2) HFG_GO(DT, 2); else HFG_GO(DT, 4); } while (0)
  if (dtype == DLE_F16) HFG_PICK(DLE_F16); else HFG_PICK(DLE_BF16);
#undef HFG_GO
#undef HFG_PICK
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- conv_post + tanh ------------------------------------------------------------------------------------------------------
#define HFG_POST_TT 256
#define HFG_POST_MAXK 11

template <int DT>
__global__ __launch_bounds__(256) void hfg_post_kernel(const unsigned short* x, const unsigned short* w, const float* bias,
                                                       float* audio, int T, int C, int ksize, int ttiles, float slope) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[(HFG_POST_TT + HFG_POST_MAXK - 1) * HFG_PITCH];
  __shared__ __attribute__((aligned(16))) float wl[HFG_POST_MAXK * HFG_CC];
  const int b = blockIdx.x / ttiles, t0 = (blockIdx.x - b * ttiles) * HFG_POST_TT;
  const int halo = (ksize - 1) / 2;
  hfg_stage<DT>(lds, x + (long long)b * T * C, T, C, t0, halo, HFG_POST_TT + 2 * halo, 0, C >> 3, slope);
  for (int i = threadIdx.x; i < ksize * C; i += 256) wl[i] = Elem<DT>::to_f32(w[i]);
  __syncthreads();
  const int t = t0 + threadIdx.x;
  if (t >= T) return;
  float acc = bias[0];
  for (int k = 0; k < ksize; ++k) {
    const unsigned short* row = lds + (threadIdx.x + k) * HFG_PITCH;
    const float* wr = wl + k * C;
    for (int c = 0; c < C; c += 8) {
      float v[8];
      unpack8<DT>(*(const ushort8_t*)(row + c), v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(wr[c + e], v[e], acc);
    }
  }
  audio[(long long)b * T + t] = tanhf(acc);
}

extern "C" int dle_hfg_post_fwd(const void* x, const void* w, const float* bias, float* audio, int B, int T, int C, int ksize,
                                float slope, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "hfg_post_fwd: 16-bit activations and weights only");
  DLE_CHECK_ARG(B >= 0 && T >= 1, "hfg_post_fwd: bad shape (B = %d, T = %d)", B, T);
  DLE_CHECK_ARG(C >= 8 && C <= HFG_CC && C % 8 == 0, "hfg_post_fwd: C must be a multiple of 8 in [8, 64] (got %d)", C);
  DLE_CHECK_ARG(ksize >= 1 && ksize <= HFG_POST_MAXK && (ksize & 1), "hfg_post_fwd: ksize must be odd in [1, 11] (got %d)", ksize);
  if (B == 0) return 0;
  DLE_CHECK_ARG(x && w && bias && audio, "hfg_post_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(x, w, audio) && dle_aligned<4>(bias),
                "hfg_post_fwd: x, w and audio must be 16-byte aligned");
  DLE_CHECK_ARG(c1d_under_4gib((long long)B * T * C * 2, (long long)B * T * 4), "hfg_post_fwd: each tensor must be smaller than 4 GiB");
  const int ttiles = (T + HFG_POST_TT - 1) / HFG_POST_TT;
  const long long gx = (long long)B * ttiles;
  DLE_CHECK_ARG(gx <= 0x7FFFFFFFLL, "hfg_post_fwd: too many time tiles");
  const dim3 grid((unsigned)gx), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((hfg_post_kernel<DLE_F16>), grid, block, 0, stream, (const unsigned short*)x, (const unsigned short*)w, bias,
                       audio, T, C, ksize, ttiles, slope);
  else
    hipLaunchKernelGGL((hfg_post_kernel<DLE_BF16>), grid, block, 0, stream, (const unsigned short*)x, (const unsigned short*)w, bias,
                       audio, T, C, ksize, ttiles, slope);
  DLE_LAUNCH_CHECK();
  return 0;
}
