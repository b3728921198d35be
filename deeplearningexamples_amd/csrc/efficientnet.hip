// EfficientNet inference (MBConv blocks): the depthwise convolution with its BatchNorm, both SiLUs and the squeeze-and-excitation
// pooling in one launch, the SE gate with a SiLU (or ReLU) hidden layer of any width, and SiLU + global average pooling.
//
// Replaces, under model.eval() (Classification/ConvNets/image_classification/):
//   models/common.py:31-79     LayerBuilder.conv with groups == in_planes (convDepSep: nn.Conv2d -> BatchNorm2d -> SiLU)
//   models/common.py:123-128   the SiLU behind the stem, the expand and the features units (applied here, by the READER)
//   models/common.py:146-164, :231-250   SequentialSqueezeAndExcitation (mean over H x W, Linear, SiLU, Linear, sigmoid)
//   models/efficientnet.py:300-310       AdaptiveAvgPool2d(1) behind the features unit
//
//  * dwconv_kernel: a 256-thread workgroup owns one image, DW_TR x DW_TQ output pixels and DW_CCHUNK channels.  It stages the
//    input tile with its halo in LDS as 16-bit values AFTER the input SiLU (computed once per element, zero outside the image),
//    16 bytes = 8 channels per lane, and the k x k x 64 weights next to it.  A thread is (8-channel group, output column, half of
//    the rows): it walks down its column of taps, reads every input pixel of that column once and feeds the DW_TR / 2 output
//    rows the pixel belongs to (fp32 fmaf).  Epilogue: fmaf(scale, acc, shift), the output SiLU, one rounding, a 16-byte
//    store; the rounded values are summed per thread, then over the tile through LDS in a fixed order -> one pool partial per
//    (image, tile, channel), written once (no atomics: the result does not depend on how workgroups are scheduled).
//  * se_gate_act_kernel: one 1024-thread workgroup per image, as se_gate_kernel (csrc/se.hip) but fed by the pool partials, with
//    the mean and the hidden vector in LDS.
//  * silu_avgpool_kernel: thread = (phase, 8-channel group); fp32 sums of the ROUNDED SiLU values, phases folded in a fixed order.
#include "common.h"

#define DW_TR 8          // output rows per workgroup      (DLE_DWCONV_TILE_ROWS)
#define DW_TQ 16         // output columns per workgroup   (DLE_DWCONV_TILE_COLS)
#define DW_CCHUNK 64     // channels per workgroup         (DLE_DWCONV_CHUNK)
#define DW_THREADS 256
#define DW_RPT (DW_TR / 2)   // output rows per thread
static_assert(DW_TR == DLE_DWCONV_TILE_ROWS && DW_TQ == DLE_DWCONV_TILE_COLS && DW_CCHUNK == DLE_DWCONV_CHUNK, "header and kernel disagree");
static_assert(DW_THREADS == (DW_CCHUNK / 8) * DW_TQ * 2, "thread = (channel group, column, row half)");

// silu(v) = v / (1 + exp(-v)): the accurate expf and a true division.  Below -88 expf(-v) overflows fp32 (the quotient would be -0
// while the value, down to v = -103, is still a bf16 subnormal); there 1 + exp(v) == 1 in fp32, so the same quotient is v * exp(v).
// No NaN for finite v; silu(large negative) = -0.
__device__ __forceinline__ float silu_f32(float v) { return v < -88.0f ? v * expf(v) : v / (1.0f + expf(-v)); }

template <int DT, int K, int S>
__global__ __launch_bounds__(DW_THREADS) void dwconv_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ w,
                                                            unsigned short* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ pool, int H, int W,
                                                            int C, int P, int Q, int tiles_q, int tiles, int chunks, int in_act,
                                                            int out_act) {
  constexpr int PAD = K / 2, IR = (DW_TR - 1) * S + K, IC = (DW_TQ - 1) * S + K;
  extern __shared__ __attribute__((aligned(16))) unsigned char dw_lds[];
  ushort8_t* tile = (ushort8_t*)dw_lds;                    // [IR][IC][8 channel groups]
  ushort8_t* wl = tile + IR * IC * 8;                      // [K * K][8 channel groups]
  float* red = (float*)dw_lds;                             // [32][64] pool partials, over the tile once it has been read
  int b = blockIdx.x;
  const int chunk = b % chunks;
  b /= chunks;
  const int t = b % tiles, n = b / tiles;
  const int tp = t / tiles_q, tq = t - tp * tiles_q;
  const int p0 = tp * DW_TR, q0 = tq * DW_TQ, c0 = chunk * DW_CCHUNK;
  const int ncg = (C - c0) / 8 < 8 ? (C - c0) / 8 : 8;     // channel groups of this chunk that exist
  const int tid = threadIdx.x;
  const int h0 = p0 * S - PAD, w0 = q0 * S - PAD;
  const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  // ---- stage the input tile (after the input SiLU, rounded) and the weights
#pragma unroll 2
  for (int i = tid; i < IR * IC * 8; i += DW_THREADS) {
    const int g = i & 7, pix = i >> 3, r = pix / IC, c = pix - r * IC;
    const int h = h0 + r, ww = w0 + c;
    ushort8_t v = zero;
    if (g < ncg && h >= 0 && h < H && ww >= 0 && ww < W) {
      v = *(const ushort8_t*)(x + (((long long)n * H + h) * W + ww) * C + c0 + g * 8);
      if (in_act) {
        float f[8];
        unpack8<DT>(v, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = silu_f32(f[k]);
        v = pack8<DT>(f);
      }
    }
    tile[i] = v;
  }
  for (int i = tid; i < K * K * 8; i += DW_THREADS) {
    const int g = i & 7, tap = i >> 3;
    wl[i] = g < ncg ? *(const ushort8_t*)(w + (long long)tap * C + c0 + g * 8) : zero;
  }
  __syncthreads();
  // ---- thread = (channel group, output column, row half): DW_RPT output rows of one column
  const int cg = tid & 7, ql = (tid >> 3) & (DW_TQ - 1), rh = tid >> 7;
  constexpr int NR = (DW_RPT - 1) * S + K;                 // input rows under this thread's outputs
  const ushort8_t* col = tile + ((rh * DW_RPT * S) * IC + ql * S) * 8 + cg;
  float acc[DW_RPT][8];
#pragma unroll
  for (int j = 0; j < DW_RPT; ++j)
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
#pragma unroll 1   // (one column of taps at a time: unrolled, the K * NR tile reads are all hoisted and the kernel spills)
  for (int s = 0; s < K; ++s) {
    float wf[K][8];
#pragma unroll
    for (int r = 0; r < K; ++r) unpack8<DT>(wl[(r * K + s) * 8 + cg], wf[r]);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      float a[8];
      unpack8<DT>(col[(i * IC + s) * 8], a);
#pragma unroll
      for (int j = 0; j < DW_RPT; ++j) {
        const int r = i - j * S;                           // (compile time after unrolling)
        if (r >= 0 && r < K) {
#pragma unroll
          for (int k = 0; k < 8; ++k) acc[j][k] = __builtin_fmaf(wf[r][k], a[k], acc[j][k]);
        }
      }
    }
  }
  // ---- epilogue: BatchNorm, the output SiLU, one rounding; the pool partial of the rounded values
  const bool live = cg < ncg && q0 + ql < Q;
  float sc[8], sh[8], psum[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) sc[k] = sh[k] = psum[k] = 0.f;
  if (live) {
    const float4_t s0 = *(const float4_t*)(scale + c0 + cg * 8), s1 = *(const float4_t*)(scale + c0 + cg * 8 + 4);
    const float4_t b0 = *(const float4_t*)(shift + c0 + cg * 8), b1 = *(const float4_t*)(shift + c0 + cg * 8 + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { sc[k] = s0[k]; sc[k + 4] = s1[k]; sh[k] = b0[k]; sh[k + 4] = b1[k]; }
  }
#pragma unroll
  for (int j = 0; j < DW_RPT; ++j) {
    const int p = p0 + rh * DW_RPT + j;
    if (live && p < P) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = __builtin_fmaf(sc[k], acc[j][k], sh[k]);
        if (out_act) v[k] = silu_f32(v[k]);
      }
      const ushort8_t o = pack8<DT>(v);
      *(ushort8_t*)(y + (((long long)n * P + p) * Q + q0 + ql) * C + c0 + cg * 8) = o;
      unpack8<DT>(o, v);
#pragma unroll
      for (int k = 0; k < 8; ++k) psum[k] += v[k];
    }
  }
  if (pool) {                                              // (uniform over the grid)
    __syncthreads();                                       // every thread has read the tile: red may overwrite it
#pragma unroll
    for (int k = 0; k < 8; ++k) red[(tid >> 3) * DW_CCHUNK + cg * 8 + k] = psum[k];
    __syncthreads();
    if (tid < ncg * 8) {
      float s = red[tid];
      for (int i = 1; i < DW_THREADS / 8; ++i) s += red[i * DW_CCHUNK + tid];
      pool[((long long)n * tiles + t) * C + c0 + tid] = s;
    }
  }
}

template <int K, int S>
static constexpr size_t dw_lds_bytes() {
  return (size_t)(((DW_TR - 1) * S + K) * ((DW_TQ - 1) * S + K) + K * K) * 8 * 16;
}
static_assert(dw_lds_bytes<3, 1>() >= (DW_THREADS / 8) * DW_CCHUNK * sizeof(float), "the pool partials must fit over the tile");
static_assert(dw_lds_bytes<5, 2>() <= 160 * 1024, "tile larger than the LDS");

static int dw_tiles(int H, int W, int ksize, int stride, int* P, int* Q, int* tiles_q) {
  const int pad = ksize / 2;
  *P = (H + 2 * pad - ksize) / stride + 1;
  *Q = (W + 2 * pad - ksize) / stride + 1;
  *tiles_q = (*Q + DW_TQ - 1) / DW_TQ;
  const long long t = (long long)((*P + DW_TR - 1) / DW_TR) * *tiles_q;
  return t < (1ll << 30) ? (int)t : -1;
}

extern "C" int dle_dwconv2d_pool_bands(int H, int W, int C, int ksize, int stride) {
  DLE_CHECK_ARG(H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "dwconv2d_pool_bands: bad shape (H, W >= 1, C a multiple of 8)");
  DLE_CHECK_ARG(ksize == 3 || ksize == 5, "dwconv2d_pool_bands: ksize 3 or 5 (got %d)", ksize);
  DLE_CHECK_ARG(stride == 1 || stride == 2, "dwconv2d_pool_bands: stride 1 or 2 (got %d)", stride);
  int P, Q, tq;
  return dw_tiles(H, W, ksize, stride, &P, &Q, &tq);
}

template <int DT, int K, int S>
static void dw_launch(const void* x, const void* w, void* y, const float* scale, const float* shift, float* pool, int H, int W, int C,
                      int P, int Q, int tiles_q, int tiles, int chunks, unsigned grid, int in_act, int out_act, hipStream_t stream) {
  DLE_LAUNCH_LDS((dwconv_kernel<DT, K, S>), dim3(grid), dim3(DW_THREADS), (dw_lds_bytes<K, S>()), stream, (const unsigned short*)x,
                 (const unsigned short*)w, (unsigned short*)y, scale, shift, pool, H, W, C, P, Q, tiles_q, tiles, chunks, in_act, out_act);
}

extern "C" int dle_dwconv2d_act_fwd(const void* x, const void* w, void* y, const float* scale, const float* shift, float* pool,
                                    int64_t pool_bytes, int N, int H, int W, int C, int ksize, int stride, int in_act, int out_act,
                                    int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "dwconv2d_act_fwd: 16-bit activations and weights only");
  DLE_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && C >= 8 && C % 8 == 0, "dwconv2d_act_fwd: bad shape (C must be a multiple of 8, got %d)", C);
  DLE_CHECK_ARG(ksize == 3 || ksize == 5, "dwconv2d_act_fwd: ksize 3 or 5 (got %d)", ksize);
  DLE_CHECK_ARG(stride == 1 || stride == 2, "dwconv2d_act_fwd: stride 1 or 2 (got %d)", stride);
  DLE_CHECK_ARG((in_act == 0 || in_act == 1) && (out_act == 0 || out_act == 1), "dwconv2d_act_fwd: in_act / out_act are 0 or 1");
  int P, Q, tiles_q;
  const int tiles = dw_tiles(H, W, ksize, stride, &P, &Q, &tiles_q);
  const int chunks = (C + DW_CCHUNK - 1) / DW_CCHUNK;
  const long long blocks = (long long)N * (tiles > 0 ? tiles : 0) * chunks;
  DLE_CHECK_ARG(tiles > 0 && blocks < (1ll << 31) && (long long)N * H * W * C < (1ll << 31) && (long long)N * tiles * C < (1ll << 31),
                "dwconv2d_act_fwd: tensor too large (each tensor below 2^31 elements, fewer than 2^31 workgroups)");
  DLE_CHECK_ARG(!pool || pool_bytes >= (int64_t)N * tiles * C * 4,
                "dwconv2d_act_fwd: pool holds %lld bytes, N * G * C fp32 = %lld needed (G = %d from dle_dwconv2d_pool_bands)",
                (long long)pool_bytes, (long long)N * tiles * C * 4, tiles);
  if (N == 0) return 0;
  DLE_CHECK_ARG(x && w && y && scale && shift, "dwconv2d_act_fwd: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y) | ((uintptr_t)scale) | ((uintptr_t)shift) | ((uintptr_t)pool)) & 15),
                "dwconv2d_act_fwd: every operand must be 16-byte aligned");
#define DW_GO(DT, K, S) dw_launch<DT, K, S>(x, w, y, scale, shift, pool, H, W, C, P, Q, tiles_q, tiles, chunks, (unsigned)blocks, in_act, out_act, stream)
  if (dtype == DLE_F16) {
    if (ksize == 3) { if (stride == 1) DW_GO(DLE_F16, 3, 1); else DW_GO(DLE_F16, 3, 2); }
    else { if (stride == 1) DW_GO(DLE_F16, 5, 1); else DW_GO(DLE_F16, 5, 2); }
  } else {
    if (ksize == 3) { if (stride == 1) DW_GO(DLE_BF16, 3, 1); else DW_GO(DLE_BF16, 3, 2); }
    else { if (stride == 1) DW_GO(DLE_BF16, 5, 1); else DW_GO(DLE_BF16, 5, 2); }
  }
#undef DW_GO
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- SE gate
#define SEA_THREADS 1024

__global__ __launch_bounds__(SEA_THREADS) void se_gate_act_kernel(const float* __restrict__ pool, int G, float inv_hw,
                                                                  const float* __restrict__ w1, const float* __restrict__ b1,
                                                                  const float* __restrict__ w2, const float* __restrict__ b2,
                                                                  float* __restrict__ gate, int C, int S, int act) {
  extern __shared__ __attribute__((aligned(16))) float sea_lds[];
  float* mean = sea_lds;                                   // [C]
  float* hid = sea_lds + C;                                // [S]
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* pn = pool + (long long)n * G * C;
  for (int c = tid; c < C; c += SEA_THREADS) {
    float s = pn[c];
    for (int g = 1; g < G; ++g) s += pn[(long long)g * C + c];
    mean[c] = inv_hw * s;
  }
  __syncthreads();
  // ---- squeeze: hid[s] = f(b1[s] + w1[s, :] . mean), one wavefront per s
  const int lane = tid & 63, wave = tid >> 6;
  for (int s = wave; s < S; s += SEA_THREADS / 64) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = __builtin_fmaf(w1[(long long)s * C + c], mean[c], a);
    a = wave_sum(a) + b1[s];
    if (lane == 0) hid[s] = act ? silu_f32(a) : (a > 0.f ? a : 0.f);
  }
  __syncthreads();
  // ---- expand + sigmoid
  for (int c = tid; c < C; c += SEA_THREADS) {
    float z = b2[c];
    for (int s = 0; s < S; ++s) z = __builtin_fmaf(w2[(long long)c * S + s], hid[s], z);
    gate[(long long)n * C + c] = 1.0f / (1.0f + expf(-z));
  }
}

extern "C" int dle_se_gate_act(const float* pool, int G, float inv_hw, const float* w1, const float* b1, const float* w2,
                               const float* b2, float* gate, int N, int C, int S, int act, hipStream_t stream) {
  DLE_CHECK_ARG(N >= 0 && G >= 1 && C >= 8 && C % 8 == 0, "se_gate_act: bad shape (G >= 1, C a multiple of 8)");
  DLE_CHECK_ARG(S >= 1 && C + S <= DLE_SE_GATE_ACT_MAX_C_PLUS_S,
                "se_gate_act: C + S = %d: the mean and the hidden vector live in LDS, C + S <= %d", C + S, DLE_SE_GATE_ACT_MAX_C_PLUS_S);
  DLE_CHECK_ARG(act == 0 || act == 1, "se_gate_act: act is 0 (ReLU) or 1 (SiLU)");
  DLE_CHECK_ARG((long long)N * G * C < (1ll << 31), "se_gate_act: pool too large (below 2^31 elements)");
  if (N == 0) return 0;
  DLE_CHECK_ARG(pool && w1 && b1 && w2 && b2 && gate, "se_gate_act: null pointer");
  const size_t lds = (size_t)(C + S) * sizeof(float);
  hipLaunchKernelGGL(se_gate_act_kernel, dim3(N), dim3(SEA_THREADS), lds, stream, pool, G, inv_hw, w1, b1, w2, b2, gate, C, S, act);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ------------------------------------------------------------------------------------------------ SiLU + average pooling
#define SAP_PHASES 32

template <int DT>
__global__ __launch_bounds__(SAP_PHASES * 8) void silu_avgpool_kernel(const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
                                                                      int HW, int C, int cblocks) {
  __shared__ float red[SAP_PHASES * 64];
  const int n = blockIdx.x / cblocks, c0 = (blockIdx.x % cblocks) * 64;
  const int tid = threadIdx.x, cg = tid & 7, ph = tid >> 3;
  const bool live = c0 + cg * 8 < C;
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  if (live) {
    const unsigned short* xn = x + (long long)n * HW * C + c0 + cg * 8;
    for (int hw = ph; hw < HW; hw += SAP_PHASES) {
      float f[8];
      unpack8<DT>(*(const ushort8_t*)(xn + (long long)hw * C), f);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = silu_f32(f[k]);
      unpack8<DT>(pack8<DT>(f), f);                        // the SiLU writes a 16-bit tensor
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] += f[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[ph * 64 + cg * 8 + k] = acc[k];
  __syncthreads();
  if (tid < 64 && c0 + tid < C) {
    float s = red[tid];
    for (int i = 1; i < SAP_PHASES; ++i) s += red[i * 64 + tid];
    y[(long long)n * C + c0 + tid] = Elem<DT>::from_f32((1.0f / (float)HW) * s);
  }
}

extern "C" int dle_silu_avgpool_fwd(const void* x, void* y, int N, int HW, int C, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "silu_avgpool_fwd: 16-bit activations only");
  DLE_CHECK_ARG(N >= 0 && HW >= 1 && C >= 8 && C % 8 == 0, "silu_avgpool_fwd: bad shape (C must be a multiple of 8)");
  const int cblocks = (C + 63) / 64;
  DLE_CHECK_ARG((long long)N * HW * C < (1ll << 31) && (long long)N * cblocks < (1ll << 31), "silu_avgpool_fwd: tensor too large (below 2^31 elements)");
  if (N == 0) return 0;
  DLE_CHECK_ARG(x && y, "silu_avgpool_fwd: null pointer");
  DLE_CHECK_ARG(!(((uintptr_t)x) & 15), "silu_avgpool_fwd: x must be 16-byte aligned");
  if (dtype == DLE_F16) hipLaunchKernelGGL(silu_avgpool_kernel<DLE_F16>, dim3((unsigned)(N * cblocks)), dim3(SAP_PHASES * 8), 0, stream, (const unsigned short*)x, (unsigned short*)y, HW, C, cblocks);
  else hipLaunchKernelGGL(silu_avgpool_kernel<DLE_BF16>, dim3((unsigned)(N * cblocks)), dim3(SAP_PHASES * 8), 0, stream, (const unsigned short*)x, (unsigned short*)y, HW, C, cblocks);
  DLE_LAUNCH_CHECK();
  return 0;
}
