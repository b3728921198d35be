// nnU-Net (BraTS22 UNet3D) inference on gfx950 (reference: PyTorch/Segmentation/nnUNet/nnunet/brats22_model.py): the 3x3x3
// convolution with the InstanceNorm of its input applied on the operand load, the fold of the statistic partials into the
// (scale, shift) table of the next layer, the trilinear x2 upsample and the output block fused with the sliding-window blend.
//
// dle_conv3d_in_fwd.  Implicit GEMM out^T = W A^T with v_mfma_f32_32x32x16: the weight rows [Ko][27 C] are the A operand, 128
// output voxels of one sample the B operand, so a lane ends up with 16 output channels of ONE voxel (channel (r & 3) + 8 (r >> 2) +
// 4 (lane >> 5) of the wavefront's 32-channel block in accumulator register r) and stores them 8 bytes at a time.  A workgroup of
// four wavefronts owns a 128 voxel x 64 channel tile: wavefront w takes voxel half w & 1 and channel half w >> 1.  The K loop walks
// 64-deep chunks of (tap, channel); the chunk after the current one is in registers (global loads issued before the MFMAs of the
// current chunk), and the InstanceNorm transform  a = round16(relu?(fma(scale, x, shift)))  runs on those registers on their way
// into LDS: the normalised volume never exists in memory, and a voxel outside the volume is written as 0, not as `shift`.
// A workgroup walks the tiles of one BAND of output voxels and keeps (count, mean, M2) of what it stored per lane (Welford); at the
// end of the band the lanes and the two voxel halves are merged by Chan's formula in a fixed order and ONE thread per channel
// writes the band's partial.  No atomics, no workgroup waits on another.
#include "gemm_tiles.h"
#include "mfma32_rows.h"
#include <math.h>

#define NU_TM 128                    // output voxels per tile
#define NU_TN 64                     // output channels per tile
#define NU_BK 64                     // K chunk
#define NU_LD 72                     // halves per LDS line: 144 bytes
#define NU_THREADS 256
#define NU_MAX_BANDS 512

struct NuStat { float n, mean, m2; };

// Chan's merge of two (count, mean, M2) triples; either side may be empty
__device__ __host__ __forceinline__ NuStat nu_merge(NuStat a, NuStat b) {
  NuStat o;
  o.n = a.n + b.n;
  const float w = o.n > 0.f ? b.n / o.n : 0.f;
  const float d = b.mean - a.mean;
  o.mean = a.mean + d * w;
  o.m2 = a.m2 + b.m2 + d * d * a.n * w;
  return o;
}

struct NuConvArgs {
  const unsigned short* x;
  const float *scale, *shift;
  const unsigned short* w;
  unsigned short* y;
  float* part;
  long long ldx, x_off, ldy, y_off;
  int N, D, H, W, C, Ko, P, Q, R, stride, relu_in, relu_out;
  int ntiles, tiles_per_band, G;
};

static int nu_tiles_per_band(long long voxels, int* ntiles_out) {
  const long long ntiles = (voxels + NU_TM - 1) / NU_TM;
  if (ntiles_out) *ntiles_out = (int)ntiles;
  return (int)((ntiles + NU_MAX_BANDS - 1) / NU_MAX_BANDS);
}

template <int DT>
__global__ __launch_bounds__(NU_THREADS) void nu_conv3d_in_kernel(NuConvArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned short As[NU_TM * NU_LD];
  __shared__ __attribute__((aligned(16))) unsigned short Ws[NU_TN * NU_LD];
  __shared__ float red[2 * NU_TN * 3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, l31 = lane & 31;
  const int vh = wave & 1, kh = wave >> 1;
  const int band = blockIdx.x, ko0 = blockIdx.y * NU_TN, n = blockIdx.z;
  const int kc = tid & 7, lrow = tid >> 3;                       // the loader's view: chunk kc of rows lrow + 32 j
  const int PQR = p.P * p.Q * p.R, QR = p.Q * p.R;
  const int Kw = 27 * p.C, nk = (Kw + NU_BK - 1) / NU_BK;
  const bool stem = p.C == 8;
  const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // running statistics of the lane's voxels: one count, 16 channels
  float cnt = 0.f, mean[16], m2[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) mean[i] = m2[i] = 0.f;

  const int t_begin = band * p.tiles_per_band;
  const int t_end = min(t_begin + p.tiles_per_band, p.ntiles);
  for (int tile = t_begin; tile < t_end; ++tile) {
    // the loader's four voxels: input coordinates of tap (0, 0, 0), or a row outside the sample
    int id0[4], ih0[4], iw0[4];
    bool rok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int m = tile * NU_TM + lrow + 32 * j;
      rok[j] = m < PQR;
      const int od = m / QR, rem = m - od * QR, oh = rem / p.R, ow = rem - oh * p.R;
      id0[j] = od * p.stride - 1;
      ih0[j] = oh * p.stride - 1;
      iw0[j] = ow * p.stride - 1;
    }

    ushort8_t xr[4], wr[2];
    float sc[8], sh[8];
    unsigned inside = 0;
    auto prefetch = [&](int i) {
      const int k0 = i * NU_BK;
      int tap, c;
      if (stem) { tap = (k0 >> 3) + kc; c = 0; }
      else { tap = k0 / p.C; c = k0 - tap * p.C + kc * 8; }
      const bool tap_ok = tap < 27;
      const int kd = tap / 9, kr = tap - kd * 9, kh2 = kr / 3, kw = kr - kh2 * 3;
      inside = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = id0[j] + kd, h = ih0[j] + kh2, w = iw0[j] + kw;
        const bool ok = rok[j] && tap_ok && d >= 0 && d < p.D && h >= 0 && h < p.H && w >= 0 && w < p.W;
        xr[j] = zero8;
        if (ok) {
          const long long vox = (((long long)n * p.D + d) * p.H + h) * p.W + w;
          xr[j] = *(const ushort8_t*)(p.x + vox * p.ldx + p.x_off + c);
          inside |= 1u << j;
        }
      }
      if (p.scale != nullptr && tap_ok) {
        const float4_t s0 = *(const float4_t*)(p.scale + (long long)n * p.C + c), s1 = *(const float4_t*)(p.scale + (long long)n * p.C + c + 4);
        const float4_t h0 = *(const float4_t*)(p.shift + (long long)n * p.C + c), h1 = *(const float4_t*)(p.shift + (long long)n * p.C + c + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { sc[e] = s0[e]; sc[4 + e] = s1[e]; sh[e] = h0[e]; sh[4 + e] = h1[e]; }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = k0 + kc * 8;
        wr[j] = k < Kw ? *(const ushort8_t*)(p.w + (long long)(ko0 + lrow + 32 * j) * Kw + k) : zero8;
      }
    };
    auto stage = [&]() {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ushort8_t v = xr[j];
        if (p.scale != nullptr && (inside >> j & 1)) {
          float f[8];
          unpack8<DT>(v, f);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            f[e] = fmaf(sc[e], f[e], sh[e]);
            if (p.relu_in) f[e] = fmaxf(f[e], 0.f);
          }
          v = pack8<DT>(f);
        }
        *(ushort8_t*)(As + (lrow + 32 * j) * NU_LD + kc * 8) = v;
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) *(ushort8_t*)(Ws + (lrow + 32 * j) * NU_LD + kc * 8) = wr[j];
    };

    float16_t acc0, acc1;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc0[i] = acc1[i] = 0.f;

    prefetch(0);
    for (int i = 0; i < nk; ++i) {
      __syncthreads();                                   // every wavefront has read the previous chunk
      stage();
      __syncthreads();
      if (i + 1 < nk) prefetch(i + 1);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int ko = ks * 16 + hf * 8;
        const ushort8_t a = *(const ushort8_t*)(Ws + (kh * 32 + l31) * NU_LD + ko);
        const ushort8_t b0 = *(const ushort8_t*)(As + (vh * 64 + l31) * NU_LD + ko);
        const ushort8_t b1 = *(const ushort8_t*)(As + (vh * 64 + 32 + l31) * NU_LD + ko);
        acc0 = Mfma32x16<DT>::run(a, b0, acc0);
        acc1 = Mfma32x16<DT>::run(a, b1, acc1);
      }
    }

    // epilogue: ReLU, one rounding, 8-byte stores; Welford update with what was stored
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const float16_t& acc = f ? acc1 : acc0;
      const int m = tile * NU_TM + vh * 64 + f * 32 + l31;
      if (m < PQR) {
        unsigned short* yp = p.y + ((long long)n * PQR + m) * p.ldy + p.y_off + ko0 + kh * 32 + 4 * hf;
        cnt += 1.f;
        const float inv = 1.f / cnt;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          unsigned short h[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = acc[4 * g + e];
            if (p.relu_out) v = fmaxf(v, 0.f);
            h[e] = Elem<DT>::from_f32(v);
            if (p.part != nullptr) {
              const float yv = Elem<DT>::to_f32(h[e]);
              const float d = yv - mean[4 * g + e];
              mean[4 * g + e] += d * inv;
              m2[4 * g + e] = fmaf(d, yv - mean[4 * g + e], m2[4 * g + e]);
            }
          }
          uint2_t o;
          o[0] = (unsigned)h[0] | ((unsigned)h[1] << 16);
          o[1] = (unsigned)h[2] | ((unsigned)h[3] << 16);
          *(uint2_t*)(yp + 8 * g) = o;
        }
      }
    }
  }

  if (p.part == nullptr) return;
  // the 32 lanes of a half-wavefront hold the same 16 channels of different voxels: butterfly of Chan merges (fixed order)
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) {
    const float cb = __shfl_xor(cnt, o, 64);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      NuStat a = {cnt, mean[i], m2[i]}, b = {cb, __shfl_xor(mean[i], o, 64), __shfl_xor(m2[i], o, 64)};
      // both partners merge (lower lane, higher lane) in that order so that they agree bit for bit
      const NuStat r = (lane & o) ? nu_merge(b, a) : nu_merge(a, b);
      mean[i] = r.mean;
      m2[i] = r.m2;
    }
    cnt += cb;
  }
  if (l31 == 0) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int kl = kh * 32 + rt_feat(i, hf);
      float* r = red + (vh * NU_TN + kl) * 3;
      r[0] = cnt; r[1] = mean[i]; r[2] = m2[i];
    }
  }
  __syncthreads();
  if (tid < NU_TN) {
    const float* r0 = red + tid * 3;
    const float* r1 = red + (NU_TN + tid) * 3;
    const NuStat a = {r0[0], r0[1], r0[2]}, b = {r1[0], r1[1], r1[2]};
    const NuStat r = nu_merge(a, b);
    float* o = p.part + (((long long)n * p.G + band) * p.Ko + ko0 + tid) * 3;
    o[0] = r.n; o[1] = r.mean * r.n; o[2] = r.m2;
  }
}

static bool nu_aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

extern "C" int dle_conv3d_in_bands(int D, int H, int W, int stride) {
  if (D < 1 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return -1;
  const long long v = (long long)((D - 1) / stride + 1) * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  int ntiles = 0;
  const int tpb = nu_tiles_per_band(v, &ntiles);
  return (ntiles + tpb - 1) / tpb;
}

extern "C" int dle_conv3d_in_fwd(const void* x, int64_t ldx, int64_t x_off, const float* scale, const float* shift, const void* w,
                                 void* y, int64_t ldy, int64_t y_off, float* part, int N, int D, int H, int W, int C, int Ko,
                                 int stride, int relu_in, int relu_out, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "dle_conv3d_in_fwd: 16-bit operands only (dtype %d)", dtype);
  DLE_CHECK_ARG(x && w && y, "dle_conv3d_in_fwd: null operand");
  DLE_CHECK_ARG((scale == nullptr) == (shift == nullptr), "dle_conv3d_in_fwd: scale and shift go together");
  DLE_CHECK_ARG(N >= 1 && D >= 1 && H >= 1 && W >= 1, "dle_conv3d_in_fwd: bad extents N=%d D=%d H=%d W=%d", N, D, H, W);
  DLE_CHECK_ARG(stride == 1 || stride == 2, "dle_conv3d_in_fwd: stride 1 or 2 (got %d)", stride);
  DLE_CHECK_ARG(Ko >= 64 && Ko % 64 == 0, "dle_conv3d_in_fwd: Ko %% 64 == 0 (got %d)", Ko);
  DLE_CHECK_ARG(C == 8 || (C >= 64 && C % 64 == 0), "dle_conv3d_in_fwd: C %% 64 == 0 or C == 8 (got %d)", C);
  DLE_CHECK_ARG(ldx >= C && ldx % 8 == 0 && x_off >= 0 && x_off % 8 == 0 && x_off + C <= ldx,
                "dle_conv3d_in_fwd: input slice [%lld, %lld) of a line of %lld", (long long)x_off, (long long)x_off + C, (long long)ldx);
  DLE_CHECK_ARG(ldy >= Ko && ldy % 8 == 0 && y_off >= 0 && y_off % 8 == 0 && y_off + Ko <= ldy,
                "dle_conv3d_in_fwd: output slice [%lld, %lld) of a line of %lld", (long long)y_off, (long long)y_off + Ko, (long long)ldy);
  DLE_CHECK_ARG(nu_aligned16(x) && nu_aligned16(w) && nu_aligned16(y) && nu_aligned16(scale) && nu_aligned16(shift) && nu_aligned16(part),
                "dle_conv3d_in_fwd: operands must be 16-byte aligned");
  const int P = (D - 1) / stride + 1, Q = (H - 1) / stride + 1, R = (W - 1) / stride + 1;
  const long long lim = 1ll << 31;
  DLE_CHECK_ARG((long long)N * D * H * W * ldx < lim && (long long)N * P * Q * R * ldy < lim && (long long)Ko * 27 * C < lim,
                "dle_conv3d_in_fwd: a tensor has 2^31 elements or more");
  DLE_CHECK_ARG(N <= 65535 && Ko / 64 <= 65535, "dle_conv3d_in_fwd: grid too large");
  NuConvArgs a;
  a.x = (const unsigned short*)x; a.scale = scale; a.shift = shift; a.w = (const unsigned short*)w; a.y = (unsigned short*)y; a.part = part;
  a.ldx = ldx; a.x_off = x_off; a.ldy = ldy; a.y_off = y_off;
  a.N = N; a.D = D; a.H = H; a.W = W; a.C = C; a.Ko = Ko; a.P = P; a.Q = Q; a.R = R; a.stride = stride;
  a.relu_in = relu_in != 0; a.relu_out = relu_out != 0;
  a.tiles_per_band = nu_tiles_per_band((long long)P * Q * R, &a.ntiles);
  a.G = (a.ntiles + a.tiles_per_band - 1) / a.tiles_per_band;
  const dim3 grid(a.G, Ko / NU_TN, N);
  if (dtype == DLE_F16) hipLaunchKernelGGL(nu_conv3d_in_kernel<DLE_F16>, grid, dim3(NU_THREADS), 0, stream, a);
  else hipLaunchKernelGGL(nu_conv3d_in_kernel<DLE_BF16>, grid, dim3(NU_THREADS), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_instnorm_fold ------------------------------------------------------------------------------------------------------
__global__ void nu_fold_kernel(const float* part, int G, int C, const float* gamma, const float* beta, float eps, float* scale,
                               float* shift, long long ld_out, long long out_off, int N) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C;
  NuStat s = {0.f, 0.f, 0.f};
  for (int g = 0; g < G; ++g) {
    const float* q = part + (((long long)n * G + g) * C + c) * 3;
    const float cn = q[0];
    const NuStat b = {cn, cn > 0.f ? q[1] / cn : 0.f, q[2]};
    s = nu_merge(s, b);
  }
  const float var = s.n > 0.f ? s.m2 / s.n : 0.f;
  const float sc = gamma[c] / sqrtf(var + eps);
  scale[n * ld_out + out_off + c] = sc;
  shift[n * ld_out + out_off + c] = fmaf(-s.mean, sc, beta[c]);
}

extern "C" int dle_instnorm_fold(const float* part, int G, int C, const float* gamma, const float* beta, float eps, float* scale,
                                 float* shift, int64_t ld_out, int64_t out_off, int N, hipStream_t stream) {
  DLE_CHECK_ARG(part && gamma && beta && scale && shift, "dle_instnorm_fold: null operand");
  DLE_CHECK_ARG(G >= 1 && C >= 1 && N >= 1, "dle_instnorm_fold: bad sizes G=%d C=%d N=%d", G, C, N);
  DLE_CHECK_ARG(out_off >= 0 && out_off + C <= ld_out, "dle_instnorm_fold: slice [%lld, %lld) of a line of %lld", (long long)out_off,
                (long long)out_off + C, (long long)ld_out);
  DLE_CHECK_ARG(eps >= 0.f, "dle_instnorm_fold: negative eps");
  DLE_CHECK_ARG((long long)N * C < (1ll << 31) && (long long)N * G * C * 3 < (1ll << 40), "dle_instnorm_fold: too large");
  const int total = N * C;
  hipLaunchKernelGGL(nu_fold_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, part, G, C, gamma, beta, eps, scale, shift,
                     (long long)ld_out, (long long)out_off, N);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_upsample3d_x2_fwd --------------------------------------------------------------------------------------------------
// Output index i of an axis of extent E (output 2 E) reads source position i (E - 1) / (2 E - 1): i0 = floor, lambda = the
// fraction as the correctly rounded fp32 quotient of two integers, i1 = min(i0 + 1, E - 1).  Nested lerps fma(lambda, b - a, a)
// along w, h, d in fp32, one rounding at the end; equal neighbours (and extent 1) reproduce their value exactly.
#define NU_UP_THREADS 256
#define NU_UP_MAX_BANDS 1024
#define NU_UP_MIN_BAND 64

static long long nu_up_band_voxels(long long voxels) {
  const long long b = (voxels + NU_UP_MAX_BANDS - 1) / NU_UP_MAX_BANDS;
  return b > NU_UP_MIN_BAND ? b : NU_UP_MIN_BAND;
}

struct NuUpArgs {
  const unsigned short* x;
  unsigned short* y;
  float* part;
  long long ldx, x_off, ldy, y_off, band_voxels;
  int N, D, H, W, C, G;
};

__device__ __forceinline__ void nu_axis(int i, int E, int& i0, int& i1, float& lam) {
  const int den = 2 * E - 1, num = i * (E - 1);
  i0 = num / den;
  lam = (float)(num - i0 * den) / (float)den;
  i1 = min(i0 + 1, E - 1);
}

template <int DT>
__global__ __launch_bounds__(NU_UP_THREADS) void nu_upsample_kernel(NuUpArgs p) {
  extern __shared__ float up_red[];                           // [VL][C][3]
  const int CG = p.C >> 3, VL = NU_UP_THREADS / CG;
  const int tid = threadIdx.x, cg = tid % CG, vl = tid / CG;
  const int band = blockIdx.x, n = blockIdx.y;
  const int OH = 2 * p.H, OW = 2 * p.W;
  const long long V = 8ll * p.D * p.H * p.W;
  const long long v0 = band * p.band_voxels, v1 = min(v0 + p.band_voxels, V);
  float cnt = 0.f, mean[8], m2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mean[e] = m2[e] = 0.f;
  if (vl < VL) {
    const unsigned short* xn = p.x + (long long)n * p.D * p.H * p.W * p.ldx + p.x_off + cg * 8;
    for (long long v = v0 + vl; v < v1; v += VL) {
      const int od = (int)(v / ((long long)OH * OW));
      const int rem = (int)(v - (long long)od * OH * OW), oh = rem / OW, ow = rem - oh * OW;
      int d0, d1, h0, h1, w0, w1;
      float ld, lh, lw;
      nu_axis(od, p.D, d0, d1, ld);
      nu_axis(oh, p.H, h0, h1, lh);
      nu_axis(ow, p.W, w0, w1, lw);
      float c[2][2][8];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const long long row = ((long long)(a ? d1 : d0) * p.H + (b ? h1 : h0)) * p.W;
          float f0[8], f1[8];
          unpack8<DT>(*(const ushort8_t*)(xn + (row + w0) * p.ldx), f0);
          unpack8<DT>(*(const ushort8_t*)(xn + (row + w1) * p.ldx), f1);
#pragma unroll
          for (int e = 0; e < 8; ++e) c[a][b][e] = fmaf(lw, f1[e] - f0[e], f0[e]);
        }
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float t0 = fmaf(lh, c[0][1][e] - c[0][0][e], c[0][0][e]);
        const float t1 = fmaf(lh, c[1][1][e] - c[1][0][e], c[1][0][e]);
        o[e] = fmaf(ld, t1 - t0, t0);
      }
      const ushort8_t packed = pack8<DT>(o);
      *(ushort8_t*)(p.y + ((long long)n * V + v) * p.ldy + p.y_off + cg * 8) = packed;
      if (p.part != nullptr) {
        float yv[8];
        unpack8<DT>(packed, yv);
        cnt += 1.f;
        const float inv = 1.f / cnt;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float d = yv[e] - mean[e];
          mean[e] += d * inv;
          m2[e] = fmaf(d, yv[e] - mean[e], m2[e]);
        }
      }
    }
  }
  if (p.part == nullptr) return;
  if (vl < VL) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float* r = up_red + ((long long)vl * p.C + cg * 8 + e) * 3;
      r[0] = cnt; r[1] = mean[e]; r[2] = m2[e];
    }
  }
  __syncthreads();
  for (int c = tid; c < p.C; c += NU_UP_THREADS) {
    NuStat s = {0.f, 0.f, 0.f};
    for (int l = 0; l < VL; ++l) {
      const float* r = up_red + ((long long)l * p.C + c) * 3;
      const NuStat b = {r[0], r[1], r[2]};
      s = nu_merge(s, b);
    }
    float* o = p.part + (((long long)n * p.G + band) * p.C + c) * 3;
    o[0] = s.n; o[1] = s.mean * s.n; o[2] = s.m2;
  }
}

extern "C" int dle_upsample3d_x2_bands(int D, int H, int W) {
  if (D < 1 || H < 1 || W < 1) return -1;
  const long long V = 8ll * D * H * W, bv = nu_up_band_voxels(V);
  return (int)((V + bv - 1) / bv);
}

extern "C" int dle_upsample3d_x2_fwd(const void* x, int64_t ldx, int64_t x_off, void* y, int64_t ldy, int64_t y_off, float* part, int N,
                                     int D, int H, int W, int C, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "dle_upsample3d_x2_fwd: 16-bit operands only (dtype %d)", dtype);
  DLE_CHECK_ARG(x && y, "dle_upsample3d_x2_fwd: null operand");
  DLE_CHECK_ARG(N >= 1 && N <= 65535 && D >= 1 && H >= 1 && W >= 1, "dle_upsample3d_x2_fwd: bad extents N=%d D=%d H=%d W=%d", N, D, H, W);
  DLE_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= 8 * NU_UP_THREADS, "dle_upsample3d_x2_fwd: C %% 8 == 0, C <= %d (got %d)", 8 * NU_UP_THREADS, C);
  DLE_CHECK_ARG(ldx >= C && ldx % 8 == 0 && x_off >= 0 && x_off % 8 == 0 && x_off + C <= ldx,
                "dle_upsample3d_x2_fwd: input slice [%lld, %lld) of a line of %lld", (long long)x_off, (long long)x_off + C, (long long)ldx);
  DLE_CHECK_ARG(ldy >= C && ldy % 8 == 0 && y_off >= 0 && y_off % 8 == 0 && y_off + C <= ldy,
                "dle_upsample3d_x2_fwd: output slice [%lld, %lld) of a line of %lld", (long long)y_off, (long long)y_off + C, (long long)ldy);
  DLE_CHECK_ARG(nu_aligned16(x) && nu_aligned16(y) && nu_aligned16(part), "dle_upsample3d_x2_fwd: operands must be 16-byte aligned");
  const long long V = 8ll * D * H * W, lim = 1ll << 31;
  DLE_CHECK_ARG((long long)N * D * H * W * ldx < lim && (long long)N * V * ldy < lim, "dle_upsample3d_x2_fwd: a tensor has 2^31 elements or more");
  NuUpArgs a;
  a.x = (const unsigned short*)x; a.y = (unsigned short*)y; a.part = part;
  a.ldx = ldx; a.x_off = x_off; a.ldy = ldy; a.y_off = y_off;
  a.N = N; a.D = D; a.H = H; a.W = W; a.C = C;
  a.band_voxels = nu_up_band_voxels(V);
  a.G = (int)((V + a.band_voxels - 1) / a.band_voxels);
  const int VL = NU_UP_THREADS / (C / 8);
  const size_t lds = part ? (size_t)VL * C * 3 * sizeof(float) : 0;          // at most 256 / (C / 8) * C * 12 = 24 KiB
  if (dtype == DLE_F16) hipLaunchKernelGGL(nu_upsample_kernel<DLE_F16>, dim3(a.G, N), dim3(NU_UP_THREADS), lds, stream, a);
  else hipLaunchKernelGGL(nu_upsample_kernel<DLE_BF16>, dim3(a.G, N), dim3(NU_UP_THREADS), lds, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_nnunet_head_blend_fwd ----------------------------------------------------------------------------------------------
#define NU_HEAD_MAXK 8
#define NU_HEAD_MAXC 512

struct NuHeadArgs {
  const unsigned short *x, *w;
  const float *b, *imp;
  float* out;
  long long ldx;
  int K, C, Dp, Hp, Wp, Dv, Hv, Wv, d0, h0, w0;
};

template <int DT>
__global__ __launch_bounds__(256) void nu_head_blend_kernel(NuHeadArgs p) {
  __shared__ float wsh[NU_HEAD_MAXK * NU_HEAD_MAXC];
  for (int i = threadIdx.x; i < p.K * p.C; i += blockDim.x) wsh[i] = Elem<DT>::to_f32(p.w[i]);
  __syncthreads();
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= p.Dp * p.Hp * p.Wp) return;
  const int d = v / (p.Hp * p.Wp), rem = v - d * p.Hp * p.Wp, h = rem / p.Wp, w = rem - h * p.Wp;
  float acc[NU_HEAD_MAXK];
#pragma unroll
  for (int k = 0; k < NU_HEAD_MAXK; ++k) acc[k] = 0.f;
  const unsigned short* xp = p.x + (long long)v * p.ldx;
  for (int c = 0; c < p.C; c += 8) {
    float f[8];
    unpack8<DT>(*(const ushort8_t*)(xp + c), f);
#pragma unroll
    for (int k = 0; k < NU_HEAD_MAXK; ++k)
      if (k < p.K) {                                   // (uniform: the classes that exist, 3 for this network)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[k] = fmaf(wsh[k * p.C + c + e], f[e], acc[k]);
      }
  }
  const float iw = p.imp[v];
  const long long plane = (long long)p.Dv * p.Hv * p.Wv;
  const long long o = ((long long)(p.d0 + d) * p.Hv + (p.h0 + h)) * p.Wv + (p.w0 + w);
#pragma unroll
  for (int k = 0; k < NU_HEAD_MAXK; ++k)
    if (k < p.K) p.out[k * plane + o] += iw * (p.b[k] + acc[k]);
}

extern "C" int dle_nnunet_head_blend_fwd(const void* x, int64_t ldx, const void* w, const float* b, const float* imp, float* out, int K,
                                         int C, int Dp, int Hp, int Wp, int Dv, int Hv, int Wv, int d0, int h0, int w0, int dtype,
                                         hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "dle_nnunet_head_blend_fwd: 16-bit activations only (dtype %d)", dtype);
  DLE_CHECK_ARG(x && w && b && imp && out, "dle_nnunet_head_blend_fwd: null operand");
  DLE_CHECK_ARG(K >= 1 && K <= NU_HEAD_MAXK, "dle_nnunet_head_blend_fwd: 1 <= K <= %d (got %d)", NU_HEAD_MAXK, K);
  DLE_CHECK_ARG(C >= 8 && C % 8 == 0 && C <= NU_HEAD_MAXC, "dle_nnunet_head_blend_fwd: C %% 8 == 0, C <= %d (got %d)", NU_HEAD_MAXC, C);
  DLE_CHECK_ARG(ldx >= C && ldx % 8 == 0, "dle_nnunet_head_blend_fwd: ldx %lld for %d channels", (long long)ldx, C);
  DLE_CHECK_ARG(Dp >= 1 && Hp >= 1 && Wp >= 1 && d0 >= 0 && h0 >= 0 && w0 >= 0 && (long long)d0 + Dp <= Dv && (long long)h0 + Hp <= Hv &&
                    (long long)w0 + Wp <= Wv,
                "dle_nnunet_head_blend_fwd: window [%d+%d, %d+%d, %d+%d] outside the volume [%d, %d, %d]", d0, Dp, h0, Hp, w0, Wp, Dv, Hv, Wv);
  DLE_CHECK_ARG(nu_aligned16(x) && nu_aligned16(w), "dle_nnunet_head_blend_fwd: x and w must be 16-byte aligned");
  const long long lim = 1ll << 31;
  DLE_CHECK_ARG((long long)Dp * Hp * Wp * ldx < lim && (long long)K * Dv * Hv * Wv < lim, "dle_nnunet_head_blend_fwd: a tensor has 2^31 elements or more");
  NuHeadArgs a;
  a.x = (const unsigned short*)x; a.w = (const unsigned short*)w; a.b = b; a.imp = imp; a.out = out; a.ldx = ldx;
  a.K = K; a.C = C; a.Dp = Dp; a.Hp = Hp; a.Wp = Wp; a.Dv = Dv; a.Hv = Hv; a.Wv = Wv; a.d0 = d0; a.h0 = h0; a.w0 = w0;
  const int vox = Dp * Hp * Wp;
  if (dtype == DLE_F16) hipLaunchKernelGGL(nu_head_blend_kernel<DLE_F16>, dim3((vox + 255) / 256), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(nu_head_blend_kernel<DLE_BF16>, dim3((vox + 255) / 256), dim3(256), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}
