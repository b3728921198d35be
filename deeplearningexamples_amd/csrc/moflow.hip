// MoFlow molecule generation on gfx950, the reverse flow (reference: PyTorch/DrugDiscovery/MoFlow/moflow/model/model.py:205-236,
// glow.py, coupling.py, basic.py).  Contracts and rounding points: include/dle_mi355x.h.
//
// dle_mf_couple_fwd replaces, per bond flow, the third Conv2d, chunk, exp, mul, sub, cat (coupling.py:86-100) and ActNorm.reverse
// (basic.py:92-93).  The squeezed image has at most nine positions, so the convolution is a dense product; a wavefront owns 32
// elements (q, c) of 32 samples and runs TWO accumulators over K, the s rows and the t rows of those elements, so that s and t of
// an element meet in one lane and the coupling inverse needs no exchange.  Operand order and lane layout: mfma32_rows.h; the paired
// K loop (one B fragment for two MFMAs) is this kernel's own walk.
// dle_mf_atom_reverse_fwd replaces the whole of GlowOnGraph.reverse (38 x ~25 launches at ZINC250k sizes): no dependency between
// samples, so a workgroup of eight wavefronts keeps the N x T states of 32 samples in LDS and walks the flows; only the weights move:
// they stream from L2 in MFMA fragment order (1 KB per wavefront request), eight fragments requested ahead of the MFMAs that use them.
// Measured: 1.4 ms for 38 flows at batch 512 against 25 - 29 ms for the reference's modules under autocast; the time
// is the chain's latency (six barriers and four exposed L2 round trips per flow), not arithmetic.
#include "mfma32_rows.h"
#include <math.h>

// channel c of position p of the squeezed image -> (edge type, row, column) of the [4][N][N] tensor (glow.py:152-179)
__device__ __forceinline__ void mf_unsqueeze(int c, int p, int G, int fold, int& e, int& i, int& j) {
  const int fx = c % fold, t = c / fold, fy = t % fold;
  e = t / fold;
  i = (p / G) * fold + fy;
  j = (p % G) * fold + fx;
}

// ---- dle_mf_squeeze_fwd ---------------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(256) void mf_squeeze_kernel(const float* __restrict__ z, long long ldz, float* __restrict__ state,
                                                         unsigned short* __restrict__ img, long long total, int N, int fold,
                                                         int img_half) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int G = N / fold, C = 4 * fold * fold, PC = G * G * C, Ch = C / 2;
  const long long b = idx / PC;
  const int q = (int)(idx % PC), p = q / C, c = q % C;
  int e, i, j;
  mf_unsqueeze(c, p, G, fold, e, i, j);
  const float v = z[b * ldz + ((long long)e * N + i) * N + j];
  state[idx] = v;
  if (img && c / Ch == img_half) img[b * (PC / 2) + p * Ch + (c - img_half * Ch)] = Elem<DT>::from_f32(v);
}

extern "C" int dle_mf_squeeze_fwd(const float* z_adj, int64_t ldz, float* state, void* img, int B, int N, int fold, int img_half,
                                  int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "mf_squeeze_fwd: the image is 16-bit");
  DLE_CHECK_ARG(z_adj && state, "mf_squeeze_fwd: null pointer");
  DLE_CHECK_ARG(B >= 0 && N >= 1 && N <= 1024 && fold >= 1 && N % fold == 0, "mf_squeeze_fwd: bad sizes (B %d, N %d, fold %d)", B, N, fold);
  DLE_CHECK_ARG(img_half == 0 || img_half == 1, "mf_squeeze_fwd: img_half is 0 or 1");
  DLE_CHECK_ARG(ldz >= 4LL * N * N, "mf_squeeze_fwd: row pitch below 4 N N");
  const long long total = 4LL * N * N * B;
  DLE_CHECK_ARG(total < 0x7FFFFFFFLL, "mf_squeeze_fwd: tensor too large");
  if (total == 0) return 0;
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == DLE_F16)
    hipLaunchKernelGGL(mf_squeeze_kernel<DLE_F16>, grid, dim3(256), 0, stream, z_adj, (long long)ldz, state, (unsigned short*)img, total, N, fold, img_half);
  else
    hipLaunchKernelGGL(mf_squeeze_kernel<DLE_BF16>, grid, dim3(256), 0, stream, z_adj, (long long)ldz, state, (unsigned short*)img, total, N, fold, img_half);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_mf_couple_fwd ----------------------------------------------------------------------------------------------------------
struct MfCoupleArgs {
  const unsigned short *h2, *w3;
  const float *b3, *scale, *loc, *sin;
  float* sout;
  unsigned short* img;
  long long ldh;
  int B, P, Ch, K, swap, img_half;
};

template <int DT>
__global__ __launch_bounds__(256) void mf_couple_kernel(MfCoupleArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hf = lane >> 5, row = lane & 31;
  const int M = p.P * p.Ch, blk = blockIdx.x;
  const long long tile = (long long)blockIdx.y * 4 + wave;
  if (tile * 32 >= p.B) return;                        // (wavefront-uniform; the kernel has no barrier)
  const long long smp = tile * 32 + row;
  const long long srd = smp < p.B ? smp : p.B - 1;     // lanes behind the batch read the last row and store nothing
  const unsigned short* xr = p.h2 + srd * p.ldh + hf * 8;
  const unsigned short* ws = p.w3 + (long long)(blk * 32 + row) * p.K + hf * 8;
  const unsigned short* wt = ws + (long long)M * p.K;
  float16_t as, at;
#pragma unroll
  for (int r = 0; r < 16; ++r) as[r] = at[r] = 0.f;
#pragma unroll 4
  for (int ks = 0; ks < p.K; ks += 16) {
    const ushort8_t x = *(const ushort8_t*)(xr + ks);
    as = Mfma32x16<DT>::run(*(const ushort8_t*)(ws + ks), x, as);
    at = Mfma32x16<DT>::run(*(const ushort8_t*)(wt + ks), x, at);
  }
  if (smp >= p.B) return;
  const int boff = p.swap ? 0 : p.Ch, aoff = p.swap ? p.Ch : 0, bhalf = p.swap ? 0 : 1;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int j0 = blk * 32 + 8 * g + 4 * hf, pos = j0 / p.Ch, c0 = j0 % p.Ch;
    const long long base = smp * (2LL * M) + (long long)pos * (2 * p.Ch) + c0;
    const float4_t bs = *(const float4_t*)(p.b3 + j0), bt = *(const float4_t*)(p.b3 + M + j0);
    const float4_t ob = *(const float4_t*)(p.sin + base + boff), oa = *(const float4_t*)(p.sin + base + aoff);
    const float4_t scb = *(const float4_t*)(p.scale + boff + c0), lcb = *(const float4_t*)(p.loc + boff + c0);
    const float4_t sca = *(const float4_t*)(p.scale + aoff + c0), lca = *(const float4_t*)(p.loc + aoff + c0);
    float4_t nb, na;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float s = __fadd_rn(as[4 * g + i], bs[i]), t = __fadd_rn(at[4 * g + i], bt[i]);
      const float inb = __fsub_rn(__fmul_rn(ob[i], __fadd_rn(1.f, expf(-s))), t);
      nb[i] = __fsub_rn(__fdiv_rn(inb, scb[i]), lcb[i]);
      na[i] = __fsub_rn(__fdiv_rn(oa[i], sca[i]), lca[i]);
    }
    *(float4_t*)(p.sout + base + boff) = nb;
    *(float4_t*)(p.sout + base + aoff) = na;
    if (p.img) {
      const float4_t v = p.img_half == bhalf ? nb : na;
      *(uint2_t*)(p.img + smp * M + j0) = rt_pack4<DT>(v[0], v[1], v[2], v[3]);
    }
  }
}

extern "C" int dle_mf_couple_fwd(const void* h2, int64_t ldh, const void* w3, const float* b3, const float* scale, const float* loc,
                                 const float* state_in, float* state_out, void* img, int B, int P, int half_channels, int K,
                                 int mask_swap, int img_half, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "mf_couple_fwd: 16-bit operands only");
  DLE_CHECK_ARG(h2 && w3 && b3 && scale && loc && state_in && state_out, "mf_couple_fwd: null pointer");
  DLE_CHECK_ARG(B >= 0 && P >= 1 && P <= 9 && half_channels >= 4 && K >= 16, "mf_couple_fwd: bad sizes (B %d, P %d, C/2 %d, K %d)", B, P,
                half_channels, K);
  DLE_CHECK_ARG(half_channels % 4 == 0 && ((long long)P * half_channels) % 32 == 0 && K % 16 == 0 && (long long)P * half_channels < (1 << 24),
                "mf_couple_fwd: built for C/2 %% 4 == 0, P C/2 %% 32 == 0, K %% 16 == 0 (got C/2 %d, P %d, K %d)", half_channels, P, K);
  DLE_CHECK_ARG(ldh >= K && ldh % 8 == 0, "mf_couple_fwd: the pitch of h2 must be a multiple of 8 and at least K");
  DLE_CHECK_ARG(mask_swap == 0 || mask_swap == 1, "mf_couple_fwd: mask_swap is 0 or 1");
  DLE_CHECK_ARG(!img || img_half == 0 || img_half == 1, "mf_couple_fwd: img_half is 0 or 1");
  DLE_CHECK_ARG(dle_aligned<16>(h2, w3, b3, scale, loc, state_in, state_out) && dle_aligned<8>(img), "mf_couple_fwd: misaligned tensor");
  const int M = P * half_channels;
  DLE_CHECK_ARG((long long)B * 2 * M < 0x7FFFFFFFLL * 4, "mf_couple_fwd: tensor too large");
  if (B == 0) return 0;
  const long long tiles = ((long long)B + 31) / 32, gy = (tiles + 3) / 4;
  DLE_CHECK_ARG(gy <= 65535, "mf_couple_fwd: batch too large");
  MfCoupleArgs a;
  a.h2 = (const unsigned short*)h2; a.w3 = (const unsigned short*)w3; a.b3 = b3; a.scale = scale; a.loc = loc; a.sin = state_in;
  a.sout = state_out; a.img = (unsigned short*)img; a.ldh = ldh; a.B = B; a.P = P; a.Ch = half_channels; a.K = K; a.swap = mask_swap;
  a.img_half = img_half;
  const dim3 grid((unsigned)(M / 32), (unsigned)gy);
  if (dtype == DLE_F16) hipLaunchKernelGGL(mf_couple_kernel<DLE_F16>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(mf_couple_kernel<DLE_BF16>, grid, dim3(256), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_mf_bond_decide_fwd -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mf_bond_decide_kernel(const float* __restrict__ state, uint8_t* __restrict__ mask,
                                                             uint8_t* __restrict__ code, float* __restrict__ adj01,
                                                             float* __restrict__ hadj, long long total, int N, int fold, int unshift) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int G = N / fold, C = 4 * fold * fold, NN = N * N;
  const long long b = idx / NN;
  const int ij = (int)(idx % NN), i = ij / N, j = ij % N;
  const int pij = (i / fold) * G + j / fold, pji = (j / fold) * G + i / fold;
  const float* sb = state + b * ((long long)G * G * C);
  float v[4], raw[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float a = sb[pij * C + (e * fold + i % fold) * fold + j % fold];
    float t = sb[pji * C + (e * fold + j % fold) * fold + i % fold];
    raw[e] = a;
    if (unshift) {
      a = __fmul_rn(__fadd_rn(a, 0.5f), 2.f);
      t = __fmul_rn(__fadd_rn(t, 0.5f), 2.f);
    }
    v[e] = __fdiv_rn(__fadd_rn(a, t), 2.f);
  }
  const float m = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
  unsigned bits = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) bits |= (v[e] == m ? 1u : 0u) << e;
  mask[idx] = (uint8_t)bits;
  code[idx] = (uint8_t)(bits ? __builtin_ctz(bits) : 0);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const long long o = (b * 4 + e) * NN + ij;
    if (adj01) adj01[o] = (bits >> e) & 1u ? 1.f : 0.f;
    if (hadj) hadj[o] = raw[e];
  }
}

extern "C" int dle_mf_bond_decide_fwd(const float* state, uint8_t* mask, uint8_t* code, float* adj01, float* h_adj, int B, int N,
                                      int fold, int unshift, hipStream_t stream) {
  DLE_CHECK_ARG(state && mask && code, "mf_bond_decide_fwd: null pointer");
  DLE_CHECK_ARG(B >= 0 && N >= 1 && N <= 1024 && fold >= 1 && N % fold == 0, "mf_bond_decide_fwd: bad sizes (B %d, N %d, fold %d)", B, N, fold);
  DLE_CHECK_ARG(dle_aligned<4>(state, adj01, h_adj), "mf_bond_decide_fwd: misaligned tensor");
  const long long total = (long long)B * N * N;
  DLE_CHECK_ARG(total * 4 < 0x7FFFFFFFLL, "mf_bond_decide_fwd: tensor too large");
  if (total == 0) return 0;
  hipLaunchKernelGGL(mf_bond_decide_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, state, mask, code, adj01, h_adj,
                     total, N, fold, unshift);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_mf_atom_reverse_fwd ----------------------------------------------------------------------------------------------------
#define MF_R 32                      // samples per tile
#define MF_THREADS 512                // eight wavefronts: twice the weight loads in flight of four, half the elementwise trip counts
#define MF_CHUNK 8                    // weight fragments of one request group (8 KB per wavefront)
#define MF_MROW 64                   // bytes per sample of the adjacency row image (N <= 64)
#define MF_STLD 33                   // floats per sample of the s | t image
#define MF_LDS_MAX (160 * 1024)

struct MfAtomArgs {
  const float* z;
  const unsigned char* mask;
  const unsigned short* w;
  const float* p32;
  float* x;
  long long ldz, wstride, pstride;
  int B, N, T, KG, D1, D2, D3, nflow, rstride, unshift;
};

struct MfAtomLds { int ys, st, mrow, imga, imgb, lda, ldb, nt1, bytes; };

static inline int mf_up(int v, int m) { return (v + m - 1) / m * m; }

static MfAtomLds mf_atom_lds(int N, int T, int KG, int D1, int D2, int D3) {
  MfAtomLds l;
  l.nt1 = (N * T) | 1;                               // odd pitch: the 32 samples of a wavefront start in 32 different banks
  l.lda = (KG > D2 ? KG : D2) + 8;
  l.ldb = (D1 > D3 ? D1 : D3) + 8;
  l.ys = 0;
  l.st = mf_up(l.ys + MF_R * l.nt1 * 4, 16);
  l.mrow = mf_up(l.st + MF_R * MF_STLD * 4, 16);
  l.imga = mf_up(l.mrow + MF_R * MF_MROW, 16);
  l.imgb = mf_up(l.imga + MF_R * l.lda * 2, 16);
  l.bytes = mf_up(l.imgb + MF_R * l.ldb * 2, 16);
  return l;
}

// out[sample][32 blk + f] = round16(relu(W x + b)) for the wavefront's feature blocks; W in fragment order [blk][ks][lane][8]
template <int DT>
__device__ __forceinline__ void mf_layer(const unsigned short* __restrict__ W, int K, int nblk, const unsigned short* X, int ldx,
                                         const float* __restrict__ bias, unsigned short* out, int ldo, int wave, int lane) {
  const int hf = lane >> 5, row = lane & 31, nks = K >> 4;
  for (int blk = wave; blk < nblk; blk += MF_THREADS / 64) {
    float16_t acc = rt_load16(bias, 32 * blk, hf);
    // the block's fragments arrive in groups of MF_CHUNK, the next group requested before the current one's MFMAs: the weights come
    // from L2 with a latency of microseconds, and a wavefront that waits for each load streams a few GB/s
    const ushort8_t* wp = (const ushort8_t*)W + (long long)blk * nks * 64 + lane;
    const unsigned short* xp = X + row * ldx + hf * 8;
    ushort8_t cur[MF_CHUNK] = {}, nxt[MF_CHUNK] = {};
#pragma unroll
    for (int u = 0; u < MF_CHUNK; ++u)
      if (u < nks) cur[u] = wp[u * 64];
    for (int c = 0; c < nks; c += MF_CHUNK) {
#pragma unroll
      for (int u = 0; u < MF_CHUNK; ++u)
        if (c + MF_CHUNK + u < nks) nxt[u] = wp[(c + MF_CHUNK + u) * 64];
#pragma unroll
      for (int u = 0; u < MF_CHUNK; ++u)
        if (c + u < nks) acc = Mfma32x16<DT>::run(cur[u], *(const ushort8_t*)(xp + (c + u) * 16), acc);
#pragma unroll
      for (int u = 0; u < MF_CHUNK; ++u) cur[u] = nxt[u];
    }
    rt_store16<DT, true>(out + row * ldo, 32 * blk, hf, acc);
  }
}

template <int DT>
__global__ __launch_bounds__(MF_THREADS) void mf_atom_kernel(MfAtomArgs p, MfAtomLds l) {
  extern __shared__ __attribute__((aligned(16))) unsigned char mf_lds[];
  float* ys = (float*)(mf_lds + l.ys);
  float* st = (float*)(mf_lds + l.st);
  unsigned char* mrow = mf_lds + l.mrow;
  unsigned short* imga = (unsigned short*)(mf_lds + l.imga);
  unsigned short* imgb = (unsigned short*)(mf_lds + l.imgb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, row = lane & 31;
  const int N = p.N, T = p.T, NT = N * T;
  const long long ntiles = ((long long)p.B + MF_R - 1) / MF_R;
  const long long wg = (long long)p.D1 * p.KG, w1 = (long long)p.D2 * p.D1, w2 = (long long)p.D3 * p.D2;

  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long s0 = tile * MF_R;
    __syncthreads();                                   // the previous tile's stores have read ys
    for (int idx = tid; idx < MF_R * NT; idx += MF_THREADS) {
      const int s = idx / NT, k = idx % NT;
      ys[s * l.nt1 + k] = s0 + s < p.B ? p.z[(s0 + s) * p.ldz + k] : 0.f;
    }
    for (int i = p.nflow - 1; i >= 0; --i) {
      const int r = (int)(((long long)i * p.rstride) % N);
      const unsigned short* W = p.w + (long long)i * p.wstride;
      const float* P32 = p.p32 + (long long)i * p.pstride;
      const float *bg = P32, *b1 = bg + p.D1, *b2 = b1 + p.D2, *b3 = b2 + p.D3, *scale = b3 + 32, *loc = scale + N;
      // row r of the samples' adjacency bit masks (samples behind the batch: no bond)
      for (int idx = tid; idx < MF_R * N; idx += MF_THREADS) {
        const int s = idx / N, n = idx % N;
        mrow[s * MF_MROW + n] = s0 + s < p.B ? p.mask[((s0 + s) * N + r) * N + n] : (unsigned char)0;
      }
      __syncthreads();                                 // and the previous flow's ys
      // g = [sum over n != r of bit_e(n) y[n,t] | deg_e | 0], fp32 in ascending n, one rounding
      {
        const int s = tid & 31;
        const float* y = ys + s * l.nt1;
        const unsigned char* mr = mrow + s * MF_MROW;
        for (int q = tid >> 5; q < p.KG; q += MF_THREADS / 32) {
          float v = 0.f;
          if (q < 4 * T) {
            const int e = q / T, t = q % T;
            for (int n = 0; n < N; ++n)
              if (n != r && ((mr[n] >> e) & 1)) v = __fadd_rn(v, y[n * T + t]);
          } else if (q < 4 * T + 4) {
            const int e = q - 4 * T;
            for (int n = 0; n < N; ++n) v += (float)((mr[n] >> e) & 1);
          }
          imga[s * l.lda + q] = Elem<DT>::from_f32(v);
        }
      }
      __syncthreads();
      mf_layer<DT>(W, p.KG, p.D1 >> 5, imga, l.lda, bg, imgb, l.ldb, wave, lane);
      __syncthreads();
      mf_layer<DT>(W + wg, p.D1, p.D2 >> 5, imgb, l.ldb, b1, imga, l.lda, wave, lane);
      __syncthreads();
      mf_layer<DT>(W + wg + w1, p.D2, p.D3 >> 5, imga, l.lda, b2, imgb, l.ldb, wave, lane);
      __syncthreads();
      if (wave == 0) {                                 // the last linear: rows 0.. = s, 16.. = t, fp32, not rounded
        const float16_t acc = rt_mma<DT>(W + wg + w1 + w2 + lane * 8, 512, imgb + row * l.ldb + hf * 8, p.D3 >> 4, rt_load16(b3, 0, hf));
#pragma unroll
        for (int q = 0; q < 16; ++q) st[row * MF_STLD + rt_feat(q, hf)] = acc[q];
      }
      __syncthreads();
      // the coupling inverse on row r, ActNorm's inverse on all rows
      for (int idx = tid; idx < MF_R * NT; idx += MF_THREADS) {
        const int s = idx / NT, k = idx % NT, n = k / T, t = k % T;
        float v = ys[s * l.nt1 + k];
        if (n == r) v = __fsub_rn(__fmul_rn(v, __fadd_rn(1.f, expf(-st[s * MF_STLD + t]))), st[s * MF_STLD + 16 + t]);
        ys[s * l.nt1 + k] = __fsub_rn(__fdiv_rn(v, scale[n]), loc[n]);
      }
    }
    __syncthreads();
    for (int idx = tid; idx < MF_R * NT; idx += MF_THREADS) {
      const int s = idx / NT, k = idx % NT;
      if (s0 + s < p.B) {
        const float v = ys[s * l.nt1 + k];
        p.x[(s0 + s) * NT + k] = p.unshift ? __fmul_rn(__fadd_rn(v, 0.5f), 2.f) : v;
      }
    }
  }
}

extern "C" int dle_mf_atom_supported(int N, int T, int n_block, int n_gnn, int gnn0, int n_lin, int lin0, int lin1, int n_flow,
                                     int mask_row_size) {
  if (n_block != 1 || n_gnn != 1 || n_lin != 2 || mask_row_size != 1 || n_flow < 1) return 0;
  if (N < 2 || N > 64 || T < 1 || T > 16) return 0;
  if (gnn0 < 1 || gnn0 > 512 || lin0 < 1 || lin0 > 512 || lin1 < 1 || lin1 > 512) return 0;
  const MfAtomLds l = mf_atom_lds(N, T, mf_up(4 * T + 4, 16), mf_up(gnn0, 32), mf_up(lin0, 32), mf_up(lin1, 32));
  return l.bytes <= MF_LDS_MAX ? 1 : 0;
}

extern "C" int dle_mf_atom_reverse_fwd(const float* z_x, int64_t ldz, const uint8_t* mask, const void* w16, int64_t w_stride,
                                       const float* p32, int64_t p_stride, float* x, int B, int N, int T, int gnn0, int lin0, int lin1,
                                       int n_flow, int row_stride, int unshift, int tile, int max_workgroups, int dtype,
                                       hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "mf_atom_reverse_fwd: 16-bit weights only");
  DLE_CHECK_ARG(dle_mf_atom_supported(N, T, 1, 1, gnn0, 2, lin0, lin1, n_flow, 1),
                "mf_atom_reverse_fwd: outside the envelope (N %d, T %d, gnn %d, lin %d %d, %d flows)", N, T, gnn0, lin0, lin1, n_flow);
  DLE_CHECK_ARG(tile == MF_R, "mf_atom_reverse_fwd: built for tiles of 32 samples (got %d)", tile);
  DLE_CHECK_ARG(z_x && mask && w16 && p32 && x, "mf_atom_reverse_fwd: null pointer");
  DLE_CHECK_ARG(B >= 0 && row_stride >= 0 && ldz >= (long long)N * T, "mf_atom_reverse_fwd: bad batch, row stride or pitch");
  DLE_CHECK_ARG(max_workgroups >= 0, "mf_atom_reverse_fwd: max_workgroups must be 0 (the device's CU count) or positive");
  MfAtomArgs a;
  a.KG = mf_up(4 * T + 4, 16); a.D1 = mf_up(gnn0, 32); a.D2 = mf_up(lin0, 32); a.D3 = mf_up(lin1, 32);
  const long long wneed = (long long)a.D1 * a.KG + (long long)a.D2 * a.D1 + (long long)a.D3 * a.D2 + 32LL * a.D3;
  const long long pneed = a.D1 + a.D2 + a.D3 + 32 + 2 * N;
  DLE_CHECK_ARG(w_stride >= wneed && w_stride % 8 == 0 && p_stride >= pneed && p_stride % 4 == 0,
                "mf_atom_reverse_fwd: a flow needs %lld weights (pitch a multiple of 8) and %lld fp32 values (pitch a multiple of 4)", wneed, pneed);
  DLE_CHECK_ARG(dle_aligned<16>(w16, p32) && dle_aligned<4>(z_x, x), "mf_atom_reverse_fwd: misaligned tensor");
  if (B == 0) return 0;
  const DleDeviceLimits* lim = dle_device_limits();
  DLE_CHECK_ARG(lim != nullptr, "mf_atom_reverse_fwd: no usable device");
  const MfAtomLds l = mf_atom_lds(N, T, a.KG, a.D1, a.D2, a.D3);
  DLE_CHECK_ARG(lim->lds_per_block >= l.bytes, "mf_atom_reverse_fwd: the device offers %d bytes of LDS per workgroup, %d needed",
                lim->lds_per_block, l.bytes);
  a.z = z_x; a.mask = mask; a.w = (const unsigned short*)w16; a.p32 = p32; a.x = x; a.ldz = ldz; a.wstride = w_stride; a.pstride = p_stride;
  a.B = B; a.N = N; a.T = T; a.nflow = n_flow; a.rstride = row_stride; a.unshift = unshift;
  const long long grid = rt_persistent_grid(((long long)B + MF_R - 1) / MF_R, max_workgroups, lim);
  if (dtype == DLE_F16) DLE_LAUNCH_LDS((mf_atom_kernel<DLE_F16>), dim3((unsigned)grid), dim3(MF_THREADS), l.bytes, stream, a, l);
  else DLE_LAUNCH_LDS((mf_atom_kernel<DLE_BF16>), dim3((unsigned)grid), dim3(MF_THREADS), l.bytes, stream, a, l);
  DLE_LAUNCH_CHECK();
  return 0;
}
