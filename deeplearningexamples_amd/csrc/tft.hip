// Temporal Fusion Transformer inference on gfx950 (reference: PyTorch/Forecasting/TFT/modeling.py): the gated residual network,
// the variable selection network, a whole LSTM layer and the interpretable attention of the decoder positions, one launch each.
//
// Hidden size 128 everywhere.  Every linear layer of the model is a [128 or 256][128] matrix against a tile of 32 rows, and all of
// them share one building block: out^T = W X^T in the operand order and lane layout of mfma32_rows.h.  The weight rows come
// straight from global memory (16 bytes per lane and k step; the matrices, 32 - 64 KB each, stay in L2), the 32 rows of the tile
// out of a [32][136] LDS image.  A lane holds 16 features of ONE row, so the a and b halves of a GLU sit in the same lane, and a
// LayerNorm is 16 registers, one lane exchange and one exchange through LDS between the four wavefronts.  Intermediates never
// leave the compute unit.  The biases are read element by element (rt_load16s): the entry points ask fp32 vectors for 4-byte
// alignment only.
#include "mfma32_rows.h"

#define TF_H 128
#define TF_R 32                      // rows per workgroup
#define TF_LD 136                    // halves per line of a row image: 272 bytes, so the 32 lines start in 8 different bank groups
#define TF_IMG (TF_R * TF_LD)
#define TF_MAXF 8                    // variables per selection network
#define TF_MAXQ 8                    // quantiles of the tail
#define TF_MAXT 192                  // time steps of the attention (6 key tiles held in registers)
#define TF_VLD 40                    // halves per V line in LDS

// acc += W[n0 + 0..31][0..127] . X[0..31][0..127]^T; W is row-major with 128 columns, X an LDS row image
template <int DT>
__device__ __forceinline__ float16_t tf_block(const unsigned short* __restrict__ W, int n0, const unsigned short* X, int lane, float16_t acc) {
  return rt_mma<DT>(W + (n0 + (lane & 31)) * TF_H + (lane >> 5) * 8, 16, X + (lane & 31) * TF_LD + (lane >> 5) * 8, TF_H / 16, acc);
}

__device__ __forceinline__ float tf_elu(float v) { return v > 0.f ? v : expm1f(v); }
__device__ __forceinline__ float tf_sigmoid(float v) { return 1.f / (1.f + __expf(-v)); }

// 32 rows of 128 halves from global memory into an LDS row image; row(i) gives the source row pointer of tile row i or nullptr
template <class RowFn>
__device__ __forceinline__ void tf_load_img(unsigned short* X, int tid, RowFn row) {
  const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = tid + it * 256, r = c >> 4, c8 = c & 15;
    const unsigned short* src = row(r);
    *(ushort8_t*)(X + r * TF_LD + c8 * 8) = src ? *(const ushort8_t*)(src + c8 * 8) : zero8;
  }
}

// GLU linear (256 outputs) on the image G, a * sigmoid(b), + res, LayerNorm over the 128 features -> outv (fp32, this lane's 16
// features of its row).  Every thread of the workgroup calls it; red is [2][4][32] floats.
template <int DT>
__device__ __forceinline__ void tf_glu_ln(const unsigned short* G, const unsigned short* __restrict__ wg, const float* __restrict__ bg,
                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float* red,
                                          int wave, int lane, const float* res, float* outv) {
  const int hf = lane >> 5, row = lane & 31, n0 = wave * 32;
  float16_t a, b;
#pragma unroll
  for (int r = 0; r < 16; ++r) {                      // (interleaved: as two rt_load16s calls tft_grn_kernel takes 13 more VGPRs)
    a[r] = bg[n0 + rt_feat(r, hf)];
    b[r] = bg[TF_H + n0 + rt_feat(r, hf)];
  }
  a = tf_block<DT>(wg, n0, G, lane, a);
  b = tf_block<DT>(wg, TF_H + n0, G, lane, b);
  float y[16], s = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    y[r] = a[r] * tf_sigmoid(b[r]) + res[r];
    s += y[r];
  }
  s += __shfl_xor(s, 32, 64);
  if (hf == 0) red[wave * TF_R + row] = s;
  __syncthreads();
  const float mean = (red[row] + red[TF_R + row] + red[2 * TF_R + row] + red[3 * TF_R + row]) * (1.f / TF_H);
  float s2 = 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    y[r] -= mean;
    s2 += y[r] * y[r];
  }
  s2 += __shfl_xor(s2, 32, 64);
  if (hf == 0) red[4 * TF_R + wave * TF_R + row] = s2;
  __syncthreads();
  const float var = (red[4 * TF_R + row] + red[5 * TF_R + row] + red[6 * TF_R + row] + red[7 * TF_R + row]) * (1.f / TF_H);
  const float rstd = 1.f / sqrtf(var + eps);
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + rt_feat(r, hf);
    outv[r] = y[r] * rstd * gamma[n] + beta[n];
  }
}

// ---- dle_tft_grn_fwd: GRN.forward (modeling.py:48-77); gate mode: GLU + residual + LayerNorm (:403-405, 418-420, 426-428); the
// tail is quantile_proj (:430) -------------------------------------------------------------------------------------------------
struct TftGrnArgs {
  const unsigned short* x; long long ldx; const int* xidx; long long n_xrows;
  const unsigned short* ctx; long long ldc, rows_per_ctx;
  const unsigned short* res; long long ldr, res_rpb, res_bs;
  const unsigned short *wa, *wc, *wi, *wg;
  const float *ba, *bi, *bg, *gamma, *beta;
  unsigned short* out; long long ldo;
  const float *wq, *bq; float* qout; int nq;
  long long rows; float eps;
};

template <int DT>
__global__ __launch_bounds__(256) void tft_grn_kernel(TftGrnArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned short Xs[TF_IMG], Cs[TF_IMG], Hs[TF_IMG], Gs[TF_IMG];
  __shared__ float red[8 * TF_R];
  __shared__ float qs[4 * TF_R * TF_MAXQ];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, row = lane & 31, n0 = wave * 32;
  const long long row0 = (long long)blockIdx.x * TF_R;
  const bool gate = p.wa == nullptr;
  auto xrow = [&](int i) -> const unsigned short* {
    const long long r = row0 + i;
    if (r >= p.rows) return nullptr;
    if (!p.xidx) return p.x + r * p.ldx;
    const long long s = p.xidx[r];
    return (s >= 0 && s < p.n_xrows) ? p.x + s * p.ldx : nullptr;
  };
  if (gate) {
    // the GLU input is x; the residual is a second tensor, addressed per (batch element, step) when res_rpb is given
    tf_load_img(Gs, tid, xrow);
    tf_load_img(Xs, tid, [&](int i) -> const unsigned short* {
      const long long r = row0 + i;
      if (r >= p.rows) return nullptr;
      return p.res_rpb ? p.res + (r / p.res_rpb) * p.res_bs + (r % p.res_rpb) * p.ldr : p.res + r * p.ldr;
    });
    __syncthreads();
  } else {
    tf_load_img(Xs, tid, xrow);
    if (p.ctx)
      tf_load_img(Cs, tid, [&](int i) -> const unsigned short* {
        const long long r = row0 + i;
        return r < p.rows ? p.ctx + (r / p.rows_per_ctx) * p.ldc : nullptr;
      });
    __syncthreads();
    float16_t acc = tf_block<DT>(p.wa, n0, Xs, lane, rt_load16s(p.ba, n0, hf));
    float v[16];
    if (p.ctx) acc = tf_block<DT>(p.wc, n0, Cs, lane, acc);
#pragma unroll
    for (int r = 0; r < 16; ++r) v[r] = tf_elu(acc[r]);
    rt_store16<DT, false>(Hs + row * TF_LD, n0, hf, v);
    __syncthreads();
    acc = tf_block<DT>(p.wi, n0, Hs, lane, rt_load16s(p.bi, n0, hf));
    rt_store16<DT, false>(Gs + row * TF_LD, n0, hf, acc);
    __syncthreads();
  }
  float res[16], outv[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) res[r] = Elem<DT>::to_f32(Xs[row * TF_LD + n0 + rt_feat(r, hf)]);
  tf_glu_ln<DT>(Gs, p.wg, p.bg, p.gamma, p.beta, p.eps, red, wave, lane, res, outv);
  const bool ok = row0 + row < p.rows;
  if (ok && p.out) rt_store16<DT, false>(p.out + (row0 + row) * p.ldo, n0, hf, outv);
  if (p.qout) {
    for (int q = 0; q < p.nq; ++q) {
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) s += outv[r] * p.wq[q * TF_H + n0 + rt_feat(r, hf)];
      s += __shfl_xor(s, 32, 64);
      if (hf == 0) qs[(wave * TF_R + row) * TF_MAXQ + q] = s;
    }
    __syncthreads();
    if (tid < TF_R * TF_MAXQ) {
      const int r = tid / TF_MAXQ, q = tid % TF_MAXQ;
      if (q < p.nq && row0 + r < p.rows) {
        float s = p.bq[q];
#pragma unroll
        for (int w = 0; w < 4; ++w) s += qs[(w * TF_R + r) * TF_MAXQ + q];
        p.qout[(row0 + r) * p.nq + q] = s;
      }
    }
  }
}

extern "C" int dle_tft_grn_fwd(const void* x, int64_t ldx, const int32_t* x_index, int64_t n_x_rows, const void* ctx, int64_t ldc,
                               int64_t rows_per_ctx, const void* res, int64_t ldr, int64_t res_rows_per_batch,
                               int64_t res_batch_stride, const void* wa, const float* ba, const void* wc, const void* wi,
                               const float* bi, const void* wg, const float* bg, const float* gamma, const float* beta, float eps,
                               void* out, int64_t ldo, const float* wq, const float* bq, float* qout, int nq, int64_t rows,
                               int hidden, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "tft_grn_fwd: 16-bit operands only");
  DLE_CHECK_ARG(hidden == TF_H, "tft_grn_fwd: built for hidden size 128 (got %d)", hidden);
  DLE_CHECK_ARG(rows >= 0 && (rows + TF_R - 1) / TF_R < 0x7FFFFFFFLL, "tft_grn_fwd: bad row count");
  DLE_CHECK_ARG(x && wg && bg && gamma && beta, "tft_grn_fwd: null pointer");
  DLE_CHECK_ARG(out || qout, "tft_grn_fwd: neither an output nor a quantile output");
  DLE_CHECK_ARG(ldx >= TF_H && (ldx & 7) == 0, "tft_grn_fwd: ldx must be a multiple of 8, at least 128");
  DLE_CHECK_ARG(!out || (ldo >= TF_H && (ldo & 7) == 0), "tft_grn_fwd: ldo must be a multiple of 8, at least 128");
  DLE_CHECK_ARG(!x_index || n_x_rows > 0, "tft_grn_fwd: a row index list needs the number of source rows");
  const bool gate = wa == nullptr;
  if (gate) {
    DLE_CHECK_ARG(!wi && !wc && !ctx && !ba && !bi, "tft_grn_fwd: gate mode (wa NULL) takes no lin_a / lin_i / lin_c operands");
    DLE_CHECK_ARG(res, "tft_grn_fwd: gate mode needs the residual tensor");
    DLE_CHECK_ARG(ldr >= TF_H && (ldr & 7) == 0, "tft_grn_fwd: ldr must be a multiple of 8, at least 128");
    DLE_CHECK_ARG(res_rows_per_batch >= 0 && (res_rows_per_batch == 0 || (res_batch_stride >= res_rows_per_batch * ldr &&
                                                                          (res_batch_stride & 7) == 0)),
                  "tft_grn_fwd: the residual's batch stride must be a multiple of 8, at least rows_per_batch * ldr");
  } else {
    DLE_CHECK_ARG(wi && ba && bi, "tft_grn_fwd: null pointer");
    DLE_CHECK_ARG(!res, "tft_grn_fwd: the residual of the full network is its input");
    DLE_CHECK_ARG((ctx == nullptr) == (wc == nullptr), "tft_grn_fwd: context and lin_c go together");
    DLE_CHECK_ARG(!ctx || (ldc >= TF_H && (ldc & 7) == 0 && rows_per_ctx >= 1),
                  "tft_grn_fwd: ldc must be a multiple of 8, at least 128, and rows_per_ctx >= 1");
  }
  DLE_CHECK_ARG(!qout || (wq && bq && nq >= 1 && nq <= TF_MAXQ), "tft_grn_fwd: the quantile tail needs wq, bq and 1 <= nq <= 8");
  DLE_CHECK_ARG(dle_aligned<16>(x, ctx, res, wa, wc, wi, wg, out), "tft_grn_fwd: tensors must be 16-byte aligned");
  if (rows == 0) return 0;
  TftGrnArgs a = {};
  a.x = (const unsigned short*)x; a.ldx = ldx; a.xidx = x_index; a.n_xrows = n_x_rows;
  a.ctx = (const unsigned short*)ctx; a.ldc = ldc; a.rows_per_ctx = rows_per_ctx;
  a.res = (const unsigned short*)res; a.ldr = ldr; a.res_rpb = res_rows_per_batch; a.res_bs = res_batch_stride;
  a.wa = (const unsigned short*)wa; a.wc = (const unsigned short*)wc; a.wi = (const unsigned short*)wi; a.wg = (const unsigned short*)wg;
  a.ba = ba; a.bi = bi; a.bg = bg; a.gamma = gamma; a.beta = beta;
  a.out = (unsigned short*)out; a.ldo = ldo; a.wq = wq; a.bq = bq; a.qout = qout; a.nq = qout ? nq : 0; a.rows = rows; a.eps = eps;
  const dim3 grid((unsigned)((rows + TF_R - 1) / TF_R));
  if (dtype == DLE_F16) hipLaunchKernelGGL(tft_grn_kernel<DLE_F16>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(tft_grn_kernel<DLE_BF16>, grid, dim3(256), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_tft_vsn_fwd: TFTEmbedding._apply_embedding for continuous variables (modeling.py:162-189) and
// VariableSelectionNetwork.forward (:286-303) -------------------------------------------------------------------------------------
// The embedding of variable f is x_f a_f + b_f, so the first linear of every network is x_f (W a_f) + (W b_f + bias): the caller
// folds it (float64) and the kernel forms it with F fused multiply-adds per element.  Layouts of the two parameter blocks:
//   w16: [wc 128x128 (zeros without a context)] [joint lin_i 128x128] [joint GLU 32x128: row f = a part, row 8 + f = b part]
//        then per variable [lin_i 128x128] [GLU 256x128]
//   p32: ju [F][128], jv [128], joint lin_i bias [128], joint GLU bias [32] (padded like its weight), jo [F][8], jov [8],
//        joint LayerNorm gamma [8], beta [8]; then per variable vu, vv, a, b, lin_i bias [128 each], GLU bias [256], gamma, beta [128]
#define TF_W16_V (TF_H * TF_H + 2 * TF_H * TF_H)
#define TF_P32_V (5 * TF_H + 2 * TF_H + 2 * TF_H)

struct TftVsnArgs {
  const float* seg[3]; long long seg_ld[3]; int seg_n[3];
  long long tn, src_T, src_t0;
  const unsigned short* ctx; long long ldc;
  const unsigned short* w16; const float* p32;
  unsigned short* out; long long ldo, out_T, out_t0;
  float* wout;
  long long rows; int F; float eps;
};

template <int DT>
__global__ __launch_bounds__(256) void tft_vsn_kernel(TftVsnArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned short Cs[TF_IMG], Hs[TF_IMG], Gs[TF_IMG];
  __shared__ float red[8 * TF_R];
  __shared__ float xs[TF_R * TF_MAXF], wsel[TF_R * TF_MAXF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, row = lane & 31, n0 = wave * 32, F = p.F;
  const long long row0 = (long long)blockIdx.x * TF_R;
  {
    const int i = tid >> 3, f = tid & 7;
    const long long r = row0 + i;
    float v = 0.f;
    if (r < p.rows && f < F) {
      const long long srow = (r / p.tn) * p.src_T + p.src_t0 + r % p.tn;
      v = f < p.seg_n[0] ? p.seg[0][srow * p.seg_ld[0] + f]
        : f < p.seg_n[0] + p.seg_n[1] ? p.seg[1][srow * p.seg_ld[1] + f - p.seg_n[0]]
                                      : p.seg[2][srow * p.seg_ld[2] + f - p.seg_n[0] - p.seg_n[1]];
    }
    xs[i * TF_MAXF + f] = v;
  }
  if (p.ctx)
    tf_load_img(Cs, tid, [&](int i) -> const unsigned short* {
      const long long r = row0 + i;
      return r < p.rows ? p.ctx + (r / p.tn) * p.ldc : nullptr;
    });
  __syncthreads();

  const float* P = p.p32;
  const float *ju = P, *jv = ju + F * TF_H, *jbi = jv + TF_H, *jbg = jbi + TF_H, *jo = jbg + 32, *jov = jo + F * 8, *jgam = jov + 8,
              *jbet = jgam + 8, *pv = jbet + 8;
  const unsigned short *wc = p.w16, *jwi = wc + TF_H * TF_H, *jwg = jwi + TF_H * TF_H, *wv = jwg + 32 * TF_H;
  float16_t acc;
  float v[16];
  // joint network: first linear folded, + lin_c(context), ELU, lin_i
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int n = n0 + rt_feat(r, hf);
    float s = jv[n];
    for (int f = 0; f < F; ++f) s = fmaf(xs[row * TF_MAXF + f], ju[f * TF_H + n], s);
    acc[r] = s;
  }
  if (p.ctx) acc = tf_block<DT>(wc, n0, Cs, lane, acc);
#pragma unroll
  for (int r = 0; r < 16; ++r) v[r] = tf_elu(acc[r]);
  rt_store16<DT, false>(Hs + row * TF_LD, n0, hf, v);
  __syncthreads();
  acc = tf_block<DT>(jwi, n0, Hs, lane, rt_load16s(jbi, n0, hf));
  rt_store16<DT, false>(Gs + row * TF_LD, n0, hf, acc);
  __syncthreads();
  // joint GLU (2F outputs in one padded 32-row block; every wavefront computes it, so nothing is exchanged), the folded out_proj
  // residual, LayerNorm over F (Identity when F == 1, MaybeLayerNorm) and the softmax
  {
    acc = tf_block<DT>(jwg, 0, Gs, lane, rt_load16s(jbg, 0, hf));
    float g[TF_MAXF];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int f = 4 * hf + i;                    // registers 0..3: a of variable f, registers 4..7: b of variable f
      float resid = jov[f];
      for (int f2 = 0; f2 < F; ++f2) resid = fmaf(xs[row * TF_MAXF + f2], jo[f2 * 8 + f], resid);
      const float mine = acc[i] * tf_sigmoid(acc[4 + i]) + resid;
      const float other = __shfl_xor(mine, 32, 64);
      g[i] = hf ? other : mine;
      g[4 + i] = hf ? mine : other;
    }
    if (F > 1) {
      float s = 0.f;
#pragma unroll
      for (int f = 0; f < TF_MAXF; ++f) s += f < F ? g[f] : 0.f;
      const float mean = s / (float)F;
      float s2 = 0.f;
#pragma unroll
      for (int f = 0; f < TF_MAXF; ++f) s2 += f < F ? (g[f] - mean) * (g[f] - mean) : 0.f;
      const float rstd = 1.f / sqrtf(s2 / (float)F + p.eps);
#pragma unroll
      for (int f = 0; f < TF_MAXF; ++f) g[f] = (g[f] - mean) * rstd * jgam[f] + jbet[f];
    }
    float m = -INFINITY;
#pragma unroll
    for (int f = 0; f < TF_MAXF; ++f) m = f < F ? fmaxf(m, g[f]) : m;
    float sum = 0.f;
#pragma unroll
    for (int f = 0; f < TF_MAXF; ++f) {
      g[f] = f < F ? __expf(g[f] - m) : 0.f;
      sum += g[f];
    }
    const float inv = 1.f / sum;
    if (wave == 0 && hf == 0) {
#pragma unroll
      for (int f = 0; f < TF_MAXF; ++f) {
        wsel[row * TF_MAXF + f] = g[f] * inv;
        if (p.wout && f < F && row0 + row < p.rows) p.wout[(row0 + row) * F + f] = g[f] * inv;
      }
    }
  }
  // (wsel is read after the first barrier of the loop below)
  float o[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  for (int f = 0; f < F; ++f) {
    const float* q = pv + (long long)f * TF_P32_V;
    const float *vu = q, *vv = vu + TF_H, *va = vv + TF_H, *vb = va + TF_H, *bi = vb + TF_H, *bg = bi + TF_H, *gam = bg + 2 * TF_H,
                *bet = gam + TF_H;
    const unsigned short *wi = wv + (long long)f * TF_W16_V, *wg = wi + TF_H * TF_H;
    const float xf = xs[row * TF_MAXF + f];
    float res[16], outv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + rt_feat(r, hf);
      v[r] = tf_elu(fmaf(xf, vu[n], vv[n]));
      res[r] = fmaf(xf, va[n], vb[n]);
    }
    rt_store16<DT, false>(Hs + row * TF_LD, n0, hf, v);
    __syncthreads();
    acc = tf_block<DT>(wi, n0, Hs, lane, rt_load16s(bi, n0, hf));
    rt_store16<DT, false>(Gs + row * TF_LD, n0, hf, acc);
    __syncthreads();
    tf_glu_ln<DT>(Gs, wg, bg, gam, bet, p.eps, red, wave, lane, res, outv);
    const float w = wsel[row * TF_MAXF + f];
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = fmaf(w, outv[r], o[r]);
  }
  const long long r = row0 + row;
  if (r < p.rows) rt_store16<DT, false>(p.out + ((r / p.tn) * p.out_T + p.out_t0 + r % p.tn) * p.ldo, n0, hf, o);
}

extern "C" int dle_tft_vsn_fwd(const float* x0, int64_t ld0, int n0, const float* x1, int64_t ld1, int n1, const float* x2, int64_t ld2,
                               int n2, int64_t rows_per_batch, int64_t src_steps, int64_t src_t0, const void* ctx, int64_t ldc,
                               const void* w16, const float* p32, void* out, int64_t ldo, int64_t out_steps, int64_t out_t0,
                               float* weights, int64_t rows, int hidden, float eps, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "tft_vsn_fwd: 16-bit operands only");
  DLE_CHECK_ARG(hidden == TF_H, "tft_vsn_fwd: built for hidden size 128 (got %d)", hidden);
  DLE_CHECK_ARG(n0 >= 0 && n1 >= 0 && n2 >= 0 && n0 + n1 + n2 >= 1 && n0 + n1 + n2 <= TF_MAXF,
                "tft_vsn_fwd: 1 to 8 continuous variables (got %d + %d + %d)", n0, n1, n2);
  DLE_CHECK_ARG((n0 == 0 || (x0 && ld0 >= n0)) && (n1 == 0 || (x1 && ld1 >= n1)) && (n2 == 0 || (x2 && ld2 >= n2)),
                "tft_vsn_fwd: a variable group needs its pointer and a pitch of at least its width");
  DLE_CHECK_ARG(rows >= 0 && (rows + TF_R - 1) / TF_R < 0x7FFFFFFFLL, "tft_vsn_fwd: bad row count");
  DLE_CHECK_ARG(rows_per_batch >= 1 && rows % rows_per_batch == 0, "tft_vsn_fwd: rows must be batch * rows_per_batch");
  DLE_CHECK_ARG(src_t0 >= 0 && src_t0 + rows_per_batch <= src_steps, "tft_vsn_fwd: the source window lies outside its %lld steps",
                (long long)src_steps);
  DLE_CHECK_ARG(out_t0 >= 0 && out_t0 + rows_per_batch <= out_steps, "tft_vsn_fwd: the output window lies outside its %lld steps",
                (long long)out_steps);
  DLE_CHECK_ARG(w16 && p32 && out, "tft_vsn_fwd: null pointer");
  DLE_CHECK_ARG(ldo >= TF_H && (ldo & 7) == 0, "tft_vsn_fwd: ldo must be a multiple of 8, at least 128");
  DLE_CHECK_ARG(!ctx || (ldc >= TF_H && (ldc & 7) == 0), "tft_vsn_fwd: ldc must be a multiple of 8, at least 128");
  DLE_CHECK_ARG(dle_aligned<16>(ctx, w16, out) && dle_aligned<4>(x0, x1, x2, p32, weights),
                "tft_vsn_fwd: 16-bit tensors must be 16-byte aligned, fp32 tensors 4-byte aligned");
  if (rows == 0) return 0;
  TftVsnArgs a = {};
  a.seg[0] = x0; a.seg[1] = x1; a.seg[2] = x2; a.seg_ld[0] = ld0; a.seg_ld[1] = ld1; a.seg_ld[2] = ld2;
  a.seg_n[0] = n0; a.seg_n[1] = n1; a.seg_n[2] = n2;
  a.tn = rows_per_batch; a.src_T = src_steps; a.src_t0 = src_t0;
  a.ctx = (const unsigned short*)ctx; a.ldc = ldc; a.w16 = (const unsigned short*)w16; a.p32 = p32;
  a.out = (unsigned short*)out; a.ldo = ldo; a.out_T = out_steps; a.out_t0 = out_t0; a.wout = weights;
  a.rows = rows; a.F = n0 + n1 + n2; a.eps = eps;
  const dim3 grid((unsigned)((rows + TF_R - 1) / TF_R));
  if (dtype == DLE_F16) hipLaunchKernelGGL(tft_vsn_kernel<DLE_F16>, grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(tft_vsn_kernel<DLE_BF16>, grid, dim3(256), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_tft_lstm_fwd: nn.LSTM(H, H, batch_first=True) over all steps (modeling.py:368-370, 395-397) ---------------------------
// One workgroup of eight wavefronts per 32 batch rows.  Wavefront w owns hidden units 16 w .. 16 w + 15: its 64 rows of W_hh (four
// gates) are 64 VGPRs per lane for the whole launch, loaded once.  Per step: gates^T = xproj + W_hh h^T (16 MFMAs per wavefront),
// the cell update in fp32 registers, the new h (rounded) into the other of two LDS images, one barrier.  Block 0 of a wavefront
// is gates i | f, block 1 is g | o, so the four gates of a unit meet in one lane.  No workgroup waits for another.
struct TftLstmArgs {
  const float* xp; long long xp_bs, xp_ts;
  const unsigned short *whh, *h0;
  const void* c0; int c0_f32;
  unsigned short* out; long long out_bs, out_ts;
  unsigned short* hn; float* cn;
  int B, T;
};

template <int DT>
__global__ __launch_bounds__(512) void tft_lstm_kernel(TftLstmArgs p) {
  __shared__ __attribute__((aligned(16))) unsigned short hs[2 * TF_IMG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, row = lane & 31;
  const int b = blockIdx.x * TF_R + row;
  const bool ok = b < p.B;
  const int bc = ok ? b : p.B - 1;
  ushort8_t wf[2][8];
#pragma unroll
  for (int blk = 0; blk < 2; ++blk) {
    const int gate = 2 * blk + (row >> 4), unit = 16 * wave + (row & 15);
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) wf[blk][ks] = *(const ushort8_t*)(p.whh + (gate * TF_H + unit) * TF_H + ks * 16 + hf * 8);
  }
  {
    const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int r = tid >> 4, c8 = tid & 15, bb = blockIdx.x * TF_R + r;
    *(ushort8_t*)(hs + r * TF_LD + c8 * 8) = bb < p.B ? *(const ushort8_t*)(p.h0 + (long long)bb * TF_H + c8 * 8) : zero8;
  }
  const int u0 = 16 * wave + 4 * hf;                       // the lane's units: u0 + 0..3 and u0 + 8 + 0..3
  float c[8];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const long long at = (long long)bc * TF_H + u0 + rt_feat(r, 0);
    c[r] = p.c0_f32 ? ((const float*)p.c0)[at] : Elem<DT>::to_f32(((const unsigned short*)p.c0)[at]);
  }
  const float* xrow = p.xp + (long long)bc * p.xp_bs + u0;
  float4_t xg[4][2];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int g = 0; g < 2; ++g) xg[q][g] = *(const float4_t*)(xrow + q * TF_H + 8 * g);
  uint2_t hp[2] = {};
  __syncthreads();
  for (int t = 0; t < p.T; ++t) {
    const unsigned short* cur = hs + (t & 1) * TF_IMG;
    unsigned short* nxt = hs + ((t + 1) & 1) * TF_IMG;
    float16_t a0, a1;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      a0[r] = xg[0][r >> 2][r & 3];
      a0[8 + r] = xg[1][r >> 2][r & 3];
      a1[r] = xg[2][r >> 2][r & 3];
      a1[8 + r] = xg[3][r >> 2][r & 3];
    }
    {
      // the next step's input projection is in flight while this step computes
      const float* xn = xrow + (long long)(t + 1 < p.T ? t + 1 : t) * p.xp_ts;
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int g = 0; g < 2; ++g) xg[q][g] = *(const float4_t*)(xn + q * TF_H + 8 * g);
    }
    const unsigned short* hrow = cur + row * TF_LD + hf * 8;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const ushort8_t hfrag = *(const ushort8_t*)(hrow + ks * 16);
      a0 = Mfma32x16<DT>::run(wf[0][ks], hfrag, a0);
      a1 = Mfma32x16<DT>::run(wf[1][ks], hfrag, a1);
    }
    float h[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const float ig = tf_sigmoid(a0[r]), fg = tf_sigmoid(a0[8 + r]), gg = fast_tanh(a1[r]), og = tf_sigmoid(a1[8 + r]);
      c[r] = fg * c[r] + ig * gg;
      h[r] = og * fast_tanh(c[r]);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      hp[g] = rt_pack4<DT>(h[4 * g], h[4 * g + 1], h[4 * g + 2], h[4 * g + 3]);
      *(uint2_t*)(nxt + row * TF_LD + u0 + 8 * g) = hp[g];
      if (ok && p.out) *(uint2_t*)(p.out + (long long)b * p.out_bs + (long long)t * p.out_ts + u0 + 8 * g) = hp[g];
    }
    __syncthreads();
  }
  if (ok) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
      if (p.hn) *(uint2_t*)(p.hn + (long long)b * TF_H + u0 + 8 * g) = hp[g];
    if (p.cn) {
#pragma unroll
      for (int r = 0; r < 8; ++r) p.cn[(long long)b * TF_H + u0 + rt_feat(r, 0)] = c[r];
    }
  }
}

extern "C" int dle_tft_lstm_fwd(const float* xproj, int64_t xp_batch_stride, int64_t xp_step_stride, const void* whh, const void* h0,
                                const void* c0, int c0_dtype, void* out, int64_t out_batch_stride, int64_t out_step_stride, void* hn,
                                float* cn, int B, int T, int hidden, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "tft_lstm_fwd: 16-bit operands only");
  DLE_CHECK_ARG(hidden == TF_H, "tft_lstm_fwd: built for hidden size 128 (got %d)", hidden);
  DLE_CHECK_ARG(B >= 1 && T >= 1, "tft_lstm_fwd: bad batch or step count (%d, %d)", B, T);
  DLE_CHECK_ARG(c0_dtype == DLE_F32 || c0_dtype == dtype, "tft_lstm_fwd: c0 is fp32 or of the operand type");
  DLE_CHECK_ARG(xproj && whh && h0 && c0, "tft_lstm_fwd: null pointer");
  DLE_CHECK_ARG(out || hn || cn, "tft_lstm_fwd: no output");
  DLE_CHECK_ARG(xp_step_stride >= 4 * TF_H && (xp_step_stride & 3) == 0 && (xp_batch_stride & 3) == 0 &&
                    (B == 1 || xp_batch_stride >= 4 * TF_H),
                "tft_lstm_fwd: the projection's strides must be multiples of 4, at least 512");
  DLE_CHECK_ARG(!out || (out_step_stride >= TF_H && (out_step_stride & 3) == 0 && (out_batch_stride & 3) == 0 &&
                         (B == 1 || out_batch_stride >= TF_H)),
                "tft_lstm_fwd: the output's strides must be multiples of 4, at least 128");
  DLE_CHECK_ARG(dle_aligned<16>(xproj, whh, h0, c0, cn) && dle_aligned<8>(out, hn), "tft_lstm_fwd: misaligned tensor");
  TftLstmArgs a = {};
  a.xp = xproj; a.xp_bs = xp_batch_stride; a.xp_ts = xp_step_stride; a.whh = (const unsigned short*)whh;
  a.h0 = (const unsigned short*)h0; a.c0 = c0; a.c0_f32 = c0_dtype == DLE_F32;
  a.out = (unsigned short*)out; a.out_bs = out_batch_stride; a.out_ts = out_step_stride; a.hn = (unsigned short*)hn; a.cn = cn;
  a.B = B; a.T = T;
  const dim3 grid((unsigned)((B + TF_R - 1) / TF_R));
  if (dtype == DLE_F16) hipLaunchKernelGGL(tft_lstm_kernel<DLE_F16>, grid, dim3(512), 0, stream, a);
  else hipLaunchKernelGGL(tft_lstm_kernel<DLE_BF16>, grid, dim3(512), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_tft_attention_fwd: InterpretableMultiHeadAttention.forward after qkv_linears, for the decoder positions only
// (modeling.py:337-360, 414) ------------------------------------------------------------------------------------------------------
// One wavefront per (batch element, 32 queries).  Per head, S^T = K Q^T over the key tiles up to the last query's position
// (2 MFMAs a tile, d_head = 32), softmax in registers with the causal mask by index, and the probabilities are summed over the
// heads in the accumulator layout: V is shared, so mean_h(P_h V) = (mean_h P_h) V.  That mean is the B operand of
// context^T = V^T P^T as it stands, and context^T is the B operand of out^T = W_o context^T.
struct TftAttnArgs {
  const unsigned short *qkv, *wo;
  long long ld;
  unsigned short* out;
  float* probs;
  int T, enc, nq, nqt;
  float scale;
};

template <int DT>
__global__ __launch_bounds__(64) void tft_attn_kernel(TftAttnArgs p) {
  constexpr int NT = TF_MAXT / 32;
  __shared__ __attribute__((aligned(16))) unsigned short Vs[TF_MAXT * TF_VLD];
  const int lane = threadIdx.x, hf = lane >> 5, qi = lane & 31;
  const int qt = blockIdx.x % p.nqt, b = blockIdx.x / p.nqt;
  const int i = p.enc + qt * 32 + qi;
  const bool qok = i < p.T;
  const int ic = qok ? i : p.T - 1;
  const int imax = p.enc + qt * 32 + 31 < p.T - 1 ? p.enc + qt * 32 + 31 : p.T - 1;
  const int ntiles = imax / 32 + 1;
  const unsigned short* base = p.qkv + (long long)b * p.T * p.ld;
  const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int idx = lane; idx < ntiles * 32 * 4; idx += 64) {
    const int key = idx >> 2, c8 = idx & 3;
    *(ushort8_t*)(Vs + key * TF_VLD + c8 * 8) = key < p.T ? *(const ushort8_t*)(base + (long long)key * p.ld + 2 * TF_H + c8 * 8) : zero8;
  }
  float16_t pm[NT];
#pragma unroll
  for (int kt = 0; kt < NT; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) pm[kt][r] = 0.f;
#pragma unroll
  for (int head = 0; head < 4; ++head) {
    ushort8_t qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *(const ushort8_t*)(base + (long long)ic * p.ld + head * 32 + ks * 16 + hf * 8);
    float16_t s[NT];
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < ntiles) {
        const int key = kt * 32 + qi, kc = key < p.T ? key : p.T - 1;
        const unsigned short* krow = base + (long long)kc * p.ld + TF_H + head * 32 + hf * 8;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) s[kt] = Mfma32x16<DT>::run(*(const ushort8_t*)(krow + ks * 16), qf[ks], s[kt]);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = kt * 32 + rt_feat(r, hf);
          s[kt][r] = j <= ic ? s[kt][r] * p.scale : -INFINITY;
          m = fmaxf(m, s[kt][r]);
        }
      }
    }
    m = fmaxf(m, __shfl_xor(m, 32, 64));                  // key 0 is never masked: m is finite
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < ntiles) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          s[kt][r] = s[kt][r] == -INFINITY ? 0.f : __expf(s[kt][r] - m);
          sum += s[kt][r];
        }
      }
    }
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
#pragma unroll
    for (int kt = 0; kt < NT; ++kt) {
      if (kt < ntiles) {
#pragma unroll
        for (int r = 0; r < 16; ++r) pm[kt][r] += s[kt][r] * inv;
      }
    }
  }
  const long long orow = (long long)b * p.nq + (ic - p.enc);
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      pm[kt][r] = kt < ntiles ? pm[kt][r] * 0.25f : 0.f;
      const int j = kt * 32 + rt_feat(r, hf);
      if (p.probs && qok && j < p.T) p.probs[orow * p.T + j] = pm[kt][r];
    }
  }
  __syncthreads();
  // context^T[d][q] = sum_key V[key][d] mean P[q][key]: element e of k step s of the accumulator-as-operand is key 16 s + 8 (e >> 2)
  // + 4 hf + (e & 3) of the tile, and the V fragment is gathered in that order
  float16_t ctx;
#pragma unroll
  for (int r = 0; r < 16; ++r) ctx[r] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NT; ++kt) {
    if (kt < ntiles) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float pv[8];
        ushort8_t vf;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          pv[e] = pm[kt][8 * ks + e];
          vf[e] = Vs[(kt * 32 + 16 * ks + rt_feat(e, hf)) * TF_VLD + qi];
        }
        ctx = Mfma32x16<DT>::run(vf, pack8<DT>(pv), ctx);
      }
    }
  }
  // out^T[n][q] = sum_d W_o[n][d] context[q][d], the same operand order over d
  ushort8_t cf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    float cv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cv[e] = ctx[8 * ks + e];
    cf[ks] = pack8<DT>(cv);
  }
#pragma unroll
  for (int nb = 0; nb < 4; ++nb) {
    float16_t o;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[r] = 0.f;
    const unsigned short* wrow = p.wo + (nb * 32 + qi) * 32 + 4 * hf;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint2_t lo = *(const uint2_t*)(wrow + 16 * ks), hi = *(const uint2_t*)(wrow + 16 * ks + 8);
      uint4_t w4;
      w4[0] = lo[0]; w4[1] = lo[1]; w4[2] = hi[0]; w4[3] = hi[1];
      o = Mfma32x16<DT>::run(__builtin_bit_cast(ushort8_t, w4), cf[ks], o);
    }
    if (qok) rt_store16<DT, false>(p.out + orow * TF_H, nb * 32, hf, o);
  }
}

extern "C" int dle_tft_attention_fwd(const void* qkv, int64_t ld, const void* wo, void* out, float* probs, int B, int T,
                                     int encoder_length, int heads, int d_head, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "tft_attention_fwd: 16-bit operands only");
  DLE_CHECK_ARG(heads == 4 && d_head == 32, "tft_attention_fwd: built for 4 heads of 32 (got %d of %d)", heads, d_head);
  DLE_CHECK_ARG(B >= 1 && T >= 2 && T <= TF_MAXT, "tft_attention_fwd: 2 <= T <= 192 and a positive batch (got %d, %d)", T, B);
  DLE_CHECK_ARG(encoder_length >= 1 && encoder_length < T, "tft_attention_fwd: 1 <= encoder_length < T (got %d, %d)", encoder_length, T);
  DLE_CHECK_ARG(qkv && wo && out, "tft_attention_fwd: null pointer");
  DLE_CHECK_ARG(ld >= 9 * 32 && (ld & 7) == 0, "tft_attention_fwd: ld must be a multiple of 8, at least 288");
  DLE_CHECK_ARG(dle_aligned<16>(qkv, wo, out) && dle_aligned<4>(probs), "tft_attention_fwd: misaligned tensor");
  const int nq = T - encoder_length, nqt = (nq + 31) / 32;
  DLE_CHECK_ARG((long long)B * nqt < 0x7FFFFFFFLL, "tft_attention_fwd: grid too large");
  TftAttnArgs a = {};
  a.qkv = (const unsigned short*)qkv; a.wo = (const unsigned short*)wo; a.ld = ld; a.out = (unsigned short*)out; a.probs = probs;
  a.T = T; a.enc = encoder_length; a.nq = nq; a.nqt = nqt; a.scale = 1.0f / sqrtf((float)d_head);
  const dim3 grid((unsigned)(B * nqt));
  if (dtype == DLE_F16) hipLaunchKernelGGL(tft_attn_kernel<DLE_F16>, grid, dim3(64), 0, stream, a);
  else hipLaunchKernelGGL(tft_attn_kernel<DLE_BF16>, grid, dim3(64), 0, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}
