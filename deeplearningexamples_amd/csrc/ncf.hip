// Neural Collaborative Filtering (NeuMF) inference on gfx950 (reference: PyTorch/Recommendation/NCF/neumf.py, ncf.py): the whole
// forward of a sample in one persistent launch, and the HR@K / NDCG@K tail of the evaluation without a sort.
//
// dle_ncf_score_fwd.  A sample is four table rows (64 + 64 halves for the GMF branch, 128 + 128 for the MLP branch), a
// 256 -> 256 -> 128 -> 64 ReLU MLP and one 128-wide dot product.  One workgroup of eight wavefronts per compute unit walks tiles
// of 64 samples (two halves of 32).  The layers are out^T = W X^T in the operand order and lane layout of mfma32_rows.h.  The
// weights are read once per workgroup: W1 (128 KB) is 64 VGPRs per lane over the eight wavefronts (wavefront w owns output
// features 32 w .. 32 w + 31), W2 (64 KB) another 64 VGPRs (wavefront w owns feature block w & 3 for the samples of half w >> 2,
// so each block is held twice), W3 (16 KB), the biases and the final layer's fp32 weights are in LDS.
// The rows of the NEXT tile are requested before the current tile's first MFMA and land in the X image after layer 1 has read it;
// the indices are read one tile further ahead still, so no row address waits for an index.  Nothing of a sample but its score
// leaves the compute unit.
#include "mfma32_rows.h"
#include <math.h>

#define NC_F 64                      // GMF factors
#define NC_E 128                     // width of one MLP embedding row (L0 / 2)
#define NC_L1 256
#define NC_L2 128
#define NC_L3 64
#define NC_R 64                      // samples per tile
#define NC_LDX 264                   // halves per line of the 256-wide images: 528 bytes, 16 lines start in 16 different 16-byte slots
#define NC_LDH 136                   // halves per line of the 128-wide images: 272 bytes, 32 lines start in 8 different bank groups
#define NC_THREADS 512

// LDS map (bytes): X image, H1 image, H2 image, W3 image, fp32 block (b1 | b2 | b3 | wf mlp part | wf gmf part), partial dots of the
// two feature blocks of layer 3, GMF dots and validity of two tiles in flight
#define NC_OFF_H1 (NC_R * NC_LDX * 2)
#define NC_OFF_H2 (NC_OFF_H1 + NC_R * NC_LDX * 2)
#define NC_OFF_W3 (NC_OFF_H2 + NC_R * NC_LDH * 2)
#define NC_OFF_P32 (NC_OFF_W3 + NC_L3 * NC_LDH * 2)
#define NC_P32_FLOATS (NC_L1 + NC_L2 + NC_L3 + NC_L3 + NC_F)
#define NC_OFF_PART (NC_OFF_P32 + NC_P32_FLOATS * 4)
#define NC_OFF_GMF (NC_OFF_PART + 2 * NC_R * 4)
#define NC_OFF_VALID (NC_OFF_GMF + 2 * NC_R * 4)
#define NC_LDS_BYTES (NC_OFF_VALID + 2 * NC_R * 4)

struct NcfScoreArgs {
  const unsigned short *mfu, *mfi, *mlu, *mli, *w1, *w2, *w3;
  const float *b1, *b2, *b3, *wf, *bf;
  const void *user, *item;
  const float* label;
  float *logit, *prob, *loss;
  long long B, U, I;
  int idx64, n_partials;
};

template <int DT>
__global__ __launch_bounds__(NC_THREADS) void ncf_score_kernel(NcfScoreArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nc_lds[];
  unsigned short* Xs = (unsigned short*)nc_lds;
  unsigned short* H1 = (unsigned short*)(nc_lds + NC_OFF_H1);
  unsigned short* H2 = (unsigned short*)(nc_lds + NC_OFF_H2);
  unsigned short* W3s = (unsigned short*)(nc_lds + NC_OFF_W3);
  float* p32 = (float*)(nc_lds + NC_OFF_P32);
  float *b1s = p32, *b2s = b1s + NC_L1, *b3s = b2s + NC_L2, *wfm = b3s + NC_L3, *wfg = wfm + NC_L3;
  float* part = (float*)(nc_lds + NC_OFF_PART);
  float* gmf = (float*)(nc_lds + NC_OFF_GMF);
  int* valid = (int*)(nc_lds + NC_OFF_VALID);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, row = lane & 31;
  const int lrow = tid >> 3, lk = tid & 7;             // the loader's view: eight threads per sample, 16 bytes per thread and piece
  const long long ntiles = (p.B + NC_R - 1) / NC_R, stride = gridDim.x;
  const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

  // checked indices of the loader's sample in `tile`: -1 outside the batch or outside the table; no address is formed from them
  auto load_index = [&](long long tile, int& iu, int& ii) {
    iu = ii = -1;
    const long long r = tile * NC_R + lrow;
    if (tile < ntiles && r < p.B) {
      const long long u = p.idx64 ? ((const long long*)p.user)[r] : (long long)((const int*)p.user)[r];
      const long long i = p.idx64 ? ((const long long*)p.item)[r] : (long long)((const int*)p.item)[r];
      iu = (u >= 0 && u < p.U) ? (int)u : -1;
      ii = (i >= 0 && i < p.I) ? (int)i : -1;
    }
  };
  ushort8_t xr[4], mr[2];
  auto load_rows = [&](int iu, int ii) -> int {
    const int ok = iu >= 0 && ii >= 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) xr[j] = zero8;
    mr[0] = mr[1] = zero8;
    if (ok) {
      const unsigned short* a = p.mlu + (long long)iu * NC_E + lk * 8;
      const unsigned short* b = p.mli + (long long)ii * NC_E + lk * 8;
      xr[0] = *(const ushort8_t*)a;
      xr[1] = *(const ushort8_t*)(a + 64);
      xr[2] = *(const ushort8_t*)b;
      xr[3] = *(const ushort8_t*)(b + 64);
      mr[0] = *(const ushort8_t*)(p.mfu + (long long)iu * NC_F + lk * 8);
      mr[1] = *(const ushort8_t*)(p.mfi + (long long)ii * NC_F + lk * 8);
    }
    return ok;
  };
  // the requested rows into the X image, and the GMF half of the final dot product (fp32 throughout) into slot `par`
  auto store_rows = [&](int par, int ok) {
    unsigned short* line = Xs + lrow * NC_LDX + lk * 8;
    *(ushort8_t*)line = xr[0];
    *(ushort8_t*)(line + 64) = xr[1];
    *(ushort8_t*)(line + 128) = xr[2];
    *(ushort8_t*)(line + 192) = xr[3];
    float a[8], b[8], s = 0.f;
    unpack8<DT>(mr[0], a);
    unpack8<DT>(mr[1], b);
#pragma unroll
    for (int e = 0; e < 8; ++e) s = fmaf(a[e] * b[e], wfg[lk * 8 + e], s);
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (lk == 0) {
      gmf[par * NC_R + lrow] = s;
      valid[par * NC_R + lrow] = ok;
    }
  };

  int iu, ii;
  load_index(blockIdx.x, iu, ii);
  int ok_next = load_rows(iu, ii);
  load_index(blockIdx.x + stride, iu, ii);

  // the weights, once per workgroup
  ushort8_t w1f[16], w2f[16];
  {
    const unsigned short* r1 = p.w1 + (32 * wave + row) * NC_L1 + hf * 8;
    const unsigned short* r2 = p.w2 + (32 * (wave & 3) + row) * NC_L1 + hf * 8;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
      w1f[ks] = *(const ushort8_t*)(r1 + ks * 16);
      w2f[ks] = *(const ushort8_t*)(r2 + ks * 16);
    }
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int c = tid + it * NC_THREADS, r = c >> 4, c8 = c & 15;
      *(ushort8_t*)(W3s + r * NC_LDH + c8 * 8) = *(const ushort8_t*)(p.w3 + r * NC_L2 + c8 * 8);
    }
    for (int i = tid; i < NC_P32_FLOATS; i += NC_THREADS)
      p32[i] = i < NC_L1 ? p.b1[i]
             : i < NC_L1 + NC_L2 ? p.b2[i - NC_L1]
             : i < NC_L1 + NC_L2 + NC_L3 ? p.b3[i - NC_L1 - NC_L2]
             : i < NC_L1 + NC_L2 + 2 * NC_L3 ? p.wf[NC_F + (i - NC_L1 - NC_L2 - NC_L3)]
                                             : p.wf[i - NC_L1 - NC_L2 - 2 * NC_L3];
  }
  if (p.loss && blockIdx.x == 0)
    for (int i = gridDim.x + tid; i < p.n_partials; i += NC_THREADS) p.loss[i] = 0.f;
  __syncthreads();                                     // wfg is in LDS before the first GMF dot
  store_rows(0, ok_next);
  __syncthreads();

  const float bf = p.bf[0];
  float lacc = 0.f;
  int par = 0;
  for (long long tile = blockIdx.x; tile < ntiles; tile += stride) {
    ok_next = load_rows(iu, ii);                       // tile + stride: in flight under this tile's MFMAs
    load_index(tile + 2 * stride, iu, ii);

    // layer 1: wavefront w -> features 32 w .. 32 w + 31 of both halves of the tile
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float16_t acc = rt_load16(b1s, 32 * wave, hf);
      const unsigned short* xrow = Xs + (s * 32 + row) * NC_LDX + hf * 8;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) acc = Mfma32x16<DT>::run(w1f[ks], *(const ushort8_t*)(xrow + ks * 16), acc);
      rt_store16<DT, true>(H1 + (s * 32 + row) * NC_LDX, 32 * wave, hf, acc);
    }
    __syncthreads();
    // layer 2: wavefront w -> feature block w & 3 of half w >> 2
    {
      const int blk = wave & 3, s = wave >> 2;
      float16_t acc = rt_load16(b2s, 32 * blk, hf);
      const unsigned short* xrow = H1 + (s * 32 + row) * NC_LDX + hf * 8;
#pragma unroll
      for (int ks = 0; ks < 16; ++ks) acc = Mfma32x16<DT>::run(w2f[ks], *(const ushort8_t*)(xrow + ks * 16), acc);
      rt_store16<DT, true>(H2 + (s * 32 + row) * NC_LDH, 32 * blk, hf, acc);
    }
    store_rows(par ^ 1, ok_next);                      // layer 1 was the X image's last reader
    __syncthreads();
    // layer 3 (fp32 output, not rounded) and its half of the final dot product: wavefronts 0..3 -> block w & 1 of half w >> 1
    if (wave < 4) {
      const int blk = wave & 1, s = wave >> 1;
      const float16_t acc = rt_mma<DT>(W3s + (32 * blk + row) * NC_LDH + hf * 8, 16, H2 + (s * 32 + row) * NC_LDH + hf * 8, NC_L2 / 16,
                                       rt_load16(b3s, 32 * blk, hf));
      const float16_t w = rt_load16(wfm, 32 * blk, hf);
      float d = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) d = fmaf(fmaxf(acc[r], 0.f), w[r], d);
      d += __shfl_xor(d, 32, 64);
      if (hf == 0) part[blk * NC_R + s * 32 + row] = d;
    }
    __syncthreads();
    if (tid < NC_R) {
      const long long r = tile * NC_R + tid;
      if (r < p.B) {
        const bool ok = valid[par * NC_R + tid] != 0;
        const float x = ok ? (part[tid] + part[NC_R + tid]) + gmf[par * NC_R + tid] + bf : __builtin_nanf("");
        p.logit[r] = x;
        if (p.prob) p.prob[r] = 1.f / (1.f + expf(-x));
        if (p.loss && ok) {
          // torch's binary_cross_entropy on p = sigmoid(x), from the logit: log p = min(x, 0) - log1p(exp(-|x|))
          const float y = p.label[r], sp = log1pf(expf(-fabsf(x)));
          const float lp = fmaxf(fminf(x, 0.f) - sp, -100.f), lq = fmaxf(fminf(-x, 0.f) - sp, -100.f);
          lacc -= y * lp + (1.f - y) * lq;
        }
      }
    }
    par ^= 1;
  }
  if (p.loss && wave == 0) {
    const float t = wave_sum(lacc);
    if (lane == 0) p.loss[blockIdx.x] = t;
  }
}

extern "C" int dle_ncf_score_supported(int factors, int l0, int l1, int l2, int l3) {
  return factors == NC_F && l0 == 2 * NC_E && l1 == NC_L1 && l2 == NC_L2 && l3 == NC_L3 ? 1 : 0;
}

extern "C" int dle_ncf_score_fwd(const void* mf_user, const void* mf_item, const void* mlp_user, const void* mlp_item, int64_t n_users,
                                 int64_t n_items, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                                 const float* b3, const float* wf, const float* bf, const void* user, const void* item, int index_bits,
                                 const float* label, float* logit, float* prob, float* loss_partials, int n_partials, int64_t batch,
                                 int factors, int l0, int l1, int l2, int l3, int max_workgroups, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "ncf_score_fwd: 16-bit tables and weights only");
  DLE_CHECK_ARG(dle_ncf_score_supported(factors, l0, l1, l2, l3),
                "ncf_score_fwd: built for --factors 64 --layers 256 256 128 64 (got %d and %d %d %d %d)", factors, l0, l1, l2, l3);
  DLE_CHECK_ARG(index_bits == 32 || index_bits == 64, "ncf_score_fwd: indices are int32 or int64 (got %d bits)", index_bits);
  DLE_CHECK_ARG(mf_user && mf_item && mlp_user && mlp_item && w1 && b1 && w2 && b2 && w3 && b3 && wf && bf && user && item && logit,
                "ncf_score_fwd: null pointer");
  DLE_CHECK_ARG(n_users >= 1 && n_items >= 1 && n_users < 0x7FFFFFFFLL && n_items < 0x7FFFFFFFLL, "ncf_score_fwd: bad table sizes");
  DLE_CHECK_ARG(batch >= 0, "ncf_score_fwd: bad batch size");
  DLE_CHECK_ARG(max_workgroups >= 0, "ncf_score_fwd: max_workgroups must be 0 (the device's CU count) or positive");
  DLE_CHECK_ARG((loss_partials == nullptr) == (label == nullptr), "ncf_score_fwd: the labels and the loss partials go together");
  DLE_CHECK_ARG(!loss_partials || n_partials >= 1, "ncf_score_fwd: the loss needs at least one partial slot");
  DLE_CHECK_ARG(dle_aligned<16>(mf_user, mf_item, mlp_user, mlp_item, w1, w2, w3), "ncf_score_fwd: tables and weights must be 16-byte aligned");
  DLE_CHECK_ARG(dle_aligned<4>(b1, b2, b3, wf, bf, label, logit, prob, loss_partials) &&
                    (index_bits == 64 ? dle_aligned<8>(user, item) : dle_aligned<4>(user, item)), "ncf_score_fwd: misaligned tensor");
  if (batch == 0) {
    if (loss_partials) (void)hipMemsetAsync(loss_partials, 0, sizeof(float) * n_partials, stream);
    return 0;
  }
  const DleDeviceLimits* lim = dle_device_limits();
  DLE_CHECK_ARG(lim != nullptr, "ncf_score_fwd: no usable device");
  DLE_CHECK_ARG(lim->lds_per_block >= NC_LDS_BYTES, "ncf_score_fwd: the device offers %d bytes of LDS per workgroup, %d needed",
                lim->lds_per_block, NC_LDS_BYTES);
  long long grid = rt_persistent_grid((batch + NC_R - 1) / NC_R, max_workgroups, lim);
  if (loss_partials && grid > n_partials) grid = n_partials;
  NcfScoreArgs a = {};
  a.mfu = (const unsigned short*)mf_user; a.mfi = (const unsigned short*)mf_item;
  a.mlu = (const unsigned short*)mlp_user; a.mli = (const unsigned short*)mlp_item;
  a.w1 = (const unsigned short*)w1; a.w2 = (const unsigned short*)w2; a.w3 = (const unsigned short*)w3;
  a.b1 = b1; a.b2 = b2; a.b3 = b3; a.wf = wf; a.bf = bf; a.user = user; a.item = item; a.label = label;
  a.logit = logit; a.prob = prob; a.loss = loss_partials; a.B = batch; a.U = n_users; a.I = n_items;
  a.idx64 = index_bits == 64; a.n_partials = loss_partials ? n_partials : 0;
  if (dtype == DLE_F16) DLE_LAUNCH_LDS((ncf_score_kernel<DLE_F16>), dim3((unsigned)grid), dim3(NC_THREADS), NC_LDS_BYTES, stream, a);
  else DLE_LAUNCH_LDS((ncf_score_kernel<DLE_BF16>), dim3((unsigned)grid), dim3(NC_THREADS), NC_LDS_BYTES, stream, a);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dle_ncf_rank_fwd: the tail of val_epoch (ncf.py:150-162) as a stated rule, one wavefront per series --------------------------
// r_j = -1 where ignore_j is set, else rating_j; rank_j = #{i : r_i > r_j or (r_i == r_j and i < j)}, NaN below everything and among
// themselves by index; label-1 elements with rank_j < k count: hits, and dcg += log 2 / log(rank_j + 2).  Only the label-1 elements
// need a rank, so the work is S compares per positive, not a sort.
#define NC_MAXS 4096

__device__ __forceinline__ bool nc_above(float ri, float rj, int i, int j) {
  const bool ni = ri != ri, nj = rj != rj;
  if (ni || nj) return ni && nj ? i < j : nj;
  return ri > rj || (ri == rj && i < j);
}

__global__ __launch_bounds__(64) void ncf_rank_kernel(const float* __restrict__ rating, const float* __restrict__ label,
                                                      const uint8_t* __restrict__ ignore, int* __restrict__ hits,
                                                      float* __restrict__ dcg, int S, int k) {
  __shared__ float rs[NC_MAXS];
  const int lane = threadIdx.x;
  const long long base = (long long)blockIdx.x * S;
  for (int i = lane; i < S; i += 64) rs[i] = (ignore && ignore[base + i]) ? -1.f : rating[base + i];
  __syncthreads();
  int nh = 0;
  float d = 0.f;
  for (int j0 = 0; j0 < S; j0 += 64) {
    const int j = j0 + lane;
    unsigned long long pos = __ballot(j < S && label[base + j] == 1.f);
    while (pos) {
      const int jj = j0 + __builtin_ctzll(pos);
      pos &= pos - 1;
      const float rj = rs[jj];
      int cnt = 0;
      for (int i = lane; i < S; i += 64) cnt += nc_above(rs[i], rj, i, jj) ? 1 : 0;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
      if (cnt < k) {
        nh += 1;
        d += logf(2.f) / logf((float)(cnt + 2));
      }
    }
  }
  if (lane == 0) {
    hits[blockIdx.x] = nh;
    dcg[blockIdx.x] = d;
  }
}

extern "C" int dle_ncf_rank_fwd(const float* rating, const float* label, const uint8_t* ignore, int32_t* hits, float* dcg,
                                int64_t n_series, int S, int k, hipStream_t stream) {
  DLE_CHECK_ARG(S >= 1 && S <= NC_MAXS, "ncf_rank_fwd: 1 <= samples per series <= 4096 (got %d)", S);
  DLE_CHECK_ARG(k >= 1 && k <= S, "ncf_rank_fwd: 1 <= k <= samples per series (got k = %d, %d per series)", k, S);
  DLE_CHECK_ARG(n_series >= 0 && n_series < 0x7FFFFFFFLL, "ncf_rank_fwd: bad series count");
  DLE_CHECK_ARG(rating && label && hits && dcg, "ncf_rank_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<4>(rating, label, hits, dcg), "ncf_rank_fwd: misaligned tensor");
  if (n_series == 0) return 0;
  hipLaunchKernelGGL(ncf_rank_kernel, dim3((unsigned)n_series), dim3(64), 0, stream, rating, label, ignore, hits, dcg, S, k);
  DLE_LAUNCH_CHECK();
  return 0;
}
