// Transformer-XL evaluation on gfx950: relative multi-head attention over a ring of cached K / V rows, and the three row
// kernels of the evaluator (ring append, gather-scale, row negative log-likelihood).
//
// dle_txl_rel_attention_fwd replaces RelPartialLearnableMultiHeadAttn.forward between qkv_net and o_net
// (LanguageModeling/Transformer-XL/pytorch/mem_transformer.py:249-293): the reference builds AC and BD as two
// [bsz, n_head, qlen, klen] tensors, shifts BD with a pad / view / narrow copy (_rel_shift, :210-223), adds, scales, masks,
// takes the softmax and contracts with V -- five tensors of that shape through HBM.  Here none of them leaves the compute unit.
//
//  * one workgroup (4 wavefronts) per (batch element, head, tile of 32 queries): B x heads x ceil(qlen / 32) workgroups -- 256 at
//    the base evaluation shape (16 x 8 heads, 64 queries), 1024 at the large one (16 x 16 heads, 128 queries) on 256 CUs;
//  * the key tiles (32 keys) inside the query tile's band are dealt round-robin to the four wavefronts; a wavefront keeps its own
//    running maximum, sum and context of ALL 32 queries over its tiles (online softmax), and the four partial results are merged
//    once at the end through LDS, in a fixed order.  Tiles wholly outside the band are never visited;
//  * S^T = K a^T (v_mfma_f32_32x32x16, operands swapped): a lane holds one query's scores of a tile, the other half in lane ^ 32;
//    K rows are the A operand straight from the ring (16 bytes per lane and k step, a row is read once);
//  * the position term of a tile needs the 63 distances i + mlen - j it spans: G^T = r[dlo .. dlo + 63] b^T is two more
//    accumulators; they go to a wavefront-private fp32 LDS image [query][65] and come back skewed, G[q][q + 31 - key] -- this IS
//    _rel_shift, per tile;
//  * P^T in the accumulator layout is the B operand of context^T = V^T P^T; the V tile goes through a swizzled LDS image and is
//    read with the transposing ds_read_b64_tr_b16 in the key order the accumulator has (as csrc/attention.hip does);
//  * ring rows at or past the logical window, distances outside the table and queries past qlen are SELECTED to zero when they
//    are loaded and the scores outside the band are selected to -inf: what those rows hold never reaches an MFMA.
#include "gemm_tiles.h"
#include "mfma32_rows.h"

#define TX_D 64
#define TX_T 32                       // queries per workgroup = keys per tile
#define TX_GLD 65                     // floats per query line of the band image (odd: lanes of a half-wave hit 32 banks)
#define TX_G_FLOATS (TX_T * TX_GLD)
#define TX_LDS_BYTES (4 * TX_G_FLOATS * 4 + 4 * TX_T * TX_D * 2 + 2 * 4 * TX_T * 4)

struct TxlAttnArgs {
  const unsigned short* q;      // [B * qlen, ldq], head h at columns h * 64
  const unsigned short* u;      // [heads, 64] r_w_bias
  const unsigned short* v;      // [heads, 64] r_r_bias
  const unsigned short* kv;     // ring [B, cap, 2H]: K | V
  const unsigned short* r;      // [n_dist, H] by distance
  unsigned short* ctx;          // [B * qlen, H]
  long long ldq;
  int nh, H, qlen, mlen, klen, cap, start, n_dist, shift, nqt;
  float scale;
};

// 16-byte chunk swizzle of a [rows][64] image and the transposing fragment read of csrc/attention.hip (at_swz, at_frag_cols<true>):
// lane -> column col0 + (lane & 31); its 8 values are rows 16 ks + 4 hf + (e & 3) + 8 (e >> 2), the order in which a 32x32
// accumulator holds its rows
__device__ __forceinline__ int tx_swz(int row) {
  const int s = (row >> 1) & 7;
  return ((s & 1) << 2) | (s >> 1);
}
__device__ __forceinline__ ushort8_t tx_frag_cols(const unsigned short* t, int col0, int ks, int lane) {
  const int tg = lane >> 4, ti = lane & 15, hf = tg >> 1;
  const int chunk = ((col0 + ((tg & 1) << 4)) >> 3) + ((ti & 3) >> 1);
  ushort8_t f;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int line = ks * 16 + hf * 4 + h * 8 + (ti >> 2);
    const short4_t v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) short4_t*)(t + line * TX_D + ((chunk ^ tx_swz(line)) << 3) + ((ti & 1) << 2)));
#pragma unroll
    for (int e = 0; e < 4; ++e) f[h * 4 + e] = (unsigned short)v[e];
  }
  return f;
}

template <int DT>
__global__ __launch_bounds__(256) void txl_rel_attn_kernel(TxlAttnArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hf = lane >> 5, qi = lane & 31;
  float* G = (float*)smem_raw + wave * TX_G_FLOATS;                                     // this wavefront's band image
  unsigned short* Vt = (unsigned short*)(smem_raw + 4 * TX_G_FLOATS * 4) + wave * (TX_T * TX_D);
  float* stat = (float*)(smem_raw + 4 * TX_G_FLOATS * 4 + 4 * TX_T * TX_D * 2);        // [2][4 waves][32 queries]
  const int qt = blockIdx.x % p.nqt, bh = blockIdx.x / p.nqt, b = bh / p.nh, h = bh - b * p.nh;
  const int i0 = qt * TX_T, i = i0 + qi;
  const bool qok = i < p.qlen;
  const ushort8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const long long ring_ld = 2LL * p.H;
  const unsigned short* ring = p.kv + (long long)b * p.cap * ring_ld + h * TX_D;

  // a = round16(q + u), b = round16(q + v): the B operands (lane: query qi, columns 16 ks + 8 hf .. + 7)
  ushort8_t aq[4], bq[4];
  {
    const unsigned short* qrow = p.q + ((long long)b * p.qlen + (qok ? i : 0)) * p.ldq + h * TX_D;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int d0 = ks * 16 + hf * 8;
      const ushort8_t xl = *(const ushort8_t*)(qrow + d0);
      const ushort8_t x = qok ? xl : zero8;
      float xf[8], uf[8], vf[8];
      unpack8<DT>(x, xf);
      unpack8<DT>(*(const ushort8_t*)(p.u + h * TX_D + d0), uf);
      unpack8<DT>(*(const ushort8_t*)(p.v + h * TX_D + d0), vf);
#pragma unroll
      for (int e = 0; e < 8; ++e) { uf[e] += xf[e]; vf[e] += xf[e]; }
      aq[ks] = pack8<DT>(uf);
      bq[ks] = pack8<DT>(vf);
    }
  }

  // key tiles that meet the band of this query tile: allowed(i, j) = (i - shift < j) and (j <= i + mlen)
  const int ilast = (i0 + TX_T - 1 < p.qlen - 1) ? i0 + TX_T - 1 : p.qlen - 1;
  const long long jlo_ll = (long long)i0 - p.shift + 1;
  const int jlo = jlo_ll < 0 ? 0 : (int)jlo_ll;
  const int jhi = (ilast + p.mlen < p.klen - 1) ? ilast + p.mlen : p.klen - 1;
  const int t0 = jlo / TX_T, t1 = jhi / TX_T;
  const int iters = (t1 - t0 + 1 + 3) >> 2;

  float m_run = -INFINITY, l_run = 0.f;
  float16_t o[2];
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;

  for (int it = 0; it < iters; ++it) {
    const int t = t0 + it * 4 + wave;
    const bool act = t <= t1;                                   // wavefront-uniform; every wavefront meets both barriers
    const int j0 = t * TX_T;
    float16_t s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    if (act) {
      // every global load of the tile is issued before the first use: the addresses are valid whatever the predicates say (the
      // row index is clamped), so the loads are unconditional and what must not count is selected to zero afterwards
      const int dlo = i0 + p.mlen - j0 - (TX_T - 1);
      ushort8_t kf[4], rf[2][4], vf[4];
      const int jk = j0 + qi;
      const bool kok = jk < p.klen;
      {
        int phys = p.start + (kok ? jk : 0);
        phys = phys >= p.cap ? phys - p.cap : phys;
        const unsigned short* krow = ring + phys * ring_ld + hf * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) kf[ks] = *(const ushort8_t*)(krow + ks * 16);
      }
      bool rok[2];
#pragma unroll
      for (int eb = 0; eb < 2; ++eb) {
        const int d = dlo + eb * 32 + qi;
        rok[eb] = d >= 0 && d < p.n_dist;
        const unsigned short* rrow = p.r + (long long)(rok[eb] ? d : 0) * p.H + h * TX_D + hf * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) rf[eb][ks] = *(const ushort8_t*)(rrow + ks * 16);
      }
      bool vok[4];
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const int jv = j0 + c4 * 8 + (lane >> 3);
        vok[c4] = jv < p.klen;
        int phys = p.start + (vok[c4] ? jv : 0);
        phys = phys >= p.cap ? phys - p.cap : phys;
        vf[c4] = *(const ushort8_t*)(ring + phys * ring_ld + p.H + (lane & 7) * 8);
      }
      // S^T[key][q] = sum_d K[key][d] a[q][d]: lane's A row is key j0 + qi of the ring
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s = Mfma32x16<DT>::run(kok ? kf[ks] : zero8, aq[ks], s);
      // G^T[e][q] = sum_d r[dlo + e][d] b[q][d], e = 0 .. 63: the distances i + mlen - j of the tile are dlo + (q + 31 - key)
      float16_t g[2];
#pragma unroll
      for (int eb = 0; eb < 2; ++eb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) g[eb][r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) g[eb] = Mfma32x16<DT>::run(rok[eb] ? rf[eb][ks] : zero8, bq[ks], g[eb]);
      }
#pragma unroll
      for (int eb = 0; eb < 2; ++eb)
#pragma unroll
        for (int r = 0; r < 16; ++r) G[qi * TX_GLD + eb * 32 + rt_feat(r, hf)] = g[eb][r];
      // V tile -> swizzled [32 keys][64] image; keys at or past klen are zero whatever the ring holds there
#pragma unroll
      for (int c4 = 0; c4 < 4; ++c4) {
        const int row = c4 * 8 + (lane >> 3), c = lane & 7;
        *(ushort8_t*)(Vt + row * TX_D + ((c ^ tx_swz(row)) << 3)) = vok[c4] ? vf[c4] : zero8;
      }
    }
    __syncthreads();
    if (act) {
      float v = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kj = rt_feat(r, hf), j = j0 + kj;
        const float x = (s[r] + G[qi * TX_GLD + qi + (TX_T - 1) - kj]) * p.scale;
        const bool ok = qok && (i - p.shift < j) && (j <= i + p.mlen) && (j < p.klen);
        s[r] = ok ? x : -INFINITY;
        v = fmaxf(v, s[r]);
      }
      v = fmaxf(v, __shfl_xor(v, 32, 64));
      const float m_new = fmaxf(m_run, v);
      const float m_use = m_new == -INFINITY ? 0.f : m_new;    // a row with no allowed key so far: every exp below is 0
      const float alpha = __expf(m_run - m_use);
      float pv[16], sum = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        pv[r] = __expf(s[r] - m_use);
        sum += pv[r];
      }
      sum += __shfl_xor(sum, 32, 64);
      l_run = l_run * alpha + sum;
      m_run = m_new;
#pragma unroll
      for (int db = 0; db < 2; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
      const ushort8_t pd0 = pack8<DT>(pv), pd1 = pack8<DT>(pv + 8);
      // context^T[d][q] += sum_key V[key][d] P[q][key]
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        o[db] = Mfma32x16<DT>::run(tx_frag_cols(Vt, db * 32, 0, lane), pd0, o[db]);
        o[db] = Mfma32x16<DT>::run(tx_frag_cols(Vt, db * 32, 1, lane), pd1, o[db]);
      }
    }
    __syncthreads();
  }

  // merge the four wavefronts: total maximum and sum per query, then the scaled partial contexts through the band images
  if (hf == 0) {
    stat[wave * TX_T + qi] = m_run;
    stat[4 * TX_T + wave * TX_T + qi] = l_run;
  }
  __syncthreads();
  float mt = -INFINITY;
#pragma unroll
  for (int w = 0; w < 4; ++w) mt = fmaxf(mt, stat[w * TX_T + qi]);
  float lt = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float mw = stat[w * TX_T + qi];
    lt += mw == -INFINITY ? 0.f : stat[4 * TX_T + w * TX_T + qi] * __expf(mw - mt);
  }
  const float f = m_run == -INFINITY ? 0.f : __expf(m_run - mt) / lt;
#pragma unroll
  for (int db = 0; db < 2; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) G[qi * TX_GLD + db * 32 + rt_feat(r, hf)] = o[db][r] * f;
  __syncthreads();
  {
    const int qo = tid >> 3, c = tid & 7;
    const float* G0 = (const float*)smem_raw + qo * TX_GLD + c * 8;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = G0[e];
#pragma unroll
    for (int w = 1; w < 4; ++w)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += G0[w * TX_G_FLOATS + e];
    if (i0 + qo < p.qlen)
      *(ushort8_t*)(p.ctx + ((long long)b * p.qlen + i0 + qo) * p.H + h * TX_D + c * 8) = pack8<DT>(acc);
  }
}

static unsigned long long g_txl_attn_launches = 0;

extern "C" int dle_txl_attention_supported(int qlen, int klen, int head_dim) {
  return (head_dim == TX_D && qlen >= 1 && qlen <= 512 && klen >= qlen && klen <= 4096) ? 1 : 0;
}
extern "C" uint64_t dle_txl_attention_launch_count(void) { return __atomic_load_n(&g_txl_attn_launches, __ATOMIC_RELAXED); }

extern "C" int dle_txl_rel_attention_fwd(const void* q, int64_t ldq, const void* u, const void* v, const void* kv, const void* r,
                                         void* ctx, int B, int heads, int head_dim, int qlen, int mlen, int cap, int start,
                                         int n_dist, int shift, float scale, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "txl_rel_attention_fwd: 16-bit operands only");
  DLE_CHECK_ARG(mlen >= 0 && mlen <= 4096, "txl_rel_attention_fwd: mlen must be in [0, 4096] (got %d)", mlen);
  const int klen = mlen + qlen;
  DLE_CHECK_ARG(dle_txl_attention_supported(qlen, klen, head_dim),
                "txl_rel_attention_fwd: built for 64-wide heads, 1 <= qlen <= 512 and klen <= 4096 (got %d, %d, %d)", head_dim, qlen, klen);
  DLE_CHECK_ARG(B > 0 && heads > 0 && heads <= 4096, "txl_rel_attention_fwd: bad batch / heads");
  DLE_CHECK_ARG(cap >= klen && cap <= 4096, "txl_rel_attention_fwd: klen <= cap <= 4096 (got cap %d, klen %d)", cap, klen);
  DLE_CHECK_ARG(start >= 0 && start < cap, "txl_rel_attention_fwd: 0 <= start < cap (got %d)", start);
  DLE_CHECK_ARG(shift >= 1, "txl_rel_attention_fwd: shift >= 1 (got %d)", shift);
  DLE_CHECK_ARG(n_dist >= klen, "txl_rel_attention_fwd: the distance table has %d rows for %d keys", n_dist, klen);
  const long long H = (long long)heads * head_dim;
  DLE_CHECK_ARG(ldq >= H && (ldq & 7) == 0, "txl_rel_attention_fwd: ldq must be a multiple of 8, at least heads * 64");
  DLE_CHECK_ARG((unsigned long long)B * qlen * (unsigned long long)ldq * 2ULL < (1ULL << 32) &&
                    (unsigned long long)B * cap * 2ULL * H * 2ULL < (1ULL << 32) && (unsigned long long)n_dist * H * 2ULL < (1ULL << 32),
                "txl_rel_attention_fwd: an operand of 4 GiB or more (32-bit offsets)");
  const int nqt = (qlen + TX_T - 1) / TX_T;
  DLE_CHECK_ARG((long long)B * heads * nqt < 0x7FFFFFFFLL, "txl_rel_attention_fwd: grid too large");
  DLE_CHECK_ARG(q && u && v && kv && r && ctx, "txl_rel_attention_fwd: null pointer");
  DLE_CHECK_ARG(((((uintptr_t)q) | ((uintptr_t)u) | ((uintptr_t)v) | ((uintptr_t)kv) | ((uintptr_t)r) | ((uintptr_t)ctx)) & 15) == 0,
                "txl_rel_attention_fwd: tensors must be 16-byte aligned");
  TxlAttnArgs a = {};
  a.q = (const unsigned short*)q; a.u = (const unsigned short*)u; a.v = (const unsigned short*)v;
  a.kv = (const unsigned short*)kv; a.r = (const unsigned short*)r; a.ctx = (unsigned short*)ctx;
  a.ldq = ldq; a.nh = heads; a.H = (int)H; a.qlen = qlen; a.mlen = mlen; a.klen = klen; a.cap = cap; a.start = start;
  a.n_dist = n_dist; a.shift = shift; a.nqt = nqt; a.scale = scale;
  const dim3 grid(B * heads * nqt);
  if (dtype == DLE_F16) DLE_LAUNCH_LDS((txl_rel_attn_kernel<DLE_F16>), grid, dim3(256), TX_LDS_BYTES, stream, a);
  else DLE_LAUNCH_LDS((txl_rel_attn_kernel<DLE_BF16>), grid, dim3(256), TX_LDS_BYTES, stream, a);
  DLE_LAUNCH_CHECK();
  __atomic_fetch_add(&g_txl_attn_launches, 1, __ATOMIC_RELAXED);
  return 0;
}

// ---- ring append: the K | V thirds of the segment's projection are one contiguous run of 2H elements per row -----------------
__global__ __launch_bounds__(256) void txl_kv_append_kernel(const ushort8_t* qkv, ushort8_t* kv, int qlen, int mlen, int cap,
                                                            int start, int c8, int ld8, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % c8);
  const long long row = idx / c8;
  const int t = (int)(row % qlen);
  const long long b = row / qlen;
  int phys = start + mlen + t;
  phys = phys >= cap ? phys - cap : phys;
  kv[(b * cap + phys) * c8 + c] = qkv[row * ld8 + (c8 >> 1) + c];
}

extern "C" int dle_txl_kv_append(const void* qkv, int64_t ld, void* kv, int B, int H, int qlen, int mlen, int cap, int start,
                                 int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "txl_kv_append: 16-bit operands only");
  DLE_CHECK_ARG(B > 0 && H > 0 && (H & 7) == 0, "txl_kv_append: bad batch, or H not a multiple of 8");
  DLE_CHECK_ARG(qlen >= 1 && mlen >= 0 && mlen <= 4096 && qlen <= 4096 && mlen + qlen <= cap && cap <= 4096,
                "txl_kv_append: mlen + qlen <= cap <= 4096 (got %d, %d, %d)", mlen, qlen, cap);
  DLE_CHECK_ARG(start >= 0 && start < cap, "txl_kv_append: 0 <= start < cap (got %d)", start);
  DLE_CHECK_ARG(ld >= 3LL * H && (ld & 7) == 0, "txl_kv_append: ld must be a multiple of 8, at least 3H");
  DLE_CHECK_ARG(qkv && kv, "txl_kv_append: null pointer");
  DLE_CHECK_ARG(((((uintptr_t)qkv) | ((uintptr_t)kv)) & 15) == 0, "txl_kv_append: tensors must be 16-byte aligned");
  const int c8 = 2 * H / 8;
  const long long total = (long long)B * qlen * c8;
  DLE_CHECK_ARG((total + 255) / 256 < 0x7FFFFFFFLL, "txl_kv_append: grid too large");
  hipLaunchKernelGGL(txl_kv_append_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const ushort8_t*)qkv,
                     (ushort8_t*)kv, qlen, mlen, cap, start, c8, (int)(ld / 8), total);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- dst[dst_idx[r], :] = round16(scale * float(src[src_idx[r], :])) ------------------------------------------------------------
// A row whose source or destination index lies outside its tensor is skipped: a wrong table touches nothing outside src / dst.
template <int DT>
__global__ __launch_bounds__(256) void rows_gather_scale_kernel(const unsigned short* src, const int* src_idx, unsigned short* dst,
                                                                const int* dst_idx, long long rows, int w8, long long ld_src,
                                                                long long ld_dst, long long n_src, long long n_dst, float scale) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= rows * w8) return;
  const int c = (int)(idx % w8);
  const long long row = idx / w8;
  const long long sr = src_idx ? (long long)src_idx[row] : row, dr = dst_idx ? (long long)dst_idx[row] : row;
  if (sr < 0 || sr >= n_src || dr < 0 || dr >= n_dst) return;
  float x[8];
  unpack8<DT>(*(const ushort8_t*)(src + sr * ld_src + c * 8), x);
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] *= scale;
  *(ushort8_t*)(dst + dr * ld_dst + c * 8) = pack8<DT>(x);
}

extern "C" int dle_rows_gather_scale(const void* src, const int32_t* src_idx, void* dst, const int32_t* dst_idx, int64_t rows,
                                     int width, int64_t ld_src, int64_t ld_dst, int64_t n_src_rows, int64_t n_dst_rows,
                                     float scale, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "rows_gather_scale: 16-bit operands only");
  DLE_CHECK_ARG(rows >= 0 && width > 0 && (width & 7) == 0, "rows_gather_scale: width must be a positive multiple of 8");
  DLE_CHECK_ARG(ld_src >= width && ld_dst >= width && (ld_src & 7) == 0 && (ld_dst & 7) == 0,
                "rows_gather_scale: row pitches must be multiples of 8, at least the width");
  DLE_CHECK_ARG(n_src_rows > 0 && n_dst_rows > 0, "rows_gather_scale: empty source or destination");
  DLE_CHECK_ARG(src_idx || rows <= n_src_rows, "rows_gather_scale: %lld rows out of a source of %lld", (long long)rows, (long long)n_src_rows);
  DLE_CHECK_ARG(dst_idx || rows <= n_dst_rows, "rows_gather_scale: %lld rows into a destination of %lld", (long long)rows, (long long)n_dst_rows);
  DLE_CHECK_ARG(src && dst, "rows_gather_scale: null pointer");
  DLE_CHECK_ARG(((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0, "rows_gather_scale: tensors must be 16-byte aligned");
  if (rows == 0) return 0;
  const long long total = rows * (width / 8);
  DLE_CHECK_ARG((total + 255) / 256 < 0x7FFFFFFFLL, "rows_gather_scale: grid too large");
  const dim3 grid((unsigned)((total + 255) / 256));
  if (dtype == DLE_F16)
    hipLaunchKernelGGL(rows_gather_scale_kernel<DLE_F16>, grid, dim3(256), 0, stream, (const unsigned short*)src, src_idx,
                       (unsigned short*)dst, dst_idx, rows, width / 8, ld_src, ld_dst, n_src_rows, n_dst_rows, scale);
  else
    hipLaunchKernelGGL(rows_gather_scale_kernel<DLE_BF16>, grid, dim3(256), 0, stream, (const unsigned short*)src, src_idx,
                       (unsigned short*)dst, dst_idx, rows, width / 8, ld_src, ld_dst, n_src_rows, n_dst_rows, scale);
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- nll[pos[r]] (+)= logsumexp(logits[r, :n_classes]) - logits[r, target[r]] -----------------------------------------------------
// One workgroup per row, two passes over the row (maximum, then the sum of exp); a row whose target or position is out of range
// writes nothing.
__global__ __launch_bounds__(256) void row_nll_kernel(const float* logits, long long ld, const int* target, const int* pos, float* nll,
                                                      int n_classes, long long n_out, int accumulate) {
  __shared__ float red[16];
  const long long row = blockIdx.x;
  const float* x = logits + row * ld;
  float m = -INFINITY;
  for (int c = threadIdx.x; c < n_classes; c += 256) m = fmaxf(m, x[c]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s = 0.f;
  for (int c = threadIdx.x; c < n_classes; c += 256) s += __expf(x[c] - m);
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const int t = target[row];
    const long long o = pos ? (long long)pos[row] : row;
    if (t >= 0 && t < n_classes && o >= 0 && o < n_out) {
      const float v = m + logf(s) - x[t];
      nll[o] = accumulate ? nll[o] + v : v;
    }
  }
}

extern "C" int dle_row_nll(const float* logits, int64_t ld, const int32_t* target, const int32_t* pos, float* nll, int64_t rows,
                           int n_classes, int64_t n_out, int accumulate, hipStream_t stream) {
  DLE_CHECK_ARG(rows >= 0 && rows < 0x7FFFFFFFLL, "row_nll: bad row count");
  DLE_CHECK_ARG(n_classes >= 1 && n_classes <= 160003, "row_nll: 1 <= n_classes <= 160003 (got %d)", n_classes);
  DLE_CHECK_ARG(ld >= n_classes, "row_nll: ld is smaller than n_classes");
  DLE_CHECK_ARG(n_out > 0 && (pos || rows <= n_out), "row_nll: %lld rows into an output of %lld", (long long)rows, (long long)n_out);
  DLE_CHECK_ARG(logits && target && nll, "row_nll: null pointer");
  if (rows == 0) return 0;
  hipLaunchKernelGGL(row_nll_kernel, dim3((unsigned)rows), dim3(256), 0, stream, logits, (long long)ld, target, pos, nll, n_classes,
                     (long long)n_out, accumulate);
  DLE_LAUNCH_CHECK();
  return 0;
}
