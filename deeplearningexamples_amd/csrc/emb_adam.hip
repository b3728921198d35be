// Duplicate-free sparse Adam on the joint embedding table for gfx950 (DLRM --Adam_embedding_optimizer).
//
// Replaces torch.optim.SparseAdam over the joint table (DLRM/dlrm/scripts/main.py:479-482, the math of
// torch.optim._functional.sparse_adam): the COO gradient (one entry per lookup) is coalesced -- duplicates summed -- and every
// looked-up row, INCLUDING one whose summed gradient is exactly 0, takes
//   m += (1 - b1) (g - m);  v += (1 - b2) (g^2 - v);  w -= lr sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)
// while rows nobody looked up keep w, m and v bit for bit.  Adam is not linear in g, so the per-lookup atomic scatter of the SGD
// path is no option even in principle: each touched row is updated ONCE, from the fp32 sum of its gradients, with no float
// atomics in global memory.  The sums are formed by the machinery of the duplicate-free SGD (csrc/embedding.hip), by table class:
//   * small tables (rows * dim * 4 <= 64 KiB, the SGD's "small" set): per (table, batch slice) fp32 partial blocks in scratch --
//     the one-hot MFMA segment sum of csrc/emb_onehot.hip (dim 128, 16-bit gradients) or an LDS-resident image here -- plus a
//     "touched" byte per row (a looked-up row whose sum is 0 is told apart from one nobody looked up); a fold pass adds a row's
//     partials in slice order and applies Adam to the touched rows.  A 4-row table that takes every sample of the batch is
//     spread over up to 64 slices, not one chain;
//   * mid tables (<= 4096 rows, dim <= 128): eight lists per row (one per residue of the sample index), each list's head writes
//     its partial sum to scratch, a fold pass adds the eight in residue order and applies Adam;
//   * large tables: one list per row; its head sums the duplicates and applies Adam to the w / m / v rows in place.
// head[] (int32 per joint row) is the SGD's persistent workspace: all -1 on entry and on exit.
// Algorithmic bytes per call: touched rows x 6 x dim x 4 (w, m, v read and written) + lookups x dim x gradient size + 8 B row id.
#include "common.h"

#define EA_SMALL_LDS_BYTES (64 * 1024)    // = DLE_EMB_SMALL_LDS_BYTES of embedding.hip (the SGD's "small" rule)
#define EA_MAX_SMALL 64
#define EA_MID_S 8                        // lists per mid-table row
#define EA_MID_ROWS 4096
#define EA_MID_TABLES 16
#define EA_MAX_TABLES 128
#define EA_LDS_SLICE 512                  // samples per workgroup of the LDS form
#define EA_MAX_SLICES 64

template <int IDT> struct EaIn4;
template <> struct EaIn4<DLE_F32> {
  typedef float4_t V;
  static __device__ __forceinline__ float4_t up(V v) { return v; }
};
template <> struct EaIn4<DLE_F16> {
  typedef ushort4_t V;
  static __device__ __forceinline__ float4_t up(V v) {
    float4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = Elem<DLE_F16>::to_f32(v[i]);
    return o;
  }
};
template <> struct EaIn4<DLE_BF16> {
  typedef ushort4_t V;
  static __device__ __forceinline__ float4_t up(V v) {
    float4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = Elem<DLE_BF16>::to_f32(v[i]);
    return o;
  }
};

// per-call constants of the update; step_size = lr sqrt(1 - b2^t) / (1 - b1^t) in double, as sparse_adam forms it on the host
struct EaHyper {
  const float* lr_dev;
  float lr_host;
  const float* gmul;                      // gradient multiplier (loss-scale inverse [/ world]); NULL: 1
  const float* skip;                      // found_inf: != 0 -> nothing is written
  const int* step;                        // t of this update (advanced by the caller)
  float om1, om2, eps;                    // 1 - beta1, 1 - beta2 (passed as such: 1 - 0.999f is 1.3e-5 off 1e-3)
};
struct EaCoef {
  float om1, om2, eps, neg_step, gmul;
};
__device__ __forceinline__ EaCoef ea_coef(const EaHyper& h) {
  EaCoef c;
  const double t = (double)*h.step;
  const double lr = h.lr_dev ? (double)*h.lr_dev : (double)h.lr_host;
  c.neg_step = (float)(-lr * sqrt(1.0 - pow(1.0 - (double)h.om2, t)) / (1.0 - pow(1.0 - (double)h.om1, t)));
  c.om1 = h.om1;
  c.om2 = h.om2;
  c.eps = h.eps;
  c.gmul = h.gmul ? *h.gmul : 1.0f;
  return c;
}
__device__ __forceinline__ bool ea_skipped(const EaHyper& h) { return h.skip && *h.skip != 0.0f; }

// the Adam epilogue on 4 consecutive elements of one row: w, m, v read and written together
__device__ __forceinline__ void ea_update4(float* w, float* m, float* v, float4_t s, const EaCoef& c) {
  float4_t wv = *(const float4_t*)w, mv = *(const float4_t*)m, vv = *(const float4_t*)v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float g = s[j] * c.gmul;
    const float mn = mv[j] + (g - mv[j]) * c.om1;
    const float vn = vv[j] + (g * g - vv[j]) * c.om2;
    mv[j] = mn;
    vv[j] = vn;
    wv[j] = wv[j] + c.neg_step * (mn / (sqrtf(vn) + c.eps));
  }
  *(float4_t*)w = wv;
  *(float4_t*)m = mv;
  *(float4_t*)v = vv;
}

struct EaTable {
  float* w;
  float* m;
  float* v;
};

// ------------------------------------------------------------------------------------------------ small tables
struct EaSmall {
  int n;                                  // small tables
  int t[EA_MAX_SMALL];                    // column index
  int rows[EA_MAX_SMALL];
  int moff[EA_MAX_SMALL];                 // first row of the table in the touched bytes (and in the fold's row numbering)
  long long base[EA_MAX_SMALL];           // first joint row
  long long pbase[EA_MAX_SMALL];          // first float of the table's partial blocks in the scratch
  long long sstride[EA_MAX_SMALL];        // floats between two slices' blocks
  int rstride[EA_MAX_SMALL];              // floats between two rows of a block
  int slices[EA_MAX_SMALL];
  int lds_k[EA_MAX_SMALL];                // the tables the LDS form sums (workgroup j / slices takes table lds_k[j])
  int rows_total;
};

// touched[moff[k] + r] = 1 for every lookup of a small table (plain byte stores of one value: no atomics; a loaded 1 skips the store)
__global__ __launch_bounds__(256) void emb_adam_mark(const long long* __restrict__ rows, unsigned char* __restrict__ touched,
                                                     EaSmall sm, long long batch, int T, const float* __restrict__ skip) {
  if (skip && *skip != 0.0f) return;
  const long long n = batch * sm.n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long b = i / sm.n;
    const int k = (int)(i - b * sm.n);
    unsigned char* p = touched + sm.moff[k] + (rows[b * T + sm.t[k]] - sm.base[k]);
    if (*p == 0) *p = 1;
  }
}

// LDS form: workgroup (table, slice) sums its slice of the batch into an LDS image [rows][dim] (ds_add_f32) and writes it out as
// ONE partial block; a half-wavefront takes a sample, its lanes 16-byte column chunks
template <int IDT>
__global__ __launch_bounds__(256) void emb_adam_small_partial(const long long* __restrict__ rows,
                                                              const typename EaIn4<IDT>::V* __restrict__ grad, float* __restrict__ ws,
                                                              EaSmall sm, long long batch, int T,
                                                              int D4, long long g_bstride4, int slices, const float* __restrict__ skip) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  if (skip && *skip != 0.0f) return;
  float* acc = (float*)smem_raw;
  const int j = blockIdx.x / slices, sl = blockIdx.x - j * slices;
  const int k = sm.lds_k[j];
  const int t = sm.t[k], nrows = sm.rows[k];
  const long long base = sm.base[k];
  const int D = D4 * 4;
  for (int q = threadIdx.x; q < nrows * D; q += 256) acc[q] = 0.f;
  __syncthreads();
  const long long per = (batch + slices - 1) / slices;
  const long long b0 = (long long)sl * per;
  const long long b1 = b0 + per < batch ? b0 + per : batch;
  const int hw = threadIdx.x >> 5, l = threadIdx.x & 31;
  for (long long b = b0 + hw; b < b1; b += 8) {
    const long long r = rows[b * T + t] - base;
    const long long goff = b * g_bstride4 + (long long)t * D4;
    for (int c = l; c < D4; c += 32) {
      const float4_t g = EaIn4<IDT>::up(grad[goff + c]);
      float* a = acc + r * D + c * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) atomicAdd(a + e, g[e]);   // ds_add_f32 (LDS)
    }
  }
  __syncthreads();
  float* out = ws + sm.pbase[k] + (long long)sl * sm.sstride[k];
  for (int q = threadIdx.x; q < nrows * D; q += 256) out[q] = acc[q];
}

// fold: a half-wavefront per small-table row; a touched row adds its partials in slice order and takes the Adam step
__global__ __launch_bounds__(256) void emb_adam_small_fold(EaTable tb, const float* __restrict__ ws,
                                                           const unsigned char* __restrict__ touched, EaSmall sm, int D4, EaHyper h) {
  if (ea_skipped(h)) return;
  const int q = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 5), l = threadIdx.x & 31;
  if (q >= sm.rows_total || !touched[q]) return;
  int k = 0;
  while (k + 1 < sm.n && q >= sm.moff[k + 1]) ++k;
  const int r = q - sm.moff[k];
  const EaCoef c = ea_coef(h);
  const long long row = sm.base[k] + r;
  const int ns = sm.slices[k];
  const long long ss = sm.sstride[k];
  for (int cc = l; cc < D4; cc += 32) {
    const float* src = ws + sm.pbase[k] + (long long)r * sm.rstride[k] + cc * 4;
    float4_t s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
    int s = 0;
    for (; s + 4 <= ns; s += 4) {
      s0 += *(const float4_t*)(src + (s + 0) * ss);
      s1 += *(const float4_t*)(src + (s + 1) * ss);
      s2 += *(const float4_t*)(src + (s + 2) * ss);
      s3 += *(const float4_t*)(src + (s + 3) * ss);
    }
    for (; s < ns; ++s) s0 += *(const float4_t*)(src + s * ss);
    const float4_t sum = (s0 + s1) + (s2 + s3);
    const long long o = row * (D4 * 4) + cc * 4;
    ea_update4(tb.w + o, tb.m + o, tb.v + o, sum, c);
  }
}

// ------------------------------------------------------------------------------------------------ list tables (mid + large)
struct EaLists {
  int nl, T;                              // list tables, all tables
  unsigned mul_nl, shr_nl, mul_t, shr_t;  // 32-bit multiply-shift divisions by nl and by T
  unsigned char t[EA_MAX_TABLES];         // column of list slot k
  int moff[EA_MAX_TABLES];                // mid tables: first row in the sub-list heads / partials, -1: large table
  long long mbase[EA_MAX_TABLES];         // mid tables: first joint row
  int* mhead;                             // [mid rows * EA_MID_S]: -1 on entry (memset per call); a head that wrote its partial: -2
  float* mpart;                           // [mid rows * EA_MID_S][dim]
};
static void ea_make_div(int d, unsigned& mul, unsigned& shr) {
  if (d <= 1) { mul = 0; shr = 0; return; }
  unsigned lg = 0;
  while ((1u << lg) < (unsigned)d) ++lg;
  const unsigned p = 31 + lg;
  mul = (unsigned)(((1ull << p) + (unsigned)d - 1) / (unsigned)d);
  shr = p - 32;
}
__device__ __forceinline__ int ea_div(int n, int d, unsigned mul, unsigned shr) {
  return d <= 1 ? n : (int)(__umulhi((unsigned)n, mul) >> shr);
}

// pass 1: thread every lookup of a list table into its row's list (head[row] <- atomicExch, next[i] <- previous head)
__global__ __launch_bounds__(256) void emb_adam_link(const long long* __restrict__ rows, int* __restrict__ head, int* __restrict__ next,
                                                     int n_lookups, EaLists lm, const float* __restrict__ skip) {
  __shared__ unsigned char t_lds[EA_MAX_TABLES];
  __shared__ int moff_lds[EA_MAX_TABLES];
  __shared__ long long mbase_lds[EA_MAX_TABLES];
  if (skip && *skip != 0.0f) return;
  if (threadIdx.x < EA_MAX_TABLES) {
    t_lds[threadIdx.x] = lm.t[threadIdx.x];
    moff_lds[threadIdx.x] = lm.moff[threadIdx.x];
    mbase_lds[threadIdx.x] = lm.mbase[threadIdx.x];
  }
  __syncthreads();
  for (int i = (int)(blockIdx.x * blockDim.x + threadIdx.x); i < n_lookups; i += (int)(gridDim.x * blockDim.x)) {
    const int b = ea_div(i, lm.nl, lm.mul_nl, lm.shr_nl);
    const int k = i - b * lm.nl;
    const int li = b * lm.T + t_lds[k];
    const long long r = rows[li];
    const int mo = moff_lds[k];
    int* slot = mo >= 0 ? lm.mhead + ((long long)(mo + (int)(r - mbase_lds[k])) * EA_MID_S + (b & (EA_MID_S - 1))) : head + r;
    next[li] = atomicExch(slot, li);
  }
}

// pass 2: the head of each list sums its chain in fp32; a large table's head applies Adam to its row and restores head[row] = -1,
// a mid table's head leaves its partial sum for the fold.  Half-wavefront per lookup, lanes = 16-byte column chunks (dim > 128: the
// chain is walked once per 128 columns).  The batch is walked from its end: a list's head is the lookup linked last.
template <int IDT>
__global__ __launch_bounds__(256) void emb_adam_lists(EaTable tb, const long long* __restrict__ rows,
                                                      const typename EaIn4<IDT>::V* __restrict__ grad, int* __restrict__ head,
                                                      const int* __restrict__ next, int n, EaLists lm, int D4, long long g_bstride4,
                                                      EaHyper h) {
  __shared__ unsigned char t_lds[EA_MAX_TABLES];
  __shared__ int moff_lds[EA_MAX_TABLES];
  __shared__ long long mbase_lds[EA_MAX_TABLES];
  if (ea_skipped(h)) return;
  if (threadIdx.x < EA_MAX_TABLES) {
    t_lds[threadIdx.x] = lm.t[threadIdx.x];
    moff_lds[threadIdx.x] = lm.moff[threadIdx.x];
    mbase_lds[threadIdx.x] = lm.mbase[threadIdx.x];
  }
  __syncthreads();
  const EaCoef c = ea_coef(h);
  const int T = lm.T;
  const int sub = (threadIdx.x & 63) >> 5, l = threadIdx.x & 31;
  const int wave_id = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  const int n_waves = (int)(gridDim.x * (blockDim.x >> 6));
  constexpr int U = 2;
  for (int base = wave_id * (2 * U); base < n; base += n_waves * (2 * U)) {
    int iu[U], ms[U], hd[U];
    long long r[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = n - 1 - (base + 2 * u + sub);
      ok[u] = i >= 0;
      const int ic = i >= 0 ? i : 0;
      const int b = ea_div(ic, lm.nl, lm.mul_nl, lm.shr_nl);
      const int k = ic - b * lm.nl;
      iu[u] = b * T + t_lds[k];
      r[u] = rows[iu[u]];
      const int mo = moff_lds[k];
      ms[u] = mo >= 0 ? (mo + (int)(r[u] - mbase_lds[k])) * EA_MID_S + (b & (EA_MID_S - 1)) : -1;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) hd[u] = *(ms[u] >= 0 ? (const int*)lm.mhead + ms[u] : (const int*)head + r[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (!ok[u] || hd[u] != iu[u]) continue;        // not the list head: the head does the work
      for (int cc = l; cc < D4; cc += 32) {
        float4_t s = {0.f, 0.f, 0.f, 0.f};
        int j = iu[u];
        while (j >= 0) {
          const int jb = ea_div(j, T, lm.mul_t, lm.shr_t);
          s += EaIn4<IDT>::up(grad[jb * g_bstride4 + (long long)(j - jb * T) * D4 + cc]);
          j = next[j];
        }
        if (ms[u] >= 0) {                            // mid table (D4 <= 32): this list's share of the row's sum
          ((float4_t*)(lm.mpart + (long long)ms[u] * (D4 * 4)))[cc] = s;
        } else {
          const long long o = r[u] * (D4 * 4) + cc * 4;
          ea_update4(tb.w + o, tb.m + o, tb.v + o, s, c);
        }
      }
      if (l == 0) {
        if (ms[u] >= 0) lm.mhead[ms[u]] = -2;
        else head[r[u]] = -1;                        // restore the workspace invariant
      }
    }
  }
}

struct EaMidFold {
  int n, rows_total;
  int off[EA_MID_TABLES];
  long long base[EA_MID_TABLES];
};

// pass 3 (mid tables): a half-wavefront per row adds the partials of its written lists in residue order; a row with at least one
// written list (= looked up, whatever its sum) takes the Adam step
__global__ __launch_bounds__(256) void emb_adam_mid_fold(EaTable tb, const int* __restrict__ mhead, const float* __restrict__ mpart,
                                                         EaMidFold mf, int D4, EaHyper h) {
  if (ea_skipped(h)) return;
  const int q = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 5), l = threadIdx.x & 31;
  if (q >= mf.rows_total || l >= D4) return;
  int j = 0;
  while (j + 1 < mf.n && q >= mf.off[j + 1]) ++j;
  const long long row = mf.base[j] + (q - mf.off[j]);
  float4_t sum = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
#pragma unroll
  for (int s = 0; s < EA_MID_S; ++s) {
    if (mhead[q * EA_MID_S + s] == -2) {             // (unwritten partials are never read)
      sum += ((const float4_t*)(mpart + ((long long)q * EA_MID_S + s) * (D4 * 4)))[l];
      any = true;
    }
  }
  if (!any) return;
  const EaCoef c = ea_coef(h);
  const long long o = row * (D4 * 4) + l * 4;
  ea_update4(tb.w + o, tb.m + o, tb.v + o, sum, c);
}

// ------------------------------------------------------------------------------------------------ host side
static long long ea_align(long long v) { return (v + 255) / 256 * 256; }

// Scratch layout: [one-hot partials of the small tables (dim 128) | LDS-form partials of every small table | touched bytes |
// mid sub-list heads | mid partials], each part 256-byte aligned.  Both partial areas are reserved: which
// form a small table takes depends on the gradient's dtype and alignment, known at the call.
struct EaPlan {
  int n_small, n_mid, mid_rows, small_rows, lds_slices;
  long long small_rows_dim;               // sum over small tables of rows * dim
  long long oh_off, lds_off, touched_off, mhead_off, mpart_off, total;
};
static int ea_lds_slices(int64_t batch) {
  long long s = (batch + EA_LDS_SLICE - 1) / EA_LDS_SLICE;
  if (s > EA_MAX_SLICES) s = EA_MAX_SLICES;
  return (int)(s < 1 ? 1 : s);
}
static bool ea_is_small(long long r, int dim, int n_small) { return r * dim * 4 <= EA_SMALL_LDS_BYTES && n_small < EA_MAX_SMALL; }
static bool ea_is_mid(long long r, int dim, int n_mid) { return r <= EA_MID_ROWS && dim <= 128 && n_mid < EA_MID_TABLES; }

static EaPlan ea_plan(const int64_t* off, int tables, int dim, int64_t batch) {
  EaPlan pl = {};
  for (int t = 0; t < tables; ++t) {
    const long long r = off[t + 1] - off[t];
    if (ea_is_small(r, dim, pl.n_small)) {
      ++pl.n_small;
      pl.small_rows += (int)r;
      pl.small_rows_dim += r * dim;
    } else if (ea_is_mid(r, dim, pl.n_mid)) {
      ++pl.n_mid;
      pl.mid_rows += (int)r;
    }
  }
  pl.lds_slices = ea_lds_slices(batch);
  pl.oh_off = 0;
  const long long oh_bytes = dim == 128 ? dle_emb_onehot_workspace_bytes(pl.n_small, batch) : 0;
  pl.lds_off = ea_align(pl.oh_off + oh_bytes);
  pl.touched_off = ea_align(pl.lds_off + (long long)pl.lds_slices * pl.small_rows_dim * 4);
  pl.mhead_off = ea_align(pl.touched_off + pl.small_rows);
  pl.mpart_off = ea_align(pl.mhead_off + (long long)pl.mid_rows * EA_MID_S * 4);
  pl.total = pl.mpart_off + (long long)pl.mid_rows * EA_MID_S * dim * 4;
  return pl;
}

extern "C" int64_t dle_emb_adam_workspace_bytes(const int64_t* table_offsets_host, int tables, int dim, int64_t batch) {
  if (!table_offsets_host || tables <= 0 || dim <= 0 || batch <= 0) return 0;
  return ea_plan(table_offsets_host, tables, dim, batch).total;
}

static int ea_grid(long long work, int per_block) {
  long long g = (work + per_block - 1) / per_block;
  if (g > 256 * 8) g = 256 * 8;
  return (int)(g < 1 ? 1 : g);
}

extern "C" int dle_emb_adam_dedup_ws(float* weight, float* exp_avg, float* exp_avg_sq, const int64_t* rows, const void* grad,
                                     int32_t* head, int32_t* next, const int64_t* table_offsets_host, const float* lr_dev,
                                     float lr_host, const float* grad_mul_dev, const float* skip_flag_dev, const int32_t* step_dev,
                                     float one_minus_beta1, float one_minus_beta2, float eps, int64_t batch, int tables, int dim,
                                     int64_t grad_batch_stride, int grad_dtype, void* ws, int64_t ws_bytes, hipStream_t stream) {
  DLE_CHECK_ARG(dim > 0 && dim % 4 == 0 && tables > 0, "emb_adam_dedup: bad shape (dim %d must be a multiple of 4)", dim);
  DLE_CHECK_ARG(tables <= EA_MAX_TABLES, "emb_adam_dedup: at most %d tables per joint matrix (got %d)", EA_MAX_TABLES, tables);
  if (batch == 0) return 0;
  DLE_CHECK_ARG(weight && exp_avg && exp_avg_sq && rows && grad && head && next && table_offsets_host && step_dev && ws,
                "emb_adam_dedup: null pointer");
  DLE_CHECK_ARG(batch * tables < 2147483647LL, "emb_adam_dedup: more than 2^31 lookups per call");
  DLE_CHECK_ARG(grad_dtype == DLE_F32 || grad_dtype == DLE_F16 || grad_dtype == DLE_BF16, "emb_adam_dedup: bad dtype %d", grad_dtype);
  if (grad_batch_stride == 0) grad_batch_stride = (int64_t)tables * dim;
  DLE_CHECK_ARG(grad_batch_stride % 4 == 0 && grad_batch_stride >= (int64_t)tables * dim,
                "emb_adam_dedup: grad batch stride must be a multiple of 4 and >= tables * dim");
  DLE_CHECK_ARG((((uintptr_t)weight | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0 && (((uintptr_t)grad) & 7) == 0 &&
                (((uintptr_t)ws) & 255) == 0, "emb_adam_dedup: misaligned table / gradient / scratch");
  const EaPlan pl = ea_plan(table_offsets_host, tables, dim, batch);
  DLE_CHECK_ARG(ws_bytes >= pl.total, "emb_adam_dedup: scratch of %lld bytes, %lld needed", (long long)ws_bytes, pl.total);
  const int D4 = dim / 4;
  const long long gs4 = grad_batch_stride / 4;
  char* wsb = (char*)ws;
  EaTable tb = {weight, exp_avg, exp_avg_sq};
  EaHyper hy = {lr_dev, lr_host, grad_mul_dev, skip_flag_dev, step_dev, one_minus_beta1, one_minus_beta2, eps};

  // ---- classes (the rules of dle_emb_sgd_dedup_ws)
  EaSmall sm;
  sm.n = 0; sm.rows_total = 0;
  EaLists lm;
  lm.nl = 0; lm.T = tables;
  for (int i = 0; i < EA_MAX_TABLES; ++i) { lm.t[i] = 0; lm.moff[i] = -1; lm.mbase[i] = 0; }
  EaMidFold mf;
  mf.n = 0; mf.rows_total = 0;
  for (int t = 0; t < tables; ++t) {
    const long long r = table_offsets_host[t + 1] - table_offsets_host[t];
    if (ea_is_small(r, dim, sm.n)) {
      const int k = sm.n++;
      sm.t[k] = t; sm.rows[k] = (int)r; sm.moff[k] = sm.rows_total; sm.base[k] = table_offsets_host[t];
      sm.rows_total += (int)r;
      continue;
    }
    const int k = lm.nl++;
    lm.t[k] = (unsigned char)t;
    if (ea_is_mid(r, dim, mf.n)) {
      lm.moff[k] = mf.rows_total; lm.mbase[k] = table_offsets_host[t];
      mf.off[mf.n] = mf.rows_total; mf.base[mf.n] = table_offsets_host[t];
      ++mf.n;
      mf.rows_total += (int)r;
    }
  }
  ea_make_div(lm.nl, lm.mul_nl, lm.shr_nl);
  ea_make_div(tables, lm.mul_t, lm.shr_t);

  // ---- small tables: partial blocks + touched bytes, then the fold
  if (sm.n > 0) {
    hipError_t e = hipMemsetAsync(wsb + pl.touched_off, 0, (size_t)sm.rows_total, stream);
    if (e != hipSuccess) { dle_set_error("emb_adam_dedup memset: %s", hipGetErrorString(e)); return (int)e; }
    hipLaunchKernelGGL(emb_adam_mark, dim3(ea_grid((long long)batch * sm.n, 256)), dim3(256), 0, stream, (const long long*)rows,
                       (unsigned char*)(wsb + pl.touched_off), sm, (long long)batch, tables, skip_flag_dev);
    DLE_LAUNCH_CHECK();
    int oh_slices = 0;
    bool onehot = false;
    if (dim == 128 && grad_dtype != DLE_F32) {
      static_assert(sizeof(long long) == sizeof(int64_t), "table bases are passed as int64");
      DLE_TRY(dle_emb_onehot_partials(rows, grad, skip_flag_dev, sm.t, (const int64_t*)sm.base, sm.rows, sm.n, batch, tables, dim,
                                      grad_batch_stride, grad_dtype, wsb + pl.oh_off, pl.lds_off - pl.oh_off, &oh_slices, stream),
              onehot = true);
    }
    int n_lds = 0, max_rows = 0;
    long long lds_pos = pl.lds_off / 4;
    for (int k = 0; k < sm.n; ++k) {
      if (onehot) {                                   // the one-hot kernel's layout: [k][slice][128 rows][128]
        sm.slices[k] = oh_slices;
        sm.pbase[k] = (pl.oh_off / 4) + (long long)k * oh_slices * 128 * 128;
        sm.sstride[k] = 128 * 128;
        sm.rstride[k] = 128;
      } else {
        sm.slices[k] = pl.lds_slices;
        sm.pbase[k] = lds_pos;
        sm.sstride[k] = (long long)sm.rows[k] * dim;
        sm.rstride[k] = dim;
        lds_pos += (long long)pl.lds_slices * sm.rows[k] * dim;
        sm.lds_k[n_lds++] = k;
        if (sm.rows[k] > max_rows) max_rows = sm.rows[k];
      }
    }
    if (n_lds > 0) {
      const size_t lds = (size_t)max_rows * dim * 4;
#define GO(IDT, VT) hipLaunchKernelGGL(emb_adam_small_partial<IDT>, dim3(n_lds * pl.lds_slices), dim3(256), lds, stream, (const long long*)rows, (const VT*)grad, (float*)ws, sm, (long long)batch, tables, D4, gs4, pl.lds_slices, skip_flag_dev)
      if (grad_dtype == DLE_F32) GO(DLE_F32, float4_t);
      else if (grad_dtype == DLE_F16) GO(DLE_F16, ushort4_t);
      else GO(DLE_BF16, ushort4_t);
#undef GO
      DLE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(emb_adam_small_fold, dim3((sm.rows_total * 32 + 255) / 256), dim3(256), 0, stream, tb, (const float*)ws,
                       (const unsigned char*)(wsb + pl.touched_off), sm, D4, hy);
    DLE_LAUNCH_CHECK();
  }

  // ---- list tables: link, heads apply (large) or leave partials (mid), fold (mid)
  if (lm.nl > 0) {
    lm.mhead = (int*)(wsb + pl.mhead_off);
    lm.mpart = (float*)(wsb + pl.mpart_off);
    if (mf.n > 0) {
      hipError_t e = hipMemsetAsync(lm.mhead, 0xFF, (size_t)mf.rows_total * EA_MID_S * 4, stream);
      if (e != hipSuccess) { dle_set_error("emb_adam_dedup memset: %s", hipGetErrorString(e)); return (int)e; }
    }
    const long long n_lk = (long long)batch * lm.nl;
    hipLaunchKernelGGL(emb_adam_link, dim3(ea_grid(n_lk, 256)), dim3(256), 0, stream, (const long long*)rows, head, next, (int)n_lk,
                       lm, skip_flag_dev);
    DLE_LAUNCH_CHECK();
#define GO(IDT, VT) hipLaunchKernelGGL(emb_adam_lists<IDT>, dim3(ea_grid(n_lk, 4 * 2)), dim3(256), 0, stream, tb, (const long long*)rows, (const VT*)grad, head, (const int*)next, (int)n_lk, lm, D4, gs4, hy)
    if (grad_dtype == DLE_F32) GO(DLE_F32, float4_t);
    else if (grad_dtype == DLE_F16) GO(DLE_F16, ushort4_t);
    else GO(DLE_BF16, ushort4_t);
#undef GO
    DLE_LAUNCH_CHECK();
    if (mf.n > 0) {
      hipLaunchKernelGGL(emb_adam_mid_fold, dim3((mf.rows_total * 32 + 255) / 256), dim3(256), 0, stream, tb, (const int*)lm.mhead,
                         (const float*)lm.mpart, mf, D4, hy);
      DLE_LAUNCH_CHECK();
    }
  }
  return 0;
}
