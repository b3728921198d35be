// The conv1d family: what csrc/hifigan.hip, fastpitch.hip, quartznet.hip and jasper.hip share around their arithmetic cores.  The
// cores differ for measured reasons (each file's header says why); the packed-table arithmetic, the operand movement, the
// epilogues and the host checks are the same and live here, once.  A new conv1d kernel takes them from this header and writes only
// its own tap / chunk walk.
//
// Conventions.  Activations are 16-bit, channels-last [rows, C].  A PACKED batch is [total_rows, C] with a device int32 table
// cu[B + 1]: sequence b owns rows cu[b] .. cu[b + 1] - 1.  Starts and lengths are clamped to the operands inside the kernels: a wrong
// table gives wrong answers but reaches no memory outside the operands.  Workgroups have 256 threads; in the staging helpers a
// thread owns 8 channels (cc = threadIdx.x & 7) of rows r0 = threadIdx.x >> 3, r0 + 32, ...; in the epilogues a lane owns row
// fr = lane & 31 of a 32 x 32 accumulator and, per group of 8 channels, the 4 at 4 fh (fh = lane >> 5).
//
// Contraction.  fastpitch.hip turns contraction off BEHIND its includes, so this header is compiled with the default: no product
// here may be followed by a sum it could fuse with, unless it is written as __builtin_fmaf.
#pragma once
#include "gemm_tiles.h"

// ---- packed tables -----------------------------------------------------------------------------------------------------------
// sequence b of a table: first row and length, clamped so that [start, start + len) lies inside [0, total) and len <= max_len
template <class L>
__device__ __forceinline__ void c1d_seq(const int32_t* cu, int b, long long total, long long& start, L& len,
                                        long long max_len = 0x7FFFFFFFFFFFLL) {
  long long s = cu[b];
  long long l = (long long)cu[b + 1] - s;
  s = s < 0 ? 0 : (s > total ? total : s);
  l = l < 0 ? 0 : (l > max_len ? max_len : l);
  if (s + l > total) l = total - s;
  start = s;
  len = (L)l;
}
// the out_len a sequence really has: what the table says, never more than its (clamped) input gives
__device__ __forceinline__ long long c1d_out_len(long long in_len, long long out_len_tab, int stride) {
  const long long m = in_len > 0 ? (in_len - 1) / stride + 1 : 0;
  return out_len_tab < m ? out_len_tab : m;
}

// ---- operand movement --------------------------------------------------------------------------------------------------------
// 8 values of x -> a: leaky ReLU as an fp32 product rounded to the storage type (slope 0: ReLU); x >= 0, -0 and NaN pass unchanged
template <int DT>
__device__ __forceinline__ ushort8_t c1d_act8(ushort8_t v, float slope) {
  ushort8_t o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float f = Elem<DT>::to_f32(v[e]);
    o[e] = f < 0.f ? Elem<DT>::from_f32(f * slope) : v[e];
  }
  return o;
}

// A fragments of one tap of the 64-channel chunk at c0, from global memory: wrow = the lane's row of w [Ko, ksize, C] (lane = ko),
// channels c0 + 16 ks + 8 fh + e.  Zero beyond C and for the rows beyond Ko (ko_ok false), where no address is formed and no load
// issued (with C = 8 the upper half-step would otherwise read past the last row of w); the k-steps beyond the chunk (wave-uniform)
// are not loaded either: the caller skips their MFMAs.
__device__ __forceinline__ void c1d_load_tap(ushort8_t* f, const unsigned short* wrow, int tap, int C, int c0, int fh, bool ko_ok) {
  const int cw = C - c0 < 64 ? C - c0 : 64;
  const int nks = (cw + 15) >> 4;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    f[ks] = ushort8_t{0, 0, 0, 0, 0, 0, 0, 0};
    if (ks < nks) {
      const int c = c0 + ks * 16 + fh * 8;
      if (ko_ok && c < C) f[ks] = *(const ushort8_t*)(wrow + (long long)tap * C + c);
    }
  }
}

// Rows plus halo of one 64-channel chunk, in two halves so that the global loads of chunk i + 1 are in flight while chunk i is
// computed.  c1d_stage_load reads staged rows r < rows (sequence times tbase + r of the sequence at xs, len rows long) x channels
// [c0, c0 + 64) into registers, N passes of 32 rows; c1d_stage_store writes them to lds[r][PITCH].  C need not be a multiple of
// 64: pieces at or beyond C are zero.  The activation (slope != 1) is applied at the load, once.
template <int DT, int N>
__device__ __forceinline__ void c1d_stage_load(ushort8_t (&v)[N], const unsigned short* xs, long long len, int C, long long tbase,
                                               int rows, int c0, float slope = 1.f) {
  const int cc = threadIdx.x & 7, r0 = threadIdx.x >> 3;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int r = r0 + 32 * i;
    const long long t = tbase + r;
    v[i] = ushort8_t{0, 0, 0, 0, 0, 0, 0, 0};
    if (r < rows && t >= 0 && t < len && c0 + cc * 8 < C) {
      v[i] = *(const ushort8_t*)(xs + t * C + c0 + cc * 8);
      if (slope != 1.f) v[i] = c1d_act8<DT>(v[i], slope);
    }
  }
}
template <int N, int PITCH>
__device__ __forceinline__ void c1d_stage_store(unsigned short* lds, const ushort8_t (&v)[N], int rows) {
  const int cc = threadIdx.x & 7, r0 = threadIdx.x >> 3;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int r = r0 + 32 * i;
    if (r < rows) *(ushort8_t*)(lds + r * PITCH + cc * 8) = v[i];
  }
}

// ---- epilogues on one 32 x 32 accumulator --------------------------------------------------------------------------------------
// The lane writes its 16 values of output row `row` (an element offset, row index * Ko): channels k0 + 8 qd + 4 fh + i.
// y = round16((acc + bias (+ add1) (+ add2)) * alpha), 8-byte stores; a run of 4 at or beyond Ko is skipped (Ko % 8 == 0: it is
// inside or outside whole).  An addend is read by the lane that writes the same element afterwards, so y may be an addend.
template <int DT>
__device__ __forceinline__ void c1d_epilogue_bias(const float16_t& acc, const float* bias, const unsigned short* add1,
                                                  const unsigned short* add2, unsigned short* y, long long row, int k0, int fh, int Ko,
                                                  float alpha) {
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int k4 = k0 + qd * 8 + fh * 4;
    if (k4 >= Ko) continue;
    const float4_t bs = *(const float4_t*)(bias + k4);
    ushort4_t a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0};
    if (add1) a1 = *(const ushort4_t*)(add1 + row + k4);
    if (add2) a2 = *(const ushort4_t*)(add2 + row + k4);
    ushort4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = acc[qd * 4 + i] + bs[i];
      if (add1) v += Elem<DT>::to_f32(a1[i]);
      if (add2) v += Elem<DT>::to_f32(a2[i]);
      o[i] = Elem<DT>::from_f32(v * alpha);
    }
    *(ushort4_t*)(y + row + k4) = o;
  }
}
// y = round16(relu?(fmaf(scale, acc, shift) (+ res))), 8-byte stores; Ko % 32 == 0 and k0 < Ko: every run is inside
template <int DT>
__device__ __forceinline__ void c1d_epilogue_bn(const float16_t& acc, const float* scale, const float* shift, const unsigned short* res,
                                                unsigned short* y, long long row, int k0, int fh, int relu) {
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    const int k4 = k0 + qd * 8 + fh * 4;
    const float4_t sc = *(const float4_t*)(scale + k4), sh = *(const float4_t*)(shift + k4);
    ushort4_t rs = {0, 0, 0, 0};
    if (res) rs = *(const ushort4_t*)(res + row + k4);
    ushort4_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = __builtin_fmaf(sc[i], acc[qd * 4 + i], sh[i]);
      if (res) v += Elem<DT>::to_f32(rs[i]);
      if (relu) v = v > 0.f ? v : 0.f;
      o[i] = Elem<DT>::from_f32(v);
    }
    *(ushort4_t*)(y + row + k4) = o;
  }
}

// ---- host checks (the entries keep their own messages) ---------------------------------------------------------------------------
inline bool c1d_overlap(const void* a, long long abytes, const void* b, long long bbytes) {
  if (!a || !b) return false;
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}
// y may BE an addend (the lane that writes an element read it before), but not overlap it otherwise
inline bool c1d_addend_ok(const void* add, const void* y, long long ybytes) { return add == y || !c1d_overlap(add, ybytes, y, ybytes); }
// tensors of these byte counts stay below the 4 GiB a 32-bit byte offset reaches
template <class... N>
inline bool c1d_under_4gib(N... bytes) { return (... && ((long long)bytes < 0xFFFFFFF0LL)); }
// the (B, total rows) envelope of a packed batch and its output
inline bool c1d_batch_ok(int B, long long total_in, long long total_out) {
  return B >= 1 && B <= (1 << 20) && total_in >= 0 && total_in < (1LL << 31) && total_out >= 0 && total_out <= total_in;
}
// Launch of KERNEL(S, D) -- a macro of the caller's that names the instantiation -- for stride / dilation in {1, 2}, not both 2,
// with the dynamic-LDS opt-in of DLE_LAUNCH_LDS
#define C1D_LAUNCH_SD(KERNEL, stride, dilation, grid, block, lds, stream, ...)                              \
  do {                                                                                                      \
    if ((stride) == 2) DLE_LAUNCH_LDS((KERNEL(2, 1)), grid, block, lds, stream, __VA_ARGS__);               \
    else if ((dilation) == 2) DLE_LAUNCH_LDS((KERNEL(1, 2)), grid, block, lds, stream, __VA_ARGS__);        \
    else DLE_LAUNCH_LDS((KERNEL(1, 1)), grid, block, lds, stream, __VA_ARGS__);                             \
  } while (0)
