// The row-tile family: what csrc/tft.hip, ncf.hip and moflow.hip share around their walks.  Every linear layer of these models is
// out^T = W X^T with v_mfma_f32_32x32x16 against a tile of 32 samples; which weights sit in registers, which stream from L2 and how
// far ahead differs per kernel for measured reasons (each file's header says why).  The layout that follows from the operand order,
// the bias load, the rounding store and the plain K loop are the same and live here, once.  A new row-tile kernel takes them from
// this header and writes only its own walk.
//
// Operand order.  The weight rows are the A operand: lane l holds 8 consecutive k of row (l & 31), the upper half-wave
// (hf = l >> 5) the second 8 of a 16-wide k step.  The 32 samples of the tile are the B operand, read the same way out of a ROW
// IMAGE: 16-bit, one line per sample, pitch = width + 8 halves, so that the 32 lines of a fragment read start in different bank
// groups (the files keep their pitch constants and the reason for each value).
//
// Layout.  A lane ends up with 16 output features of ONE sample, row (l & 31): accumulator register r is feature rt_feat(r, hf) =
// (r & 3) + 8 (r >> 2) + 4 hf of the wavefront's 32-feature block.  Four consecutive features per register quad: the next image is
// written with 8-byte stores, a bias is four float4 loads, and the two halves of a gate or of an s | t pair sit in one lane.
//
// Contraction.  This header is compiled with the default setting and forms no product: the only arithmetic is the MFMA and a
// maximum.  What a kernel does between the K loop and the store (moflow.hip's __fadd_rn / __fmul_rn chains) stays in its file.
#pragma once
#include "common.h"

// accumulator register r of half-wave hf -> feature of the 32-feature block (rt_feat(r, 0): the map inside an 8-feature group pair)
__device__ __forceinline__ int rt_feat(int r, int hf) { return (r & 3) + 8 * (r >> 2) + 4 * hf; }

// four fp32 values, each rounded once, as four consecutive 16-bit values
template <int DT>
__device__ __forceinline__ uint2_t rt_pack4(float a, float b, float c, float d) {
  uint2_t o;
  o[0] = (unsigned)Elem<DT>::from_f32(a) | ((unsigned)Elem<DT>::from_f32(b) << 16);
  o[1] = (unsigned)Elem<DT>::from_f32(c) | ((unsigned)Elem<DT>::from_f32(d) << 16);
  return o;
}

// the lane's 16 values of an fp32 vector (a bias, LDS or global): features n0 + rt_feat(r, hf), by float4 loads; p + n0 must be
// 16-byte aligned.  rt_load16s reads them one by one, for vectors whose entry point asks for 4-byte alignment only.
__device__ __forceinline__ float16_t rt_load16(const float* p, int n0, int hf) {
  float16_t acc;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const float4_t v = *(const float4_t*)(p + n0 + 8 * g + 4 * hf);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[4 * g + i] = v[i];
  }
  return acc;
}
__device__ __forceinline__ float16_t rt_load16s(const float* p, int n0, int hf) {
  float16_t acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = p[n0 + rt_feat(r, hf)];
  return acc;
}

// the lane's 16 values v (float16_t or float[16]), ReLU if asked, one rounding, into columns n0 + feature of `line`: the lane's
// line of an LDS row image or its row of a 16-bit tensor; line + n0 must be 8-byte aligned
template <int DT, bool RELU, class V>
__device__ __forceinline__ void rt_store16(unsigned short* line, int n0, int hf, const V& v) {
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float q[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = RELU ? fmaxf(v[4 * g + i], 0.f) : v[4 * g + i];
    *(uint2_t*)(line + n0 + 4 * hf + 8 * g) = rt_pack4<DT>(q[0], q[1], q[2], q[3]);
  }
}

// acc += A B^T over nks k steps of 16: a = the lane's 8 halves of step 0 of its A row (memory or LDS), astep halves from one step to
// the next (16 for a row-major matrix, 512 for fragment order), b = the lane's line of a row image + 8 hf
template <int DT>
__device__ __forceinline__ float16_t rt_mma(const unsigned short* a, int astep, const unsigned short* b, int nks, float16_t acc) {
  for (int ks = 0; ks < nks; ++ks) acc = Mfma32x16<DT>::run(*(const ushort8_t*)(a + ks * astep), *(const ushort8_t*)(b + ks * 16), acc);
  return acc;
}

// the persistent-grid rule of the kernels that walk tiles: one workgroup per tile, at most max_workgroups of them, or at most one per
// compute unit of the device when max_workgroups is 0
inline long long rt_persistent_grid(long long tiles, int max_workgroups, const DleDeviceLimits* lim) {
  const long long cap = max_workgroups > 0 ? max_workgroups : lim->cus;
  return tiles < cap ? tiles : cap;
}
