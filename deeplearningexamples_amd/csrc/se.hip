// Squeeze-and-excitation for inference (SE-ResNeXt): the gate of one block in one launch, its application in another.
//
// Replaces, under model.eval(), SqueezeAndExcitation (Classification/ConvNets/image_classification/models/common.py:146-164:
// mean over H x W -> nn.Linear(C, S) -> ReLU -> nn.Linear(S, C) -> sigmoid) and `out = residual + out * gate; relu` of the
// bottleneck (models/resnet.py:165-173).
//
//  * se_gate_kernel: one 1024-thread workgroup per image.  Threads are laid out [row phase][8-channel group]; each sums its
//    pixels of the 16-bit t in fp32 (16-byte loads), the phases are folded in a fixed order (deterministic), then both small
//    products run in fp32 on the fp32 weights: one wavefront per hidden unit for the squeeze, one thread per channel for the
//    expand.  sigmoid = 1 / (1 + expf(-z)) with the accurate expf and a correctly rounded division.
//  * se_apply_kernel: y = relu?(fmaf(t, gate[n, c], residual)), 16 bytes per lane, one rounding.
#include "common.h"

#define SE_THREADS 1024

template <int DT>
__global__ __launch_bounds__(SE_THREADS) void se_gate_kernel(const unsigned short* __restrict__ t, const float* __restrict__ w1,
                                                             const float* __restrict__ b1, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, float* __restrict__ gate, int HW, int C,
                                                             int S, int phases) {
  extern __shared__ __attribute__((aligned(16))) float se_lds[];
  float* part = se_lds;                                    // [phases][C] partial sums, then [0][C] the means
  float* hid = se_lds + (size_t)phases * C;                // [S]
  const int n = blockIdx.x, tid = threadIdx.x, C8 = C >> 3;
  const unsigned short* tn = t + (long long)n * HW * C;
  // ---- per-channel sums: thread = (phase, channel group); wide tensors (C8 > SE_THREADS) loop over channel groups
  const int ph = tid / C8, cg0 = tid - ph * C8;
  if (ph < phases) {
    for (int cg = cg0; cg < C8; cg += SE_THREADS) {
      float acc[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = 0.f;
      for (int hw = ph; hw < HW; hw += phases) {
        const ushort8_t v = *(const ushort8_t*)(tn + (long long)hw * C + cg * 8);
        float f[8];
        unpack8<DT>(v, f);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += f[k];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) part[ph * C + cg * 8 + k] = acc[k];
    }
  }
  __syncthreads();
  const float inv = 1.0f / (float)HW;
  for (int c = tid; c < C; c += SE_THREADS) {
    float s = part[c];
    for (int q = 1; q < phases; ++q) s += part[q * C + c];
    part[c] = s * inv;                                     // (row 0 is read by this thread only)
  }
  __syncthreads();
  // ---- squeeze: hid[s] = relu(b1[s] + w1[s, :] . mean), one wavefront per s
  const int lane = tid & 63, wave = tid >> 6;
  for (int s = wave; s < S; s += SE_THREADS / 64) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = __builtin_fmaf(w1[(long long)s * C + c], part[c], a);
    a = wave_sum(a) + b1[s];
    if (lane == 0) hid[s] = a > 0.f ? a : 0.f;
  }
  __syncthreads();
  // ---- expand + sigmoid
  for (int c = tid; c < C; c += SE_THREADS) {
    float z = b2[c];
    for (int s = 0; s < S; ++s) z = __builtin_fmaf(w2[(long long)c * S + s], hid[s], z);
    gate[(long long)n * C + c] = 1.0f / (1.0f + expf(-z));
  }
}

template <int DT>
__global__ __launch_bounds__(256) void se_apply_kernel(const unsigned short* __restrict__ t, const float* __restrict__ gate,
                                                       const unsigned short* __restrict__ residual, unsigned short* __restrict__ y,
                                                       long long total, long long per_image, int C8, int relu) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long n = i / per_image;
    const int c8 = (int)(i % C8);
    const float* g = gate + (n * C8 + c8) * 8;
    const float4_t g0 = *(const float4_t*)g, g1 = *(const float4_t*)(g + 4);
    const float gv[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
    float tv[8], rv[8];
    unpack8<DT>(((const ushort8_t*)t)[i], tv);
    const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    unpack8<DT>(residual ? ((const ushort8_t*)residual)[i] : zero, rv);
    float v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      v[k] = __builtin_fmaf(tv[k], gv[k], rv[k]);
      if (relu) v[k] = v[k] > 0.f ? v[k] : 0.f;
    }
    ((ushort8_t*)y)[i] = pack8<DT>(v);
  }
}

extern "C" int dle_se_gate(const void* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                           int N, int HW, int C, int S, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "se_gate: 16-bit activations only");
  DLE_CHECK_ARG(N >= 0 && HW >= 1 && C >= 8 && C % 8 == 0, "se_gate: bad shape (C must be a multiple of 8)");
  DLE_CHECK_ARG(S >= 1 && S <= 64, "se_gate: hidden width 1..64 (got %d)", S);
  if (N == 0) return 0;
  DLE_CHECK_ARG(t && w1 && b1 && w2 && b2 && gate, "se_gate: null pointer");
  DLE_CHECK_ARG(!(((uintptr_t)t) & 15), "se_gate: t must be 16-byte aligned");
  const int C8 = C / 8;
  int phases = SE_THREADS / C8;
  if (phases < 1) phases = 1;
  if (phases > HW) phases = HW;
  const size_t lds = ((size_t)phases * C + S) * sizeof(float);
  DLE_CHECK_ARG(lds <= 64 * 1024, "se_gate: C = %d needs %zu bytes of LDS (limit 64 KiB)", C, lds);
  if (dtype == DLE_F16) hipLaunchKernelGGL(se_gate_kernel<DLE_F16>, dim3(N), dim3(SE_THREADS), lds, stream, (const unsigned short*)t, w1, b1, w2, b2, gate, HW, C, S, phases);
  else hipLaunchKernelGGL(se_gate_kernel<DLE_BF16>, dim3(N), dim3(SE_THREADS), lds, stream, (const unsigned short*)t, w1, b1, w2, b2, gate, HW, C, S, phases);
  DLE_LAUNCH_CHECK();
  return 0;
}

extern "C" int dle_se_apply(const void* t, const float* gate, const void* residual, void* y,
                            int64_t N, int HW, int C, int dtype, int relu, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "se_apply: 16-bit activations only");
  DLE_CHECK_ARG(N >= 0 && HW >= 1 && C >= 8 && C % 8 == 0, "se_apply: bad shape (C must be a multiple of 8)");
  if (N == 0) return 0;
  DLE_CHECK_ARG(t && gate && y, "se_apply: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)t) | ((uintptr_t)gate) | ((uintptr_t)residual) | ((uintptr_t)y)) & 15),
                "se_apply: every operand must be 16-byte aligned");
  const long long per_image = (long long)HW * (C / 8), total = (long long)N * per_image;
  const DleDeviceLimits* lim = dle_device_limits();
  const long long cap = (long long)(lim ? lim->cus : 256) * 16, want = (total + 255) / 256;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  if (dtype == DLE_F16) hipLaunchKernelGGL(se_apply_kernel<DLE_F16>, dim3(grid), dim3(256), 0, stream, (const unsigned short*)t, gate, (const unsigned short*)residual, (unsigned short*)y, total, per_image, C / 8, relu);
  else hipLaunchKernelGGL(se_apply_kernel<DLE_BF16>, dim3(grid), dim3(256), 0, stream, (const unsigned short*)t, gate, (const unsigned short*)residual, (unsigned short*)y, total, per_image, C / 8, relu);
  DLE_LAUNCH_CHECK();
  return 0;
}
