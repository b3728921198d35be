// Grouped 3x3 / pad 1 / stride 1 or 2 convolution (forward, inference epilogue) for gfx950: conv2 of the ResNeXt bottleneck.
//
// Replaces cuDNN's grouped conv fwd behind nn.Conv2d(groups=32) + the evaluation-mode BatchNorm + ReLU that follow it
// (Classification/ConvNets/image_classification/models/resnet.py:107-175 with cardinality 32, models/common.py:31-60).
//
// With C == Ko and Cg = C / groups in {4, 8, 16, 32}, the 32 output channels [32 b, 32 b + 32) read the 32 input channels of the
// same range and nothing else, whatever Cg is.  One wavefront owns one such 32-channel block `b` and walks 32-pixel tiles of the
// flat output index (n, p, q):
//
//  * the weights of the block live in REGISTERS for the wavefront's whole life: 9 taps x 2 k-steps of the A operand of
//    v_mfma_f32_32x32x16 (lane = output channel, 8 input channels each), built once from the packed [Ko][3][3][Cg] tensor.  For
//    Cg < 32 the fragment is the block-diagonal form: a lane keeps the 16-bit weights of its own group unmodified and exact zeros
//    elsewhere, so the accumulator sums ko's group only (32 / Cg x the necessary MFMA work, on a layer that activation traffic
//    bounds: 18 MFMAs per 32 x 32 outputs for every Cg);
//  * the activations are the B operand, gathered straight from global memory: lane (pixel, k-half) loads the 16 bytes of its
//    pixel's tap position with one bounds-checked buffer load (padding and the ragged last tile read as zero through the
//    buffer range check -- no LDS, no barrier, any stride, any H / W).  The nine taps re-read neighbouring pixels out of the
//    vector L1; the four wavefronts of a workgroup take four adjacent channel blocks of the same pixels, so every 128-byte line
//    is used whole;
//  * epilogue on the accumulator registers: lane = pixel, 4 runs of 4 consecutive channels; y = relu?(fmaf(scale, acc, shift)),
//    one rounding, 8-byte stores.
//
// An infinite or NaN activation in one group reaches the other groups of its 32-channel block as NaN (0 * inf), as it would on
// zero-expanded dense weights.
#include "gemm_tiles.h"

struct GcArgs {
  const unsigned short* x;     // [N, H, W, C]
  const unsigned short* w;     // [Ko, 3, 3, Cg]
  unsigned short* y;           // [N, P, Q, Ko]
  const float* scale;          // [Ko]
  const float* shift;          // [Ko]
  int H, W, C, P, Q, stride, relu;
  int NPQ, PQ;                 // output pixels in all / per image
  int tiles, nb, walkers;      // 32-pixel tiles, 32-channel blocks, wavefronts per channel block
  unsigned xbytes;
  FastDiv dPQ, dQ, dNB;
};

template <int DT, int CG>
__global__ __launch_bounds__(256, 2) void conv_grouped_kernel(GcArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 31, fh = lane >> 5;
  const int gw = blockIdx.x * 4 + wave;
  if (gw >= p.nb * p.walkers) return;                      // (no barrier below)
  const int walker = fd_div(gw, p.dNB), cb = gw - walker * p.nb;

  // ---- the block's weights as 18 A fragments: lane = output channel ko, elements = input channels 16 ks + 8 fh + e of the block
  ushort8_t wf[9][2];
  {
    const int ko = cb * 32 + fr, gl = fr / CG;             // gl: ko's group within the block
    const unsigned short* wk = p.w + (long long)ko * 9 * CG;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int ci0 = ks * 16 + fh * 8;
        const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (CG >= 8) {
          const int rel = ci0 - gl * CG;                   // first of the 8 channels, relative to ko's group
          const bool in = rel >= 0 && rel < CG;
          const ushort8_t v = *(const ushort8_t*)(wk + tap * CG + (in ? rel : 0));
          wf[tap][ks] = in ? v : zero;
        } else {
          const ushort4_t v = *(const ushort4_t*)(wk + tap * 4);
          const bool lo = ci0 == gl * 4, hi = ci0 + 4 == gl * 4;
          ushort8_t o = zero;
          if (lo) { o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
          if (hi) { o[4] = v[0]; o[5] = v[1]; o[6] = v[2]; o[7] = v[3]; }
          wf[tap][ks] = o;
        }
      }
  }
  // the lane's 16 output channels 8 qd + 4 fh + i of the block
  float4_t sc[4], sh[4];
#pragma unroll
  for (int qd = 0; qd < 4; ++qd) {
    sc[qd] = *(const float4_t*)(p.scale + cb * 32 + qd * 8 + fh * 4);
    sh[qd] = *(const float4_t*)(p.shift + cb * 32 + qd * 8 + fh * 4);
  }

  __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)p.x, 0, (int)p.xbytes, 0x00020000);
  const int chan = cb * 32 + fh * 8;

  for (int t = walker; t < p.tiles; t += p.walkers) {
    const int pix = t * 32 + fr;
    const bool valid = pix < p.NPQ;
    const int pc = valid ? pix : 0;
    const int n = fd_div(pc, p.dPQ), rem = pc - n * p.PQ;
    const int pp = fd_div(rem, p.dQ), qq = rem - pp * p.Q;
    const int h0 = pp * p.stride - 1, w0 = qq * p.stride - 1;
    // byte offset of (n, h0, w0, chan); may be negative for a padding position, exact (< 2^32) wherever the tap is inside
    const long long base = ((((long long)n * p.H + h0) * p.W + w0) * p.C + chan) * 2;
    ushort8_t fa[9][2];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int s = 0; s < 3; ++s) {
        const bool ok = valid && (unsigned)(h0 + r) < (unsigned)p.H && (unsigned)(w0 + s) < (unsigned)p.W;
        const unsigned off = (unsigned)(base + ((long long)(r * p.W + s) * p.C) * 2);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
          fa[r * 3 + s][ks] = __builtin_bit_cast(ushort8_t, __builtin_amdgcn_raw_buffer_load_b128(rs, ok ? off + ks * 32 : OOB_OFF, 0, 0));
      }
    float16_t acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) acc = Mfma32x16<DT>::run(wf[tap][ks], fa[tap][ks], acc);
    // D: lane owns pixel fr, channels 8 (i >> 2) + 4 fh + (i & 3)
    if (valid) {
      unsigned short* yo = p.y + (long long)pix * p.C + cb * 32 + fh * 4;
#pragma unroll
      for (int qd = 0; qd < 4; ++qd) {
        ushort4_t o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float v = __builtin_fmaf(sc[qd][i], acc[qd * 4 + i], sh[qd][i]);
          if (p.relu) v = v > 0.f ? v : 0.f;
          o[i] = Elem<DT>::from_f32(v);
        }
        *(ushort4_t*)(yo + qd * 8) = o;
      }
    }
  }
}

extern "C" int dle_conv2d_grouped_fwd_affine(const void* x, const void* w, void* y, const float* scale, const float* shift,
                                             int N, int H, int W, int C, int Ko, int groups, int stride,
                                             int dtype, int relu, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "conv2d_grouped_fwd_affine: 16-bit activations and weights only");
  DLE_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && C >= 64 && groups >= 1, "conv2d_grouped_fwd_affine: bad shape");
  DLE_CHECK_ARG(C == Ko, "conv2d_grouped_fwd_affine: C == Ko only (got C = %d, Ko = %d)", C, Ko);
  DLE_CHECK_ARG(C % 64 == 0, "conv2d_grouped_fwd_affine: C must be a multiple of 64 (got %d)", C);
  DLE_CHECK_ARG(C % groups == 0, "conv2d_grouped_fwd_affine: groups must divide C");
  const int Cg = C / groups;
  DLE_CHECK_ARG(Cg == 4 || Cg == 8 || Cg == 16 || Cg == 32,
                "conv2d_grouped_fwd_affine: C / groups must be 4, 8, 16 or 32 (got %d)", Cg);
  DLE_CHECK_ARG(stride == 1 || stride == 2, "conv2d_grouped_fwd_affine: stride 1 or 2 (got %d)", stride);
  if (N == 0) return 0;
  DLE_CHECK_ARG(x && w && y && scale && shift, "conv2d_grouped_fwd_affine: null pointer");
  DLE_CHECK_ARG(!((((uintptr_t)x) | ((uintptr_t)w) | ((uintptr_t)y) | ((uintptr_t)scale) | ((uintptr_t)shift)) & 15),
                "conv2d_grouped_fwd_affine: every operand must be 16-byte aligned");
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  const long long xbytes = (long long)N * H * W * C * 2, npq = (long long)N * P * Q;
  DLE_CHECK_ARG(xbytes < 0xFFFFFFF0LL, "conv2d_grouped_fwd_affine: each tensor must be smaller than 4 GiB");
  const DleDeviceLimits* lim = dle_device_limits();
  GcArgs p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.y = (unsigned short*)y; p.scale = scale; p.shift = shift;
  p.H = H; p.W = W; p.C = C; p.P = P; p.Q = Q; p.stride = stride; p.relu = relu;
  p.NPQ = (int)npq; p.PQ = P * Q;
  p.tiles = (int)((npq + 31) / 32); p.nb = C / 32;
  // two wavefronts per SIMD on every CU, split evenly over the channel blocks; never more walkers than tiles
  int walkers = (lim ? lim->cus : 256) * 8 / p.nb;
  if (walkers < 1) walkers = 1;
  if (walkers > p.tiles) walkers = p.tiles;
  p.walkers = walkers;
  p.xbytes = (unsigned)xbytes;
  p.dPQ = make_fastdiv(p.PQ); p.dQ = make_fastdiv(Q); p.dNB = make_fastdiv(p.nb);
  const dim3 grid((unsigned)((p.nb * walkers + 3) / 4)), block(256);
#define GC_GO(DT, CGV) hipLaunchKernelGGL((conv_grouped_kernel<DT, CGV>), grid, block, 0, stream, p)
#define GC_PICK(DT) do { if (Cg == 4) GC_GO(DT, 4); else if (Cg == 8) GC_GO(DT, 8); else if (Cg == 16) GC_GO(DT, 16); \
                         else GC_GO(DT, 32); } while (0)
  if (dtype == DLE_F16) GC_PICK(DLE_F16); else GC_PICK(DLE_BF16);
#undef GC_GO
#undef GC_PICK
  DLE_LAUNCH_CHECK();
  return 0;
}
