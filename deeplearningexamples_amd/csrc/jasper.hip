// Jasper, inference (SpeechRecognition/Jasper/jasper/model.py:58-85 MaskedConv1d, :128-131 _conv_bn, :137-162 JasperBlock.forward)
// on PACKED utterances, the layout and the conventions of csrc/quartznet.hip: activations are 16-bit, channels-last
// [total_rows, C]; sequence b owns rows cu[b] .. cu[b + 1] - 1 of a device int32 table cu[B + 1]; rows outside a row's own
// sequence read as zero; starts and lengths are clamped to the operands inside the kernel.
//
// dle_conv1d_bn_packed_fwd -- one Jasper sub-block per launch: DENSE masked Conv1d (ksize <= 29 taps, stride 1 / 2, dilation
// 1 / 2) -> evaluation-mode BatchNorm (scale / shift) -> (+ residual) -> (ReLU).  An implicit GEMM with a contraction of
// ksize * C <= 29 * 1024 per output, bound by the matrix pipes, so BOTH operands go through LDS:
//  * One workgroup of 4 wavefronts per (sequence, time tile of JS_TT = 128 OUTPUT rows, block of JS_KB = 128 output channels);
//    a tile never spans two sequences.  The grid is one-dimensional in tiles as in qn_tcs_kernel (blockIdx.x < total_out / 128
//    + B, an upper bound of sum_b ceil(out_len_b / 128)); EVERY wavefront finds its (sequence, tile) by the same prefix sum
//    over the per-sequence tile counts, so a workgroup without a tile exits before any barrier and before any LDS access.
//  * C is walked in chunks of JS_CC = 64 channels.  Per chunk the input rows [t0 * stride - halo, ...) x 64 channels are staged
//    ONCE (16-byte loads, zeros outside [0, len) of the own sequence, pitch 72 elements: the 16 rows of a ds_read_b128 lane group
//    cover the 64 banks once); the ksize taps read shifted windows of that one image as the B operand of v_mfma_f32_32x32x16
//    (lane = time step).  Per (chunk, tap) the weight slab [128 output channels][64 channels] is staged once per WORKGROUP (same
//    pitch) and read by all four wavefronts as the A operand (lane = output channel).
//  * Both images are double-buffered: while (chunk, tap) is multiplied, the slab of the next (chunk, tap) -- and, during a chunk's
//    first tap, the input rows of the next chunk -- are in flight to registers; they are stored to the other buffer behind the
//    MFMAs and published by the ONE barrier of the iteration.  The loop has one form.  (A second register stage, the slab two
//    iterations ahead behind LDS-only barriers, was measured 8 - 25 % slower at 16 x 843 rows and is not kept: DESIGN.md 4m.)
//  * Wavefront (wr, wc) owns rows wr * 64 .. + 64 x channels wc * 64 .. + 64 of the tile: 2 x 2 accumulators of 32 x 32.  Per
//    16-channel step it reads 2 A and 2 B fragments (4 ds_read_b128) for 4 MFMAs: one LDS read per MFMA, a third of what
//    saturates the LDS array (MI355X_MICROARCH, LDS: three ds_read_b128 per MFMA gap).
//  * Epilogue on the accumulators: fmaf(scale, acc, shift) (+ residual) (ReLU), one rounding, 8-byte stores.
// Tile.  128 rows x 128 channels: a staged slab of 16 KiB feeds 128 x 128 x 64 multiply-adds, 1 weight byte from HBM / L2 per
// 64 multiply-adds and none per MFMA from the vector memory path of the other three wavefronts; fp_conv1d_packed_kernel (64 x 128,
// each wavefront loading its own fragments) reads 1 per 32 and issues one 16-byte global load per MFMA pair.  At 16 x 1,686
// frames (843 rows each behind Conv1) the grid is 112 time tiles x Ko / 128 = 224 (Ko 256) to 896 (Ko 1024) workgroups for 256
// CUs; one utterance gives 7 time tiles, so a single utterance leaves CUs idle whatever the tile (a smaller tile would trade that
// for weight traffic; batch 1 is bound by the 111 launches and by the serial walk over ksize * C / 64 iterations either way).
// 256 rows would halve the slab traffic again but double the accumulators, halve the workgroup count, and leave an 843-row
// utterance with a 4th tile that is 71 % padding instead of a 7th that is 41 %.
// LDS: 2 x rows x 144 B for the input image + 2 x 18,432 B for the slabs, rows = 127 stride + 1 + (ksize - 1) dilation:
// 76,608 B at ksize 11 (two workgroups per CU), 81,792 B at ksize 29, 89,856 B at ksize 29 dilation 2, 118,368 B at stride 2
// ksize 29 (one workgroup per CU); above 64 KiB the launch opts in through DLE_LAUNCH_LDS.
#include "conv1d_family.h"

#define JS_TT 128          // output rows per time tile
#define JS_KB 128          // output channels per workgroup
#define JS_CC 64           // input channels per staged chunk
#define JS_P 72            // LDS row pitch in elements
#define JS_MAXK 29

struct JsArgs {
  const unsigned short* x;      // [total_in, C]
  const unsigned short* w;      // [Ko, ksize, C]
  const float* scale;           // [Ko]
  const float* shift;           // [Ko]
  const unsigned short* res;    // [total_out, Ko] or null
  unsigned short* y;            // [total_out, Ko]
  const int32_t* cu_in;
  const int32_t* cu_out;
  long long total_in, total_out;
  int B, C, Ko, ksize, rows, relu;
};

template <int DT, int S, int D>
__global__ __launch_bounds__(256) void js_conv1d_bn_kernel(JsArgs p) {
  // staged input rows at the largest ksize, and the 16-byte pieces of them per thread
  constexpr int MAXROWS = (JS_TT - 1) * S + 1 + (JS_MAXK - 1) * D;
  constexpr int XI = (MAXROWS * 8 + 255) / 256;
  constexpr int WI = JS_KB * 8 / 256;
  extern __shared__ __attribute__((aligned(16))) unsigned short js_lds[];
  const int ximg = p.rows * JS_P;                                  // elements of one input image
  unsigned short* xl = js_lds;                                     // [2][rows][72]
  unsigned short* wl = js_lds + 2 * ximg;                          // [2][128][72]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // The search is written out here as in qn_tcs_kernel: through a shared function the stride-2 instantiation measured 0.5 - 1.5 %
  // slower at one utterance (Conv1) in four runs, and 0.993 of the parent's time written out (profiles/conv1d_family_variants.md).
  // (sequence, tile) of this workgroup: every wavefront runs the same search on the same data
  long long fb = -1, ft = 0;
  {
    const long long g = blockIdx.x;
    long long run = 0;
    for (int b0 = 0; b0 < p.B; b0 += 64) {
      const int b = b0 + lane;
      long long n = 0;
      if (b < p.B) {
        long long si, li, so, lo;
        c1d_seq(p.cu_in, b, p.total_in, si, li);
        c1d_seq(p.cu_out, b, p.total_out, so, lo);
        n = (c1d_out_len(li, lo, S) + JS_TT - 1) / JS_TT;
      }
      long long inc = n;                                           // inclusive prefix over the 64 lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const long long up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
      }
      const unsigned long long hit = __ballot(run + inc > g);
      if (hit) {
        const int l = __ffsll((long long)hit) - 1;
        const long long incl = __shfl(inc, l, 64), nl = __shfl(n, l, 64);
        fb = b0 + l;
        ft = g - (run + incl - nl);
        break;
      }
      run += __shfl(inc, 63, 64);
    }
  }
  if (fb < 0) return;                                              // workgroup-uniform, before any barrier
  const int b = (int)fb;
  const long long t0 = ft * JS_TT;                         // first output row of the tile inside its sequence
  long long in0, in_len, out0, out_len;
  c1d_seq(p.cu_in, b, p.total_in, in0, in_len);
  c1d_seq(p.cu_out, b, p.total_out, out0, out_len);
  out_len = c1d_out_len(in_len, out_len, S);
  const int live = (int)(out_len - t0 < JS_TT ? out_len - t0 : JS_TT);     // >= 1 by construction

  const int fr = lane & 31, fh = lane >> 5;
  const int wr = wave >> 1, wc = wave & 1;
  const int kblk = blockIdx.y * JS_KB;
  const int kob = kblk + wc * 64;
  const int nts = live - wr * 64 > 32 ? 2 : (live - wr * 64 > 0 ? 1 : 0);  // live 32-row sub-tiles of this wavefront
  const bool wave_on = kob < p.Ko && nts > 0;                      // Ko % 64 == 0: a wavefront's 64 channels are inside or outside whole
  const unsigned short* xs = p.x + in0 * p.C;
  const long long tbase = t0 * S - (long long)(p.ksize / 2) * D;   // sequence time of staged row 0
  const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};

  float16_t acc[2][2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][nt][i] = 0.f;

  // staging: thread = 8 channels (cc) of rows r0, r0 + 32, ...
  const int cc = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  ushort8_t xr[XI], wreg[WI];
  // load_x / store_x are c1d_stage_load / c1d_stage_store (conv1d_family.h) written out: through the shared pair the dilation-2
  // instantiation measured 1.5 - 3 % slower (Conv2 at 1 and 16 utterances) and stride 2 about 1 %.
  auto load_x = [&](int c0) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int r = r0 + 32 * i;
      const long long t = tbase + r;
      xr[i] = zero;
      if (r < p.rows && t >= 0 && t < in_len) xr[i] = *(const ushort8_t*)(xs + t * p.C + c0 + cc * 8);
    }
  };
  auto store_x = [&](unsigned short* img) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int r = r0 + 32 * i;
      if (r < p.rows) *(ushort8_t*)(img + r * JS_P + cc * 8) = xr[i];
    }
  };
  auto load_w = [&](int c0, int tap) {
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int ko = kblk + r0 + 32 * i;
      wreg[i] = zero;
      if (ko < p.Ko) wreg[i] = *(const ushort8_t*)(p.w + ((long long)ko * p.ksize + tap) * p.C + c0 + cc * 8);
    }
  };
  auto store_w = [&](unsigned short* slab) {
#pragma unroll
    for (int i = 0; i < WI; ++i) *(ushort8_t*)(slab + (r0 + 32 * i) * JS_P + cc * 8) = wreg[i];
  };

  load_x(0);
  load_w(0, 0);
  store_x(xl);
  store_w(wl);
  __syncthreads();
  const int nchunks = p.C / JS_CC;
  int it = 0;
  for (int ch = 0; ch < nchunks; ++ch) {
    const unsigned short* ximg_cur = xl + (ch & 1) * ximg;
    const bool more_x = ch + 1 < nchunks;
    for (int tap = 0; tap < p.ksize; ++tap, ++it) {
      const bool last_tap = tap + 1 == p.ksize;
      const bool more_w = !last_tap || more_x;
      // the next iteration's operands: in flight during this iteration's MFMAs
      if (more_w) load_w(last_tap ? (ch + 1) * JS_CC : ch * JS_CC, last_tap ? 0 : tap + 1);
      if (tap == 0 && more_x) load_x((ch + 1) * JS_CC);
      if (wave_on) {
        const unsigned short* xa = ximg_cur + ((wr * 64 + fr) * S + tap * D) * JS_P + fh * 8;
        const unsigned short* wa = wl + (it & 1) * (JS_KB * JS_P) + (wc * 64 + fr) * JS_P + fh * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          const ushort8_t a0 = *(const ushort8_t*)(wa + ks * 16);
          const ushort8_t a1 = *(const ushort8_t*)(wa + 32 * JS_P + ks * 16);
#pragma unroll
          for (int nt = 0; nt < 2; ++nt)
            if (nt < nts) {
              const ushort8_t fb8 = *(const ushort8_t*)(xa + nt * 32 * S * JS_P + ks * 16);
              acc[0][nt] = Mfma32x16<DT>::run(a0, fb8, acc[0][nt]);
              acc[1][nt] = Mfma32x16<DT>::run(a1, fb8, acc[1][nt]);
            }
        }
      }
      // the other buffers were last read one iteration (slab) / one chunk (image) ago, in front of the previous barrier
      if (more_w) store_w(wl + ((it + 1) & 1) * (JS_KB * JS_P));
      if (last_tap && more_x) store_x(xl + ((ch + 1) & 1) * ximg);
      if (more_w) __syncthreads();
    }
  }
  if (!wave_on) return;

  // D: lane owns row fr of the sub-tile, channels kob + 32 nb + 8 (i >> 2) + 4 fh + (i & 3)
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int t = wr * 64 + nt * 32 + fr;
    if (t >= live) continue;
    const long long row = (out0 + t0 + t) * p.Ko;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      c1d_epilogue_bn<DT>(acc[nb][nt], p.scale, p.shift, p.res, p.y, row, kob + nb * 32, fh, p.relu);
  }
}

template <int DT>
static void js_launch(const JsArgs& p, dim3 grid, int lds, int stride, int dilation, hipStream_t stream) {
#define JS_KERNEL(S, D) js_conv1d_bn_kernel<DT, S, D>               // DT: this function's
  C1D_LAUNCH_SD(JS_KERNEL, stride, dilation, grid, dim3(256), lds, stream, p);
#undef JS_KERNEL
}

extern "C" int dle_conv1d_bn_packed_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* residual,
                                        void* y, const int32_t* cu_in, const int32_t* cu_out, int B, int64_t total_in,
                                        int64_t total_out, int C, int Ko, int ksize, int stride, int dilation, int relu, int dtype,
                                        hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "conv1d_bn_packed_fwd: 16-bit activations and weights only");
  DLE_CHECK_ARG(c1d_batch_ok(B, total_in, total_out), "conv1d_bn_packed_fwd: bad batch / total rows");
  DLE_CHECK_ARG(C >= 64 && C <= 1024 && C % 64 == 0, "conv1d_bn_packed_fwd: C must be a multiple of 64 in [64, 1024] (got %d)", C);
  DLE_CHECK_ARG(Ko >= 64 && Ko <= 1024 && Ko % 64 == 0, "conv1d_bn_packed_fwd: Ko must be a multiple of 64 in [64, 1024] (got %d)", Ko);
  DLE_CHECK_ARG(ksize >= 1 && ksize <= JS_MAXK && (ksize & 1), "conv1d_bn_packed_fwd: ksize must be odd in [1, 29] (got %d)", ksize);
  DLE_CHECK_ARG((stride == 1 || stride == 2) && (dilation == 1 || dilation == 2) && !(stride == 2 && dilation == 2),
                "conv1d_bn_packed_fwd: stride and dilation in {1, 2}, not both 2 (got %d, %d)", stride, dilation);
  if (total_out == 0) return 0;
  DLE_CHECK_ARG(x && w && scale && shift && y && cu_in && cu_out, "conv1d_bn_packed_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(x, w, scale, shift, residual, y) && dle_aligned<4>(cu_in, cu_out),
                "conv1d_bn_packed_fwd: x, w, scale, shift, residual and y must be 16-byte aligned");
  const long long xbytes = (long long)total_in * C * 2, ybytes = (long long)total_out * Ko * 2;
  const long long wbytes = (long long)Ko * ksize * C * 2;
  DLE_CHECK_ARG(c1d_under_4gib(xbytes, ybytes), "conv1d_bn_packed_fwd: each tensor must be smaller than 4 GiB");
  DLE_CHECK_ARG(!c1d_overlap(x, xbytes, y, ybytes) && !c1d_overlap(residual, ybytes, y, ybytes) && !c1d_overlap(w, wbytes, y, ybytes) &&
                    !c1d_overlap(scale, Ko * 4LL, y, ybytes) && !c1d_overlap(shift, Ko * 4LL, y, ybytes),
                "conv1d_bn_packed_fwd: y must not overlap x, w, scale, shift or residual");
  JsArgs p;
  p.x = (const unsigned short*)x; p.w = (const unsigned short*)w; p.scale = scale; p.shift = shift;
  p.res = (const unsigned short*)residual; p.y = (unsigned short*)y; p.cu_in = cu_in; p.cu_out = cu_out;
  p.total_in = total_in; p.total_out = total_out; p.B = B; p.C = C; p.Ko = Ko; p.ksize = ksize; p.relu = relu;
  p.rows = (JS_TT - 1) * stride + 1 + (ksize - 1) * dilation;
  const int lds = (2 * p.rows * JS_P + 2 * JS_KB * JS_P) * 2;
  const long long gx = total_out / JS_TT + B;
  DLE_CHECK_ARG(gx <= 0x7FFFFFFFLL, "conv1d_bn_packed_fwd: too many time tiles");
  const dim3 grid((unsigned)gx, (unsigned)((Ko + JS_KB - 1) / JS_KB));
  if (dtype == DLE_F16) js_launch<DLE_F16>(p, grid, lds, stride, dilation, stream);
  else js_launch<DLE_BF16>(p, grid, lds, stride, dilation, stream);
  DLE_LAUNCH_CHECK();
  return 0;
}
