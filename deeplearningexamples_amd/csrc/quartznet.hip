// QuartzNet, inference (SpeechRecognition/QuartzNet/quartznet/model.py:80-112 MaskedConv1d, :207-249 the `separable` branch of
// JasperBlock._get_conv_bn_layer, :257-292 JasperBlock.forward, :341-349 the decoder's log_softmax and GreedyCTCDecoder;
// common/features.py:158-170,290-302 normalize_batch "per_feature" and the mask; common/helpers.py:35-61
// ctc_decoder_predictions_tensor) on PACKED utterances, the layout of csrc/fastpitch.hip: activations are 16-bit, channels-last
// [total_rows, C]; sequence b owns rows cu[b] .. cu[b + 1] - 1 of a device int32 table cu[B + 1].  The reference's "masked"
// convolution zeroes the frames at and behind a sequence's length in front of EVERY convolution; here those rows do not exist and
// every kernel reads rows outside the row's own sequence as zero.  Starts and lengths are clamped to the operands inside every
// kernel: a wrong table gives wrong answers but reaches no memory outside the operands.
//
// dle_tcs_conv1d_packed_fwd -- the time-channel separable unit in ONE launch: depthwise Conv1d (ksize taps, stride 1 / 2, dilation
// 1 / 2) -> pointwise Conv1d -> evaluation-mode BatchNorm (scale / shift) -> (+ residual) -> (ReLU).  The depthwise result `d` lives
// in LDS only (d_out, the tests' seam, aside).
//  * One workgroup of 4 wavefronts per (sequence, time tile of QN_TT = 64 OUTPUT rows, block of QN_KB = 256 output channels); a
//    tile never spans two sequences.  There is no max_len in the contract, so the grid is one-dimensional in tiles: blockIdx.x is
//    the g-th tile of the batch, g < total_out / 64 + B (an upper bound of sum_b ceil(out_len_b / 64)), and wavefront 0 finds
//    (sequence, tile) by a prefix sum of the per-sequence tile counts, 64 sequences per step; blockIdx.y is the channel block.
//    Nothing is persistent: there is no grid cap and no second trip.
//  * The channel axis C is walked in chunks of QN_CC = 64 channels (the K = 87, dilation 2 halo of 172 rows at C = 512 would not
//    fit LDS otherwise, and the depthwise is per channel anyway: each chunk is one 64-deep K slice of the pointwise product).
//    Per chunk: (1) the input rows [t0 * stride - halo, ...) x 64 channels and the chunk's depthwise taps are staged in LDS with
//    16-byte loads, zeros outside [0, len) of the OWN sequence; the taps are padded to a multiple of 8 (the padding taps are skipped); (2) the depthwise:
//    thread = (channel PAIR, 8 consecutive output rows), 32-bit LDS reads, taps in blocks of 8: 8 tap words + (7 stride + 7 dilation
//    + 1) input words feed 128 fp32 FMAs, the sums run over the taps in ascending order as one fmaf chain per output; `d` is rounded
//    once to the storage type and written to the [64 rows][pitch 72] LDS tile (and to d_out by channel block 0); (3) the pointwise
//    product: d is the B operand of v_mfma_f32_32x32x16 (lane = time step), the UNMODIFIED 16-bit pw weights are the A operand
//    (lane = output channel; 16-byte global loads issued before the depthwise so that they land under it), every wavefront owns
//    64 output channels x 2 sub-tiles of 32 rows.  Three barriers per chunk; the LDS images are single.  While the grid
//    holds no more workgroups than the device has CUs (PF), the global loads of chunk i + 1 (input rows, taps) are issued into
//    registers right after chunk i's are stored to LDS and land under its depthwise and MFMAs (LDS-only barriers, so that they stay
//    in flight); a larger grid stages each chunk when it needs it and leaves the overlap to the two workgroups that share a CU (the launcher says what was measured).
//  * Epilogue on the accumulators: fmaf(scale, acc, shift) (+ residual) (ReLU), one rounding, 8-byte stores.
//  Ko > 256 recomputes the depthwise once per channel block (2 x at Ko = 512); at the network's row counts (8 x 835 rows = 105
//  time tiles) the grid is below the CU count either way, so a wider channel block would only lower the workgroup count.
//
// dle_qn_normalize_pack, dle_ctc_greedy_packed -- bound by launch latency; written for exactness of their contract.
#include "conv1d_family.h"
#include <math.h>

#define QN_TT 64           // output rows per time tile
#define QN_KB 256          // output channels per workgroup (64 per wavefront)
#define QN_CC 64           // input channels per staged chunk
#define QN_DP 72           // pitch (elements) of the d tile: the 16 rows of a ds_read_b128 lane group cover the 64 banks once
#define QN_RG 8            // output rows per depthwise thread; also the tap block

struct QnTcsArgs {
  const unsigned short* x;      // [total_in, C]
  const unsigned short* dw;     // [ksize, C]
  const unsigned short* pw;     // [Ko, C]
  const float* scale;           // [Ko]
  const float* shift;           // [Ko]
  const unsigned short* res;    // [total_out, Ko] or null
  unsigned short* y;            // [total_out, Ko]
  unsigned short* d_out;        // [total_out, C] or null
  const int32_t* cu_in;
  const int32_t* cu_out;
  long long total_in, total_out;
  int B, C, Ko, ksize, kp, rstage, rreal, relu;
};

template <int DT, int S, int D, bool PF>
__global__ __launch_bounds__(256) void qn_tcs_kernel(QnTcsArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned short qn_lds[];
  unsigned short* xl = qn_lds;                                   // [rstage][64]
  unsigned short* wl = xl + p.rstage * QN_CC;                    // [kp][64]
  unsigned short* dl = wl + p.kp * QN_CC;                        // [64][72]
  __shared__ long long s_where[2];                               // (sequence, tile) of this workgroup; sequence -1: none

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // The search is written out here as in js_conv1d_bn_kernel: through a shared function the prefetch form measured 1 - 2 % slower
  // per unit and 8 - 9 % slower at dilation 2 (ksize 87), same registers but another scalar spilled (profiles/conv1d_family_variants.md).
  if (wave == 0) {
    const long long g = blockIdx.x;
    long long run = 0, fb = -1, ft = 0;
    for (int b0 = 0; b0 < p.B; b0 += 64) {
      const int b = b0 + lane;
      long long n = 0;
      if (b < p.B) {
        long long si, li, so, lo;
        c1d_seq(p.cu_in, b, p.total_in, si, li);
        c1d_seq(p.cu_out, b, p.total_out, so, lo);
        n = (c1d_out_len(li, lo, S) + QN_TT - 1) / QN_TT;
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
    if (lane == 0) { s_where[0] = fb; s_where[1] = ft; }
  }
  __syncthreads();
  if (s_where[0] < 0) return;                                      // workgroup-uniform, before any other barrier
  const int b = (int)s_where[0];
  const long long t0 = s_where[1] * QN_TT;                         // first output row of the tile inside its sequence
  long long in0, in_len, out0, out_len;
  c1d_seq(p.cu_in, b, p.total_in, in0, in_len);
  c1d_seq(p.cu_out, b, p.total_out, out0, out_len);
  out_len = c1d_out_len(in_len, out_len, S);
  const int live = (int)(out_len - t0 < QN_TT ? out_len - t0 : QN_TT);     // >= 1 by construction
  const int nts = live > 32 ? 2 : 1;

  const int fr = lane & 31, fh = lane >> 5;
  const int kob = blockIdx.y * QN_KB + wave * 64;
  const bool wave_on = kob < p.Ko;                                 // Ko % 64 == 0: a wavefront's 64 channels are inside or outside whole
  const unsigned short* xs = p.x + in0 * p.C;
  const long long tbase = t0 * S - (long long)(p.ksize / 2) * D;   // sequence time of staged row 0

  float16_t acc[2][2];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][nt][i] = 0.f;

  const int cp = threadIdx.x & 31, rg = threadIdx.x >> 5;          // depthwise: channel pair, row group
  const int p0 = rg * QN_RG;
  const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};

  // The staging below stays private to this kernel: through c1d_stage_load / c1d_stage_store (conv1d_family.h) the prefetch form
  // went from 2 to 28 - 45 scalar spills and from 251 to 255 VGPRs.
  // The staged operands of one chunk in two halves, so that the global loads of chunk i + 1 are in flight while chunk i is
  // computed: qn_load reads the input rows and the taps into registers (thread = 8 channels of rows r0, r0 + 32, ...; zeros outside
  // [0, len) of the own sequence and for the padding taps), qn_store writes them to LDS behind the barrier.
  constexpr int XI = 10, WI = 4;                                   // rstage <= 318 rows, kp <= 128 taps: 32 per pass
  ushort8_t xr[XI], wr[WI];
  const int cc = threadIdx.x & 7, r0 = threadIdx.x >> 3;
  auto qn_load = [&](int c0) {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int r = r0 + 32 * i;
      const long long t = tbase + r;
      xr[i] = zero;
      if (r < p.rreal && t >= 0 && t < in_len) xr[i] = *(const ushort8_t*)(xs + t * p.C + c0 + cc * 8);
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int k = r0 + 32 * i;
      wr[i] = zero;
      if (k < p.ksize) wr[i] = *(const ushort8_t*)(p.dw + (long long)k * p.C + c0 + cc * 8);
    }
  };
  auto qn_store = [&]() {
#pragma unroll
    for (int i = 0; i < XI; ++i) {
      const int r = r0 + 32 * i;
      if (r < p.rstage) *(ushort8_t*)(xl + r * QN_CC + cc * 8) = xr[i];
    }
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int k = r0 + 32 * i;
      if (k < p.kp) *(ushort8_t*)(wl + k * QN_CC + cc * 8) = wr[i];
    }
  };

  // PF: LDS-only barriers (a full barrier would wait for the prefetch); otherwise the plain barrier
  auto qn_barrier = [&]() { if (PF) lds_barrier(); else __syncthreads(); };

  if (PF) qn_load(0);
  for (int c0 = 0; c0 < p.C; c0 += QN_CC) {
    // A fragments of this chunk: lane = ko, channels c0 + 16 ks + 8 fh + e
    ushort8_t wf[2][4];
    if (wave_on) {
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          wf[nb][ks] = *(const ushort8_t*)(p.pw + (long long)(kob + nb * 32 + fr) * p.C + c0 + ks * 16 + fh * 8);
    }
    if (c0) qn_barrier();                                          // the previous chunk's depthwise and MFMAs are done with LDS
    if (PF) {
      qn_store();
      if (c0 + QN_CC < p.C) qn_load(c0 + QN_CC);                   // in flight during this chunk's depthwise and MFMAs
    } else {
      for (int r = r0; r < p.rstage; r += 32) {
        const long long t = tbase + r;
        ushort8_t v = zero;
        if (r < p.rreal && t >= 0 && t < in_len) v = *(const ushort8_t*)(xs + t * p.C + c0 + cc * 8);
        *(ushort8_t*)(xl + r * QN_CC + cc * 8) = v;
      }
      for (int k = r0; k < p.kp; k += 32) {
        ushort8_t v = zero;
        if (k < p.ksize) v = *(const ushort8_t*)(p.dw + (long long)k * p.C + c0 + cc * 8);
        *(ushort8_t*)(wl + k * QN_CC + cc * 8) = v;
      }
    }
    qn_barrier();
    if (p0 < live) {
      constexpr int NX = 7 * S + 7 * D + 1;
      float a[QN_RG][2];
#pragma unroll
      for (int r = 0; r < QN_RG; ++r) a[r][0] = a[r][1] = 0.f;
      const unsigned* xw = (const unsigned*)xl + cp;
      const unsigned* ww = (const unsigned*)wl + cp;
      for (int k0 = 0; k0 < p.kp; k0 += QN_RG) {
        float w[QN_RG][2], xv[NX][2];
#pragma unroll
        for (int kk = 0; kk < QN_RG; ++kk) {
          const unsigned u = ww[(k0 + kk) * (QN_CC / 2)];
          w[kk][0] = Elem<DT>::to_f32((unsigned short)(u & 0xffffu));
          w[kk][1] = Elem<DT>::to_f32((unsigned short)(u >> 16));
        }
        const int rb = p0 * S + k0 * D;                            // <= rstage - NX
#pragma unroll
        for (int j = 0; j < NX; ++j) {
          const unsigned u = xw[(rb + j) * (QN_CC / 2)];
          xv[j][0] = Elem<DT>::to_f32((unsigned short)(u & 0xffffu));
          xv[j][1] = Elem<DT>::to_f32((unsigned short)(u >> 16));
        }
        // the padding taps of the last block are SKIPPED, not multiplied by zero: 0 x inf would put a NaN where the sum has none
#pragma unroll
        for (int kk = 0; kk < QN_RG; ++kk) {
          if (k0 + kk >= p.ksize) break;                           // workgroup-uniform
#pragma unroll
          for (int r = 0; r < QN_RG; ++r) {
            a[r][0] = __builtin_fmaf(w[kk][0], xv[r * S + kk * D][0], a[r][0]);
            a[r][1] = __builtin_fmaf(w[kk][1], xv[r * S + kk * D][1], a[r][1]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < QN_RG; ++r) {
        const unsigned u = (unsigned)Elem<DT>::from_f32(a[r][0]) | ((unsigned)Elem<DT>::from_f32(a[r][1]) << 16);
        *(unsigned*)(dl + (p0 + r) * QN_DP + cp * 2) = u;
        if (p.d_out && blockIdx.y == 0 && p0 + r < live)
          *(unsigned*)(p.d_out + (out0 + t0 + p0 + r) * p.C + c0 + cp * 2) = u;
      }
    }
    qn_barrier();
    if (wave_on) {
      const unsigned short* win = dl + fr * QN_DP + fh * 8;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
          if (nt < nts) {
            const ushort8_t fa = *(const ushort8_t*)(win + nt * 32 * QN_DP + ks * 16);
#pragma unroll
            for (int nb = 0; nb < 2; ++nb) acc[nb][nt] = Mfma32x16<DT>::run(wf[nb][ks], fa, acc[nb][nt]);
          }
    }
  }
  if (!wave_on) return;

  // D: lane owns row fr of the sub-tile, channels kob + 32 nb + 8 (i >> 2) + 4 fh + (i & 3)
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int t = nt * 32 + fr;
    if (t >= live) continue;
    const long long row = (out0 + t0 + t) * p.Ko;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
      c1d_epilogue_bn<DT>(acc[nb][nt], p.scale, p.shift, p.res, p.y, row, kob + nb * 32, fh, p.relu);
  }
}

template <int DT, bool PF>
static void qn_tcs_launch(const QnTcsArgs& p, dim3 grid, int lds, int stride, int dilation, hipStream_t stream) {
#define QN_KERNEL(S, D) qn_tcs_kernel<DT, S, D, PF>                 // DT, PF: this function's
  C1D_LAUNCH_SD(QN_KERNEL, stride, dilation, grid, dim3(256), lds, stream, p);
#undef QN_KERNEL
}

static std::atomic<int> qn_pf_mode{2};
extern "C" int dle_tcs_prefetch_mode(int mode) {
  const int old = qn_pf_mode.load(std::memory_order_relaxed);
  if (mode >= 0 && mode <= 2) qn_pf_mode.store(mode, std::memory_order_relaxed);
  return old;
}

extern "C" int dle_tcs_conv1d_packed_fwd(const void* x, const void* dw, const void* pw, const float* scale, const float* shift,
                                         const void* residual, void* y, void* d_out, const int32_t* cu_in, const int32_t* cu_out,
                                         int B, int64_t total_in, int64_t total_out, int C, int Ko, int ksize, int stride,
                                         int dilation, int relu, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "tcs_conv1d_packed_fwd: 16-bit activations and weights only");
  DLE_CHECK_ARG(c1d_batch_ok(B, total_in, total_out), "tcs_conv1d_packed_fwd: bad batch / total rows");
  DLE_CHECK_ARG(C >= 64 && C <= 1024 && C % 64 == 0, "tcs_conv1d_packed_fwd: C must be a multiple of 64 in [64, 1024] (got %d)", C);
  DLE_CHECK_ARG(Ko >= 64 && Ko <= 1024 && Ko % 64 == 0, "tcs_conv1d_packed_fwd: Ko must be a multiple of 64 in [64, 1024] (got %d)", Ko);
  DLE_CHECK_ARG(ksize >= 3 && ksize <= 127 && (ksize & 1), "tcs_conv1d_packed_fwd: ksize must be odd in [3, 127] (got %d)", ksize);
  DLE_CHECK_ARG((stride == 1 || stride == 2) && (dilation == 1 || dilation == 2) && !(stride == 2 && dilation == 2),
                "tcs_conv1d_packed_fwd: stride and dilation in {1, 2}, not both 2 (got %d, %d)", stride, dilation);
  if (total_out == 0) return 0;
  DLE_CHECK_ARG(x && dw && pw && scale && shift && y && cu_in && cu_out, "tcs_conv1d_packed_fwd: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(x, dw, pw, scale, shift, residual, y, d_out) && dle_aligned<4>(cu_in, cu_out),
                "tcs_conv1d_packed_fwd: x, dw, pw, scale, shift, residual, y and d_out must be 16-byte aligned");
  const long long xbytes = (long long)total_in * C * 2, ybytes = (long long)total_out * Ko * 2, dbytes = (long long)total_out * C * 2;
  DLE_CHECK_ARG(c1d_under_4gib(xbytes, ybytes), "tcs_conv1d_packed_fwd: each tensor must be smaller than 4 GiB");
  DLE_CHECK_ARG(!c1d_overlap(x, xbytes, y, ybytes) && !c1d_overlap(residual, ybytes, y, ybytes) && !c1d_overlap(d_out, dbytes, y, ybytes) &&
                    !c1d_overlap(d_out, dbytes, x, xbytes) && !c1d_overlap(d_out, dbytes, residual, ybytes),
                "tcs_conv1d_packed_fwd: y and d_out must not overlap x, residual or each other");
  QnTcsArgs p;
  p.x = (const unsigned short*)x; p.dw = (const unsigned short*)dw; p.pw = (const unsigned short*)pw; p.scale = scale; p.shift = shift;
  p.res = (const unsigned short*)residual; p.y = (unsigned short*)y; p.d_out = (unsigned short*)d_out; p.cu_in = cu_in; p.cu_out = cu_out;
  p.total_in = total_in; p.total_out = total_out; p.B = B; p.C = C; p.Ko = Ko; p.ksize = ksize; p.relu = relu;
  p.kp = (ksize + QN_RG - 1) / QN_RG * QN_RG;
  p.rreal = (QN_TT - 1) * stride + 1 + (ksize - 1) * dilation;
  p.rstage = (QN_TT - 1) * stride + 1 + (p.kp - 1) * dilation;
  const int lds = (p.rstage * QN_CC + p.kp * QN_CC + QN_TT * QN_DP) * 2;
  const long long gx = total_out / QN_TT + B;
  DLE_CHECK_ARG(gx <= 0x7FFFFFFFLL, "tcs_conv1d_packed_fwd: too many time tiles");
  const dim3 grid((unsigned)gx, (unsigned)((Ko + QN_KB - 1) / QN_KB));
  // PF, the register prefetch of the next chunk behind LDS-only barriers: 237 - 251 VGPRs, ONE wavefront per SIMD, so one workgroup
  // per CU.  While the grid gives a CU at most one workgroup anyway, the kernel waits on its own loads and the prefetch pays; with
  // more workgroups than CUs the plain form (144 - 158 VGPRs, two workgroups per CU, which cover each other's loads) is the faster
  // one.  Both forms compute the same bits; dle_tcs_prefetch_mode forces one of them (tests, A/B timing).
  const DleDeviceLimits* lim = dle_device_limits();
  const int mode = qn_pf_mode.load(std::memory_order_relaxed);
  const bool pf = mode == 2 ? gx * (long long)grid.y <= (lim ? lim->cus : 256) : mode == 1;
  if (dtype == DLE_F16) { if (pf) qn_tcs_launch<DLE_F16, true>(p, grid, lds, stride, dilation, stream); else qn_tcs_launch<DLE_F16, false>(p, grid, lds, stride, dilation, stream); }
  else { if (pf) qn_tcs_launch<DLE_BF16, true>(p, grid, lds, stride, dilation, stream); else qn_tcs_launch<DLE_BF16, false>(p, grid, lds, stride, dilation, stream); }
  DLE_LAUNCH_CHECK();
  return 0;
}

// ---- per-feature normalisation + mask + transpose + 16-bit cast ------------------------------------------------------------------
// one workgroup per (sequence, 8 features): wavefront w takes the statistics of features 2w, 2w + 1 (two passes in fp32: the mean,
// then the squared deviations from it), then every thread writes whole 16-byte groups of 8 features.  `lead` zero rows stand in
// front of every sequence (dle_qn_normalize_pack_lead; Jasper/inference.py:329-333): the table counts them, the statistics do not.
template <int DT>
__global__ __launch_bounds__(256) void qn_normalize_pack_kernel(const float* x, unsigned short* y, const int32_t* cu, long long total,
                                                                int F, int t_pad, int lead) {
  __shared__ float s_mean[8], s_den[8];
  const int b = blockIdx.x, f0 = blockIdx.y * 8;
  long long start, len;
  c1d_seq(cu, b, total, start, len);
  if (lead > 0) {                                                   // workgroup-uniform
    const long long nz = len < lead ? len : lead;
    const ushort8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long t = threadIdx.x; t < nz; t += 256) *(ushort8_t*)(y + (start + t) * F + f0) = zero;
    start += nz;
    len -= nz;
  }
  if (len > t_pad) len = t_pad;
  if (len <= 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = (int)len;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int f = wave * 2 + j;
    const float* row = x + ((long long)b * F + f0 + f) * t_pad;
    float s = 0.f;
    for (int t = lane; t < n; t += 64) s += row[t];
    s = wave_sum(s);
    const float mean = s / (float)n;
    float q = 0.f;
    for (int t = lane; t < n; t += 64) { const float dv = row[t] - mean; q = __builtin_fmaf(dv, dv, q); }
    q = wave_sum(q);
    if (lane == 0) {
      s_mean[f] = mean;
      s_den[f] = __fsqrt_rn(q / (float)(n - 1)) + 1e-5f;            // n = 1: 0 / 0 = NaN, as the reference; the host rejects it
    }
  }
  __syncthreads();
  for (int t = threadIdx.x; t < n; t += 256) {
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = __fdiv_rn(x[((long long)b * F + f0 + e) * t_pad + t] - s_mean[e], s_den[e]);
    *(ushort8_t*)(y + (start + t) * F + f0) = pack8<DT>(o);
  }
}

extern "C" int dle_qn_normalize_pack_lead(const float* x, void* y, const int32_t* cu_seqlens, int B, int F, int T_pad, int lead,
                                          int64_t total, int dtype, hipStream_t stream) {
  DLE_CHECK_ARG(lead >= 0 && lead <= 65536, "qn_normalize_pack: lead must be in [0, 65536] (got %d)", lead);
  DLE_CHECK_ARG(dtype == DLE_F16 || dtype == DLE_BF16, "qn_normalize_pack: 16-bit output only");
  DLE_CHECK_ARG(B >= 1 && B <= 65535 && total >= 0 && total < (1LL << 31), "qn_normalize_pack: bad batch / total rows");
  DLE_CHECK_ARG(F >= 8 && F <= 128 && F % 8 == 0, "qn_normalize_pack: F must be a multiple of 8, <= 128 (got %d)", F);
  DLE_CHECK_ARG(T_pad >= 1 && (long long)B * F * T_pad < (1LL << 31), "qn_normalize_pack: bad T_pad (%d)", T_pad);
  if (total == 0) return 0;
  DLE_CHECK_ARG(x && y && cu_seqlens, "qn_normalize_pack: null pointer");
  DLE_CHECK_ARG(dle_aligned<16>(y) && dle_aligned<4>(x, cu_seqlens), "qn_normalize_pack: y must be 16-byte aligned");
  const dim3 grid((unsigned)B, (unsigned)(F / 8)), block(256);
  if (dtype == DLE_F16)
    hipLaunchKernelGGL((qn_normalize_pack_kernel<DLE_F16>), grid, block, 0, stream, x, (unsigned short*)y, cu_seqlens, (long long)total, F, T_pad, lead);
  else
    hipLaunchKernelGGL((qn_normalize_pack_kernel<DLE_BF16>), grid, block, 0, stream, x, (unsigned short*)y, cu_seqlens, (long long)total, F, T_pad, lead);
  DLE_LAUNCH_CHECK();
  return 0;
}

extern "C" int dle_qn_normalize_pack(const float* x, void* y, const int32_t* cu_seqlens, int B, int F, int T_pad, int64_t total,
                                     int dtype, hipStream_t stream) {
  return dle_qn_normalize_pack_lead(x, y, cu_seqlens, B, F, T_pad, 0, total, dtype, stream);
}

// ---- log_softmax + argmax + the CTC collapse ---------------------------------------------------------------------------------------
// one workgroup per sequence.  Phase 1: a wavefront per row (lane l takes classes l, l + 64, ... in ascending order; the reduction
// prefers the larger value and, between equal values, the smaller index: the FIRST maximum).  Phase 2: the rows in blocks of 256, one
// per thread: keep = (id != previous or previous == blank) and id != blank with previous = blank in front of the sequence's first
// row; the kept ids are written in order behind a ballot prefix count.
__global__ __launch_bounds__(256) void qn_ctc_greedy_kernel(const float* logits, float* logp, int32_t* ids, int32_t* tokens,
                                                            int32_t* n_tokens, const int32_t* cu, long long total, int n_classes,
                                                            int ld) {
  __shared__ int s_cnt[4];
  const int b = blockIdx.x;
  long long start, len;
  c1d_seq(cu, b, total, start, len);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int blank = n_classes - 1;
  for (long long r = wave; r < len; r += 4) {
    const float* row = logits + (start + r) * ld;
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int c = lane; c < n_classes; c += 64) {
      const float v = row[c];
      if (v > m || mi == 0x7fffffff) { m = v; mi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float om = __shfl_xor(m, o, 64);
      const int oi = __shfl_xor(mi, o, 64);
      if (oi != 0x7fffffff && (mi == 0x7fffffff || om > m || (om == m && oi < mi))) { m = om; mi = oi; }
    }
    if (lane == 0) ids[start + r] = mi;
    if (logp) {
      float s = 0.f;
      for (int c = lane; c < n_classes; c += 64) s += expf(row[c] - m);
      s = wave_sum(s);
      const float ls = logf(s);
      for (int c = lane; c < n_classes; c += 64) logp[(start + r) * n_classes + c] = (row[c] - m) - ls;
    }
  }
  __syncthreads();                                                     // this workgroup's ids are visible to all of its threads
  int run = 0;
  for (long long r0 = 0; r0 < len; r0 += 256) {
    const long long r = r0 + threadIdx.x;
    int id = blank;
    bool keep = false;
    if (r < len) {
      id = ids[start + r];
      const int prev = r > 0 ? ids[start + r - 1] : blank;
      keep = (id != prev || prev == blank) && id != blank;
    }
    const unsigned long long bal = __ballot(keep);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int base = run;
    for (int w = 0; w < wave; ++w) base += s_cnt[w];
    if (keep) tokens[start + base + before] = id;
    run += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_tokens[b] = run;
}

extern "C" int dle_ctc_greedy_packed(const float* logits, float* logp, int32_t* ids, int32_t* tokens, int32_t* n_tokens,
                                     const int32_t* cu_seqlens, int B, int64_t total, int n_classes, int ld, hipStream_t stream) {
  DLE_CHECK_ARG(c1d_batch_ok(B, total, total), "ctc_greedy_packed: bad batch / total rows");
  DLE_CHECK_ARG(n_classes >= 2 && n_classes <= 4096 && ld >= n_classes && ld <= 65536,
                "ctc_greedy_packed: 2 <= n_classes <= 4096 and n_classes <= ld (got %d, %d)", n_classes, ld);
  DLE_CHECK_ARG(n_tokens && cu_seqlens && (total == 0 || (logits && ids && tokens)), "ctc_greedy_packed: null pointer");
  DLE_CHECK_ARG(dle_aligned<4>(logits, logp, ids, tokens, n_tokens, cu_seqlens), "ctc_greedy_packed: misaligned operand");
  hipLaunchKernelGGL(qn_ctc_greedy_kernel, dim3((unsigned)B), dim3(256), 0, stream, logits, logp, ids, tokens, n_tokens, cu_seqlens,
                     (long long)total, n_classes, ld);
  DLE_LAUNCH_CHECK();
  return 0;
}
