// dle_gemm: argument checks and the route -- which kernel of the family takes a call.  No kernel lives here.
//
//   C[M,N] = epilogue( alpha * sum_k A(m,k) * B(n,k) )          (operand storage and epilogues: gemm.hip, gemm_family.h)
//
// The routes are tried in this order; each `*_try` declines (0) outside its own envelope and the next one is asked.
//
//   route                      file             asked when                                               measured (profiles/)
//   -------------------------  ---------------  -------------------------------------------------------  -------------------------------------------
//   1 small-M weight stream    gemm_smallm.hip  M <= 256, both operands k-contiguous, no split-K, no     recurrent steps and heads: N / 16..32
//                                               aux, epilogue none / ADD                                  workgroups instead of a dozen 128x128 tiles
//   2 masked add, ping-pong    gemm8.hip        ADD_MASKED data gradient (A k-, B row-contiguous),       K = 512: 57 against 63 us; K = 256: 71 against
//                                               K >= 512, M <= 65536, no bias / alpha / accumulate        63 us, so K < 512 goes on to route 3
//   3 channel-widening stream  gemm_expand.hip  A k-contiguous, K in {64, 128, 256}, N >= 2 K,           store-only K = 64 stays on the tile kernel's
//                                               M >= 4096, epilogue none (K >= 128) / ADD / ADD_MASKED    PLAIN epilogue: 135 against 152 us
//   4 LDS-DMA tiles            gemm_dma.hip     K > 0, 16-byte aligned operands, K and pitches           tries the ping-pong kernel first (M, N >= 256,
//                                               multiples of 8                                            >= 128 items), then its 256x256 / 128x128 tiles
//   5 register-staged tiles    gemm.hip         everything else (unaligned / tiny shapes)                epilogues up to RELU_BWD only
#include "gemm_family.h"

// row limit of route 2: 7 x 7 at batch 256 (above it the streaming kernel of route 3 is faster)
static const int GEMM8_MASKED_MAX_M = 65536;

// C ABI.  a_kc / b_kc: operand stored with the contraction dimension contiguous (see gemm.hip).
extern "C" int dle_gemm(const void* A, const void* B, void* C, void* aux, const float* bias,
                        const void* mask_src, int M, int N, int K, int64_t lda, int64_t ldb,
                        int64_t ldc, int a_kc, int b_kc, int in_dtype, int out_dtype, int act,
                        int splitk, int accumulate, float alpha, void* workspace, int64_t workspace_bytes,
                        hipStream_t stream) {
  DLE_CHECK_ARG(A && B && C, "gemm: null pointer");
  DLE_CHECK_ARG(M >= 0 && N >= 0 && K >= 0, "gemm: negative dimension");
  DLE_CHECK_ARG(in_dtype == DLE_F16 || in_dtype == DLE_BF16, "gemm: inputs must be f16/bf16 (got %d)", in_dtype);
  DLE_CHECK_ARG(out_dtype == DLE_F32 || out_dtype == DLE_F16 || out_dtype == DLE_BF16, "gemm: bad out dtype");
  DLE_CHECK_ARG(!(a_kc == 0 && b_kc != 0), "gemm: (A m-contiguous, B k-contiguous) is not a hot-path layout");
  const bool needs_src = act_needs_src(act);
  DLE_CHECK_ARG(act >= ACT_NONE && act <= ACT_LAST_PUBLIC, "gemm: unknown epilogue %d", act);
  DLE_CHECK_ARG(!needs_src || mask_src, "gemm: this epilogue needs mask_src");
  DLE_CHECK_ARG(act != ACT_ADD_MASKED || (aux && (ldc & 7) == 0), "gemm: the masked add reads its keep bits through aux (ldc a multiple of 8)");
  DLE_CHECK_ARG(act != ACT_GELU_DAUX || aux, "gemm: DLE_ACT_GELU_DAUX writes the derivative to aux");
  DLE_CHECK_ARG(!needs_src || out_dtype == in_dtype, "gemm: mask_src dtype = in dtype = out dtype");
  if (splitk < 1) splitk = 1;
  {
    const int kt = K > 0 ? (K + BK - 1) / BK : 1;
    if (splitk > kt) splitk = kt;          // every K slice owns at least one K tile
  }
  if (splitk > 1)
    DLE_CHECK_ARG(out_dtype == DLE_F32 && !bias && act == ACT_NONE && !aux, "gemm: split-K needs a plain fp32 output");
  else
    DLE_CHECK_ARG(!accumulate || out_dtype == DLE_F32, "gemm: accumulate needs fp32 output");
  if (M == 0 || N == 0) return 0;

  // 1. few rows (recurrent steps, heads): the weight-streaming kernel of gemm_smallm.hip -- N / 16..32 workgroups instead of a
  // dozen 128x128 tiles
  if (K > 0 && M <= 256 && a_kc && b_kc && splitk == 1 && !aux && (act == ACT_NONE || act == ACT_ADD) &&
      (!accumulate || out_dtype == DLE_F32))
    DLE_TRY(dle_gemm_smallm_try(A, B, C, bias, mask_src, M, N, K, lda, ldb, ldc, in_dtype, out_dtype, act == ACT_ADD, accumulate,
                                alpha, stream),
            return 0);

  // 2. the masked-addend data gradient of the deepest stage's conv1 (K >= 512, M <= 65536 rows: 7 x 7 at batch 256): the
  // ping-pong kernel's source-tensor epilogue with the keep bits (gemm8_kernel.h, ACT_ADD_MASKED)
  // (K >= 512 only: at K = 256 -- 50176 x 1024 x 256, four K tiles per item -- the item is all epilogue and the streaming kernel
  //  below is faster, 63 against 71 us; at K = 512 the ping-pong kernel wins, 57 against 63 us: profiles/r06_rn50_shapes_*.txt)
  if (act == ACT_ADD_MASKED && a_kc && !b_kc && splitk == 1 && !accumulate && !bias && alpha == 1.0f && K >= 512 &&
      M <= GEMM8_MASKED_MAX_M)
    DLE_TRY(dle_gemm8_try(A, B, C, aux, bias, mask_src, M, N, K, lda, ldb, ldc, a_kc, b_kc, in_dtype, out_dtype, act, 1, 0, alpha,
                          nullptr, nullptr, stream),
            return 0);

  // 3. many rows, K <= 256, N >= 2 K (the channel-widening 1x1 convolutions): the streaming kernel of gemm_expand.hip
  // (store-only products with K = 64 stay on the tile kernel's PLAIN epilogue: 135 vs 152 us at 802816 x 256 x 64)
  if (a_kc && splitk == 1 && !accumulate && !bias && alpha == 1.0f &&
      (act == ACT_NONE ? (!aux && K >= 128) : act == ACT_ADD ? !aux : act == ACT_ADD_MASKED) && dle_gemm_expand_enabled())
    DLE_TRY(dle_gemm_expand_try(A, B, C, mask_src, act == ACT_ADD_MASKED ? aux : nullptr, nullptr, M, N, K, lda, ldb, ldc, b_kc,
                                in_dtype, out_dtype, expand_act_kind(act), stream),
            return 0);

  // 4. the LDS-DMA fed kernels (gemm_dma.hip), the ping-pong kernel first
  if (K > 0)
    DLE_TRY(dle_gemm_dma_try(A, B, C, aux, bias, mask_src, M, N, K, lda, ldb, ldc, a_kc, b_kc, in_dtype, out_dtype, act, splitk,
                             accumulate, alpha, workspace, workspace_bytes, stream),
            return 0);

  // 5. the register-staged kernel (gemm.hip)
  DLE_CHECK_ARG(act <= ACT_RELU_BWD, "gemm: epilogue %d needs the aligned (LDS-DMA) path: K, lda, ldb multiples of 8, 16-byte "
                "aligned operands", act);
  return gemm_regs_launch(A, B, C, aux, bias, mask_src, M, N, K, lda, ldb, ldc, a_kc, b_kc, in_dtype, out_dtype, act, splitk,
                          accumulate, alpha, stream);
}
