// Internal contract of the GEMM / convolution family: the epilogue codes, the tile constants every host router and kernel
// shares, the cross-file `*_try` prototypes (their one convention: common.h).  Every file of the family includes this header
// (directly or through gemm_tiles.h), so a definition that drifts from its prototype no longer compiles.
#pragma once
#include "common.h"

// tile of the register-staged (gemm.hip) and the LDS-DMA (gemm_dma.hip) kernels; BK is also the K depth of every LDS image of
// gemm_tiles.h and of the ping-pong kernel's half-tiles
#define BM 128
#define BN 128
#define BK 64

// ---- epilogue codes: the kernels' short spelling of the public DLE_ACT_* values (include/dle_mi355x.h) ---------------------
enum { ACT_NONE = DLE_ACT_NONE, ACT_RELU = DLE_ACT_RELU, ACT_GELU = DLE_ACT_GELU, ACT_RELU_BWD = DLE_ACT_RELU_BWD,
       ACT_ADD = DLE_ACT_ADD, ACT_GELU_BWD = DLE_ACT_GELU_BWD, ACT_TANH = DLE_ACT_TANH, ACT_TANH_BWD = DLE_ACT_TANH_BWD,
       ACT_ADD_MASKED = DLE_ACT_ADD_MASKED,   // C = acc + (bit ? mask_src : 0); aux = bit-packed keep bits of the addend (INPUT, 1 bit / element)
       ACT_MUL = DLE_ACT_MUL,                 // C = acc * mask_src (e.g. the GELU derivative the forward GEMM left behind)
       ACT_GELU_DAUX = DLE_ACT_GELU_DAUX,     // C = gelu(v), aux = gelu'(v) (instead of the pre-activation): the backward is a plain multiply
       ACT_LAST_PUBLIC = DLE_ACT_GELU_DAUX,
       // the ReLU of a linear layer as ONE BIT per element (ping-pong kernel only: dle_gemm8_relu_bits_try / ..._bwd_bits_try):
       // forward (EPI 1): bias + ReLU, aux RECEIVES the keep bits (bit (m N + n) & 7 of byte (m N + n) >> 3 = rounded output > 0);
       // backward (EPI 2): C = product where the bit is set, aux = those bits, NO source tensor is read
       ACT_RELU_BITS = 11, ACT_RELU_BWD_BITS = 12,
       // inference (dle_conv2d_fwd_affine; the PLAIN = 2 tile kernels of gemm_dma.hip only): C = relu(scale * acc + shift + mask_src)
       ACT_ADD_RELU = 13 };

// epilogues that read the source tensor `mask_src` (same shape / pitch / dtype as C)
inline bool act_needs_src(int act) {
  return act == ACT_RELU_BWD || act == ACT_ADD || act == ACT_GELU_BWD || act == ACT_TANH_BWD || act == ACT_ADD_MASKED || act == ACT_MUL ||
         act == ACT_ADD_RELU;
}

// the streaming kernel of gemm_expand.hip numbers its three epilogues itself (template parameter ACT of gemm_expand_kernel)
enum { EX_ACT_NONE = 0, EX_ACT_ADD = 1, EX_ACT_ADD_MASKED = 2 };
inline int expand_act_kind(int act) { return act == ACT_NONE ? EX_ACT_NONE : act == ACT_ADD ? EX_ACT_ADD : EX_ACT_ADD_MASKED; }

// DLE_GEMM_EXPAND=0 pins the tile kernels where the streaming kernel of gemm_expand.hip would run (read per call: tests switch
// it inside one process)
inline bool dle_gemm_expand_enabled() { return dle_env_int("DLE_GEMM_EXPAND", 1) != 0; }

// tile rows per walk group of the XCD-aware tile walks (tile_coords of gemm_dma.hip, gemm8_walk.h): DLE_GEMM_GM, default 8
inline int dle_gemm_gm() {
  static const int gm = dle_env_int("DLE_GEMM_GM", 8);
  return gm > 0 ? gm : 8;
}

// ---- tanh-GELU of the tile kernels' epilogues ---------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_tanh(float x) {
  const float k0 = 0.7978845608028654f, k1 = 0.044715f;
  const float u = k0 * (x + k1 * x * x * x);
  return 0.5f * x * (1.0f + fast_tanh(u));
}
// gelu(x) and d gelu / dx from one tanh
__device__ __forceinline__ float gelu_tanh_d(float x, float& d) {
  const float k0 = 0.7978845608028654f, k1 = 0.044715f;
  const float x2 = x * x;
  const float th = fast_tanh(k0 * (x + k1 * x2 * x));
  const float hp = 0.5f * (1.0f + th);
  d = hp + 0.5f * x * (1.f - th * th) * k0 * (1.f + 3.f * k1 * x2);
  return x * hp;
}

// ---- the family's `*_try` functions (convention and the DLE_TRY call-site idiom: common.h) -----------------------------------
extern "C" {
// gemm_dma.hip: the LDS-DMA tile kernels; tries the ping-pong kernel first
int dle_gemm_dma_try(const void* A, const void* B, void* C, void* aux, const float* bias, const void* mask_src, int M, int N, int K,
                     int64_t lda, int64_t ldb, int64_t ldc, int a_kc, int b_kc, int in_dtype, int out_dtype, int act, int splitk,
                     int accumulate, float alpha, void* workspace, int64_t workspace_bytes, hipStream_t stream);
// gemm8.hip: the persistent ping-pong 256 x 256 kernel
int dle_gemm8_try(const void* A, const void* B, void* C, void* aux, const float* bias, const void* src, int M, int N, int K,
                  int64_t lda, int64_t ldb, int64_t ldc, int a_kc, int b_kc, int in_dtype, int out_dtype, int act, int splitk,
                  int accumulate, float alpha, float* ws, float* stats, hipStream_t stream);
int dle_gemm8_colstats_try(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                           int dtype, float* stats, hipStream_t stream);
int dle_gemm8_relu_bwd_bits_try(const void* dY, const void* W, void* dX, const void* bits, float* colsum_partial, int M, int N,
                                int K, int64_t lddy, int64_t ldw, int dtype, hipStream_t stream);
// gemm_smallm.hip: the weight-streaming kernel for M <= 256
int dle_gemm_smallm_try(const void* A, const void* B, void* C, const float* bias, const void* src, int M, int N, int K, int64_t lda,
                        int64_t ldb, int64_t ldc, int in_dtype, int out_dtype, int act_add, int accumulate, float alpha,
                        hipStream_t stream);
// gemm_expand.hip: the streaming kernel of the channel-widening 1x1 convolutions; act = EX_ACT_*; groups = partial rows of `stats`
int dle_gemm_expand_try(const void* A, const void* B, void* C, const void* src, const void* bits, float* stats, int M, int N, int K,
                        int64_t lda, int64_t ldb, int64_t ldc, int b_kc, int in_dtype, int out_dtype, int act, hipStream_t stream);
int dle_gemm_expand_groups(int M, int N, int K);
// conv3x3.hip / conv3x3_wgrad.hip: the halo-tile 3x3 stride-1 kernels; tiles = partial rows of `stats`
int dle_conv3x3_try(const void* x, const void* w, void* y, float* stats, long long stats_bytes, int N, int H, int W, int C, int Ko,
                    int dgrad, int dtype, hipStream_t stream);
int dle_conv3x3_tiles(int N, int H, int W);
// ... its inference instantiations: y = relu?(fmaf(scale[ko], acc, shift[ko]) + residual), forward only
int dle_conv3x3_affine_try(const void* x, const void* w, void* y, const float* scale, const float* shift, const void* residual, int N,
                           int H, int W, int C, int Ko, int dtype, int relu, hipStream_t stream);
int dle_conv3x3_wgrad_try(const void* dy, const void* x, float* dw, int N, int H, int W, int C, int Ko, int dtype, int accumulate,
                          void* workspace, int64_t workspace_bytes, hipStream_t stream);
}
// gemm.hip: the register-staged kernel (any alignment, epilogues ACT_NONE .. ACT_RELU_BWD); 0 = ok, else a hipError_t
int gemm_regs_launch(const void* A, const void* B, void* C, void* aux, const float* bias, const void* mask_src, int M, int N, int K,
                     int64_t lda, int64_t ldb, int64_t ldc, int a_kc, int b_kc, int in_dtype, int out_dtype, int act, int splitk,
                     int accumulate, float alpha, hipStream_t stream);
// wgrad1x1.hip: dw (+)= the sum of the G partial blocks of `ws` (also folds the weight-gradient form of conv_bnbwd.hip)
hipError_t wgrad1x1_fold(const float* ws, float* dw, long long total4, int G, int accumulate, hipStream_t stream);
// (dle_wgrad1x1_try and dle_emb_onehot_try follow the same convention and are declared in include/dle_mi355x.h)
