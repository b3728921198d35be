/* dle_mi355x.h -- C ABI of libdle_mi355x.so, the MI355X (gfx950 / CDNA4) kernels behind the
 * NVIDIA/DeepLearningExamples AMP+DDP train-step hot path (RN50, BERT-L, DLRM).
 *
 * Conventions:
 *   - every entry point is extern "C", takes plain device pointers + sizes and a hipStream_t
 *     (pass torch.cuda.current_stream().cuda_stream), returns int: 0 = ok, -1 = invalid argument,
 *     >0 = hipError_t.  dle_last_error() returns the message (thread local).  Nothing exits the
 *     process (the reference's CHK_CUDA calls std::exit, gather_gpu_fused.cu:6-14).
 *   - inputs are borrowed, outputs are caller-allocated; no hidden allocation, no host sync,
 *     no global state -> every call is hipGraph-capturable.
 *   - dtype codes: DLE_F32 = 0, DLE_F16 = 1, DLE_BF16 = 2.
 * Paths are relative to /root/reference/PyTorch/.
 */
#ifndef DLE_MI355X_H
#define DLE_MI355X_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* hipStream_t;

enum { DLE_F32 = 0, DLE_F16 = 1, DLE_BF16 = 2 };
enum { DLE_ACT_NONE = 0, DLE_ACT_RELU = 1, DLE_ACT_GELU = 2, DLE_ACT_RELU_BWD = 3, DLE_ACT_ADD = 4,
       DLE_ACT_GELU_BWD = 5, DLE_ACT_TANH = 6, DLE_ACT_TANH_BWD = 7,
       DLE_ACT_ADD_MASKED = 8, /* C = acc + (bit ? mask_src : 0): aux is an INPUT here, the bit-packed keep bits of the
                                  addend (bit k of byte i <-> element 8 i + k of the [M, ldc] addend): the residual-branch
                                  gradient dy * (y > 0) of a ResNet block without materialising it */
       DLE_ACT_MUL = 9,        /* C = acc * mask_src */
       DLE_ACT_GELU_DAUX = 10  /* C = gelu(v), aux = gelu'(v): the backward GEMM then multiplies (DLE_ACT_MUL) */ };

/* ---- library plumbing ---------------------------------------------------------------------- */
const char* dle_last_error(void);
int dle_abi_version(void);
int dle_device_check(int device, char* arch_name, int arch_name_len); /* 0 iff gfx950 */

/* ---- DLRM dot interaction -------------------------------------------------------------------
 * replaces dlrm.cuda_ext.interaction_{ampere,volta}.dotBasedInteractFwd / dotBasedInteractBwd
 *   Recommendation/DLRM/dlrm/cuda_src/dot_based_interact_ampere/pytorch_ops.cpp:3-12
 *   .../dot_based_interact_ampere/dot_based_interact_pytorch_types.cu:10-75
 * x[B,R,C] -> out[B, OW], OW = ceil8(R(R-1)/2 + C): [x[:,0,:] | strict lower tri of X X^T | 0 pad]. */
int dle_dot_interact_out_width(int rows, int cols);
int dle_dot_interact_fwd(const void* x, void* out, int batch, int rows, int cols, int dtype,
                         int force_generic, hipStream_t stream);
/* grad[B,R,C] = U_sym X, mlp_grad[B,C] = upstream[:, :C]  (dotBasedInteractBwd returns both).
 * mlp_grad == NULL: fused form, upstream[:, :C] is added onto grad[:, 0, :] (the sum autograd forms
 * because bottom_mlp_output and input[:,0] are the same tensor, dot_based_interact_fp16_bwd.cu:329-331). */
int dle_dot_interact_bwd(const void* x, const void* upstream, void* grad, void* mlp_grad,
                         int batch, int rows, int cols, int dtype, int force_generic,
                         hipStream_t stream);
/* The same, and *found_inf = 1 when any element of grad as stored is inf / nan (left untouched otherwise): the check
 * torch's GradScaler.unscale_ makes on this gradient (dlrm/scripts/main.py:585-608 scaler.step), without a pass over it. */
int dle_dot_interact_bwd_checked(const void* x, const void* upstream, void* grad, void* mlp_grad,
                                 int batch, int rows, int cols, int dtype, int force_generic,
                                 float* found_inf, hipStream_t stream);

/* Inference: the embedding gather fused into the interaction forward (X is never materialised).  Replaces
 * FusedJointEmbedding + dotBasedInteractFwd under model.half()
 *   Recommendation/DLRM/dlrm/nn/embeddings.py:163-224, dlrm/nn/interactions.py:85-101, dlrm/scripts/main.py:520-522
 * table16: 16-bit joint table [sum rows, dim] (dtype DLE_F16 / DLE_BF16); indices int64 [batch, tables]; offsets / hash_sizes as
 * for dle_emb_gather_fwd (NULL: joint ids / no hashing; same int64 arithmetic); mlp_out [batch, dim] 16-bit = row 0 of X;
 * out [batch, OW], OW = dle_dot_interact_out_width(tables + 1, dim): [mlp_out | strict lower tri of X X^T | 0 pad], bit-identical
 * to dle_dot_interact_fwd over cat(mlp_out, table16[rows]).  Envelope: tables + 1 <= 32, dim % 16 == 0, 16-bit dtype, 16-byte
 * aligned table16 / mlp_out / out.
 * 1: launched, 0: outside the envelope (caller takes gather + dle_dot_interact_fwd), > 1 or -1: error */
int dle_dlrm_gather_interact_try(const void* table16, const int64_t* indices, const int64_t* offsets,
                                 const int64_t* hash_sizes, const void* mlp_out, void* out,
                                 int64_t batch, int tables, int dim, int dtype, hipStream_t stream);

/* ---- DLRM embeddings --------------------------------------------------------------------------
 * replaces dlrm.cuda_ext.fused_embedding.gather_gpu_fused_fwd / _bwd
 *   Recommendation/DLRM/dlrm/cuda_src/pytorch_embedding_ops.cpp:3-21, gather_gpu_fused.cu:107-220
 * and dlrm.cuda_ext.sparse_gather.gather_gpu_fwd / gather_gpu_bwd / gather_gpu_bwd_fuse_sgd
 *   Recommendation/DLRM/dlrm/cuda_src/sparse_gather/sparse_pytorch_ops.cpp:1-15, gather_gpu.cu:79-171
 * weight fp32 [sum rows, dim]; indices int64 [batch, tables]; offsets int64 [tables(+1)] or NULL when
 * indices already address the joint table; hash_sizes int64 [tables] or NULL (idx %= size).       */
/* out_batch_stride (elements, 0 = tables*dim): row (b,t) lands at out + b*stride + t*dim, so the gather
 * can write straight into rows 1.. of the [B, 1+tables, dim] interaction input (no torch.cat).        */
int dle_emb_gather_fwd(const float* weight, const int64_t* indices, const int64_t* offsets,
                       const int64_t* hash_sizes, void* out, int64_t batch, int tables, int dim,
                       int out_dtype, int64_t out_batch_stride, hipStream_t stream);
int dle_emb_offset_indices(const int64_t* indices, const int64_t* offsets, const int64_t* hash_sizes,
                           int64_t* rows_out, int64_t batch, int tables, hipStream_t stream);
/* fp32 COO values of the sparse weight gradient: values = (float)grad * (*scale_dev or 1) */
int dle_emb_grad_values(const void* grad, float* values, const float* scale_dev, int64_t n_elems,
                        int grad_dtype, hipStream_t stream);
/* W[rows[i],:] -= lr * scale * grad[i,:]; lr from lr_dev if non-NULL else lr_host; whole update is
 * skipped when *skip_flag_dev != 0 (GradScaler found_inf). */
int dle_emb_sparse_sgd(float* weight, const int64_t* rows, const void* grad, const float* lr_dev,
                       float lr_host, const float* scale_dev, const float* skip_flag_dev,
                       int64_t n_rows, int tables, int dim, int64_t grad_batch_stride, int grad_dtype,
                       hipStream_t stream);
/* Same update without float atomics (the train step's path): tiny tables are reduced in LDS, all other
 * rows through per-row lists (one 4-byte atomicExch per lookup) and ONE plain row read-modify-write.
 * head: int32[total rows] device workspace, all -1 on entry and restored on exit; next: int32[batch*tables]
 * scratch; is_small: uint8[tables] device copy of dle_emb_small_table_mask(); table_offsets_host: HOST
 * int64[tables+1].  grad row (b,t) at grad + b*grad_batch_stride + t*dim (stride 0 = tables*dim). */
int dle_emb_small_table_mask(const int64_t* table_offsets_host, int tables, int dim, unsigned char* mask_host);
int dle_emb_sgd_dedup(float* weight, const int64_t* rows, const void* grad, int32_t* head, int32_t* next,
                      const unsigned char* is_small_dev, const int64_t* table_offsets_host,
                      const float* lr_dev, float lr_host, const float* scale_dev,
                      const float* skip_flag_dev, int64_t batch, int tables, int dim,
                      int64_t grad_batch_stride, int grad_dtype, hipStream_t stream);
/* The same with a scratch buffer: tables of <= 128 rows (dim 128, 16-bit gradients) are summed as OneHot(ids)^T G on the matrix
 * pipe (csrc/emb_onehot.hip: the gradient rows stream HBM -> LDS once, the one-hot operand is built in registers; one fp32
 * partial block per (table, batch slice), folded in slice order -- bit-reproducible, no float atomics; replaces the per-lookup
 * atomicAdd of gather_gpu_fused.cu:161-202 on the tables every sample hits); tables of <= 4096 rows thread EIGHT lists per row
 * (one per residue of the sample index: the ~70-deep duplicate chains of 1-2 k-row tables become 8 chains walked side by side),
 * whose partial sums meet in a third small pass.  ws: dle_emb_sgd_workspace_bytes() bytes of scratch, 256-byte aligned, or NULL
 * (= dle_emb_sgd_dedup).  dle_emb_onehot_try is the one-hot kernel's own entry (1 launched, 0 outside its envelope; scratch
 * dle_emb_onehot_workspace_bytes): tab_t / tab_base / tab_rows = column index, first joint row, row count of each table (host).
 * Non-finite gradients: the one-hot product multiplies every gradient row into every row of a tiny table, so an inf / NaN gradient
 * row turns the WHOLE table NaN (row-local in the reference).  skip_flag_dev must therefore be final before the call (the fp16
 * path: dle_check_nonfinite on the gradient first); without a scaler a non-finite gradient loses the table instead of the row. */
int64_t dle_emb_sgd_workspace_bytes(const int64_t* table_offsets_host, int tables, int dim, int64_t batch);
int64_t dle_emb_onehot_workspace_bytes(int n_tables, int64_t batch);
int dle_emb_sgd_dedup_ws(float* weight, const int64_t* rows, const void* grad, int32_t* head, int32_t* next,
                         const unsigned char* is_small_dev, const int64_t* table_offsets_host,
                         const float* lr_dev, float lr_host, const float* scale_dev,
                         const float* skip_flag_dev, int64_t batch, int tables, int dim,
                         int64_t grad_batch_stride, int grad_dtype, void* ws, int64_t ws_bytes, hipStream_t stream);
int dle_emb_onehot_try(float* weight, const int64_t* rows, const void* grad, const float* lr_dev, float lr_host,
                       const float* scale_dev, const float* skip_flag_dev, const int* tab_t, const int64_t* tab_base,
                       const int* tab_rows, int n_tab, int64_t batch, int tables, int dim, int64_t grad_batch_stride,
                       int grad_dtype, void* ws, int64_t ws_bytes, hipStream_t stream);

/* The one-hot segment sums alone (no update): fp32 partial blocks ws[k][slice][r][128] for r < tab_rows[k], *slices_out = the
 * slice count; the sparse Adam update folds them itself.  1: launched, 0: outside the kernel's envelope, > 1: error. */
int dle_emb_onehot_partials(const int64_t* rows, const void* grad, const float* skip_flag_dev, const int* tab_t,
                            const int64_t* tab_base, const int* tab_rows, int n_tab, int64_t batch, int tables, int dim,
                            int64_t grad_batch_stride, int grad_dtype, void* ws, int64_t ws_bytes, int* slices_out,
                            hipStream_t stream);

/* ---- duplicate-free sparse Adam on the joint table (csrc/emb_adam.hip): torch.optim.SparseAdam over the joint embedding
 * (DLRM/dlrm/scripts/main.py:479-482, torch.optim._functional.sparse_adam) behind --Adam_embedding_optimizer.  Duplicate
 * lookups are summed in fp32 first; every looked-up row -- a row whose sum is exactly 0 included -- takes ONE step
 *   m += (1-b1)(g-m);  v += (1-b2)(g^2-v);  w -= lr sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps),   g = sum * (*grad_mul_dev)
 * and every other row keeps w, exp_avg (m) and exp_avg_sq (v) bit for bit.  No float atomics in global memory, no host
 * synchronisation or allocation (graph capturable).  w, m, v: fp32 [total rows, dim]; rows int64 [batch, tables] joint ids; grad
 * fp32 / fp16 / bf16, row (b,t) at grad + b*grad_batch_stride + t*dim (stride 0 = tables*dim); head / next as for
 * dle_emb_sgd_dedup_ws (head all -1 on entry and on exit); step_dev: int32 device word = t of THIS update (the caller advances
 * it); skip_flag_dev != 0: nothing is written.  The betas are passed as 1 - beta (1 - 0.999f would be 1.3e-5 off
 * the 1e-3 the reference multiplies v by).  ws: dle_emb_adam_workspace_bytes() bytes, 256-byte aligned.  tables <= 128. */
int64_t dle_emb_adam_workspace_bytes(const int64_t* table_offsets_host, int tables, int dim, int64_t batch);
int dle_emb_adam_dedup_ws(float* weight, float* exp_avg, float* exp_avg_sq, const int64_t* rows, const void* grad, int32_t* head,
                          int32_t* next, const int64_t* table_offsets_host, const float* lr_dev, float lr_host,
                          const float* grad_mul_dev, const float* skip_flag_dev, const int32_t* step_dev, float one_minus_beta1,
                          float one_minus_beta2, float eps, int64_t batch, int tables, int dim, int64_t grad_batch_stride, int grad_dtype, void* ws,
                          int64_t ws_bytes, hipStream_t stream);

/* ---- dense contraction with fused epilogue ---------------------------------------------------
 * replaces cuBLAS GEMM + NVFuser/apex epilogues: apex.mlp (Recommendation/DLRM/dlrm/nn/mlps.py:18-43),
 * F.linear + bias + gelu (LanguageModeling/BERT/modeling.py:130-165), RN50 fc.
 * C[M,N] = act(alpha * A(m,k) B(n,k) + bias[n]); a_kc/b_kc = operand stored contraction-contiguous
 * ([M][lda] / [N][ldb]) or not ([K][lda] / [K][ldb]).  aux = optional pre-activation output.
 * DLE_ACT_RELU_BWD: C = (mask_src > 0) ? acc : 0.  splitk > 1 requires a plain fp32 output; with a
 * caller-provided workspace of >= splitk*M*N*4 bytes the K slices are summed from fp32 slabs, without it by
 * fp32 atomics (10x slower on this part).                                                             */
int dle_gemm(const void* A, const void* B, void* C, void* aux, const float* bias,
             const void* mask_src, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
             int a_kc, int b_kc, int in_dtype, int out_dtype, int act, int splitk, int accumulate,
             float alpha, void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* The big linear layers (M, N >= 256, K >= 128 and a multiple of 8, >= 128 (tile, K slice) items) run on the persistent
 * ping-pong 256 x 256 kernel of csrc/gemm8.hip; dle_gemm8_mode(0 / 1) switches it off / on for A/B measurements and parity
 * tests (-1: query), returns the previous setting; environment default DLE_GEMM_8PH (1).
 * dle_gemm8_min_items(n): the item count from which dle_gemm routes a shape to that kernel (n < 0: query; environment default
 * DLE_GEMM_8PH_MIN_ITEMS, 128) -- the parity tests set 1 so that small and ragged shapes reach it; returns the previous value.
 * dle_gemm8_launch_count(): launches of that kernel by this process so far (tests assert that a call was NOT declined).  */
int dle_gemm8_mode(int mode);
int dle_gemm8_min_items(int n);
int64_t dle_gemm8_launch_count(void);
/* Epilogues that read mask_src (same shape/ld as C): RELU_BWD (mask by mask_src > 0), ADD (C = acc + mask_src),
 * GELU_BWD (acc * gelu'(mask_src), mask_src = saved pre-activation), TANH_BWD (acc * (1 - mask_src^2)).
 * Batched form (attention contractions, torch.bmm at LanguageModeling/BERT/modeling.py:354,373):
 * slice z = (z / batch_inner, z % batch_inner) of X starts at X + zo*sx_o + zi*sx_i (elements).              */
int dle_gemm_batched(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb,
                     int64_t ldc, int a_kc, int b_kc, int in_dtype, int out_dtype, float alpha, int batch,
                     int batch_inner, int64_t sa_o, int64_t sa_i, int64_t sb_o, int64_t sb_i, int64_t sc_o,
                     int64_t sc_i, hipStream_t stream);

/* ---- convolutions as implicit GEMM (csrc/gemm_dma.hip) ------------------------------------------------
 * replace cuDNN conv forward / backward-data / backward-filter behind nn.Conv2d(bias=False)
 *   Classification/ConvNets/image_classification/models/common.py:31-60, models/resnet.py:126-175
 * Layouts: activations NHWC, weights KRSC (= torch channels_last memory of an OIHW tensor), 16-bit in,
 * fp32 accumulate.  C and Ko multiples of 8; each tensor < 4 GiB.  P = (H+2*pad-R)/stride+1.
 *   fwd:   y[N,P,Q,Ko]  = conv(x[N,H,W,C], w[Ko,R,S,C]) (+bias, DLE_ACT_RELU optional)
 *   dgrad: dx[N,H,W,C]  = conv_transpose(dy[N,P,Q,Ko], w) (+ addend[N,H,W,C] if non-NULL: skip-branch sum)
 *   wgrad: dw[Ko,R,S,C] (fp32) (+)= dy^T * im2col(x); split-K slabs through the workspace                */
int dle_conv2d_fwd(const void* x, const void* w, void* y, const float* bias, int N, int H, int W, int C,
                   int Ko, int R, int S, int stride, int pad, int dtype, int out_dtype, int act,
                   hipStream_t stream);
int dle_conv2d_dgrad(const void* dy, const void* w, void* dx, const void* addend, int N, int H, int W, int C,
                     int Ko, int R, int S, int stride, int pad, int dtype, hipStream_t stream);
/* Inference: the convolution with the evaluation-mode BatchNorm, the residual add and the ReLU in its epilogue -- one launch
 * instead of conv + BatchNorm-apply, the activation is written once and rounded once.  Replaces, under model.eval(),
 *   Classification/ConvNets/image_classification/models/resnet.py:148-175 (conv -> bn -> relu, `out += residual`),
 *   classify.py:79-99 / main.py --evaluate (the forward those run)
 *   y[n,p,q,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) + float(residual[n,p,q,ko]) ) )
 * acc: the fp32 accumulator over the UNMODIFIED 16-bit KRSC weights (no folded copy); scale / shift fp32 [Ko]
 * (scale = gamma * rsqrt(running_var + eps), shift = beta - running_mean * scale); residual 16-bit [N,P,Q,Ko] or NULL;
 * round-to-nearest-even, once.  Every operand 16-byte aligned, C and Ko multiples of 8.  No allocation, no synchronisation
 * (graph capturable).  3x3 / stride 1 / pad 1 with C, Ko multiples of 64 runs on the halo-tile kernel (csrc/conv3x3.hip);
 * dle_conv3x3_affine_launch_count(): launches of that kernel by this process so far (tests assert it was NOT declined).      */
int dle_conv2d_fwd_affine(const void* x, const void* w, void* y, const float* scale, const float* shift,
                          const void* residual, int N, int H, int W, int C, int Ko, int R, int S, int stride, int pad,
                          int dtype, int relu, hipStream_t stream);
int64_t dle_conv3x3_affine_launch_count(void);
/* Inference, grouped: the 3x3 / pad 1 / stride 1 or 2 convolution with `groups` groups (conv2 of the ResNeXt bottleneck) with the
 * evaluation-mode BatchNorm and the ReLU in its epilogue.  Replaces, under model.eval(), the cuDNN grouped convolution behind
 *   Classification/ConvNets/image_classification/models/resnet.py:107-175 (Bottleneck with cardinality 32: nn.Conv2d(groups=32)
 *   -> bn2 -> relu), models/resnet.py:412-458 (resnext101-32x4d, se-resnext101-32x4d)
 *   y[n,p,q,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) ) ),   P = (H-1)/stride + 1
 * x [N,H,W,C] NHWC 16-bit; w [Ko][3][3][Cg] 16-bit = torch's grouped OIHW weight [Ko, Cg, 3, 3] permuted (0,2,3,1); acc: the fp32
 * MFMA accumulator over the UNMODIFIED 16-bit weights of ko's group only; round-to-nearest-even, once; no residual operand.
 * Envelope: C == Ko, C % 64 == 0, Cg = C / groups in {4, 8, 16, 32}, stride in {1, 2}, any H, W >= 1, each tensor < 4 GiB, every
 * operand 16-byte aligned; anything else is an argument error (-1), never a fallback.  No allocation, no synchronisation (graph
 * capturable); no dynamic LDS (csrc/conv_grouped.hip). */
int dle_conv2d_grouped_fwd_affine(const void* x, const void* w, void* y, const float* scale, const float* shift,
                                  int N, int H, int W, int C, int Ko, int groups, int stride,
                                  int dtype, int relu, hipStream_t stream);
/* Inference, squeeze-and-excitation (csrc/se.hip).  Replaces, under model.eval(),
 *   models/common.py:146-164 (SqueezeAndExcitation: mean over H x W -> nn.Linear(C, S) -> ReLU -> nn.Linear(S, C) -> sigmoid),
 *   models/resnet.py:165-173 (`out = torch.addcmul(residual, out, self.squeeze(out))`, relu)
 * se_gate:  gate[n,c] = sigmoid(b2[c] + sum_s w2[c,s] * relu(b1[s] + sum_c' w1[s,c'] * mean_hw t[n,hw,c']))
 *           t [N,HW,C] 16-bit (16-byte aligned), the mean in fp32; w1 [S,C], b1 [S], w2 [C,S], b2 [C], gate [N,C] fp32 -- both
 *           products in fp32 on fp32 weights (the reference's autocast runs them in fp16).  S <= 64, C % 8 == 0.
 * se_apply: y = round16( relu?( fmaf(float(t), gate[n,c], float(residual)) ) ), residual 16-bit [N,HW,C] or NULL, 16-byte loads and
 *           stores (every operand 16-byte aligned, C % 8 == 0).
 * No allocation, no synchronisation. */
int dle_se_gate(const void* t, const float* w1, const float* b1, const float* w2, const float* b2, float* gate,
                int N, int HW, int C, int S, int dtype, hipStream_t stream);
int dle_se_apply(const void* t, const float* gate, const void* residual, void* y,
                 int64_t N, int HW, int C, int dtype, int relu, hipStream_t stream);
/* Inference, EfficientNet's MBConv block (csrc/efficientnet.hip): the depthwise k x k convolution with the evaluation-mode
 * BatchNorm, the SiLU of the unit BEFORE it (applied to the input while it is staged), its own SiLU and the squeeze-and-excitation
 * pooling in one launch.  Replaces, under model.eval(),
 *   Classification/ConvNets/image_classification/models/common.py:31-79 (LayerBuilder.conv with groups == in_planes, padding
 *   int((k-1)/2), no bias -> BatchNorm2d -> SiLU), :123-128 (nn.SiLU), models/efficientnet.py:384-452 (MBConvBlock.depsep)
 *   a[n,h,w,c]  = in_act ? round16(silu(float(x[n,h,w,c]))) : x[n,h,w,c]                     (0 outside the image)
 *   acc         = sum_{r,s} float(w[r,s,c]) * float(a[n, p*stride + r - k/2, q*stride + s - k/2, c])          fp32 fmaf
 *   y[n,p,q,c]  = round16( out_act ? silu(v) : v ),   v = fmaf(scale[c], acc, shift[c])
 *   pool[n,g,c] = fp32 sum of float(y[n,p,q,c]) over the output pixels of tile g                 (pool == NULL: not written)
 *   P = (H + 2 (k/2) - k) / stride + 1, likewise Q;   silu(v) = v / (1 + expf(-v)), accurate expf, true division (v < -88, where
 *   expf(-v) overflows: the same quotient as v * expf(v))
 * x, y NHWC 16-bit; w [k][k][C] 16-bit = torch's [C,1,k,k] permuted (functional.pack_depthwise_weight); scale / shift fp32 [C].
 * Tiling: a workgroup owns DLE_DWCONV_TILE_ROWS x DLE_DWCONV_TILE_COLS output pixels of one image and DLE_DWCONV_CHUNK channels;
 * the input tile with its halo sits in LDS after the input SiLU (at most 88,320 bytes of dynamic LDS at k 5 / stride 2, opted in
 * per device).  Pool "bands" are those tiles, row-major: G = ceil(P / TILE_ROWS) * ceil(Q / TILE_COLS) =
 * dle_dwconv2d_pool_bands(H, W, C, ksize, stride) (host only; -1 on a bad argument).  Each partial is written once by one
 * workgroup (no atomics) and summed over its pixels in a fixed order: bitwise reproducible.  pool_bytes >= N * G * C * 4.
 * Envelope: C % 8 == 0, ksize in {3, 5}, stride in {1, 2}, any H, W >= 1, in_act / out_act in {0, 1}, every operand 16-byte
 * aligned, each tensor below 2^31 elements; anything else is an argument error (-1), never a fallback.  No allocation, no
 * synchronisation (graph capturable). */
#define DLE_DWCONV_TILE_ROWS 8
#define DLE_DWCONV_TILE_COLS 16
#define DLE_DWCONV_CHUNK 64
int dle_dwconv2d_act_fwd(const void* x, const void* w, void* y, const float* scale, const float* shift, float* pool,
                         int64_t pool_bytes, int N, int H, int W, int C, int ksize, int stride, int in_act, int out_act,
                         int dtype, hipStream_t stream);
int dle_dwconv2d_pool_bands(int H, int W, int C, int ksize, int stride);
/* The squeeze-and-excitation gate of an MBConv block from the pool partials of dle_dwconv2d_act_fwd.  Replaces, under
 * model.eval(), models/common.py:146-164 and :231-250 (SequentialSqueezeAndExcitation._attention with the SiLU activation)
 *   mean[n,c] = inv_hw * (pool[n,0,c] + pool[n,1,c] + ... + pool[n,G-1,c], in this order)
 *   gate[n,c] = sigmoid(b2[c] + sum_s w2[c,s] * f(b1[s] + sum_c' w1[s,c'] * mean[n,c'])),   f = SiLU (act 1) or ReLU (act 0)
 * pool [N,G,C], w1 [S,C], b1 [S], w2 [C,S], b2 [C], gate [N,C], all fp32 -- both products in fp32 on fp32 weights (the
 * reference's autocast runs them in fp16).  Any S >= 1; the mean and the hidden vector live in LDS (64 KiB, no opt-in), so
 * C + S <= DLE_SE_GATE_ACT_MAX_C_PLUS_S; C % 8 == 0.  No allocation, no synchronisation.  dle_se_gate is unchanged. */
#define DLE_SE_GATE_ACT_MAX_C_PLUS_S 16384
int dle_se_gate_act(const float* pool, int G, float inv_hw, const float* w1, const float* b1, const float* w2,
                    const float* b2, float* gate, int N, int C, int S, int act, hipStream_t stream);
/* The features unit's SiLU with AdaptiveAvgPool2d(1) behind it (models/efficientnet.py:289-310, common.py:123-128):
 *   y[n,c] = round16( (1/HW) * sum_hw float(round16(silu(float(x[n,hw,c])))) ),  the fp32 sum in a fixed order
 * x [N,HW,C] 16-bit (16-byte aligned), y [N,C] 16-bit, C % 8 == 0, x below 2^31 elements.  No allocation, no synchronisation. */
int dle_silu_avgpool_fwd(const void* x, void* y, int N, int HW, int C, int dtype, hipStream_t stream);
/* Inference, SSD300 detection post-processing (csrc/ssd.hip): three launches, fixed-size outputs, no host read.
 *
 * dle_ssd_decode_fwd: head outputs -> boxes and class probabilities.  Replaces Detection/SSD/ssd/model.py:108-115
 * (SSD300.bbox_view) and ssd/utils.py:127-159 (Encoder.scale_back_batch).
 *   heads[m] (a HOST array of nmaps <= DLE_SSD_MAX_MAPS device pointers): the 16-bit NHWC head tensor [N, fs, fs, pitch] of map m;
 *   geom (a HOST array of 5 ints per map): fs, nd, pitch, loc, conf -- channels [loc, loc + 4 nd) are the location part, channels
 *   [conf, conf + L nd) the confidence part (both inside the pitch; what else the pitch holds is not read).
 *   INDEX RULE.  The reference reshapes the NCHW head output [N, nd*4, H, W] to [N, 4, nd*H*W] (and [N, nd*L, H, W] to
 *   [N, L, nd*H*W]), so channel c of the location part is coordinate c / nd of anchor c % nd, channel c of the confidence part is
 *   label c / nd of anchor c % nd, and the box of (anchor a, pixel h, w) has index a*H*W + h*W + w inside its map; the maps follow
 *   each other in table order, B = sum nd * fs * fs.
 *   fp32, every operation rounded on its own (no contraction), as the reference after .float():
 *     x = (scale_xy * loc_x) * d_w + d_x   (y likewise)      w = expf(scale_wh * loc_w) * d_w   (h likewise)
 *     boxes[n,b] = (x - 0.5 w, y - 0.5 h, x + 0.5 w, y + 0.5 h)       probs[n,l,b] = expf(c_l - max_l c) / sum_l expf(c_l - max_l c)
 *   dboxes_xywh [B,4] fp32 (16-byte aligned); boxes [N,B,4] fp32; probs [N,L,B] fp32, class-major (dle_ssd_nms_fwd reads rows).
 *   loc == 0 returns d_xy -+ 0.5 d_wh exactly.  L >= 2, B < 2^24, N * L * B < 2^31.
 *
 * dle_ssd_nms_fwd: one workgroup per (image, label 1..L-1).  Replaces the body of the class loop of Encoder.decode_single
 * (ssd/utils.py:179-209) with calc_iou_tensor (utils.py:32-66).
 *   candidates: the boxes with probs[n,l,b] > threshold (the reference: 0.05); the max_num best are kept (the reference: 200),
 *   best = higher probability, then LOWER box index (the reference's sort leaves the order of equal scores open; this is the rule
 *   here); greedy from the best downwards: a candidate survives a kept one only if iou < criteria -- written !(iou < criteria)
 *   suppresses, so a NaN (a zero-area box against itself, 0/0) suppresses, as the reference's boolean index drops it.
 *   iou: calc_iou_tensor's fp32 operations in its order -- max, min, subtract, clamp at 0, multiply, the two areas,
 *   (area1 + area2) - intersect, a correctly rounded division -- without contraction: on the same fp32 boxes and scores the kept
 *   set is the reference's bit for bit.
 *   kept_idx [N,L-1,max_num] int32 (box indices, best first; -1 past the count), kept_score [N,L-1,max_num] fp32 (0 past the
 *   count), kept_count [N,L-1] int32.  1 <= max_num <= DLE_SSD_MAX_KEEP, 1 <= B <= DLE_SSD_MAX_BOXES (the candidates' 64-bit keys are
 *   sorted in LDS: 8 * pow2(B) + 14,368 bytes, opted in per device), boxes 16-byte aligned.  No atomics: deterministic.
 *
 * dle_ssd_select_fwd: one workgroup per image.  Replaces the tail of decode_single (utils.py:211-221).
 *   the max_output best of all kept candidates, best first: higher score, then lower label, then lower box index.
 *   det_boxes [N,max_output,4] fp32 (16-byte aligned), det_label (1..L-1), det_score, det_idx (the default-box index)
 *   [N,max_output], det_count [N]; rows past the count are zero.  max_output <= DLE_SSD_MAX_KEEP and
 *   (L - 1) * min(max_num, max_output) <= DLE_SSD_MAX_BOXES (only the first max_output entries of a class can be selected; they
 *   are sorted in LDS).
 * All three: a bad argument returns -1 without a launch; no allocation, no synchronisation (graph capturable). */
#define DLE_SSD_MAX_MAPS 8
#define DLE_SSD_MAX_KEEP 256
#define DLE_SSD_MAX_BOXES 16384
int dle_ssd_decode_fwd(const void* const* heads, const int* geom, int nmaps, const float* dboxes_xywh, float* boxes, float* probs,
                       int N, int B, int L, float scale_xy, float scale_wh, int dtype, hipStream_t stream);
int dle_ssd_nms_fwd(const float* boxes, const float* probs, int* kept_idx, float* kept_score, int* kept_count, int N, int B, int L,
                    float threshold, float criteria, int max_num, hipStream_t stream);
int dle_ssd_select_fwd(const float* boxes, const int* kept_idx, const float* kept_score, const int* kept_count, float* det_boxes,
                       int* det_label, float* det_score, int* det_idx, int* det_count, int N, int B, int L, int max_num,
                       int max_output, hipStream_t stream);
int dle_conv2d_wgrad(const void* dy, const void* x, float* dw, int N, int H, int W, int C, int Ko, int R, int S,
                     int stride, int pad, int dtype, int splitk, int accumulate, void* workspace,
                     int64_t workspace_bytes, hipStream_t stream);
/* dw [Ko, C] fp32 (+)= dy [M, Ko]^T x [M, C] for the 1x1 convolutions whose whole output fits one workgroup's accumulators
 * ((Ko, C) in {(256,64), (64,256), (64,64), (128,256), (256,128), (512,128), (128,512)}, M >= 8192): a streaming kernel that reads
 * every operand byte once (csrc/wgrad1x1.hip; replaces cuDNN's bwd-filter behind the 1x1 nn.Conv2d of models/resnet.py:148-175).
 * Returns 1 when launched, 0 outside the envelope (use dle_gemm with split-K); workspace >= dle_wgrad1x1_workspace() bytes.
 * dle_wgrad1x1_mode(0 / 1): off / on for A/B measurements. */
int64_t dle_wgrad1x1_workspace(void);
int dle_wgrad1x1_mode(int mode);
/* workspace of one shape in bytes; 0: (M, Ko, C) is outside the envelope of dle_wgrad1x1_try (do not allocate, do not call) */
int64_t dle_wgrad1x1_workspace_for(int M, int Ko, int C);
int dle_wgrad1x1_try(const void* dy, const void* x, float* dw, int M, int Ko, int C, int dtype, int accumulate, void* workspace,
                     int64_t workspace_bytes, hipStream_t stream);
/* 3x3 / stride 1 / pad 1 weight gradients with C, Ko multiples of 64 run on the halo-tile kernel of csrc/conv3x3_wgrad.hip when the
 * workspace holds dle_conv3x3_wgrad_workspace() bytes (256 partial blocks of 64 x 9 x 64 fp32, folded in a fixed order);
 * dle_conv3x3_wgrad_mode(0 / 1) switches it off / on for A/B measurements (returns the previous value). */
int64_t dle_conv3x3_wgrad_workspace(void);
int dle_conv3x3_wgrad_mode(int mode);

/* out[n] (+)= sum_m x[m][n]  (bias gradients).  workspace (optional, fp32, >= 2048*N*4 bytes is always
 * enough): row groups are combined through it instead of through same-address atomics. */
int dle_colsum(const void* x, float* out, int64_t M, int N, int64_t ld, int dtype, int accumulate,
               void* workspace, int64_t workspace_bytes, hipStream_t stream);
/* The same sums for n same-shaped 16-bit matrices in one launch pair (the bias gradients of a stack of layers whose output
 * gradients are kept until the end of backward: WaveGlow's 96 res_skip layers, waveglow/model.py:138-157).  table_dev: n x
 * { int64 address of the [M, N] matrix (row pitch ld), int64 address of its fp32 [N] destination } in device memory;
 * workspace >= dle_colsum_batched_workspace_bytes(n, M, N). */
int64_t dle_colsum_batched_workspace_bytes(int n, int64_t M, int N);
int dle_colsum_batched(const int64_t* table_dev, int n, int64_t M, int N, int64_t ld, int dtype, void* workspace,
                       int64_t workspace_bytes, hipStream_t stream);

/* ---- multi-tensor optimizer kernels -----------------------------------------------------------
 * replaces fused_lamb_CUDA.multi_tensor_l2norm / multi_tensor_lamb
 *   LanguageModeling/BERT/lamb_amp_opt/csrc/frontend.cpp:3-32
 *   .../csrc/multi_tensor_l2norm_kernel.cu:153-216, .../csrc/multi_tensor_lamb.cu:371-500
 * and the dense SGD steps (apex FusedSGD, Recommendation/DLRM/dlrm/scripts/main.py:468-471;
 * torch.optim.SGD, Classification/ConvNets/image_classification/optimizers.py:34-56).
 * Tensor lists are described by a device-resident int64 table:
 *   { size[n] | chunk_start[n+1] | ptr[list 0][n] | ptr[list 1][n] | ... }
 * built on the host with dle_mt_table_fill and copied to the device once per address set.
 * The table rule, checked by every dle_mt_* entry point below and by dle_mt_adam / dle_mt_adam_copy / dle_mt_ema before anything
 * is launched (-1, message in dle_last_error()): chunk > 0 and chunk % 4 == 0; 0 <= total_chunks <= INT_MAX, total_chunks being
 * chunk_start[n] of a table filled with the same chunk.  Zero-length tensors are legal (chunk_start[t] == chunk_start[t + 1]);
 * n_tensors == 0 or total_chunks == 0 launches nothing, and the norm outputs of such a call are zeros.                        */
int64_t dle_mt_table_len(int n_tensors, int n_lists);
int64_t dle_mt_table_fill(int64_t* table_host, int n_tensors, int n_lists, const int64_t* sizes,
                          const void* const* ptrs, int chunk);
int dle_mt_l2norm(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, int dtype,
                  float* partial_scratch, float* ret, float* ret_per_tensor, int per_tensor,
                  int* noop_flag, hipStream_t stream);
/* lists: g (grad_dtype; overwritten with the update), p, m, v (fp32) */
int dle_mt_lamb_stage1(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk,
                       int grad_dtype, const int* noop_flag, float beta1, float beta2, float beta3,
                       const int* step_dev, int bias_correction, float eps, int mode,
                       float weight_decay, const float* global_grad_norm, const float* max_grad_norm,
                       const float* inv_scale, hipStream_t stream);
/* lists: update (grad_dtype), p (fp32) [, model copy (copy_dtype; -1 = no copy list)] */
/* Stage 1 that also leaves the two per-tensor norms multi_tensor_lamb_cuda takes in l2norm sweeps around it
 * (lamb_amp_opt/csrc/multi_tensor_lamb.cu:380-420: ||p_t|| before the step, ||update_t|| after stage 1): per-chunk partial sums
 * leave with the pass (partial: fp32 scratch, >= 2 * total_chunks), a fold writes param_norm / update_norm (fp32 [n_tensors]) and
 * raises noop_flag on a non-finite sum -- two sweeps over 1.34 GB each less per BERT-Large step.  weight_decay != 0 (without decay
 * and NVLAMB stage 2 ignores the norms).  The update, m and v are bit-identical to dle_mt_lamb_stage1. */
int dle_mt_lamb_stage1_norms(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, int grad_dtype,
                             int* noop_flag, float beta1, float beta2, float beta3, const int* step_dev, int bias_correction,
                             float eps, int mode, float weight_decay, const float* global_grad_norm, const float* max_grad_norm,
                             const float* inv_scale, float* partial, float* param_norm, float* update_norm, hipStream_t stream);
int dle_mt_lamb_stage2(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk,
                       int grad_dtype, int copy_dtype, const int* noop_flag,
                       const float* param_norm, const float* update_norm, const float* lr_dev,
                       float weight_decay, int use_nvlamb, hipStream_t stream);
/* lists: g (grad_dtype), p (fp32) [, momentum buffer (fp32)] [, low-precision model copy (copy_dtype)];
 * copy_dtype = -1: no copy list.  The copy is the 16-bit working weight the next forward reads, written
 * in the same pass (replaces autocast's per-forward weight cast). */
int dle_mt_sgd(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, int grad_dtype,
               int has_momentum, const float* skip_flag_dev, const float* lr_dev, float lr_host,
               float momentum, float dampening, float weight_decay, int nesterov, int first_step,
               const float* inv_scale_dev, int copy_dtype, hipStream_t stream);

/* ---- small train-step kernels (csrc/elementwise.hip) -------------------------------------------
 * dle_cast_rows: out[r, c] = (out_dtype) in[r, c] for c < cols, 0 for cols <= c < cols_out; replaces
 *   autocast's activation/weight casts (Recommendation/DLRM/dlrm/scripts/main.py:588).
 * dle_bce_logits: torch.nn.BCEWithLogitsLoss(reduction="mean") forward + backward in one pass
 *   (main.py:556,589-592): loss_out[0] = mean loss (fp32), dlogits[i] = (sigmoid(x_i) - y_i) * (*grad_scale)/n
 *   in the logits' dtype (dlogits may be NULL); logits element i at logits[i*ld_logits].
 * dle_amp_update_scale: GradScaler.update() = torch._amp_update_scale_ on device scalars (main.py:497,608).
 * dle_check_nonfinite: found_inf = 1 if any element is inf/nan (GradScaler.unscale_'s check).        */
int dle_cast_rows(const void* in, void* out, int64_t rows, int cols, int cols_out, int64_t ld_in,
                  int64_t ld_out, int in_dtype, int out_dtype, hipStream_t stream);
/* y[c][r] = (16-bit) x[r][c]: transposed 16-bit working copy of a weight matrix (fp32 master or 16-bit copy), made once per
 * iteration for the products that contract over the OUTPUT dimension with k-contiguous operands (data gradients of the
 * recurrent cells, model.py:405-455 backward); torch.nn.LSTMCell's backward reads weight.t() the same way. */
int dle_transpose_cast(const void* x, void* y, int rows, int cols, int64_t ld_x, int64_t ld_y, int in_dtype, int out_dtype,
                       hipStream_t stream);
/* Exchange buffer <-> interaction input of the DLRM bottom -> top all-to-all (dlrm/model/distributed.py:32-98: torch.cat(dim=1) of
 * the received blocks forward, the split of the gradient backward).  blocks = concatenation over ranks s of contiguous
 * [rows, widths[s]] matrices; x = [rows, sum widths]; pack = 0: x <- blocks, 1: blocks <- x.  widths in elements (host array of
 * `world` <= 8 ints), widths[s] * elem_size a multiple of 16. */
int dle_a2a_blocks(void* blocks, void* x, int rows, int world, const int* widths, int elem_size, int pack, hipStream_t stream);
int dle_bce_logits(const void* logits, const float* target, float* loss_out, void* dlogits,
                   const float* grad_scale_dev, int64_t n, int64_t ld_logits, int dtype, hipStream_t stream);
/* Data gradient of a linear layer through the activation derivative of the layer below + that layer's bias gradient in one launch
 * (csrc/gemm_dma.hip): C[M, N] = f(A[M, K] B[K, N], src[M, N]) (16-bit, pitch ldc for C and src), colsum_out[n] (+)= sum_m C[m, n]
 * of the rounded output (fp32).  act = DLE_ACT_RELU_BWD: C = product where src > 0 else 0 (dlrm/nn/mlps.py:38-43 backward, apex.mlp);
 * DLE_ACT_MUL: C = product * src, src = the stored GELU derivative (BERT/modeling.py:130-160, bias_gelu backward).  One partial row
 * per tile row in `workspace` (>= ceil(M / 128) * N * 4 bytes), folded in a fixed order.  A k-contiguous, B n-contiguous.
 * 1: launched; 0: outside the envelope (run dle_gemm + dle_colsum). */
int dle_gemm_colsum(const void* A, const void* B, void* C, const void* src, float* colsum_out, int M, int N, int K, int64_t lda,
                    int64_t ldb, int64_t ldc, int dtype, int act, int accumulate_colsum, void* workspace,
                    int64_t workspace_bytes, hipStream_t stream);
/* The head of the DLRM top model in one pass (csrc/dlrm_head.hip): the last linear layer (out_features = 1,
 * dlrm/model/distributed.py top MLP, dlrm/nn/mlps.py:38-43), BCEWithLogitsLoss(mean) (scripts/main.py:556,589-592) and the
 * backward of both -- replaces dle_gemm (batch x 1 x K) + dle_bce_logits + dle_gemm (batch x K x 1, ReLU mask) + dle_gemm
 * (1 x K x batch) + dle_colsum x 2 with the same 16-bit rounding points:
 *   z = (16-bit) (h w + bias); loss_out[0] = mean BCE(z, target); dz = (16-bit) ((sigmoid(z) - target) * (*grad_scale) / M);
 *   dh[m, k] = h[m, k] > 0 ? (16-bit) (dz[m] w[k]) : 0; gw[k] = sum_m dz[m] h[m, k]; gb = sum_m dz[m];
 *   gprev_bias[k] (optional) = sum_m dh[m, k]  (bias gradient of the layer that produced h); logits_out (optional) = z.
 * K % 8 == 0, K <= 512; ws: dle_head_bce_workspace_bytes(M, K) bytes of scratch (one partial row per workgroup, folded in a
 * fixed order by a second small launch: bit-reproducible). */
int64_t dle_head_bce_workspace_bytes(int64_t M, int K);
int dle_head_bce_fwd_bwd(const void* h, const void* w16, const float* bias, const float* target,
                         const float* grad_scale_dev, float* loss_out, void* logits_out, void* dh, float* gw, float* gb,
                         float* gprev_bias, void* ws, int64_t ws_bytes, int64_t M, int K, int64_t ldh, int64_t ldd,
                         int dtype, hipStream_t stream);
int dle_amp_update_scale(float* scale, int* growth_tracker, float* found_inf, float* inv_scale,
                         float growth_factor, float backoff_factor, int growth_interval,
                         int clear_found_inf, hipStream_t stream);
int dle_check_nonfinite(const void* x, float* found_inf, int64_t n, int dtype, hipStream_t stream);
/* out = a * x + b * y on flat fp32 arrays (16-byte aligned; out may alias x or y; y is not read when b == 0): the
 * accumulation of micro-batch gradients behind --optimizer-batch-size (Classification/ConvNets/main.py:405-416,
 * image_classification/training.py:86-96,167-186: loss / divide_loss, autograd's += into .grad; apex amp_C.multi_tensor_axpby). */
int dle_axpby_f32(const float* x, const float* y, float* out, float a, float b, int64_t n, hipStream_t stream);
/* out = g * act'(src) on flat 16-bit arrays; act = DLE_ACT_GELU_BWD (src = pre-activation) or DLE_ACT_TANH_BWD */
int dle_act_bwd(const void* g, const void* src, void* out, int64_t n, int act, int dtype, hipStream_t stream);
/* out[r,c] = y[r,c] > 0 ? g[r,c] : 0 on 16-bit strided views (nn.ReLU backward, dlrm/nn/mlps.py:85-87) */
int dle_relu_bwd(const void* g, const void* y, void* out, int64_t rows, int cols, int64_t ld_g, int64_t ld_y,
                 int64_t ld_out, int dtype, hipStream_t stream);

/* ---- ResNet-50 HBM-bound kernels (csrc/convnet.hip), NHWC 16-bit activations, fp32 statistics ----------------
 * replace nn.BatchNorm2d(train) + nn.ReLU + residual add, nn.MaxPool2d(3,2,1), nn.AdaptiveAvgPool2d(1)
 *   Classification/ConvNets/image_classification/models/resnet.py:148-175,270,299, models/common.py:107-128
 * and LabelSmoothing / CrossEntropyLoss (smoothing.py:18-40, main.py:453-457; ignore_index as used by
 * LanguageModeling/BERT/run_pretraining.py:75-95).  M = N*H*W rows of C channels (C % 8 == 0).
 * BN workspace: fp32 scratch of dle_bn_workspace_bytes(M, C).                                              */
int dle_nchw_to_nhwc(const float* x, void* y, int64_t N, int C, int64_t HW, int C_padded, int out_dtype,
                     hipStream_t stream);
int64_t dle_bn_workspace_bytes(int64_t M, int C);
/* mean/rstd (biased var, eps) of x over M; running stats updated with `momentum` (unbiased var) when non-NULL */
int dle_bn_fwd_stats(const void* x, int64_t M, int C, float eps, float momentum, float* mean, float* rstd,
                     float* running_mean, float* running_var, void* workspace, int64_t workspace_bytes,
                     int dtype, hipStream_t stream);
/* Batch statistics without re-reading the activation: dle_conv2d_fwd_colstats is dle_conv2d_fwd (no bias / act) whose
 * epilogue also leaves column sums of the rounded output in col_partial[groups][2][Ko]: one row per 128-row tile, or -- the
 * channel-widening 1x1 convolutions on the streaming kernel (csrc/gemm_expand.hip), chosen when the buffer also holds
 * min(1032, ceil(M / 64) + 8) rows -- one row per workgroup group; the buffer holds >= ceil(N*P*Q / 128) * 2 * Ko floats and
 * *groups receives the number of rows written; dle_bn_stats_from_partials folds them (fixed order, deterministic) into
 * mean / rstd / running stats exactly like dle_bn_fwd_stats.  workspace: >= 64*C floats. */
int dle_conv2d_fwd_colstats(const void* x, const void* w, void* y, int N, int H, int W, int C, int Ko, int R, int S,
                            int stride, int pad, int dtype, float* col_partial, int64_t col_partial_bytes,
                            int* groups, hipStream_t stream);
int dle_bn_stats_from_partials(const float* partial, int groups, int64_t M, int C, float eps, float momentum,
                               float* mean, float* rstd, float* running_mean, float* running_var, void* workspace,
                               int64_t workspace_bytes, hipStream_t stream);
/* y = act((x - mean) * rstd * gamma + beta (+ residual)), act = ReLU when relu != 0.
 * relu_mask (optional, M*C/8 bytes): bit k of byte i = (y[8 i + k] > 0) -- the backward pass then reads 1 bit per
 * element instead of the 2-byte output to rebuild the ReLU mask.                                                */
int dle_bn_fwd_apply(const void* x, const void* residual, void* y, void* relu_mask, const float* mean,
                     const float* rstd, const float* gamma, const float* beta, int64_t M, int C, int relu,
                     int dtype, hipStream_t stream);
/* y = relu(bn(x) + round16(bn_r(xr))) + keep bits: the bn3 apply of a bottleneck whose residual comes from the downsample branch
 * (conv -> BatchNorm, no ReLU: models/resnet.py:166-173, `residual = self.downsample(x)`) with that branch's BatchNorm taken on
 * the residual's load -- its 16-bit output is never written.  Bit-identical to dle_bn_fwd_apply(xr -> res, relu = 0) followed by
 * dle_bn_fwd_apply(x, res, relu = 1).  mean_r / rstd_r / gamma_r / beta_r: the branch's BatchNorm, fp32 [C].                  */
int dle_bn_fwd_apply2(const void* x, const void* xr, void* y, void* relu_mask, const float* mean, const float* rstd,
                      const float* gamma, const float* beta, const float* mean_r, const float* rstd_r, const float* gamma_r,
                      const float* beta_r, int64_t M, int C, int dtype, hipStream_t stream);
/* g = dy * relu'(y): from relu_mask when given, else from y > 0 (both NULL: g = dy);
 * dgamma = sum g*xhat, dbeta = sum g */
int dle_bn_bwd_reduce(const void* dy, const void* y, const void* relu_mask, const void* x, const float* mean,
                      const float* rstd, float* dgamma, float* dbeta, int64_t M, int C, int accumulate,
                      void* workspace, int64_t workspace_bytes, int dtype, hipStream_t stream);
/* The same reduction for TWO BatchNorms that receive the same gradient (bn3 and the downsample branch's BatchNorm of a
 * bottleneck's first block, models/resnet.py:166-173: both see dy under the block's output keep bits): dy and relu_mask are read
 * ONCE.  Bit-identical to two dle_bn_bwd_reduce calls.  workspace >= 2 * dle_bn_workspace_bytes(M, C). */
int dle_bn_bwd_reduce2(const void* dy, const void* relu_mask, const void* x1, const float* mean1, const float* rstd1, float* dgamma1,
                       float* dbeta1, const void* x2, const float* mean2, const float* rstd2, float* dgamma2, float* dbeta2,
                       int64_t M, int C, void* workspace, int64_t workspace_bytes, int dtype, hipStream_t stream);
/* dx = gamma*rstd*(g - dbeta/M - xhat*dgamma/M); g_out (optional) = g, the skip-branch gradient */
int dle_bn_bwd_apply(const void* dy, const void* y, const void* relu_mask, const void* x, void* dx, void* g_out,
                     const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                     const float* dbeta, int64_t M, int C, int dtype, hipStream_t stream);
/* ---- conv + BatchNorm + ReLU as ONE unit (csrc/conv_bnload.hip): the PRODUCER unit's BatchNorm-apply (+ residual) + ReLU runs on
 * the operand load of the CONSUMER 1x1 convolution (models/resnet.py:148-175: relu(bn2(.)) -> conv3, relu(bn3(.) + residual) ->
 * the next block's conv1; models/common.py:31-128).  out [M, N] = relu(t * sc + sh (+ res)) W^T with sc = rstd * gamma,
 * sh = beta - mean * sc; side outputs y [M, K] (16-bit), bits [M*K/8] (bit k of byte i = y[8 i + k] > 0) and, when stats != NULL,
 * the column sums / sums of squares of the rounded out ([dle_conv1x1_bnload_groups(M, N, K)][2][N], fold with
 * dle_bn_stats_from_partials).  Bit-identical to dle_bn_fwd_apply followed by dle_conv2d_fwd_colstats.  Returns 1 when launched,
 * 0 when the shape is outside the envelope (K in {64, 128, 256}, N % 64 == 0, M >= 4096), > 1 on error.                      */
int dle_conv1x1_bnload_groups(int M, int N, int K);
int dle_conv1x1_bnload_fwd(const void* t, const void* res, const void* w, void* out, void* y, void* bits, const float* mean,
                           const float* rstd, const float* gamma, const float* beta, float* stats, int64_t stats_bytes, int M,
                           int N, int K, int dtype, hipStream_t stream);
/* The same with the residual taken through its own BatchNorm on load (the downsample branch, as dle_bn_fwd_apply2):
 * y = relu(bn(t) + round16(bn_r(res))); bit-identical to dle_bn_fwd_apply(res) followed by dle_conv1x1_bnload_fwd.            */
int dle_conv1x1_bnload_fwd2(const void* t, const void* res, const void* w, void* out, void* y, void* bits, const float* mean,
                            const float* rstd, const float* gamma, const float* beta, const float* mean_r, const float* rstd_r,
                            const float* gamma_r, const float* beta_r, float* stats, int64_t stats_bytes, int M, int N, int K,
                            int dtype, hipStream_t stream);
/* The backward counterpart (csrc/conv_bnbwd.hip): BatchNorm backward (second pass) on the operand load of the 1x1 data gradient
 * that consumes it -- the conv3 / bn3 unit of a bottleneck (models/resnet.py:148-175 backward).  dt [M, K] = ka (g - dbeta / M -
 * xhat dgamma / M) with g = dy under relu_mask (bit-packed, may be NULL), dx [M, N] = dt W, W [K][N] n-contiguous; dgamma / dbeta
 * = the sums dle_bn_bwd_reduce left.  dt and dx are bit-identical to dle_bn_bwd_apply + dle_gemm; dt is never re-read.
 * t2 / bits2 / mean2 / rstd2 / partial (all or none, NULL: off): dx is itself the gradient that enters a second BatchNorm (bn2 of the
 * bottleneck, ReLU keep bits bits2); partial [dle_conv1x1_bnbwd_groups(M)][2][N] receives its backward reduction (sum g, sum g xhat
 * per workgroup; fold with dle_bn_bwd_finish), as dle_gemm_expand_masked_bnred does for bn3.
 * 1: launched; 0: outside the envelope (K = 256, N = 64, M >= 4096, 16-byte aligned dense operands). */
int dle_conv1x1_bnbwd_dgrad(const void* dy, const void* t, const void* relu_mask, const void* w, void* dt, void* dx,
                            const float* mean, const float* rstd, const float* gamma, const float* dgamma, const float* dbeta,
                            const void* t2, const void* bits2, const float* mean2, const float* rstd2, float* partial,
                            int64_t partial_bytes, int M, int N, int K, int dtype, hipStream_t stream);
int dle_conv1x1_bnbwd_groups(int M);
/* The same launch WITH conv3's weight gradient and without dt: gw [K][N] (fp32, written) = dt^T x, x [M, N] the unit's saved input.
 * The kernel that holds the rounded 16-bit dt in registers forms the product itself (dt and x rows through LDS, one fp32 [K][N]
 * partial per workgroup in `workspace`, folded in workgroup order: deterministic, no atomics), so dt is never written or read
 * back.  dx and `partial` are bit-identical to dle_conv1x1_bnbwd_dgrad, gw to dle_wgrad1x1_try on the dt that call writes (the
 * same MFMA steps over the same tiles in the same order; bn2's per-tile values leave unsummed and a small launch adds them in
 * the plain form's order).  workspace >= dle_conv1x1_bnbwd_wgrad_workspace(M, t2 != NULL) bytes, 16-byte aligned; with t2,
 * partial holds dle_conv1x1_bnbwd_groups(M) rows.  1: launched; 0: outside the envelope (as above) or workspace too small. */
int dle_conv1x1_bnbwd_dgrad_wgrad(const void* dy, const void* t, const void* relu_mask, const void* w, void* dx,
                                  const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                                  const float* dbeta, const void* t2, const void* bits2, const float* mean2, const float* rstd2,
                                  float* partial, int64_t partial_bytes, const void* x, float* gw, void* workspace,
                                  int64_t workspace_bytes, int M, int N, int K, int dtype, hipStream_t stream);
int64_t dle_conv1x1_bnbwd_wgrad_workspace(int M, int bnred);
/* The backward reduction of a BatchNorm taken where its input gradient is PRODUCED (csrc/gemm_expand.hip, BRED): conv1's data
 * gradient of the next bottleneck, C = A B^T + src under `bits` (the DLE_ACT_ADD_MASKED form of dle_gemm), is the gradient of the
 * previous block's output; with g = C under bits2 and xhat = (t2 - mean2) rstd2 the kernel also leaves partial [groups][2][N] rows
 * of (sum g, sum g xhat) -- groups = dle_gemm_expand_groups(M, N, K) -- which dle_bn_bwd_finish folds into dgamma / dbeta (what
 * dle_bn_bwd_reduce computes from dy + t + mask in a pass of its own).  t2 [M, N] with C's pitch; bits2 indexed like bits.
 * 1: launched; 0: outside the envelope (K in {64, 128}, N >= 2 K, N % 128 == 0, M >= 4096, 16-byte aligned operands). */
int dle_gemm_expand_masked_bnred(const void* A, const void* B, void* C, const void* src, const void* bits, const void* t2,
                                 const void* bits2, const float* mean2, const float* rstd2, float* partial, int64_t partial_bytes,
                                 int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int b_kc, int dtype, hipStream_t stream);
int dle_bn_bwd_finish(const float* partial, int groups, int C, float* dgamma, float* dbeta, int accumulate, hipStream_t stream);
/* ---- the ResNet stem (csrc/stem.hip): conv7x7 / stride 2 / pad 3 of a 3-channel image, forward (+ BatchNorm partial sums) and
 * weight gradient, on a 4-channel NHWC image (dle_nchw_to_nhwc with C_padded = 4: 8 bytes per pixel, channel 3 zero).
 *   replaces cuDNN behind builder.conv7x7(3, 64, stride=2) + bn1's statistics: Classification/ConvNets/image_classification/
 *   models/resnet.py:262-268,318-322, models/common.py:31-60.
 * w2: packed 16-bit weights [64][7][8][4] (k = r*32 + s*4 + c, zero for s = 7 / c = 3) written by dle_stem_pack_weight from the
 * fp32 master in KRSC memory order [64][7][7][3] (a channels_last nn.Conv2d.weight).  Images up to 224 pixels wide.
 * fwd: y [N, P, Q, 64]; stats (optional): [dle_stem_conv7_groups(N, H)][2][64] column sums / sums of squares of the ROUNDED output
 *      (contract of dle_conv2d_fwd_colstats; fold with dle_bn_stats_from_partials).
 * wgrad: dw [64][7][7][3] fp32 in the master's memory order (+)= sum over pixels dy x im2col(x); workspace >=
 *      dle_stem_conv7_wgrad_workspace(N, H) bytes (one partial per persistent workgroup, folded in a fixed order).      */
int dle_stem_conv7_groups(int N, int H);
int dle_stem_conv7_fwd(const void* x4, const void* w2, void* y, float* stats, int64_t stats_bytes, int N, int H, int W,
                       int dtype, hipStream_t stream);
int64_t dle_stem_conv7_wgrad_workspace(int N, int H);
int dle_stem_conv7_wgrad(const void* dy, const void* x4, float* dw, void* workspace, int64_t workspace_bytes, int N, int H,
                         int W, int dtype, int accumulate, hipStream_t stream);
int dle_stem_pack_weight(const float* w_krsc, void* out, int dtype, hipStream_t stream);
/* argmax: uint8 [N,P,Q,C] window-scan index of the first maximum (ATen tie rule) */
int dle_maxpool_fwd(const void* x, void* y, void* argmax, int N, int H, int W, int C, int ksize, int stride,
                    int pad, int dtype, hipStream_t stream);
/* BatchNorm-apply + ReLU + MaxPool2d(3, 2, 1) in one pass (the stem: models/resnet.py:318-322 bn1 -> relu -> maxpool): y
 * [N, H/2, W/2, C], argmax and relu_mask exactly as dle_bn_fwd_apply + dle_maxpool_fwd would leave them (bit-identical); the
 * 16-bit activation between the two never exists.  H, W even. */
int dle_bn_relu_maxpool_fwd(const void* x, void* y, void* argmax, void* relu_mask, const float* mean, const float* rstd,
                            const float* gamma, const float* beta, int N, int H, int W, int C, int dtype, hipStream_t stream);
int dle_maxpool_bwd(const void* dy, const void* argmax, void* dx, int N, int H, int W, int C, int ksize,
                    int stride, int pad, int dtype, hipStream_t stream);
/* The stem's backward chain MaxPool2d(3, 2, 1) -> ReLU -> BatchNorm (models/resnet.py:318-322 backward; cuDNN pooling backward +
 * batch_norm_backward in the reference) without the pooling gradient's full-resolution tensor: dz [N, H, W, C] = BatchNorm backward
 * (keep bits relu_mask [N H W C / 8], x = the BatchNorm's input) of the gradient dle_maxpool_bwd would scatter from dy
 * [N, H/2, W/2, C] + argmax; dgamma / dbeta (fp32 [C]) are written.  dz equals dle_maxpool_bwd + dle_bn_bwd_apply bit for bit
 * given the same dgamma / dbeta; the reduction groups its fp32 partial sums differently.  workspace: fp32,
 * >= dle_pool_bn_bwd_workspace_bytes (0 = shape outside the envelope: H, W even, C / 8 a power of two <= 256). */
int64_t dle_pool_bn_bwd_workspace_bytes(int N, int H, int W, int C);
int dle_pool_bn_bwd(const void* dy, const void* argmax, const void* relu_mask, const void* x, void* dz, const float* mean,
                    const float* rstd, const float* gamma, float* dgamma, float* dbeta, int N, int H, int W, int C, void* workspace,
                    int64_t workspace_bytes, int dtype, hipStream_t stream);
int dle_avgpool_fwd(const void* x, void* y, int64_t N, int HW, int C, int dtype, hipStream_t stream);
int dle_avgpool_bwd(const void* dy, void* dx, int64_t N, int HW, int C, int dtype, hipStream_t stream);
/* C [M = n_img*H*W, N] = A [M, K] B^T + zero_stuffed(compact [n_img*(H/2)*(W/2), N]): the data gradient of a bottleneck's first 1x1
 * convolution plus the gradient of the stride-2 1x1 downsample branch (models/resnet.py:148-175,150-158), whose full-resolution
 * zero-stuffed form is never written (csrc/gemm_expand.hip).  Returns 1 when launched, 0 when the shape is outside the streaming
 * kernel's envelope (K in {64, 128, 256}, N % 128 == 0, N >= 2 K, H and W even): the caller then materialises dle_upsample_zero
 * and uses dle_gemm with DLE_ACT_ADD. */
int dle_gemm_expand_add_up2(const void* A, const void* B, void* C, const void* compact, int M, int N, int K, int64_t lda,
                            int64_t ldb, int64_t ldc, int64_t ld_compact, int b_kc, int H, int W, int dtype, hipStream_t stream);
/* y[n,h,w,:] = x[n,h/s,w/s,:] where h, w are multiples of s, else 0: with a plain GEMM on the P x Q grid this is the
 * data gradient of a 1x1 stride-s convolution (ResNet downsample branches, models/resnet.py:150-158)           */
int dle_upsample_zero(const void* x, void* y, int64_t N, int P, int Q, int H, int W, int C, int stride, int dtype,
                      hipStream_t stream);
/* loss_out[0] = mean over rows with target != ignore_index of (1-s)*nll + s*(lse - mean logits);
 * dlogits (optional, dlogits_dtype, row stride ld_out) = d loss / d logits * (*grad_scale_dev).
 * scratch: one int32 device word.                                                                           */
int dle_softmax_xent(const float* logits, const int64_t* target, float* loss_out, void* dlogits,
                     const float* grad_scale_dev, int* scratch, int64_t rows, int classes, int64_t ld,
                     int64_t ld_out, float smoothing, int64_t ignore_index, int dlogits_dtype,
                     hipStream_t stream);

/* ---- BERT HBM-bound kernels (csrc/transformer.hip): hidden states [tokens, H] 16-bit, statistics fp32 --------
 * replace LayerNorm(dense(x) + residual) (LanguageModeling/BERT/modeling.py:394-398,430-434), BertEmbeddings
 * (modeling.py:285-301), scores/sqrt(d) + mask -> softmax (modeling.py:354-366), the masked-row index_select of
 * the dense MLM head (modeling.py:587-595) and the pooler's token-0 slice (modeling.py:518-524).               */
int dle_layernorm_fwd(const void* x, const void* residual, void* z_out, void* y, const float* gamma,
                      const float* beta, float* mean, float* rstd, int64_t rows, int H, float eps, int dtype,
                      hipStream_t stream);
int64_t dle_layernorm_workspace_bytes(int H);
/* dz = d/dz of LN; dgamma/dbeta (fp32, (+)= when accumulate) */
int dle_layernorm_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                      void* dz, float* dgamma, float* dbeta, int64_t rows, int H, int accumulate, void* workspace,
                      int64_t workspace_bytes, int dtype, hipStream_t stream);
/* z[t] = word[ids[t]] + pos[t mod S] + type[token_type[t]]  (fp32 tables -> 16-bit) */
int dle_embed_sum(const float* word, const float* pos, const float* type, const int64_t* ids,
                  const int64_t* token_type, void* z, int64_t tokens, int S, int H, int dtype, hipStream_t stream);
/* The same with the position row given per token, z[t] = word[ids[t]] + pos[position_ids[t]] + type[token_type[t]]: the
 * embedding sum of a PACKED batch (sequences back to back, no padding rows), where row t is not at position t mod S.  Same
 * arithmetic and rounding as dle_embed_sum.  position_ids: int32 [tokens]. */
int dle_embed_sum_packed(const float* word, const float* pos, const float* type, const int64_t* ids,
                         const int64_t* token_type, const int32_t* position_ids, void* z, int64_t tokens, int H, int dtype,
                         hipStream_t stream);
/* grad_word[ids[t], :] += dz[t, :] (fp32) */
int dle_embed_scatter_add(const void* dz, const int64_t* ids, float* grad_word, int64_t tokens, int H, int dtype,
                          hipStream_t stream);
/* out[k, :] (+)= sum of rows t with sel[t] == k, k < K <= 4; workspace >= 128*K*H*4 bytes */
int dle_rows_select_sum(const void* x, const int64_t* sel, float* out, int64_t rows, int H, int K, int accumulate,
                        void* workspace, int64_t workspace_bytes, int dtype, hipStream_t stream);
int dle_rows_gather(const void* src, const int64_t* idx, void* dst, int64_t n, int H, int dtype, hipStream_t stream);
int dle_rows_scatter(const void* src, const int64_t* idx, void* dst, int64_t n, int H, int accumulate, int dtype,
                     hipStream_t stream);
/* in place: p = softmax(s * scale + mask_add[row / rows_per_batch][col]); rows of length L (power of two <= 512) */
int dle_softmax_fwd(void* scores, const float* mask_add, int64_t rows, int L, int rows_per_batch, float scale,
                    int dtype, hipStream_t stream);
/* in place over dprobs: dS = P * (dP - sum(dP * P)) * scale */
int dle_softmax_bwd(const void* probs, void* dprobs, int64_t rows, int L, float scale, int dtype,
                    hipStream_t stream);

/* ---- dropout (training-mode nn.Dropout of the BERT path: modeling.py:276,296 embeddings; :320,369 attention
 * probabilities; :392-396, :428-432 BertSelfOutput / BertOutput before the residual LayerNorm).
 * Counter-based Philox4x32-10: key = seed, counter = (8-element chunk index, offset); the caller advances `offset`
 * per call site and per step.  Masks are bit-packed (bit k of byte i <-> element 8 i + k, 1 = kept), n / 8 bytes;
 * the drop probability is quantised to round(p * 65536) / 65536 and kept values are scaled by its complement.
 * The reference draws from torch's CUDA Philox stream, so masks are NOT bit-identical to the reference's; parity of
 * the step is checked against the oracle under the masks these entry points produce.                            */
/* backward of dle_dropout_add_layernorm_fwd in ONE pass: dz (residual branch), dx = dz * keep / (1 - p) (dense branch),
 * dgamma / dbeta, and dbias (+)= column sums of dx when non-NULL -- the dropout-backward pass and the dense layer's bias
 * gradient pass (autograd of modeling.py:394-398,430-434) folded into the LayerNorm backward. */
int dle_dropout_add_layernorm_bwd(const void* dy, const void* z, const float* mean, const float* rstd, const float* gamma,
                                  const void* keep_mask, float p, void* dz, void* dx, float* dgamma, float* dbeta,
                                  float* dbias, int64_t rows, int H, int accumulate, void* workspace,
                                  int64_t workspace_bytes, int dtype, hipStream_t stream);
int dle_dropout_fwd(const void* x, void* y, void* mask, int64_t n, float p, uint64_t seed, uint64_t offset,
                    const uint64_t* offset_base,
                    int dtype, hipStream_t stream);
int dle_dropout_bwd(const void* dy, const void* mask, void* dx, int64_t n, float p, int dtype, hipStream_t stream);
/* y = LayerNorm(dropout(x) + residual); z_out = dropout(x) + residual (16-bit, for the backward pass) */
int dle_dropout_add_layernorm_fwd(const void* x, const void* residual, void* z_out, void* y, void* mask,
                                  const float* gamma, const float* beta, float* mean, float* rstd, int64_t rows,
                                  int H, float eps, float p, uint64_t seed, uint64_t offset,
                                  const uint64_t* offset_base, int dtype,
                                  hipStream_t stream);
/* scores -> probs in place; dropped = dropout(probs) is the operand of the P V contraction */
int dle_softmax_dropout_fwd(void* scores, void* dropped, void* mask, const float* mask_add, int64_t rows, int L,
                            int rows_per_batch, float scale, float p, uint64_t seed, uint64_t offset,
                            const uint64_t* offset_base, int dtype,
                            hipStream_t stream);
/* in place over dprobs: g = dP * mask / (1 - p); dS = P * (g - sum(g * P)) * scale */
int dle_softmax_dropout_bwd(const void* probs, void* dprobs, const void* mask, int64_t rows, int L, float scale,
                            float p, int dtype, hipStream_t stream);

/* uint8 NCHW images -> (x - mean[c]) / std[c] as 16-bit NHWC (channels zero-padded to C_padded): the normalisation of
 * PrefetchedWrapper.prefetched_loader (Classification/ConvNets/image_classification/dataloaders.py:354-384) fused with the
 * layout change of the step's first kernel. */
int dle_u8_nchw_normalize_nhwc(const void* x, void* y, const float* mean, const float* std, int64_t N, int C, int64_t HW,
                               int C_padded, int out_dtype, hipStream_t stream);

/* 3x3 / stride 2 / pad 1 data gradient as four parity-class correlations (1 + 2 + 2 + 4 taps: no zero work), each written
 * into its strided sub-grid of dx -- cuDNN's bwd-data behind the strided 3x3 convolutions of the ResNet bottleneck
 * (Classification/ConvNets/image_classification/models/resnet.py:126,148-175).  H, W even; Ko % 64 == 0; workspace:
 * >= 9 * Ko * C * 2 bytes (tap-restricted weight matrices, rebuilt by every call). */
int dle_conv2d_dgrad_s2(const void* dy, const void* w, void* dx, int N, int H, int W, int C, int Ko, void* workspace,
                        int64_t workspace_bytes, int dtype, hipStream_t stream);

/* ---- fused self-attention (64-wide heads; S = 128, or a multiple of 128 up to 1024 -- phase 2 runs S = 512): replaces
 * BertSelfAttention.forward between the QKV and the output projection, LanguageModeling/BERT/modeling.py:340-384 (torch.bmm +
 * softmax + nn.Dropout + torch.bmm) and its autograd backward.  qkv [T = B*S, 3H] (q | k | v, head h at columns h*64 of each
 * third), ctx / dctx [T, H], dqkv [T, 3H]; mask_add fp32 [B, S] (0 / -10000) or NULL; stats fp32 [B*heads, S, W] with
 * W = dle_attention_stats_floats(S), 2 at S = 128 and 4 for S > 128 (never [B*heads, S, 2] there): words 0, 1 of a row are
 * (row max, 1 / row sum) saved for backward; for S > 128 word 2 is scratch of the backward pass (the row's delta) and word 3 is
 * unused; keep_mask (optional, B*heads*S*S/8 bytes) = the dropout keep bits in the layout of
 * dle_softmax_dropout_fwd.  The backward regenerates probabilities and mask from (qkv, stats, seed, offset): nothing of shape
 * [B, heads, S, S] is stored -- for S > 128 K / V are streamed through LDS in 128-key blocks (forward: online max / sum, then a
 * second pass with the final statistics; backward: a per-query-block kernel for delta and dQ, a per-key-block kernel for dK / dV).
 * colsum_partial (optional, fp32 [B * S / 128, 3H]): column sums of dqkv per (sequence, 128-row block) -- their sum over the rows
 * is the bias gradient of the QKV projection.  dle_attention_supported: 1 when (S, head_dim) is inside the kernels' envelope. */
int dle_attention_supported(int S, int head_dim);
int dle_attention_stats_floats(int S);
int dle_attention_fwd(const void* qkv, const float* mask_add, void* ctx, float* stats, void* keep_mask, int B, int S,
                      int heads, int head_dim, float scale, float p, uint64_t seed, uint64_t offset,
                      const uint64_t* offset_base, int dtype,
                      hipStream_t stream);
int dle_attention_bwd(const void* qkv, const void* dctx, const float* mask_add, const float* stats, void* dqkv,
                      float* colsum_partial, int B, int S, int heads, int head_dim, float scale, float p, uint64_t seed,
                      uint64_t offset, const uint64_t* offset_base, int dtype, hipStream_t stream);
/* The same with the keep mask the forward pass wrote (keep_mask of dle_attention_fwd) READ instead of re-drawn from the Philox
 * counters (S = 128: 16 bytes per query row replace 8 generator calls per lane); identical results.  keep_mask may be NULL. */
int dle_attention_bwd_keep(const void* qkv, const void* dctx, const float* mask_add, const float* stats, const void* keep_mask,
                           void* dqkv, float* colsum_partial, int B, int S, int heads, int head_dim, float scale, float p,
                           uint64_t seed, uint64_t offset, const uint64_t* offset_base, int dtype, hipStream_t stream);

/* ---- packed (variable-length) forward attention, inference only: BertSelfAttention.forward under model.eval()
 * (LanguageModeling/BERT/modeling.py:340-384) on the real rows of a batch that extract_features.py:262-294 pads to
 * [B, max_seq_length].  qkv [T, 3H] (column layout of dle_attention_fwd) holds the sequences back to back; sequence b owns rows
 * cu_seqlens[b] .. cu_seqlens[b + 1] - 1 (cu_seqlens: DEVICE int32 [B + 1], cu_seqlens[0] = 0, no sequence longer than
 * max_seqlen); ctx [T, H].  No dropout, no statistics output, no mask_add: the length is the mask, and a sequence's rows get
 * the bits dle_attention_fwd(p = 0) gives them in a padded batch under a 0 / -10000 mask.  One workgroup per (sequence, head,
 * 128-query block), keys streamed through LDS in 128-key blocks; max_seqlen need not be a multiple of 128.
 * Rows of the next sequence that a 128-row tile covers are read as zero (the buffer resource ends with the sequence), so a
 * sequence's result does not depend on its neighbours' values, Inf and NaN included.
 * Offsets into qkv are 32-bit and a tile reaches up to 127 rows past a sequence's last: (total_tokens + 127) * 3H * 2 >= 2^32
 * bytes is an error (-1, dle_last_error), as is anything outside
 * dle_attention_varlen_supported (1: head_dim == 64 and 1 <= max_seqlen <= 1024).  Lengths are clamped to [0, max_seqlen] and
 * rows to total_tokens inside the kernel: a wrong table gives wrong answers but reaches no memory outside qkv / ctx.
 * dle_attention_varlen_launch_count(): launches by this process so far (tests assert which path ran). */
int dle_attention_varlen_supported(int max_seqlen, int head_dim);
int dle_attention_fwd_varlen(const void* qkv, const int32_t* cu_seqlens, void* ctx, int B, int max_seqlen,
                             int64_t total_tokens, int heads, int head_dim, float scale, int dtype, hipStream_t stream);
uint64_t dle_attention_varlen_launch_count(void);

/* ---- torch.optim.Adam over a tensor table (csrc/multi_tensor.hip): GradScaler.unscale_ + clip_grad_norm_ + Adam.step of
 * SpeechSynthesis/Tacotron2/train.py:400-401,487-497 in one pass.  lists: g, p, exp_avg, exp_avg_sq (all fp32).
 * step_dev: int32 device word = the step number t of THIS update (the caller advances it when the step is not skipped);
 * grad_norm_dev: L2 norm of the (still scaled) gradients from dle_mt_l2norm, max_grad_norm <= 0 disables clipping. */
int dle_mt_adam(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, const float* skip_flag_dev,
                const float* lr_dev, float lr_host, float beta1, float beta2, float eps, float weight_decay,
                const int* step_dev, const float* inv_scale_dev, const float* grad_norm_dev, float max_grad_norm,
                hipStream_t stream);

/* ---- apex FusedAdam (bias_correction, weight_decay 0) with the 16-bit working-copy refresh (csrc/multi_tensor.hip): DLRM's
 * --Adam_MLP_optimizer (Recommendation/DLRM/dlrm/scripts/main.py:468-471).  lists: g, p, exp_avg, exp_avg_sq (fp32) and a 16-bit
 * copy of p (copy_dtype; pointer 0 where a tensor has none, copy_dtype -1: no copy list).  grad = g * inv_scale *
 * tensor_mul_dev[tensor] (fp32 [n_tensors] or NULL); step_dev: int32 device word = t of THIS update; skip_flag_dev != 0: the
 * step is skipped. */
int dle_mt_adam_copy(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, int copy_dtype,
                     const float* skip_flag_dev, const float* lr_dev, float lr_host, float beta1, float beta2, float eps,
                     const int* step_dev, const float* inv_scale_dev, const float* tensor_mul_dev, hipStream_t stream);

/* ---- exponential moving average of a model's state over a tensor table (csrc/multi_tensor.hip): EMA.__call__ of
 * Classification/ConvNets/image_classification/models/common.py:191-212, `ema.mul_(mu); ema.add_((1 - mu) * x)` on every
 * state_dict entry, run after each Trainer.train_step (training.py:148-152,183-184).  lists: x (source, fp32, read only),
 * e (shadow, fp32, in place).  e' = rn(rn(mu * e) + rn(one_minus_mu * x)): the three fp32 roundings of the two tensor ops, no
 * fused multiply-add -- bit-identical to them.  coef_dev: two fp32 device words {mu, 1 - mu} (the caller takes 1 - mu in double), or
 * NULL: the two host values are used.  No skip flag: the average also moves on steps the loss scaler skips. */
int dle_mt_ema(const int64_t* table_dev, int n_tensors, int64_t total_chunks, int chunk, const float* coef_dev, float mu_host,
               float one_minus_mu_host, hipStream_t stream);

/* ---- WaveGlow training step (csrc/waveglow.hip): SpeechSynthesis/Tacotron2/waveglow/model.py + loss_function.py -------
 * Channels-last: a series [B, C, T] of the reference is the matrix [B*T, C]; Conv1d = dle_gemm over rows.  The flow state
 * is fp32 [M, 8] (M = B*T/8 groups of n_group = 8 samples); a flow with c remaining channels works on columns [8-c, 8).
 * dle_wg_taps: row gather of a k-tap dilated Conv1d, col[b,t,k*C+ch] = x[b, t+(k-left)*dilation, ch] (0 outside [0,T); x rows ld_x apart);
 *   WN in_layers (model.py:112-118, left = 1) and ConvTranspose1d(1024, stride 256) (model.py:165-167; dilation -1, left 0).
 * dle_wg_taps_bwd: its transpose, dx[b,t,ch] = sum_k dcol[b, t-(k-left)*dilation, k*C+ch] (+ addend; dx may alias addend).
 * dle_wg_gate_fwd/bwd: fused_add_tanh_sigmoid_multiply (model.py:34-41) on the summed pre-activation s [M, 2nc] (row stride ld).
 * dle_wg_invconv_fwd/bwd: Invertible1x1Conv.forward (model.py:62-85) on the active channels, and its backward incl. the
 *   d/dW of the log-determinant term; dle_wg_logdet_inv: log|det W|, sign and W^-T of the c x c matrix (torch.logdet).
 * dle_wg_coupling_fwd/bwd: audio_1 = exp(log_s) * audio_1 + b (model.py:217-222); o fp32 [M, 8] = (b | log_s | 0).
 * dle_wg_loss / dle_wg_dz_init: WaveGlowLoss.forward (loss_function.py:30-48) and its gradient wrt z.
 * dle_wg_weight_norm_fwd/bwd: torch.nn.utils.weight_norm(dim 0) of Conv1d weights (model.py:95-136) -> 16-bit GEMM operand
 *   w16[co, tap*Cip + ci]; g NULL = plain weight.  dle_wg_upsample_weight(_bwd): ConvTranspose1d weight [Cm, Cm, ksize] <->
 *   GEMM operand b16[(r*Cm+co), (j*Cm+ci)] = w[ci, co, r + stride*j] and the bias repeated per phase r. */
int dle_wg_taps(const void* x, void* col, int B, int T, int C, int ntaps, int dilation, int left, int64_t ld_x, int dtype,
                hipStream_t stream);
int dle_wg_taps_bwd(const void* dcol, const void* addend, void* dx, int B, int T, int C, int ntaps, int dilation, int left,
                    int64_t ld_add, int64_t ld_dx, int dtype, hipStream_t stream);
int dle_wg_gate_fwd(const void* s, void* acts, int64_t M, int nc, int64_t ld_s, int dtype, hipStream_t stream);
int dle_wg_gate_bwd(const void* dacts, const void* s, void* ds, int64_t M, int nc, int64_t ld_s, int64_t ld_ds, int dtype,
                    hipStream_t stream);
int dle_wg_invconv_fwd(const float* x, const float* W, float* y, void* a0_16, int64_t M, int c, int dtype,
                       hipStream_t stream);
int dle_wg_invconv_bwd_partials(int64_t M);
int dle_wg_invconv_bwd(const float* dy, const float* da0, const float* x, const float* W, const float* WinvT, float* dx,
                       float* dW, const float* scale_dev, float logdet_coef, float* workspace, int64_t M, int c,
                       hipStream_t stream);
int dle_wg_logdet_inv(const float* W, float* logdet, float* WinvT, float* sign, int c, hipStream_t stream);
int dle_wg_coupling_partials(int64_t M);
int dle_wg_coupling_fwd(const float* y, const float* o, float* z, float* logs_partial, int64_t M, int c, hipStream_t stream);
int dle_wg_coupling_bwd(const float* dz, const float* y, const float* o, float* dy, void* d_o16, const float* scale_dev,
                        float logs_coef, int64_t M, int c, int dtype, hipStream_t stream);
int dle_wg_loss(const float* z, const float* logs_partial, int n_logs, const float* logdets, int n_flows, float sigma,
                int64_t M, float* loss_out, float* workspace, hipStream_t stream);
int dle_wg_dz_init(const float* z, float* dz, const float* scale_dev, float coef, int64_t M, hipStream_t stream);
int dle_wg_weight_norm_fwd(const float* v, const float* g, void* w16, int Co, int Ci, int Kt, int Cip, int dtype,
                           hipStream_t stream);
int dle_wg_weight_norm_bwd(const float* dw, const float* v, const float* g, float* dv, float* dg, int Co, int Ci, int Kt,
                           int Cip, hipStream_t stream);
int dle_wg_upsample_weight(const float* w, const float* bias, void* b16, float* bias_rep, int Cm, int ksize, int stride,
                           int dtype, hipStream_t stream);
int dle_wg_upsample_weight_bwd(const float* db, float* dw, int Cm, int ksize, int stride, hipStream_t stream);
/* One launch for every tensor of the network.  Weight-norm table: n_entries x 11 int64 = { row_start, Co, Ci, Kt, Cip, v, g
 * (0: plain weight), w16, dw, dv, dg } (device addresses), sorted by row_start, total_rows = sum of Co.  Log-determinant
 * table: n_flows x 2 int64 = { element offset of the c x c matrix from base, c }; WinvT: n_flows x 64 floats. */
int dle_wg_weight_norm_fwd_batched(const int64_t* table_dev, int n_entries, int64_t total_rows, int dtype, hipStream_t stream);
int dle_wg_weight_norm_bwd_batched(const int64_t* table_dev, int n_entries, int64_t total_rows, hipStream_t stream);
int dle_wg_logdet_inv_batched(const float* base, const int64_t* table_dev, float* logdets, float* WinvT, float* signs,
                              int n_flows, hipStream_t stream);
/* Inference, WaveGlow.infer (model.py:234-272): one launch per flow of the reverse pass on the fp32 state [M, 8].
 * dle_wg_flow_inv: audio_1 = (audio_1 - b) * exp(-log_s) with o = (b | log_s | 0) fp32 [M, 8] from the `end` GEMM, then W^-1 on
 *   the c active columns [8-c, 8) (WinvT as dle_wg_logdet_inv(_batched) writes it).  early > 0: columns [8-c-early, 8-c) <-
 *   sigma * noise[:, z_col .. z_col+early), noise fp32 [M, 8] = the rows of the reference's z [B, 8, T/8].  Columns below pass
 *   through bit for bit; out may be state.  a0_16 (optional): the first next_c/2 columns from 8-next_c of the new state, zero
 *   padded to 8, 16-bit -- the `start` operand of the flow that runs next (the shape dle_wg_invconv_fwd emits).
 * dle_wg_flow_inv_first: the starting state, columns [8-c, 8) = sigma * noise[:, 0 .. c), the others 0, and its a0. */
int dle_wg_flow_inv(const float* state, const float* o, const float* WinvT, const float* noise, float* out, void* a0_16,
                    int64_t M, int c, int early, int z_col, float sigma, int next_c, int dtype, hipStream_t stream);
int dle_wg_flow_inv_first(const float* noise, float* out, void* a0_16, int64_t M, int c, float sigma, int dtype,
                          hipStream_t stream);

/* ---- Tacotron2 training step (csrc/tacotron2.hip): SpeechSynthesis/Tacotron2/tacotron2/model.py + loss_function.py -----------
 * dle_t2_lstm_fwd/bwd: the pointwise part of nn.LSTM / nn.LSTMCell (model.py:205-214,425-444) on gates [B, 4H] (i, f, g, o, biases
 *   included; replaced in place by the gate activations, which the backward reads) + the F.dropout on the hidden state (bit-packed
 *   keep mask of dle_dropout_fwd, bit <-> element keep_index + b*H + j, scale inv_keep); h goes to up to three row-strided
 *   destinations (the operand buffers of its consumers).  live (fp32 [B], optional): rows with 0 keep (h_prev, c_prev) and write 0
 *   to out_dst -- pack_padded_sequence semantics of the encoder (model.py:205-214).
 * dle_t2_attention_fwd/bwd: Attention.forward of one decoder step (model.py:79-121): energies v . tanh(q + pl) (pl = processed
 *   memory + location term, [B*Ti, A]), softmax over the first lengths[b] text positions, context = weights x memory ([B*Ti, E]);
 *   awc rows = (weights, cumulative weights, 0 x 6) 16-bit = the next step's location-convolution input.  Backward accumulates
 *   d_memory (fp32; NULL: the caller sums weights_t (x) d_ctx_t over the steps itself) / d_pm (fp32; NULL: the caller folds the
 *   kept d_pl with dle_t2_sum_steps) and the per-sample partials
 *   of dv (dv_acc fp32 [B, A]: one owner per row, no atomics; the caller folds the rows) across steps, writes d_pl (16-bit), dq
 *   (fp32 [B, A] and / or 16-bit dq16 = the operand of the query layer's products) and, when dctx16 is given, the summed context
 *   gradient in 16 bits.  The context gradient is the sum of up to three fp32 row-strided pieces d_ctx0..2 [B, E] (NULL = absent),
 *   the gradient reaching the weights the sum of d_aw0 (+ d_aw1) fp32 [B, Ti]: autograd's accumulation of the gradients a tensor
 *   receives from its consumers (model.py:405-455), done on load.  dh1 / dh2 of dle_t2_lstm_bwd likewise.
 *   wloc (forward) / wlocT (backward) non-NULL: the location term of the layer (model.py:40-76: Conv1d(2 -> F, kernel KL, no bias)
 *   on (previous, cumulative) weights followed by Linear(F -> A)) is fused: `pl` is then the processed memory alone, wloc the
 *   pre-multiplied 16-bit [A, KK] matrix (k = tap * 2 + channel, zero padded to KK >= 2 KL, KK % 16 == 0), wlocT its transpose
 *   [KK, A] (KK % 32 == 0); the backward writes the gradient of the previous weights to d_prev (may be d_aw0's buffer) and
 *   accumulates that of the cumulative weights into d_cum (may be d_aw1's), fp32 [B, Ti].
 * dle_t2_location_bwd: transpose of the row gather of the 2-channel location convolution (model.py:40-76): dcol 16-bit
 *   [B*Ti, KL*8] -> d_prev (channel 0, written) and d_cum (channel 1, accumulated), fp32 [B, Ti].
 * dle_t2_tanh_fwd: torch.tanh of the postnet (model.py:170).  dle_t2_mel_loss: MSE(mel_out) + MSE(mel_out + postnet) of
 *   Tacotron2Loss (loss_function.py:42-44) and its gradients (scaled by *scale_dev); workspace >= 1024 floats. */
int dle_t2_tanh_fwd(const void* x, void* y, int64_t n, int dtype, hipStream_t stream);
int dle_t2_lstm_fwd(void* gates, int64_t ld_g, const float* c_prev, float* c_out, void* d0, int64_t ld0, void* d1, int64_t ld1,
                    void* d2, int64_t ld2, const void* keep, int64_t keep_index, float inv_keep, const float* live,
                    const void* h_prev, int64_t ld_hp, void* out_dst, int64_t ld_out, int B, int H, int dtype, hipStream_t stream);
/* One LSTMCell of the decoder in ONE launch (the few-row weight-streaming kernel of csrc/gemm_smallm.hip with the cell as its
 * epilogue): gates [B, 4H] = x [B, K] w [4H, K]^T (+ bias[4H]) (+ addend [B, 4H], 16-bit, row pitch ld_g), rounded to 16 bits as
 * the unfused dle_gemm output would be, then exactly dle_t2_lstm_fwd: activations to `gates`, c_out, dropout(h) to d0..d2.
 * H, K and every pitch multiples of 8 and no pitch below its row (K, 4H, H), 16-byte aligned bases; keep_index is any bit
 * position, as for dle_t2_lstm_fwd. */
int dle_t2_lstm_gemm_fwd(const void* x, int64_t ldx, const void* w, int64_t ldw, const float* bias, const void* addend,
                         const float* c_prev, float* c_out, void* gates, int64_t ld_g, void* d0, int64_t ld0, void* d1, int64_t ld1,
                         void* d2, int64_t ld2, const void* keep, int64_t keep_index, float inv_keep, int B, int H, int K, int dtype,
                         hipStream_t stream);
int dle_t2_lstm_bwd(const float* dh, int64_t ld_dh, const float* dh1, int64_t ld_dh1, const float* dh2, int64_t ld_dh2,
                    const float* dc_next, const void* act, int64_t ld_act, const float* c_prev,
                    void* dgates, int64_t ld_dg, float* dc_prev, const void* keep, int64_t keep_index, float inv_keep,
                    const float* live, float* dh_prev, int B, int H, int dtype, hipStream_t stream);
int dle_t2_attention_fwd(const float* q, const void* pl, const float* v, const void* memory, const int64_t* lengths,
                         const void* awc_prev, void* tanh_out, float* aw_out, void* awc_next, void* d0, int64_t ld0, void* d1,
                         int64_t ld1, void* d2, int64_t ld2, const void* wloc, int KL, int KK, int B, int Ti, int A, int E, int dtype,
                         hipStream_t stream);
int dle_t2_attention_bwd(const float* d_ctx0, int64_t ld_c0, const float* d_ctx1, int64_t ld_c1, const float* d_ctx2, int64_t ld_c2,
                         const float* d_aw0, const float* d_aw1, const float* aw, const void* tanh_out, const float* v,
                         const void* memory, float* d_memory, void* d_pl, float* dq, void* dq16, void* dctx16, float* dv_acc,
                         float* d_pm_acc, const void* wlocT, int KL, int KK, float* d_prev, float* d_cum, int B, int Ti, int A, int E,
                         int dtype, hipStream_t stream);
/* out[r] += sum over the n_steps rows of x (16-bit [n_steps, R], R % 8 == 0), fp32 out: folds the kept per-step gradients of the
 * processed memory (d_pm_acc = NULL in dle_t2_attention_bwd). */
int dle_t2_sum_steps(const void* x, float* out, int n_steps, int64_t R, int dtype, hipStream_t stream);
int dle_t2_location_bwd(const void* dcol, float* d_prev, float* d_cum, int B, int Ti, int KL, int dtype, hipStream_t stream);
int dle_t2_mel_loss(const float* out_all, int64_t ld_out, const void* post, const float* target, const float* scale_dev,
                    void* d_out, int64_t ld_dout, void* d_post, float* loss, float* workspace, int64_t R, int n_mel, int dtype,
                    hipStream_t stream);
/* --mask-padding (Tacotron2.parse_output, model.py:648-655): rows (b, t) with t >= lengths[b] of x[B*To, cols] (row pitch ld,
 * dtype DLE_F32 / F16 / BF16) := value.  The trainer applies it to the mel outputs (0), the gate energies (1e3) and -- because
 * masked_fill_ cuts the graph at those positions -- to the gradients that flow back into them (0). */
int dle_t2_mask_rows(void* x, int64_t ld, int cols, const int64_t* lengths, int64_t B, int To, float value, int dtype,
                     hipStream_t stream);

/* ---- Tacotron2 inference (csrc/tacotron2.hip): the free-running decoder step of Decoder.infer (model.py:515-595) -------------
 * RNG contract of the prenet's dropout, which stays on at inference (model.py:129): the keep mask of decoder step t (0-based),
 * prenet layer l (0 or 1), over the row-major [B, prenet_dim] block is the counter-based stream of csrc/dropout.h with
 * (seed, call offset 1 + 2 t + l), p = 0.5 (kept values x 2).  t is read from a DEVICE word, so a captured graph draws fresh
 * masks on every replay and the same seed gives the same spectrogram.
 * state: int64 [4] on the device.  [0] / [1] = the step index as read by even / odd steps: a launch of parity p reads state[p],
 * dle_t2_frame_infer writes state[1 - p] = t + 1 (no launch reads a word that a workgroup of the same launch writes);
 * [2] = n_steps, the number of steps up to and including the first one after which no sample is unfinished (max_steps if that
 * never happens); [3] = 1 once that step has run.  Reset all four to 0 before step 0.
 * dle_t2_prenet_infer: relu(x W0^T) -> dropout -> relu(. W1^T) -> dropout for B <= 8 rows.  frame fp32 [B, NM] (NULL: the go
 *   frame, zeros), rounded to 16 bits as the trainer's decoder input is; w0 [P, NM], w1 [P, P] 16-bit; dst 16-bit [B, P] rows of
 *   pitch ld_dst (the prenet columns of the attention LSTM's operand); mask0 / mask1 (optional): the bit-packed keep masks
 *   [B P / 8] of the two layers; step_dev = &state[t & 1].
 * dle_t2_frame_infer: the tail of step t = state[parity].  hc 16-bit [B, K] = [decoder_hidden | context]; w 16-bit [NM + 1, K] =
 *   linear_projection's rows then gate_layer's, bias fp32 [NM + 1]; mel_out fp32 [B, out_steps, NM] and gate_out fp32
 *   [B, out_steps] receive row t; frame_next fp32 [B, NM] the next step's prenet input; then model.py:578-582 on the device:
 *   dec = sigmoid(gate) <= gate_threshold; not_finished *= dec; mel_lengths += not_finished (int32 [B]); n_steps / done / the step
 *   words as above.  A step with t >= max_steps (or out_steps) only advances the step words.  w0 != NULL: ONE workgroup runs the
 *   frame and, behind it, the prenet of step t + 1 into pre_dst (pitch ld_pre) -- the one-launch form of the pair. */
int dle_t2_prenet_infer(const float* frame, const void* w0, const void* w1, void* dst, int64_t ld_dst, void* mask0, void* mask1,
                        uint64_t seed, const int64_t* step_dev, int B, int NM, int P, int dtype, hipStream_t stream);
int dle_t2_frame_infer(const void* hc, int64_t ld_hc, const void* w, int64_t ldw, const float* bias, float* mel_out,
                       float* gate_out, float* frame_next, int32_t* not_finished, int32_t* mel_lengths, int64_t* state, int parity,
                       float gate_threshold, int max_steps, int64_t out_steps, const void* w0, const void* w1, void* pre_dst,
                       int64_t ld_pre, uint64_t seed, int B, int NM, int K, int P, int dtype, hipStream_t stream);

/* ---- the ReLU of an MLP layer as one bit per element (csrc/gemm8_kernel.h, round 6; Recommendation/DLRM/dlrm/nn/mlps.py:38-43,
 * 106-114 = apex mlp_cuda forward / backward).  dle_gemm8_relu_bits_try: Y [M, N] = relu(X [M, K] W [N, K]^T + bias) AND the keep
 * bits of Y (bits [M N / 8]: bit (m N + n) & 7 of byte (m N + n) >> 3 = rounded Y > 0); dense Y, N % 16 == 0.
 * dle_gemm_colsum_bits: the masked data gradient C = (A B) under those bits + the column sums of the rounded C (the bias gradient
 * of the layer below), as dle_gemm_colsum but reading 1 bit per element instead of the 16-bit activation; M % 256 == 0,
 * workspace >= ceil(M / 128) * N floats.  Both: 1 = launched, 0 = outside the ping-pong kernel's envelope (use dle_gemm with
 * DLE_ACT_RELU / dle_gemm_colsum with the activation), > 1 = error. */
int dle_gemm8_relu_bits_try(const void* X, const void* W, void* Y, void* bits, const float* bias, int M, int N, int K, int64_t ldx,
                            int64_t ldw, int dtype, hipStream_t stream);
int dle_gemm_colsum_bits(const void* A, const void* B, void* C, const void* bits, float* colsum_out, int M, int N, int K, int64_t lda,
                         int64_t ldb, int dtype, int accumulate_colsum, void* workspace, int64_t workspace_bytes,
                         hipStream_t stream);

/* ---- HiFi-GAN generator, inference (csrc/hifigan.hip; SpeechSynthesis/HiFiGAN/hifigan/models.py) ----------------------------
 * Activations channels-last [B, T, C], 16-bit; weights 16-bit; fp32 accumulation on MFMA; no allocation, no synchronisation.
 * dle_conv1d_lrelu_fwd: "same" dilated Conv1d with the leaky ReLU that precedes it and the elementwise steps that follow it:
 *     a[b,t,c]  = x < 0 ? round16(fl32(float(x) * slope)) : x                  (slope == 1: a = x; applied once, where the tile is staged)
 *     acc       = sum_k sum_c float(w[ko,k,c]) * float(a[b, t + (k - (ksize-1)/2) * dilation, c])       (0 outside [0, T))
 *     y[b,t,ko] = round16((acc + bias[ko] (+ add1[b,t,ko]) (+ add2[b,t,ko])) * alpha)                   (one rounding)
 *   w [Ko, ksize, C] = torch's Conv1d weight permuted (0, 2, 1); bias fp32 [Ko]; add1 / add2 16-bit [B, T, Ko] or NULL.
 *   Envelope: C, Ko multiples of 8 in [8, 2048]; ksize odd in [1, 11]; dilation >= 1 with (ksize-1)/2 * dilation <= 36; B >= 0,
 *   T >= 1; every tensor < 4 GiB; operands 16-byte aligned.  y must not overlap x.  y MAY be add1 or add2 itself (the same base
 *   pointer: every element is read by the lane that then writes it); a partial overlap is an error.
 * dle_hfg_post_fwd: audio[b,t] = tanhf(bias[0] + sum_k sum_c float(w[k,c]) * float(a[b, t + k - (ksize-1)/2, c])), fp32 [B, T],
 *   `a` as above; w 16-bit [ksize, C]; C a multiple of 8 in [8, 64], ksize odd in [1, 11]. */
int dle_conv1d_lrelu_fwd(const void* x, const void* w, const float* bias, const void* add1, const void* add2, void* y, int B, int T,
                         int C, int Ko, int ksize, int dilation, float slope, float alpha, int dtype, hipStream_t stream);
int dle_hfg_post_fwd(const void* x, const void* w, const float* bias, float* audio, int B, int T, int C, int ksize, float slope,
                     int dtype, hipStream_t stream);

/* ---- FastPitch, inference on PACKED utterances (csrc/fastpitch.hip; SpeechSynthesis/FastPitch/fastpitch/model.py:327-385) ----
 * Activations 16-bit channels-last [total_rows, C]; sequence b owns rows cu[b] .. cu[b + 1] - 1 of a DEVICE int32 table
 * cu[B + 1] (cu[0] = 0).  No padding rows, no masks: rows outside a row's OWN sequence read as zero, so every utterance gets what
 * the reference gives it at batch 1.  Common envelope: B >= 1, 1 <= max_len <= 1024, total >= 1 (those of dle_attention_fwd_varlen).
 * Lengths are clamped to [0, max_len] and rows to `total` inside every kernel: a wrong table gives wrong answers but reaches no
 * memory outside the operands.  No allocation, no synchronisation, the caller's stream; 0 = ok, -1 / a HIP error otherwise
 * (dle_last_error).
 *
 * dle_conv1d_packed_fwd: "same" Conv1d, dilation 1 (transformer.py:47-52 CoreNet's two convolutions with the ReLU between them,
 *   common/layers.py:79-86 ConvReLUNorm's convolution), per sequence:
 *     a[r,c]  = x < 0 ? round16(fl32(float(x) * slope)) : x        (slope 1: no activation; slope 0: ReLU; applied once, at staging)
 *     acc     = sum_k sum_c float(w[ko,k,c]) * float(a[r + k - (ksize-1)/2, c])                (0 outside the row's own sequence)
 *     y[r,ko] = round16(acc + bias[ko] (+ add1[r,ko]))                                          (fp32 accumulation on MFMA, one rounding)
 *   w [Ko, ksize, C] = torch's Conv1d weight permuted (0, 2, 1); bias fp32 [Ko]; add1 16-bit [total, Ko] or NULL, and it may be y
 *   itself (the same base pointer).  C, Ko multiples of 8 in [8, 2048]; ksize odd in [1, 11]; tensors < 4 GiB, 16-byte aligned;
 *   y must not overlap x.  One workgroup per (sequence, 64-row tile, 128-channel block).
 * dle_fp_relu_layernorm_fwd: the tail of ConvReLUNorm (common/layers.py:86-87) and TemporalPredictor.fc (model.py:103,108):
 *     t = relu(x);  y[r,:] = round16((t - mean) * rstd * gamma + beta)   (fp32 statistics, biased variance, rstd = rsqrt(var + eps))
 *     pred[r,j] = fc_b[j] + sum_c fc_w[j,c] * float(y[r,c])               (fp32 [rows, n_pred], on the ROUNDED y; n_pred = 0: none)
 *   H a multiple of 8, <= 1024; n_pred in [0, 4]; fc_w fp32 [n_pred, H]; y may be NULL when only pred is wanted.
 * dle_fp_embed: y[r,:] = round16((word[ids[r],:] + pos[p,:]) (+ spk[:])), p = r's position inside its sequence (transformer.py:200-207
 *   with model.py:331-337); ids int64 [total] (clamped to the table), word fp32 [n_symbols, D], pos fp32 [n_pos >= max_len, D], spk
 *   fp32 [D] or NULL; fp32 additions in that order.
 * dle_fp_scalar_conv_add: pitch_emb / energy_emb (model.py:183-186, 358-373), Conv1d(1 -> D, ksize) of an fp32 per-token series
 *   v [total], added in place:  s = b[c]; for k = 0 .. ksize-1: s = fl(s + fl(w[c,k] * v[r + k - (ksize-1)/2]))  (0 outside the
 *   sequence);  enc[r,c] = round16(fl(float(enc[r,c]) + s)).  w fp32 [D, ksize], ksize odd in [1, 11].
 * dle_fp_durations: model.py:344 and regulate_len's integer part (model.py:47-55), ONE workgroup.  from_log != 0: src = log
 *   durations, dur = clamp(expf(src) - 1, 0, max_duration), written to dur_pred (fp32 [total], may be NULL); from_log == 0: src =
 *   durations, dur_pred untouched.  reps[i] = (int)(dur / pace + 0.5f) in fp32 (IEEE division; negative or NaN: 0);
 *   tok_start[i] = sum of reps of the tokens before i in its sequence; cu_out[B + 1] = prefix sum of the sequences' frame counts.
 *   A sequence's frames are cut at max_out (its last tokens lose repetitions) so that tok_start and cu_out stay consistent.
 *   All int32 (the reference casts the cumsum to fp16 under AMP, exact to 2048 only: not copied).  B <= 65536.
 * dle_fp_expand: the length regulator (model.py:57-61) as a gather + the decoder's positional embedding (transformer.py:204-207):
 *   y[cu_out[b] + p, :] = round16(float(enc[j,:]) + pos[p,:]), j = the token of sequence b with tok_start[j] <= p < tok_start[j] +
 *   reps[j] (binary search per row; tokens with 0 repetitions vanish).  pos fp32 [n_pos >= max_out, D].
 * dle_fp_unpack_mel: packed proj output [total_out, n_mel] 16-bit -> mel fp32 [B, n_mel, t_pad]; frames at and behind a sequence's
 *   length hold bias[m] (what proj gives the reference's zeroed padding rows, model.py:381-384).  1 <= t_pad <= 1024. */
int dle_conv1d_packed_fwd(const void* x, const void* w, const float* bias, const void* add1, void* y, const int32_t* cu_seqlens,
                          int B, int max_len, int64_t total, int C, int Ko, int ksize, float slope, int dtype, hipStream_t stream);
int dle_fp_relu_layernorm_fwd(const void* x, void* y, const float* gamma, const float* beta, const float* fc_w, const float* fc_b,
                              float* pred, int64_t rows, int H, int n_pred, float eps, int dtype, hipStream_t stream);
int dle_fp_embed(const int64_t* ids, const float* word, const float* pos, const float* spk, void* y, const int32_t* cu_seqlens,
                 int B, int max_len, int64_t total, int n_symbols, int n_pos, int D, int dtype, hipStream_t stream);
int dle_fp_scalar_conv_add(void* enc, const float* v, const float* w, const float* bias, const int32_t* cu_seqlens, int B, int max_len,
                           int64_t total, int D, int ksize, int dtype, hipStream_t stream);
int dle_fp_durations(const float* src, int from_log, float* dur_pred, int32_t* reps, int32_t* tok_start, int32_t* cu_out,
                     const int32_t* cu_in, int B, int max_len, int64_t total, float pace, float max_duration, int max_out,
                     hipStream_t stream);
int dle_fp_expand(const void* enc, const float* pos, const int32_t* reps, const int32_t* tok_start, const int32_t* cu_in,
                  const int32_t* cu_out, void* y, int B, int max_in, int64_t total_in, int max_out, int64_t total_out, int n_pos,
                  int D, int dtype, hipStream_t stream);
int dle_fp_unpack_mel(const void* x, const float* bias, float* mel, const int32_t* cu_seqlens, int B, int64_t total, int n_mel,
                      int t_pad, int dtype, hipStream_t stream);

/* ---- QuartzNet, inference on PACKED utterances (csrc/quartznet.hip; SpeechRecognition/QuartzNet/quartznet/model.py:80-112,
 * 207-292, 341-349; common/features.py:158-170, 290-302; common/helpers.py:35-61) ----------------------------------------------
 * The conventions of the FastPitch block: activations 16-bit channels-last [total_rows, C]; sequence tables DEVICE int32 cu[B + 1],
 * cu[0] = 0; starts and lengths are clamped inside every kernel (a wrong table gives wrong answers but reaches no memory outside the
 * operands); no allocation, no synchronisation, the caller's stream; 0 = ok, -1 / a HIP error otherwise (dle_last_error); every
 * operand 16-byte aligned, every tensor < 4 GiB; anything outside an envelope is an argument error, never a fallback.
 *
 * dle_tcs_conv1d_packed_fwd: ONE launch per time-channel separable unit (model.py:207-249, the `separable` branch: depthwise
 *   MaskedConv1d -> pointwise MaskedConv1d -> BatchNorm1d(eps 1e-3), with JasperBlock.forward's residual sum and `mout` for the last
 *   unit of a block).  For output row p of sequence b, len = cu_in[b+1] - cu_in[b], out_len = (len - 1) / stride + 1 =
 *   cu_out[b+1] - cu_out[b] (stride 1: cu_out may be cu_in itself):
 *     d[p,c]  = round16( sum_k float(dw[k,c]) * float(x[cu_in[b] + p*stride + (k - ksize/2)*dilation, c]) )     (index outside [0, len): 0)
 *     y[p,ko] = round16( relu?( fmaf(scale[ko], sum_c float(pw[ko,c]) * float(d[p,c]), shift[ko]) + float(residual[p,ko]) ) )
 *   Both sums accumulate in fp32: the depthwise as one fmaf chain over the taps in ascending order, the pointwise on MFMA over the
 *   UNMODIFIED 16-bit weights (no folded copy).  d is rounded once to the storage type (what the reference's half-precision depthwise
 *   convolution hands to its pointwise one) and never goes to HBM, except through d_out; y is rounded once.
 *   dw [ksize, C] = torch's depthwise weight [C, 1, ksize] transposed; pw [Ko, C]; scale / shift fp32 [Ko]; residual 16-bit
 *   [total_out, Ko] or NULL; d_out 16-bit [total_out, C] or NULL: the d tile as it is fed to the MFMA (y is bit-identical with and
 *   without it).  Envelope: C, Ko multiples of 64 in [64, 1024]; ksize odd in [3, 127]; stride, dilation in {1, 2}, not both 2
 *   (model.py:60-63); B >= 1; zero-length sequences produce nothing; no operand aliases another.
 *   One workgroup per (sequence, tile of 64 OUTPUT rows, block of 256 output channels), C walked in chunks of 64 channels; the
 *   depthwise thread owns a channel pair x 8 rows and takes the taps in blocks of 8.  Not persistent: no grid cap.  Two forms of
 *   the chunk loop give the same bits: with a register prefetch of the next chunk (grids of at most one workgroup per CU) and
 *   without.  dle_tcs_prefetch_mode(0 / 1 / 2): never / always / by grid size (the default); -1: query; returns the previous
 *   setting (tests and A/B timing, as dle_gemm8_mode).
 * dle_qn_normalize_pack: normalize_batch(.., "per_feature"), the mask, the transpose and the 16-bit cast (features.py:158-170,
 *   290-302): x fp32 [B, F, T_pad] log-mel -> y[cu[b] + t, f] = round16((x[b,f,t] - mean_bf) / (std_bf + 1e-5)) for t < len_b; mean
 *   and UNBIASED standard deviation over the sequence's own frames in fp32 (two passes); IEEE division.  F a multiple of 8, <= 128.
 *   A sequence of one frame gives NaN as the reference does (the host rejects it).
 * dle_ctc_greedy_packed: log_softmax + GreedyCTCDecoder + ctc_decoder_predictions_tensor (model.py:341-349, helpers.py:35-61).
 *   logits fp32 [total, ld], the first n_classes <= ld columns of a row count; logp fp32 [total, n_classes] or NULL; ids int32 [total]
 *   = the FIRST maximum of the row; tokens int32 [total]: packed per sequence at cu[b], the ids left after
 *   `(p != previous or previous == blank) and p != blank` (previous = blank in front of the first row); n_tokens int32 [B];
 *   blank = n_classes - 1.  One workgroup per sequence.  2 <= n_classes <= 4096. */
int dle_tcs_conv1d_packed_fwd(const void* x, const void* dw, const void* pw, const float* scale, const float* shift,
                              const void* residual, void* y, void* d_out, const int32_t* cu_in, const int32_t* cu_out,
                              int B, int64_t total_in, int64_t total_out, int C, int Ko, int ksize, int stride, int dilation,
                              int relu, int dtype, hipStream_t stream);
int dle_tcs_prefetch_mode(int mode);
int dle_qn_normalize_pack(const float* x, void* y, const int32_t* cu_seqlens, int B, int F, int T_pad, int64_t total, int dtype,
                          hipStream_t stream);
int dle_ctc_greedy_packed(const float* logits, float* logp, int32_t* ids, int32_t* tokens, int32_t* n_tokens,
                          const int32_t* cu_seqlens, int B, int64_t total, int n_classes, int ld, hipStream_t stream);

/* ---- Jasper, inference on PACKED utterances (csrc/jasper.hip, csrc/quartznet.hip; SpeechRecognition/Jasper/jasper/model.py:58-85,
 * 128-162; inference.py:329-333) ------------------------------------------------------------------------------------------------
 * The conventions of the QuartzNet block above.
 *
 * dle_conv1d_bn_packed_fwd: ONE launch per Jasper sub-block: dense MaskedConv1d -> BatchNorm1d(eps 1e-3, evaluation mode), with
 *   JasperBlock.forward's residual sum and activation for the last sub-block of a block.  For output row p of sequence b,
 *   len = cu_in[b+1] - cu_in[b], out_len = (len - 1) / stride + 1 = cu_out[b+1] - cu_out[b] (stride 1: cu_out may be cu_in itself):
 *     acc     = sum_k sum_c float(w[ko,k,c]) * float(x[cu_in[b] + p*stride + (k - ksize/2)*dilation, c])     (index outside [0, len): 0)
 *     y[p,ko] = round16( relu?( fmaf(scale[ko], acc, shift[ko]) + float(residual[p,ko]) ) )
 *   acc is fp32 on v_mfma_f32_32x32x16_{bf16,f16} over the UNMODIFIED 16-bit weights (no folded copy); y is rounded once.
 *   w [Ko, ksize, C] = torch's Conv1d weight [Ko, C, ksize] permuted (0, 2, 1); scale / shift fp32 [Ko]; residual 16-bit
 *   [total_out, Ko] or NULL.  Envelope: C, Ko multiples of 64 in [64, 1024]; ksize odd in [1, 29]; stride, dilation in {1, 2}, not
 *   both 2 (model.py:52-55); B >= 1; no cap on the sequence length; zero-length sequences produce nothing; no operand aliases y.
 *   One workgroup per (sequence, tile of 128 OUTPUT rows, block of 128 output channels), C walked in chunks of 64 channels; the
 *   input rows of a chunk and the weight slab of a (chunk, tap) are staged in LDS once per workgroup, double-buffered (up to
 *   118,368 bytes of dynamic LDS).  Not persistent: no grid cap.  The loop has one form.
 * dle_qn_normalize_pack_lead: dle_qn_normalize_pack with `lead` >= 0 zero rows in front of every sequence (inference.py:329-333,
 *   --pad_leading on the normalised features): cu describes the OUTPUT rows, len_b + lead per sequence; rows [0, lead) of a
 *   sequence are zero, the statistics run over the len_b real frames; lead = 0 gives the bits of dle_qn_normalize_pack. */
int dle_conv1d_bn_packed_fwd(const void* x, const void* w, const float* scale, const float* shift, const void* residual, void* y,
                             const int32_t* cu_in, const int32_t* cu_out, int B, int64_t total_in, int64_t total_out, int C, int Ko,
                             int ksize, int stride, int dilation, int relu, int dtype, hipStream_t stream);
int dle_qn_normalize_pack_lead(const float* x, void* y, const int32_t* cu_seqlens, int B, int F, int T_pad, int lead, int64_t total,
                               int dtype, hipStream_t stream);

/* ---- Transformer-XL, evaluation with memory (csrc/transformer_xl.hip; LanguageModeling/Transformer-XL/pytorch/mem_transformer.py,
 * utils/proj_adaptive_softmax.py) ------------------------------------------------------------------------------------------------
 * All tensors 16-bit (DLE_F16 / DLE_BF16) unless said otherwise, 16-byte aligned; accumulation, softmax and the scale are fp32.
 *
 * dle_txl_rel_attention_fwd: RelPartialLearnableMultiHeadAttn.forward between qkv_net and o_net (mem_transformer.py:249-293, with
 *   _rel_shift :210-223 and the masks of MemTransformerLM._forward :691-699) in ONE launch per layer and segment:
 *     a_i = round16(float(q_i) + float(u)),  b_i = round16(float(q_i) + float(v))                  (u = r_w_bias, v = r_r_bias)
 *     score(i,j)   = scale * ( a_i . K_j + b_i . r[i + mlen - j] )
 *     allowed(i,j) = (i - shift < j) and (j <= i + mlen)
 *     ctx_i        = round16( sum_j softmax_j(score(i,.) over the allowed j) * V_j )
 *   q [B*qlen, ldq], rows batch-major, head h at columns h*64 (ldq lets it read the Q third of a [.., 3H] projection in place);
 *   u, v [heads, 64]; kv a RING [B, cap, 2H], K in columns 0..H-1 and V in H..2H-1: logical key j (0 <= j < klen = mlen + qlen)
 *   of batch element n lives at physical row (start + j) mod cap, the last qlen logical rows are the current segment's; r
 *   [n_dist, H] indexed BY DISTANCE (row d = r_net(pos_emb(min(d, clamp_len))), n_dist >= klen); ctx [B*qlen, H].  shift =
 *   qlen - (klen - mem_len - 1) under same_length when that is positive, any value >= qlen for "no lower bound".  Physical ring
 *   rows outside the logical window never influence the result, whatever bits they hold.
 *   Envelope: head_dim == 64, 1 <= qlen <= 512, 0 <= mlen, klen <= cap <= 4096, 0 <= start < cap, shift >= 1, every operand below
 *   4 GiB; dle_txl_attention_supported(qlen, klen, head_dim) tells; anything else is -1 and a message, nothing launched.
 *   dle_txl_attention_launch_count: launches by this process so far (tests).
 * dle_txl_kv_append: the K and V thirds of the segment's projection qkv [B*qlen, ld >= 3H] -> ring rows (start + mlen + t) mod cap
 *   (what `cat([mems, w])` followed by qkv_net recomputes in the reference, :239-247; _update_mems :652-682 is the ring's start).
 * dle_rows_gather_scale: dst[dst_idx[r], :width] = round16(scale * float(src[src_idx[r], :width])) for r < rows; either int32 index
 *   list may be NULL (= r).  The embedding lookup times sqrt(d_model) (AdaptiveEmbedding.forward :484-513) and the row gathers /
 *   scatters of both adaptive layers (proj_adaptive_softmax.py:166-199).  width a multiple of 8; a row whose index is outside
 *   [0, n_src_rows) / [0, n_dst_rows) is skipped; destination rows must be distinct.
 * dle_row_nll: nll[pos[r]] (+)= logsumexp(logits[r, :n_classes]) - logits[r, target[r]] on fp32 logits [rows, ld]
 *   (-log_softmax(..).gather(..), proj_adaptive_softmax.py:150-152, 179-199); pos int32 or NULL (= r), positions of one call
 *   distinct; accumulate != 0 adds.  One workgroup per row, 1 <= n_classes <= 160003; a row whose target or position is out of
 *   range writes nothing. */
int dle_txl_attention_supported(int qlen, int klen, int head_dim);
uint64_t dle_txl_attention_launch_count(void);
int dle_txl_rel_attention_fwd(const void* q, int64_t ldq, const void* u, const void* v, const void* kv, const void* r, void* ctx,
                              int B, int heads, int head_dim, int qlen, int mlen, int cap, int start, int n_dist, int shift,
                              float scale, int dtype, hipStream_t stream);
int dle_txl_kv_append(const void* qkv, int64_t ld, void* kv, int B, int H, int qlen, int mlen, int cap, int start, int dtype,
                      hipStream_t stream);
int dle_rows_gather_scale(const void* src, const int32_t* src_idx, void* dst, const int32_t* dst_idx, int64_t rows, int width,
                          int64_t ld_src, int64_t ld_dst, int64_t n_src_rows, int64_t n_dst_rows, float scale, int dtype,
                          hipStream_t stream);
int dle_row_nll(const float* logits, int64_t ld, const int32_t* target, const int32_t* pos, float* nll, int64_t rows,
                int n_classes, int64_t n_out, int accumulate, hipStream_t stream);

/* ---- Temporal Fusion Transformer inference (csrc/tft.hip; reference PyTorch/Forecasting/TFT/modeling.py) ---------------------
 * Hidden size 128 only; 16-bit tensors (DLE_F16 / DLE_BF16) 16-byte aligned with pitches that are multiples of 8, weights
 * row-major [out][in] as nn.Linear keeps them, biases / LayerNorm parameters / quantile weights fp32, accumulation fp32.
 * Anything outside an envelope is -1 and a message, nothing launched.
 *
 * dle_tft_grn_fwd: GRN.forward (modeling.py:48-77) on 32 rows per workgroup, one launch:
 *     h = ELU(wa x + ba [+ wc ctx[row / rows_per_ctx]]);  g = wi round16(h) + bi;  (a | b) = wg round16(g) + bg;
 *     out = LayerNorm(a * sigmoid(b) + x; gamma, beta, eps)
 *   x_index (int32 or NULL): row r of x is x[x_index[r]] (the static embedding gather, :169); an index outside [0, n_x_rows)
 *   reads a zero row.  Gate mode, wa == NULL (wi, wc, ctx, ba, bi NULL too): the GLU is applied to x itself and the residual is
 *   `res`, row r at res + r * ldr, or at res + (r / res_rows_per_batch) * res_batch_stride + (r % res_rows_per_batch) * ldr when
 *   res_rows_per_batch > 0 -- input_gate / attention_gate / decoder_gate with their LayerNorms (:403-405, 418-420, 426-428).
 *   Tail, qout != NULL: qout[r, q] = bq[q] + sum_n wq[q, n] out[r, n] on the unrounded LayerNorm output, 1 <= nq <= 8
 *   (quantile_proj, :430); out may then be NULL.
 * dle_tft_vsn_fwd: the embedding of continuous variables and VariableSelectionNetwork.forward (:162-189, 286-303) in one launch.
 *   Row r = (b, t) of the launch reads the F = n0 + n1 + n2 raw values x_s[(b * src_steps + src_t0 + t) * ld_s + j] (fp32, up to
 *   three column groups) and writes out[(b * out_steps + out_t0 + t) * ldo]; ctx [batch, ldc] or NULL; weights [rows, F] fp32 or
 *   NULL.  w16 / p32 are the packed parameter blocks whose layout csrc/tft.hip states (functional.tft_vsn_pack builds them; the
 *   first linear of every network is folded over the rank-1 embedding there).  1 <= F <= 8; with F == 1 the joint LayerNorm is
 *   the Identity of MaybeLayerNorm and the weight is exactly 1.
 * dle_tft_lstm_fwd: nn.LSTM(128, 128) over T steps (:368-370, 395-397), gates i, f, g, o: xproj fp32 = W_ih x + b_ih + b_hh for
 *   every step, row (b, t) at xproj + b * xp_batch_stride + t * xp_step_stride; whh [512][128]; h0 [B, 128]; c0 [B, 128] fp32 or
 *   the operand type (c0_dtype); out (16-bit, may be NULL) row (b, t) at out + b * out_batch_stride + t * out_step_stride; hn
 *   [B, 128] 16-bit and cn [B, 128] fp32 (either may be NULL).  One workgroup per 32 batch rows, no wait between workgroups.
 * dle_tft_attention_fwd: InterpretableMultiHeadAttention.forward behind qkv_linears for positions encoder_length .. T - 1 only
 *   (:337-360, 414): qkv [B * T, ld >= 288] = (q of 4 heads | k of 4 heads | shared v), causal mask by index, mean of the heads'
 *   probabilities times V, out_proj wo [128][32] -> out [B, T - encoder_length, 128]; probs (fp32 [B, T - encoder_length, T] or
 *   NULL) receives the mean probabilities, zeros behind the mask.  4 heads of 32, 2 <= T <= 192, 1 <= encoder_length < T. */
int dle_tft_grn_fwd(const void* x, int64_t ldx, const int32_t* x_index, int64_t n_x_rows, const void* ctx, int64_t ldc,
                    int64_t rows_per_ctx, const void* res, int64_t ldr, int64_t res_rows_per_batch, int64_t res_batch_stride,
                    const void* wa, const float* ba, const void* wc, const void* wi, const float* bi, const void* wg,
                    const float* bg, const float* gamma, const float* beta, float eps, void* out, int64_t ldo, const float* wq,
                    const float* bq, float* qout, int nq, int64_t rows, int hidden, int dtype, hipStream_t stream);
int dle_tft_vsn_fwd(const float* x0, int64_t ld0, int n0, const float* x1, int64_t ld1, int n1, const float* x2, int64_t ld2, int n2,
                    int64_t rows_per_batch, int64_t src_steps, int64_t src_t0, const void* ctx, int64_t ldc, const void* w16,
                    const float* p32, void* out, int64_t ldo, int64_t out_steps, int64_t out_t0, float* weights, int64_t rows,
                    int hidden, float eps, int dtype, hipStream_t stream);
int dle_tft_lstm_fwd(const float* xproj, int64_t xp_batch_stride, int64_t xp_step_stride, const void* whh, const void* h0,
                     const void* c0, int c0_dtype, void* out, int64_t out_batch_stride, int64_t out_step_stride, void* hn, float* cn,
                     int B, int T, int hidden, int dtype, hipStream_t stream);
int dle_tft_attention_fwd(const void* qkv, int64_t ld, const void* wo, void* out, float* probs, int B, int T, int encoder_length,
                          int heads, int d_head, int dtype, hipStream_t stream);

/* ---- Neural Collaborative Filtering inference and evaluation (csrc/ncf.hip; reference PyTorch/Recommendation/NCF) -----------
 * dle_ncf_score_fwd: NeuMF.forward (neumf.py:80-98) with the sigmoid of inference.py:90 and the binary cross-entropy of
 *   val_epoch (ncf.py:141-144), one persistent launch:
 *     logit[b] = wf[:F] . (mf_user[user[b]] * mf_item[item[b]]) + wf[F:] . relu(W3 h2 + b3) + bf,
 *     h1 = round16(relu(W1 [mlp_user[user[b]] | mlp_item[item[b]]] + b1)),  h2 = round16(relu(W2 h1 + b2)).
 *   Tables mf_* [n, factors], mlp_* [n, l0 / 2] and W1 [l1][l0], W2 [l2][l1], W3 [l3][l2] are 16-bit (DLE_F16 / DLE_BF16), row-major,
 *   16-byte aligned; b1..b3, wf [factors + l3] and bf [1] are fp32.  Rounding contract: h1 and h2 are rounded to 16 bits once, on
 *   their way into the next MFMA operand; the GMF product, the third layer's output, the dot product, the sigmoid and the loss
 *   are fp32 and never rounded.  user / item: `batch` indices of index_bits = 32 or 64.  A sample whose user or item index is
 *   outside [0, n_users) / [0, n_items) reads nothing from the tables, gets a NaN logit and probability and adds nothing to the
 *   loss.  prob (fp32 [batch] or NULL) = sigmoid(logit).  label (fp32 [batch]) and loss_partials (fp32 [n_partials]) go together
 *   or are both NULL: workgroup g writes the sum of -(y max(log p, -100) + (1 - y) max(log(1 - p), -100)) over its samples to
 *   loss_partials[g] (computed from the fp32 logit), the slots behind the grid are zeroed, no atomics: the caller folds them.
 *   The grid is min(ceil(batch / 64), max_workgroups or the device's CU count when 0, n_partials when the loss is asked for).
 *   Envelope (dle_ncf_score_supported, host only, 1 / 0): factors 64, layers 256 256 128 64 -- ncf.py's defaults (:69-73).
 * dle_ncf_rank_fwd: the ranking tail of val_epoch (ncf.py:150-162: the -1 over the mask, topk, gather, nonzero) per series of S
 *   elements, without a sort and without topk's tie order: r_j = -1 where ignore_j (one byte per element, or NULL) is set, else
 *   rating_j; rank_j = #{i : r_i > r_j or (r_i == r_j and i < j)}; NaN ranks below everything, NaNs among themselves by index.
 *   hits[s] = #{j : label_j == 1 and rank_j < k}, dcg[s] = sum over those j of log 2 / log(rank_j + 2).  1 <= k <= S <= 4096.
 * Both: -1 and a message, nothing launched, on a bad argument.                                                                 */
int dle_ncf_score_supported(int factors, int l0, int l1, int l2, int l3);
int dle_ncf_score_fwd(const void* mf_user, const void* mf_item, const void* mlp_user, const void* mlp_item, int64_t n_users,
                      int64_t n_items, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                      const float* b3, const float* wf, const float* bf, const void* user, const void* item, int index_bits,
                      const float* label, float* logit, float* prob, float* loss_partials, int n_partials, int64_t batch,
                      int factors, int l0, int l1, int l2, int l3, int max_workgroups, int dtype, hipStream_t stream);
int dle_ncf_rank_fwd(const float* rating, const float* label, const uint8_t* ignore, int32_t* hits, float* dcg, int64_t n_series,
                     int S, int k, hipStream_t stream);

/* ---- nnU-Net BraTS22 UNet3D inference (csrc/nnunet.hip; reference PyTorch/Segmentation/nnUNet/nnunet/brats22_model.py) ------
 * Volumes are channels-last: x [N, D, H, W, ldx], y [N, P, Q, R, ldy], 16-bit (DLE_F16 / DLE_BF16); a tensor is addressed as
 * (base, leading dimension, channel offset), so a layer reads and writes a channel slice of a wider buffer (the concat buffer of
 * UpsampleBlock.forward, :119-121, is never copied into).  Statistic partials: fp32 [N][G][channels][3] = (count, sum, M2) of the
 * STORED 16-bit values over the output voxels of band g of sample n, written once by one workgroup in a fixed order, no atomics.
 * dle_conv3d_in_fwd: ConvLayer.forward (:94-98: InstanceNorm3d, Conv3d 3x3x3 pad 1 bias=False, ReLU) and the two halves of
 *   InputBlock.forward (:78-84), with the normalisation applied on the operand load:
 *     a[n,d,h,w,c]  = inside the volume ? round16(relu_in ? max(.,0) : . of fmaf(scale[n,c], float(x), shift[n,c])) : 0
 *                     (scale == shift == NULL: a = x)
 *     y[n,p,q,r,ko] = round16(relu_out ? max(acc, 0) : acc),  acc = fp32 sum over the 27 taps and c of float(w) * float(a)
 *   w [Ko][3][3][3][C]; scale, shift fp32 [N][C]; stride 1 or 2, P = (D - 1) / stride + 1; part NULL or [N][G][Ko][3] with
 *   G = dle_conv3d_in_bands(D, H, W, stride) (host only).  Envelope: Ko % 64 == 0; C % 64 == 0 or C == 8; offsets and leading
 *   dimensions multiples of 8; every pointer 16-byte aligned; every tensor below 2^31 elements.
 * dle_instnorm_fold: nn.InstanceNorm3d(affine=True) in eval (:37) as a table: the bands of part [N][G][C][3] are merged by
 *   Chan's formula in band order, scale = gamma / sqrt(M2 / count + eps), shift = beta - mean * scale (biased variance), written to
 *   scale / shift [N][ld_out] at channel out_off.
 * dle_upsample3d_x2_fwd: F.interpolate(scale_factor=2, mode="trilinear", align_corners=True) (:119): output index i of an axis
 *   of extent E reads position i (E - 1) / (2 E - 1) (extent 1 copies); nested fp32 lerps along w, h, d, one rounding; part NULL
 *   or [N][G][C][3], G = dle_upsample3d_x2_bands(D, H, W).  C % 8 == 0, C <= 2048.
 * dle_nnunet_head_blend_fwd: OutputBlock.forward (:130-131, 1x1x1 convolution with bias) of ONE window x [Dp, Hp, Wp, ldx] fused
 *   with the weighted accumulation of sliding_window_inference:
 *     out[k, d0 + d, h0 + h, w0 + w] += imp[d,h,w] * (b[k] + sum_c float(w[k,c]) * float(x[d,h,w,c]))
 *   out fp32 [K, Dv, Hv, Wv], imp fp32 [Dp, Hp, Wp], w 16-bit [K][C], b fp32 [K]; K <= 8, C % 8 == 0, C <= 512.  One window per
 *   launch: overlapping windows are ordered by the stream, no atomics.
 * All: no allocation, no synchronisation, graph capturable; -1 and a message, nothing launched, on a bad argument.              */
int dle_conv3d_in_bands(int D, int H, int W, int stride);
int dle_conv3d_in_fwd(const void* x, int64_t ldx, int64_t x_off, const float* scale, const float* shift, const void* w, void* y,
                      int64_t ldy, int64_t y_off, float* part, int N, int D, int H, int W, int C, int Ko, int stride, int relu_in,
                      int relu_out, int dtype, hipStream_t stream);
int dle_instnorm_fold(const float* part, int G, int C, const float* gamma, const float* beta, float eps, float* scale, float* shift,
                      int64_t ld_out, int64_t out_off, int N, hipStream_t stream);
int dle_upsample3d_x2_bands(int D, int H, int W);
int dle_upsample3d_x2_fwd(const void* x, int64_t ldx, int64_t x_off, void* y, int64_t ldy, int64_t y_off, float* part, int N, int D,
                          int H, int W, int C, int dtype, hipStream_t stream);
int dle_nnunet_head_blend_fwd(const void* x, int64_t ldx, const void* w, const float* b, const float* imp, float* out, int K, int C,
                              int Dp, int Hp, int Wp, int Dv, int Hv, int Wv, int d0, int h0, int w0, int dtype, hipStream_t stream);

/* ---- MoFlow molecule generation, the reverse flow (csrc/moflow.hip; reference PyTorch/DrugDiscovery/MoFlow/moflow/model) ------
 * Bond flow (Glow.reverse, glow.py:229; conv_lu == 2, one block).  The squeezed image has G x G = P <= 9 positions, so a 3x3 / pad 1
 * convolution is the dense map [B, P Cin] x [P Cin, P Cout] of its live taps (packed on the host); layers 1 and 2 of a coupling
 * (Conv2d + BatchNorm2d in evaluation mode + ReLU, coupling.py:59-63) run on dle_gemm with the BatchNorm folded into weight and
 * bias in fp32 BEFORE the single rounding of the weight to 16 bits.  The flow state is fp32 [B][P][C], C = 4 fold^2 channels
 * innermost, channel c = (e fold + fy) fold + fx of Block._squeeze (glow.py:152-170); a half is channels [0, C/2) or [C/2, C).
 * dle_mf_squeeze_fwd: z_adj fp32 [B][4][N][N] (row pitch ldz) -> the state and the 16-bit image [B][P][C/2] of half img_half.
 * dle_mf_couple_fwd: the third convolution of AffineCoupling (coupling.py:64) with the rest of Flow.reverse (glow.py:78-84,
 *   coupling.py:86-100, basic.py:92-93) in its epilogue.  w3 [2 M][K], M = P C/2: row j = q C/2 + c holds s of element (q, c), row
 *   M + j its t; b3 fp32 [2 M] likewise; h2 16-bit [B][K] (row pitch ldh).  With a / b the pass-through / updated half (b is the
 *   first half when mask_swap):
 *     s = acc_s + b3[j], t = acc_t + b3[M + j]                        (fp32 MFMA accumulation from 0, then the bias)
 *     out[b half] = (in[b half] * (1 + exp(-s)) - t) / scale - loc,   out[a half] = in[a half] / scale - loc
 *   each operation rounded to fp32 on its own (no contraction, true division); no clamp on exp: an overflow gives that element's
 *   inf / NaN and touches nothing else.  scale, loc fp32 [C].  state_out may be state_in.  img (NULL or 16-bit [B][P][C/2]) = the
 *   rounding of out's half img_half, what the next flow's first layer reads.  Envelope: C/2 % 4 == 0, M % 32 == 0, K % 16 == 0.
 * dle_mf_bond_decide_fwd: MoFlow.reverse (model.py:222-229) in one pass: un-squeeze by index, h = (h + 0.5) * 2 when unshift
 *   (noise_scale == 0), v_e = (h[e,i,j] + h[e,j,i]) / 2 in fp32, and the discretisation as a rule: bit e of mask[b,i,j] is set iff
 *   v_e equals the maximum of the four (ties set several bits, as floor(softmax / max) does); code = the lowest set bit's index
 *   (argmax of the 0/1 tensor).  It differs from the reference only where two softmax values round equal while the logits differ;
 *   a NaN among the four sets no bit for it.  adj01 (NULL or fp32 [B][4][N][N]) = the reference's tensor, h_adj (NULL or fp32
 *   [B][4][N][N]) = the un-squeezed state before the un-shift.
 * dle_mf_atom_reverse_fwd: GlowOnGraph.reverse (glow.py:263-270) in one launch, a workgroup per tile of 32 samples, the N x T states
 *   in LDS across all flows.  Flow i (last to first) updates row r = (i row_stride) % N only (mask_row_size == 1): the graph
 *   convolution of row r (basic.py:187-194) regrouped as g = [sum_n adj[e,r,n] y[n,:] (n != r) for e | deg_e(r) | 0] (fp32 sums in
 *   ascending n, rounded to 16 bits once) times [4 T + 4 -> gnn] weights, then the linear blocks and the last linear, every
 *   BatchNorm2d(n_node) of row r (an affine per flow in evaluation mode) folded into weight and bias in fp32 before the weight's
 *   single rounding; hidden activations are rounded to 16 bits after the ReLU, s and t stay fp32;
 *   y[r,:] = y[r,:] * (1 + exp(-s)) - t, then y[n,:] = y[n,:] / scale[n] - loc[n] for all n (fp32, uncontracted).
 *   w16: per flow (pitch w_stride elements) Wg [D1][KG], W1 [D2][D1], W2 [D3][D2], W3 [32][D3] (rows 0.. = s, 16.. = t), each in MFMA
 *   fragment order [row / 32][k / 16][lane][8]; KG = 4 T + 4 rounded up to 16, D* = the widths rounded up to 32, zero padded.
 *   p32: per flow (pitch p_stride) bg [D1], b1 [D2], b2 [D3], b3 [32], scale [N], loc [N].  mask = dle_mf_bond_decide_fwd's bits.
 *   x fp32 [B][N][T], (x + 0.5) * 2 when unshift.  tile must be 32 (16 and 64 are not built); the grid is min(ceil(B / 32),
 *   max_workgroups or the device's CU count when 0).  Envelope (dle_mf_atom_supported, host only, 1 / 0): one block, one gnn layer,
 *   two linear blocks, mask_row_size 1, N <= 64, T <= 16, widths <= 512, the LDS image within 160 KB.
 * All: no allocation, no synchronisation, graph capturable; -1 and a message, nothing launched, on a bad argument.              */
int dle_mf_squeeze_fwd(const float* z_adj, int64_t ldz, float* state, void* img, int B, int N, int fold, int img_half, int dtype,
                       hipStream_t stream);
int dle_mf_couple_fwd(const void* h2, int64_t ldh, const void* w3, const float* b3, const float* scale, const float* loc,
                      const float* state_in, float* state_out, void* img, int B, int P, int half_channels, int K, int mask_swap,
                      int img_half, int dtype, hipStream_t stream);
int dle_mf_bond_decide_fwd(const float* state, uint8_t* mask, uint8_t* code, float* adj01, float* h_adj, int B, int N, int fold,
                           int unshift, hipStream_t stream);
int dle_mf_atom_supported(int N, int T, int n_block, int n_gnn, int gnn0, int n_lin, int lin0, int lin1, int n_flow,
                          int mask_row_size);
int dle_mf_atom_reverse_fwd(const float* z_x, int64_t ldz, const uint8_t* mask, const void* w16, int64_t w_stride, const float* p32,
                            int64_t p_stride, float* x, int B, int N, int T, int gnn0, int lin0, int lin1, int n_flow, int row_stride,
                            int unshift, int tile, int max_workgroups, int dtype, hipStream_t stream);

/* ---- collectives over librccl.so (csrc/rccl_comm.hip) -------------------------------------------------
 * What the reference reaches through torch.distributed's ProcessGroupNCCL: the gradient all-reduce of the DDP reducer
 * (Classification/ConvNets/image_classification/training.py:78-84), BERT's comm hook (LanguageModeling/BERT/run_pretraining.py:
 * 461-470: `dist.all_reduce(bucket, async_op=True)` behind a pre-division) and DLRM's `dist.all_to_all` of the bottom -> top
 * exchange and its backward (Recommendation/DLRM/dlrm/model/distributed.py:68,95).  RCCL is bound with dlopen at first use (the
 * copy the process already holds, else /opt/rocm/lib); every call is enqueued on the stream the caller names and returns at
 * once; 0 = ok.  The 128-byte unique id of rank 0 travels over the caller's rendezvous (utils/rccl.py: torch.distributed's
 * MASTER_ADDR / MASTER_PORT store).  dtype: DLE_F32 / DLE_F16 / DLE_BF16, 100 = int32, 101 = int64, 102 = uint8.            */
int dle_rccl_available(void);
int dle_rccl_unique_id(void* id128);
int dle_rccl_init(const void* id128, int rank, int world, void** comm_out);          /* ncclCommInitRank on the current device */
int dle_rccl_count(void* comm);                                                       /* ncclCommCount: ranks that joined      */
int dle_rccl_destroy(void* comm);
int dle_rccl_allreduce(void* comm, void* buf, int64_t count, int dtype, int op, hipStream_t stream);   /* op: 0 sum, 2 max, 4 avg */
int dle_rccl_broadcast(void* comm, void* buf, int64_t bytes, int root, hipStream_t stream);
/* all_to_all_single with split lists: peer p gets send_bytes[p] bytes from send + sum(send_bytes[:p]) and delivers recv_bytes[p]
 * bytes at recv + sum(recv_bytes[:p]); one grouped ncclSend / ncclRecv pair per peer; the size arrays are HOST memory.       */
int dle_rccl_alltoallv(void* comm, const void* send, const int64_t* send_bytes, void* recv, const int64_t* recv_bytes, int world,
                       hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLE_MI355X_H */
