// Standalone timing harness for the BatchNorm passes of the ResNet-50 step (no torch): HIP-event timings of
// dle_bn_bwd_reduce / dle_bn_bwd_apply / dle_bn_fwd_apply (and dle_bn_fwd_stats) on the layer shapes of batch 256.
//   bn_bench [repeats [dtype [mask_kind]]]     dtype 1 = fp16, 2 = bf16 (default); ReLU mask 0 = none, 1 = bits (default), 2 = saved output
// Each repeat prints one line per shape and the per-step totals; repeats show the run-to-run spread.  Build (from this folder):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 bn_bench.cpp -L../../deeplearningexamples_amd/lib -ldle_mi355x \
//         -Wl,-rpath,'$ORIGIN/../../../deeplearningexamples_amd/lib' -o bin/bn_bench
// To time another build of the library (tools/build_lib_at.sh), put it first on LD_LIBRARY_PATH as libdle_mi355x.so.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

extern "C" {
int64_t dle_bn_workspace_bytes(int64_t M, int C);
int dle_bn_fwd_stats(const void* x, int64_t M, int C, float eps, float momentum, float* mean, float* rstd, float* running_mean,
                     float* running_var, void* workspace, int64_t workspace_bytes, int dtype, hipStream_t stream);
int dle_bn_fwd_apply(const void* x, const void* residual, void* y, void* relu_mask, const float* mean, const float* rstd,
                     const float* gamma, const float* beta, int64_t M, int C, int relu, int dtype, hipStream_t stream);
int dle_bn_bwd_reduce(const void* dy, const void* y, const void* relu_mask, const void* x, const float* mean,
                      const float* rstd, float* dgamma, float* dbeta, int64_t M, int C, int accumulate, void* workspace,
                      int64_t workspace_bytes, int dtype, hipStream_t stream);
int dle_bn_bwd_apply(const void* dy, const void* y, const void* relu_mask, const void* x, void* dx, void* g_out,
                     const float* mean, const float* rstd, const float* gamma, const float* dgamma, const float* dbeta,
                     int64_t M, int C, int dtype, hipStream_t stream);
const char* dle_last_error(void);
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)

template <class F> static float timeit(F f, int iters) {
  hipEvent_t s, e; CK(hipEventCreate(&s)); CK(hipEventCreate(&e));
  for (int i = 0; i < 3; ++i) f();
  CK(hipEventRecord(s));
  for (int i = 0; i < iters; ++i) f();
  CK(hipEventRecord(e)); CK(hipEventSynchronize(e));
  float ms; CK(hipEventElapsedTime(&ms, s, e));
  return ms / iters * 1e3f;
}

int main(int argc, char** argv) {
  struct Sh { long long M; int C; int calls; };
  const Sh shapes[] = {{802816, 256, 4}, {802816, 64, 6}, {200704, 512, 5}, {200704, 128, 7}, {50176, 1024, 7},
                       {50176, 256, 11}, {12544, 2048, 4}, {12544, 512, 5}, {3211264, 64, 1}};
  const size_t maxe = 802816ULL * 256;
  uint16_t *x, *dy, *dx, *g;
  unsigned char* mask;
  float *mean, *rstd, *gamma, *dgamma, *dbeta, *ws;
  CK(hipMalloc(&x, maxe * 2)); CK(hipMalloc(&dy, maxe * 2)); CK(hipMalloc(&dx, maxe * 2)); CK(hipMalloc(&g, maxe * 2));
  CK(hipMalloc(&mask, maxe / 8));
  CK(hipMemset(x, 0x3c, maxe * 2)); CK(hipMemset(dy, 0x3b, maxe * 2)); CK(hipMemset(mask, 0xa5, maxe / 8));
  CK(hipMalloc(&mean, 4096 * 4)); CK(hipMalloc(&rstd, 4096 * 4)); CK(hipMalloc(&gamma, 4096 * 4));
  CK(hipMalloc(&dgamma, 4096 * 4)); CK(hipMalloc(&dbeta, 4096 * 4));
  CK(hipMemset(mean, 0, 4096 * 4)); CK(hipMemset(rstd, 0, 4096 * 4)); CK(hipMemset(gamma, 0, 4096 * 4));
  const size_t wsb = 64ULL << 20;
  CK(hipMalloc(&ws, wsb));
  const int repeats = argc > 1 ? atoi(argv[1]) : 1, dt = argc > 2 ? atoi(argv[2]) : 2, mk = argc > 3 ? atoi(argv[3]) : 1;
  const void* ysave = mk == 2 ? x : nullptr;            // (any 16-bit buffer serves as the saved output)
  const void* bits = mk == 1 ? mask : nullptr;
  for (int rep = 0; rep < repeats; ++rep) {
    double tot_red = 0, tot_app = 0, tot_fwd = 0, tot_st = 0;
    for (const Sh& s : shapes) {
      const double bytes = (double)s.M * s.C * 2;
      const float t_red = timeit([&] { if (dle_bn_bwd_reduce(dy, ysave, bits, x, mean, rstd, dgamma, dbeta, s.M, s.C, 0, ws, wsb, dt, 0)) { printf("%s\n", dle_last_error()); exit(3); } }, 20);
      const float t_app = timeit([&] { dle_bn_bwd_apply(dy, ysave, bits, x, dx, s.C >= 256 ? g : nullptr, mean, rstd, gamma, dgamma, dbeta, s.M, s.C, dt, 0); }, 20);
      const float t_fwd = timeit([&] { dle_bn_fwd_apply(x, s.C >= 256 ? dy : nullptr, dx, mask, mean, rstd, gamma, dbeta, s.M, s.C, 1, dt, 0); }, 20);
      const float t_st = timeit([&] { dle_bn_fwd_stats(x, s.M, s.C, 1e-5f, 0.1f, dgamma, dbeta, nullptr, nullptr, ws, wsb, dt, 0); }, 20);
      printf("M %8lld C %5d : reduce+finish %7.1f us %5.2f TB/s | bwd_apply %7.1f us %5.2f TB/s | fwd_apply %7.1f us %5.2f TB/s | fwd_stats %7.1f us\n",
             s.M, s.C, t_red, 2.0625 * bytes / t_red / 1e6, t_app, (s.C >= 256 ? 4.0625 : 3.0625) * bytes / t_app / 1e6,
             t_fwd, (s.C >= 256 ? 3.0625 : 2.0625) * bytes / t_fwd / 1e6, t_st);
      tot_red += t_red * s.calls; tot_app += t_app * s.calls; tot_fwd += t_fwd * s.calls; tot_st += t_st * s.calls;
    }
    printf("== repeat %d dtype %d mask %d: per step reduce %.2f ms  bwd_apply %.2f ms  fwd_apply %.2f ms  (fwd_stats %.2f ms)\n", rep, dt, mk,
           tot_red / 1e3, tot_app / 1e3, tot_fwd / 1e3, tot_st / 1e3);
  }
  return 0;
}
