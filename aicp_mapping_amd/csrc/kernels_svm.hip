// kernels_svm.hip — the failure-prediction classifier (aicp_core/src/classification/svm.cpp:
// cv::ml::SVM::predict(sample, RAW_OUTPUT) of a two-class C_SVC with a POLY kernel, then the
// logistic of svm.cpp:82) and the gate App derives from it (app.cpp:243-245, 362).
//
// One wave per sample, four samples per workgroup. The model's decision-function entries (support
// vector gathered by the file's index, alpha) are staged in LDS once per workgroup. Lane l takes
// entries l, l + 64, ... in index order and accumulates alpha * K in double; a fixed xor butterfly
// joins the 64 partial sums (a + b == b + a, so every lane holds the same bits) and -rho is added
// last. No atomics: a sample's result depends on the sample and the model alone, whatever the batch
// it is in. The float products, the float base and the float K are the roundings OpenCV's float
// kernel rows make; -ffp-contract=off keeps the compiler from fusing any of them.
#include <hip/hip_runtime.h>

#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {

namespace {

constexpr int kSvmThreads = 256;
constexpr int kSvmWaves = kSvmThreads / 64;

__global__ __launch_bounds__(kSvmThreads) void k_svm_predict(uint32_t n, SvmParams prm,
                                                             const SvmEntry* __restrict__ entries,
                                                             const float* __restrict__ samples,
                                                             float* __restrict__ raw, double* __restrict__ risk,
                                                             int32_t* __restrict__ gate, float* __restrict__ ratio) {
  extern __shared__ SvmEntry s_e[];
  for (uint32_t j = threadIdx.x; j < prm.count; j += kSvmThreads) s_e[j] = entries[j];
  __syncthreads();
  const uint32_t i = blockIdx.x * kSvmWaves + (threadIdx.x >> 6);
  if (i >= n) return;  // (whole waves: nothing below synchronises across waves)
  const uint32_t lane = threadIdx.x & 63u;
  const float x0 = samples[2 * (size_t)i], x1 = samples[2 * (size_t)i + 1];
  double acc = 0.0;
  for (uint32_t j = lane; j < prm.count; j += 64) {
    const SvmEntry e = s_e[j];
    const float p0 = e.v0 * x0, p1 = e.v1 * x1;
    const double s = (double)p0 + (double)p1;
    const float base = (float)(s * prm.gamma + prm.coef0);
    const float K = (float)pow((double)base, prm.degree);
    acc += e.alpha * (double)K;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane != 0) return;
  const float r = (float)(acc - prm.rho);
  const double p = 1.0 - 1.0 / (1.0 + exp(-(double)r));
  if (raw) raw[i] = r;
  risk[i] = p;
  if (gate) gate[i] = !(p <= prm.threshold) ? 1 : 0;  // a NaN risk gates (app.cpp:244, 363)
  if (ratio) ratio[i] = autotune_ratio_fast(x0);      // app.cpp:197-204
}

}  // namespace

void launch_svm_predict(hipStream_t s, uint32_t n, const SvmParams& prm, const SvmEntry* entries,
                        const float* samples, float* raw, double* risk, int32_t* gate, float* ratio) {
  if (n == 0) return;
  const uint32_t blocks = (n + kSvmWaves - 1) / kSvmWaves;
  hipLaunchKernelGGL(k_svm_predict, dim3(blocks), dim3(kSvmThreads), (size_t)prm.count * sizeof(SvmEntry), s, n, prm,
                     entries, samples, raw, risk, gate, ratio);
}

}  // namespace aicp
