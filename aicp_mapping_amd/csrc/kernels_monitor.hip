// Registration quality monitor (aicp_core/src/utils/icpMonitor.cpp): hausdorffDistance (:12-81),
// distancesKNN (:89-138) and pairedPointsMeanDistance (:146-231) from the squared distances of the
// 1-NN launches (k_mon_nn, kernels_icp.hip) and the limits of the exact select (k_sel_*).
//
//   k_mon_transform   out = T * cloud for every pair of a batch, in k_transform's arithmetic
//   k_mon_stage       the resident front end: a reference and a reading that lie on the device go
//                     into the point arena, the reading moved by a correction in device memory
//   k_mon_reduce      one pass over the squared distances, a flat grid over chunk slots (segments
//                     differ in size by orders of magnitude): the maximum, distancesKNN's valid
//                     count and sum and, under the select's limit, the kept count and sum
//   k_mon_finish      per pair: chunk partials added in index order, the square roots, the means
//
// The fixed-order rule: no floating-point atomics. The two sums are fp64, taken in
// slabs of 256 values with a fixed binary tree in LDS (a short slab padded with zeros), a chunk's 16
// slabs added in index order by its workgroup and a segment's chunks in index order by
// k_mon_finish. The maximum (on the bits of the non-negative floats) and the counts are integers:
// atomics in any order give the same value.
#include <hip/hip_runtime.h>

#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {
namespace {

constexpr int kMonThreads = 256;
constexpr uint32_t kMonInf = 0x7f800000u;

// correctly rounded float square root: the double one rounded to float (53 >= 2 * 24 + 2 bits),
// bit-identical to sqrtf on the host (see kernels_prefilter.hip)
__device__ __forceinline__ float mon_sqrt(float x) { return (float)sqrt((double)x); }

__global__ __launch_bounds__(kMonThreads) void k_mon_transform(BlockMap m, const uint2* __restrict__ xf,
                                                               const float* __restrict__ T, float4* pts) {
  const int pair = m.pair[blockIdx.x];
  const uint32_t j = m.start[blockIdx.x] + threadIdx.x;
  const uint2 c = xf[pair];
  if (j >= c.y) return;
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = T[16 * (size_t)pair + k];
  const float4 p = pts[c.x + j];
  float o[3];
  apply4(Tl, p.x, p.y, p.z, o);
  pts[c.x + j] = make_float4(o[0], o[1], o[2], 1.f);
}

// The resident front end (monitor.cpp: monitor_resident): a reference and a reading that lie on the
// device already go into the point arena, the reference first, as the uploaded form lays them out.
// One thread per point, one 128-bit load and one 128-bit store: a reference point is copied as it
// is, a point of the reading is moved by the correction the registration left in device memory
// (every thread reads the same 16 floats: the loads are uniform), in k_mon_transform's and
// k_transform's expression (apply4, no FMA contraction, w = 1). No LDS, no atomics. pts aliases
// neither input.
__global__ __launch_bounds__(kMonThreads) void k_mon_stage(uint32_t n_ref, uint32_t n_read,
                                                           const float4* __restrict__ ref,
                                                           const float4* __restrict__ read,
                                                           const float* __restrict__ T, float4* __restrict__ pts) {
  const uint32_t i = blockIdx.x * kMonThreads + threadIdx.x;
  if (i < n_ref) {
    pts[i] = ref[i];
    return;
  }
  const uint32_t j = i - n_ref;
  if (j >= n_read) return;
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = T[k];
  const float4 p = read[j];
  float o[3];
  apply4(Tl, p.x, p.y, p.z, o);
  pts[i] = make_float4(o[0], o[1], o[2], 1.f);
}

// Behind a tree build whose levels were planned (nothing read back, so the host cannot refuse a
// broken tree before the searches are enqueued): when the build left an error in its control block
// (a tree deeper than the search stacks among them), every segment of the 1-NN launches loses its
// queries, so that k_mon_nn finds only padding slots and no search enters the tree. The host reads
// the same control block after the call and drops the result.
__global__ void k_mon_guard(const TreeCtl* __restrict__ ctl, MonSeg* a, int na, MonSeg* b, int nb) {
  if (!ctl->error) return;
  for (int i = threadIdx.x; i < na; i += blockDim.x) a[i].nq = 0;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) b[i].nq = 0;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kMonThreads) void k_mon_reduce(BlockMap m, const MonRed* __restrict__ red,
                                                            const float* __restrict__ d2,
                                                            const PairState* __restrict__ lim_st, double max_accepted,
                                                            MonAcc* acc, double* __restrict__ partial,
                                                            float* __restrict__ dist) {
  __shared__ double sh[2][kMonThreads];
  const MonRed r = red[m.pair[blockIdx.x]];
  const uint32_t t = threadIdx.x, first = m.start[blockIdx.x];
  const uint32_t end = min(r.n, first + kMonChunk);
  bool gated = false;
  float limit = 0.f;
  if (r.lim >= 0 && lim_st[r.lim].status == 0) {  // (a select that found no finite distance keeps nothing)
    gated = true;
    limit = lim_st[r.lim].limit;
  }
  double sum_v = 0.0, sum_k = 0.0;  // thread 0's: the chunk's slabs in index order
  uint32_t mx = 0, nv = 0, nk = 0;
  for (uint32_t s0 = first; s0 < end; s0 += kMonThreads) {
    double v = 0.0, k = 0.0;
    const uint32_t j = s0 + t;
    if (j < end) {
      const float x = d2[r.d2_off + j];
      const uint32_t bits = __float_as_uint(x);
      const float d = mon_sqrt(x);
      if (dist) dist[r.d2_off + j] = d;
      if (bits != kMonInf) mx = max(mx, bits);
      if (r.knn && (double)d <= max_accepted) {
        v = (double)d;
        ++nv;
      }
      if (gated && x <= limit) {
        k = (double)d;
        ++nk;
      }
    }
    sh[0][t] = v;
    sh[1][t] = k;
    __syncthreads();
    for (uint32_t h = kMonThreads / 2; h > 0; h >>= 1) {
      if (t < h) {
        sh[0][t] += sh[0][t + h];
        sh[1][t] += sh[1][t + h];
      }
      __syncthreads();
    }
    if (t == 0) {
      sum_v += sh[0][0];
      sum_k += sh[1][0];
    }
    __syncthreads();
  }
  if (t == 0) {
    partial[2 * (size_t)blockIdx.x] = sum_v;
    partial[2 * (size_t)blockIdx.x + 1] = sum_k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
  const unsigned long long wv = wave_sum(nv), wk = wave_sum(nk);
  if ((t & 63) == 0) {
    MonAcc& a = acc[r.acc];
    if (mx) atomicMax(&a.max_bits, mx);
    if (wv) atomicAdd(&a.n_valid, wv);
    if (wk) atomicAdd(&a.kept, wk);
  }
}

__device__ double mon_chunk_sum(const MonRed& r, const double* __restrict__ partial, int which) {
  const uint32_t chunks = (r.n + kMonChunk - 1) / kMonChunk;
  double a = 0.0;
  for (uint32_t k = 0; k < chunks; ++k) a += partial[2 * (size_t)(r.slot0 + k) + which];
  return a;
}

__global__ void k_mon_finish(int n_pairs, const MonPair* __restrict__ mp, const MonRed* __restrict__ red,
                             const MonAcc* __restrict__ acc, const double* __restrict__ partial,
                             const PairState* __restrict__ sel_q, const PairState* __restrict__ sel_p,
                             MonOut* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const MonPair q = mp[p];
  MonOut o{};
  for (int dir = 0; dir < 2; ++dir) {
    o.max_d2[dir] = __uint_as_float(acc[red[q.red[dir]].acc].max_bits);
    o.quantile_d2[dir] = sel_q[q.sel_q[dir]].limit;
    o.pad |= sel_q[q.sel_q[dir]].status;  // a direction without a finite distance: the host reports it
  }
  o.hausdorff = mon_sqrt(fmaxf(o.max_d2[0], o.max_d2[1]));
  o.hausdorff_quantile = mon_sqrt(fmaxf(o.quantile_d2[0], o.quantile_d2[1]));
  const float qnan = __uint_as_float(0x7fc00000u);
  {
    const MonRed& r = red[q.red[0]];
    const unsigned long long n = acc[r.acc].n_valid;
    o.knn_valid = n;
    o.knn_mean_dist = n ? (float)(mon_chunk_sum(r, partial, 0) / (double)n) : qnan;  // the reference: 0 / 0
  }
  o.paired_mean_dist = qnan;
  o.paired_limit_d2 = qnan;
  if (q.sel_p >= 0 && q.red[2] >= 0 && sel_p[q.sel_p].status == 0) {
    const MonRed& r = red[q.red[2]];
    const unsigned long long n = acc[r.acc].kept;
    o.paired_kept = n;
    o.paired_limit_d2 = sel_p[q.sel_p].limit;
    if (n) o.paired_mean_dist = (float)(mon_chunk_sum(r, partial, 1) / (double)n);
  }
  out[p] = o;
}

}  // namespace

void launch_mon_transform(hipStream_t s, BlockMap m, const uint2* xf, const float* T, float4* pts) {
  if (m.n_blocks) k_mon_transform<<<m.n_blocks, kMonThreads, 0, s>>>(m, xf, T, pts);
}
void launch_mon_stage(hipStream_t s, uint32_t n_ref, uint32_t n_read, const float4* ref, const float4* read,
                      const float* T, float4* pts) {
  const uint64_t n = (uint64_t)n_ref + n_read;
  if (n) k_mon_stage<<<(unsigned)((n + kMonThreads - 1) / kMonThreads), kMonThreads, 0, s>>>(n_ref, n_read, ref, read, T, pts);
}
void launch_mon_guard(hipStream_t s, const TreeCtl* ctl, MonSeg* a, int na, MonSeg* b, int nb) {
  k_mon_guard<<<1, 64, 0, s>>>(ctl, a, na, b, nb);
}
void launch_mon_reduce(hipStream_t s, BlockMap m, const MonRed* red, const float* d2, const PairState* lim_st,
                       double max_accepted, MonAcc* acc, double* partial, float* dist) {
  if (m.n_blocks) k_mon_reduce<<<m.n_blocks, kMonThreads, 0, s>>>(m, red, d2, lim_st, max_accepted, acc, partial, dist);
}
void launch_mon_finish(hipStream_t s, int n_pairs, const MonPair* mp, const MonRed* red, const MonAcc* acc,
                       const double* partial, const PairState* sel_q, const PairState* sel_p, MonOut* out) {
  k_mon_finish<<<(n_pairs + 63) / 64, 64, 0, s>>>(n_pairs, mp, red, acc, partial, sel_q, sel_p, out);
}

}  // namespace aicp
