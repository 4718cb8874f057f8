// kernels_overlap_sparse.hip — the overlap's key sets as sorted key lists, for batches and stream
// windows whose dense voxel maps do not fit (a return kilometres away makes a key box of 10^12
// voxels).
//
// Same sets as the dense path and as octomap (kernels_overlap.hip): every key of
// computeRayKeys(origin, p) plus p's own key, per cloud, from the same walk (overlap_keys.hpp).
// Here each key is written out as a 64-bit word  cloud << 48 | k0 << 32 | k1 << 16 | k2, the
// words of one side's clouds (OvlKeySide) are sorted together (rocprim radix sort), and:
//   |S_c|      = the distinct words of cloud c (a word differs from its predecessor);
//   |A ∩ B|    = the distinct words of reading p whose key is present under p's group in the
//                reference list (binary search of group << 48 | key).
// The batch has one side, groups then readings, sized exactly after one host read of the key
// total; the stream has a readings' side and a one-cloud reference side per window, each of `cap`
// words, a host bound of the keys the rays can visit (no read-back: the stream stays free of
// host synchronisation); the words past the true total are padding (n_clouds << 48, sorted last,
// never counted). One kernel set serves both.
// Cost: 8 B per ray key written and sorted, where the dense path stores 1 byte per ray key into
// an L2-resident map; it is the fallback, not the default.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "aicp_common.hpp"
#include "kernels.hpp"
#include "overlap_keys.hpp"

namespace aicp {

namespace {

__device__ __forceinline__ const float4* cloud_pts(const OvlCloud& c, const float4* ref, const float4* read) {
  return (c.side ? read : ref) + c.pts_off;
}

__global__ __launch_bounds__(256) void k_spo_count(const uint32_t* __restrict__ blk_cloud,
                                                   const uint32_t* __restrict__ blk_start,
                                                   const OvlCloud* __restrict__ clouds, const float4* __restrict__ ref,
                                                   const float4* __restrict__ read, double res,
                                                   uint32_t* __restrict__ cnt) {
  const OvlCloud& c = clouds[blk_cloud[blockIdx.x]];
  const uint32_t j = blk_start[blockIdx.x] + threadIdx.x;
  if (j >= c.n) return;
  uint32_t k = 0;
  ray_keys(res, c.origin, cloud_pts(c, ref, read)[j], [&](int, int, int) { ++k; });
  cnt[c.slot + j] = k;
}

// est (nullable): a cloud whose words would pass cap reports est[cloud].ovl_err (a host bound
// that was wrong: reported, never written past)
__global__ __launch_bounds__(256) void k_spo_emit(const uint32_t* __restrict__ blk_cloud,
                                                  const uint32_t* __restrict__ blk_start,
                                                  const OvlCloud* __restrict__ clouds, const float4* __restrict__ ref,
                                                  const float4* __restrict__ read, double res,
                                                  const uint64_t* __restrict__ off, uint64_t cap,
                                                  uint64_t* __restrict__ keys, PairState* est) {
  const uint32_t ci = blk_cloud[blockIdx.x];
  const OvlCloud& c = clouds[ci];
  const uint32_t j = blk_start[blockIdx.x] + threadIdx.x;
  if (j >= c.n) return;
  uint64_t o = off[c.slot + j];
  const uint64_t hi = (uint64_t)ci << 48;
  bool over = false;
  ray_keys(res, c.origin, cloud_pts(c, ref, read)[j], [&](int a, int b, int d) {
    if (o < cap)
      keys[o++] = hi | ((uint64_t)a << 32) | ((uint64_t)b << 16) | (uint64_t)d;
    else
      over = true;
  });
  if (over && est) atomicOr(&est[ci].ovl_err, 1);
}

// a cloud's origin written on the device: the reference's by k_seq_ref_points, a debug-mode
// reading's by k_debug_prep
__global__ void k_spo_origin(OvlCloud* c, const double* __restrict__ o) {
  if (threadIdx.x < 3) c->origin[threadIdx.x] = o[threadIdx.x];
}

// words [total, cap) := pad, total = off[n - 1] + cnt[n - 1]
__global__ __launch_bounds__(256) void k_spo_pad(const uint64_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                 uint32_t n, uint64_t cap, uint64_t pad, uint64_t* keys) {
  const uint64_t total = n ? off[n - 1] + cnt[n - 1] : 0;
  for (uint64_t i = total + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap;
       i += (uint64_t)gridDim.x * blockDim.x)
    keys[i] = pad;
}

// distinct words per cloud of a sorted list, padding (cloud n_clouds) left out (wave-aggregated
// atomics: sorted runs share their cloud)
__global__ __launch_bounds__(256) void k_spo_unique(const uint64_t* __restrict__ keys, uint64_t cap,
                                                    uint32_t n_clouds, unsigned long long* __restrict__ per_cloud) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = i < cap;
  const uint64_t k = in ? keys[i] : 0;
  const uint32_t cloud = (uint32_t)(k >> 48);
  const bool uniq = in && cloud < n_clouds && (i == 0 || keys[i - 1] != k);
  const uint32_t c0 = __shfl(cloud, 0, 64);
  if (__all(!in || cloud == c0)) {
    const uint64_t m = __ballot(uniq);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&per_cloud[c0], (unsigned long long)__popcll(m));
  } else if (uniq) {
    atomicAdd(&per_cloud[cloud], 1ull);
  }
}

// |A ∩ B| per reading (clouds first_read .. first_read + n_read - 1 of the list rk): its distinct
// words whose key is in the reference list gk under the reading's group, pd[p].ogroup (the batch:
// gk is rk itself) or 0 without pd (the stream: gk holds the window's one reference)
__global__ __launch_bounds__(256) void k_spo_intersect(const uint64_t* __restrict__ rk, uint64_t cap_r,
                                                       uint32_t first_read, uint32_t n_read,
                                                       const uint64_t* __restrict__ gk, uint64_t cap_g,
                                                       const PairDesc* __restrict__ pd,
                                                       unsigned long long* __restrict__ per_pair) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap_r) return;
  const uint64_t k = rk[i];
  const uint32_t p = (uint32_t)(k >> 48) - first_read;  // (a group's word wraps to a large p)
  if (p >= n_read || (i > 0 && rk[i - 1] == k)) return;
  const uint64_t want = ((uint64_t)(pd ? pd[p].ogroup : 0) << 48) | (k & 0xFFFFFFFFFFFFull);
  uint64_t lo = 0, hi = cap_g;  // first position with gk[pos] >= want
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (gk[mid] < want)
      lo = mid + 1;
    else
      hi = mid;
  }
  if (lo < cap_g && gk[lo] == want) atomicAdd(&per_pair[p], 1ull);
}

// the counts into the states, whichever are given: per_cloud (n_groups groups, then n_pairs
// readings) -> gst[g].ovl_counts[0] and st[p].ovl_counts[1]; per_pair -> st[p].ovl_counts[2]
__global__ void k_spo_counts(int n_groups, int n_pairs, const unsigned long long* __restrict__ per_cloud,
                             const unsigned long long* __restrict__ per_pair, PairState* gst, PairState* st) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (per_cloud && i < n_groups) gst[i].ovl_counts[0] = per_cloud[i];
  if (i < n_pairs) {
    if (per_cloud) st[i].ovl_counts[1] = per_cloud[n_groups + i];
    if (per_pair) st[i].ovl_counts[2] = per_pair[i];
  }
}

__global__ void k_spo_zero(unsigned long long* v, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = 0ull;
}

int key_end_bit(int n_clouds) {
  int b = 1;
  while ((1 << b) <= n_clouds) ++b;
  return 48 + b;
}

void launch_counts(hipStream_t s, int n_groups, int n_pairs, const unsigned long long* per_cloud,
                   const unsigned long long* per_pair, PairState* gst, PairState* st) {
  const int m = n_groups > n_pairs ? n_groups : n_pairs;
  k_spo_counts<<<(m + 63) / 64, 64, 0, s>>>(n_groups, n_pairs, per_cloud, per_pair, gst, st);
}

}  // namespace

size_t ovl_keys_temp_bytes(size_t n_points, size_t cap, int n_clouds) {
  size_t a = 0, b = 0;
  (void)rocprim::exclusive_scan(nullptr, a, (const uint32_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, n_points,
                                rocprim::plus<uint64_t>());
  (void)rocprim::radix_sort_keys(nullptr, b, (const uint64_t*)nullptr, (uint64_t*)nullptr, cap, 0,
                                 key_end_bit(n_clouds));
  return a > b ? a : b;
}

hipError_t launch_ovl_keys_count(hipStream_t s, const OvlKeySide& k, const double* origin0, const float4* ref,
                                 const float4* read, double res) {
  if (origin0) k_spo_origin<<<1, 64, 0, s>>>(k.clouds, origin0);
  if (!k.n_blocks) return hipSuccess;
  k_spo_count<<<k.n_blocks, 256, 0, s>>>(k.blk_cloud, k.blk_start, k.clouds, ref, read, res, k.cnt);
  size_t b = k.temp_bytes;
  return rocprim::exclusive_scan(k.temp, b, k.cnt, k.off, (uint64_t)0, k.n_points, rocprim::plus<uint64_t>(), s);
}

hipError_t launch_ovl_keys_sets(hipStream_t s, const OvlKeySide& k, const float4* ref, const float4* read,
                                double res, PairState* st, int slot) {
  if (k.n_blocks)
    k_spo_emit<<<k.n_blocks, 256, 0, s>>>(k.blk_cloud, k.blk_start, k.clouds, ref, read, res, k.off, k.cap, k.keys0,
                                          st);
  const uint64_t pad = (uint64_t)k.n_clouds << 48;
  const uint64_t pb = (k.cap + 255) / 256;
  if (k.cap && st)
    k_spo_pad<<<(unsigned)(pb < 4096 ? pb : 4096), 256, 0, s>>>(k.off, k.cnt, k.n_points, k.cap, pad, k.keys0);
  k_spo_zero<<<(k.n_clouds + 63) / 64, 64, 0, s>>>(k.per_cloud, k.n_clouds);
  if (k.cap) {
    size_t b = k.temp_bytes;
    const hipError_t e =
        rocprim::radix_sort_keys(k.temp, b, k.keys0, k.keys1, k.cap, 0, key_end_bit(k.n_clouds), s);
    if (e != hipSuccess) return e;
    k_spo_unique<<<(unsigned)pb, 256, 0, s>>>(k.keys1, k.cap, (uint32_t)k.n_clouds, k.per_cloud);
  }
  if (st) launch_counts(s, slot ? 0 : k.n_clouds, slot ? k.n_clouds : 0, k.per_cloud, nullptr, st, st);
  return hipGetLastError();
}

hipError_t launch_ovl_keys(hipStream_t s, const OvlKeySide& k, const double* origin0, const float4* pts,
                           double res, PairState* st, int slot) {
  const hipError_t e = launch_ovl_keys_count(s, k, origin0, pts, pts, res);
  return e != hipSuccess ? e : launch_ovl_keys_sets(s, k, pts, pts, res, st, slot);
}

hipError_t launch_ovl_keys_intersect(hipStream_t s, const OvlKeySide& rd, const OvlKeySide& ref, int first_read,
                                     const PairDesc* pd, unsigned long long* per_pair, PairState* gst,
                                     PairState* st) {
  const int n_read = rd.n_clouds - first_read;
  k_spo_zero<<<(n_read + 63) / 64, 64, 0, s>>>(per_pair, n_read);
  if (rd.cap)
    k_spo_intersect<<<(unsigned)((rd.cap + 255) / 256), 256, 0, s>>>(rd.keys1, rd.cap, (uint32_t)first_read,
                                                                     (uint32_t)n_read, ref.keys1, ref.cap, pd,
                                                                     per_pair);
  launch_counts(s, gst ? first_read : 0, n_read, gst ? rd.per_cloud : nullptr, per_pair, gst, st);
  return hipGetLastError();
}

}  // namespace aicp
