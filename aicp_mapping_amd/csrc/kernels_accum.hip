// kernels_accum.hip — one lidar sweep appended to a device-resident raw reading:
// VelodyneAccumulatorROS::processLidar (aicp_ros/src/velodyne_accumulator.cpp:58-66), i.e.
//   getPointsInOrientedBox(sweep, -30, 30, Identity)       crop_keep (kernels.hpp), identity frame
//   pcl::transformPointCloud(sweep, offset, quaternion)     apply4, float, no FMA (as k_transform)
//   accumulated_point_cloud_ += point_cloud_                kept points at their rank behind the tail
//
// Two launches per sweep, order-preserving like the crop:
//   k_accum_count    one 1024-point tile per block: keep flags -> per-tile count
//   k_accum_scatter  every block first sums the counts of the tiles before it (a sweep has a few
//                    dozen tiles, so that is a few dozen words per block and saves the crop's
//                    single-block scan launch), then the crop's ballot / LDS prefix, 4 rounds per
//                    tile in index order; a kept point is moved on its way out.
// The tail is an array of running totals on the device: sweep j starts at tails[j] and the last
// block of its scatter writes tails[j + 1], so the host never learns a count while it pushes, no
// atomic is needed and no workgroup waits for another.
// Algorithmic bytes: 2 x 12|16 B per input point (flags recomputed instead of stored) + 16 B per
// kept point + 4 B per tile written and (tiles - 1) / 2 x 4 B per tile read.
#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {
namespace {

constexpr int kAccThreads = 256;
constexpr int kAccTile = 1024;  // 4 rounds of 256 (crop_tiles)

// row i of the staged sweep: a row of 16 bytes is one 128-bit load, a row of 12 three 32-bit loads
__device__ __forceinline__ float4 accum_row(const float* __restrict__ rows, int stride_w, int i) {
  if (stride_w == 4) return reinterpret_cast<const float4*>(rows)[i];
  const float* p = rows + (size_t)i * (size_t)stride_w;
  return make_float4(p[0], p[1], p[2], 1.f);
}

__global__ __launch_bounds__(kAccThreads) void k_accum_count(int n, const float* __restrict__ rows, int stride_w,
                                                             CropBoxArgs a, uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wsum[kAccThreads / 64];
  const int base = blockIdx.x * kAccTile;
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < kAccTile / kAccThreads; ++r) {
    const int i = base + r * kAccThreads + threadIdx.x;
    if (i < n && crop_keep(a, accum_row(rows, stride_w, i))) ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kAccThreads) void k_accum_scatter(int n, const float* __restrict__ rows, int stride_w,
                                                               AccumSweep a, const uint32_t* __restrict__ tile_cnt,
                                                               uint32_t* tails, int j, float4* __restrict__ out,
                                                               uint32_t cap) {
  __shared__ uint32_t wpre[kAccThreads / 64];
  __shared__ uint32_t wcnt[kAccThreads / 64];
  const int base = blockIdx.x * kAccTile;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  // kept points of the tiles before this one
  uint32_t c = 0;
  for (int t = threadIdx.x; t < (int)blockIdx.x; t += kAccThreads) c += tile_cnt[t];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) wpre[w] = c;
  __syncthreads();
  uint32_t run = tails[j] + (wpre[0] + wpre[1] + wpre[2] + wpre[3]);
#pragma unroll 1
  for (int r = 0; r < kAccTile / kAccThreads; ++r) {
    const int i = base + r * kAccThreads + threadIdx.x;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool keep = false;
    if (i < n) {
      p = accum_row(rows, stride_w, i);
      keep = crop_keep(a.box, p);
    }
    const uint64_t m = __ballot(keep);
    const uint32_t below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t wb = run;
    for (int q = 0; q < w; ++q) wb += wcnt[q];
    const uint32_t at = wb + below;
    if (keep && at < cap) {
      float q[3];
      apply4(a.T, p.x, p.y, p.z, q);
      out[at] = make_float4(q[0], q[1], q[2], 1.f);
    }
    run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
  // the last tile's end is the sweep's: the next sweep's start
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) tails[j + 1] = run;
}

}  // namespace

void launch_accum_sweep(hipStream_t s, int n, const void* rows, size_t stride, const AccumSweep& a, uint32_t* tile_cnt,
                        uint32_t* tails, int j, float4* out, uint32_t cap) {
  const int tiles = (n + kAccTile - 1) / kAccTile;
  const int sw = (int)(stride / 4);
  if (tiles)
    k_accum_count<<<tiles, kAccThreads, 0, s>>>(n, (const float*)rows, sw, a.box, tile_cnt);
  // (an empty sweep: one block that only copies the tail forward)
  k_accum_scatter<<<tiles ? tiles : 1, kAccThreads, 0, s>>>(n, (const float*)rows, sw, a, tile_cnt, tails, j, out, cap);
}

}  // namespace aicp
