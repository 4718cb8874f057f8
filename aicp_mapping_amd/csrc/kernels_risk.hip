// Alignment-risk features (App::computeAlignmentRisk, aicp_core/src/registration/app.cpp:143-185):
// overlapFilter (aicp_core/src/utils/filteringUtils.cpp:111-193) and the part of
// alignabilityFilter (:196-430, helpers :432-576) between the two pre-filters and the result.
//
//   k_fov_count / k_fov_scatter   FOV filter of one cloud against the other pose: order-preserving
//                     compaction like the crop (count -> the crop's tile scan -> scatter)
//   k_risk_gather     pre-filter results -> 8 floats per sampled point + cluster labels
//   k_risk_keys / k_risk_segs   (label, index) sort keys; segment bounds of the sorted list
//   k_risk_moments    fp64 moments of every cluster in a fixed order: slabs of 256 points in
//                     sampled-cloud order, a fixed tree inside a slab, a chunk's 16 slabs added in
//                     index order by its workgroup
//   k_risk_frame      per cluster: chunks added in index order, the axes of the oriented box (getOBB)
//   k_risk_extents / k_risk_box   extents in that frame (integer-encoded atomic min / max), the
//                     box and its CropBox frame
//   k_risk_counts     points of one cloud in the boxes of the other: boxes staged in LDS in tiles
//                     of 64, integer tallies in an LDS histogram when (tile x clusters) fits
//   k_risk_match      one workgroup: the sequential matching of :236-286 and the PCA of the
//                     matched normals
// No floating-point atomics anywhere: every sum has one order, whatever the grid.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {
namespace {

constexpr int kRiskThreads = 256;
constexpr int kFovTile = 1024;  // 4 rounds of 256
constexpr int kBoxTile = 64;    // boxes staged in LDS per round
constexpr int kHistWords = 8192;  // LDS histogram: kBoxTile x clusters words when it fits

inline unsigned blocks_for(uint32_t n) { return (n + 255u) / 256u; }

// ---- FOV filter ----------------------------------------------------------------------------
struct FovPoint {
  bool keep;
  float gx, gy, gz;
};

__device__ __forceinline__ FovPoint fov_point(const FovArgs& a, float4 p) {
  float q[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* m = a.pinv + 4 * r;
    const double v = __dadd_rn(
        __dadd_rn(__dadd_rn(__dmul_rn(m[0], (double)p.x), __dmul_rn(m[1], (double)p.y)), __dmul_rn(m[2], (double)p.z)),
        m[3]);
    q[r] = (float)v;
  }
  const double qx = q[0], qy = q[1], qz = q[2];
  const double r = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(qx, qx), __dmul_rn(qy, qy)), __dmul_rn(qz, qz)));
  const double theta = atan2(qy, qx) * 180.0 / M_PI;
  FovPoint o;
  o.keep = (theta < a.thresh && theta > -a.thresh) && r < a.range;
  const float* R = a.R;
  o.gx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], q[0]), __fmul_rn(R[1], q[1])), __fmul_rn(R[2], q[2])), a.t[0]);
  o.gy = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3], q[0]), __fmul_rn(R[4], q[1])), __fmul_rn(R[5], q[2])), a.t[1]);
  o.gz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[6], q[0]), __fmul_rn(R[7], q[1])), __fmul_rn(R[8], q[2])), a.t[2]);
  return o;
}

__global__ __launch_bounds__(kRiskThreads) void k_fov_count(uint32_t n, FovArgs a, const float4* __restrict__ pts,
                                                            uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wsum[kRiskThreads / 64];
  const uint32_t base = blockIdx.x * kFovTile;
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < kFovTile / kRiskThreads; ++r) {
    const uint32_t i = base + r * kRiskThreads + threadIdx.x;
    if (i < n && fov_point(a, pts[i]).keep) ++c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kRiskThreads) void k_fov_scatter(uint32_t n, FovArgs a, const float4* __restrict__ pts,
                                                              const uint32_t* __restrict__ tile_off,
                                                              float4* __restrict__ out) {
  __shared__ uint32_t wcnt[kRiskThreads / 64];
  const uint32_t base = blockIdx.x * kFovTile;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t run = tile_off[blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < kFovTile / kRiskThreads; ++r) {
    const uint32_t i = base + r * kRiskThreads + threadIdx.x;
    FovPoint f;
    f.keep = false;
    f.gx = f.gy = f.gz = 0.f;
    if (i < n) f = fov_point(a, pts[i]);
    const uint64_t m = __ballot(f.keep);
    const uint32_t below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t wb = run;
    for (int q = 0; q < w; ++q) wb += wcnt[q];
    if (f.keep) out[wb + below] = make_float4(f.gx, f.gy, f.gz, 1.f);  // (wb + below < kept total <= n)
    run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
}

// ---- clusters ------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_risk_gather(uint32_t V, const float4* __restrict__ sampled,
                                                     const float4* __restrict__ nrm, const uint32_t* __restrict__ inv,
                                                     const int32_t* __restrict__ cluster_of, float* __restrict__ s8,
                                                     int32_t* __restrict__ lab) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= V) return;
  const float4 p = sampled[i];
  const float4 nb = nrm[inv[i]];
  float4* o = (float4*)(s8 + 8 * (size_t)i);
  o[0] = make_float4(p.x, p.y, p.z, nb.w);
  o[1] = make_float4(nb.x, nb.y, nb.z, 0.f);
  lab[i] = cluster_of[i];
}

// sort keys: the cluster, or all ones for a point of no cluster (label < 0 or >= nc)
__global__ __launch_bounds__(256) void k_risk_keys(uint32_t V, uint32_t nc, const int32_t* __restrict__ lab,
                                                   uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= V) return;
  const int32_t l = lab[i];
  keys[i] = (l >= 0 && (uint32_t)l < nc) ? (uint32_t)l : 0xFFFFFFFFu;
  vals[i] = i;
}

// seg[c] = first position of the sorted keys that is >= c, c in [0, nc]
__global__ __launch_bounds__(256) void k_risk_segs(uint32_t V, uint32_t nc, const uint32_t* __restrict__ keys,
                                                   uint32_t* __restrict__ seg) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c > nc) return;
  uint32_t lo = 0, hi = V;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  seg[c] = lo;
}

__device__ __forceinline__ void risk_fix_sign(double* ax) {
  int big = 0;
  for (int k = 1; k < 3; ++k)
    if (fabs(ax[k]) > fabs(ax[big])) big = k;
  if (ax[big] < 0)
    for (int k = 0; k < 3; ++k) ax[k] = -ax[k];
}

constexpr int kMomVals = 18;  // S(p - p0) 3, S(p - p0)(p - p0)^T 6, S n 3, S n n^T 6
constexpr int kChunkSlabs = 16;  // slabs of kRiskThreads points per workgroup of the moment / extent passes
constexpr uint32_t kChunk = kChunkSlabs * kRiskThreads;

// order-preserving bits of a double, for integer atomic min / max
__device__ __forceinline__ unsigned long long risk_enc(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double risk_dec(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// Slot s of the flat grid of the moment / extent passes -> (cluster, chunk). Cluster c owns the
// slots from seg[c] / kChunk + c on, one per chunk of kChunk points; the ranges do not overlap,
// and V / kChunk + nc + 1 slots hold them all. False for a slot in a gap.
__device__ __forceinline__ bool risk_slot(const uint32_t* __restrict__ seg, uint32_t nc, uint32_t s, uint32_t* c_out,
                                          uint32_t* k_out) {
  uint32_t lo = 0, hi = nc;  // the last cluster whose first slot is <= s
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seg[mid] / kChunk + mid <= s) lo = mid;
    else hi = mid;
  }
  const uint32_t off = seg[lo] / kChunk + lo;
  if (s < off) return false;
  const uint32_t cnt = seg[lo + 1] - seg[lo], k = s - off;
  if ((uint64_t)k * kChunk >= cnt) return false;
  *c_out = lo;
  *k_out = k;
  return true;
}

// Chunk partials of the moments: the workgroup of a slot sums slabs [16 chunk, 16 chunk + 16) of
// the cluster's points (sampled-cloud order): a fixed binary tree in LDS inside a slab (a short
// slab padded with zeros), the chunk's slabs added in index order. The moments are taken about the
// cluster's first point p0 (a fixed choice) to keep the covariance free of cancellation.
__global__ __launch_bounds__(kRiskThreads) void k_risk_moments(uint32_t nc, const float* __restrict__ s8,
                                                               const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ seg,
                                                               double* __restrict__ partial) {
  __shared__ double sh[kMomVals][kRiskThreads];
  __shared__ double acc[kMomVals];
  uint32_t c, chunk;
  if (!risk_slot(seg, nc, blockIdx.x, &c, &chunk)) return;  // (the whole workgroup)
  const uint32_t b = seg[c], e = seg[c + 1], t = threadIdx.x;
  const uint64_t first = (uint64_t)b + (uint64_t)chunk * kChunk;
  const uint32_t end = (uint32_t)min((uint64_t)e, first + kChunk);
  if (t < kMomVals) acc[t] = 0.0;
  const float* q0 = s8 + 8 * (size_t)idx[b];
  const double p0[3] = {q0[0], q0[1], q0[2]};
  __syncthreads();
  for (uint32_t s0 = (uint32_t)first; s0 < end; s0 += kRiskThreads) {
    double v[kMomVals];
#pragma unroll
    for (int k = 0; k < kMomVals; ++k) v[k] = 0.0;
    if (s0 + t < end) {
      const float4* q = (const float4*)(s8 + 8 * (size_t)idx[s0 + t]);
      const float4 P = q[0], N = q[1];
      const double x = (double)P.x - p0[0], y = (double)P.y - p0[1], z = (double)P.z - p0[2];
      const double nx = N.x, ny = N.y, nz = N.z;
      v[0] = x, v[1] = y, v[2] = z;
      v[3] = x * x, v[4] = x * y, v[5] = x * z, v[6] = y * y, v[7] = y * z, v[8] = z * z;
      v[9] = nx, v[10] = ny, v[11] = nz;
      v[12] = nx * nx, v[13] = nx * ny, v[14] = nx * nz, v[15] = ny * ny, v[16] = ny * nz, v[17] = nz * nz;
    }
#pragma unroll
    for (int k = 0; k < kMomVals; ++k) sh[k][t] = v[k];
    __syncthreads();
    for (uint32_t h = kRiskThreads / 2; h > 0; h >>= 1) {
      if (t < h) {
#pragma unroll
        for (int k = 0; k < kMomVals; ++k) sh[k][t] += sh[k][t + h];
      }
      __syncthreads();
    }
    if (t < kMomVals) acc[t] += sh[t][0];
    __syncthreads();
  }
  if (t < kMomVals) partial[(size_t)blockIdx.x * kMomVals + t] = acc[t];
}

// One wave per cluster: the chunk partials added in index order, then the box frame (getOBB's
// axes); the extent keys start at +-1e300.
__global__ __launch_bounds__(64) void k_risk_frame(uint32_t nc, const float* __restrict__ s8,
                                                   const uint32_t* __restrict__ idx, const uint32_t* __restrict__ seg,
                                                   const double* __restrict__ partial, RiskCluster* __restrict__ out) {
  __shared__ double acc[kMomVals];
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const uint32_t b = seg[c], e = seg[c + 1], cnt = e - b;
  if (t < kMomVals) {
    const uint32_t chunks = (cnt + kChunk - 1) / kChunk;
    const double* p = partial + ((size_t)(b / kChunk) + c) * kMomVals + t;
    double a = 0.0;
    for (uint32_t k = 0; k < chunks; ++k) a += p[(size_t)k * kMomVals];
    acc[t] = a;
  }
  __syncthreads();
  if (t != 0) return;
  RiskCluster& o = out[c];
  double p0[3] = {0, 0, 0};
  if (cnt) {
    const float* q = s8 + 8 * (size_t)idx[b];
    p0[0] = q[0], p0[1] = q[1], p0[2] = q[2];
  }
  o.count = cnt;
  const double n = cnt ? (double)cnt : 1.0;
  double m[3], C[9], w[3], Vv[9];
  for (int k = 0; k < 3; ++k) m[k] = acc[k] / n;
  const double sxx = acc[3] / n - m[0] * m[0], sxy = acc[4] / n - m[0] * m[1], sxz = acc[5] / n - m[0] * m[2],
               syy = acc[6] / n - m[1] * m[1], syz = acc[7] / n - m[1] * m[2], szz = acc[8] / n - m[2] * m[2];
  C[0] = sxx, C[1] = sxy, C[2] = sxz, C[3] = sxy, C[4] = syy, C[5] = syz, C[6] = sxz, C[7] = syz, C[8] = szz;
  jacobi_eig<3>(C, w, Vv);
  int mj = 0, mn = 0;
  for (int k = 1; k < 3; ++k) {
    if (w[k] > w[mj]) mj = k;
    if (w[k] < w[mn]) mn = k;
  }
  if (mj == mn) mn = (mj + 1) % 3;  // (all equal)
  double major[3], minor[3], middle[3];
  double nj = 0, nn = 0;
  for (int k = 0; k < 3; ++k) {
    major[k] = Vv[3 * k + mj];
    minor[k] = Vv[3 * k + mn];
    nj += major[k] * major[k];
    nn += minor[k] * minor[k];
  }
  nj = sqrt(nj), nn = sqrt(nn);
  for (int k = 0; k < 3; ++k) major[k] /= nj, minor[k] /= nn;
  // one sign per axis, whatever the solver returns: the component of largest magnitude (the
  // first of equals) is positive. CropBox's frame goes through Euler angles that PCL composes
  // in the other order, so it is not the same for R and R diag(+-1).
  risk_fix_sign(major);
  risk_fix_sign(minor);
  middle[0] = minor[1] * major[2] - minor[2] * major[1];
  middle[1] = minor[2] * major[0] - minor[0] * major[2];
  middle[2] = minor[0] * major[1] - minor[1] * major[0];
  for (int k = 0; k < 3; ++k) {
    o.frame[k] = m[k];  // (relative to p0)
    o.frame[3 + k] = major[k];
    o.frame[6 + k] = middle[k];
    o.frame[9 + k] = minor[k];
    o.p0[k] = p0[k];
    o.sum_n[k] = acc[9 + k];
    o.sum_p[k] = acc[k] + (double)cnt * p0[k];
    o.ext[k] = risk_enc(1e300);
    o.ext[3 + k] = risk_enc(-1e300);
  }
  for (int k = 0; k < 6; ++k) o.sum_nn[k] = acc[12 + k];
}

// Extents of a chunk of a cluster's points in its box frame, merged with integer atomics on the
// order-preserving bits: min / max are order-free.
__global__ __launch_bounds__(kRiskThreads) void k_risk_extents(uint32_t nc, const float* __restrict__ s8,
                                                               const uint32_t* __restrict__ idx,
                                                               const uint32_t* __restrict__ seg, RiskCluster* out) {
  __shared__ double sh[6][kRiskThreads];
  __shared__ double fr[15];
  uint32_t c, chunk;
  if (!risk_slot(seg, nc, blockIdx.x, &c, &chunk)) return;
  const uint32_t b = seg[c], e = seg[c + 1], t = threadIdx.x;
  const uint64_t first = (uint64_t)b + (uint64_t)chunk * kChunk;
  const uint32_t end = (uint32_t)min((uint64_t)e, first + kChunk);
  if (t < 12) fr[t] = out[c].frame[t];
  if (t >= 12 && t < 15) fr[t] = out[c].p0[t - 12];
  __syncthreads();
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (uint32_t i = (uint32_t)first + t; i < end; i += kRiskThreads) {
    const float* q = s8 + 8 * (size_t)idx[i];
    const double x = ((double)q[0] - fr[12]) - fr[0], y = ((double)q[1] - fr[13]) - fr[1],
                 z = ((double)q[2] - fr[14]) - fr[2];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double l = x * fr[3 + 3 * a] + y * fr[4 + 3 * a] + z * fr[5 + 3 * a];
      lo[a] = fmin(lo[a], l);
      hi[a] = fmax(hi[a], l);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    sh[a][t] = lo[a];
    sh[3 + a][t] = hi[a];
  }
  __syncthreads();
  for (uint32_t h = kRiskThreads / 2; h > 0; h >>= 1) {
    if (t < h) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        sh[a][t] = fmin(sh[a][t], sh[a][t + h]);
        sh[3 + a][t] = fmax(sh[3 + a][t], sh[3 + a][t + h]);
      }
    }
    __syncthreads();
  }
  if (t < 3) atomicMin(&out[c].ext[t], risk_enc(sh[t][0]));
  else if (t < 6) atomicMax(&out[c].ext[t], risk_enc(sh[t][0]));
}

// One thread per cluster: the centre moves to the middle of the extents, min / max become
// +-half, overlapBoxFilter's scaling, and CropBox's frame of the box.
__global__ __launch_bounds__(64) void k_risk_box(uint32_t nc, float scale_x, float scale_y, float scale_z,
                                                 RiskCluster* __restrict__ out) {
  const uint32_t c = blockIdx.x * 64u + threadIdx.x;
  if (c >= nc) return;
  RiskCluster& o = out[c];
  const double sc[3] = {scale_x, scale_y, scale_z};
  const double* frame = o.frame;
  double shift[3], half[3];
  for (int a = 0; a < 3; ++a) {
    if (o.count) {
      const double lo = risk_dec(o.ext[a]), hi = risk_dec(o.ext[3 + a]);
      shift[a] = (hi + lo) / 2;
      half[a] = (hi - lo) / 2;
    } else {
      shift[a] = half[a] = 0;
    }
  }
  float Rf[9];
  for (int k = 0; k < 3; ++k) {
    // centre = mean + R shift, R's columns the axes
    o.centre[k] = (o.p0[k] + frame[k]) + (frame[3 + k] * shift[0] + frame[6 + k] * shift[1] + frame[9 + k] * shift[2]);
    for (int a = 0; a < 3; ++a) {
      o.rot[3 * k + a] = frame[3 + 3 * a + k];
      Rf[3 * k + a] = (float)o.rot[3 * k + a];
    }
    o.half[k] = half[k] * sc[k];
    o.box.half[k] = (float)o.half[k];
    o.box.t[k] = (float)o.centre[k];
  }
  float rpy[3];
  crop_rotation_inverse(Rf, o.box.inv, rpy);
  o.box.pad = 0.f;
}

// CropBox membership of (x, y, z) in a staged box (k_crop_count's test with min = -half, max = half)
__device__ __forceinline__ bool risk_in_box(const RiskBox& a, float px, float py, float pz) {
  if (!isfinite(px) || !isfinite(py) || !isfinite(pz)) return false;
  const float x = __fsub_rn(px, a.t[0]), y = __fsub_rn(py, a.t[1]), z = __fsub_rn(pz, a.t[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const float l = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.inv[3 * r], x), __fmul_rn(a.inv[3 * r + 1], y)),
                                        __fmul_rn(a.inv[3 * r + 2], z)),
                              0.f);
    if (l < -a.half[r] || l > a.half[r]) return false;
  }
  return true;
}

// cnt[box * ncx + label] += 1 for every point of X (label in [0, ncx)) inside box of Y
__global__ __launch_bounds__(kRiskThreads) void k_risk_counts(uint32_t V, uint32_t ncx, uint32_t ncy,
                                                              const float* __restrict__ s8,
                                                              const int32_t* __restrict__ lab,
                                                              const RiskCluster* __restrict__ boxes,
                                                              uint32_t* __restrict__ cnt) {
  __shared__ RiskBox sb[kBoxTile];
  __shared__ uint32_t hist[kHistWords];
  const uint32_t i = blockIdx.x * kRiskThreads + threadIdx.x;
  const bool use_lds = (size_t)kBoxTile * ncx <= (size_t)kHistWords;
  int32_t l = -1;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (i < V) {
    l = lab[i];
    if (l >= (int32_t)ncx) l = -1;
    px = s8[8 * (size_t)i];
    py = s8[8 * (size_t)i + 1];
    pz = s8[8 * (size_t)i + 2];
  }
  for (uint32_t b0 = 0; b0 < ncy; b0 += kBoxTile) {
    const uint32_t nb = min((uint32_t)kBoxTile, ncy - b0);
    if (threadIdx.x < nb) sb[threadIdx.x] = boxes[b0 + threadIdx.x].box;
    if (use_lds)
      for (uint32_t k = threadIdx.x; k < nb * ncx; k += kRiskThreads) hist[k] = 0u;
    __syncthreads();
    if (l >= 0) {
      for (uint32_t j = 0; j < nb; ++j) {
        if (risk_in_box(sb[j], px, py, pz)) {
          if (use_lds) atomicAdd(&hist[j * ncx + (uint32_t)l], 1u);
          else atomicAdd(&cnt[(size_t)(b0 + j) * ncx + (uint32_t)l], 1u);
        }
      }
    }
    __syncthreads();
    if (use_lds)
      for (uint32_t k = threadIdx.x; k < nb * ncx; k += kRiskThreads) {
        const uint32_t h = hist[k];
        if (h) atomicAdd(&cnt[(size_t)b0 * ncx + k], h);
      }
    __syncthreads();
  }
}

// ---- matching and PCA (filteringUtils.cpp:236-286, 288-424), one workgroup -----------------
__device__ __forceinline__ float risk_overlap(uint32_t a_in_b, uint32_t na, uint32_t b_in_a, uint32_t nb) {
  const float pa = (float)a_in_b / (float)na;
  const float pb = (float)b_in_a / (float)nb;
  const float ov = __fmul_rn(pa, pb);
  return (float)((double)ov * 100.0);
}

__device__ __forceinline__ float risk_angle(const double* a, const double* b, double na, double nb) {
  // the clusters' mean normals; their cosine clamped to [-1, 1]
  const double ax = a[0] / na, ay = a[1] / na, az = a[2] / na, bx = b[0] / nb, by = b[1] / nb, bz = b[2] / nb;
  const double den = sqrt(ax * ax + ay * ay + az * az) * sqrt(bx * bx + by * by + bz * bz);
  if (!(den > 0.0)) return NAN;
  double c = (ax * bx + ay * by + az * bz) / den;
  c = fmin(1.0, fmax(-1.0, c));
  return (float)(acos(c) * 180.0 / M_PI);
}

__global__ __launch_bounds__(kRiskThreads) void k_risk_match(uint32_t nca, uint32_t ncb,
                                                             const RiskCluster* __restrict__ ca,
                                                             const RiskCluster* __restrict__ cb,
                                                             const uint32_t* __restrict__ a_in_b,  // [ncb][nca]
                                                             const uint32_t* __restrict__ b_in_a,  // [nca][ncb]
                                                             float max_angle, int32_t* __restrict__ best_j,
                                                             float* __restrict__ best_ov, float* __restrict__ best_d,
                                                             int32_t* __restrict__ m_idx, float* __restrict__ m_ov,
                                                             float* __restrict__ m_dist, RiskOut* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  for (uint32_t i = t; i < nca; i += kRiskThreads) {
    float mx = 0.f, cd = -1.f;
    int32_t bj = -1;
    const uint32_t na = ca[i].count;
    for (uint32_t j = 0; j < ncb; ++j) {
      const uint32_t nb = cb[j].count;
      const float dist = risk_angle(ca[i].sum_n, cb[j].sum_n, (double)na, (double)nb);
      const float ov = risk_overlap(a_in_b[(size_t)j * nca + i], na, b_in_a[(size_t)i * ncb + j], nb);
      if (ov > mx && dist < max_angle) {
        bj = (int32_t)j;
        mx = ov;
        cd = dist;
      }
    }
    best_j[i] = mx > 0.f ? bj : -1;
    best_ov[i] = mx;
    best_d[i] = cd;
  }
  __syncthreads();  // (one workgroup: best_* written above are read below)
  for (uint32_t j = t; j < ncb; j += kRiskThreads) {
    int32_t mi = -1;
    float mo = -1.f, md = -1.f;
    for (uint32_t i = 0; i < nca; ++i) {
      if (best_j[i] != (int32_t)j) continue;
      if (mi == -1 || best_ov[i] > mo) {
        mi = (int32_t)i;
        mo = best_ov[i];
        md = best_d[i];
      }
    }
    m_idx[j] = mi;
    m_ov[j] = mo;
    m_dist[j] = md;
  }
  __syncthreads();
  if (t != 0) return;
  RiskOut o{};
  double S[6] = {0, 0, 0, 0, 0, 0}, sp[3] = {0, 0, 0};
  uint64_t npts = 0;
  for (uint32_t j = 0; j < ncb; ++j) {
    const int32_t i = m_idx[j];
    if (i < 0) continue;
    ++o.n_matches;
    for (int k = 0; k < 6; ++k) S[k] += ca[i].sum_nn[k];
    for (int k = 0; k < 3; ++k) sp[k] += ca[i].sum_p[k];
    npts += ca[i].count;
  }
  if (o.n_matches) {
    const double C[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
    double w[3], Vv[9];
    jacobi_eig<3>(C, w, Vv);
    int ord[3] = {0, 1, 2};
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2 - a; ++b)
        if (w[ord[b]] < w[ord[b + 1]]) {
          const int tmp = ord[b];
          ord[b] = ord[b + 1];
          ord[b + 1] = tmp;
        }
    const double sum = (w[ord[0]] + w[ord[1]]) + w[ord[2]];
    for (int k = 0; k < 3; ++k) {
      o.eigenvalues[k] = sum > 0 ? w[ord[k]] / sum : 0.0;
      for (int r = 0; r < 3; ++r) o.eigenvectors[3 * r + k] = Vv[3 * r + ord[k]];
      o.centroid[k] = npts ? sp[k] / (double)npts : 0.0;
    }
    const double l0 = w[ord[0]], l2 = w[ord[2]];
    o.alignability = l0 > 0 ? (float)(100.0 * (l2 / l0)) : 0.f;
  }
  *out = o;
}

}  // namespace

size_t fov_tiles(size_t n) { return (n + kFovTile - 1) / kFovTile; }

void launch_fov_filter(hipStream_t s, uint32_t n, const FovArgs& a, const float4* pts, uint32_t* tile_cnt,
                       uint32_t* tile_off, uint32_t* total, float4* out) {
  const uint32_t tiles = (uint32_t)fov_tiles(n);
  if (tiles == 0) {
    (void)hipMemsetAsync(total, 0, sizeof(uint32_t), s);
    return;
  }
  k_fov_count<<<tiles, kRiskThreads, 0, s>>>(n, a, pts, tile_cnt);
  launch_tile_scan(s, (int)tiles, tile_cnt, tile_off, total);
  k_fov_scatter<<<tiles, kRiskThreads, 0, s>>>(n, a, pts, tile_off, out);
}

void launch_risk_gather(hipStream_t s, uint32_t V, const float4* sampled, const float4* nrm, const uint32_t* inv,
                        const int32_t* cluster_of, float* s8, int32_t* lab) {
  if (V) k_risk_gather<<<blocks_for(V), 256, 0, s>>>(V, sampled, nrm, inv, cluster_of, s8, lab);
}

size_t risk_sort_temp_bytes(size_t n) {
  size_t b = 0;
  (void)rocprim::radix_sort_pairs(nullptr, b, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, n, 0, 32);
  return b;
}

size_t risk_partial_bytes(size_t V, size_t nc) { return (V / kChunk + nc + 2) * kMomVals * sizeof(double); }

hipError_t launch_risk_clusters(hipStream_t s, uint32_t V, uint32_t nc, const float* s8, const int32_t* lab,
                                uint32_t* k0, uint32_t* k1, uint32_t* v0, uint32_t* idx, uint32_t* seg, void* temp,
                                size_t temp_bytes, double* partial, const float scale[3], RiskCluster* out) {
  if (nc == 0 || V == 0) return hipSuccess;
  k_risk_keys<<<blocks_for(V), 256, 0, s>>>(V, nc, lab, k0, v0);
  const hipError_t e = rocprim::radix_sort_pairs(temp, temp_bytes, k0, k1, v0, idx, V, 0, 32, s);
  if (e != hipSuccess) return e;
  k_risk_segs<<<blocks_for(nc + 1), 256, 0, s>>>(V, nc, k1, seg);
  const uint32_t grid = V / kChunk + nc + 1;  // every slot (risk_slot)
  k_risk_moments<<<grid, kRiskThreads, 0, s>>>(nc, s8, idx, seg, partial);
  k_risk_frame<<<nc, 64, 0, s>>>(nc, s8, idx, seg, partial, out);
  k_risk_extents<<<grid, kRiskThreads, 0, s>>>(nc, s8, idx, seg, out);
  k_risk_box<<<(nc + 63) / 64, 64, 0, s>>>(nc, scale[0], scale[1], scale[2], out);
  return hipGetLastError();
}

void launch_risk_counts(hipStream_t s, uint32_t V, uint32_t ncx, uint32_t ncy, const float* s8, const int32_t* lab,
                        const RiskCluster* boxes, uint32_t* cnt) {
  if (V && ncx && ncy) k_risk_counts<<<blocks_for(V), kRiskThreads, 0, s>>>(V, ncx, ncy, s8, lab, boxes, cnt);
}

void launch_risk_match(hipStream_t s, uint32_t nca, uint32_t ncb, const RiskCluster* ca, const RiskCluster* cb,
                       const uint32_t* a_in_b, const uint32_t* b_in_a, float max_angle, int32_t* best_j,
                       float* best_ov, float* best_d, int32_t* m_idx, float* m_ov, float* m_dist, RiskOut* out) {
  k_risk_match<<<1, kRiskThreads, 0, s>>>(nca, ncb, ca, cb, a_in_b, b_in_a, max_angle, best_j, best_ov, best_d, m_idx,
                                          m_ov, m_dist, out);
}

}  // namespace aicp
