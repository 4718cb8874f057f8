// Sampled ICP chains: libpointmatcher's MinDist, RandomSampling and MaxDensity
// data-point filters, the SurfaceNormal densities, and the MaxDist outlier rule's select step.
//
// A filter is an order-preserving stream compaction, the shape of kernels_crop.hip:
//   k_chain_flag     one 1024-point tile per block: keep flags (one byte per point) -> tile count
//   launch_tile_scan the crop's exclusive scan of the tile counts; its total is the next count
//   k_chain_scatter  ballot prefix inside each wave, LDS prefix over the 4 waves, 4 rounds per
//                    tile in index order -> the kept rows at their rank, with their descriptors
// The point count of every stage lives on the device (ChainCtl::n): the grids are sized by the
// input cloud, the kernels read the count of the cloud they receive, and the host reads all counts
// once after the last filter. Rows are float4 with the input index in w, as bpts carries it, and
// move with one 128-bit load and store. No atomics: a row's place is its rank among the kept.
#include <algorithm>

#include "chain_draw.hpp"
#include "kernels.hpp"

namespace aicp {
namespace {

constexpr int kChainThreads = 256;
constexpr int kChainTile = 1024;  // 4 rounds of 256, the crop's tile (its scan serves both)

// Correctly rounded float square root, as sqrtf on the host (kernels_prefilter.hip: __fsqrt_rn is
// the native instruction on gfx950, one ulp off on some inputs; the densities then differed from
// the oracle's by up to 7 ulp, the radius being cubed)
__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }

// The keep rule of filter `a` for point i of the n it receives.
__device__ __forceinline__ bool chain_keep(const ChainFilterArgs& a, uint32_t i, uint32_t n,
                                           const float4* __restrict__ pts, const float* __restrict__ dens,
                                           const ChainCtl* __restrict__ ctl) {
  switch (a.kind) {
    case kChainMinDist: {
      const float4 p = pts[i];
      if (a.dim < 0) {
        // MinDistDataPointsFilter: the norm of the point, float, one rounding per operation
        const float d = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y)), __fmul_rn(p.z, p.z)));
        return d > fabsf(a.min_dist);
      }
      const float c = a.dim == 0 ? p.x : (a.dim == 1 ? p.y : p.z);
      return fabsf(c) > a.min_dist;
    }
    case kChainRandom:
      return chain_uniform(a.seed, a.slot, i) < a.prob;  // every point draws
    case kChainMaxDensity: {
      const float d = dens[i];
      if (!(d > a.max_density)) return true;  // kept without a draw
      float accept = __fdiv_rn(a.max_density, d);
      // the saturated points (density == the cloud's maximum): integer division, so the factor is
      // 1 unless every point is saturated, and 0 then
      if (d == __uint_as_float(ctl->max_bits)) accept = __fmul_rn(accept, (float)(1 - (int32_t)(ctl->n_sat / n)));
      return chain_uniform(a.seed, a.slot, i) < accept;
    }
    default:
      return true;
  }
}

__global__ __launch_bounds__(kChainThreads) void k_chain_flag(ChainFilterArgs a, const ChainCtl* __restrict__ ctl,
                                                              const float4* __restrict__ pts,
                                                              const float* __restrict__ dens, uint8_t* __restrict__ flag,
                                                              uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wsum[kChainThreads / 64];
  const uint32_t n = ctl->n[a.pos];
  const uint32_t base = blockIdx.x * kChainTile;
  uint32_t c = 0;
#pragma unroll
  for (int r = 0; r < kChainTile / kChainThreads; ++r) {
    const uint32_t i = base + r * kChainThreads + threadIdx.x;
    if (i < n) {
      const bool keep = chain_keep(a, i, n, pts, dens, ctl);
      flag[i] = keep ? 1 : 0;
      c += keep ? 1u : 0u;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  // (a tile past the cloud this filter receives counts 0: the scan runs over the input's tiles)
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(kChainThreads) void k_chain_scatter(int pos, const ChainCtl* __restrict__ ctl,
                                                                 const uint8_t* __restrict__ flag,
                                                                 const uint32_t* __restrict__ tile_off,
                                                                 const float4* __restrict__ pts, float4* __restrict__ out,
                                                                 const float4* __restrict__ nrm, float4* __restrict__ nrm_out,
                                                                 const float* __restrict__ dens, float* __restrict__ dens_out) {
  __shared__ uint32_t wcnt[kChainThreads / 64];
  const uint32_t n = ctl->n[pos];
  const uint32_t base = blockIdx.x * kChainTile;
  if (base >= n) return;  // (whole block)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t run = tile_off[blockIdx.x];
#pragma unroll 1
  for (int r = 0; r < kChainTile / kChainThreads; ++r) {
    const uint32_t i = base + r * kChainThreads + threadIdx.x;
    const bool keep = i < n && flag[i] != 0;
    const uint64_t m = __ballot(keep);
    const uint32_t below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t wb = run;
    for (int q = 0; q < w; ++q) wb += wcnt[q];
    if (keep) {
      const uint32_t o = wb + below;  // < the kept count <= n: inside every output array
      out[o] = pts[i];
      if (nrm_out) nrm_out[o] = nrm[i];
      if (dens_out) dens_out[o] = dens[i];  // (null behind the MaxDensity: nobody reads them any more)
    }
    run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
}

// MaxDensity's lastDensity (the maximum density, as bits) and nbSaturated (the points equal to it)
// of the cloud the filter receives. One workgroup: a maximum and a count of exact matches do not
// depend on the order they are taken in.
__global__ __launch_bounds__(1024) void k_chain_density_max(int pos, ChainCtl* ctl, const float* __restrict__ dens) {
  __shared__ float wmax[16];
  __shared__ uint32_t wcnt[16];
  const uint32_t n = ctl->n[pos];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float m = -INFINITY;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) {
    const float d = dens[i];
    if (d > m) m = d;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float u = __shfl_xor(m, o, 64);
    if (u > m) m = u;
  }
  if (lane == 0) wmax[w] = m;
  __syncthreads();
  m = wmax[0];
  for (int q = 1; q < 16; ++q)
    if (wmax[q] > m) m = wmax[q];
  uint32_t c = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) c += dens[i] == m ? 1u : 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if (lane == 0) wcnt[w] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int q = 0; q < 16; ++q) t += wcnt[q];
    ctl->max_bits = __float_as_uint(m);
    ctl->n_sat = t;
  }
}

// the cloud as uploaded: w = the point's input index; the control block's start
__global__ __launch_bounds__(256) void k_chain_begin(uint32_t n, float4* pts, ChainCtl* ctl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    ctl->n[0] = n;
    for (int q = 1; q <= kChainMaxFilters; ++q) ctl->n[q] = 0;
    ctl->max_bits = 0;
    ctl->n_sat = 0;
    ctl->degenerate = 0;
  }
  if (i < n) pts[i].w = __int_as_float((int32_t)i);
}

// a SurfaceNormal keeps every point
__global__ void k_chain_pass(int pos, ChainCtl* ctl, const PairState* st) {
  ctl->n[pos + 1] = ctl->n[pos];
  if (st) ctl->degenerate = (uint32_t)st->degenerate;
}

// SurfaceNormal's outputs from the raw tree's bucket order (bpts, w = the point's position in the
// cloud at the filter) into that cloud's order: the normals k_normals_from_ids wrote, and the
// densities from the kNN ids k_knn_ids wrote (bucket positions, -1 past the cloud's size), as
// libpointmatcher computes them: the float mean of the neighbours in list order, the largest float
// norm of the centred neighbours, the ball's volume in double, realKnn / volume in float.
template <int K>
__global__ __launch_bounds__(256) void k_chain_sn_out(uint32_t n, const float4* __restrict__ bpts,
                                                      const int32_t* __restrict__ ids,
                                                      const float4* __restrict__ bnrm, float4* __restrict__ nrm,
                                                      float* __restrict__ dens) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  const uint32_t id = (uint32_t)__float_as_int(bpts[s].w);
  if (id >= n) return;  // (never: the tree's ids are the cloud's positions)
  if (nrm) nrm[id] = bnrm[s];
  if (!dens) return;
  int32_t nb[K];
#pragma unroll
  for (int i = 0; i < K; ++i) nb[i] = ids[(size_t)s * K + i];
  float sx = 0.f, sy = 0.f, sz = 0.f;
  int kk = 0;
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (nb[i] >= 0 && (uint32_t)nb[i] < n) {
      const float4 p = bpts[nb[i]];
      sx = __fadd_rn(sx, p.x);
      sy = __fadd_rn(sy, p.y);
      sz = __fadd_rn(sz, p.z);
      ++kk;
    }
  const float fk = (float)kk;
  const float mx = __fdiv_rn(sx, fk), my = __fdiv_rn(sy, fk), mz = __fdiv_rn(sz, fk);
  float far = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i)
    if (nb[i] >= 0 && (uint32_t)nb[i] < n) {
      const float4 p = bpts[nb[i]];
      const float a = __fsub_rn(p.x, mx), b = __fsub_rn(p.y, my), c = __fsub_rn(p.z, mz);
      const float r = sqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(a, a), __fmul_rn(b, b)), __fmul_rn(c, c)));
      far = fmaxf(far, r);
    }
  const double m = (double)far;
  const float vol = (float)((4. / 3.) * 3.14159265358979323846 * (m * m * m));
  dens[id] = __fdiv_rn(fk, vol);  // far == 0: +inf
}

// bnrm (the matcher tree's bucket order) from the reference's given normals (its input order)
__global__ __launch_bounds__(256) void k_chain_gather_normals(uint32_t n, const float4* __restrict__ bpts,
                                                              const float4* __restrict__ given,
                                                              float4* __restrict__ bnrm) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t id = (uint32_t)__float_as_int(bpts[j].w);
  if (id < n) bnrm[j] = given[id];
}

// the filtered rows as an uploaded cloud holds them: x, y, z, 1
__global__ __launch_bounds__(256) void k_chain_rows(uint32_t n, const float4* __restrict__ in, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  out[i] = make_float4(p.x, p.y, p.z, 1.f);
}

// MaxDistOutlierFilter's select step: the constant limit where k_icp_select writes the k-th distance
__global__ void k_chain_select_maxdist(int n_pairs, PairState* st, float limit_d2) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_pairs && st[p].active) st[p].limit = limit_d2;
}

inline unsigned grid_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t chain_tiles(size_t n) { return (n + kChainTile - 1) / kChainTile; }

void launch_chain_begin(hipStream_t s, uint32_t n, float4* pts, ChainCtl* ctl) {
  k_chain_begin<<<std::max(1u, grid_of(n)), 256, 0, s>>>(n, pts, ctl);
}

void launch_chain_pass(hipStream_t s, int pos, ChainCtl* ctl, const PairState* st) {
  k_chain_pass<<<1, 1, 0, s>>>(pos, ctl, st);
}

void launch_chain_filter(hipStream_t s, uint32_t cap, const ChainFilterArgs& a, ChainCtl* ctl, uint8_t* flag,
                         uint32_t* tile_cnt, uint32_t* tile_off, const float4* pts, float4* out, const float4* nrm,
                         float4* nrm_out, const float* dens, float* dens_out) {
  const int tiles = (int)chain_tiles(cap);
  if (tiles == 0) {
    launch_chain_pass(s, a.pos, ctl, nullptr);
    return;
  }
  if (a.kind == kChainMaxDensity) k_chain_density_max<<<1, 1024, 0, s>>>(a.pos, ctl, dens);
  k_chain_flag<<<tiles, kChainThreads, 0, s>>>(a, ctl, pts, dens, flag, tile_cnt);
  launch_tile_scan(s, tiles, tile_cnt, tile_off, &ctl->n[a.pos + 1]);
  k_chain_scatter<<<tiles, kChainThreads, 0, s>>>(a.pos, ctl, flag, tile_off, pts, out, nrm, nrm_out, dens, dens_out);
}

bool launch_chain_sn_out(hipStream_t s, uint32_t n, int knn, const float4* bpts, const int32_t* ids, const float4* bnrm,
                         float4* nrm, float* dens) {
  if (!n) return true;
  switch (knn) {
    case 10: k_chain_sn_out<10><<<grid_of(n), 256, 0, s>>>(n, bpts, ids, bnrm, nrm, dens); break;
    case 20: k_chain_sn_out<20><<<grid_of(n), 256, 0, s>>>(n, bpts, ids, bnrm, nrm, dens); break;
    case 30: k_chain_sn_out<30><<<grid_of(n), 256, 0, s>>>(n, bpts, ids, bnrm, nrm, dens); break;
    default: return false;
  }
  return true;
}

void launch_chain_gather_normals(hipStream_t s, uint32_t n, const float4* bpts, const float4* given, float4* bnrm) {
  if (n) k_chain_gather_normals<<<grid_of(n), 256, 0, s>>>(n, bpts, given, bnrm);
}

void launch_chain_rows(hipStream_t s, uint32_t n, const float4* in, float4* out) {
  if (n) k_chain_rows<<<grid_of(n), 256, 0, s>>>(n, in, out);
}

void launch_chain_select_maxdist(hipStream_t s, int n_pairs, PairState* st, float limit_d2) {
  k_chain_select_maxdist<<<(n_pairs + 63) / 64, 64, 0, s>>>(n_pairs, st, limit_d2);
}

}  // namespace aicp
