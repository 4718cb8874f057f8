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

// The keep rule of filter `a` for point i of the n its cloud holds there. pts / dens: that cloud's
// rows; maxsat: the cloud's {max_bits, n_sat} (ChainCtl's, or one ChainCloud's of a batch).
__device__ __forceinline__ bool chain_keep(const ChainFilterArgs& a, uint32_t i, uint32_t n,
                                           const float4* __restrict__ pts, const float* __restrict__ dens,
                                           const uint32_t* __restrict__ maxsat) {
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
      if (d == __uint_as_float(maxsat[0])) accept = __fmul_rn(accept, (float)(1 - (int32_t)(maxsat[1] / n)));
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
      const bool keep = chain_keep(a, i, n, pts, dens, &ctl->max_bits);
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
// One slot s (< n) of one cloud's tree: bpts / ids / bnrm / nrm / dens are that cloud's (a batch
// passes them moved by the cloud's offset).
template <int K>
__device__ __forceinline__ void chain_sn_slot(uint32_t n, uint32_t s, const float4* __restrict__ bpts,
                                              const int32_t* __restrict__ ids, const float4* __restrict__ bnrm,
                                              float4* __restrict__ nrm, float* __restrict__ dens) {
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

template <int K>
__global__ __launch_bounds__(256) void k_chain_sn_out(uint32_t n, const float4* __restrict__ bpts,
                                                      const int32_t* __restrict__ ids,
                                                      const float4* __restrict__ bnrm, float4* __restrict__ nrm,
                                                      float* __restrict__ dens) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) chain_sn_slot<K>(n, s, bpts, ids, bnrm, nrm, dens);
}

// bnrm (the matcher trees' bucket order) from the references' given normals (each in its input
// order, at the reference's ref_off): slot j's reference by search over the ascending ref_off
__global__ __launch_bounds__(256) void k_chain_gather_normals(int n_refs, const PairDesc* __restrict__ rd, uint32_t n,
                                                              const float4* __restrict__ bpts,
                                                              const float4* __restrict__ given,
                                                              float4* __restrict__ bnrm) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int lo = 0, hi = n_refs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rd[mid].ref_off <= j) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t off = rd[lo].ref_off;
  const uint32_t id = (uint32_t)__float_as_int(bpts[j].w);
  if (id < rd[lo].n_ref) bnrm[j] = given[off + id];  // off + id < off + n_ref <= n
}

// ---- the batch form: one side's clouds concatenated ("chains in batches") ---------
// Stage q of the side holds cloud c at rows [cl[c].off[q], + cl[c].n[q]); the clouds follow each
// other without gaps, so an order-preserving compaction of the whole concatenation keeps every cloud
// contiguous and in order, and the kept rows before a cloud's first row are its next offset.
// ChainCtl::n holds the concatenation's totals. A point finds its cloud by search over the offsets.

// the last cloud whose offset at stage q is <= i: the one that holds row i (an emptied cloud shares
// its offset with the cloud behind it, which the search prefers)
__device__ __forceinline__ int chainb_cloud_of(const ChainCloud* __restrict__ cl, int n_clouds, int q, uint32_t i) {
  int lo = 0, hi = n_clouds - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (cl[mid].off[q] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// rows of the clouds as uploaded (w = 1) -> the side's first buffer, w = the index in the own cloud
__global__ __launch_bounds__(256) void k_chainb_begin(int n_clouds, const ChainCloud* __restrict__ cl, uint32_t total,
                                                      const float4* __restrict__ src, const uint32_t* __restrict__ src_off,
                                                      float4* __restrict__ pts, ChainCtl* ctl) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    ctl->n[0] = total;
    for (int q = 1; q <= kChainMaxFilters; ++q) ctl->n[q] = 0;
    ctl->max_bits = 0;
    ctl->n_sat = 0;
    ctl->degenerate = 0;
  }
  if (i >= total) return;
  const int c = chainb_cloud_of(cl, n_clouds, 0, i);
  const uint32_t k = i - cl[c].off[0];
  float4 p = src[src_off[c] + k];  // (k < cl[c].n[0]: inside the cloud's rows of the upload)
  p.w = __int_as_float((int32_t)k);
  pts[i] = p;
}

__global__ __launch_bounds__(kChainThreads) void k_chainb_flag(ChainFilterArgs a, int n_clouds,
                                                               const ChainCloud* __restrict__ cl,
                                                               const ChainCtl* __restrict__ ctl,
                                                               const float4* __restrict__ pts,
                                                               const float* __restrict__ dens, uint8_t* __restrict__ flag,
                                                               uint32_t* __restrict__ tile_cnt) {
  __shared__ uint32_t wsum[kChainThreads / 64];
  const uint32_t n = ctl->n[a.pos];
  const uint32_t base = blockIdx.x * kChainTile;
  uint32_t c = 0;
  if (base < n) {
    // the tile's first cloud once; a lane steps on from there (a 1024-row tile and a 64-lane wave can
    // hold rows of several clouds)
    const int c0 = chainb_cloud_of(cl, n_clouds, a.pos, base);
#pragma unroll 1
    for (int r = 0; r < kChainTile / kChainThreads; ++r) {
      const uint32_t i = base + r * kChainThreads + threadIdx.x;
      if (i < n) {
        int cc = c0;
        while (cc + 1 < n_clouds && cl[cc + 1].off[a.pos] <= i) ++cc;
        const uint32_t off = cl[cc].off[a.pos];
        const bool keep = chain_keep(a, i - off, cl[cc].n[a.pos], pts + off, dens ? dens + off : nullptr, &cl[cc].max_bits);
        flag[i] = keep ? 1 : 0;
        c += keep ? 1u : 0u;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// kept rows before row b of the stage the filter received (b <= its total n): the scanned tile
// offset plus the flags of the tile's rows before b, summed by one wave
__device__ __forceinline__ uint32_t chainb_rank(uint32_t b, uint32_t n, uint32_t n_next,
                                                const uint8_t* __restrict__ flag,
                                                const uint32_t* __restrict__ tile_off, int lane) {
  if (b >= n) return n_next;  // (uniform over the wave)
  const uint32_t t = b / kChainTile;
  uint32_t c = 0;
  for (uint32_t i = t * kChainTile + lane; i < b; i += 64) c += flag[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  return tile_off[t] + c;
}

// one wave per cloud, behind the scan: the cloud's next offset and count
__global__ __launch_bounds__(64) void k_chainb_counts(int pos, int n_clouds, ChainCloud* cl,
                                                      const ChainCtl* __restrict__ ctl,
                                                      const uint8_t* __restrict__ flag,
                                                      const uint32_t* __restrict__ tile_off) {
  const int c = blockIdx.x;
  if (c >= n_clouds) return;
  const uint32_t n = ctl->n[pos], n_next = ctl->n[pos + 1];
  const uint32_t b0 = cl[c].off[pos], b1 = b0 + cl[c].n[pos];
  const uint32_t r0 = chainb_rank(b0, n, n_next, flag, tile_off, threadIdx.x);
  const uint32_t r1 = chainb_rank(b1, n, n_next, flag, tile_off, threadIdx.x);
  if (threadIdx.x == 0) {
    cl[c].off[pos + 1] = r0;
    cl[c].n[pos + 1] = r1 - r0;
  }
}

// MaxDensity's lastDensity and nbSaturated per cloud, over as many workgroups as the side has
// tiles: densities are never negative (k / volume, +inf for a zero radius), so their bits order as
// they do, and a maximum and a count of exact matches are the same in any order: integer atomics,
// one per wave where the wave lies inside one cloud
__global__ void k_chainb_density_reset(int n_clouds, ChainCloud* cl) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < n_clouds) {
    cl[c].max_bits = 0;
    cl[c].n_sat = 0;
  }
}

template <bool kCount>
__global__ __launch_bounds__(kChainThreads) void k_chainb_density(int pos, int n_clouds, ChainCloud* cl,
                                                                 const ChainCtl* __restrict__ ctl,
                                                                 const float* __restrict__ dens) {
  const uint32_t n = ctl->n[pos];
  const uint32_t base = blockIdx.x * kChainTile;
  if (base >= n) return;
  const int c0 = chainb_cloud_of(cl, n_clouds, pos, base);
#pragma unroll 1
  for (int r = 0; r < kChainTile / kChainThreads; ++r) {
    const uint32_t i = base + r * kChainThreads + threadIdx.x;
    const bool in = i < n;
    int cc = c0;
    uint32_t v = 0;
    if (in) {
      while (cc + 1 < n_clouds && cl[cc + 1].off[pos] <= i) ++cc;
      const uint32_t bits = __float_as_uint(dens[i]);
      v = kCount ? (bits == cl[cc].max_bits ? 1u : 0u) : bits;
    }
    // a wave whose live lanes share one cloud: one atomic for the wave
    const int cf = __shfl(cc, __ffsll((unsigned long long)__ballot(in)) - 1, 64);
    if (__all(!in || cc == cf)) {
      uint32_t w = v;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const uint32_t u = __shfl_xor(w, o, 64);
        w = kCount ? w + u : (u > w ? u : w);
      }
      if (__ballot(in) && (threadIdx.x & 63) == 0) {
        if (kCount) {
          if (w) atomicAdd(&cl[cf].n_sat, w);
        } else {
          atomicMax(&cl[cf].max_bits, w);
        }
      }
    } else if (in) {
      if (kCount) {
        if (v) atomicAdd(&cl[cc].n_sat, 1u);
      } else {
        atomicMax(&cl[cc].max_bits, v);
      }
    }
  }
}

// a SurfaceNormal keeps every point of every cloud; st (nullable): the states launch_normals counted
// the degenerate points in, one per cloud that had points (cl[c].sn_slot, -1: none)
__global__ void k_chainb_pass(int pos, int n_clouds, ChainCloud* cl, ChainCtl* ctl, const PairState* st) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) ctl->n[pos + 1] = ctl->n[pos];
  if (c >= n_clouds) return;
  cl[c].n[pos + 1] = cl[c].n[pos];
  cl[c].off[pos + 1] = cl[c].off[pos];
  if (st && cl[c].sn_slot >= 0) cl[c].degenerate = (uint32_t)st[cl[c].sn_slot].degenerate;
}

// k_chain_sn_out over the trees of the clouds that had points (pd: ascending ref_off, the cloud's
// offset at the filter, where its rows, normals and densities lie too)
template <int K>
__global__ __launch_bounds__(256) void k_chainb_sn_out(int n_trees, const PairDesc* __restrict__ pd, uint32_t total,
                                                       const float4* __restrict__ bpts,
                                                       const int32_t* __restrict__ ids,
                                                       const float4* __restrict__ bnrm, float4* __restrict__ nrm,
                                                       float* __restrict__ dens) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= total) return;
  int lo = 0, hi = n_trees - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pd[mid].ref_off <= s) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t off = pd[lo].ref_off, n = pd[lo].n_ref;
  if (s - off >= n) return;  // (never: the trees tile [0, total))
  chain_sn_slot<K>(n, s - off, bpts + off, ids + (size_t)off * K, bnrm + off, nrm ? nrm + off : nullptr,
                   dens ? dens + off : nullptr);
}

// the kept rows of the clouds that run, as upload_pairs stores clouds: segment g's n rows from
// in + src to out + dst (x, y, z, 1), the normals beside them (nullable)
__global__ __launch_bounds__(256) void k_chainb_rows(int n_segs, const ChainSeg* __restrict__ sg, uint32_t total,
                                                     const float4* __restrict__ in, float4* __restrict__ out,
                                                     const float4* __restrict__ nrm, float4* __restrict__ nrm_out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = n_segs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sg[mid].dst <= i) lo = mid;
    else hi = mid - 1;
  }
  const uint32_t k = i - sg[lo].dst;
  if (k >= sg[lo].n) return;  // (never: the segments tile [0, total))
  const float4 p = in[sg[lo].src + k];
  out[i] = make_float4(p.x, p.y, p.z, 1.f);
  if (nrm_out) nrm_out[i] = nrm[sg[lo].src + k];
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

void launch_chain_gather_normals(hipStream_t s, int n_refs, const PairDesc* rd, uint32_t n, const float4* bpts,
                                 const float4* given, float4* bnrm) {
  if (n && n_refs > 0) k_chain_gather_normals<<<grid_of(n), 256, 0, s>>>(n_refs, rd, n, bpts, given, bnrm);
}

void launch_chain_rows(hipStream_t s, uint32_t n, const float4* in, float4* out) {
  if (n) k_chain_rows<<<grid_of(n), 256, 0, s>>>(n, in, out);
}

void launch_chain_select_maxdist(hipStream_t s, int n_pairs, PairState* st, float limit_d2) {
  k_chain_select_maxdist<<<(n_pairs + 63) / 64, 64, 0, s>>>(n_pairs, st, limit_d2);
}

// ---- the batch form ---------------------------------------------------------------------------
void launch_chainb_begin(hipStream_t s, int n_clouds, const ChainCloud* cl, uint32_t total, const float4* src,
                         const uint32_t* src_off, float4* pts, ChainCtl* ctl) {
  k_chainb_begin<<<std::max(1u, grid_of(total)), 256, 0, s>>>(n_clouds, cl, total, src, src_off, pts, ctl);
}

void launch_chainb_pass(hipStream_t s, int pos, int n_clouds, ChainCloud* cl, ChainCtl* ctl, const PairState* st) {
  k_chainb_pass<<<(n_clouds + 63) / 64, 64, 0, s>>>(pos, n_clouds, cl, ctl, st);
}

void launch_chainb_filter(hipStream_t s, uint32_t cap, const ChainFilterArgs& a, int n_clouds, ChainCloud* cl,
                          ChainCtl* ctl, uint8_t* flag, uint32_t* tile_cnt, uint32_t* tile_off, const float4* pts,
                          float4* out, const float4* nrm, float4* nrm_out, const float* dens, float* dens_out) {
  const int tiles = (int)chain_tiles(cap);
  if (tiles == 0) {
    launch_chainb_pass(s, a.pos, n_clouds, cl, ctl, nullptr);
    return;
  }
  if (a.kind == kChainMaxDensity) {
    k_chainb_density_reset<<<(n_clouds + 63) / 64, 64, 0, s>>>(n_clouds, cl);
    k_chainb_density<false><<<tiles, kChainThreads, 0, s>>>(a.pos, n_clouds, cl, ctl, dens);
    k_chainb_density<true><<<tiles, kChainThreads, 0, s>>>(a.pos, n_clouds, cl, ctl, dens);
  }
  k_chainb_flag<<<tiles, kChainThreads, 0, s>>>(a, n_clouds, cl, ctl, pts, dens, flag, tile_cnt);
  launch_tile_scan(s, tiles, tile_cnt, tile_off, &ctl->n[a.pos + 1]);
  k_chainb_counts<<<n_clouds, 64, 0, s>>>(a.pos, n_clouds, cl, ctl, flag, tile_off);
  // (the one-pair scatter: the concatenation is one stream of ctl->n[pos] rows)
  k_chain_scatter<<<tiles, kChainThreads, 0, s>>>(a.pos, ctl, flag, tile_off, pts, out, nrm, nrm_out, dens, dens_out);
}

bool launch_chainb_sn_out(hipStream_t s, int n_trees, const PairDesc* pd, uint32_t total, int knn, const float4* bpts,
                          const int32_t* ids, const float4* bnrm, float4* nrm, float* dens) {
  if (!total || n_trees < 1) return true;
  switch (knn) {
    case 10: k_chainb_sn_out<10><<<grid_of(total), 256, 0, s>>>(n_trees, pd, total, bpts, ids, bnrm, nrm, dens); break;
    case 20: k_chainb_sn_out<20><<<grid_of(total), 256, 0, s>>>(n_trees, pd, total, bpts, ids, bnrm, nrm, dens); break;
    case 30: k_chainb_sn_out<30><<<grid_of(total), 256, 0, s>>>(n_trees, pd, total, bpts, ids, bnrm, nrm, dens); break;
    default: return false;
  }
  return true;
}

void launch_chainb_rows(hipStream_t s, int n_segs, const ChainSeg* sg, uint32_t total, const float4* in, float4* out,
                        const float4* nrm, float4* nrm_out) {
  if (total && n_segs > 0) k_chainb_rows<<<grid_of(total), 256, 0, s>>>(n_segs, sg, total, in, out, nrm, nrm_out);
}

}  // namespace aicp
