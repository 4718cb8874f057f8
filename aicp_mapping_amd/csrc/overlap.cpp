// overlap.cpp — the octree overlap's host side: the batch's voxel maps
// and sorted key words (overlap_maps, overlap_sparse; run_batch calls the first), and a stream
// window's plan and device steps (ovl_window_*; the frame-to-reference stream and
// aicp_hip_test_overlap call them). The kernels are in kernels_overlap.hip (maps),
// kernels_overlap_sparse.hip (key lists) and kernels_sequence.hip (device-sized window maps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

namespace {

// voxel-map capacity (bytes) of a cloud with AABB b plus origin o at resolution res: `rigid`
// allows any rotation (a rigid motion keeps the diameter; the device sizes the box after the
// transform), otherwise the axis extents. Both include the 2 + 2 voxels of padding, one more
// for the floor of each end, the rounding of the corrected origin, and the brick alignment of
// both box ends (ovl_axis: up to 2 x 7 voxels).
uint64_t map_cap(const Box& b0, const double* o, double res, bool rigid) {
  Box b = b0;
  b.add((float)o[0], (float)o[1], (float)o[2]);
  double ext[3], d2 = 0;
  for (int k = 0; k < 3; ++k) {
    ext[k] = std::max(0.0, (double)b.hi[k] - (double)b.lo[k]);
    d2 += ext[k] * ext[k];
  }
  uint64_t vox = 1;
  double voxd = 1;
  for (int k = 0; k < 3; ++k) {
    const double e = rigid ? std::sqrt(d2) : ext[k];
    const double side = std::ceil(e / res) + 8 + 2 * (kOvlBrick0 - 1);
    voxd *= side;
    // a finite return far outside the key range (1e30 m) must not wrap the product into a small
    // capacity: such a window is over every budget and runs on key lists
    if (!(voxd < 0x1p50)) return uint64_t(1) << 50;  // (4096 such slots still add up within 64 bits)
    vox *= (uint64_t)side;
  }
  return (vox + kOvlBrickBytes - 1) / kOvlBrickBytes * kOvlBrickBytes;
}

}  // namespace

namespace aicp {
namespace rt {

// A window's voxel maps beyond this many bytes (all of them together) take the sorted-key path
// instead: a far return (a key box of 10^9+ voxels) or a very wide scan. The C2/C3 scenes need
// ~3 MB per reading map and ~80 MB for a reference (sized for any rotation of its source).
const uint64_t kSeqMapBudget = uint64_t(1) << 30;

const uint64_t kMaxRayKeys = 3 * 65536 + 8;  // keys are 16-bit per axis: a ray's walk is bounded

// Upper bound of the keys computeRayKeys(o, p) + p's own key visit, summed over a cloud: one
// step per key crossed on an axis, plus the origin, the endpoint and a margin for the walk's
// float overshoot. rigid: for any rigid motion of both cloud and origin (the corrected reference
// of the next window), from the distance: sum_i |dk_i| <= sqrt(3) |p - o| / res + 3.
// A point without a key (non-finite or beyond the key range) visits nothing.
uint64_t key_bound(WorkerPool& pool, const aicp_cloud& c, const double* org, double res, bool rigid) {
  constexpr uint64_t kChunk = 1 << 15;
  const size_t tasks = (size_t)((c.n + kChunk - 1) / kChunk);
  std::vector<uint64_t> part(tasks, 0);
  const double rf = 1.0 / res;
  const float of[3] = {(float)org[0], (float)org[1], (float)org[2]};
  double ko[3];
  for (int k = 0; k < 3; ++k) ko[k] = std::floor(rf * (double)of[k]);
  pool.run(tasks, [&](size_t t) {
    const char* src = reinterpret_cast<const char*>(c.pts);
    uint64_t sum = 0;
    const uint64_t a = t * kChunk, b = std::min<uint64_t>(c.n, a + kChunk);
    for (uint64_t i = a; i < b; ++i) {
      const float* p = reinterpret_cast<const float*>(src + i * c.stride);
      if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) continue;
      double v;
      if (rigid) {
        double d2 = 0;
        for (int k = 0; k < 3; ++k) d2 += ((double)p[k] - org[k]) * ((double)p[k] - org[k]);
        v = std::ceil(1.7320508075688772 * (std::sqrt(d2) * (1 + 1e-5) + 1e-3) * rf) + 8;
      } else {
        v = 8;
        for (int k = 0; k < 3; ++k) v += std::fabs(std::floor(rf * (double)p[k]) - ko[k]);
      }
      sum += v < (double)kMaxRayKeys ? (uint64_t)v : kMaxRayKeys;
    }
    part[t] = sum;
  });
  uint64_t s = 0;
  for (uint64_t v : part) s += v;
  return s;
}

// voxel maps: [0] the reference (capacity for any rigid motion of its source), [1 + i] readings
void ovl_window_slots(OvlWinPlan& W, const Box& src_box, const double* src_origin, bool src_rigid, const Box* boxes,
                      const aicp_cloud* reads, size_t np, double res, bool read_rigid) {
  W.od.assign(np + 1, OvlDesc{});
  W.cap.assign(np + 1, 0);
  W.bm = W.cap_max = 0;
  for (size_t i = 0; i <= np; ++i) {
    W.cap[i] = i == 0 ? map_cap(src_box, src_origin, res, src_rigid)
                      : map_cap(boxes[i - 1], reads[i - 1].origin, res, read_rigid);  // debug: moved by initialT_
    W.od[i].off = W.bm;
    W.bm += W.cap[i];
    W.cap_max = std::max(W.cap_max, W.cap[i]);
  }
}

// key lists sized by host bounds of the rays' keys (readings from their own points; the reference
// for any rigid motion of its source), so the stream needs no read-back
void ovl_window_keys(OvlWinPlan& W, WorkerPool& pool, const aicp_cloud& src, const double* ref_origin, bool ref_rigid,
                     const aicp_cloud* reads, const uint32_t* loff, size_t np, double res, bool read_rigid) {
  W.scl.clear();
  W.sbc.clear();
  W.sbs.clear();
  W.kb_read.clear();
  W.cap_r = W.cap_g = 0;
  uint64_t slot = 0;
  for (size_t i = 0; i <= np; ++i) {  // readings 0..np-1, then the reference
    const bool ref = i == np;
    const aicp_cloud& c = ref ? src : reads[i];
    OvlCloud o{};
    o.pts_off = ref ? 0u : loff[i];
    o.n = (uint32_t)c.n;
    o.side = ref ? 0u : 1u;
    for (int k = 0; k < 3; ++k) o.origin[k] = ref ? ref_origin[k] : c.origin[k];
    o.slot = ref ? 0 : slot;
    slot += ref ? 0 : c.n;
    W.scl.push_back(o);
    const uint32_t ci = ref ? 0u : (uint32_t)i;
    for (uint32_t j = 0; j < o.n; j += 256) {
      W.sbc.push_back(ci);
      W.sbs.push_back(j);
    }
    const uint64_t kb = key_bound(pool, c, c.origin, res, ref ? ref_rigid : read_rigid);
    if (!ref) W.kb_read.push_back(kb);
    (ref ? W.cap_g : W.cap_r) += kb;
  }
}

void ovl_window_sides(const OvlWinPlan& W, size_t np, uint64_t nread, uint32_t n_ref, OvlCloud* dcl,
                      const uint32_t* dbc, uint32_t* cnt, uint64_t* off, uint64_t* keys_r, uint64_t* keys_g,
                      void* tmp_r, size_t tmp_rb, void* tmp_g, size_t tmp_gb, unsigned long long* pc, OvlKeySide& kr,
                      OvlKeySide& kg) {
  const size_t nb = W.sbc.size();
  const uint32_t* dbs = dbc + nb;
  const uint32_t nbr = (uint32_t)(nb - (n_ref + 255) / 256);  // the readings' blocks come first
  kr = OvlKeySide{dcl, (int)np, dbc, dbs, nbr, (uint32_t)nread, cnt, off, W.cap_r, keys_r, keys_r + W.cap_r,
                  tmp_r, tmp_rb, pc};
  kg = OvlKeySide{dcl + np, 1, dbc + nbr, dbs + nbr, (uint32_t)(nb - nbr), n_ref, cnt + nread, off + nread,
                  W.cap_g, keys_g, keys_g + W.cap_g, tmp_g, tmp_gb, pc + np};
}

// one side's voxel maps (or key list) and its |S|: side 1 the np readings (|B|), side 0 the
// reference (|A|); origin0 (nullable): the reference's origin where the device wrote it
int ovl_window_side(std::string& err, hipStream_t s, const OvlWinDev& D, int side, const double* origin0,
                    const float4* pts) {
  const int n = side ? (int)D.np : 1;
  const PairDesc* pd = side ? D.dDesc : D.dG;
  PairState* st = side ? D.dState : D.dGst;
  launch_ovl_init(s, n, pd, st, D.res, side ? 2 : 1);
  if (D.sparse) {
    TCHK(launch_ovl_keys(s, side ? *D.kr : *D.kg, origin0, pts, D.res, st, side));
  } else {
    OvlDesc* od = D.dOvl + side;  // slot 0 the reference's, then the readings'
    launch_ovl_bbox(s, side ? D.m_read : D.m_gref, pd, st, pts, side, D.res);
    launch_ovl_size(s, n, st, od, D.dCap + side);
    launch_ovl_clear(s, n, od, D.bmp, side ? D.cap_max : D.cap0);
    launch_ovl_mark(s, side ? D.m_read : D.m_gref, pd, od, st, pts, side, D.res, D.bmp, D.filter);
    launch_ovl_popcount(s, n, od, st, side, D.bmp, D.wide);
  }
  return AICP_OK;
}

// |A ∩ B| of every reading, the percentage and the ratio
int ovl_window_counts(std::string& err, hipStream_t s, const OvlWinDev& D) {
  if (D.sparse)
    TCHK(launch_ovl_keys_intersect(s, *D.kr, *D.kg, 0, nullptr, D.per_pair, nullptr, D.dState));
  else
    launch_ovl_intersect(s, (int)D.np, D.dDesc, D.dOvl + 1, D.dOvl, D.dState, D.bmp, D.wide);
  launch_ovl_finish(s, (int)D.np, D.dDesc, D.dState, D.dGst, 1);
  return AICP_OK;
}

// ---- the batch ----

// The overlap from sorted key words (kernels_overlap_sparse.hip) when the dense voxel maps of a
// batch do not fit: one key side of the G groups then the P readings; counts per point -> offsets
// (one host read of the total, which sizes the list exactly) -> words -> sort -> distinct counts
// and intersections. Same sets, same counts as the maps.
static int overlap_sparse(aicp_hip_ctx* ctx, aicp_hip_batch* B, size_t P, size_t G, PairDesc* dDesc, PairState* dState,
                   PairState* dGst, const float4* readS, double res, bool set_ratio, std::string& err) {
  hipStream_t s = ctx->stream;
  std::vector<OvlCloud> cl(G + P);
  std::vector<uint32_t> bc, bs;
  uint64_t slots = 0;
  for (size_t c = 0; c < G + P; ++c) {
    OvlCloud& o = cl[c];
    o = OvlCloud{};
    const PairDesc& d = c < G ? B->gdesc[c] : B->desc[c - G];
    o.side = c < G ? 0 : 1;
    o.pts_off = c < G ? d.ref_off : d.read_off;
    o.n = c < G ? d.n_ref : d.n_read;
    for (int k = 0; k < 3; ++k) o.origin[k] = c < G ? d.ref_origin[k] : d.read_origin[k];
    o.slot = slots;
    slots += o.n;
    for (uint32_t j = 0; j < o.n; j += 256) {
      bc.push_back((uint32_t)c);
      bs.push_back(j);
    }
  }
  if (slots >= (1ull << 32)) TFAIL(AICP_ERR_UNSUPPORTED, "sparse overlap: more than 2^32 points");
  const size_t nb = bc.size();
  const size_t scan_b = ovl_keys_temp_bytes(slots, 0, (int)(G + P));
  const size_t o_cl = 0, o_bc = o_cl + (G + P) * sizeof(OvlCloud), o_bs = o_bc + nb * 4,
               o_cnt = (o_bs + nb * 4 + 255) & ~size_t(255), o_off = (o_cnt + slots * 4 + 255) & ~size_t(255),
               o_pc = o_off + slots * 8, o_pp = o_pc + (G + P) * 8, o_tmp = (o_pp + P * 8 + 255) & ~size_t(255);
  TCHK(ensure(ctx->ovl_sp, o_tmp + scan_b));
  const size_t o_tail = (o_bs + nb * 4 + 7) & ~size_t(7);  // read-back of the key total
  TCHK(ensure(ctx->pin_ovl, o_tail + 16));
  char* h = ctx->pin_ovl.as<char>();
  std::memcpy(h + o_cl, cl.data(), (G + P) * sizeof(OvlCloud));
  std::memcpy(h + o_bc, bc.data(), nb * 4);
  std::memcpy(h + o_bs, bs.data(), nb * 4);
  char* d = ctx->ovl_sp.as<char>();
  TCHK(hipMemcpyAsync(d, h, o_bs + nb * 4, hipMemcpyHostToDevice, s));
  TCHK(hipEventRecord(ctx->ev[6], s));
  uint32_t* cnt = (uint32_t*)(d + o_cnt);
  uint64_t* off = (uint64_t*)(d + o_off);
  OvlKeySide k{(OvlCloud*)(d + o_cl), (int)(G + P), (const uint32_t*)(d + o_bc), (const uint32_t*)(d + o_bs),
               (uint32_t)nb, (uint32_t)slots, cnt, off, 0, nullptr, nullptr, d + o_tmp, scan_b,
               (unsigned long long*)(d + o_pc)};
  const float4* refS = B->ref_raw.as<float4>();
  TCHK(launch_ovl_keys_count(s, k, nullptr, refS, readS, res));
  uint64_t* tail = (uint64_t*)(h + o_tail);
  TCHK(hipMemcpyAsync(tail, off + (slots - 1), 8, hipMemcpyDeviceToHost, s));
  uint32_t* tailc = (uint32_t*)(tail + 1);
  TCHK(hipMemcpyAsync(tailc, cnt + (slots - 1), 4, hipMemcpyDeviceToHost, s));
  TCHK(hipStreamSynchronize(s));
  const uint64_t n_keys = slots ? tail[0] + tailc[0] : 0;
  const size_t sort_b = ovl_keys_temp_bytes(slots, n_keys, (int)(G + P));
  size_t free_b = 0, total_b = 0;
  TCHK(hipMemGetInfo(&free_b, &total_b));
  if (n_keys * 16 + sort_b > ctx->ovl_keys.cap + free_b / 2)
    TFAIL(AICP_ERR_UNSUPPORTED, "sparse overlap: " + std::to_string(n_keys) + " ray keys do not fit");
  TCHK(ensure(ctx->ovl_keys, n_keys * 16 + sort_b + 256));
  k.cap = n_keys;  // exact: no pad words
  k.keys0 = ctx->ovl_keys.as<uint64_t>();
  k.keys1 = k.keys0 + n_keys;
  k.temp = (void*)(((uintptr_t)(k.keys1 + n_keys) + 255) & ~uintptr_t(255));
  k.temp_bytes = sort_b;
  TCHK(launch_ovl_keys_sets(s, k, refS, readS, res, nullptr, 0));
  TCHK(launch_ovl_keys_intersect(s, k, k, (int)G, dDesc, (unsigned long long*)(d + o_pp), dGst, dState));
  launch_ovl_finish(s, (int)P, dDesc, dState, dGst, set_ratio || ctx->ovl_probe.on ? 1 : 0);
  TCHK(hipGetLastError());
  if (ctx->ovl_probe.on) {
    OvlProbe& probe = ctx->ovl_probe;
    probe.ran_path = 2;
    probe.ran_filter = probe.ran_wide = 0;
    probe.n_points = slots;
    probe.n_keys = n_keys;
    probe.cnt = cnt;
    probe.off = off;
    probe.keys1 = k.keys1;
  }
  return AICP_OK;
}

// dense voxel maps of one batch beyond this size take the sorted-key path instead (a 60 x 60 x 6 m
// scene at 0.2 m is ~2.7 MB per map; 8 GiB covers thousands of such clouds)
constexpr uint64_t kDenseMapBudget = uint64_t(8) << 30;

// The overlap's second half on stream s (the first, the key boxes, is queued before the trees):
// wait for the boxes, size one byte map per reading and per reference group, mark, count,
// ratio. Runs on its own host thread while the main thread queues the trees, so the marking
// starts as soon as the boxes are known instead of after the raw tree's host polls.
int overlap_maps(aicp_hip_ctx* ctx, aicp_hip_batch* B, size_t P, size_t G, PairDesc* dDesc, PairState* dState,
                 PairDesc* dG, PairState* dGst, const float4* readS, double res, bool set_ratio, std::string& err) {
  hipStream_t s = ctx->stream;
  TCHK(hipSetDevice(ctx->device));
  TCHK(hipEventSynchronize(ctx->ev[1]));
  RefCache& rc = ctx->refc;
  const bool hit = rc.hit_ovl;  // the one group's map is the cached reference's (ctx->bitmap[0, rc.od.bytes))
  OvlProbe& probe = ctx->ovl_probe;
  set_ratio = set_ratio || probe.on;
  if (ctx->opt.overlap_path == 1 || (probe.on && probe.keys)) {  // the sorted-key path for every batch (tests)
    rc.ovl = false;
    return overlap_sparse(ctx, B, P, G, dDesc, dState, dGst, readS, res, set_ratio, err);
  }
  // one map per overlap group (reference side) and one per pair (reading side), each over
  // the padded key box of that cloud's keys and origin; the groups' maps first, so a cached
  // reference's map keeps its place at offset 0
  uint64_t bm_bytes = 0;
  TCHK(ensure(ctx->pin_ovl, (P + G) * sizeof(OvlDesc)));
  TCHK(ensure(ctx->ovl, (P + G) * sizeof(OvlDesc)));
  OvlDesc* ho = ctx->pin_ovl.as<OvlDesc>();
  auto size_map = [&](const PairState& hs, OvlDesc& o) -> bool {
    const int br[3] = {kOvlBrick0, kOvlBrick1, kOvlBrick2};
    for (int k = 0; k < 3; ++k) ovl_axis(hs.ovl_bbox[k], hs.ovl_bbox[3 + k], br[k], o.min[k], o.dim[k]);
    const uint64_t vox = ovl_bytes(o.dim);
    o.bytes = vox;
    o.off = bm_bytes;
    bm_bytes += o.bytes;
    return vox <= (1ull << 34);
  };
  bool fits = true;
  if (hit) {
    ho[P] = rc.od;
    bm_bytes = rc.od.bytes;
  } else {
    for (size_t g = 0; g < G; ++g) fits &= size_map(ctx->pin_gstate.as<PairState>()[g], ho[P + g]);
  }
  const uint64_t ref_bytes = bm_bytes;
  for (size_t i = 0; i < P; ++i) fits &= size_map(ctx->pin_state.as<PairState>()[i], ho[i]);
  // all maps of the batch at once within half the free device memory (beyond what the arena
  // already holds); otherwise (far outlier points: key boxes of 10^9+ voxels) the sorted-key path
  size_t free_b = 0, total_b = 0;
  TCHK(hipMemGetInfo(&free_b, &total_b));
  const uint64_t limit = std::min<uint64_t>(ctx->bitmap.cap + free_b / 2, kDenseMapBudget);
  if (!fits || bm_bytes > limit) {  // (a cached group state is in dGst; the sparse path recounts |A|)
    rc.ovl = false;
    return overlap_sparse(ctx, B, P, G, dDesc, dState, dGst, readS, res, set_ratio, err);
  }
  if (hit && bm_bytes > ctx->bitmap.cap) {  // grow, keeping the cached map
    DevBuf nb;
    hipError_t e = ensure(nb, bm_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(nb.p, ctx->bitmap.p, ref_bytes, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) release(nb);  // (a DevBuf is not released by its destructor)
    TCHK(e);
    release(ctx->bitmap);
    ctx->bitmap = nb;
  }
  TCHK(ensure(ctx->bitmap, bm_bytes));
  TCHK(hipMemcpyAsync(ctx->ovl.p, ho, (P + G) * sizeof(OvlDesc), hipMemcpyHostToDevice, s));
  TCHK(hipEventRecord(ctx->ev[6], s));
  uint8_t* bm = ctx->bitmap.as<uint8_t>();
  const OvlDesc* dOvl = ctx->ovl.as<OvlDesc>();
  // the marks' LDS cache of stored voxels pays off where many rays share the maps (C5: 66 against
  // 111 GB written per dispatch); a few clouds mark faster with plain stores (the
  // stream's measurement)
  const bool filter = probe.on && probe.filter >= 0 ? probe.filter != 0 : P + G > 8;
  // the counts' wide grids for the one-shot call of one pair alone (count_bpm, kernels_overlap.hip)
  const bool wide = probe.on && probe.wide >= 0 ? probe.wide != 0 : P + G <= 2;
  if (probe.on) {
    probe.ran_path = 1;
    probe.ran_filter = filter;
    probe.ran_wide = wide;
    probe.arena_bytes = bm_bytes;
  }
  if (hit) {  // the readings' maps only: the reference's map and |A| are the cached ones
    TCHK(hipMemsetAsync(bm + ref_bytes, 0, bm_bytes - ref_bytes, s));
    launch_ovl_mark(s, B->m_read, dDesc, dOvl, dState, readS, 1, res, bm, filter);
    launch_ovl_popcount(s, (int)P, dOvl, dState, 1, bm, P == 1);
    launch_ovl_intersect(s, (int)P, dDesc, dOvl, dOvl + P, dState, bm, P == 1);
    ++rc.ovl_hits;
  } else {
    TCHK(hipMemsetAsync(bm, 0, bm_bytes, s));
    launch_ovl_mark(s, B->m_gref, dG, dOvl + P, dGst, B->ref_raw.as<float4>(), 0, res, bm, filter);
    launch_ovl_mark(s, B->m_read, dDesc, dOvl, dState, readS, 1, res, bm, filter);
    launch_ovl_count(s, (int)P, (int)G, dDesc, dOvl, dOvl + P, dState, dGst, bm, wide);
    rc.ovl = false;
    if (rc.use && G == 1) {  // keep the reference's map (offset 0) and its group state for the next call
      TCHK(ensure(rc.gst, sizeof(PairState)));
      TCHK(hipMemcpyAsync(rc.gst.p, dGst, sizeof(PairState), hipMemcpyDeviceToDevice, s));
      rc.ovl = true;
      rc.od = ho[P];
      rc.res = res;
      for (int k = 0; k < 3; ++k) rc.origin[k] = B->gdesc[0].ref_origin[k];
      ++rc.ovl_builds;
    }
  }
  launch_ovl_finish(s, (int)P, dDesc, dState, dGst, set_ratio ? 1 : 0);
  TCHK(hipGetLastError());
  return AICP_OK;
}

}  // namespace rt
}  // namespace aicp
