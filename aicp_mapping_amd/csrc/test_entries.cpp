// test_entries.cpp — the kernel-level test surface of libaicp_hip.so, every aicp_hip_test_* entry
// point: production kernels behind the launches the production path gives them, on given inputs,
// and everything they wrote handed back (tests/test_*_kernels.py). Every entry checks all of its
// arguments before it touches the device or the context; the helpers here are called after that.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

namespace {

// Total and maximum (nullable) of n counts; false for a zero entry or a total at or above `limit`.
bool count_check(const uint32_t* c, size_t n, uint64_t limit, uint64_t* total, uint64_t* max = nullptr) {
  uint64_t sum = 0, top = 0;
  for (size_t i = 0; i < n; ++i) {
    if (c[i] == 0) return false;
    sum += c[i];
    top = std::max<uint64_t>(top, c[i]);
  }
  *total = sum;
  if (max) *max = top;
  return sum < limit;
}

// The descriptors of R references laid end to end, as upload_pairs makes them
std::vector<PairDesc> ref_descs(const uint32_t* counts, size_t R) {
  std::vector<PairDesc> rd(R, PairDesc{});
  uint32_t off = 0;
  for (size_t r = 0; r < R; ++r) {
    rd[r].ref_off = off;
    rd[r].n_ref = counts[r];
    rd[r].ratio = 0.5f;
    rd[r].ref_id = (int32_t)r;
    ident4(rd[r].Tin);
    off += counts[r];
  }
  return rd;
}

// Device buffers of one call, freed on every return (get()'s references stay valid: a deque);
// sync: a stream to wait for first, where a return can leave work on them in flight
struct CallBufs {
  std::deque<DevBuf> bufs;
  hipStream_t sync = nullptr;
  DevBuf& get() {
    bufs.emplace_back();
    return bufs.back();
  }
  ~CallBufs() {
    if (sync) (void)hipStreamSynchronize(sync);
    for (DevBuf& b : bufs) release(b);
  }
};

constexpr size_t kGuard = 64;  // guard words on each side of a guarded array

// changed words among the kGuard guard words of `word_bytes` (4 or 8) bytes at g, of a host copy
uint64_t guard_dirty(const void* g, size_t word_bytes, uint64_t fill) {
  uint64_t n = 0;
  for (size_t k = 0; k < kGuard; ++k)
    n += std::memcmp(static_cast<const char*>(g) + k * word_bytes, &fill, word_bytes) != 0;  // (little-endian)
  return n;
}

// A call-local array of n 4-byte words with kGuard guard words on both sides, all of it filled
// with a sentinel before the kernels under test write the payload.
struct Guarded {
  DevBuf* b = nullptr;
  size_t n = 0;
  uint32_t fill = 0;
  size_t words() const { return n + 2 * kGuard; }
  hipError_t alloc(CallBufs& loc, size_t payload_words, uint32_t sentinel) {
    b = &loc.get();
    n = payload_words;
    fill = sentinel;
    return ensure(*b, words() * 4);
  }
  hipError_t refill(hipStream_t s) const { return hipMemsetD32Async((hipDeviceptr_t)b->p, (int)fill, words(), s); }
  void* payload() const { return b->as<uint32_t>() + kGuard; }
  // from a host copy of all words(): the payload to out, the changed guard words added to dirty
  void take(const uint32_t* back, void* out, uint64_t& dirty) const {
    dirty += guard_dirty(back, 4, fill) + guard_dirty(back + kGuard + n, 4, fill);
    std::memcpy(out, back + kGuard, n * 4);
  }
  hipError_t fetch(std::vector<uint32_t>& back, void* out, uint64_t& dirty) const {  // (blocking)
    back.resize(std::max(back.size(), words()));
    const hipError_t e = hipMemcpy(back.data(), b->p, words() * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) take(back.data(), out, dirty);
    return e;
  }
};

// n packed xyz points as float4 (w = 1) onto the device, through pk (blocking)
hipError_t upload_xyz4(std::vector<float>& pk, const float* xyz, uint64_t n, void* dst) {
  pk.resize(std::max<size_t>(pk.size(), 4 * (size_t)n));
  pack_xyz4(xyz, n, 12, pk.data());
  return hipMemcpy(dst, pk.data(), n * 16, hipMemcpyHostToDevice);
}

// The batched kd-tree build of R clouds (ctx->ref1; the largest has n_max points) enqueued on
// ctx->stream with run_batch's plan: set 1 the matcher's (tb[1], ctx->bpts / nodes), set 0 the raw
// trees' (tb[0], bpts_raw / nodes_raw, the lean plan). The wait and device_trees_check stay the
// caller's (the entries differ in what comes first). *begun (nullable): device_trees_begin succeeded.
int enqueue_trees(aicp_hip_ctx* ctx, int set, size_t R, uint64_t total, uint64_t n_max, PairDesc* dDesc, int center,
                  int bucket, bool* begun = nullptr) {
  const bool raw = set == 0;
  TreeBufs& T = ctx->tb[set];
  DevBuf& bpts = raw ? ctx->bpts_raw : ctx->bpts;
  DevBuf& nodes = raw ? ctx->nodes_raw : ctx->nodes;
  const int rc = device_trees_begin(T, ctx->err, ctx->stream, R, total, dDesc, ctx->ref1.as<float4>(), center, bucket,
                                    bpts, nodes);
  if (rc) return rc;
  if (begun) *begun = true;
  return device_trees_end(T, ctx->err, ctx->stream, R, total, dDesc, bucket, bpts, nodes,
                          plan_levels(n_max, T, ctx->opt.tree_plan, raw));
}

// The ICP loop's set-up as run_batch makes it, for P pairs whose readings lie end to end: the
// descriptors, the block map of `granule` readings a block, zeroed arrival and NN counters, states
// from launch_init_state (behind a memset with zero_state), per pair then its T (init_T, nullable)
// and a cleared `active` (active, nullable); *m the block map, *y the IcpIterSync over all P pairs.
int icp_iter_setup(aicp_hip_ctx* ctx, const std::vector<PairDesc>& desc, uint32_t granule, bool zero_state,
                   const float* init_T, const uint8_t* active, BlockMap* m, IcpIterSync* y) {
  const size_t P = desc.size();
  hipStream_t s = ctx->stream;
  Maps ms;
  for (size_t p = 0; p < P; ++p) ms.add((int)p, desc[p].n_read, granule);
  const size_t nb = ms.pair.size();
  const uint64_t total = (uint64_t)desc[P - 1].read_off + desc[P - 1].n_read;
  HIPC(ensure(ctx->desc, P * sizeof(PairDesc)));
  HIPC(ensure(ctx->state, P * sizeof(PairState)));
  HIPC(ensure(ctx->qmap, nb * 8));
  HIPC(ensure(ctx->isync, icp_sync_words(P) * 4));
  HIPC(ensure(ctx->active, active_list_bytes(total, P)));
  HIPC(ensure(ctx->ctrs, kCtrWords * 4));
  PairDesc* dDesc = ctx->desc.as<PairDesc>();
  PairState* dState = ctx->state.as<PairState>();
  uint32_t* sync = ctx->isync.as<uint32_t>();
  HIPC(hipMemcpy(dDesc, desc.data(), P * sizeof(PairDesc), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->qmap.p, ms.pair.data(), nb * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->qmap.as<uint32_t>() + nb, ms.start.data(), nb * 4, hipMemcpyHostToDevice));
  *m = BlockMap{ctx->qmap.as<int32_t>(), ctx->qmap.as<uint32_t>() + nb, (uint32_t)nb};
  HIPC(hipMemsetAsync(sync, 0, icp_sync_words(P) * 4, s));
  HIPC(hipMemsetAsync(ctx->ctrs.p, 0, kCtrWords * 4, s));
  if (zero_state) HIPC(hipMemsetAsync(dState, 0, P * sizeof(PairState), s));
  launch_init_state(s, (int)P, dDesc, dState);
  for (size_t p = 0; p < P; ++p) {
    if (init_T) HIPC(hipMemcpyAsync(dState[p].T, init_T + 16 * p, 64, hipMemcpyHostToDevice, s));
    if (active && !active[p]) HIPC(hipMemsetAsync(&dState[p].active, 0, sizeof(int32_t), s));
  }
  *y = icp_iter_sync(sync, P, (int)P, dDesc, dState, ctx->active.as<ActiveList>(), ctx->ctrs.as<uint32_t>());
  return AICP_OK;
}

// aicp_hip_test_overlap's outputs: cloud c (groups, then readings) from its state, pair p from
// its state, cloud c's map descriptor (its offset counted from `base`)
void put_cloud(aicp_test_overlap_out* out, size_t c, const PairState& st, bool group) {
  out->cloud_keys[c] = st.ovl_counts[group ? 0 : 1];
  out->cloud_err[c] = st.ovl_err;
  for (int k = 0; k < 6; ++k) out->cloud_bbox[6 * c + k] = st.ovl_bbox[k];
}
void put_pair(aicp_test_overlap_out* out, size_t p, const PairState& st) {
  for (int k = 0; k < 3; ++k) out->pair_counts[3 * p + k] = st.ovl_counts[k];
  out->pair_percent[p] = st.overlap;
  out->pair_ratio[p] = st.ratio;
  out->pair_err[p] = st.ovl_err;
}
void put_desc(aicp_test_overlap_out* out, size_t c, const OvlDesc& o, uint64_t base) {
  for (int k = 0; k < 3; ++k) {
    out->desc_min[3 * c + k] = o.min[k];
    out->desc_dim[3 * c + k] = o.dim[k];
  }
  out->desc_off[c] = base + o.off;
  out->desc_bytes[c] = o.bytes;
}

// aicp_hip_test_overlap's paths 3 and 4: each overlap group of the batch as one stream window, on
// buffers of this call, through the plan and the device steps the stream itself calls (path 3 maps
// sized on the device, 4 capped key lists); caps (nullable): explicit capacities per cloud, groups
// then readings (bytes, or key words). Fills out's per-cloud and per-pair fields, the descriptors
// and arena or the lists; out->dirty: changed guard words of its own buffers.
int ovl_window_test(aicp_hip_ctx* ctx, const aicp_hip_batch* B, const aicp_pair* pairs, double res, int path,
                    int filter, int wide, const uint64_t* caps, int rigid, aicp_test_overlap_out* out) {
  const size_t P = B->P, G = B->gdesc.size();
  hipStream_t s = ctx->stream;
  WorkerPool pool{0};
  constexpr uint32_t kFill32 = 0xA5A5A5A5u;  // (guard words of 8 bytes here)
  constexpr uint64_t kFill64 = 0xA5A5A5A5A5A5A5A5ull;
  const bool sparse = path == 4;
  out->path = path;
  out->filter = sparse ? 0 : (filter > 0);
  out->wide = sparse ? 0 : (wide > 0);
  out->n_groups = (int32_t)G;
  out->arena_bytes = out->n_points = out->n_words = out->dirty = 0;
  for (size_t p = 0; p < P; ++p) out->pair_group[p] = B->desc[p].ogroup;
  uint64_t ref_pts_before = 0, total_ref_pts = 0, total_read_pts = 0;
  for (size_t g = 0; g < G; ++g) total_ref_pts += B->gdesc[g].n_ref;
  std::vector<uint64_t> read_first(P + 1, 0);
  for (size_t p = 0; p < P; ++p) read_first[p + 1] = read_first[p] + pairs[p].n_read;
  total_read_pts = read_first[P];
  if (sparse && total_ref_pts + total_read_pts > out->points_cap) FAIL(AICP_ERR_INVALID, "points_cap");
  if (sparse) out->n_points = total_ref_pts + total_read_pts;
  for (size_t g = 0; g < G; ++g) {
    CallBufs loc;
    loc.sync = s;
    std::vector<size_t> idx;
    for (size_t p = 0; p < P; ++p)
      if ((size_t)B->desc[p].ogroup == g) idx.push_back(p);
    const size_t np = idx.size();
    const aicp_pair& p0 = pairs[idx[0]];
    aicp_cloud src{p0.ref, p0.n_ref, p0.ref_stride, {p0.ref_origin[0], p0.ref_origin[1], p0.ref_origin[2]}};
    const uint32_t n_ref = (uint32_t)src.n;
    std::vector<aicp_cloud> reads(np);
    std::vector<uint32_t> loff(np);
    uint64_t nread = 0;
    for (size_t i = 0; i < np; ++i) {
      const aicp_pair& q = pairs[idx[i]];
      reads[i] = aicp_cloud{q.read, q.n_read, q.read_stride, {q.read_origin[0], q.read_origin[1], q.read_origin[2]}};
      loff[i] = (uint32_t)nread;
      nread += q.n_read;
    }
    // pack (+ AABBs), descriptors, block maps: as the stream's window upload
    std::vector<float> h_read(4 * nread), h_ref(4 * (size_t)n_ref);
    std::vector<PackSeg> segs;
    for (size_t i = 0; i < np; ++i)
      segs.push_back(PackSeg{reads[i].pts, reads[i].n, reads[i].stride, h_read.data() + 4 * (size_t)loff[i]});
    segs.push_back(PackSeg{src.pts, src.n, src.stride, h_ref.data()});
    std::vector<Box> boxes;
    pack_clouds(pool, segs, boxes);
    Maps mr, mg;
    std::vector<PairDesc> hd(np + 1, PairDesc{});  // the readings, then the group
    for (size_t i = 0; i < np; ++i) {
      PairDesc& d = hd[i];
      d.n_ref = n_ref;
      d.read_off = loff[i];
      d.n_read = (uint32_t)reads[i].n;
      ident4(d.Tin);
      d.ratio = 0.7f;
      for (int k = 0; k < 3; ++k) {
        d.read_origin[k] = reads[i].origin[k];
        d.ref_origin[k] = src.origin[k];
      }
      mr.add((int)i, d.n_read, kNNBlock);
    }
    hd[np].n_ref = n_ref;
    ident4(hd[np].Tin);
    for (int k = 0; k < 3; ++k) hd[np].ref_origin[k] = src.origin[k];
    mg.add(0, n_ref, kNNBlock);
    OvlWinPlan W;
    uint64_t cap_r = 0, cap_g = 0;
    size_t tmp_rb = 0, tmp_gb = 0;
    if (!sparse) {
      ovl_window_slots(W, boxes[np], src.origin, rigid != 0, boxes.data(), reads.data(), np, res, false);
      if (caps) {
        W.bm = W.cap_max = 0;
        for (size_t i = 0; i <= np; ++i) {
          W.cap[i] = i == 0 ? caps[g] : caps[G + idx[i - 1]];
          W.od[i].off = W.bm;
          W.bm += (W.cap[i] + 127) & ~uint64_t(127);  // (the maps stay 128-byte aligned)
          W.cap_max = std::max(W.cap_max, W.cap[i]);
        }
      }
      if (W.bm > kSeqMapBudget)
        FAIL(AICP_ERR_UNSUPPORTED, "the window's voxel maps exceed the stream's budget: it runs on key lists");
      out->cloud_bound[g] = W.cap[0];
      for (size_t i = 0; i < np; ++i) out->cloud_bound[G + idx[i]] = W.cap[1 + i];
    } else {
      ovl_window_keys(W, pool, src, src.origin, rigid != 0, reads.data(), loff.data(), np, res, false);
      if (caps) {
        W.cap_g = caps[g];
        W.cap_r = 0;
        for (size_t i = 0; i < np; ++i) W.cap_r += (W.kb_read[i] = caps[G + idx[i]]);
      }
      cap_r = W.cap_r;
      cap_g = W.cap_g;
      out->cloud_bound[g] = cap_g;
      for (size_t i = 0; i < np; ++i) out->cloud_bound[G + idx[i]] = W.kb_read[i];
      tmp_rb = ovl_keys_temp_bytes(nread, cap_r, (int)np);
      tmp_gb = ovl_keys_temp_bytes(n_ref, cap_g, 1);
      size_t free_b = 0, total_b = 0;
      HIPC(hipMemGetInfo(&free_b, &total_b));
      if (16 * (cap_r + cap_g) + tmp_rb + tmp_gb > free_b / 2)
        FAIL(AICP_ERR_UNSUPPORTED, "sparse overlap: " + std::to_string(cap_r + cap_g) + " ray keys do not fit");
    }
    // device: points, descriptors, states, block maps
    DevBuf &d_read = loc.get(), &d_ref = loc.get(), &d_desc = loc.get(), &d_state = loc.get(), &d_maps = loc.get();
    HIPC(ensure(d_read, nread * 16));
    HIPC(ensure(d_ref, (size_t)n_ref * 16));
    HIPC(ensure(d_desc, (np + 1) * sizeof(PairDesc)));
    HIPC(ensure(d_state, (np + 1) * sizeof(PairState)));
    const size_t nr = mr.pair.size(), nf = mg.pair.size();
    std::vector<uint32_t> hm(2 * (nr + nf));
    std::memcpy(hm.data(), mr.pair.data(), nr * 4);
    std::memcpy(hm.data() + nr, mr.start.data(), nr * 4);
    std::memcpy(hm.data() + 2 * nr, mg.pair.data(), nf * 4);
    std::memcpy(hm.data() + 2 * nr + nf, mg.start.data(), nf * 4);
    HIPC(ensure(d_maps, hm.size() * 4));
    HIPC(hipMemcpy(d_read.p, h_read.data(), nread * 16, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_ref.p, h_ref.data(), (size_t)n_ref * 16, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_desc.p, hd.data(), (np + 1) * sizeof(PairDesc), hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_maps.p, hm.data(), hm.size() * 4, hipMemcpyHostToDevice));
    HIPC(hipMemsetAsync(d_state.p, 0, (np + 1) * sizeof(PairState), s));
    PairDesc* dDesc = d_desc.as<PairDesc>();
    PairState* dState = d_state.as<PairState>();
    launch_init_state(s, (int)np + 1, dDesc, dState);
    OvlWinDev D;
    D.sparse = sparse;
    D.np = np;
    D.res = res;
    D.dDesc = dDesc;
    D.dState = dState;
    D.dG = dDesc + np;
    D.dGst = dState + np;
    D.m_read = BlockMap{d_maps.as<int32_t>(), d_maps.as<uint32_t>() + nr, (uint32_t)nr};
    D.m_gref = BlockMap{d_maps.as<int32_t>() + 2 * nr, d_maps.as<uint32_t>() + 2 * nr + nf, (uint32_t)nf};
    D.filter = filter > 0;
    D.wide = wide > 0;
    OvlKeySide kr{}, kg{};
    DevBuf &d_arena = loc.get(), &d_ovl = loc.get(), &d_cap = loc.get(), &d_par = loc.get(), &d_cnt = loc.get(),
           &d_off = loc.get(), &d_kr = loc.get(), &d_kg = loc.get(), &d_tr = loc.get(), &d_tg = loc.get(),
           &d_pc = loc.get();
    const size_t kr_words = 2 * cap_r + 3 * kGuard, kg_words = 2 * cap_g + 3 * kGuard;
    if (!sparse) {
      HIPC(ensure(d_arena, W.bm + 2 * kGuard * 8));
      HIPC(ensure(d_ovl, (np + 1) * sizeof(OvlDesc)));
      HIPC(ensure(d_cap, (np + 1) * 8));
      HIPC(hipMemsetD32Async((hipDeviceptr_t)d_arena.p, (int)kFill32, (W.bm + 2 * kGuard * 8) / 4, s));
      HIPC(hipMemcpy(d_ovl.p, W.od.data(), (np + 1) * sizeof(OvlDesc), hipMemcpyHostToDevice));
      HIPC(hipMemcpy(d_cap.p, W.cap.data(), (np + 1) * 8, hipMemcpyHostToDevice));
      D.dOvl = d_ovl.as<OvlDesc>();
      D.dCap = d_cap.as<uint64_t>();
      D.bmp = d_arena.as<uint8_t>() + kGuard * 8;
      D.cap_max = W.cap_max;
      D.cap0 = W.cap[0];
    } else {
      const size_t ncl = W.scl.size(), nb = W.sbc.size();
      std::vector<char> par(ncl * sizeof(OvlCloud) + 8 * nb);
      std::memcpy(par.data(), W.scl.data(), ncl * sizeof(OvlCloud));
      std::memcpy(par.data() + ncl * sizeof(OvlCloud), W.sbc.data(), nb * 4);
      std::memcpy(par.data() + ncl * sizeof(OvlCloud) + nb * 4, W.sbs.data(), nb * 4);
      HIPC(ensure(d_par, par.size()));
      HIPC(hipMemcpy(d_par.p, par.data(), par.size(), hipMemcpyHostToDevice));
      HIPC(ensure(d_cnt, (nread + n_ref) * 4));
      HIPC(ensure(d_off, (nread + n_ref) * 8));
      HIPC(ensure(d_kr, kr_words * 8));
      HIPC(ensure(d_kg, kg_words * 8));
      HIPC(ensure(d_tr, tmp_rb));
      HIPC(ensure(d_tg, tmp_gb));
      HIPC(ensure(d_pc, (2 * np + 1) * 8));
      HIPC(hipMemsetD32Async((hipDeviceptr_t)d_kr.p, (int)kFill32, kr_words * 2, s));
      HIPC(hipMemsetD32Async((hipDeviceptr_t)d_kg.p, (int)kFill32, kg_words * 2, s));
      HIPC(hipMemsetAsync(d_cnt.p, 0, (nread + n_ref) * 4, s));
      HIPC(hipMemsetAsync(d_off.p, 0, (nread + n_ref) * 8, s));
      char* Dp = d_par.as<char>();
      ovl_window_sides(W, np, nread, n_ref, reinterpret_cast<OvlCloud*>(Dp),
                       reinterpret_cast<const uint32_t*>(Dp + ncl * sizeof(OvlCloud)), d_cnt.as<uint32_t>(),
                       d_off.as<uint64_t>(), d_kr.as<uint64_t>() + kGuard, d_kg.as<uint64_t>() + kGuard, d_tr.p, tmp_rb,
                       d_tg.p, tmp_gb, d_pc.as<unsigned long long>(), kr, kg);
      kr.keys1 = kr.keys0 + cap_r + kGuard;  // (guard words between the emitted and the sorted array too)
      kg.keys1 = kg.keys0 + cap_g + kGuard;
      D.kr = &kr;
      D.kg = &kg;
      D.per_pair = d_pc.as<unsigned long long>() + np + 1;
    }
    int rc = ovl_window_side(ctx->err, s, D, 1, nullptr, d_read.as<float4>());
    if (!rc) rc = ovl_window_side(ctx->err, s, D, 0, nullptr, d_ref.as<float4>());
    if (!rc) rc = ovl_window_counts(ctx->err, s, D);
    if (rc) return rc;
    HIPC(hipGetLastError());
    HIPC(hipStreamSynchronize(s));
    // results
    std::vector<PairState> hs(np + 1);
    HIPC(hipMemcpy(hs.data(), dState, (np + 1) * sizeof(PairState), hipMemcpyDeviceToHost));
    put_cloud(out, g, hs[np], true);
    for (size_t i = 0; i < np; ++i) {
      put_cloud(out, G + idx[i], hs[i], false);
      put_pair(out, idx[i], hs[i]);
    }
    if (!sparse) {
      std::vector<OvlDesc> od(np + 1);
      HIPC(hipMemcpy(od.data(), d_ovl.p, (np + 1) * sizeof(OvlDesc), hipMemcpyDeviceToHost));
      for (size_t i = 0; i <= np; ++i) put_desc(out, i == 0 ? g : G + idx[i - 1], od[i], out->arena_bytes);
      std::vector<uint8_t> back(W.bm + 2 * kGuard * 8);
      HIPC(hipMemcpy(back.data(), d_arena.p, back.size(), hipMemcpyDeviceToHost));
      out->dirty += guard_dirty(back.data(), 8, kFill64) + guard_dirty(back.data() + kGuard * 8 + W.bm, 8, kFill64);
      if (out->arena_bytes < out->arena_cap)
        std::memcpy(out->arena + out->arena_bytes, back.data() + kGuard * 8,
                    std::min<uint64_t>(W.bm, out->arena_cap - out->arena_bytes));
      out->arena_bytes += W.bm;
    } else {
      std::vector<uint32_t> cnt(nread + n_ref);
      std::vector<uint64_t> off(nread + n_ref);
      HIPC(hipMemcpy(cnt.data(), d_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost));
      HIPC(hipMemcpy(off.data(), d_off.p, off.size() * 8, hipMemcpyDeviceToHost));
      std::memcpy(out->key_counts + ref_pts_before, cnt.data() + nread, (size_t)n_ref * 4);
      std::memcpy(out->key_offsets + ref_pts_before, off.data() + nread, (size_t)n_ref * 8);
      for (size_t i = 0; i < np; ++i) {
        const uint64_t dst = total_ref_pts + read_first[idx[i]];
        std::memcpy(out->key_counts + dst, cnt.data() + loff[i], (size_t)reads[i].n * 4);
        std::memcpy(out->key_offsets + dst, off.data() + loff[i], (size_t)reads[i].n * 8);
      }
      for (int side = 0; side < 2; ++side) {  // guards | emitted | guards | sorted | guards
        const uint64_t cap = side ? cap_g : cap_r;
        const size_t words = side ? kg_words : kr_words;
        std::vector<uint64_t> back(words);
        HIPC(hipMemcpy(back.data(), side ? d_kg.p : d_kr.p, words * 8, hipMemcpyDeviceToHost));
        for (size_t at : {size_t(0), kGuard + cap, 2 * kGuard + 2 * cap})
          out->dirty += guard_dirty(back.data() + at, 8, kFill64);
        out->list_off[2 * g + side] = out->n_words;
        out->list_cap[2 * g + side] = cap;
        if (out->n_words < out->words_cap)
          std::memcpy(out->words + out->n_words, back.data() + 2 * kGuard + cap,
                      8 * std::min<uint64_t>(cap, out->words_cap - out->n_words));
        out->n_words += cap;
      }
    }
    ref_pts_before += n_ref;
  }
  return AICP_OK;
}

// The tail of an ICP iteration (launch_active_list, then launch_icp_reduce_f: k_icp_reduce and
// k_icp_update_f) on given matches, set up as batch_run sets the ICP loop up (descriptors with
// red_blk_off / n_red_blk, states, the kReduceBlock-reading block map, zeroed work space,
// IcpIterSync). Every argument is checked before the device is touched. The readings, reference
// points and normals live in buffers of this call (the context's hold the resident reference).
// ref_nrm null: the point-to-point kernels (aicp_hip_test_step_p2p), which read no normals.
int test_step_run(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* n_read, const uint32_t* n_ref,
                  const uint32_t* ref_off, size_t total_ref, const float* read_c, const float* ref_pts,
                  const float* ref_nrm, const float* init_T, const uint8_t* active, int32_t max_iter, int32_t smooth,
                  float min_rot, float min_trans, size_t n_steps, const float* limit, const int32_t* match,
                  const float* d2, const uint32_t* touched, double* out_slab, float* out_T, int32_t* out_state,
                  float* out_inlier, uint64_t* out_touched, double* out_dqdt, uint64_t* out_dirty) {
  if (!ctx || !n_read || !n_ref || !ref_off || !read_c || !ref_pts || !limit || !match || !d2 ||
      !touched || !out_slab || !out_T || !out_state || !out_inlier || !out_touched || !out_dqdt || !out_dirty)
    return AICP_ERR_INVALID;
  if (n_pairs == 0 || n_pairs > (size_t)kMaxPairs || n_steps == 0 || total_ref == 0) return AICP_ERR_INVALID;
  if (smooth < 1 || smooth >= kHistRing) return AICP_ERR_INVALID;
  if (total_ref >= (1ull << 28)) return AICP_ERR_INVALID;
  const size_t P = n_pairs;
  uint64_t total, rows = 0;
  if (!count_check(n_read, P, 1ull << 31, &total)) return AICP_ERR_INVALID;
  for (size_t p = 0; p < P; ++p) {
    if (n_ref[p] == 0 || (uint64_t)ref_off[p] + n_ref[p] > total_ref) return AICP_ERR_INVALID;
    rows += (n_read[p] + (uint32_t)kReduceBlock - 1) / (uint32_t)kReduceBlock;
  }
  if (total * n_steps >= (1ull << 32)) return AICP_ERR_INVALID;
  for (size_t s = 0; s < n_steps; ++s) {
    uint64_t o = s * total;
    for (size_t p = 0; p < P; ++p) {
      const float lim = limit[s * P + p];
      if (!std::isfinite(lim)) return AICP_ERR_INVALID;
      for (uint32_t j = 0; j < n_read[p]; ++j, ++o)  // what the reduce would gather
        if (d2[o] <= lim && (match[o] < 0 || (uint32_t)match[o] >= n_ref[p])) return AICP_ERR_INVALID;
    }
  }
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st_ = ctx->stream;
  std::vector<PairDesc> desc(P, PairDesc{});
  uint32_t off = 0, red = 0;
  for (size_t p = 0; p < P; ++p) {
    PairDesc& d = desc[p];
    d.ref_off = ref_off[p];
    d.n_ref = n_ref[p];
    d.read_off = off;
    d.n_read = n_read[p];
    d.red_blk_off = red;
    d.n_red_blk = (n_read[p] + (uint32_t)kReduceBlock - 1) / (uint32_t)kReduceBlock;
    d.ratio = 1.f;
    ident4(d.Tin);
    ident4(d.Tinit);
    ident4(d.Tmean);
    off += n_read[p];
    red += d.n_red_blk;
  }
  CallBufs loc;
  DevBuf &l_read = loc.get(), &l_bpts = loc.get(), &l_bnrm = loc.get();
  HIPC(ensure(l_read, total * 16));
  HIPC(ensure(l_bpts, total_ref * 16));
  if (ref_nrm) HIPC(ensure(l_bnrm, total_ref * 16));
  HIPC(ensure(ctx->match, total * n_steps * 4));
  HIPC(ensure(ctx->d2, total * n_steps * 4));
  HIPC(ensure(ctx->touch, total * n_steps * 4));
  HIPC(ensure(ctx->slab, rows * kRedCols * 8));
  std::vector<float> pk;
  HIPC(upload_xyz4(pk, read_c, total, l_read.p));
  HIPC(upload_xyz4(pk, ref_pts, total_ref, l_bpts.p));
  if (ref_nrm) HIPC(upload_xyz4(pk, ref_nrm, total_ref, l_bnrm.p));
  HIPC(hipMemcpy(ctx->match.p, match, total * n_steps * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->d2.p, d2, total * n_steps * 4, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(ctx->touch.p, touched, total * n_steps * 4, hipMemcpyHostToDevice));
  BlockMap m;  // (one block per slab row)
  IcpIterSync y;
  const int rc = icp_iter_setup(ctx, desc, kReduceBlock, true, init_T, active, &m, &y);
  if (rc) return rc;
  PairDesc* dDesc = ctx->desc.as<PairDesc>();
  PairState* dState = ctx->state.as<PairState>();
  double* slab = ctx->slab.as<double>();
  aicp_icp_config tc{};  // (nn_epsilon 0: every match is exact)
  tc.knn_normals = ref_nrm ? 20 : 0;  // (which pair of kernels launch_icp_reduce_f launches)
  tc.nn_max_dist = INFINITY;
  tc.max_iter = max_iter;
  tc.smooth_length = smooth;
  tc.min_diff_rot = min_rot;
  tc.min_diff_trans = min_trans;
  const IcpParams prm = icp_params(&tc);
  std::vector<PairState> hs(P);
  constexpr uint32_t kSentinel = 0x7FF8DEADu;  // both halves: a NaN no sum produces
  for (size_t s = 0; s < n_steps; ++s) {
    for (size_t p = 0; p < P; ++p)
      HIPC(hipMemcpyAsync(&dState[p].limit, limit + s * P + p, 4, hipMemcpyHostToDevice, st_));
    HIPC(hipMemsetD32Async((hipDeviceptr_t)slab, (int)kSentinel, rows * kRedCols * 2, st_));
    launch_active_list(st_, (int)P, dDesc, dState, y.al, y.ctr);
    launch_icp_reduce_f(st_, m, dDesc, dState, l_read.as<float4>(), ctx->match.as<int32_t>() + s * total,
                        ctx->d2.as<float>() + s * total, ctx->touch.as<uint32_t>() + s * total, l_bpts.as<float4>(),
                        l_bnrm.as<float4>(), slab, prm, y);
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out_slab + s * rows * kRedCols, slab, rows * kRedCols * 8, hipMemcpyDeviceToHost, st_));
    HIPC(hipMemcpyAsync(hs.data(), dState, P * sizeof(PairState), hipMemcpyDeviceToHost, st_));
    HIPC(hipStreamSynchronize(st_));
    for (size_t p = 0; p < P; ++p) {
      const size_t o = s * P + p;
      const PairState& h = hs[p];
      std::memcpy(out_T + 16 * o, h.T, 64);
      int32_t* w = out_state + 6 * o;
      w[0] = h.kept;
      w[1] = h.iters;
      w[2] = h.status;
      w[3] = h.active;
      w[4] = h.converged;
      w[5] = h.hist_count;
      out_inlier[o] = h.inlier_ratio;
      out_touched[2 * o] = h.touched_pts;
      out_touched[2 * o + 1] = h.touched_nodes;
      const int last = (int)((uint32_t)(h.hist_count - 1) % (uint32_t)kHistRing);  // the entry just pushed
      out_dqdt[2 * o] = h.dq[last];
      out_dqdt[2 * o + 1] = h.dt[last];
    }
  }
  // the arrival counters the iteration tail leaves for the next one: red | pairs, all zero
  std::vector<uint32_t> w(P + 2);
  HIPC(hipMemcpy(w.data(), y.red, (P + 2) * 4, hipMemcpyDeviceToHost));
  uint64_t dirty = 0;
  for (uint32_t v : w) dirty += v != 0;
  *out_dirty = dirty;
  return AICP_OK;
}

}  // namespace

extern "C" {

int aicp_hip_test_force_scan_stall(int on) { return set_lb_force_stall(on) == hipSuccess ? AICP_OK : AICP_ERR_HIP; }

// Any select variant on given distances, set up as batch_run sets the ICP loop up (descriptors,
// states, the 4096-reading block map, zeroed work space, active list, IcpIterSync); between steps
// the update kernel's part of an iteration: the group's pairs counter zeroed, the active list rebuilt.
int aicp_hip_test_select(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* counts, const float* ratios,
                         const uint8_t* active, size_t n_steps, const int32_t* variant, const float* d2,
                         float* out_limit, int32_t* out_status, int32_t* out_n_finite, uint32_t* out_b1,
                         uint32_t* out_miss, uint64_t* out_dirty) {
  if (!ctx || !counts || !ratios || !variant || !d2 || !out_limit || !out_status || !out_n_finite || !out_b1 ||
      !out_miss || !out_dirty)
    return AICP_ERR_INVALID;
  if (n_pairs == 0 || n_pairs > (size_t)kMaxPairs || n_steps == 0) return AICP_ERR_INVALID;
  const size_t P = n_pairs;
  uint64_t total, max_read;
  if (!count_check(counts, P, 1ull << 31, &total, &max_read)) return AICP_ERR_INVALID;
  for (size_t p = 0; p < P; ++p)
    if (!(ratios[p] >= 0.f && ratios[p] <= 1.f)) return AICP_ERR_INVALID;
  if (total * n_steps >= (1ull << 32)) return AICP_ERR_INVALID;
  for (size_t s = 0; s < n_steps; ++s) {
    if (variant[s] < 0 || variant[s] > 5) return AICP_ERR_INVALID;
    if (variant[s] == 5 && !sel_pair_fits(P, max_read, 1)) return AICP_ERR_INVALID;
  }
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st_ = ctx->stream;
  std::vector<PairDesc> desc(P, PairDesc{});
  uint32_t off = 0;
  for (size_t p = 0; p < P; ++p) {
    desc[p].read_off = off;
    desc[p].n_read = counts[p];
    desc[p].ratio = ratios[p];
    off += counts[p];
  }
  HIPC(ensure(ctx->d2, total * n_steps * 4));
  HIPC(ensure(ctx->sel_hist, P * kHistBins * 4));
  HIPC(ensure(ctx->sel_cand, total * 4));
  HIPC(ensure(ctx->sel_cnt, P * 4));
  uint32_t* hist = ctx->sel_hist.as<uint32_t>();
  uint32_t* cand = ctx->sel_cand.as<uint32_t>();
  uint32_t* cnt = ctx->sel_cnt.as<uint32_t>();
  HIPC(hipMemcpy(ctx->d2.p, d2, total * n_steps * 4, hipMemcpyHostToDevice));
  HIPC(hipMemsetAsync(hist, 0, P * kHistBins * 4, st_));
  HIPC(hipMemsetAsync(cnt, 0, P * 4, st_));
  BlockMap m;
  IcpIterSync y;
  const int rc = icp_iter_setup(ctx, desc, kNNBlock * kSelPerThread, false, nullptr, active, &m, &y);
  if (rc) return rc;
  PairDesc* dDesc = ctx->desc.as<PairDesc>();
  PairState* dState = ctx->state.as<PairState>();
  std::vector<PairState> hs(P);
  for (size_t s = 0; s < n_steps; ++s) {
    HIPC(hipMemsetAsync(y.pairs, 0, 4, st_));  // (stopped pairs arrived there; the update kernel's arrivals complete it)
    launch_active_list(st_, (int)P, dDesc, dState, y.al, y.ctr);
    const float* d = ctx->d2.as<float>() + s * total;
    switch (variant[s]) {
      case 0: launch_icp_select(st_, m, (int)P, dDesc, dState, d, hist, cand, cnt); break;
      case 1: launch_icp_select_f(st_, m, dDesc, dState, d, hist, cand, cnt, y); break;
      case 2: launch_icp_select_fused(st_, m, dDesc, dState, d, hist, cand, cnt, y); break;
      case 3: launch_icp_select_fused(st_, m, dDesc, dState, d, hist, cand, cnt, y, (uint32_t)kHistBins); break;
      case 4: launch_icp_select_fused(st_, m, dDesc, dState, d, hist, cand, cnt, y, kFinalLds); break;
      default: launch_icp_select_pair(st_, (int)P, dDesc, dState, d, cand, y); break;
    }
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(hs.data(), dState, P * sizeof(PairState), hipMemcpyDeviceToHost, st_));
    HIPC(hipStreamSynchronize(st_));
    for (size_t p = 0; p < P; ++p) {
      const size_t o = s * P + p;
      out_limit[o] = hs[p].limit;
      out_status[o] = hs[p].status;
      out_n_finite[o] = hs[p].n_finite;
      out_b1[o] = hs[p].sel_b1;
      out_miss[o] = hs[p].sel_miss;
    }
  }
  // what the selects leave for the next iteration: the histograms, the candidate counts and the
  // arrival counters of both select launches, all zero
  std::vector<uint32_t> w(P * kHistBins + 3 * P);
  HIPC(hipMemcpy(w.data(), hist, P * kHistBins * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(w.data() + P * kHistBins, cnt, P * 4, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(w.data() + P * kHistBins + P, y.sel1, 2 * P * 4, hipMemcpyDeviceToHost));  // sel1 | sel2
  uint64_t dirty = 0;
  for (uint32_t v : w) dirty += v != 0;
  *out_dirty = dirty;
  return AICP_OK;
}

int aicp_hip_test_step(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* n_read, const uint32_t* n_ref,
                       const uint32_t* ref_off, size_t total_ref, const float* read_c, const float* ref_pts,
                       const float* ref_nrm, const float* init_T, const uint8_t* active, int32_t max_iter,
                       int32_t smooth, float min_rot, float min_trans, size_t n_steps, const float* limit,
                       const int32_t* match, const float* d2, const uint32_t* touched, double* out_slab,
                       float* out_T, int32_t* out_state, float* out_inlier, uint64_t* out_touched,
                       double* out_dqdt, uint64_t* out_dirty) {
  if (!ref_nrm) return AICP_ERR_INVALID;
  return test_step_run(ctx, n_pairs, n_read, n_ref, ref_off, total_ref, read_c, ref_pts, ref_nrm, init_T, active,
                       max_iter, smooth, min_rot, min_trans, n_steps, limit, match, d2, touched, out_slab, out_T,
                       out_state, out_inlier, out_touched, out_dqdt, out_dirty);
}

int aicp_hip_test_step_p2p(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* n_read, const uint32_t* n_ref,
                           const uint32_t* ref_off, size_t total_ref, const float* read_c, const float* ref_pts,
                           const float* init_T, const uint8_t* active, int32_t max_iter, int32_t smooth,
                           float min_rot, float min_trans, size_t n_steps, const float* limit, const int32_t* match,
                           const float* d2, const uint32_t* touched, double* out_slab, float* out_T,
                           int32_t* out_state, float* out_inlier, uint64_t* out_touched, double* out_dqdt,
                           uint64_t* out_dirty) {
  return test_step_run(ctx, n_pairs, n_read, n_ref, ref_off, total_ref, read_c, ref_pts, nullptr, init_T, active,
                       max_iter, smooth, min_rot, min_trans, n_steps, limit, match, d2, touched, out_slab, out_T,
                       out_state, out_inlier, out_touched, out_dqdt, out_dirty);
}

// The matcher's batched build (matcher_trees: device_trees_begin / device_trees_end on tb[1] with
// run_batch's plan, then device_trees_check) on given clouds, and everything it wrote, verbatim.
// A build that reports through the control block (a depth beyond the device stack, a scan that
// took its slow path) still ran to its end, so the outputs are downloaded whatever it reports.
int aicp_hip_test_tree(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* counts, const float* pts, int32_t center,
                       int32_t bucket, uint32_t* out_node_off, uint32_t* out_n_nodes, int32_t* out_depth,
                       float* out_mean, uint32_t* out_nodes, float* out_bpts, uint32_t* out_ctl) {
  static_assert(sizeof(TreeCtl) == 4 * AICP_TEST_TREE_CTL_WORDS, "aicp_hip.h: the control block's words");
  if (!ctx || !counts || !pts || !out_node_off || !out_n_nodes || !out_depth || !out_mean || !out_nodes ||
      !out_bpts || !out_ctl)
    return AICP_ERR_INVALID;
  if (n_refs == 0 || n_refs > (size_t)kMaxPairs || center < 0 || center > 1 || bucket < 1 || bucket > 4096)
    return AICP_ERR_INVALID;
  const size_t P = n_refs;
  uint64_t total, n_max;
  if (!count_check(counts, P, 1ull << 28, &total, &n_max)) return AICP_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ctx->refc.invalidate();  // (ctx->bpts / nodes are rewritten)
  std::vector<PairDesc> desc = ref_descs(counts, P);
  HIPC(ensure(ctx->ref1, total * 16));
  HIPC(ensure(ctx->desc, P * sizeof(PairDesc)));
  PairDesc* dDesc = ctx->desc.as<PairDesc>();
  std::vector<float> pk;
  HIPC(upload_xyz4(pk, pts, total, ctx->ref1.p));
  HIPC(hipMemcpy(dDesc, desc.data(), P * sizeof(PairDesc), hipMemcpyHostToDevice));
  TreeBufs& T = ctx->tb[1];
  bool begun = false;
  int rc = enqueue_trees(ctx, 1, P, total, n_max, dDesc, center, bucket, &begun);
  if (!begun) return rc;
  HIPC(hipStreamSynchronize(s));
  if (!rc) rc = device_trees_check(T, ctx->err);
  HIPC(hipMemcpy(desc.data(), dDesc, P * sizeof(PairDesc), hipMemcpyDeviceToHost));
  for (size_t p = 0; p < P; ++p) {
    out_node_off[p] = desc[p].node_off;
    out_n_nodes[p] = desc[p].n_nodes;
    out_depth[p] = desc[p].tree_depth;
    for (int k = 0; k < 3; ++k) out_mean[3 * p + k] = desc[p].mean[k];
  }
  HIPC(hipMemcpy(out_nodes, ctx->nodes.p, (2 * (size_t)total + 2) * 16, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(out_bpts, ctx->bpts.p, (size_t)total * 16, hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(out_ctl, T.tw.ctl, sizeof(TreeCtl), hipMemcpyDeviceToHost));
  return rc;
}

// The production NN launch (launch_active_list, then launch_icp_nn with the grid and engine
// run_batch gives it) on given references, readings and per-step transforms. The trees are the
// matcher's batched build as aicp_hip_test_tree runs it (no centring), the treelets
// matcher_treelets' (the function matcher_trees calls) and the engine plan_treelets' choice. The
// three result arrays live in buffers of this call, 64 guard words on both sides, refilled with
// sentinels before every step. Every argument is checked before the device is touched.
// Non-finite query coordinates are out of scope (libnabo gives no order for them).
int aicp_hip_test_nn(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* ref_counts, const float* ref_pts,
                     int32_t bucket, size_t n_pairs, const uint32_t* pair_ref, const uint32_t* n_read,
                     const float* read_c, size_t n_steps, const float* T, const uint8_t* active, float epsilon,
                     float max_dist, int32_t* out_match, float* out_d2, uint32_t* out_touched, int32_t* out_ids,
                     int32_t* out_engine, uint64_t* out_dirty) {
  if (!ctx || !ref_counts || !ref_pts || !pair_ref || !n_read || !read_c || !T || !out_match || !out_d2 ||
      !out_touched || !out_ids || !out_engine || !out_dirty)
    return AICP_ERR_INVALID;
  if (n_refs == 0 || n_refs > (size_t)kMaxPairs || n_pairs == 0 || n_pairs > (size_t)kMaxPairs || n_steps == 0 ||
      bucket < 1 || bucket > 4096)
    return AICP_ERR_INVALID;
  if (!(epsilon >= 0.f) || !(max_dist >= 0.f)) return AICP_ERR_INVALID;  // (negative or NaN)
  const size_t R = n_refs, P = n_pairs;
  uint64_t total_ref, n_max, total;
  if (!count_check(ref_counts, R, 1ull << 28, &total_ref, &n_max) || !count_check(n_read, P, 1ull << 28, &total))
    return AICP_ERR_INVALID;
  for (size_t p = 0; p < P; ++p)
    if (pair_ref[p] >= R) return AICP_ERR_INVALID;
  if (total * n_steps >= (1ull << 32)) return AICP_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ctx->refc.invalidate();  // (ctx->bpts / nodes / tl are rewritten)
  std::vector<PairDesc> rdesc = ref_descs(ref_counts, R), desc(P, PairDesc{});
  for (PairDesc& d : rdesc) ident4(d.Tmean);  // (no centring: the build leaves it as given)
  ctx->tl_total = plan_treelets(rdesc.data(), R, bucket, ctx->opt.nn_engine);
  uint32_t off = 0;
  for (size_t p = 0; p < P; ++p) {
    PairDesc& d = desc[p];
    d.ref_off = rdesc[pair_ref[p]].ref_off;
    d.n_ref = rdesc[pair_ref[p]].n_ref;
    d.read_off = off;
    d.n_read = n_read[p];
    d.ratio = 1.f;
    d.ref_id = (int32_t)pair_ref[p];
    ident4(d.Tin);
    off += n_read[p];
  }
  constexpr uint32_t kSentinel = AICP_TEST_NN_SENTINEL, kTouchSentinel = AICP_TEST_NN_TOUCH_SENTINEL;
  CallBufs loc;
  DevBuf& l_read = loc.get();
  Guarded g_match, g_d2, g_touch;
  HIPC(ensure(l_read, total * 16));
  HIPC(g_match.alloc(loc, total, kSentinel));
  HIPC(g_d2.alloc(loc, total, kSentinel));
  HIPC(g_touch.alloc(loc, total, kTouchSentinel));
  const Guarded* const results[3] = {&g_match, &g_d2, &g_touch};
  HIPC(ensure(ctx->ref1, total_ref * 16));
  HIPC(ensure(ctx->rdesc, R * sizeof(PairDesc)));
  HIPC(ensure(ctx->desc, P * sizeof(PairDesc)));
  HIPC(ensure(ctx->state, P * sizeof(PairState)));
  HIPC(ensure(ctx->active, active_list_bytes(total, P)));
  HIPC(ensure(ctx->ctrs, kCtrWords * 4));
  std::vector<float> pk;
  HIPC(upload_xyz4(pk, ref_pts, total_ref, ctx->ref1.p));
  HIPC(upload_xyz4(pk, read_c, total, l_read.p));
  PairDesc* dRdesc = ctx->rdesc.as<PairDesc>();
  PairDesc* dDesc = ctx->desc.as<PairDesc>();
  PairState* dState = ctx->state.as<PairState>();
  HIPC(hipMemcpy(dRdesc, rdesc.data(), R * sizeof(PairDesc), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dDesc, desc.data(), P * sizeof(PairDesc), hipMemcpyHostToDevice));
  // the trees, then the treelets and the pairs' frames, as matcher_trees enqueues them
  TreeBufs& Tb = ctx->tb[1];
  int rc = enqueue_trees(ctx, 1, R, total_ref, n_max, dRdesc, 0, bucket);
  if (rc) return rc;
  rc = matcher_treelets(ctx, s, R, total_ref, dRdesc, bucket, ctx->err);
  if (rc) return rc;
  launch_pairs_from_refs(s, (int)P, dDesc, dRdesc);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  // a tree deeper than the device stacks, or treelets beyond their allotment: no search is run
  rc = device_trees_check(Tb, ctx->err);
  if (rc) return rc;
  if (ctx->tl_total && (Tb.pin_ctl.as<TreeCtl>()->error & 4))
    FAIL(AICP_ERR_HIP, "matcher treelets exceed their allotment");
  *out_engine = ctx->tl_total ? 0 : 1;
  {
    std::vector<float> b4(4 * (size_t)total_ref);
    HIPC(hipMemcpy(b4.data(), ctx->bpts.p, total_ref * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < total_ref; ++i) std::memcpy(out_ids + i, &b4[4 * i + 3], 4);
  }
  HIPC(hipMemsetAsync(ctx->ctrs.p, 0, kCtrWords * 4, s));
  HIPC(hipMemsetAsync(dState, 0, P * sizeof(PairState), s));
  launch_init_state(s, (int)P, dDesc, dState);
  std::vector<PairState> hs(P);
  HIPC(hipMemcpyAsync(hs.data(), dState, P * sizeof(PairState), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  aicp_icp_config tc{};
  tc.nn_epsilon = epsilon;
  tc.nn_max_dist = max_dist;
  const IcpParams prm = icp_params(&tc);
  ActiveList* al = ctx->active.as<ActiveList>();
  const uint4* tl = ctx->tl_total ? ctx->tl.as<uint4>() : nullptr;
  const uint2* ptl = ctx->tl_total ? ctx->ptl.as<uint2>() : nullptr;
  const size_t words = g_match.words();
  std::vector<uint32_t> back(3 * words);
  uint64_t dirty = 0;
  for (size_t k = 0; k < n_steps; ++k) {
    for (size_t p = 0; p < P; ++p) {
      std::memcpy(hs[p].T, T + 16 * (k * P + p), 64);
      hs[p].active = !active || active[k * P + p] ? 1 : 0;
    }
    HIPC(hipMemcpyAsync(dState, hs.data(), P * sizeof(PairState), hipMemcpyHostToDevice, s));
    for (const Guarded* g : results) HIPC(g->refill(s));
    launch_active_list(s, (int)P, dDesc, dState, al, ctx->ctrs.as<uint32_t>());
    launch_icp_nn(s, (int)total, dDesc, dState, al, l_read.as<float4>(), ctx->nodes.as<uint4>(), tl, nullptr,
                  ctx->bpts.as<float4>(), ptl, static_cast<int32_t*>(g_match.payload()),
                  static_cast<float*>(g_d2.payload()), static_cast<uint32_t*>(g_touch.payload()),
                  ctx->ctrs.as<uint32_t>(), prm);
    HIPC(hipGetLastError());
    for (size_t a = 0; a < 3; ++a)
      HIPC(hipMemcpyAsync(back.data() + a * words, results[a]->b->p, words * 4, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    g_match.take(back.data(), out_match + k * total, dirty);
    g_d2.take(back.data() + words, out_d2 + k * total, dirty);
    g_touch.take(back.data() + 2 * words, out_touched + k * total, dirty);
  }
  *out_dirty = dirty;
  return AICP_OK;
}

// The SurfaceNormal chain of run_batch's references on given clouds: the raw trees on tb[0] with
// the lean plan, launch_init_state, launch_normals with the normals' counters, a second
// launch_knn_ids with the touched counters, the centred matcher trees on tb[1] and
// launch_normals_to_matcher, all on one stream (run_batch launches launch_init_state ahead of the
// raw trees; it reads the descriptors alone, so its place before the normals is all that counts).
// The id buffers and the two normal arrays are this call's, 64 guard words on both sides,
// sentinel-filled before the launches. Every argument is checked before the device is touched,
// each tree before anything searches it.
int aicp_hip_test_normals(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* counts, const float* pts, int32_t knn,
                          int32_t matcher_bucket, int32_t* out_ids, int32_t* out_ids2, int32_t* out_raw_id,
                          float* out_nrm, int32_t* out_degenerate, uint64_t* out_touched, float* out_bnrm,
                          int32_t* out_matcher_id, int32_t* out_engine, uint64_t* out_dirty) {
  if (!ctx || !counts || !pts || !out_ids || !out_ids2 || !out_raw_id || !out_nrm || !out_degenerate ||
      !out_touched || !out_bnrm || !out_matcher_id || !out_engine || !out_dirty)
    return AICP_ERR_INVALID;
  if (n_refs == 0 || n_refs > (size_t)kMaxPairs || matcher_bucket < 1 || matcher_bucket > 4096)
    return AICP_ERR_INVALID;
  const size_t R = n_refs;
  uint64_t total, n_max;
  if (!count_check(counts, R, 1ull << 28, &total, &n_max)) return AICP_ERR_INVALID;
  if (knn != 10 && knn != 20 && knn != 30) FAIL(AICP_ERR_UNSUPPORTED, "knn must be 10, 20 or 30");
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  ctx->refc.invalidate();  // (ctx->rdesc / rstate / bpts / nodes are rewritten)
  const std::vector<PairDesc> rdesc = ref_descs(counts, R);
  constexpr uint32_t kSentinel = AICP_TEST_NN_SENTINEL;
  CallBufs loc;
  Guarded g_ids, g_ids2, g_nrm, g_bnrm;
  HIPC(g_ids.alloc(loc, (size_t)total * (size_t)knn, kSentinel));
  HIPC(g_ids2.alloc(loc, (size_t)total * (size_t)knn, kSentinel));
  HIPC(g_nrm.alloc(loc, (size_t)total * 4, kSentinel));
  HIPC(g_bnrm.alloc(loc, (size_t)total * 4, kSentinel));
  const Guarded* const results[4] = {&g_ids, &g_ids2, &g_nrm, &g_bnrm};
  DevBuf& l_touched = loc.get();
  HIPC(ensure(l_touched, 16));
  HIPC(ensure(ctx->ref1, total * 16));
  HIPC(ensure(ctx->rdesc, R * sizeof(PairDesc)));
  HIPC(ensure(ctx->rdesc_raw, R * sizeof(PairDesc)));
  HIPC(ensure(ctx->rstate, R * sizeof(PairState)));
  HIPC(ensure(ctx->inv, total * 4));
  HIPC(ensure(ctx->ctrs, kCtrWords * 4));
  std::vector<float> pk;
  HIPC(upload_xyz4(pk, pts, total, ctx->ref1.p));
  PairDesc* dRaw = ctx->rdesc_raw.as<PairDesc>();
  PairDesc* dRdesc = ctx->rdesc.as<PairDesc>();
  PairState* dRstate = ctx->rstate.as<PairState>();
  HIPC(hipMemcpy(dRaw, rdesc.data(), R * sizeof(PairDesc), hipMemcpyHostToDevice));
  HIPC(hipMemcpy(dRdesc, rdesc.data(), R * sizeof(PairDesc), hipMemcpyHostToDevice));
  for (const Guarded* g : results) HIPC(g->refill(s));
  HIPC(hipMemsetAsync(l_touched.p, 0, 16, s));
  HIPC(hipMemsetAsync(ctx->ctrs.p, 0, kCtrWords * 4, s));
  HIPC(hipMemsetAsync(dRstate, 0, R * sizeof(PairState), s));
  // 1. the raw-coordinate trees (run_batch's build of them)
  int rc = enqueue_trees(ctx, 0, R, total, n_max, dRaw, 0, kNormalsBucket);
  if (rc) return rc;
  HIPC(hipStreamSynchronize(s));
  rc = device_trees_check(ctx->tb[0], ctx->err);  // (a tree deeper than the device stacks: no search is run)
  if (rc) return rc;
  // 2. - 4. the state, the normals, the kNN again with its counters
  int32_t* ids = static_cast<int32_t*>(g_ids.payload());
  int32_t* ids2 = static_cast<int32_t*>(g_ids2.payload());
  float4* nrm = static_cast<float4*>(g_nrm.payload());
  float4* bnrm = static_cast<float4*>(g_bnrm.payload());
  uint32_t* nCtr = ctx->ctrs.as<uint32_t>() + kKnnCtrOff;
  const int engine = ctx->opt.normals_knn_engine;
  int engine_used = 0;
  launch_init_state(s, (int)R, dRaw, dRstate);
  if (!launch_normals(s, (int)R, (uint32_t)total, dRaw, dRstate, ctx->nodes_raw.as<uint4>(), nullptr,
                      ctx->bpts_raw.as<float4>(), nrm, knn, ids, nCtr, engine))
    FAIL(AICP_ERR_UNSUPPORTED, "normals knn");
  if (!launch_knn_ids(s, (int)R, (uint32_t)total, dRaw, ctx->nodes_raw.as<uint4>(), ctx->bpts_raw.as<float4>(), knn,
                      ids2, nCtr, l_touched.as<unsigned long long>(), engine, &engine_used))
    FAIL(AICP_ERR_UNSUPPORTED, "normals knn");
  *out_engine = engine_used;  // (the kernel that launch launched)
  HIPC(hipGetLastError());
  // 5. the matcher trees (matcher_trees' build: centred)
  rc = enqueue_trees(ctx, 1, R, total, n_max, dRdesc, 1, matcher_bucket);
  if (rc) return rc;
  HIPC(hipStreamSynchronize(s));
  rc = device_trees_check(ctx->tb[1], ctx->err);
  if (rc) return rc;
  // 6. the normals in the matcher trees' order
  launch_normals_to_matcher(s, (int)R, (uint32_t)total, dRdesc, ctx->bpts.as<float4>(), ctx->bpts_raw.as<float4>(),
                            nrm, ctx->inv.as<uint32_t>(), bnrm);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  uint64_t dirty = 0;
  {
    std::vector<uint32_t> back;
    void* const outs[4] = {out_ids, out_ids2, out_nrm, out_bnrm};
    for (size_t a = 0; a < 4; ++a) HIPC(results[a]->fetch(back, outs[a], dirty));
    for (int which = 0; which < 2; ++which) {  // (4 words a point: within what the normals took)
      HIPC(hipMemcpy(back.data(), which ? ctx->bpts.p : ctx->bpts_raw.p, (size_t)total * 16, hipMemcpyDeviceToHost));
      int32_t* out = which ? out_matcher_id : out_raw_id;
      for (size_t i = 0; i < total; ++i) out[i] = (int32_t)back[4 * i + 3];
    }
  }
  std::vector<PairState> hs(R);
  HIPC(hipMemcpy(hs.data(), dRstate, R * sizeof(PairState), hipMemcpyDeviceToHost));
  for (size_t r = 0; r < R; ++r) out_degenerate[r] = hs[r].degenerate;
  HIPC(hipMemcpy(out_touched, l_touched.p, 16, hipMemcpyDeviceToHost));
  *out_dirty = dirty;
  return AICP_OK;
}

// The batch's overlap (upload_pairs, run_batch with AICP_RUN_OVERLAP: grouping, key boxes,
// overlap_maps or overlap_sparse) on given clouds and origins, and everything it wrote: the
// states, the map descriptors and arena, or the key path's counts, offsets and sorted words.
// ctx->ovl_probe carries the overrides of the two launch rules in and what ran out. Every
// argument is checked before the device is touched.
int aicp_hip_test_overlap(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* ref_counts, const float* ref_pts,
                          size_t n_pairs, const uint32_t* pair_ref, const uint32_t* n_read, const float* read_pts,
                          const double* ref_origins, const double* read_origins, double resolution, int32_t path,
                          int32_t filter, int32_t wide, int32_t cap_mode, const uint64_t* caps, int32_t rigid,
                          aicp_test_overlap_out* out) {
  if (!ctx || !ref_counts || !ref_pts || !pair_ref || !n_read || !read_pts || !ref_origins || !read_origins || !out)
    return AICP_ERR_INVALID;
  if (!out->pair_group || !out->cloud_keys || !out->cloud_err || !out->cloud_bbox || !out->pair_counts ||
      !out->pair_percent || !out->pair_ratio || !out->pair_err || !out->desc_min || !out->desc_dim || !out->desc_off ||
      !out->desc_bytes || !out->arena || !out->key_counts || !out->key_offsets || !out->words || !out->cloud_bound ||
      !out->list_off || !out->list_cap)
    return AICP_ERR_INVALID;
  if (n_refs == 0 || n_refs > (size_t)kMaxPairs || n_pairs == 0 || n_pairs > (size_t)kMaxPairs) return AICP_ERR_INVALID;
  if (!(resolution > 0) || path < 0 || path > 4 || filter < -1 || filter > 1 || wide < -1 || wide > 1 || cap_mode < 0 ||
      cap_mode > 1 || rigid < 0 || rigid > 1 || (cap_mode == 1 && (!caps || path < 3)))
    return AICP_ERR_INVALID;
  const size_t R = n_refs, P = n_pairs;
  std::vector<uint64_t> roff(R + 1, 0);
  for (size_t r = 0; r < R; ++r) {
    if (ref_counts[r] == 0) return AICP_ERR_INVALID;
    roff[r + 1] = roff[r] + ref_counts[r];
  }
  std::vector<aicp_pair> pairs(P, aicp_pair{});
  uint64_t wo = 0;
  for (size_t p = 0; p < P; ++p) {
    if (n_read[p] == 0 || pair_ref[p] >= R) return AICP_ERR_INVALID;
    aicp_pair& q = pairs[p];
    q.ref = ref_pts + 3 * roff[pair_ref[p]];
    q.n_ref = ref_counts[pair_ref[p]];
    q.ref_stride = 12;
    q.read = read_pts + 3 * wo;
    q.n_read = n_read[p];
    q.read_stride = 12;
    for (int k = 0; k < 3; ++k) {
      q.ref_origin[k] = ref_origins[3 * p + k];
      q.read_origin[k] = read_origins[3 * p + k];
    }
    wo += n_read[p];
  }
  {  // the per-point slots of the key path: one per point of every group's reference and reading
    std::vector<std::pair<uint32_t, std::array<double, 3>>> groups;
    uint64_t slots = wo;
    for (size_t p = 0; p < P; ++p) {
      const std::pair<uint32_t, std::array<double, 3>> g{
          pair_ref[p], {ref_origins[3 * p], ref_origins[3 * p + 1], ref_origins[3 * p + 2]}};
      if (std::find(groups.begin(), groups.end(), g) == groups.end()) {
        groups.push_back(g);
        slots += ref_counts[pair_ref[p]];
      }
    }
    if (slots > out->points_cap) return AICP_ERR_INVALID;
  }
  HIPC(hipSetDevice(ctx->device));
  ctx->refc.invalidate();  // (ctx->bitmap and the group states are rewritten)
  ctx->rdc.valid = ctx->rdc.hit = false;
  struct Local {  // freed, and the probe switched off, on every return
    aicp_hip_ctx* ctx;
    aicp_hip_batch* B = new aicp_hip_batch();
    ~Local() {
      ctx->ovl_probe = OvlProbe{};
      (void)hipStreamSynchronize(ctx->stream);
      free_batch(B);
    }
  } loc{ctx};
  OvlProbe& probe = ctx->ovl_probe;
  probe = OvlProbe{};
  probe.on = true;
  probe.filter = filter;
  probe.wide = wide;
  probe.keys = path == 2;
  aicp_icp_config cfg;
  aicp_hip_default_config(&cfg);
  const int saved_path = ctx->opt.overlap_path;
  if (path == 1) ctx->opt.overlap_path = 0;  // (dense wherever the maps fit)
  int rc = upload_pairs(ctx, pairs.data(), P, loc.B, false);
  out->dirty = 0;
  if (!rc && path >= 3) {  // the stream's windows, one per overlap group
    ctx->opt.overlap_path = saved_path;
    return ovl_window_test(ctx, loc.B, pairs.data(), resolution, path, filter, wide, cap_mode ? caps : nullptr, rigid,
                           out);
  }
  if (!rc) rc = run_batch(ctx, loc.B, &cfg, resolution, AICP_RUN_OVERLAP, nullptr, nullptr, nullptr);
  ctx->opt.overlap_path = saved_path;
  // a cloud's ovl_err comes back as the batch's "pair status": reported in the outputs instead
  if (rc && !(rc == AICP_ERR_HIP && ctx->err.rfind("pair status", 0) == 0)) return rc;
  const size_t G = loc.B->gdesc.size();
  out->path = probe.ran_path;
  out->filter = probe.ran_filter;
  out->wide = probe.ran_wide;
  out->n_groups = (int32_t)G;
  std::vector<PairState> hs(P), hg(G);
  HIPC(hipMemcpy(hs.data(), ctx->state.p, P * sizeof(PairState), hipMemcpyDeviceToHost));
  HIPC(hipMemcpy(hg.data(), ctx->gstate.p, G * sizeof(PairState), hipMemcpyDeviceToHost));
  for (size_t c = 0; c < G + P; ++c) put_cloud(out, c, c < G ? hg[c] : hs[c - G], c < G);
  for (size_t p = 0; p < P; ++p) {
    out->pair_group[p] = loc.B->desc[p].ogroup;
    put_pair(out, p, hs[p]);
  }
  out->arena_bytes = out->n_points = out->n_words = 0;
  if (probe.ran_path == 1) {  // the descriptors lie readings first; the outputs groups first
    std::vector<OvlDesc> od(P + G);
    HIPC(hipMemcpy(od.data(), ctx->ovl.p, (P + G) * sizeof(OvlDesc), hipMemcpyDeviceToHost));
    for (size_t c = 0; c < G + P; ++c) put_desc(out, c, od[c < G ? P + c : c - G], 0);
    out->arena_bytes = probe.arena_bytes;
    const uint64_t nb = std::min(out->arena_cap, out->arena_bytes);
    if (nb) HIPC(hipMemcpy(out->arena, ctx->bitmap.p, nb, hipMemcpyDeviceToHost));
  } else if (probe.ran_path == 2) {
    out->n_points = probe.n_points;
    out->n_words = probe.n_keys;
    if (probe.n_points > out->points_cap) FAIL(AICP_ERR_INVALID, "points_cap");
    if (probe.n_points) {
      HIPC(hipMemcpy(out->key_counts, probe.cnt, probe.n_points * 4, hipMemcpyDeviceToHost));
      HIPC(hipMemcpy(out->key_offsets, probe.off, probe.n_points * 8, hipMemcpyDeviceToHost));
    }
    const uint64_t nw = std::min(out->words_cap, out->n_words);
    if (nw) HIPC(hipMemcpy(out->words, probe.keys1, nw * 8, hipMemcpyDeviceToHost));
  } else {
    FAIL(AICP_ERR_HIP, "the batch ran no overlap");
  }
  return AICP_OK;
}

int aicp_hip_test_key_bound(const float* pts, size_t n, const double origin[3], double resolution, int32_t rigid,
                            uint64_t* out_bound, uint64_t* out_point_cap) {
  if (!pts || !origin || !out_bound || !out_point_cap || n == 0 || !(resolution > 0) || rigid < 0 || rigid > 1)
    return AICP_ERR_INVALID;
  WorkerPool pool{0};
  aicp_cloud c{};
  c.pts = pts;
  c.n = n;
  c.stride = 12;
  *out_bound = key_bound(pool, c, origin, resolution, rigid != 0);
  *out_point_cap = kMaxRayKeys;
  return AICP_OK;
}

// The raw streams' ingest alone (the upload policy of ingest_upload, k_stream_ingest)
int aicp_hip_test_ingest(aicp_hip_ctx* ctx, const float* rows, size_t n, size_t stride, const float* T, float* out4) {
  if (!ctx || (n && !rows) || stride < 12 || (stride % 4) || n > (size_t)INT32_MAX) return AICP_ERR_INVALID;
  if (n == 0) return AICP_OK;
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  // scratch: T | the rows (ingest_upload) | the output
  const size_t o_rows = 256, o_out = (o_rows + n * std::min<size_t>(stride, 16) + 255) & ~size_t(255);
  HIPC(ensure(ctx->scratch, o_out + n * 16));
  const void* drows = nullptr;
  size_t dstride = 0;
  const int rc = ingest_upload(ctx, rows, n, stride, o_rows, &drows, &dstride);
  if (rc) return rc;
  char* d = ctx->scratch.as<char>();
  if (T) HIPC(hipMemcpyAsync(d, T, 64, hipMemcpyHostToDevice, s));
  launch_stream_ingest(s, (int)n, drows, dstride, T ? (const float*)d : nullptr, nullptr, (float4*)(d + o_out));
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  if (out4) HIPC(hipMemcpy(out4, d + o_out, n * 16, hipMemcpyDeviceToHost));
  return AICP_OK;
}

// The monitor's resident core (monitor_resident: k_mon_stage, the trees, k_mon_nn, the selects,
// k_mon_reduce, k_mon_finish) as a live session runs it: the reference, the reading, T and the
// result's 56 bytes in guarded device buffers of their own, a reference tree that `runs` calls in a
// row share (the first builds it, the others reuse it, as a session's readings against one
// reference), the wait and monitor_resident_check after each. result: the last run's; *dirty: guard
// words that changed plus input words that no longer hold what was uploaded; counters:
// aicp_hip_session_monitor_counters' four.
int aicp_hip_test_monitor_resident(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg,
                                   const float* ref_xyz, size_t n_ref, const float* read_xyz, size_t n_read,
                                   const float T[16], int32_t runs, aicp_monitor_result* result, uint64_t* dirty,
                                   uint64_t counters[4]) {
  if (!ctx || !prm || !ref_xyz || !read_xyz || !T || !result || !dirty || !counters || n_ref == 0 || n_read == 0 ||
      n_ref + n_read >= (1ull << 28) || runs < 1 || runs > 8)
    return AICP_ERR_INVALID;
  if ((prm->flags & AICP_MON_PAIRED) && !cfg) return AICP_ERR_INVALID;
  int rc = monitor_params_check(ctx, prm);
  if (rc) return rc;
  *dirty = 0;
  std::memset(result, 0, sizeof(*result));
  std::memset(counters, 0, 4 * sizeof(uint64_t));
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  HIPC(hipStreamSynchronize(s));
  CallBufs loc;
  loc.sync = s;
  constexpr size_t kResWords = sizeof(aicp_monitor_result) / 4;
  Guarded gref, gread, gT, gres;
  HIPC(gref.alloc(loc, 4 * n_ref, 0x7fc0aaaau));
  HIPC(gread.alloc(loc, 4 * n_read, 0x7fc0bbbbu));
  HIPC(gT.alloc(loc, 16, 0x7fc0ccccu));
  HIPC(gres.alloc(loc, kResWords, 0xddddddddu));
  for (const Guarded* g : {&gref, &gread, &gT, &gres}) HIPC(g->refill(s));
  HIPC(hipStreamSynchronize(s));
  std::vector<float> pk, href(4 * n_ref), hread(4 * n_read);
  HIPC(upload_xyz4(pk, ref_xyz, n_ref, gref.payload()));
  std::memcpy(href.data(), pk.data(), href.size() * 4);
  HIPC(upload_xyz4(pk, read_xyz, n_read, gread.payload()));
  std::memcpy(hread.data(), pk.data(), hread.size() * 4);
  HIPC(hipMemcpy(gT.payload(), T, 64, hipMemcpyHostToDevice));
  MonRefTree tree;
  MonCounters cnt;
  std::vector<uint32_t> back;
  aicp_monitor_result last{};
  for (int r = 0; r < runs && !rc; ++r) {
    rc = monitor_resident(ctx, prm, cfg, static_cast<const float4*>(gref.payload()), n_ref,
                          static_cast<const float4*>(gread.payload()), n_read, static_cast<const float*>(gT.payload()),
                          &tree, &cnt, gres.payload());
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) {
      ctx->err = std::string("hipStreamSynchronize: ") + hipGetErrorString(e);
      rc = AICP_ERR_HIP;
    }
    if (!rc && gres.fetch(back, &last, *dirty) != hipSuccess) rc = AICP_ERR_HIP;
    if (!rc) rc = monitor_resident_check(ctx, &tree, &last);
    if (!rc) ++cnt.readings;
  }
  tree.release_all();  // (the stream is idle: every run was waited for)
  if (rc) return rc;
  // the inputs: guards untouched, payloads as uploaded
  std::vector<float> in(std::max({href.size(), hread.size(), (size_t)16}));
  if (gref.fetch(back, in.data(), *dirty) != hipSuccess) return AICP_ERR_HIP;
  *dirty += std::memcmp(in.data(), href.data(), href.size() * 4) != 0;
  if (gread.fetch(back, in.data(), *dirty) != hipSuccess) return AICP_ERR_HIP;
  *dirty += std::memcmp(in.data(), hread.data(), hread.size() * 4) != 0;
  if (gT.fetch(back, in.data(), *dirty) != hipSuccess) return AICP_ERR_HIP;
  *dirty += std::memcmp(in.data(), T, 64) != 0;
  *result = last;
  counters[0] = cnt.readings;
  counters[1] = cnt.trees;
  counters[2] = cnt.reuses;
  counters[3] = cnt.trees2;
  return AICP_OK;
}

// The live session's promotion kernels (session.cpp's four launches) on a made-up block: the
// reading, the reference buffer and the map in guarded device buffers of their own, the block in a
// call-local copy of the session's layout.
int aicp_hip_test_promote_map(aicp_hip_ctx* ctx, int32_t kernel, const float* read4, size_t n, size_t tail,
                              int32_t id, void* block, float* ref4, float* map4, uint64_t* dirty) {
  constexpr size_t kBlock = 448, kRec = 128, kHdr = 192, kGate = 256, kT = 320, kOrg = 384;
  if (!ctx || !read4 || !block || !ref4 || !map4 || !dirty || kernel < 0 || kernel > 3 || n == 0 ||
      n + tail >= (1ull << 24))
    return AICP_ERR_INVALID;
  *dirty = 0;
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  HIPC(hipStreamSynchronize(s));
  CallBufs loc;
  loc.sync = s;
  Guarded gread, gref, gmap;
  HIPC(gread.alloc(loc, 4 * n, 0xA5A5A5A5u));
  HIPC(gref.alloc(loc, 4 * n, 0xA5A5A5A5u));
  HIPC(gmap.alloc(loc, 4 * (tail + n), 0xA5A5A5A5u));
  DevBuf& blk = loc.get();
  HIPC(ensure(blk, kBlock));
  for (const Guarded* g : {&gread, &gref, &gmap}) HIPC(g->refill(s));
  HIPC(hipStreamSynchronize(s));
  HIPC(hipMemcpy(gread.payload(), read4, n * 16, hipMemcpyHostToDevice));
  HIPC(hipMemcpy(blk.p, block, kBlock, hipMemcpyHostToDevice));
  char* d = blk.as<char>();
  StreamState* dS = reinterpret_cast<StreamState*>(d);
  StreamRec* dRec = reinterpret_cast<StreamRec*>(d + kRec);
  SessionHeader* dHdr = reinterpret_cast<SessionHeader*>(d + kHdr);
  const GateRec* dGate = reinterpret_cast<const GateRec*>(d + kGate);
  float* dT = reinterpret_cast<float*>(d + kT);
  const double* dOrg = reinterpret_cast<const double*>(d + kOrg);
  const float4* dread = static_cast<const float4*>(gread.payload());
  float4* dref = static_cast<float4*>(gref.payload());
  float4* dtail = static_cast<float4*>(gmap.payload()) + tail;
  switch (kernel) {
    case 0: launch_session_promote(s, (int)n, dRec, dT, dread, id, dref, dHdr); break;
    case 1: launch_session_gate_promote(s, (int)n, dGate, dOrg, dread, id, dref, dT, dS, dRec, dHdr); break;
    case 2: launch_session_promote_map(s, (int)n, dRec, dT, dread, id, dref, dtail, dHdr); break;
    default: launch_session_gate_promote_map(s, (int)n, dGate, dOrg, dread, id, dref, dtail, dT, dS, dRec, dHdr);
  }
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  HIPC(hipMemcpy(block, blk.p, kBlock, hipMemcpyDeviceToHost));
  std::vector<uint32_t> back;
  std::vector<float> in(4 * n);
  if (gref.fetch(back, ref4, *dirty) != hipSuccess) return AICP_ERR_HIP;
  if (gmap.fetch(back, map4, *dirty) != hipSuccess) return AICP_ERR_HIP;
  if (gread.fetch(back, in.data(), *dirty) != hipSuccess) return AICP_ERR_HIP;
  *dirty += std::memcmp(in.data(), read4, n * 16) != 0;
  return AICP_OK;
}

int aicp_hip_test_chain_batch(aicp_hip_ctx* ctx, const aicp_chain* chain, int32_t side, size_t n_clouds,
                              const uint32_t* counts, const float* pts, uint64_t* out_counts, uint64_t* out_n,
                              int32_t* out_index, float* out_normals, float* out_densities) {
  if (!ctx) return AICP_ERR_INVALID;
  uint64_t total = 0;
  if (!chain || !counts || !pts || !out_counts || !out_n || !out_index || n_clouds == 0 ||
      n_clouds > (size_t)kMaxPairs || (side != AICP_CHAIN_REFERENCE && side != AICP_CHAIN_READING) ||
      !count_check(counts, n_clouds, 1ull << 28, &total))
    FAIL(AICP_ERR_INVALID, "test_chain_batch arguments");
  int rc = chain_check(ctx, chain);
  if (rc) return rc;
  bool sn = false, sn_dens = false;
  for (int q = 0; q < chain->n_filters[side]; ++q)
    if (chain->filters[side][q].kind == AICP_FILTER_SURFACE_NORMAL) {
      sn = true;
      sn_dens = chain->filters[side][q].keep_densities != 0;
    }
  if (out_normals && !sn) FAIL(AICP_ERR_INVALID, "normals asked of a side without SurfaceNormal");
  if (out_densities && !sn_dens) FAIL(AICP_ERR_INVALID, "densities asked of a side without keepDensities");
  HIPC(hipSetDevice(ctx->device));
  CallBufs loc;
  loc.sync = ctx->stream;
  DevBuf& src = loc.get();
  HIPC(ensure(src, total * 16));
  std::vector<float> pk;
  HIPC(upload_xyz4(pk, pts, total, src.p));
  std::vector<uint32_t> off(n_clouds);
  uint32_t run = 0;
  for (size_t c = 0; c < n_clouds; ++c) {
    off[c] = run;
    run += counts[c];
  }
  ChainBatchSide sb;
  rc = chain_batch_side(ctx, chain, side, n_clouds, counts, src.as<float4>(), off.data(), out_normals != nullptr,
                        out_densities != nullptr, &sb);
  if (rc) return rc;
  HIPC(hipStreamSynchronize(ctx->stream));
  const int nf = chain->n_filters[side];
  const ChainBufs& cb = ctx->chain[side];
  std::vector<float> rows(4 * (size_t)total), nrm, dens;
  HIPC(hipMemcpy(rows.data(), cb.pts[sb.cur].p, (size_t)total * 16, hipMemcpyDeviceToHost));
  if (out_normals) {
    if (!sb.nrm) FAIL(AICP_ERR_HIP, "chain normals missing");
    nrm.resize(4 * (size_t)total);
    HIPC(hipMemcpy(nrm.data(), cb.nrm[sb.cur].p, (size_t)total * 16, hipMemcpyDeviceToHost));
  }
  if (out_densities && sb.dens_sn) {
    dens.resize((size_t)total);
    HIPC(hipMemcpy(dens.data(), cb.dens_sn.p, (size_t)total * 4, hipMemcpyDeviceToHost));
  }
  uint64_t k = 0, kd = 0;
  for (size_t c = 0; c < n_clouds; ++c) {
    const ChainCloud& cl = sb.cl[c];
    for (int q = 0; q < AICP_CHAIN_MAX_FILTERS; ++q) out_counts[4 * c + q] = q < nf ? cl.n[q + 1] : 0;
    out_n[c] = cl.n[nf];
    if (cl.n[nf] > counts[c] || cl.off[nf] + (uint64_t)cl.n[nf] > total) FAIL(AICP_ERR_HIP, "chain filter count");
    for (uint32_t i = 0; i < cl.n[nf]; ++i, ++k) {
      const size_t row = (size_t)cl.off[nf] + i;
      std::memcpy(&out_index[k], &rows[4 * row + 3], 4);
      if (out_normals)
        for (int d = 0; d < 3; ++d) out_normals[3 * k + d] = nrm[4 * row + d];
    }
    if (out_densities && sb.dens_sn && sb.sn_pos >= 0) {
      if (cl.off[sb.sn_pos] + (uint64_t)cl.n[sb.sn_pos] > total) FAIL(AICP_ERR_HIP, "chain filter count");
      for (uint32_t i = 0; i < cl.n[sb.sn_pos]; ++i) out_densities[kd++] = dens[(size_t)cl.off[sb.sn_pos] + i];
    }
  }
  return AICP_OK;
}

}  // extern "C"
