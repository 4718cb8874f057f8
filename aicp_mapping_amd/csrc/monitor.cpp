// monitor.cpp — aicp_hip_monitor / aicp_hip_monitor_batch: icpMonitor.cpp's metrics chained on the
// device (include/aicp_hip.h).
//
// One call for P pairs, one stream:
//   1. H2D: every cloud once (references, then the clouds to move / the moved clouds) and one block
//      of tables (tree descriptors, NN segments, select descriptors, reduction segments)
//   2. [device] out = T * cloud (k_mon_transform), when T is given
//   3. [device] the 2P kd-trees (tree on ref, tree on out) in one build over the coordinates as
//      given, bucket 8 (KDTreeMatcher's default); the chain matcher's P trees again when its
//      bucket size differs
//   4. [device] 1-NN, d2 only: one launch for the 2P exact searches, one for the P chain-matcher
//      searches (epsilon > 0, a finite maxDist or another bucket size; else direction 0 serves)
//   5. [device] the exact select: the quantile of both directions, then the trimmed limit
//   6. [device] k_mon_reduce, k_mon_finish; D2H of the P results (and the per-point distances)
//
// The resident form (monitor_resident: the live sessions' monitor per reading) is
// the same core behind another front end, for one pair whose clouds lie on the device: the tables
// up, k_mon_stage instead of steps 1 and 2, every tree built alone with planned levels (the
// reference's in the caller's buffers, reused while they are valid; k_mon_guard behind each build),
// one 1-NN launch per direction, steps 5 and 6 with the result written where the caller says. It
// reads nothing back and waits for nothing; monitor_resident_check follows the caller's own wait.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

static_assert(sizeof(MonOut) == sizeof(aicp_monitor_result) && sizeof(MonOut) == 56, "aicp_monitor_result layout");
static_assert(offsetof(MonOut, knn_valid) == offsetof(aicp_monitor_result, knn_valid) &&
                  offsetof(MonOut, paired_mean_dist) == offsetof(aicp_monitor_result, paired_mean_dist) &&
                  offsetof(MonOut, paired_kept) == offsetof(aicp_monitor_result, paired_kept),
              "aicp_monitor_result layout");

namespace {

constexpr int kMonBucket = 8;  // KDTreeMatcher's default bucket size (hausdorffDistance, distancesKNN)

struct MonCloud {
  const float* p;
  uint64_t n, stride;
};

bool mon_valid(const MonCloud& c) { return c.p && c.n >= 1 && c.stride >= 12 && c.stride % 4 == 0; }

// consecutive 256-byte aligned regions of one allocation
struct Arena {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off = (off + bytes + 255) & ~size_t(255);
    return o;
  }
};

// segments of an NN launch -> slot offsets (whole 64-slot chunks each) and the chunk table
uint32_t mon_slots(std::vector<MonSeg>& segs, std::vector<uint32_t>& chunk_seg) {
  uint64_t slot = 0;
  chunk_seg.clear();
  for (size_t e = 0; e < segs.size(); ++e) {
    segs[e].slot_off = (uint32_t)slot;
    const uint64_t chunks = (segs[e].nq + 63) / 64;
    chunk_seg.insert(chunk_seg.end(), chunks, (uint32_t)e);
    slot += chunks * 64;
  }
  return (uint32_t)slot;
}

// The resident form's pair (P = 1): both clouds and the correction where they lie on the device,
// the reference's trees, and where k_mon_finish writes the result (device memory)
struct MonResident {
  const float4 *ref, *read;
  const float* T;
  MonRefTree* tree;
  MonCounters* cnt;
  MonOut* result;
};

// The front end gets the points into the arena: host packing, upload and k_mon_transform (R null:
// aicp_hip_monitor, _batch), or k_mon_stage from resident clouds (R: monitor_resident, whose clouds
// refs[0] / outs[0] only size). The core behind it starts from the arena: trees, k_mon_nn, the
// selects, k_mon_reduce, k_mon_finish. The resident form reads nothing back and waits for nothing
// when its tree levels are planned.
int monitor_core(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg, size_t P,
                 const MonCloud* refs, const MonCloud* outs, const float* T, aicp_monitor_result* res, float* dist_out,
                 float* dist_ref, const MonResident* R = nullptr) {
  const auto w0 = std::chrono::steady_clock::now();
  if (!(prm->quantile >= 0.f && prm->quantile <= 1.f)) FAIL(AICP_ERR_INVALID, "monitor: quantile outside [0, 1]");
  const bool paired = (prm->flags & AICP_MON_PAIRED) != 0;
  if (paired) {
    if (!cfg) FAIL(AICP_ERR_INVALID, "monitor: AICP_MON_PAIRED needs the chain configuration");
    if (cfg->knn_match != 1) FAIL(AICP_ERR_UNSUPPORTED, "KDTreeMatcher.knn != 1");
    if (!(cfg->trimmed_ratio >= 0.f && cfg->trimmed_ratio <= 1.f)) FAIL(AICP_ERR_INVALID, "TrimmedDistOutlierFilter.ratio");
    if (!(cfg->nn_epsilon >= 0.f) || !(cfg->nn_max_dist > 0.f) || cfg->bucket_size < 1)
      FAIL(AICP_ERR_INVALID, "monitor: epsilon, maxDist or bucketSize");
  }
  // the chain matcher's search is direction 0's when it is the same search in the same tree
  const bool reuse = paired && cfg->nn_epsilon == 0.f && std::isinf(cfg->nn_max_dist) && cfg->bucket_size == kMonBucket;
  const bool eps_search = paired && !reuse;
  const bool trees2 = eps_search && cfg->bucket_size != kMonBucket;

  // points: the references, then the out clouds; d2: direction 0 (per out point), direction 1 (per
  // ref point), then the chain matcher's (per out point)
  std::vector<uint32_t> ref_off(P), out_loc(P);
  uint64_t total_ref = 0, total_out = 0;
  for (size_t i = 0; i < P; ++i) {
    if (!mon_valid(refs[i]) || !mon_valid(outs[i])) FAIL(AICP_ERR_INVALID, "monitor: invalid cloud in pair " + std::to_string(i));
    ref_off[i] = (uint32_t)total_ref;
    out_loc[i] = (uint32_t)total_out;
    total_ref += refs[i].n;
    total_out += outs[i].n;
    if (total_ref + total_out >= (1ull << 28)) FAIL(AICP_ERR_UNSUPPORTED, "monitor: more than 2^28 points");
  }
  const uint64_t total = total_ref + total_out;
  const uint64_t total_d2 = total + (eps_search ? total_out : 0);
  auto dA = [&](size_t i) { return out_loc[i]; };
  auto dB = [&](size_t i) { return (uint32_t)(total_out + ref_off[i]); };
  auto dC = [&](size_t i) { return (uint32_t)(total + out_loc[i]); };

  // ---- tables ---------------------------------------------------------------------------------
  const size_t nT = 2 * P;
  std::vector<PairDesc> tdesc(nT, PairDesc{});
  for (size_t t = 0; t < nT; ++t) {
    const size_t i = t % P;
    PairDesc& d = tdesc[t];
    // (resident: every tree is built alone, from a pointer to its cloud's first point)
    d.ref_off = R ? 0u : t < P ? ref_off[i] : (uint32_t)(total_ref + out_loc[i]);
    d.n_ref = (uint32_t)(t < P ? refs[i].n : outs[i].n);
    d.ratio = 0.5f;
    ident4(d.Tin);
  }
  std::vector<MonSeg> segA(2 * P, MonSeg{}), segB(eps_search ? P : 0, MonSeg{});
  std::vector<PairDesc> selq(2 * P, PairDesc{}), selp(paired ? P : 0, PairDesc{});
  std::vector<MonRed> red((eps_search ? 3 : 2) * P, MonRed{});
  std::vector<MonPair> mp(P, MonPair{});
  std::vector<uint2> xf(P);
  Maps mq, mpm, mr, mx;
  for (size_t i = 0; i < P; ++i) {
    const uint32_t n_ref = (uint32_t)refs[i].n, n_out = (uint32_t)outs[i].n;
    const uint32_t q_out = (uint32_t)(total_ref + out_loc[i]);
    segA[2 * i].nq = n_out, segA[2 * i].q_off = q_out, segA[2 * i].tree = (uint32_t)i, segA[2 * i].d2_off = dA(i);
    segA[2 * i + 1].nq = n_ref, segA[2 * i + 1].q_off = ref_off[i], segA[2 * i + 1].tree = (uint32_t)(P + i),
                 segA[2 * i + 1].d2_off = dB(i);
    if (eps_search) segB[i].nq = n_out, segB[i].q_off = q_out, segB[i].tree = (uint32_t)i, segB[i].d2_off = dC(i);
    selq[2 * i].read_off = dA(i), selq[2 * i].n_read = n_out, selq[2 * i].ratio = prm->quantile;
    selq[2 * i + 1].read_off = dB(i), selq[2 * i + 1].n_read = n_ref, selq[2 * i + 1].ratio = prm->quantile;
    mq.add((int)(2 * i), n_out, kNNBlock * kSelPerThread);
    mq.add((int)(2 * i + 1), n_ref, kNNBlock * kSelPerThread);
    if (paired) {
      selp[i].read_off = reuse ? dA(i) : dC(i), selp[i].n_read = n_out, selp[i].ratio = cfg->trimmed_ratio;
      mpm.add((int)i, n_out, kNNBlock * kSelPerThread);
    }
    xf[i] = make_uint2(q_out, n_out);
    mx.add((int)i, n_out, 256);
    mp[i].red[0] = (int32_t)(2 * i), mp[i].red[1] = (int32_t)(2 * i + 1);
    mp[i].red[2] = !paired ? -1 : reuse ? (int32_t)(2 * i) : (int32_t)(2 * P + i);
    mp[i].sel_q[0] = (int32_t)(2 * i), mp[i].sel_q[1] = (int32_t)(2 * i + 1);
    mp[i].sel_p = paired ? (int32_t)i : -1;
  }
  for (size_t r = 0; r < red.size(); ++r) {  // (the chunk slots of a segment are consecutive)
    const size_t i = r < 2 * P ? r / 2 : r - 2 * P;
    MonRed& x = red[r];
    const bool dir0 = r < 2 * P && r % 2 == 0;
    x.d2_off = r >= 2 * P ? dC(i) : dir0 ? dA(i) : dB(i);
    x.n = (uint32_t)(r < 2 * P && !dir0 ? refs[i].n : outs[i].n);
    x.slot0 = (uint32_t)mr.pair.size();
    x.lim = (r >= 2 * P || (dir0 && reuse)) ? (int32_t)i : -1;
    x.knn = dir0 ? 1 : 0;
    x.acc = (uint32_t)r;
    mr.add((int)r, x.n, kMonChunk);
  }
  std::vector<uint32_t> chunkA, chunkB;
  uint32_t slotsA = 0, slotsA1 = 0;
  if (R) {
    // one launch per direction (the two trees lie in different buffers): each segment is its
    // launch's segment 0 and its tree its array's tree 0; one table of zeros names both
    std::vector<MonSeg> one(1);
    std::vector<uint32_t> c0, c1;
    segA[1].tree = 0;
    one[0] = segA[0], slotsA = mon_slots(one, c0), segA[0] = one[0];
    one[0] = segA[1], slotsA1 = mon_slots(one, c1), segA[1] = one[0];
    chunkA = c0.size() >= c1.size() ? c0 : c1;
  } else {
    slotsA = mon_slots(segA, chunkA);
  }
  const uint32_t slotsB = mon_slots(segB, chunkB);

  // one block of tables, at the same offsets on both sides
  Arena a;
  const size_t o_td = a.take(nT * sizeof(PairDesc)), o_td2 = a.take((trees2 ? P : 0) * sizeof(PairDesc)),
               o_sa = a.take(segA.size() * sizeof(MonSeg)), o_ca = a.take(chunkA.size() * 4),
               o_sb = a.take(segB.size() * sizeof(MonSeg)), o_cb = a.take(chunkB.size() * 4),
               o_sq = a.take(selq.size() * sizeof(PairDesc)), o_mq = a.take(mq.pair.size() * 8),
               o_sp = a.take(selp.size() * sizeof(PairDesc)), o_mp = a.take(mpm.pair.size() * 8),
               o_rd = a.take(red.size() * sizeof(MonRed)), o_mr = a.take(mr.pair.size() * 8),
               o_pr = a.take(P * sizeof(MonPair)), o_xf = a.take(P * sizeof(uint2)), o_mx = a.take(mx.pair.size() * 8),
               o_T = a.take(T ? P * 64 : 0);
  const size_t meta_bytes = a.off;
  // device only: states, the zeroed words (counters, histograms, candidate counts, tallies), the
  // points and everything computed from them
  const size_t n_hist = std::max(selq.size(), selp.size());
  const size_t o_stq = a.take(selq.size() * sizeof(PairState)), o_stp = a.take(selp.size() * sizeof(PairState));
  const size_t o_zero = a.off;
  const size_t o_ctr = a.take((R ? 3 : 2) * kPersistCtrWords * 4), o_hist = a.take(n_hist * kHistBins * 4),
               o_cnt = a.take(n_hist * 4), o_acc = a.take(red.size() * sizeof(MonAcc));
  const size_t zero_bytes = a.off - o_zero;
  const bool want_dist = dist_out || dist_ref;
  const size_t o_raw = a.take(total * 16), o_d2 = a.take(total_d2 * 4), o_cand = a.take(total_d2 * 4),
               o_part = a.take(mr.pair.size() * 16), o_out = a.take(P * sizeof(MonOut)),
               o_dist = a.take(want_dist ? total_d2 * 4 : 0);
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  HIPC(ensure(ctx->mon_ws, a.off));
  // pinned: the tables, the packed points, then the results (and the distances) coming back
  Arena h;
  const size_t h_meta = h.take(meta_bytes), h_pts = h.take(R ? 0 : total * 16), h_out = h.take(P * sizeof(MonOut)),
               h_dist = h.take(want_dist ? total * 4 : 0);
  HIPC(ensure(ctx->pin_mon, h.off));
  for (auto& e : ctx->mon_ev)
    if (!e) HIPC(hipEventCreate(&e));
  char* hm = ctx->pin_mon.as<char>() + h_meta;
  char* dv = ctx->mon_ws.as<char>();
  auto put = [&](size_t off, const void* src, size_t bytes) {
    if (bytes) std::memcpy(hm + off, src, bytes);
  };
  auto put_map = [&](size_t off, const Maps& m) {
    put(off, m.pair.data(), m.pair.size() * 4);
    put(off + m.pair.size() * 4, m.start.data(), m.start.size() * 4);
  };
  auto dev_map = [&](size_t off, const Maps& m) {
    return BlockMap{(const int32_t*)(dv + off), (const uint32_t*)(dv + off + m.pair.size() * 4), (uint32_t)m.pair.size()};
  };
  put(o_td, tdesc.data(), nT * sizeof(PairDesc));
  if (trees2) put(o_td2, tdesc.data(), P * sizeof(PairDesc));
  put(o_sa, segA.data(), segA.size() * sizeof(MonSeg));
  put(o_ca, chunkA.data(), chunkA.size() * 4);
  put(o_sb, segB.data(), segB.size() * sizeof(MonSeg));
  put(o_cb, chunkB.data(), chunkB.size() * 4);
  put(o_sq, selq.data(), selq.size() * sizeof(PairDesc));
  put_map(o_mq, mq);
  put(o_sp, selp.data(), selp.size() * sizeof(PairDesc));
  put_map(o_mp, mpm);
  put(o_rd, red.data(), red.size() * sizeof(MonRed));
  put_map(o_mr, mr);
  put(o_pr, mp.data(), P * sizeof(MonPair));
  put(o_xf, xf.data(), P * sizeof(uint2));
  put_map(o_mx, mx);
  if (T) put(o_T, T, P * 64);
  float4* raw = (float4*)(dv + o_raw);
  PairDesc* dTd = (PairDesc*)(dv + o_td);
  PairDesc* dTd2 = (PairDesc*)(dv + o_td2);
  int rc = AICP_OK;
  float* d2 = (float*)(dv + o_d2);
  uint32_t* ctr = (uint32_t*)(dv + o_ctr);
  const float inf = std::numeric_limits<float>::infinity();
  const float maxE2 = paired ? (1 + cfg->nn_epsilon) * (1 + cfg->nn_epsilon) : 1.f;
  const float maxR2 = paired ? cfg->nn_max_dist * cfg->nn_max_dist : inf;
  if (R) {
    // ---- the resident front end: the tables up, both clouds into the arena on the device -----------
    HIPC(hipMemcpyAsync(dv, hm, meta_bytes, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(dv + o_zero, 0, zero_bytes, s));
    launch_mon_stage(s, (uint32_t)total_ref, (uint32_t)total_out, R->ref, R->read, R->T, raw);
    HIPC(hipGetLastError());
    // ---- trees: each built alone, its levels planned as run_batch plans its own (a plan of 0, which
    // aicp_hip_options::tree_plan = -1 asks for there too, polls). The reference's lie in the caller's
    // buffers and are built only when they are not the current reference's; the reading's, over
    // `out`, is built every time. The planned builds leave their control blocks in pin_mon_ctl for
    // monitor_resident_check.
    MonRefTree& rt = *R->tree;
    TreeBufs& tb = ctx->tb_mon;
    HIPC(ensure(ctx->pin_mon_ctl, 3 * sizeof(TreeCtl)));
    TreeCtl* ctl = ctx->pin_mon_ctl.as<TreeCtl>();
    for (int& p : ctx->mon_planned) p = 0;
    const uint64_t n_max = std::max(total_ref, total_out);
    const int plan = plan_levels(n_max, tb, ctx->opt.tree_plan);
    // (the work space for the larger cloud first: it is not reallocated between the builds)
    rc = device_trees_begin(tb, ctx->err, s, 1, n_max, dTd + 1, raw, 0, kMonBucket, ctx->mon_bpts, ctx->mon_nodes, false);
    if (rc) return rc;
    auto build = [&](uint64_t n, PairDesc* desc, const float4* pts, int bucket, DevBuf& bpts, DevBuf& nodes, int slot) {
      int r = device_trees_begin(tb, ctx->err, s, 1, n, desc, pts, 0, bucket, bpts, nodes);
      if (!r) r = device_trees_end(tb, ctx->err, s, 1, n, desc, bucket, bpts, nodes, plan, ctl + slot);
      ctx->mon_planned[slot] = r ? 0 : tb.planned;
      // (a planned build's error is known on the device only: k_mon_guard keeps the searches out of
      // a tree deeper than their stacks; a polled build has returned it above)
      if (!r && tb.planned)
        launch_mon_guard(s, tb.tw.ctl, (MonSeg*)(dv + o_sa), (int)segA.size(), (MonSeg*)(dv + o_sb), (int)segB.size());
      return r;
    };
    HIPC(hipMemsetAsync(d2, 0, total_d2 * 4, s));  // (searches the guard switched off leave it defined)
    if (rt.valid) {
      ++R->cnt->reuses;
    } else {
      HIPC(ensure(rt.desc, sizeof(PairDesc)));
      HIPC(hipMemcpyAsync(rt.desc.p, hm + o_td, sizeof(PairDesc), hipMemcpyHostToDevice, s));
      rc = build(total_ref, rt.desc.as<PairDesc>(), raw, kMonBucket, rt.bpts, rt.nodes, 0);
      if (rc) return rc;
      rt.valid = true;
      ++R->cnt->trees;
    }
    if (trees2 && !(rt.valid2 && rt.bucket2 == cfg->bucket_size)) {
      rt.valid2 = false;
      HIPC(ensure(rt.desc2, sizeof(PairDesc)));
      HIPC(hipMemcpyAsync(rt.desc2.p, hm + o_td, sizeof(PairDesc), hipMemcpyHostToDevice, s));
      rc = build(total_ref, rt.desc2.as<PairDesc>(), raw, cfg->bucket_size, rt.bpts2, rt.nodes2, 1);
      if (rc) {
        rt.invalidate();
        return rc;
      }
      rt.valid2 = true;
      rt.bucket2 = cfg->bucket_size;
      ++R->cnt->trees2;
    }
    rc = build(total_out, dTd + 1, raw + total_ref, kMonBucket, ctx->mon_bpts, ctx->mon_nodes, 2);
    if (rc) {
      rt.invalidate();
      return rc;
    }
    ++R->cnt->trees;
    // ---- 1-NN: one launch per direction, the same searches in the same trees as the joined launch ----
    const MonSeg* sa = (const MonSeg*)(dv + o_sa);
    const uint32_t* ca = (const uint32_t*)(dv + o_ca);
    launch_mon_nn(s, slotsA, sa, ca, rt.desc.as<PairDesc>(), raw, rt.nodes.as<uint4>(), rt.bpts.as<float4>(), 1.f, inf, d2,
                  ctr);
    launch_mon_nn(s, slotsA1, sa + 1, ca, dTd + 1, raw, ctx->mon_nodes.as<uint4>(), ctx->mon_bpts.as<float4>(), 1.f, inf,
                  d2, ctr + kPersistCtrWords);
    if (eps_search)
      launch_mon_nn(s, slotsB, (const MonSeg*)(dv + o_sb), (const uint32_t*)(dv + o_cb),
                    (trees2 ? rt.desc2 : rt.desc).as<PairDesc>(), raw, (trees2 ? rt.nodes2 : rt.nodes).as<uint4>(),
                    (trees2 ? rt.bpts2 : rt.bpts).as<float4>(), maxE2, maxR2, d2, ctr + 2 * kPersistCtrWords);
    HIPC(hipGetLastError());
  } else {
    float* hp = reinterpret_cast<float*>(ctx->pin_mon.as<char>() + h_pts);
    std::vector<PackSeg> packs;
    for (size_t i = 0; i < P; ++i)
      packs.push_back(PackSeg{refs[i].p, refs[i].n, refs[i].stride, hp + 4ull * ref_off[i]});
    for (size_t i = 0; i < P; ++i)
      packs.push_back(PackSeg{outs[i].p, outs[i].n, outs[i].stride, hp + 4ull * (total_ref + out_loc[i])});
    pack_many(packs, ctx_pool(ctx));

    HIPC(hipEventRecord(ctx->mon_ev[0], s));
    HIPC(hipMemcpyAsync(dv, hm, meta_bytes, hipMemcpyHostToDevice, s));
    HIPC(hipMemcpyAsync(dv + o_raw, hp, total * 16, hipMemcpyHostToDevice, s));
    HIPC(hipMemsetAsync(dv + o_zero, 0, zero_bytes, s));
    if (T) launch_mon_transform(s, dev_map(o_mx, mx), (const uint2*)(dv + o_xf), (const float*)(dv + o_T), raw);
    HIPC(hipGetLastError());

    // ---- trees (host-polled levels, as the kernel-level entry points build theirs) ----------------
    rc = device_trees_begin(ctx->tb[0], ctx->err, s, nT, total, dTd, raw, 0, kMonBucket, ctx->mon_bpts, ctx->mon_nodes);
    if (rc) return rc;
    rc = device_trees_end(ctx->tb[0], ctx->err, s, nT, total, dTd, kMonBucket, ctx->mon_bpts, ctx->mon_nodes, 0);
    if (rc) return rc;
    if (trees2) {
      rc = device_trees_begin(ctx->tb[0], ctx->err, s, P, total_ref, dTd2, raw, 0, cfg->bucket_size, ctx->mon_bpts2,
                              ctx->mon_nodes2);
      if (rc) return rc;
      rc = device_trees_end(ctx->tb[0], ctx->err, s, P, total_ref, dTd2, cfg->bucket_size, ctx->mon_bpts2,
                            ctx->mon_nodes2, 0);
      if (rc) return rc;
    }
    HIPC(hipEventRecord(ctx->mon_ev[1], s));

    // ---- 1-NN: squared distances only ---------------------------------------------------------------
    launch_mon_nn(s, slotsA, (const MonSeg*)(dv + o_sa), (const uint32_t*)(dv + o_ca), dTd, raw,
                  ctx->mon_nodes.as<uint4>(), ctx->mon_bpts.as<float4>(), 1.f, inf, d2, ctr);
    if (eps_search)
      launch_mon_nn(s, slotsB, (const MonSeg*)(dv + o_sb), (const uint32_t*)(dv + o_cb), trees2 ? dTd2 : dTd, raw,
                    (trees2 ? ctx->mon_nodes2 : ctx->mon_nodes).as<uint4>(),
                    (trees2 ? ctx->mon_bpts2 : ctx->mon_bpts).as<float4>(), maxE2, maxR2, d2, ctr + kPersistCtrWords);
    HIPC(hipGetLastError());
    HIPC(hipEventRecord(ctx->mon_ev[2], s));
  }

  // ---- quantiles (the exact select), reduction, results ---------------------------------------------
  uint32_t* hist = (uint32_t*)(dv + o_hist);
  uint32_t* cand = (uint32_t*)(dv + o_cand);
  uint32_t* cnt = (uint32_t*)(dv + o_cnt);
  PairState* stq = (PairState*)(dv + o_stq);
  PairState* stp = (PairState*)(dv + o_stp);
  launch_init_state(s, (int)selq.size(), (const PairDesc*)(dv + o_sq), stq);
  launch_icp_select(s, dev_map(o_mq, mq), (int)selq.size(), (const PairDesc*)(dv + o_sq), stq, d2, hist, cand, cnt);
  if (paired) {  // (after the quantiles: both may read the same distances, and leave the work space zeroed)
    launch_init_state(s, (int)selp.size(), (const PairDesc*)(dv + o_sp), stp);
    launch_icp_select(s, dev_map(o_mp, mpm), (int)selp.size(), (const PairDesc*)(dv + o_sp), stp, d2, hist, cand, cnt);
  }
  float* ddist = want_dist ? (float*)(dv + o_dist) : nullptr;
  launch_mon_reduce(s, dev_map(o_mr, mr), (const MonRed*)(dv + o_rd), d2, paired ? stp : nullptr, prm->max_accepted_dist,
                    (MonAcc*)(dv + o_acc), (double*)(dv + o_part), ddist);
  launch_mon_finish(s, (int)P, (const MonPair*)(dv + o_pr), (const MonRed*)(dv + o_rd), (const MonAcc*)(dv + o_acc),
                    (const double*)(dv + o_part), stq, paired ? stp : nullptr, R ? R->result : (MonOut*)(dv + o_out));
  HIPC(hipGetLastError());
  if (R) return AICP_OK;  // (the result stays on the device: the caller's read-back brings it)
  HIPC(hipEventRecord(ctx->mon_ev[3], s));
  char* ho = ctx->pin_mon.as<char>() + h_out;
  HIPC(hipMemcpyAsync(ho, dv + o_out, P * sizeof(MonOut), hipMemcpyDeviceToHost, s));
  float* hd = reinterpret_cast<float*>(ctx->pin_mon.as<char>() + h_dist);
  if (want_dist) HIPC(hipMemcpyAsync(hd, ddist, total * 4, hipMemcpyDeviceToHost, s));
  HIPC(hipEventRecord(ctx->mon_ev[4], s));
  HIPC(hipStreamSynchronize(s));
  // (k_mon_finish leaves the quantile selects' status in pad: a direction without a finite distance)
  for (size_t i = 0; i < P; ++i)
    if (reinterpret_cast<const MonOut*>(ho)[i].pad)
      FAIL(AICP_ERR_CONVERGENCE, "monitor: no finite distance in pair " + std::to_string(i));
  std::memcpy(res, ho, P * sizeof(MonOut));
  if (dist_out) std::memcpy(dist_out, hd + dA(0), outs[0].n * 4);
  if (dist_ref) std::memcpy(dist_ref, hd + dB(0), refs[0].n * 4);
  aicp_monitor_stats& st = ctx->last_mon;
  st.trees_ms = ev_ms(ctx->mon_ev[0], ctx->mon_ev[1]);
  st.nn_ms = ev_ms(ctx->mon_ev[1], ctx->mon_ev[2]);
  st.reduce_ms = ev_ms(ctx->mon_ev[2], ctx->mon_ev[3]);
  st.device_ms = ev_ms(ctx->mon_ev[0], ctx->mon_ev[4]);
  st.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  return AICP_OK;
}

}  // namespace

namespace aicp {
namespace rt {

int monitor_params_check(aicp_hip_ctx* ctx, const aicp_monitor_params* prm) {
  if (!(prm->quantile >= 0.f && prm->quantile <= 1.f)) FAIL(AICP_ERR_INVALID, "monitor: quantile outside [0, 1]");
  return AICP_OK;
}

int MonState::set(aicp_hip_ctx* ctx, const aicp_monitor_params* p) {
  if (!p) {
    on = false;
    return AICP_OK;
  }
  const int rc = monitor_params_check(ctx, p);
  if (rc) return rc;
  prm = *p;
  on = true;
  return AICP_OK;
}

void MonState::take(aicp_hip_ctx* ctx, MonRefTree* tree, bool ran, const void* h_result, const std::string& err) {
  if (ran) {
    if (monitor_resident_check(ctx, tree, h_result) == AICP_OK) {
      std::memcpy(&last, h_result, sizeof(last));
      valid = 1;
      ++cnt.readings;
    }
  } else if (!err.empty()) {
    ctx->err = err;
  }
}

int monitor_resident(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg,
                     const float4* d_ref, size_t n_ref, const float4* d_read, size_t n_read, const float* d_T,
                     MonRefTree* tree, MonCounters* cnt, void* d_result) {
  const MonCloud r{reinterpret_cast<const float*>(d_ref), n_ref, 16}, o{reinterpret_cast<const float*>(d_read), n_read, 16};
  const MonResident R{d_ref, d_read, d_T, tree, cnt, static_cast<MonOut*>(d_result)};
  const int rc = monitor_core(ctx, prm, cfg, 1, &r, &o, nullptr, nullptr, nullptr, nullptr, &R);
  if (rc) tree->invalidate();
  return rc;
}

int monitor_resident_check(aicp_hip_ctx* ctx, MonRefTree* tree, const void* h_result) {
  TreeBufs& tb = ctx->tb_mon;
  const TreeCtl* ctl = ctx->pin_mon_ctl.as<TreeCtl>();
  int rc = AICP_OK, needed = 0;
  for (int k = 0; k < 3; ++k) {
    if (!ctx->mon_planned[k]) continue;
    tb.planned = ctx->mon_planned[k];
    std::string err;
    const int r = device_trees_check_ctl(tb, ctl + k, err);
    needed = std::max(needed, tb.needed);  // (the next plan follows the deepest of the builds)
    if (r && !rc) {
      rc = r;
      ctx->err = "monitor: " + err;
    }
    ctx->mon_planned[k] = 0;
  }
  if (needed) tb.needed = needed;
  if (!rc && static_cast<const MonOut*>(h_result)->pad) {
    rc = AICP_ERR_CONVERGENCE;
    ctx->err = "monitor: a direction without a finite distance";
  }
  if (rc) tree->invalidate();
  return rc;
}

}  // namespace rt
}  // namespace aicp

extern "C" {

void aicp_hip_default_monitor_params(aicp_monitor_params* p) {
  if (!p) return;
  *p = aicp_monitor_params{};
  p->quantile = 0.60f;           // icpMonitor.cpp:31
  p->max_accepted_dist = 0.20;   // :128
}

int aicp_hip_monitor(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg, const aicp_cloud* ref,
                     const aicp_cloud* out, const float T[16], aicp_monitor_result* result, float* dist_out,
                     float* dist_ref) {
  if (!ctx || !prm || !ref || !out || !result) return AICP_ERR_INVALID;
  const MonCloud r{ref->pts, ref->n, ref->stride}, o{out->pts, out->n, out->stride};
  return monitor_core(ctx, prm, cfg, 1, &r, &o, T, result, dist_out, dist_ref);
}

int aicp_hip_monitor_batch(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg,
                           const aicp_pair* pairs, size_t n, const float* T, aicp_monitor_result* out) {
  if (!ctx || !prm || !pairs || !out) return AICP_ERR_INVALID;
  if (n == 0 || n > (size_t)kMaxPairs) FAIL(AICP_ERR_INVALID, "monitor: no pair or more than 4096");
  std::vector<MonCloud> r(n), o(n);
  for (size_t i = 0; i < n; ++i) {
    r[i] = MonCloud{pairs[i].ref, pairs[i].n_ref, pairs[i].ref_stride};
    o[i] = MonCloud{pairs[i].read, pairs[i].n_read, pairs[i].read_stride};
  }
  return monitor_core(ctx, prm, cfg, n, r.data(), o.data(), T, out, nullptr, nullptr);
}

int aicp_hip_last_monitor_stats(const aicp_hip_ctx* ctx, aicp_monitor_stats* out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = ctx->last_mon;
  return AICP_OK;
}

}  // extern "C"
