// map_stream.cpp — App's localization streams on a device-resident map (processCloud
// app.cpp:282-414): on the prior map (aicp_hip_map_sequence_run; localize_against_prior_map,
// setReference app.cpp:37-58, map maintenance app.cpp:469-493) and on the map App has built itself
// (aicp_hip_built_map_sequence_run; localize_against_built_map, setReference app.cpp:60-69). Rules:
// include/aicp_hip.h. One driver (run_stream) serves both; what differs comes in as a Stream value.
//
// The map changes only after an accepted reading (a merge, a re-filter, a new reference), and when
// it does depends on a running count of accepted readings alone. Readings between two map changes
// see the same map, so they are independent: they run as one batch (a window), cropped on the
// device straight into the batch's reference array like aicp_hip_map_register_batch. The window
// ends where the next map change would fall if every reading were accepted
// (aicp_hip_localization_window, aicp_hip_built_map_window); a dropped reading only postpones the
// change, so the map is still unchanged at the end of the window and the next, shorter window goes
// on from the count reached. Nothing is run twice.
//
// Per window: [host] crop frames -> [device] crop counts -> [host] sizes the batch (one sync, as
// the batch call) -> [device] crop scatter, (debug mode: the reading moved by initialT_), (built
// map: overlap -> ratio beside the) trees, normals, ICP loop, finalize (run_batch) -> [device]
// k_stream_commit: drop test, count, corrected origin, initialT_, append / re-filter flags ->
// [host] reads the state and the records once -> [device] for the records that ask for it, in
// order: k_transform from the batch's copy of the reading by the device's correction to the map's
// tail, the map's pre-filter. No reading crosses the bus a second time.
//
// Raw readings (the *_run_raw entry points; setAndFilterReading, app.cpp:77-100): before the
// window's crop every raw reading is uploaded, unpacked and (debug mode) moved by the device's
// initialT_ (k_stream_ingest), pre-filtered (stream_prefilter_raw, aicp_hip.cpp), and its kept
// points wait on the device for the batch; the rest of the window is the same.
//
// Live map sessions (aicp_hip_map_session_*): the same window (stream_window) with one reading and
// a state that persists between calls in the session's own device block. There the append is
// decided on the device: the host makes room in the map before the crop when the mirrored count
// says the reading appends if accepted, k_session_map_append runs right behind k_stream_commit and
// does what the record says, and after the one read-back the host only adds to the map's size.
// With the quality monitor on (aicp_hip_mapsession_set_monitor) a registered reading's metrics
// against its crop are enqueued behind the batch and ahead of the commit (monitor_resident,
// monitor.cpp), and their 56 bytes come back in that read-back.
//
// A risk session (aicp_hip_mapsession_create_risk: failure_prediction_mode, runAicpPipeline
// app.cpp:236-245 and the gated branch app.cpp:401-411 under the two map policies) splits the
// reading's batch in two and puts the gate between, on the same crop: (built map) overlap-only batch
// -> alignment features with the FOV filters reading the crop and the reading where the batch holds
// them -> k_svm_predict -> k_session_map_gate -> [host] one read-back of state, record and the gate's
// record. A gated reading ends there; otherwise the ICP-only batch at the device's ratio, then the
// commit, the append and the read-back as above.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

namespace aicp {
namespace rt {

struct StreamTiming {
  int windows = 0, appends = 0, refilters = 0;
  double wall_ms = 0, device_ms = 0;
};

struct MapStreamBufs {
  DevBuf win;     // StreamState, then (at kRecOff) a StreamRec per reading of the window
  DevBuf origin;  // prior-pose translations of the window's readings, 3 doubles each
  PinBuf pin;     // staging: win's mirror, then the origins
  DevBuf stage;   // raw streams: the window's pre-filtered readings, one after another
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  StreamTiming last[2];  // of the last call of each stream: [0] prior map, [1] built map
};

void map_stream_bufs_free(MapStreamBufs* L) {
  if (!L) return;
  release(L->win);
  release(L->origin);
  release(L->pin);
  release(L->stage);
  if (L->ev_begin) (void)hipEventDestroy(L->ev_begin);
  if (L->ev_end) (void)hipEventDestroy(L->ev_end);
  delete L;
}

}  // namespace rt
}  // namespace aicp

namespace {

constexpr size_t kRecOff = 128;  // the records behind the state, in MapStreamBufs::win and its mirror
static_assert(sizeof(StreamState) <= kRecOff && kRecOff % alignof(StreamRec) == 0, "win's layout");

// run_stream writes both streams' results through aicp_localization_result: merged / refiltered
// are is_reference / pad (always 0) of aicp_built_map_result
#define SAME_FIELD(a, b) \
  static_assert(offsetof(aicp_localization_result, a) == offsetof(aicp_built_map_result, b), "result layout")
static_assert(sizeof(aicp_localization_result) == 128 && sizeof(aicp_built_map_result) == 128, "result layout");
SAME_FIELD(status, status);
SAME_FIELD(accepted, accepted);
SAME_FIELD(merged, is_reference);
SAME_FIELD(refiltered, pad);
SAME_FIELD(map_points, map_points);
SAME_FIELD(crop_points, crop_points);
SAME_FIELD(corrected_origin, corrected_origin);
SAME_FIELD(icp, icp);
#undef SAME_FIELD

constexpr int kLocFlags = AICP_LOC_MERGE | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;
constexpr int kBmFlags = AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;

bool valid_params(const aicp_localization_params* p) {
  return p && p->reference_update_frequency >= 1 && p->map_refilter_every >= 0 && !(p->flags & ~kLocFlags) &&
         p->max_correction_magnitude == p->max_correction_magnitude;
}
bool valid_params(const aicp_built_map_params* p) {
  return p && p->reference_update_frequency >= 1 && !(p->flags & ~kBmFlags) &&
         p->max_correction_magnitude == p->max_correction_magnitude && p->crop_min == p->crop_min &&
         p->crop_max == p->crop_max && (!(p->flags & AICP_RUN_OVERLAP) || p->resolution > 0);
}

// What differs between the two streams (exactly one of loc / bm is set)
struct Stream {
  const aicp_localization_params* loc;
  const aicp_built_map_params* bm;
  const aicp_prefilter_params* pf;  // prior map: the re-filter's parameters
  const aicp_prefilter_params* pf_read;  // raw streams: the readings' pre-filter (null: pre-filtered readings)
  StreamRules rules;
  float crop_min, crop_max;
  bool debug;
  int run_flags;      // run_batch's
  double resolution;  // the overlap's (built map)
};

// the entry points' argument checks before their parameters'
int stream_args(aicp_hip_ctx* ctx, const void* cfg, const void* prm, const aicp_hip_map* map,
                const aicp_cloud* readings, const float* poses, size_t n, const float* out_T, const void* out,
                size_t* n_done) {
  if (!ctx || !n_done) return AICP_ERR_INVALID;
  *n_done = 0;
  if (!cfg || !prm || !map || (n && (!readings || !poses || !out_T || !out))) return AICP_ERR_INVALID;
  return AICP_OK;
}

// Where a window's state, records and prior origins live: the streams' own buffers (MapStreamBufs)
// or a live session's block. On the device the records lie kRecOff behind the state, as in the mirror.
struct WinBlock {
  StreamState* dS;
  StreamRec* dRec;
  double* dOrg;
  char* pin;      // the host's mirror of state and records, read back once per window
  double* horg;   // pinned staging of the origins
  DevBuf* stage;  // raw readings: the window's pre-filtered readings, one after another
};

// A live session's reading (a window of one): where its rows lie, and its append, which the device
// decides behind the commit (launch_session_map_append) once the host has made room for it
struct Live {
  const float4* dpts = nullptr;  // the sweep accumulator's cloud where it lies (null: the caller's rows)
  size_t dn = 0;
  hipEvent_t ev_done = nullptr;  // recorded behind the commit and the append
  bool reserved = false;         // room was made in the map: the append kernel runs
  bool registered = false;       // the window reached its batch (ev_done is recorded)
  // the session's quality monitor (null: off): its counters, where its 56 bytes go in the session's
  // block (read back with the record), whether it was enqueued, and its own error if it was not
  const aicp_monitor_params* mon = nullptr;
  MonCounters* mon_cnt = nullptr;
  size_t mon_off = 0;
  bool mon_ran = false;
  std::string mon_err;
  // a risk session's gate (null: a plain session): the features' parameters, the caller's model, the
  // threshold, the reading's prior pose (column-major double), where the gate's record and the prior
  // map's constant overlap lie in the session's block, and the pipeline's record for the caller
  struct Risk {
    const aicp_risk_params* prm;
    const aicp_hip_svm* model;
    double threshold;
    const double* pose;
    size_t gate_off, fifty_off, back;  // back: the read-back that brings state | record | gate record
    aicp_pipeline_record* rec;
  };
  const Risk* risk = nullptr;
};

// how a window ended its stream, if it did
struct WinEnd {
  int status = AICP_OK;
  bool empty_crop = false, empty_read = false;
};

// A risk session's reading between its crop and its commit: runAicpPipeline's overlap, features,
// classifier and gate (app.cpp:236-245) on the batch's crop and reading where they lie, the gated
// branch taken on the device (k_session_map_gate), one read-back. *gated: the reading ended here
// (out is filled, the map changed as its record says). end->status: the overlap, the features or the
// classifier failed (out is filled). Otherwise the ICP-only batch at the device's ratio has run
// (st: its stats with the overlap's put in) and the caller goes on with the commit.
int gate_reading(aicp_hip_ctx* ctx, const Stream& P, const aicp_icp_config* cfg, aicp_hip_map* map, const WinBlock& K,
                 aicp_hip_batch* B, uint32_t crop_n, size_t map_n, float* out_T, aicp_localization_result* out,
                 aicp_icp_stats& st, StreamTiming& tm, Live* live, bool* gated, WinEnd* end) {
  const Live::Risk& R = *live->risk;
  hipStream_t s = ctx->stream;
  char* d = reinterpret_cast<char*>(K.dS);
  GateRec* dGate = reinterpret_cast<GateRec*>(d + R.gate_off);
  const StreamState* hS = reinterpret_cast<const StreamState*>(K.pin);
  const PairDesc& pd = B->desc[0];
  const float4* dref = B->ref_raw.as<float4>() + B->rdesc[0].ref_off;
  const float4* dread = B->read_raw.as<float4>() + pd.read_off;
  aicp_pipeline_record* prec = R.rec;
  prec->n_read = pd.n_read;
  auto failed = [&](int rc) {  // the reading's status: the session ends at it
    aicp_localization_result& o = out[0];
    std::memset(&o, 0, sizeof(o));
    o.status = o.icp.status = rc;
    o.map_points = map_n;
    o.crop_points = crop_n;
    o.icp.overlap_percent = -1.f;
    end->status = rc;
    return AICP_OK;
  };
  // the reading's pose as setAndFilterReading leaves it (app.cpp:87-96: debug mode, initialT_ * prior
  // pose, from the mirror of the device's initialT_); the reference's is the prior pose as given
  double prior[16];
  if (P.debug)
    pose_moved(hS->initT, R.pose, prior);
  else
    std::memcpy(prior, R.pose, sizeof(prior));
  // 1. computeOverlap. Built map: an overlap-only batch on the crop. Prior map: octree_overlap_ = 50.0
  // (app.cpp:123-127), no octree
  aicp_icp_stats ost{};
  int rc;
  if (P.bm) {
    ost.status = -1;
    rc = run_batch(ctx, B, cfg, P.resolution, AICP_RUN_OVERLAP, nullptr, &ost, nullptr);
    if (rc && ost.status == -1) return rc;  // the batch did not run to its end
    if (rc) {
      ctx->err = "overlap: " + ctx->err;
      return failed(rc);
    }
  } else {
    HIPC(ensure(ctx->outT, 64));  // (the gate kernel's correction slot; no batch has sized it yet)
  }
  // 2. and 3. the features on the crop and the reading where the batch holds them (the features'
  // pre-filters write the context's work space, never the batch's own ref_raw / read_raw; its
  // descriptors go up again with the next run_batch), the classifier, the gate and the ratio
  float fov = 0.f;
  aicp_cloud ca{}, cb{};
  ca.n = crop_n, cb.n = pd.n_read;
  ca.stride = cb.stride = 16;
  rc = gate_resident(ctx, R.prm, R.model, R.threshold, ca, cb, dref, dread, R.pose, prior, dGate, &fov,
                     P.bm ? nullptr : reinterpret_cast<const float*>(d + R.fifty_off));
  if (rc) {
    ctx->err = "risk gate: " + ctx->err;
    return failed(rc);
  }
  // 4. the gated branch, on the device; one read-back
  if (P.bm && !live->reserved) FAIL(AICP_ERR_HIP, "map session: no room was made for a gated reading");
  launch_session_map_gate(s, (int)pd.n_read, P.rules, dGate, K.dOrg, dread,
                          P.bm ? map->pts.as<float4>() + map->n : nullptr, ctx->outT.as<float>(), K.dS, K.dRec);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(live->ev_done, s));
  HIPC(hipMemcpyAsync(K.pin, d, R.back, hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  const GateRec g = *reinterpret_cast<const GateRec*>(K.pin + R.gate_off);
  prec->fov_overlap = fov;
  prec->octree_overlap = g.overlap;
  prec->alignability = g.alignability;
  prec->raw = g.raw;
  prec->risk = g.risk;
  prec->trimmed_ratio = g.ratio;
  prec->registered = g.gate ? 0 : 1;
  if (g.gate) {
    // app.cpp:401-411: the correction is the identity, initialT_ stays, no drop test
    const StreamRec& r = *reinterpret_cast<const StreamRec*>(K.pin + kRecOff);
    if (r.status != 0 || !r.accepted || r.append != (P.bm ? 1 : 0))
      FAIL(AICP_ERR_HIP, "map session: the gated reading's record");
    live->registered = true;  // (ev_done is recorded)
    aicp_localization_result& o = out[0];
    std::memset(&o, 0, sizeof(o));
    o.accepted = 1;
    o.map_points = map_n;
    o.crop_points = crop_n;
    for (int k = 0; k < 3; ++k) o.corrected_origin[k] = r.corrected_origin[k];
    o.icp.overlap_percent = g.overlap;
    o.icp.trimmed_ratio = g.ratio;
    for (int k = 0; k < 3; ++k) o.icp.overlap_keys[k] = ost.overlap_keys[k];
    ident4(out_T);
    if (r.append) {  // built map: the reading is the reference at once (done on the device already)
      map->n += pd.n_read;
      o.merged = 1;
      ++tm.appends;
    }
    if (r.refilter) {  // prior map: app.cpp:487-493 stands outside the merge and still applies
      rc = aicp_hip_map_prefilter(ctx, map, P.pf);
      if (rc) return rc;
      o.refiltered = 1;
      ++tm.refilters;
    }
    *gated = true;
    return AICP_OK;
  }
  // 5. computeRegistration at the device's ratio (app.cpp:243-245): an ICP-only batch on the same crop
  aicp_icp_config c2 = *cfg;
  c2.trimmed_ratio = g.ratio;
  st.status = -1;
  rc = run_batch(ctx, B, &c2, 0.0, AICP_RUN_ICP | (P.run_flags & AICP_RUN_TIME_NN), out_T, &st, nullptr);
  if (rc && st.status == -1) return rc;
  if (P.bm) {
    st.overlap_percent = g.overlap;
    for (int k = 0; k < 3; ++k) st.overlap_keys[k] = ost.overlap_keys[k];
  }
  return AICP_OK;
}

// One window: the w readings at `readings` / `poses`, which see the same map. Pre-filter or ingest,
// crop, staging copy, (debug mode) move, batch, commit, one read-back, the map changes the records
// ask for. Records and corrections go to out / out_T from index 0; *n_done = base + the records
// filled so far. *wr: the readings that ran. kept: raw readings, what the pre-filter kept of each.
// live (nullable): a session's call (w = 1).
int stream_window(aicp_hip_ctx* ctx, const Stream& P, const aicp_icp_config* cfg, aicp_hip_map* map,
                  const WinBlock& K, const aicp_cloud* readings, const float* poses, size_t w, float* out_T,
                  aicp_localization_result* out, std::vector<uint32_t>& kept, std::vector<aicp_icp_stats>& stats,
                  StreamTiming& tm, Live* live, size_t base, size_t* n_done, size_t* wr_out, WinEnd* end) {
  const bool raw = P.pf_read != nullptr;
  hipStream_t s = ctx->stream;
  StreamState* dS = K.dS;
  const StreamState* hS = reinterpret_cast<const StreamState*>(K.pin);
  const StreamRec* hrec = reinterpret_cast<const StreamRec*>(K.pin + kRecOff);
  double* horg = K.horg;
  int rc = AICP_OK;
  *wr_out = 0;
  const size_t map_n = map->n;
  // built map, debug mode (one reading per window): the overlap's sensor origin of the moved
  // reading, the translation of initialT_ * prior pose, from the mirror of the device's initialT_
  // (k_loc_move computes the same for the commit, on the device)
  double moved[3];
  const bool use_moved = P.bm && P.debug;
  if (use_moved) corrected_origin(hS->initT, readings[0].origin, moved);
  // every reading's crop, straight into the batch's reference array (as the batch call). An
  // empty crop ends the stream at its reading; the wr readings before it still run
  size_t wr = 0;
  const uint32_t* htot = nullptr;
  // raw streams: setAndFilterReading (app.cpp:77-100) for every reading of the window, before the
  // crop (the pre-filter and the crop share work space with the batch, not with each other: each
  // is done before the next starts). The kept points wait in the stage, sized once for the window
  // (the voxel grid never adds a point). Debug mode (one reading per window): the ingest kernel
  // moves the raw points and the prior origin by the device's initialT_. A reading the pre-filter
  // empties ends the window before it, as an empty crop does
  size_t wp = w;  // readings that reach the crop
  if (raw) {
    uint64_t sum = 0;
    for (size_t i = 0; i < w; ++i) sum += readings[i].n;
    HIPC(ensure(*K.stage, sum * 16));
    kept.assign(w, 0u);
    if (P.debug) {
      for (int k = 0; k < 3; ++k) horg[k] = readings[0].origin[k];
      HIPC(hipMemcpyAsync(K.dOrg, horg, 24, hipMemcpyHostToDevice, s));
    }
    uint64_t off = 0;
    for (size_t i = 0; i < w; ++i) {
      const aicp_cloud& c = readings[i];
      rc = stream_ingest_rows(ctx, P.pf_read, c.pts, c.n, c.stride, live ? live->dpts : nullptr,
                              P.debug ? dS->initT : nullptr, P.debug ? K.dOrg : nullptr,
                              K.stage->as<float4>() + off, &kept[i]);
      if (rc) return rc;
      if (!kept[i]) {
        wp = i;
        break;
      }
      off += kept[i];
    }
  }
  // a session's reading: room in the map now, while nothing that reads the map is in flight (the
  // pre-filter has returned with the stream idle; growing synchronises and may move the map), if
  // the mirrored count says this reading appends when it is accepted (k_stream_commit's rule)
  if (live && wp) {
    const int32_t c = hS->count;
    // (a risk session on the built map: every reading, because any reading may be gated)
    const bool appends =
        P.bm ? (c + 1 == P.rules.freq || live->risk) : (P.rules.merge && c % P.rules.freq == 0);
    if (appends) {
      rc = map_reserve(ctx, map, raw ? (size_t)kept[0] : (size_t)readings[0].n);
      if (rc) return rc;
      live->reserved = true;
    }
  }
  if (wp) {
    rc = map_crop_pairs(ctx, map, P.crop_min, P.crop_max, readings, poses, wp, use_moved ? moved : nullptr, &wr,
                        &htot, raw ? kept.data() : nullptr);
    if (rc) return rc;
  }
  *wr_out = wr;
  if (wr) {
    aicp_hip_batch* B = ctx->mapbatch;
    if (raw) {  // the staged readings into the batch (its sizes are known only after the crop)
      uint64_t off = 0;
      for (size_t i = 0; i < wr; ++i) {
        HIPC(hipMemcpyAsync(B->read_raw.as<float4>() + B->desc[i].read_off, K.stage->as<float4>() + off,
                            (size_t)kept[i] * 16, hipMemcpyDeviceToDevice, s));
        off += kept[i];
      }
    }
    if (!(raw && P.debug)) {  // (raw debug mode: up already, and moved by the ingest kernel)
      for (size_t i = 0; i < wr; ++i)
        for (int k = 0; k < 3; ++k) horg[3 * i + k] = readings[i].origin[k];
      HIPC(hipMemcpyAsync(K.dOrg, horg, wr * 24, hipMemcpyHostToDevice, s));
    }
    if (P.debug && !raw) {  // (one reading per window) moved by the device's initialT_, its prior pose too
      launch_loc_move(s, (int)B->desc[0].n_read, dS->initT, K.dOrg, B->read_raw.as<float4>() + B->desc[0].read_off);
      HIPC(hipGetLastError());
    }
    stats.assign(wr, aicp_icp_stats{});
    for (auto& st : stats) st.status = -1;
    if (live && live->risk) {
      bool gated = false;
      rc = gate_reading(ctx, P, cfg, map, K, B, htot[0], map_n, out_T, out, stats[0], tm, live, &gated, end);
      if (rc) return rc;
      if (gated || end->status) {
        *n_done = base + 1;
        return AICP_OK;
      }
    } else {
      rc = run_batch(ctx, B, cfg, P.resolution, P.run_flags, out_T, stats.data(), nullptr);
      if (rc && stats[0].status == -1) return rc;  // the batch did not run to its end (not a reading's status)
    }
    ++tm.windows;
    // a session's monitor of a registered reading, ahead of the commit and the append: the crop and
    // the reading where the batch holds them (the batch reads both only), the correction where the
    // batch left it, the chain at the reading's own ratio. An error of its own only costs the result.
    if (live && live->mon && stats[0].status == AICP_OK) {
      aicp_icp_config mc = *cfg;
      mc.trimmed_ratio = stats[0].trimmed_ratio;
      const std::string why = ctx->err;
      ctx->mon_scratch.invalidate();  // (the crop changes with every pose)
      live->mon_ran = monitor_resident(ctx, live->mon, &mc, B->ref_raw.as<float4>() + B->rdesc[0].ref_off, htot[0],
                                       B->read_raw.as<float4>() + B->desc[0].read_off, B->desc[0].n_read,
                                       ctx->outT.as<float>(), &ctx->mon_scratch, live->mon_cnt,
                                       reinterpret_cast<char*>(dS) + live->mon_off) == AICP_OK;
      if (!live->mon_ran) live->mon_err = ctx->err;
      ctx->err = why;
    }
    // App's bookkeeping for the window, on the device; one read-back of its state and records
    launch_stream_commit(s, (int)wr, ctx->state.as<PairState>(), ctx->outT.as<float>(), K.dOrg, P.rules, dS, K.dRec);
    HIPC(hipGetLastError());
    if (live) {
      // the session's append, by the record the commit has just written: no host decision in between
      if (live->reserved) {
        const PairDesc& d = B->desc[0];
        launch_session_map_append(s, (int)d.n_read, K.dRec, ctx->outT.as<float>(),
                                  B->read_raw.as<float4>() + d.read_off, map->pts.as<float4>() + map->n);
        HIPC(hipGetLastError());
      }
      HIPC(hipEventRecord(live->ev_done, s));
      live->registered = true;
    }
    const size_t back = live && live->mon_ran ? live->mon_off + sizeof(aicp_monitor_result) : kRecOff + wr * sizeof(StreamRec);
    HIPC(hipMemcpyAsync(K.pin, dS, back, hipMemcpyDeviceToHost, s));
    HIPC(hipStreamSynchronize(s));
    // the map changes the records ask for, in order (by the window rule: after the last reading)
    for (size_t i = 0; i < wr; ++i) {
      const StreamRec& r = hrec[i];
      aicp_localization_result& o = out[i];
      std::memset(&o, 0, sizeof(o));
      o.status = r.status;
      o.accepted = r.accepted;
      o.map_points = map_n;
      o.crop_points = htot[i];
      for (int k = 0; k < 3; ++k) o.corrected_origin[k] = r.corrected_origin[k];
      o.icp = stats[i];
      *n_done = base + i + 1;
      if (r.status) {
        end->status = r.status;
        break;
      }
      if (r.append) {
        const PairDesc& d = B->desc[i];
        if (live) {  // (done on the device already)
          if (!live->reserved) FAIL(AICP_ERR_HIP, "map session: the device's append disagrees with the host's count");
        } else {
          rc = map_reserve(ctx, map, d.n_read);
          if (rc) return rc;
          launch_transform(s, (int)d.n_read, ctx->outT.as<float>() + 16 * i, B->read_raw.as<float4>() + d.read_off,
                           map->pts.as<float4>() + map->n);
          HIPC(hipGetLastError());
        }
        map->n += d.n_read;
        o.merged = 1;
        ++tm.appends;
      }
      if (r.refilter) {
        rc = aicp_hip_map_prefilter(ctx, map, P.pf);
        if (rc) return rc;
        o.refiltered = 1;
        ++tm.refilters;
      }
    }
  }
  // the reading with the empty crop, or the one the pre-filter emptied (libpointmatcher throws on
  // an empty cloud); the lower index ends the stream (wr <= wp: the crop saw the readings before wp)
  if (!end->status && wr < w) {
    aicp_localization_result& o = out[wr];
    std::memset(&o, 0, sizeof(o));
    o.status = o.icp.status = AICP_ERR_INVALID;
    o.map_points = map_n;
    o.icp.overlap_percent = -1.f;
    ident4(out_T + 16 * wr);
    *n_done = base + wr + 1;
    end->status = AICP_ERR_INVALID;
    (wr < wp ? end->empty_crop : end->empty_read) = true;
  }
  return AICP_OK;
}

int run_stream(aicp_hip_ctx* ctx, const Stream& P, const aicp_icp_config* cfg, aicp_hip_map* map,
               const aicp_cloud* readings, const float* poses, size_t n, float* out_T, aicp_localization_result* out,
               uint32_t* out_kept, size_t* n_done) {
  const bool raw = P.pf_read != nullptr;
  if (out_kept) std::fill(out_kept, out_kept + n, 0u);
  for (size_t i = 0; i < n; ++i)
    if (!valid_cloud(readings[i])) FAIL(AICP_ERR_INVALID, "invalid reading " + std::to_string(i));
  int rc = check_cfg(ctx, cfg, P.run_flags);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!ctx->ms) ctx->ms = new MapStreamBufs();
  MapStreamBufs* L = ctx->ms;
  StreamTiming& tm = L->last[P.bm ? 1 : 0];
  tm = StreamTiming{};
  if (!L->ev_begin) HIPC(hipEventCreate(&L->ev_begin));
  if (!L->ev_end) HIPC(hipEventCreate(&L->ev_end));

  // the stream's state: count = 0, initialT_ = I
  const size_t wmax = std::min<size_t>(std::max<size_t>(n, 1), (size_t)kMaxPairs);
  const size_t o_org = (kRecOff + wmax * sizeof(StreamRec) + 63) & ~size_t(63);
  HIPC(ensure(L->win, kRecOff + wmax * sizeof(StreamRec)));
  HIPC(ensure(L->origin, wmax * 24));
  HIPC(ensure(L->pin, o_org + wmax * 24));
  char* lp = L->pin.as<char>();
  StreamState* dS = L->win.as<StreamState>();
  StreamRec* dRec = reinterpret_cast<StreamRec*>(L->win.as<char>() + kRecOff);
  StreamState* hS = reinterpret_cast<StreamState*>(lp);  // the host's mirror, read back with every window's records
  const WinBlock K{dS, dRec, L->origin.as<double>(), lp, reinterpret_cast<double*>(lp + o_org), &L->stage};
  std::memset(hS, 0, sizeof(StreamState));
  ident4(hS->initT);
  HIPC(hipMemcpyAsync(dS, hS, sizeof(StreamState), hipMemcpyHostToDevice, s));
  HIPC(hipEventRecord(L->ev_begin, s));
  std::vector<aicp_icp_stats> stats;
  int status = AICP_OK;
  size_t p = 0;
  bool empty_crop = false, empty_read = false;
  std::vector<uint32_t> kept;  // raw streams: what the pre-filter kept of the window's readings
  while (p < n && !status) {
    const size_t w = P.bm ? aicp_hip_built_map_window((uint64_t)hS->count, P.bm, n - p)
                          : aicp_hip_localization_window((uint64_t)hS->count, P.loc, n - p);
    if (P.bm && w == 0) FAIL(AICP_ERR_HIP, "built-map stream: the device's count left its range");
    size_t wr = 0;
    WinEnd end;
    rc = stream_window(ctx, P, cfg, map, K, readings + p, poses + 16 * p, w, out_T + 16 * p, out + p, kept, stats, tm,
                       nullptr, p, n_done, &wr, &end);
    if (rc) return rc;
    status = end.status;
    empty_crop = end.empty_crop;
    empty_read = end.empty_read;
    if (raw && out_kept)
      for (size_t i = 0; i < w && p + i < *n_done; ++i) out_kept[p + i] = kept[i];
    p += wr;
  }
  HIPC(hipEventRecord(L->ev_end, s));
  HIPC(hipStreamSynchronize(s));
  tm.device_ms = ev_ms(L->ev_begin, L->ev_end);
  tm.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (status)
    ctx->err = "reading " + std::to_string(*n_done - 1) +
               (empty_crop   ? std::string(": empty map crop")
                : empty_read ? std::string(": keeps no point after the pre-filter")
                             : ": status " + std::to_string(status));
  return status;
}

// the live map session's small device block and its pinned mirror: StreamState | StreamRec | the
// quality monitor's result | the reading's prior origin (3 doubles): the streams' window layout with
// one record, and the result right behind it, so that one read-back brings both. A risk session's
// gate record lies behind the origin (its read-back runs to the record's end), and behind that the
// prior map's constant overlap, 50.0f, written at start
constexpr size_t kSessMon = 192, kSessOrg = 256, kSessGate = 288, kSessFifty = 320, kSessBytes = 384;
static_assert(kRecOff + sizeof(StreamRec) <= kSessMon && kSessMon + sizeof(aicp_monitor_result) <= kSessOrg &&
                  kSessOrg + 24 <= kSessGate && kSessGate % alignof(GateRec) == 0 &&
                  kSessGate + sizeof(GateRec) <= kSessFifty && kSessFifty + 4 <= kSessBytes,
              "the session block's layout");

}  // namespace

struct aicp_hip_map_session {
  aicp_icp_config cfg{};
  aicp_localization_params loc{};
  aicp_built_map_params bm{};
  aicp_prefilter_params pf_read{}, pf_map{};
  Stream P{};  // points into the copies above
  DevBuf win;  // the block
  PinBuf pin;  // its mirror
  DevBuf read;  // raw readings: the last reading as it was registered (the pre-filter's kept points)
  aicp_hip_map* map = nullptr;  // the caller's
  uint64_t n_processed = 0;
  bool started = false, ended = false;
  uint64_t ended_at = 0;
  std::vector<uint32_t> kept;
  std::vector<aicp_icp_stats> stats;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  double last_wall_ms = 0, last_device_ms = 0;
  MonState mon;  // the per-reading quality monitor (aicp_hip_mapsession_set_monitor)
  // failure_prediction_mode (aicp_hip_mapsession_create_risk): the features' parameters, the caller's
  // model and the gate's threshold
  bool risk = false;
  aicp_risk_params rprm{};
  const aicp_hip_svm* model = nullptr;
  double threshold = 0;
};

extern "C" {

void aicp_hip_default_localization_params(aicp_localization_params* p) {
  if (!p) return;
  p->reference_update_frequency = 5;
  p->map_refilter_every = 30;
  p->max_correction_magnitude = 1.0f;
  p->crop_min = -15.0f;
  p->crop_max = 15.0f;
  p->flags = AICP_LOC_MERGE;
}

void aicp_hip_default_built_map_params(aicp_built_map_params* p) {
  if (!p) return;
  p->reference_update_frequency = 5;
  p->max_correction_magnitude = 1.0f;
  p->crop_min = -15.0f;
  p->crop_max = 15.0f;
  p->resolution = 0.2;
  p->flags = AICP_RUN_OVERLAP;
  p->pad = 0;
}

size_t aicp_hip_localization_window(uint64_t n_clouds, const aicp_localization_params* prm, size_t remaining) {
  if (!valid_params(prm) || remaining == 0) return 0;
  if (prm->flags & AICP_SEQ_DEBUG) return 1;
  size_t w = std::min<size_t>(remaining, (size_t)kMaxPairs);
  if (!(prm->flags & AICP_LOC_MERGE)) return w;
  // reading k of the window, if all before it are accepted too, is accepted as cloud n_clouds + k:
  // the map changes after it when (n_clouds + k - 1) is a multiple of a period
  auto to_next = [&](uint64_t period) -> uint64_t {
    const uint64_t r = n_clouds % period;  // (n_clouds + k - 1) % period == 0, k >= 1
    return r == 0 ? 1 : period - r + 1;
  };
  w = (size_t)std::min<uint64_t>(w, to_next((uint64_t)prm->reference_update_frequency));
  if (prm->map_refilter_every > 0) w = (size_t)std::min<uint64_t>(w, to_next((uint64_t)prm->map_refilter_every));
  return w;
}

size_t aicp_hip_built_map_window(uint64_t acc, const aicp_built_map_params* prm, size_t remaining) {
  if (!valid_params(prm) || remaining == 0 || acc >= (uint64_t)prm->reference_update_frequency) return 0;
  if (prm->flags & AICP_SEQ_DEBUG) return 1;
  // reading k of the window (k >= 1), if all before it are accepted too, is the (acc + k)-th
  // accepted since the last reference: the map changes after it when acc + k == frequency
  const uint64_t to_ref = (uint64_t)prm->reference_update_frequency - acc;
  return (size_t)std::min<uint64_t>(std::min<size_t>(remaining, (size_t)kMaxPairs), to_ref);
}

// the raw entry points' further checks (after stream_args): the readings' pre-filter
static int raw_args(aicp_hip_ctx* ctx, const aicp_prefilter_params* pf_read) {
  if (!pf_read) return AICP_ERR_INVALID;
  return stream_prefilter_check(ctx, pf_read);
}

// the two policies as the window code takes them (the parameters stay the caller's)
static Stream loc_rules(const aicp_localization_params* prm, const aicp_prefilter_params* pf,
                        const aicp_prefilter_params* pf_read) {
  Stream P{};
  P.loc = prm;
  P.pf = pf;
  P.pf_read = pf_read;
  P.rules.freq = prm->reference_update_frequency;
  P.rules.refilter_every = prm->map_refilter_every;
  P.rules.merge = (prm->flags & AICP_LOC_MERGE) ? 1 : 0;
  P.rules.max_corr = prm->max_correction_magnitude;
  P.crop_min = prm->crop_min;
  P.crop_max = prm->crop_max;
  P.debug = prm->flags & AICP_SEQ_DEBUG;
  P.run_flags = AICP_RUN_ICP | (prm->flags & AICP_RUN_TIME_NN);
  return P;
}

static Stream bm_rules(const aicp_built_map_params* prm, const aicp_prefilter_params* pf_read) {
  Stream P{};
  P.bm = prm;
  P.pf_read = pf_read;
  P.rules.built = 1;
  P.rules.freq = prm->reference_update_frequency;
  P.rules.overlap = (prm->flags & AICP_RUN_OVERLAP) ? 1 : 0;
  P.rules.max_corr = prm->max_correction_magnitude;
  P.crop_min = prm->crop_min;
  P.crop_max = prm->crop_max;
  P.debug = prm->flags & AICP_SEQ_DEBUG;
  P.run_flags = AICP_RUN_ICP | (prm->flags & (AICP_RUN_OVERLAP | AICP_RUN_TIME_NN));
  P.resolution = prm->resolution;
  return P;
}

// raw: readings as App receives them, pre-filtered by pf_read inside the stream
static int loc_stream(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                      const aicp_prefilter_params* pf, bool raw, const aicp_prefilter_params* pf_read,
                      aicp_hip_map* map, const aicp_cloud* readings, const float* poses, size_t n, float* out_T,
                      aicp_localization_result* out, uint32_t* out_kept, size_t* n_done) {
  int rc = stream_args(ctx, cfg, prm, map, readings, poses, n, out_T, out, n_done);
  if (!rc && raw) rc = raw_args(ctx, pf_read);
  if (rc) return rc;
  if (!valid_params(prm)) FAIL(AICP_ERR_INVALID, "localization parameters");
  aicp_prefilter_params pfd;
  if (!pf) {
    aicp_hip_default_prefilter(&pfd);
    pf = &pfd;
  }
  aicp_icp_config c = *cfg;
  c.trimmed_ratio = aicp_hip_autotune_ratio(50.0f);  // octree_overlap_ = 50.0 (app.cpp:123-127)
  return run_stream(ctx, loc_rules(prm, pf, raw ? pf_read : nullptr), &c, map, readings, poses, n, out_T, out,
                    out_kept, n_done);
}

static int bm_stream(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_built_map_params* prm, bool raw,
                     const aicp_prefilter_params* pf_read, aicp_hip_map* map, const aicp_cloud* readings,
                     const float* poses, size_t n, float* out_T, aicp_built_map_result* out, uint32_t* out_kept,
                     size_t* n_done) {
  int rc = stream_args(ctx, cfg, prm, map, readings, poses, n, out_T, out, n_done);
  if (!rc && raw) rc = raw_args(ctx, pf_read);
  if (rc) return rc;
  if (!valid_params(prm)) FAIL(AICP_ERR_INVALID, "built-map parameters");
  return run_stream(ctx, bm_rules(prm, raw ? pf_read : nullptr), cfg, map, readings, poses, n, out_T,
                    reinterpret_cast<aicp_localization_result*>(out), out_kept, n_done);
}

int aicp_hip_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                              const aicp_prefilter_params* pf, aicp_hip_map* map, const aicp_cloud* readings,
                              const float* poses, size_t n, float* out_T, aicp_localization_result* out,
                              size_t* n_done) {
  return loc_stream(ctx, cfg, prm, pf, false, nullptr, map, readings, poses, n, out_T, out, nullptr, n_done);
}

int aicp_hip_map_sequence_run_raw(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                                  const aicp_prefilter_params* pf_map, const aicp_prefilter_params* pf_read,
                                  aicp_hip_map* map, const aicp_cloud* readings, const float* poses, size_t n,
                                  float* out_T, aicp_localization_result* out, uint32_t* out_kept, size_t* n_done) {
  return loc_stream(ctx, cfg, prm, pf_map, true, pf_read, map, readings, poses, n, out_T, out, out_kept, n_done);
}

int aicp_hip_built_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_built_map_params* prm,
                                    aicp_hip_map* map, const aicp_cloud* readings, const float* poses, size_t n,
                                    float* out_T, aicp_built_map_result* out, size_t* n_done) {
  return bm_stream(ctx, cfg, prm, false, nullptr, map, readings, poses, n, out_T, out, nullptr, n_done);
}

int aicp_hip_built_map_sequence_run_raw(aicp_hip_ctx* ctx, const aicp_icp_config* cfg,
                                        const aicp_built_map_params* prm, const aicp_prefilter_params* pf_read,
                                        aicp_hip_map* map, const aicp_cloud* readings, const float* poses, size_t n,
                                        float* out_T, aicp_built_map_result* out, uint32_t* out_kept,
                                        size_t* n_done) {
  return bm_stream(ctx, cfg, prm, true, pf_read, map, readings, poses, n, out_T, out, out_kept, n_done);
}

int aicp_hip_last_localization_timing(const aicp_hip_ctx* ctx, aicp_localization_timing* out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  const StreamTiming t = ctx->ms ? ctx->ms->last[0] : StreamTiming{};
  *out = aicp_localization_timing{t.windows, t.appends, t.refilters, 0, t.wall_ms, t.device_ms};
  return AICP_OK;
}

int aicp_hip_last_built_map_timing(const aicp_hip_ctx* ctx, aicp_built_map_timing* out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  const StreamTiming t = ctx->ms ? ctx->ms->last[1] : StreamTiming{};
  *out = aicp_built_map_timing{t.windows, t.appends, t.wall_ms, t.device_ms};
  return AICP_OK;
}

// ---- the live map sessions: stream_window with w = 1 and a state that persists ----------------
// risk_prm (null: a plain session): failure_prediction_mode, with the caller's model and the threshold
static int map_session_make(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* loc,
                            const aicp_built_map_params* bm, const aicp_prefilter_params* pf_read,
                            const aicp_prefilter_params* pf_map, const aicp_risk_params* risk_prm,
                            const aicp_hip_svm* model, double threshold, aicp_hip_map_session** out) {
  if ((loc != nullptr) == (bm != nullptr)) FAIL(AICP_ERR_INVALID, "map session: exactly one of loc / bm");
  aicp_built_map_params bmo;
  if (bm && risk_prm) {  // (the overlap always runs: the classifier needs it)
    bmo = *bm;
    bmo.flags |= AICP_RUN_OVERLAP;
    bm = &bmo;
  }
  if (bm && pf_map) FAIL(AICP_ERR_INVALID, "map session: the built map is never re-filtered (pf_map)");
  if (loc && !valid_params(loc)) FAIL(AICP_ERR_INVALID, "localization parameters");
  if (bm && !valid_params(bm)) FAIL(AICP_ERR_INVALID, "built-map parameters");
  aicp_hip_map_session* s = new aicp_hip_map_session();
  s->cfg = *cfg;
  if (pf_read) s->pf_read = *pf_read;
  if (loc) {
    s->loc = *loc;
    if (pf_map)
      s->pf_map = *pf_map;
    else
      aicp_hip_default_prefilter(&s->pf_map);
    s->cfg.trimmed_ratio = aicp_hip_autotune_ratio(50.0f);  // octree_overlap_ = 50.0 (app.cpp:123-127)
    s->P = loc_rules(&s->loc, &s->pf_map, pf_read ? &s->pf_read : nullptr);
  } else {
    s->bm = *bm;
    s->P = bm_rules(&s->bm, pf_read ? &s->pf_read : nullptr);
  }
  if (risk_prm) {
    s->risk = true;
    s->rprm = *risk_prm;
    s->model = model;
    s->threshold = threshold;
    s->P.rules.overlap = 0;  // (the overlap is a batch of its own, its status checked before the gate)
  }
  int rc = check_cfg(ctx, &s->cfg, s->P.run_flags);
  if (!rc && pf_read) rc = stream_prefilter_check(ctx, pf_read);
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = ensure(s->win, kSessBytes);
    if (e == hipSuccess) e = ensure(s->pin, kSessBytes);
    if (e == hipSuccess) e = hipEventCreate(&s->ev_begin);
    if (e == hipSuccess) e = hipEventCreate(&s->ev_end);
  }
  if (rc || e != hipSuccess) {
    const std::string why = ctx->err;
    aicp_hip_map_session_free(nullptr, s);
    ctx->err = why;
    if (rc) return rc;
    HIPC(e);
  }
  *out = s;
  return AICP_OK;
}

int aicp_hip_map_session_create(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* loc,
                                const aicp_built_map_params* bm, const aicp_prefilter_params* pf_read,
                                const aicp_prefilter_params* pf_map, aicp_hip_map_session** out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!cfg) return AICP_ERR_INVALID;
  return map_session_make(ctx, cfg, loc, bm, pf_read, pf_map, nullptr, nullptr, 0.0, out);
}

int aicp_hip_mapsession_create_risk(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* loc,
                                    const aicp_built_map_params* bm, const aicp_prefilter_params* pf_read,
                                    const aicp_prefilter_params* pf_map, const aicp_risk_params* risk_prm,
                                    const aicp_hip_svm* model, double threshold, aicp_hip_map_session** out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!cfg || !risk_prm || !model) return AICP_ERR_INVALID;
  if (!(threshold == threshold)) FAIL(AICP_ERR_INVALID, "map session: threshold");
  const int rc = risk_params_check(ctx, risk_prm);
  return rc ? rc : map_session_make(ctx, cfg, loc, bm, pf_read, pf_map, risk_prm, model, threshold, out);
}

void aicp_hip_map_session_free(aicp_hip_ctx* ctx, aicp_hip_map_session* s) {
  if (!s) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  release(s->win);
  release(s->pin);
  release(s->read);
  if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
  if (s->ev_end) (void)hipEventDestroy(s->ev_end);
  delete s;
}

int aicp_hip_map_session_start(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_map* map) {
  if (!ctx || !s || !map) return AICP_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPC(hipStreamSynchronize(st));  // (the mirror is free)
  // count = 0, initialT_ = I, no record
  char* h = s->pin.as<char>();
  std::memset(h, 0, kSessBytes);
  ident4(reinterpret_cast<StreamState*>(h)->initT);
  *reinterpret_cast<float*>(h + kSessFifty) = 50.0f;  // octree_overlap_ on the prior map (app.cpp:123-127)
  HIPC(hipMemcpyAsync(s->win.p, h, kSessBytes, hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));
  s->map = map;
  s->n_processed = 0;
  s->started = true;
  s->ended = false;
  s->mon.none();
  return AICP_OK;
}

// goBackRequest (app_ros.cpp:329-357): the map App built becomes the prior map and the same App, with
// its graph and its initialT_, localises on it. The count comes from the live session's counter of
// accepted readings; initialT_ is copied from the live session's block device to device, behind
// everything on the stream, and this session's mirror is read back from its own block.
int aicp_hip_mapsession_start_go_back(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_map* map,
                                      const aicp_hip_session* from) {
  if (!ctx || !s || !map || !from) return AICP_ERR_INVALID;
  if (s->P.bm) FAIL(AICP_ERR_INVALID, "go-back: a built-map session localises on no prior map");
  uint64_t n_clouds = 0;
  const float* d_initT = nullptr;
  int rc = session_go_back(ctx, from, &n_clouds, &d_initT);
  if (rc) return rc;
  if (n_clouds > (uint64_t)INT32_MAX) FAIL(AICP_ERR_INVALID, "go-back: the graph's count");
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPC(hipStreamSynchronize(st));  // (the mirror is free)
  char* h = s->pin.as<char>();
  std::memset(h, 0, kSessBytes);
  StreamState* hS = reinterpret_cast<StreamState*>(h);
  ident4(hS->initT);
  hS->count = (int32_t)n_clouds;  // aligned_clouds_graph_->getNbClouds()
  *reinterpret_cast<float*>(h + kSessFifty) = 50.0f;  // octree_overlap_ on the prior map (app.cpp:123-127)
  HIPC(hipMemcpyAsync(s->win.p, h, kSessBytes, hipMemcpyHostToDevice, st));
  HIPC(hipMemcpyAsync(s->win.as<StreamState>()->initT, d_initT, 64, hipMemcpyDeviceToDevice, st));
  HIPC(hipMemcpyAsync(hS, s->win.p, sizeof(StreamState), hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  s->map = map;
  s->n_processed = 0;
  s->started = true;
  s->ended = false;
  s->mon.none();
  return AICP_OK;
}

int aicp_hip_mapsession_set_monitor(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_monitor_params* prm) {
  if (!ctx || !s) return AICP_ERR_INVALID;
  return s->mon.set(ctx, prm);
}

int aicp_hip_mapsession_last_monitor(const aicp_hip_map_session* s, aicp_monitor_result* out, int32_t* valid) {
  return s ? s->mon.get_last(out, valid) : AICP_ERR_INVALID;
}

int aicp_hip_mapsession_monitor_counters(const aicp_hip_map_session* s, uint64_t out[4]) {
  return s ? s->mon.counters(out) : AICP_ERR_INVALID;
}

// the call that ends the session (app.cpp:210: the worker ends), with its status
static int map_session_end(aicp_hip_ctx* ctx, aicp_hip_map_session* s, int rc) {
  s->ended = true;
  s->ended_at = s->n_processed;
  ++s->n_processed;
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// pose_d, prec: a risk session's call (the prior pose in double, column-major, and the pipeline's
// record); both null: a plain session's (pose). A handle of the other kind refuses the call.
static int map_session_process(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_cloud* reading,
                               aicp_hip_accum* acc, const float* pose, const double* pose_d, float* out_T, void* out,
                               aicp_pipeline_record* prec, uint32_t* kept_out) {
  const bool risk = pose_d != nullptr;
  if (!ctx || !s || (!reading && !acc) || (!pose && !pose_d) || !out_T || !out || (risk && !prec))
    return AICP_ERR_INVALID;
  if (s->risk != risk)
    FAIL(AICP_ERR_INVALID, risk ? "map session: not made by aicp_hip_mapsession_create_risk"
                                : "map session: a risk session takes the _risk calls");
  if (!s->started) FAIL(AICP_ERR_INVALID, "map session: process before start");
  if (s->ended) FAIL(AICP_ERR_INVALID, "map session ended at reading " + std::to_string(s->ended_at));
  const Stream& P = s->P;
  const bool raw = P.pf_read != nullptr;
  if (acc && !raw) FAIL(AICP_ERR_INVALID, "map session: a reading from the accumulator needs pf_read");
  if (reading && !valid_cloud(*reading)) FAIL(AICP_ERR_INVALID, "map session: invalid reading");
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Live live;
  live.ev_done = s->ev_end;
  if (s->mon.on) {
    live.mon = &s->mon.prm;
    live.mon_cnt = &s->mon.cnt;
    live.mon_off = kSessMon;
  }
  s->mon.none();
  // a risk session: the crop is taken at the pose cast to float (app.cpp:47, 63), the sensor origin
  // is the pose's translation
  float posef[16];
  Live::Risk lr{};
  if (risk) {
    for (int k = 0; k < 16; ++k) posef[k] = (float)pose_d[k];
    pose = posef;
    *prec = aicp_pipeline_record{};
    lr = Live::Risk{&s->rprm, s->model, s->threshold, pose_d, kSessGate, kSessFifty, kSessGate + sizeof(GateRec), prec};
    live.risk = &lr;
  }
  aicp_cloud c{};
  if (reading) {
    c = *reading;
    if (risk)
      for (int k = 0; k < 3; ++k) c.origin[k] = pose_d[12 + k];
  } else {  // the accumulator's cloud where it lies; its sensor origin is the pose's translation
    const int rc = accum_resident(ctx, acc, &live.dpts, &live.dn);  // (waits for the pushes)
    if (rc) return rc;
    if (live.dn > (size_t)INT32_MAX) FAIL(AICP_ERR_INVALID, "map session: invalid reading");
    c.pts = reinterpret_cast<const float*>(live.dpts);  // (not read on the host)
    c.n = live.dn;
    c.stride = 16;
    for (int k = 0; k < 3; ++k) c.origin[k] = risk ? pose_d[12 + k] : (double)pose[12 + k];
  }
  const std::string id = std::to_string(s->n_processed);
  aicp_localization_result* o = static_cast<aicp_localization_result*>(out);
  std::memset(o, 0, sizeof(*o));
  ident4(out_T);
  if (kept_out) *kept_out = 0;
  HIPC(hipStreamSynchronize(st));  // (the mirror is free)
  char* h = s->pin.as<char>();
  char* d = s->win.as<char>();
  const StreamState* hS = reinterpret_cast<const StreamState*>(h);
  if (P.bm && aicp_hip_built_map_window((uint64_t)hS->count, P.bm, 1) == 0) {
    (void)map_session_end(ctx, s, AICP_ERR_HIP);
    FAIL(AICP_ERR_HIP, "map session: the device's count left its range");
  }
  const WinBlock K{reinterpret_cast<StreamState*>(d), reinterpret_cast<StreamRec*>(d + kRecOff),
                   reinterpret_cast<double*>(d + kSessOrg), h, reinterpret_cast<double*>(h + kSessOrg), &s->read};
  StreamTiming tm;
  WinEnd end;
  size_t done = 0, wr = 0;
  int rc = AICP_OK;
  if (c.n == 0) {  // (an accumulator with no point) as a reading the pre-filter empties
    o->status = o->icp.status = end.status = AICP_ERR_INVALID;
    o->map_points = s->map->n;
    o->icp.overlap_percent = -1.f;
    end.empty_read = true;
  } else {
    HIPC(hipEventRecord(s->ev_begin, st));
    s->kept.clear();
    rc = stream_window(ctx, P, &s->cfg, s->map, K, &c, pose, 1, out_T, o, s->kept, s->stats, tm, &live, 0, &done, &wr,
                       &end);
    if (kept_out && (!raw || !s->kept.empty())) *kept_out = raw ? s->kept[0] : (uint32_t)c.n;
  }
  if (rc) return map_session_end(ctx, s, rc);  // (a map that cannot grow among them: nothing has changed)
  if (live.registered) {
    s->last_device_ms = ev_ms(s->ev_begin, s->ev_end);
    s->last_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  if (end.status) {
    const std::string why = ctx->err;
    (void)map_session_end(ctx, s, end.status);
    ctx->err = "map session: reading " + id +
               (end.empty_crop   ? std::string(": empty map crop")
                : end.empty_read ? std::string(": keeps no point after the pre-filter")
                                 : ": status " + std::to_string(end.status) + ": " + why);
    return end.status;
  }
  // the monitor's result came back with the record; its own errors leave valid = 0 and the call as it is
  s->mon.take(ctx, &ctx->mon_scratch, live.mon_ran, h + kSessMon, live.mon_err);
  ++s->n_processed;
  return AICP_OK;
}

int aicp_hip_map_session_process(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_cloud* reading,
                                 const float pose[16], float out_T[16], void* out, uint32_t* kept) {
  if (!reading || !pose) return AICP_ERR_INVALID;
  return map_session_process(ctx, s, reading, nullptr, pose, nullptr, out_T, out, nullptr, kept);
}

int aicp_hip_map_session_process_accum(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_accum* acc,
                                       const float pose[16], float out_T[16], void* out, uint32_t* kept) {
  if (!acc || !pose) return AICP_ERR_INVALID;
  return map_session_process(ctx, s, nullptr, acc, pose, nullptr, out_T, out, nullptr, kept);
}

int aicp_hip_mapsession_process_risk(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_cloud* reading,
                                     const double pose[16], float out_T[16], void* out, aicp_pipeline_record* rec,
                                     uint32_t* kept) {
  if (!reading || !pose || !rec) return AICP_ERR_INVALID;
  return map_session_process(ctx, s, reading, nullptr, nullptr, pose, out_T, out, rec, kept);
}

int aicp_hip_mapsession_process_accum_risk(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_accum* acc,
                                           const double pose[16], float out_T[16], void* out,
                                           aicp_pipeline_record* rec, uint32_t* kept) {
  if (!acc || !pose || !rec) return AICP_ERR_INVALID;
  return map_session_process(ctx, s, nullptr, acc, nullptr, pose, out_T, out, rec, kept);
}

int aicp_hip_map_session_state(aicp_hip_ctx* ctx, aicp_hip_map_session* s, uint64_t* n_processed, int32_t* count,
                               float initial_T[16], int32_t* ended) {
  if (!ctx || !s) return AICP_ERR_INVALID;
  if (!s->started) FAIL(AICP_ERR_INVALID, "map session: state before start");
  // (every call ends with the stream idle and the mirror read back: nothing to wait for)
  const StreamState* hS = s->pin.as<StreamState>();
  if (n_processed) *n_processed = s->n_processed;
  if (count) *count = hS->count;
  if (initial_T) std::memcpy(initial_T, hS->initT, 64);
  if (ended) *ended = s->ended ? 1 : 0;
  return AICP_OK;
}

int aicp_hip_map_session_last_timing(const aicp_hip_map_session* s, double* wall_ms, double* device_ms) {
  if (!s) return AICP_ERR_INVALID;
  if (wall_ms) *wall_ms = s->last_wall_ms;
  if (device_ms) *device_ms = s->last_device_ms;
  return AICP_OK;
}

}  // extern "C"
