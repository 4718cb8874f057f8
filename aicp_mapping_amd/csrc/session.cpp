// session.cpp — the live App session of include/aicp_hip.h: App::processCloud (app.cpp:282-414) in
// frame-to-reference mode, one reading per call, with App's state kept on the device between calls.
//
// Per reading: [host] the prior origin up -> [device] k_stream_ingest from the caller's uploaded
// rows or from the sweep accumulator's cloud where it lies (debug mode: moved by the device's
// initialT_, the origin with it), the pre-filter (pf_core), the kept points into the session's
// reading buffer -> [host] sizes the one-pair batch -> [device] reference and reading copied into
// the batch device-to-device, overlap -> ratio beside the trees and normals (or the reference
// cache's, when the session's reference is still the cached one), ICP loop, finalize (run_batch) ->
// [device] k_stream_commit (the built-map rules with one reading: app.cpp:366-391, 414), then
// k_session_promote: the reading moved by its correction into the spare reference buffer when the
// commit's record says so -> [host] one read-back of state, record and header.
//
// A risk session (aicp_hip_session_create_risk: failure_prediction_mode, runAicpPipeline
// app.cpp:236-245 and the gated branch app.cpp:401-411) splits the batch in two and puts the gate
// between: overlap-only batch -> alignment features with the FOV filters reading the reference and
// the reading where they lie -> k_svm_predict -> k_session_gate_promote (gated: the unmoved reading
// copied into the spare reference buffer, record, identity correction, count and header written on
// the device) -> [host] one read-back of state, record, header and the gate's record. A gated
// reading ends there; otherwise the ICP-only batch at the device's ratio, k_stream_commit and
// k_session_promote follow as above. The reference's pose stays on the host in double.
//
// With the quality monitor on (aicp_hip_session_set_monitor), a registered reading's metrics are
// enqueued behind its batch and ahead of k_stream_commit (monitor_resident, monitor.cpp: the
// reference where it lies, the reading as registered, the correction in device memory; the
// monitor's tree over the reference is the session's and is kept while the reference stays), and
// their 56 bytes come back in the same read-back.
//
// The reference lives in one of two buffers; a promotion writes the other one and the host flips
// them when the record reports it, so a reading that is dropped or fails leaves the reference as it
// was and a larger reference never needs a copy. Its identity in the reference cache is a number
// taken from the cache for every new reference (RefCache::owner): no host copy, no compare.
//
// aligned_map_ (aicp_hip_session_keep_aligned_map; app.cpp:310, 458-468): the session owns an
// aicp_hip_map made from the first cloud's reference bytes, and k_session_promote_map /
// k_session_gate_promote_map store every new reference a second time behind it. The host makes room
// (map_reserve) after the reading's pre-filter and before its batch, when the mirrored count says
// the reading is promoted if accepted (a risk session: every reading), and adds the kept points to
// the map's size after the call's one read-back, when the record says `append`. The go-back
// (app_ros.cpp:329-357) takes the map out of the session (aicp_hip_session_take_aligned_map) and
// starts a prior-map session at App's graph count and initialT_ (session_go_back below,
// aicp_hip_mapsession_start_go_back in map_stream.cpp).
//
// aicp_hip_session_start_on_map is load_map_from_file without localize_against_prior_map
// (app.cpp:43-59, 392-399): the reference is a map's crop around the first reading's prior pose, the
// graph is empty, and the first reading runs without the drop test and is promoted whatever the
// frequency (StreamRules by value for that call: max_corr = +inf, freq = 1).
//
// The two offline App-order entry points (aicp_hip_sequence_run_raw in debug mode,
// aicp_hip_sequence_run_risk; aicp_hip.cpp) are session_replay below: the same step, reading after
// reading, on a session private to the call.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

namespace {
// the session's small device block and its pinned mirror
constexpr size_t kOffState = 0, kOffRec = 128, kOffHdr = 192, kOffGate = 256, kOffMon = 320, kOffOrigin = 384,
                 kWinBytes = 448;
constexpr size_t kReadBack = kOffGate;                            // state + record + header
constexpr size_t kReadBackGate = kOffGate + sizeof(GateRec);      // and the gate's record
constexpr size_t kReadBackMon = kOffMon + sizeof(aicp_monitor_result);  // a monitored reading: and its 56 bytes
static_assert(sizeof(StreamState) <= kOffRec && kOffRec + sizeof(StreamRec) <= kOffHdr &&
                  kOffHdr + sizeof(SessionHeader) <= kOffGate && kOffRec % alignof(StreamRec) == 0 &&
                  kReadBackGate <= kOffMon && kOffGate % alignof(GateRec) == 0 && kReadBackMon <= kOffOrigin &&
                  kOffMon % 8 == 0 && kOffOrigin + 24 <= kWinBytes,
              "win's layout");
constexpr int kFlags = AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;
}  // namespace

struct aicp_hip_session {
  aicp_icp_config cfg{};
  aicp_sequence_params prm{};
  aicp_prefilter_params pf{};
  bool has_pf = false;
  StreamRules rules{};
  DevBuf win;     // StreamState | StreamRec | SessionHeader | GateRec | the monitor's result | the prior origin (3 doubles)
  PinBuf pin;     // its mirror
  DevBuf ref[2];  // the reference (float4, w = 1) and the buffer the next promotion writes
  int cur = 0;
  DevBuf read;    // the last reading as it was registered (kept points; debug mode: moved)
  size_t ref_n = 0;
  int32_t ref_id = -1;
  double ref_origin[3] = {0, 0, 0};
  uint64_t gen = 0;  // the reference's identity in the context's reference cache
  uint64_t n_processed = 0;
  bool started = false, ended = false;
  uint64_t ended_at = 0;
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  double last_wall_ms = 0, last_device_ms = 0;
  // failure_prediction_mode (aicp_hip_session_create_risk): the features' parameters, the caller's
  // model, the gate's threshold, and the reference's pose (host, double, column-major)
  bool risk = false;
  aicp_risk_params rprm{};
  const aicp_hip_svm* model = nullptr;
  double threshold = 0;
  double ref_pose[16] = {};
  // the per-reading quality monitor (aicp_hip_session_set_monitor): its parameters, the monitor's
  // trees over the current reference (built on the first monitored reading against it, kept until
  // the reference changes), the counters, and the last call's result
  MonState mon;
  MonRefTree mon_tree;
  // aligned_map_ (aicp_hip_session_keep_aligned_map): the session's own map, and where this
  // reading's points go if it is promoted (null: no room was made, the mirrored count rules it out)
  aicp_hip_ctx* owner = nullptr;
  bool keep_map = false;
  aicp_hip_map* amap = nullptr;
  float4* tail = nullptr;
  // App's graph (aligned_clouds_graph_->getNbClouds()): the readings accepted since the start, gated
  // ones included, beside the first cloud, which a start on a map does not have
  uint64_t n_accepted = 0;
  bool on_map = false, first_on_map = false;  // started on a map; and its first reading is still to come
};

namespace {

StreamState* host_state(aicp_hip_session* s) { return reinterpret_cast<StreamState*>(s->pin.as<char>() + kOffState); }

// rows of a reading: the caller's (c) or the accumulator's cloud where it lies
struct Rows {
  const float* hpts = nullptr;
  size_t n = 0, stride = 0;
  const float4* dpts = nullptr;
  double origin[3] = {0, 0, 0};
};

int rows_of(aicp_hip_ctx* ctx, const aicp_cloud* c, aicp_hip_accum* acc, const double* origin, Rows* r) {
  if (c) {
    if (!valid_cloud(*c)) FAIL(AICP_ERR_INVALID, "session: invalid cloud");
    r->hpts = c->pts;
    r->n = c->n;
    r->stride = c->stride;
    for (int k = 0; k < 3; ++k) r->origin[k] = c->origin[k];
    return AICP_OK;
  }
  const int rc = accum_resident(ctx, acc, &r->dpts, &r->n);  // (waits for the pushes)
  if (rc) return rc;
  if (r->n > (size_t)INT32_MAX) FAIL(AICP_ERR_INVALID, "session: invalid cloud");
  for (int k = 0; k < 3; ++k) r->origin[k] = origin[k];
  return AICP_OK;
}

int end_session(aicp_hip_ctx* ctx, aicp_hip_session* s, int rc) {
  s->ended = true;
  s->ended_at = s->n_processed;
  ++s->n_processed;
  (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

// a map of its own from n points that lie on the device, behind everything enqueued on ctx->stream:
// exactly the cloud, as aicp_hip_map_create sizes it (n = 0: an empty map, grown by its first append)
int map_from_device(aicp_hip_ctx* ctx, const float4* src, size_t n, aicp_hip_map** out) {
  aicp_hip_map* m = new aicp_hip_map();
  if (n) {
    const size_t nb = std::max<size_t>(256, n * 16);
    hipError_t e = hipMalloc(&m->pts.p, nb);
    if (e == hipSuccess) {
      m->pts.cap = nb;
      e = hipMemcpyAsync(m->pts.p, src, n * 16, hipMemcpyDeviceToDevice, ctx->stream);
    }
    if (e != hipSuccess) {
      release(m->pts);
      delete m;
      FAIL(AICP_ERR_HIP, std::string("session: aligned map allocation: ") + hipGetErrorString(e));
    }
  }
  m->n = n;
  *out = m;
  return AICP_OK;
}

// A start that can no longer fail on its inputs: the spare buffer's `kept` points are reference -1
// with the sensor origin `origin`, the state is App's at its start (count = 0, initialT_ = I, no
// record), and map (nullable: keeping is off) replaces the session's aligned map. on_map: the
// reference is a map's crop and the graph holds no first cloud (aicp_hip_session_start_on_map).
int begin_state(aicp_hip_ctx* ctx, aicp_hip_session* s, uint32_t kept, const double origin[3], aicp_hip_map* map,
                bool on_map) {
  hipStream_t st = ctx->stream;
  aicp_hip_map_free(ctx, s->amap);  // (waits for the stream)
  s->amap = map;
  s->tail = nullptr;
  s->cur = 1 - s->cur;
  s->ref_n = kept;
  s->ref_id = -1;
  for (int k = 0; k < 3; ++k) s->ref_origin[k] = origin[k];
  s->gen = ctx->refc.next_owner++;
  s->mon_tree.invalidate();
  s->mon.none();
  s->n_processed = s->n_accepted = 0;
  s->on_map = s->first_on_map = on_map;
  s->started = true;
  s->ended = false;
  // count = 0, initialT_ = I, no record, the header of reference -1
  char* h = s->pin.as<char>();
  std::memset(h, 0, kWinBytes);
  ident4(host_state(s)->initT);
  SessionHeader* hh = reinterpret_cast<SessionHeader*>(h + kOffHdr);
  hh->count = kept;
  hh->id = -1;
  for (int k = 0; k < 3; ++k) hh->origin[k] = origin[k];
  HIPC(hipMemcpyAsync(s->win.p, h, kWinBytes, hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));
  return AICP_OK;
}

// first_pose: a risk session's (nullable otherwise): the reference's pose through updateCloud
// (app.cpp:293-299), set once nothing can fail any more
int start_rows(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r, const double* first_pose) {
  if (r.n == 0) FAIL(AICP_ERR_INVALID, "session: the first cloud is empty");
  HIPC(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  HIPC(hipStreamSynchronize(st));
  // into the spare buffer: a first cloud the pre-filter empties leaves the session as it was
  DevBuf& dst = s->ref[1 - s->cur];
  HIPC(ensure(dst, r.n * 16));
  uint32_t kept = 0;
  int rc = stream_ingest_rows(ctx, s->has_pf ? &s->pf : nullptr, r.hpts, r.n, r.stride, r.dpts, nullptr, nullptr,
                              dst.as<float4>(), &kept);
  if (rc) return rc;
  if (!kept) {
    HIPC(hipStreamSynchronize(st));
    FAIL(AICP_ERR_INVALID, "session: the first cloud keeps no point after the pre-filter");
  }
  // aligned_map_ starts as the first cloud's reference (app.cpp:310): its bytes, device to device
  aicp_hip_map* map = nullptr;
  if (s->keep_map) {
    rc = map_from_device(ctx, dst.as<float4>(), kept, &map);
    if (rc) return rc;
  }
  rc = begin_state(ctx, s, kept, r.origin, map, false);
  if (rc) return rc;
  if (first_pose) pose_fix_pitch_roll(first_pose, first_pose, s->ref_pose);
  return AICP_OK;
}

// Room behind the aligned map for this reading's kept points, between its pre-filter and its batch
// (nothing that reads the map is in flight; growing synchronises and may move the map, so the tail
// is taken afterwards), when the reading is promoted if it is accepted: the mirrored count reaches
// `freq` (k_stream_commit's rule), or `every` (a risk session: the gate can promote any reading). A
// map that cannot grow is the call's error: the map and the session stay as they were.
int reserve_tail(aicp_hip_ctx* ctx, aicp_hip_session* s, uint32_t kept, int32_t freq, bool every) {
  s->tail = nullptr;
  if (!s->amap || !(every || host_state(s)->count + 1 == freq)) return AICP_OK;
  const int rc = map_reserve(ctx, s->amap, kept);
  if (rc) return rc;
  s->tail = s->amap->pts.as<float4>() + s->amap->n;
  return AICP_OK;
}

// The one-pair batch of the session's reference and reading (kept points), both copied into the
// batch device to device; the reference's voxel map and trees go through the reference cache under
// the session's owner number. stats->status stays as the caller set it when the batch did not run
// to its end; otherwise the return value is the reading's status.
int pair_batch(aicp_hip_ctx* ctx, aicp_hip_session* s, uint32_t kept, const double* read_origin,
               const aicp_icp_config* cfg, double res, int flags, float* out_T, aicp_icp_stats* stats) {
  hipStream_t st = ctx->stream;
  aicp_pair p{};
  p.ref = p.read = s->read.as<float>();  // (not read: references on the device, readings skipped)
  p.n_ref = s->ref_n;
  p.n_read = kept;
  p.ref_stride = p.read_stride = 16;
  for (int k = 0; k < 3; ++k) {
    p.ref_origin[k] = s->ref_origin[k];
    p.read_origin[k] = read_origin[k];
  }
  if (!ctx->oneshot) ctx->oneshot = new aicp_hip_batch();
  aicp_hip_batch* B = ctx->oneshot;
  int rc = upload_pairs(ctx, &p, 1, B, true, false, true, true);
  if (rc) return rc;
  HIPC(hipMemcpyAsync(B->ref_raw.as<float4>() + B->rdesc[0].ref_off, s->ref[s->cur].p, s->ref_n * 16,
                      hipMemcpyDeviceToDevice, st));
  HIPC(hipMemcpyAsync(B->read_raw.as<float4>() + B->desc[0].read_off, s->read.p, (size_t)kept * 16,
                      hipMemcpyDeviceToDevice, st));
  refcache_begin_resident(ctx, cfg, s->gen, s->ref_n, s->ref_origin, res, flags);
  rc = run_batch(ctx, B, cfg, res, flags, out_T, stats, nullptr);
  ctx->refc.use = false;
  if (rc) ctx->refc.invalidate();  // (an error may leave the reference side half written)
  return rc;
}

// a reading that fails its registration ends the worker (app.cpp:210); why: the text behind "reading <id>"
int reading_failed(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_sequence_result* out, int rc, const std::string& why) {
  out->status = out->icp.status = rc;
  const std::string id = std::to_string(s->n_processed);
  (void)end_session(ctx, s, rc);
  ctx->err = "session: reading " + id + why;
  return rc;
}

// The head of a reading's call, for both kinds of session: the outputs reset, the prior origin up,
// the rows ingested (debug mode: moved by the device's initialT_) and pre-filtered into s->read.
// odom: a risk session's prior pose (its translation is r.origin), null for a plain one. prior: the
// reading's prior pose as setAndFilterReading leaves it (app.cpp:77-100: debug mode, initialT_ *
// prior pose, from the mirror of the device's initialT_; k_stream_ingest moves the origin the same
// way for the records, on the device); a plain session has only its translation, the overlap's
// sensor origin. A non-zero return is the call's; otherwise *kept > 0 points lie in s->read.
int ingest_reading(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r, const double* odom, float* out_T,
                   aicp_sequence_result* out, uint32_t* kept_out, uint32_t* kept, double prior[16]) {
  hipStream_t st = ctx->stream;
  const bool debug = s->prm.flags & AICP_SEQ_DEBUG;
  *out = aicp_sequence_result{};
  out->reference = s->ref_id;
  ident4(out_T);
  if (kept_out) *kept_out = 0;
  s->mon.none();
  // a reading with no point, or one the pre-filter empties, fails its registration (libpointmatcher
  // throws on an empty cloud)
  if (r.n == 0) return reading_failed(ctx, s, out, AICP_ERR_INVALID, " keeps no point after the pre-filter");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(st));  // (the mirror is free)
  char* h = s->pin.as<char>();
  char* d = s->win.as<char>();
  StreamState* dS = reinterpret_cast<StreamState*>(d + kOffState);
  double* dOrg = reinterpret_cast<double*>(d + kOffOrigin);
  if (odom) {
    if (debug)
      pose_moved(host_state(s)->initT, odom, prior);
    else
      std::memcpy(prior, odom, 16 * sizeof(double));
  } else {
    std::memcpy(prior + 12, r.origin, 24);
    if (debug) corrected_origin(host_state(s)->initT, r.origin, prior + 12);
  }
  std::memcpy(h + kOffOrigin, r.origin, 24);
  HIPC(hipEventRecord(s->ev_begin, st));
  HIPC(hipMemcpyAsync(dOrg, h + kOffOrigin, 24, hipMemcpyHostToDevice, st));
  HIPC(ensure(s->read, r.n * 16));
  const int rc = stream_ingest_rows(ctx, s->has_pf ? &s->pf : nullptr, r.hpts, r.n, r.stride, r.dpts,
                                    debug ? dS->initT : nullptr, debug ? dOrg : nullptr, s->read.as<float4>(), kept);
  if (rc) return end_session(ctx, s, rc);
  if (kept_out) *kept_out = *kept;
  if (!*kept) return reading_failed(ctx, s, out, AICP_ERR_INVALID, " keeps no point after the pre-filter");
  return AICP_OK;
}

int commit_reading(aicp_hip_ctx* ctx, aicp_hip_session* s, const StreamRules& rules, uint32_t kept, int32_t id, int rc,
                   std::chrono::steady_clock::time_point t0, aicp_sequence_result* out, bool* promoted);

int process_rows(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r, float* out_T, aicp_sequence_result* out,
                 uint32_t* kept_out) {
  const auto t0 = std::chrono::steady_clock::now();
  const bool doOvl = s->prm.flags & AICP_RUN_OVERLAP;
  const int32_t id = (int32_t)s->n_processed;
  uint32_t kept = 0;
  double prior[16];
  int rc = ingest_reading(ctx, s, r, nullptr, out_T, out, kept_out, &kept, prior);
  if (rc) return rc;
  // the first reading after a start on a map (app.cpp:366-369, 383-399): the graph is empty, so no
  // drop test, and the accepted reading is the next reference whatever the frequency
  StreamRules rules = s->rules;
  if (s->first_on_map) {
    rules.max_corr = INFINITY;
    rules.freq = 1;
  }
  rc = reserve_tail(ctx, s, kept, rules.freq, false);
  if (rc) return rc;
  // the one-pair batch: both clouds are on the device already
  const int flags = AICP_RUN_ICP | (s->prm.flags & (AICP_RUN_OVERLAP | AICP_RUN_TIME_NN));
  const double res = doOvl ? s->prm.resolution : 0.0;
  aicp_icp_stats stats{};
  stats.status = -1;
  rc = pair_batch(ctx, s, kept, prior + 12, &s->cfg, res, flags, out_T, &stats);
  if (rc && stats.status == -1) {  // the batch did not run to its end (not the reading's status)
    out->status = out->icp.status = rc;
    return end_session(ctx, s, rc);
  }
  out->icp = stats;
  out->status = out->icp.status = rc;
  return commit_reading(ctx, s, rules, kept, id, rc, t0, out, nullptr);
}

// Behind the batch that registered the reading (rc: its status, out->icp filled): App's bookkeeping
// and the promotion, on the device; one read-back. *promoted (nullable): the reading is the new
// reference (the buffers are flipped, a new owner number is taken).
int commit_reading(aicp_hip_ctx* ctx, aicp_hip_session* s, const StreamRules& rules, uint32_t kept, int32_t id, int rc,
                   std::chrono::steady_clock::time_point t0, aicp_sequence_result* out, bool* promoted) {
  hipStream_t st = ctx->stream;
  char* h = s->pin.as<char>();
  char* d = s->win.as<char>();
  StreamState* dS = reinterpret_cast<StreamState*>(d + kOffState);
  StreamRec* dRec = reinterpret_cast<StreamRec*>(d + kOffRec);
  SessionHeader* dHdr = reinterpret_cast<SessionHeader*>(d + kOffHdr);
  double* dOrg = reinterpret_cast<double*>(d + kOffOrigin);
  if (promoted) *promoted = false;
  DevBuf& spare = s->ref[1 - s->cur];
  HIPC(ensure(spare, (size_t)kept * 16));
  // The monitor of a registered reading, ahead of the commit and the promotion: it reads the
  // reference the reading was registered against where it lies (a promotion writes the spare
  // buffer), the reading as registered and the correction the batch left in device memory, with
  // the chain at the reading's own tuned ratio. An error of its own only costs the result.
  bool mon_ran = false;
  std::string mon_err;
  if (s->mon.on && rc == AICP_OK) {
    aicp_icp_config mc = s->cfg;
    mc.trimmed_ratio = out->icp.trimmed_ratio;
    const std::string why = ctx->err;
    mon_ran = monitor_resident(ctx, &s->mon.prm, &mc, s->ref[s->cur].as<float4>(), s->ref_n, s->read.as<float4>(), kept,
                               ctx->outT.as<float>(), &s->mon_tree, &s->mon.cnt, d + kOffMon) == AICP_OK;
    if (!mon_ran) mon_err = ctx->err;
    ctx->err = why;
  }
  launch_stream_commit(st, 1, ctx->state.as<PairState>(), ctx->outT.as<float>(), dOrg, rules, dS, dRec);
  if (s->tail)  // (aligned_map_: the new reference also goes behind the map, app.cpp:458-468)
    launch_session_promote_map(st, (int)kept, dRec, ctx->outT.as<float>(), s->read.as<float4>(), id,
                               spare.as<float4>(), s->tail, dHdr);
  else
    launch_session_promote(st, (int)kept, dRec, ctx->outT.as<float>(), s->read.as<float4>(), id, spare.as<float4>(),
                           dHdr);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(s->ev_end, st));
  HIPC(hipMemcpyAsync(h, d, mon_ran ? kReadBackMon : kReadBack, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  const StreamRec& rec = *reinterpret_cast<const StreamRec*>(h + kOffRec);
  const SessionHeader& hdr = *reinterpret_cast<const SessionHeader*>(h + kOffHdr);
  s->last_device_ms = ev_ms(s->ev_begin, s->ev_end);
  s->last_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (rec.status != rc) {
    (void)end_session(ctx, s, AICP_ERR_HIP);
    FAIL(AICP_ERR_HIP, "session: the device's record disagrees with the registration's status");
  }
  if (rc) {  // the worker ends here (app.cpp:210)
    const std::string why = ctx->err;
    (void)end_session(ctx, s, rc);
    ctx->err = "session: reading " + std::to_string(id) + ": status " + std::to_string(rc) + ": " + why;
    return rc;
  }
  out->accepted = rec.accepted;
  for (int k = 0; k < 3; ++k) out->corrected_origin[k] = rec.corrected_origin[k];
  if (rec.accepted) ++s->n_accepted;
  if (rec.append) {  // the corrected reading is the next reference (app.cpp:375-391)
    if (hdr.count != kept || hdr.id != id) {
      (void)end_session(ctx, s, AICP_ERR_HIP);
      FAIL(AICP_ERR_HIP, "session: the promoted reference's header");
    }
    if (s->amap && !s->tail) {
      (void)end_session(ctx, s, AICP_ERR_HIP);
      FAIL(AICP_ERR_HIP, "session: the device's count left its mirror");
    }
    if (s->tail) s->amap->n += kept;
    out->is_reference = 1;
    s->cur = 1 - s->cur;
    s->ref_n = kept;
    s->ref_id = id;
    for (int k = 0; k < 3; ++k) s->ref_origin[k] = hdr.origin[k];
    s->gen = ctx->refc.next_owner++;  // (the cached trees and voxel map are the old reference's: stale)
    if (promoted) *promoted = true;
  }
  // (before the reference's trees are dropped: the check clears them on an error anyway)
  s->mon.take(ctx, &s->mon_tree, mon_ran, h + kOffMon, mon_err);
  if (rec.append) s->mon_tree.invalidate();  // (the monitor's trees are the old reference's)
  ++s->n_processed;
  s->first_on_map = false;
  return AICP_OK;
}

// One reading of a risk session, and the loop body of aicp_hip_sequence_run_risk: runAicpPipeline
// with failure_prediction_mode (app.cpp:236-245) and both branches of processCloud's `if`
// (app.cpp:362-411) on the session's resident buffers. odom: the reading's prior pose (its
// translation is r.origin).
int process_rows_risk(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r, const double* odom, float* out_T,
                      aicp_sequence_result* out, aicp_pipeline_record* prec, uint32_t* kept_out) {
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t st = ctx->stream;
  const int32_t id = (int32_t)s->n_processed;
  *prec = aicp_pipeline_record{};
  auto failed = [&](int rc, const std::string& stage) {
    return reading_failed(ctx, s, out, rc, ": status " + std::to_string(rc) + ": " + stage + ctx->err);
  };
  uint32_t kept = 0;
  double prior[16];
  int rc = ingest_reading(ctx, s, r, odom, out_T, out, kept_out, &kept, prior);
  if (rc) return rc;
  char* h = s->pin.as<char>();
  char* d = s->win.as<char>();
  StreamState* dS = reinterpret_cast<StreamState*>(d + kOffState);
  StreamRec* dRec = reinterpret_cast<StreamRec*>(d + kOffRec);
  SessionHeader* dHdr = reinterpret_cast<SessionHeader*>(d + kOffHdr);
  double* dOrg = reinterpret_cast<double*>(d + kOffOrigin);
  GateRec* dGate = reinterpret_cast<GateRec*>(d + kOffGate);
  prec->n_read = kept;
  out->icp.overlap_percent = -1.f;
  rc = reserve_tail(ctx, s, kept, s->rules.freq, true);
  if (rc) return rc;
  // 1. computeOverlap: an overlap-only batch, the poses' translations are the sensor origins (app.cpp:229)
  aicp_icp_stats ost{};
  ost.status = -1;
  rc = pair_batch(ctx, s, kept, prior + 12, &s->cfg, s->prm.resolution, AICP_RUN_OVERLAP, nullptr, &ost);
  if (rc) return failed(rc, "overlap: ");
  // 2. and 3. the features from both clouds where they lie, the classifier, the gate and the ratio;
  // 4. the gated branch, taken on the device; one read-back
  float fov = 0.f;
  aicp_cloud ca{}, cb{};
  ca.n = s->ref_n, cb.n = kept;
  ca.stride = cb.stride = 16;
  rc = gate_resident(ctx, &s->rprm, s->model, s->threshold, ca, cb, s->ref[s->cur].as<float4>(), s->read.as<float4>(),
                     s->ref_pose, prior, dGate, &fov);
  if (rc) return failed(rc, "risk gate: ");
  DevBuf& spare = s->ref[1 - s->cur];
  HIPC(ensure(spare, (size_t)kept * 16));
  if (s->tail)  // (aligned_map_: a gated reading is a new reference too, app.cpp:401-411, 458-468)
    launch_session_gate_promote_map(st, (int)kept, dGate, dOrg, s->read.as<float4>(), id, spare.as<float4>(), s->tail,
                                    ctx->outT.as<float>(), dS, dRec, dHdr);
  else
    launch_session_gate_promote(st, (int)kept, dGate, dOrg, s->read.as<float4>(), id, spare.as<float4>(),
                                ctx->outT.as<float>(), dS, dRec, dHdr);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(s->ev_end, st));
  HIPC(hipMemcpyAsync(h, d, kReadBackGate, hipMemcpyDeviceToHost, st));
  HIPC(hipStreamSynchronize(st));
  const GateRec g = *reinterpret_cast<const GateRec*>(h + kOffGate);
  prec->fov_overlap = fov;
  prec->octree_overlap = g.overlap;
  prec->alignability = g.alignability;
  prec->raw = g.raw;
  prec->risk = g.risk;
  prec->trimmed_ratio = g.ratio;
  prec->registered = g.gate ? 0 : 1;
  aicp_icp_stats ist{};
  if (g.gate) {
    // app.cpp:401-411: the unmoved reading joined the graph with its prior pose and is the reference
    // at once; the count restarted; the correction stays the identity
    const StreamRec& rec = *reinterpret_cast<const StreamRec*>(h + kOffRec);
    const SessionHeader& hdr = *reinterpret_cast<const SessionHeader*>(h + kOffHdr);
    s->last_device_ms = ev_ms(s->ev_begin, s->ev_end);
    s->last_wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rec.status != 0 || !rec.accepted || !rec.append || hdr.count != kept || hdr.id != id) {
      (void)end_session(ctx, s, AICP_ERR_HIP);
      FAIL(AICP_ERR_HIP, "session: the gated reference's record and header");
    }
    ist.overlap_percent = g.overlap;
    ist.trimmed_ratio = g.ratio;
    for (int k = 0; k < 3; ++k) ist.overlap_keys[k] = ost.overlap_keys[k];
    out->icp = ist;
    out->accepted = out->is_reference = 1;
    for (int k = 0; k < 3; ++k) out->corrected_origin[k] = rec.corrected_origin[k];
    if (s->tail) s->amap->n += kept;
    ++s->n_accepted;
    s->cur = 1 - s->cur;
    s->ref_n = kept;
    s->ref_id = id;
    pose_fix_pitch_roll(prior, odom, s->ref_pose);
    for (int k = 0; k < 3; ++k) s->ref_origin[k] = s->ref_pose[12 + k];
    s->gen = ctx->refc.next_owner++;  // (the cached voxel map is the old reference's: stale)
    s->mon_tree.invalidate();
    ++s->n_processed;
    return AICP_OK;
  }
  // 5. computeRegistration at the device's ratio (app.cpp:243-245): an ICP-only batch, then the
  // plain session's commit and promotion
  aicp_icp_config c2 = s->cfg;
  c2.trimmed_ratio = g.ratio;
  ist.status = -1;
  rc = pair_batch(ctx, s, kept, prior + 12, &c2, 0.0, AICP_RUN_ICP | (s->prm.flags & AICP_RUN_TIME_NN), out_T, &ist);
  if (rc && ist.status == -1) return failed(rc, "");
  ist.overlap_percent = g.overlap;
  for (int k = 0; k < 3; ++k) ist.overlap_keys[k] = ost.overlap_keys[k];
  out->icp = ist;
  out->status = out->icp.status = rc;
  bool promoted = false;
  rc = commit_reading(ctx, s, s->rules, kept, id, rc, t0, out, &promoted);
  if (rc) return rc;
  if (promoted) {  // App's corrected pose, in double on the host (aligned_cloud.cpp:31-74)
    double corrected[16];
    pose_moved(out_T, prior, corrected);
    pose_fix_pitch_roll(corrected, odom, s->ref_pose);
    for (int k = 0; k < 3; ++k) s->ref_origin[k] = s->ref_pose[12 + k];
  }
  return AICP_OK;
}

// risk: the call is a risk session's (_pose / _risk); a handle of the other kind refuses it
int kind_check(aicp_hip_ctx* ctx, const aicp_hip_session* s, bool risk) {
  if (s->risk == risk) return AICP_OK;
  FAIL(AICP_ERR_INVALID, risk ? "session: not made by aicp_hip_session_create_risk"
                              : "session: a risk session takes the _pose and _risk calls");
}

int process_args(aicp_hip_ctx* ctx, aicp_hip_session* s, const float* out_T, const aicp_sequence_result* out,
                 bool risk) {
  if (!ctx || !s || !out_T || !out) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, risk)) return AICP_ERR_INVALID;
  if (!s->started) FAIL(AICP_ERR_INVALID, "session: process before start");
  if (s->ended) FAIL(AICP_ERR_INVALID, "session ended at reading " + std::to_string(s->ended_at));
  return AICP_OK;
}

// aicp_hip_session_create's checks
int create_check(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                 const aicp_prefilter_params* pf) {
  if (prm->reference_update_frequency < 1) FAIL(AICP_ERR_INVALID, "reference_update_frequency must be >= 1");
  if (prm->flags & ~kFlags) FAIL(AICP_ERR_INVALID, "session: flags");
  if (!(prm->max_correction_magnitude == prm->max_correction_magnitude))
    FAIL(AICP_ERR_INVALID, "session: max_correction_magnitude");
  const bool doOvl = prm->flags & AICP_RUN_OVERLAP;
  if (doOvl && !(prm->resolution > 0)) FAIL(AICP_ERR_INVALID, "resolution");
  const int rc = check_cfg(ctx, cfg, AICP_RUN_ICP | (doOvl ? AICP_RUN_OVERLAP : 0));
  return !rc && pf ? stream_prefilter_check(ctx, pf) : rc;
}

// a session of checked parameters; risk_prm: failure_prediction_mode (null: a plain session)
int create_session(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                   const aicp_prefilter_params* pf, const aicp_risk_params* risk_prm, const aicp_hip_svm* model,
                   double threshold, aicp_hip_session** out) {
  HIPC(hipSetDevice(ctx->device));
  aicp_hip_session* s = new aicp_hip_session();
  s->owner = ctx;
  s->cfg = *cfg;
  s->prm = *prm;
  if (pf) s->pf = *pf;
  s->has_pf = pf != nullptr;
  s->rules.built = 1;  // the drop test on every reading, the count restarts at a new reference
  s->rules.freq = prm->reference_update_frequency;
  s->rules.overlap = prm->flags & AICP_RUN_OVERLAP ? 1 : 0;
  s->rules.max_corr = prm->max_correction_magnitude;
  if (risk_prm) {
    s->risk = true;
    s->rprm = *risk_prm;
    s->model = model;
    s->threshold = threshold;
    s->prm.flags |= AICP_RUN_OVERLAP;  // (the overlap always runs: the classifier needs it)
    s->rules.overlap = 0;  // (the overlap is a batch of its own, its status checked before the gate)
  }
  hipError_t e = ensure(s->win, kWinBytes);
  if (e == hipSuccess) e = ensure(s->pin, kWinBytes);
  if (e == hipSuccess) e = hipEventCreate(&s->ev_begin);
  if (e == hipSuccess) e = hipEventCreate(&s->ev_end);
  if (e != hipSuccess) {
    aicp_hip_session_free(ctx, s);
    HIPC(e);
  }
  *out = s;
  return AICP_OK;
}

}  // namespace

// The two offline entry points' loop (aicp_hip.cpp; declared in runtime.hpp).
int aicp::rt::session_replay(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                             const aicp_prefilter_params* pf, const ReplayRisk* risk, const aicp_cloud* first,
                             const aicp_cloud* readings, size_t n, float* out_T, aicp_sequence_result* out,
                             size_t* n_done) {
  aicp_sequence_params p = *prm;
  p.flags &= kFlags;  // (the entry points ignore the other bits; a NaN bound rejects nothing)
  aicp_hip_session* s = nullptr;
  int rc = create_session(ctx, cfg, &p, pf, risk ? risk->prm : nullptr, risk ? risk->model : nullptr,
                          risk ? risk->threshold : 0.0, &s);
  if (rc) return rc;
  // a risk stream's sensor origins are its poses' translations
  auto rows = [&](const aicp_cloud& c, const double* pose) {
    Rows r;
    r.hpts = c.pts, r.n = c.n, r.stride = c.stride;
    for (int k = 0; k < 3; ++k) r.origin[k] = pose ? pose[12 + k] : c.origin[k];
    return r;
  };
  rc = start_rows(ctx, s, rows(*first, risk ? risk->first_pose : nullptr), risk ? risk->first_pose : nullptr);
  for (size_t i = 0; i < n && !rc; ++i) {
    const double* pose = risk ? risk->poses + 16 * i : nullptr;
    rc = risk ? process_rows_risk(ctx, s, rows(readings[i], pose), pose, out_T + 16 * i, &out[i], &risk->rec[i], nullptr)
              : process_rows(ctx, s, rows(readings[i], nullptr), out_T + 16 * i, &out[i], nullptr);
    // (a reading that failed before it was looked at, its pre-filter for one, is not counted)
    if (!rc || out[i].status) *n_done = i + 1;
  }
  if (rc && ctx->err.rfind("session: ", 0) == 0) ctx->err.erase(0, 9);  // the entry points' wording
  aicp_hip_session_free(ctx, s);
  return rc;
}

// What a go-back takes from a live session (aicp_hip_mapsession_start_go_back, map_stream.cpp;
// declared in runtime.hpp): App's graph count, from the host's counter of accepted readings, and
// where initialT_ lies on the device. Nothing else of the session is read.
int aicp::rt::session_go_back(aicp_hip_ctx* ctx, const aicp_hip_session* s, uint64_t* n_clouds,
                              const float** d_initT) {
  if (s->owner != ctx) FAIL(AICP_ERR_INVALID, "go-back: the session lives on another context");
  if (!s->started) FAIL(AICP_ERR_INVALID, "go-back: the session has not started");
  if (s->ended) FAIL(AICP_ERR_INVALID, "go-back: the session ended at reading " + std::to_string(s->ended_at));
  *n_clouds = (s->on_map ? 0 : 1) + s->n_accepted;
  *d_initT = reinterpret_cast<const StreamState*>(s->win.as<char>() + kOffState)->initT;
  return AICP_OK;
}

extern "C" {

int aicp_hip_session_keep_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, int on) {
  if (!ctx || !s) return AICP_ERR_INVALID;
  s->keep_map = on != 0;
  if (!on && s->amap) {  // (the map goes at once: nothing would keep it up to date)
    HIPC(hipSetDevice(ctx->device));
    aicp_hip_map_free(ctx, s->amap);
    s->amap = nullptr;
    s->tail = nullptr;
  }
  return AICP_OK;
}

int aicp_hip_session_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_map** out) {
  if (!ctx || !s || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!s->keep_map) FAIL(AICP_ERR_INVALID, "session: the aligned map is not kept");
  if (!s->started || !s->amap) FAIL(AICP_ERR_INVALID, "session: no aligned map before the next start");
  *out = s->amap;
  return AICP_OK;
}

int aicp_hip_session_take_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_map** out) {
  const int rc = aicp_hip_session_aligned_map(ctx, s, out);
  if (rc) return rc;
  s->amap = nullptr;  // (the caller's now; the session goes on without one until its next start)
  s->tail = nullptr;
  return AICP_OK;
}

int aicp_hip_session_start_on_map(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_hip_map* map,
                                  const float first_pose[16], float crop_min, float crop_max) {
  if (!ctx || !s || !map || !first_pose) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, false)) return AICP_ERR_INVALID;
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  // the reference: the map around the first reading's prior pose (setReference, app.cpp:43-58), into
  // the spare buffer: an empty crop leaves the session as it was
  uint32_t kept = 0;
  int rc = map_crop_resident(ctx, map, crop_min, crop_max, first_pose, &s->ref[1 - s->cur], &kept);
  if (rc) return rc;
  if (!kept) FAIL(AICP_ERR_INVALID, "session: empty map crop");
  // aligned_map_ starts empty: there is no first cloud (app.cpp:310 is not reached)
  aicp_hip_map* amap = nullptr;
  if (s->keep_map) {
    rc = map_from_device(ctx, nullptr, 0, &amap);
    if (rc) return rc;
  }
  const double origin[3] = {first_pose[12], first_pose[13], first_pose[14]};
  return begin_state(ctx, s, kept, origin, amap, true);
}

int aicp_hip_session_create(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                            const aicp_prefilter_params* pf, aicp_hip_session** out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!cfg || !prm) return AICP_ERR_INVALID;
  const int rc = create_check(ctx, cfg, prm, pf);
  return rc ? rc : create_session(ctx, cfg, prm, pf, nullptr, nullptr, 0.0, out);
}

int aicp_hip_session_create_risk(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                                 const aicp_prefilter_params* pf, const aicp_risk_params* risk_prm,
                                 const aicp_hip_svm* model, double threshold, aicp_hip_session** out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!cfg || !prm || !risk_prm || !model) return AICP_ERR_INVALID;
  if (!(threshold == threshold)) FAIL(AICP_ERR_INVALID, "session: threshold");
  int rc = risk_params_check(ctx, risk_prm);
  if (rc) return rc;
  aicp_sequence_params p = *prm;
  p.flags |= AICP_RUN_OVERLAP;  // (checked as the session runs: with the overlap)
  rc = create_check(ctx, cfg, &p, pf);
  return rc ? rc : create_session(ctx, cfg, &p, pf, risk_prm, model, threshold, out);
}

void aicp_hip_session_free(aicp_hip_ctx* ctx, aicp_hip_session* s) {
  if (!s) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  release(s->win);
  release(s->pin);
  release(s->ref[0]);
  release(s->ref[1]);
  release(s->read);
  aicp_hip_map_free(nullptr, s->amap);  // (the stream was waited for above)
  s->mon_tree.release_all();
  if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
  if (s->ev_end) (void)hipEventDestroy(s->ev_end);
  delete s;
}

int aicp_hip_session_set_monitor(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_monitor_params* prm) {
  if (!ctx || !s) return AICP_ERR_INVALID;
  const int rc = s->mon.set(ctx, prm);
  if (!rc && prm) s->mon_tree.invalidate();  // (built again on the first monitored reading)
  return rc;
}

int aicp_hip_session_last_monitor(const aicp_hip_session* s, aicp_monitor_result* out, int32_t* valid) {
  return s ? s->mon.get_last(out, valid) : AICP_ERR_INVALID;
}

int aicp_hip_session_monitor_counters(const aicp_hip_session* s, uint64_t out[4]) {
  return s ? s->mon.counters(out) : AICP_ERR_INVALID;
}

int aicp_hip_session_start(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* first) {
  if (!ctx || !s || !first) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, false)) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, first, nullptr, nullptr, &r);
  return rc ? rc : start_rows(ctx, s, r, nullptr);
}

int aicp_hip_session_start_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3]) {
  if (!ctx || !s || !acc || !origin) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, false)) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, nullptr, acc, origin, &r);
  return rc ? rc : start_rows(ctx, s, r, nullptr);
}

int aicp_hip_session_start_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* first,
                                const double first_pose[16]) {
  if (!ctx || !s || !first || !first_pose) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, true)) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, first, nullptr, nullptr, &r);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k) r.origin[k] = first_pose[12 + k];  // (the sensor origin is the translation)
  return start_rows(ctx, s, r, first_pose);
}

int aicp_hip_session_start_accum_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc,
                                      const double first_pose[16]) {
  if (!ctx || !s || !acc || !first_pose) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, true)) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, nullptr, acc, first_pose + 12, &r);
  return rc ? rc : start_rows(ctx, s, r, first_pose);
}

int aicp_hip_session_process(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* reading, float out_T[16],
                             aicp_sequence_result* out, uint32_t* kept) {
  if (!reading) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out, false);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, reading, nullptr, nullptr, &r);
  return rc ? rc : process_rows(ctx, s, r, out_T, out, kept);
}

int aicp_hip_session_process_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3],
                                   float out_T[16], aicp_sequence_result* out, uint32_t* kept) {
  if (!acc || !origin) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out, false);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, nullptr, acc, origin, &r);
  return rc ? rc : process_rows(ctx, s, r, out_T, out, kept);
}

int aicp_hip_session_process_risk(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* reading,
                                  const double pose[16], float out_T[16], aicp_sequence_result* out,
                                  aicp_pipeline_record* rec, uint32_t* kept) {
  if (!reading || !pose || !rec) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out, true);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, reading, nullptr, nullptr, &r);
  if (rc) return rc;
  for (int k = 0; k < 3; ++k) r.origin[k] = pose[12 + k];
  return process_rows_risk(ctx, s, r, pose, out_T, out, rec, kept);
}

int aicp_hip_session_process_accum_risk(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc,
                                        const double pose[16], float out_T[16], aicp_sequence_result* out,
                                        aicp_pipeline_record* rec, uint32_t* kept) {
  if (!acc || !pose || !rec) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out, true);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, nullptr, acc, pose + 12, &r);
  return rc ? rc : process_rows_risk(ctx, s, r, pose, out_T, out, rec, kept);
}

int aicp_hip_session_reference_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, double pose[16]) {
  if (!ctx || !s || !pose) return AICP_ERR_INVALID;
  if (kind_check(ctx, s, true)) return AICP_ERR_INVALID;
  if (!s->started) FAIL(AICP_ERR_INVALID, "session: reference pose before start");
  std::memcpy(pose, s->ref_pose, sizeof(s->ref_pose));
  return AICP_OK;
}

int aicp_hip_session_state(aicp_hip_ctx* ctx, aicp_hip_session* s, uint64_t* n_processed, int32_t* reference,
                           size_t* reference_points, float initial_T[16], int32_t* ended) {
  if (!ctx || !s) return AICP_ERR_INVALID;
  if (!s->started) FAIL(AICP_ERR_INVALID, "session: state before start");
  // (every call ends with the stream idle and the mirror read back: nothing to wait for)
  if (n_processed) *n_processed = s->n_processed;
  if (reference) *reference = s->ref_id;
  if (reference_points) *reference_points = s->ref_n;
  if (initial_T) std::memcpy(initial_T, host_state(s)->initT, 64);
  if (ended) *ended = s->ended ? 1 : 0;
  return AICP_OK;
}

int aicp_hip_session_reference(aicp_hip_ctx* ctx, aicp_hip_session* s, float* out, size_t cap, size_t* out_n,
                               double origin[3]) {
  if (!ctx || !s || !out_n || (cap && !out)) return AICP_ERR_INVALID;
  *out_n = 0;
  if (!s->started) FAIL(AICP_ERR_INVALID, "session: reference before start");
  if (s->ref_n > cap) FAIL(AICP_ERR_INVALID, "session: output capacity too small");
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(ctx->stream));
  HIPC(ensure(ctx->pin_io, s->ref_n * 16));
  float* h = ctx->pin_io.as<float>();
  HIPC(hipMemcpy(h, s->ref[s->cur].p, s->ref_n * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < s->ref_n; ++i)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = h[4 * i + k];
  *out_n = s->ref_n;
  if (origin)
    for (int k = 0; k < 3; ++k) origin[k] = s->ref_origin[k];
  return AICP_OK;
}

int aicp_hip_session_last_timing(const aicp_hip_session* s, double* wall_ms, double* device_ms) {
  if (!s) return AICP_ERR_INVALID;
  if (wall_ms) *wall_ms = s->last_wall_ms;
  if (device_ms) *device_ms = s->last_device_ms;
  return AICP_OK;
}

}  // extern "C"
