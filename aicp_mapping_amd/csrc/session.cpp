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
// The reference lives in one of two buffers; a promotion writes the other one and the host flips
// them when the record reports it, so a reading that is dropped or fails leaves the reference as it
// was and a larger reference never needs a copy. Its identity in the reference cache is a number
// taken from the cache for every new reference (RefCache::owner): no host copy, no compare.
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
constexpr size_t kOffState = 0, kOffRec = 128, kOffHdr = 192, kOffOrigin = 256, kWinBytes = 320;
constexpr size_t kReadBack = kOffOrigin;  // state + record + header
static_assert(sizeof(StreamState) <= kOffRec && kOffRec + sizeof(StreamRec) <= kOffHdr &&
                  kOffHdr + sizeof(SessionHeader) <= kOffOrigin && kOffRec % alignof(StreamRec) == 0,
              "win's layout");
constexpr int kFlags = AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;
}  // namespace

struct aicp_hip_session {
  aicp_icp_config cfg{};
  aicp_sequence_params prm{};
  aicp_prefilter_params pf{};
  bool has_pf = false;
  StreamRules rules{};
  DevBuf win;     // StreamState | StreamRec | SessionHeader | the reading's prior origin (3 doubles)
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

int start_rows(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r) {
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
  s->cur = 1 - s->cur;
  s->ref_n = kept;
  s->ref_id = -1;
  for (int k = 0; k < 3; ++k) s->ref_origin[k] = r.origin[k];
  s->gen = ctx->refc.next_owner++;
  s->n_processed = 0;
  s->started = true;
  s->ended = false;
  // count = 0, initialT_ = I, no record, the header of reference -1
  char* h = s->pin.as<char>();
  std::memset(h, 0, kWinBytes);
  ident4(host_state(s)->initT);
  SessionHeader* hh = reinterpret_cast<SessionHeader*>(h + kOffHdr);
  hh->count = kept;
  hh->id = -1;
  for (int k = 0; k < 3; ++k) hh->origin[k] = r.origin[k];
  HIPC(hipMemcpyAsync(s->win.p, h, kWinBytes, hipMemcpyHostToDevice, st));
  HIPC(hipStreamSynchronize(st));
  return AICP_OK;
}

int process_rows(aicp_hip_ctx* ctx, aicp_hip_session* s, const Rows& r, float* out_T, aicp_sequence_result* out,
                 uint32_t* kept_out) {
  const auto t0 = std::chrono::steady_clock::now();
  hipStream_t st = ctx->stream;
  const bool debug = s->prm.flags & AICP_SEQ_DEBUG, doOvl = s->prm.flags & AICP_RUN_OVERLAP;
  const int32_t id = (int32_t)s->n_processed;
  *out = aicp_sequence_result{};
  out->reference = s->ref_id;
  ident4(out_T);
  if (kept_out) *kept_out = 0;
  // a reading with no point, or one the pre-filter empties, fails its registration (libpointmatcher
  // throws on an empty cloud), which ends the worker (app.cpp:210)
  auto empty_reading = [&]() {
    out->status = out->icp.status = AICP_ERR_INVALID;
    const int rc = end_session(ctx, s, AICP_ERR_INVALID);
    ctx->err = "session: reading " + std::to_string(id) + " keeps no point after the pre-filter";
    return rc;
  };
  if (r.n == 0) return empty_reading();
  HIPC(hipSetDevice(ctx->device));
  HIPC(hipStreamSynchronize(st));  // (the mirror is free)
  char* h = s->pin.as<char>();
  char* d = s->win.as<char>();
  StreamState* dS = reinterpret_cast<StreamState*>(d + kOffState);
  StreamRec* dRec = reinterpret_cast<StreamRec*>(d + kOffRec);
  SessionHeader* dHdr = reinterpret_cast<SessionHeader*>(d + kOffHdr);
  double* dOrg = reinterpret_cast<double*>(d + kOffOrigin);
  // the overlap's sensor origin of the moved reading, from the mirror of the device's initialT_
  // (k_stream_ingest computes the same for the commit, on the device)
  double o[3] = {r.origin[0], r.origin[1], r.origin[2]};
  if (debug) corrected_origin(host_state(s)->initT, r.origin, o);
  std::memcpy(h + kOffOrigin, r.origin, 24);
  HIPC(hipEventRecord(s->ev_begin, st));
  HIPC(hipMemcpyAsync(dOrg, h + kOffOrigin, 24, hipMemcpyHostToDevice, st));
  HIPC(ensure(s->read, r.n * 16));
  uint32_t kept = 0;
  int rc = stream_ingest_rows(ctx, s->has_pf ? &s->pf : nullptr, r.hpts, r.n, r.stride, r.dpts,
                              debug ? dS->initT : nullptr, debug ? dOrg : nullptr, s->read.as<float4>(), &kept);
  if (rc) return end_session(ctx, s, rc);
  if (kept_out) *kept_out = kept;
  if (!kept) return empty_reading();
  // the one-pair batch: both clouds are on the device already
  aicp_pair p{};
  p.ref = p.read = s->read.as<float>();  // (not read: references on the device, readings skipped)
  p.n_ref = s->ref_n;
  p.n_read = kept;
  p.ref_stride = p.read_stride = 16;
  for (int k = 0; k < 3; ++k) {
    p.ref_origin[k] = s->ref_origin[k];
    p.read_origin[k] = o[k];
  }
  const int flags = AICP_RUN_ICP | (s->prm.flags & (AICP_RUN_OVERLAP | AICP_RUN_TIME_NN));
  const double res = doOvl ? s->prm.resolution : 0.0;
  if (!ctx->oneshot) ctx->oneshot = new aicp_hip_batch();
  aicp_hip_batch* B = ctx->oneshot;
  rc = upload_pairs(ctx, &p, 1, B, true, false, true, true);
  if (rc) return end_session(ctx, s, rc);
  HIPC(hipMemcpyAsync(B->ref_raw.as<float4>() + B->rdesc[0].ref_off, s->ref[s->cur].p, s->ref_n * 16,
                      hipMemcpyDeviceToDevice, st));
  HIPC(hipMemcpyAsync(B->read_raw.as<float4>() + B->desc[0].read_off, s->read.p, (size_t)kept * 16,
                      hipMemcpyDeviceToDevice, st));
  refcache_begin_resident(ctx, &s->cfg, s->gen, s->ref_n, s->ref_origin, res, flags);
  aicp_icp_stats stats{};
  stats.status = -1;
  rc = run_batch(ctx, B, &s->cfg, res, flags, out_T, &stats, nullptr);
  ctx->refc.use = false;
  if (rc) ctx->refc.invalidate();  // (an error may leave the reference side half written)
  if (rc && stats.status == -1) {  // the batch did not run to its end (not the reading's status)
    out->status = out->icp.status = rc;
    return end_session(ctx, s, rc);
  }
  out->icp = stats;
  out->status = out->icp.status = rc;
  // App's bookkeeping and the promotion, on the device; one read-back
  DevBuf& spare = s->ref[1 - s->cur];
  HIPC(ensure(spare, (size_t)kept * 16));
  launch_stream_commit(st, 1, ctx->state.as<PairState>(), ctx->outT.as<float>(), dOrg, s->rules, dS, dRec);
  launch_session_promote(st, (int)kept, dRec, ctx->outT.as<float>(), s->read.as<float4>(), id, spare.as<float4>(),
                         dHdr);
  HIPC(hipGetLastError());
  HIPC(hipEventRecord(s->ev_end, st));
  HIPC(hipMemcpyAsync(h, d, kReadBack, hipMemcpyDeviceToHost, st));
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
  if (rec.append) {  // the corrected reading is the next reference (app.cpp:375-391)
    if (hdr.count != kept || hdr.id != id) {
      (void)end_session(ctx, s, AICP_ERR_HIP);
      FAIL(AICP_ERR_HIP, "session: the promoted reference's header");
    }
    out->is_reference = 1;
    s->cur = 1 - s->cur;
    s->ref_n = kept;
    s->ref_id = id;
    for (int k = 0; k < 3; ++k) s->ref_origin[k] = hdr.origin[k];
    s->gen = ctx->refc.next_owner++;  // (the cached trees and voxel map are the old reference's: stale)
  }
  ++s->n_processed;
  return AICP_OK;
}

int process_args(aicp_hip_ctx* ctx, aicp_hip_session* s, const float* out_T, const aicp_sequence_result* out) {
  if (!ctx || !s || !out_T || !out) return AICP_ERR_INVALID;
  if (!s->started) FAIL(AICP_ERR_INVALID, "session: process before start");
  if (s->ended) FAIL(AICP_ERR_INVALID, "session ended at reading " + std::to_string(s->ended_at));
  return AICP_OK;
}

}  // namespace

extern "C" {

int aicp_hip_session_create(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                            const aicp_prefilter_params* pf, aicp_hip_session** out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (!cfg || !prm) return AICP_ERR_INVALID;
  if (prm->reference_update_frequency < 1) FAIL(AICP_ERR_INVALID, "reference_update_frequency must be >= 1");
  if (prm->flags & ~kFlags) FAIL(AICP_ERR_INVALID, "session: flags");
  if (!(prm->max_correction_magnitude == prm->max_correction_magnitude))
    FAIL(AICP_ERR_INVALID, "session: max_correction_magnitude");
  const bool doOvl = prm->flags & AICP_RUN_OVERLAP;
  if (doOvl && !(prm->resolution > 0)) FAIL(AICP_ERR_INVALID, "resolution");
  int rc = check_cfg(ctx, cfg, AICP_RUN_ICP | (doOvl ? AICP_RUN_OVERLAP : 0));
  if (!rc && pf) rc = stream_prefilter_check(ctx, pf);
  if (rc) return rc;
  HIPC(hipSetDevice(ctx->device));
  aicp_hip_session* s = new aicp_hip_session();
  s->cfg = *cfg;
  s->prm = *prm;
  if (pf) s->pf = *pf;
  s->has_pf = pf != nullptr;
  s->rules.built = 1;  // the drop test on every reading, the count restarts at a new reference
  s->rules.freq = prm->reference_update_frequency;
  s->rules.overlap = doOvl ? 1 : 0;
  s->rules.max_corr = prm->max_correction_magnitude;
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
  if (s->ev_begin) (void)hipEventDestroy(s->ev_begin);
  if (s->ev_end) (void)hipEventDestroy(s->ev_end);
  delete s;
}

int aicp_hip_session_start(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* first) {
  if (!ctx || !s || !first) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, first, nullptr, nullptr, &r);
  return rc ? rc : start_rows(ctx, s, r);
}

int aicp_hip_session_start_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3]) {
  if (!ctx || !s || !acc || !origin) return AICP_ERR_INVALID;
  Rows r;
  const int rc = rows_of(ctx, nullptr, acc, origin, &r);
  return rc ? rc : start_rows(ctx, s, r);
}

int aicp_hip_session_process(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* reading, float out_T[16],
                             aicp_sequence_result* out, uint32_t* kept) {
  if (!reading) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, reading, nullptr, nullptr, &r);
  return rc ? rc : process_rows(ctx, s, r, out_T, out, kept);
}

int aicp_hip_session_process_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3],
                                   float out_T[16], aicp_sequence_result* out, uint32_t* kept) {
  if (!acc || !origin) return AICP_ERR_INVALID;
  int rc = process_args(ctx, s, out_T, out);
  if (rc) return rc;
  Rows r;
  rc = rows_of(ctx, nullptr, acc, origin, &r);
  return rc ? rc : process_rows(ctx, s, r, out_T, out, kept);
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
