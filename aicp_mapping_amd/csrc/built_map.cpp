// built_map.cpp — App's localization stream on the map it has built itself
// (aicp_hip_built_map_sequence_run; localize_against_built_map, processCloud app.cpp:282-414 with
// setReference app.cpp:60-69). Rules: include/aicp_hip.h.
//
// The map changes only when an accepted reading becomes a reference, and that depends on the
// count of readings accepted since the last reference alone. Readings between two map changes see
// the same map, so they are independent: they run as one batch (a window), each against its own
// device crop with its own overlap and ratio (the batch of aicp_hip_map_align_batch). The window
// ends where the next reference would fall if every reading were accepted
// (aicp_hip_built_map_window); a dropped reading only postpones it, so the map is still unchanged
// at the end of the window and the next, shorter window goes on from the count reached. Nothing is
// run twice.
//
// Per window: [host] crop frames -> [device] crop counts -> [host] sizes the batch (one sync) ->
// [device] crop scatter, (debug mode: the reading moved by initialT_), overlap -> ratio beside the
// trees and normals, ICP loop, finalize (run_batch) -> [device] k_bm_commit: drop test, count,
// corrected origin, initialT_, the append plan -> [host] reads the records once -> [device]
// k_loc_merge from the batch's copy of the reading by the device's correction. No reading crosses
// the bus a second time.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
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

struct BmBufs {
  DevBuf state;   // BmState
  DevBuf origin;  // prior-pose translations of the window's readings, 3 doubles each
  DevBuf rec;     // BmRec per reading of the window
  PinBuf pin;     // staging: BmState, then the origins, then the records
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  aicp_built_map_timing last{};
};

void bm_bufs_free(BmBufs* L) {
  if (!L) return;
  release(L->state);
  release(L->origin);
  release(L->rec);
  release(L->pin);
  if (L->ev_begin) (void)hipEventDestroy(L->ev_begin);
  if (L->ev_end) (void)hipEventDestroy(L->ev_end);
  delete L;
}

}  // namespace rt
}  // namespace aicp

namespace {

constexpr int kBmFlags = AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;

bool valid_params(const aicp_built_map_params* p) {
  return p && p->reference_update_frequency >= 1 && !(p->flags & ~kBmFlags) &&
         p->max_correction_magnitude == p->max_correction_magnitude && p->crop_min == p->crop_min &&
         p->crop_max == p->crop_max && (!(p->flags & AICP_RUN_OVERLAP) || p->resolution > 0);
}

}  // namespace

extern "C" {

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

size_t aicp_hip_built_map_window(uint64_t acc, const aicp_built_map_params* prm, size_t remaining) {
  if (!valid_params(prm) || remaining == 0 || acc >= (uint64_t)prm->reference_update_frequency) return 0;
  if (prm->flags & AICP_SEQ_DEBUG) return 1;
  // reading k of the window (k >= 1), if all before it are accepted too, is the (acc + k)-th
  // accepted since the last reference: the map changes after it when acc + k == frequency
  const uint64_t to_ref = (uint64_t)prm->reference_update_frequency - acc;
  return (size_t)std::min<uint64_t>(std::min<size_t>(remaining, (size_t)kMaxPairs), to_ref);
}

int aicp_hip_built_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_built_map_params* prm,
                                    aicp_hip_map* map, const aicp_cloud* readings, const float* poses, size_t n,
                                    float* out_T, aicp_built_map_result* out, size_t* n_done) {
  if (!ctx || !n_done) return AICP_ERR_INVALID;
  *n_done = 0;
  if (!cfg || !prm || !map || (n && (!readings || !poses || !out_T || !out))) return AICP_ERR_INVALID;
  if (!valid_params(prm)) FAIL(AICP_ERR_INVALID, "built-map parameters");
  for (size_t i = 0; i < n; ++i) {
    const aicp_cloud& c = readings[i];
    if (!c.pts || c.n == 0 || c.stride < 12 || (c.stride % 4) || c.n > (uint64_t)INT32_MAX)
      FAIL(AICP_ERR_INVALID, "invalid reading " + std::to_string(i));
  }
  const bool debug = prm->flags & AICP_SEQ_DEBUG;
  const int run_flags = AICP_RUN_ICP | (prm->flags & (AICP_RUN_OVERLAP | AICP_RUN_TIME_NN));
  int rc = check_cfg(ctx, cfg, run_flags);
  if (rc) return rc;
  const auto t0 = std::chrono::steady_clock::now();
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!ctx->bm) ctx->bm = new BmBufs();
  BmBufs* L = ctx->bm;
  L->last = aicp_built_map_timing{};
  if (!L->ev_begin) HIPC(hipEventCreate(&L->ev_begin));
  if (!L->ev_end) HIPC(hipEventCreate(&L->ev_end));
  BmRules rules{};
  rules.freq = prm->reference_update_frequency;
  rules.max_corr = prm->max_correction_magnitude;
  rules.overlap = (run_flags & AICP_RUN_OVERLAP) ? 1 : 0;

  // the stream's state: acc = 0, initialT_ = I
  const size_t wmax = std::min<size_t>(std::max<size_t>(n, 1), (size_t)kMaxPairs);
  const size_t o_org = (sizeof(BmState) + 63) & ~size_t(63), o_rec = o_org + ((wmax * 24 + 63) & ~size_t(63));
  HIPC(ensure(L->state, sizeof(BmState)));
  HIPC(ensure(L->origin, wmax * 24));
  HIPC(ensure(L->rec, wmax * sizeof(BmRec)));
  HIPC(ensure(L->pin, o_rec + wmax * sizeof(BmRec)));
  char* lp = L->pin.as<char>();
  BmState* dS = L->state.as<BmState>();
  BmState* hS = reinterpret_cast<BmState*>(lp);  // the host's mirror, read back with every window's records
  std::memset(hS, 0, sizeof(BmState));
  ident4(hS->initT);
  hS->append = -1;
  HIPC(hipMemcpyAsync(dS, hS, sizeof(BmState), hipMemcpyHostToDevice, s));
  HIPC(hipEventRecord(L->ev_begin, s));
  HIPC(hipStreamSynchronize(s));  // (the mirror is written again below)
  std::vector<aicp_icp_stats> stats;
  int windows = 0, appends = 0, status = AICP_OK;
  size_t p = 0;
  bool empty_crop = false;
  while (p < n && !status) {
    const size_t w = aicp_hip_built_map_window((uint64_t)hS->acc, prm, n - p);
    if (w == 0) FAIL(AICP_ERR_HIP, "built-map stream: the device's count left its range");
    const size_t map_n = map->n;
    // debug mode (one reading per window): the overlap's sensor origin of the moved reading, the
    // translation of initialT_ * prior pose, from the mirror of the device's initialT_ (k_loc_move
    // computes the same for the commit, on the device)
    double moved[3];
    if (debug) corrected_origin(hS->initT, readings[p].origin, moved);
    size_t wr = 0;
    const uint32_t* htot = nullptr;
    rc = map_crop_pairs(ctx, map, prm->crop_min, prm->crop_max, readings + p, poses + 16 * p, w,
                        debug ? moved : nullptr, &wr, &htot);
    if (rc) return rc;
    // an empty crop ends the stream at its reading; the readings before it still run
    if (wr) {
      aicp_hip_batch* B = ctx->mapbatch;
      double* horg = reinterpret_cast<double*>(lp + o_org);
      for (size_t i = 0; i < wr; ++i)
        for (int k = 0; k < 3; ++k) horg[3 * i + k] = readings[p + i].origin[k];
      HIPC(hipMemcpyAsync(L->origin.p, horg, wr * 24, hipMemcpyHostToDevice, s));
      if (debug) {  // moved by the device's initialT_, its prior pose too
        launch_loc_move(s, (int)B->desc[0].n_read, dS->initT, L->origin.as<double>(),
                        B->read_raw.as<float4>() + B->desc[0].read_off);
        HIPC(hipGetLastError());
      }
      stats.assign(wr, aicp_icp_stats{});
      for (auto& st : stats) st.status = -1;
      rc = run_batch(ctx, B, cfg, prm->resolution, run_flags, out_T + 16 * p, stats.data(), nullptr);
      if (rc && stats[0].status == -1) return rc;  // the batch did not run to its end (not a reading's status)
      ++windows;
      // App's bookkeeping for the window, on the device; one read-back of its records and state
      launch_bm_commit(s, (int)wr, ctx->state.as<PairState>(), ctx->outT.as<float>(), L->origin.as<double>(), rules,
                       dS, L->rec.as<BmRec>());
      HIPC(hipGetLastError());
      BmRec* hrec = reinterpret_cast<BmRec*>(lp + o_rec);
      HIPC(hipMemcpyAsync(hrec, L->rec.p, wr * sizeof(BmRec), hipMemcpyDeviceToHost, s));
      HIPC(hipMemcpyAsync(hS, dS, sizeof(BmState), hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      for (size_t i = 0; i < wr; ++i) {
        const BmRec& r = hrec[i];
        aicp_built_map_result& o = out[p + i];
        std::memset(&o, 0, sizeof(o));
        o.status = r.status;
        o.accepted = r.accepted;
        o.is_reference = r.is_reference;
        o.map_points = map_n;
        o.crop_points = htot[i];
        for (int k = 0; k < 3; ++k) o.corrected_origin[k] = r.corrected_origin[k];
        o.icp = stats[i];
        *n_done = p + i + 1;
        if (r.status) {
          status = r.status;
          break;
        }
      }
      // the append plan: the window's reference goes to the map's tail (by the window rule it is the
      // window's last reading, so every crop of the window saw the map without it)
      const int a = hS->append;
      if (a >= 0) {
        if ((size_t)a >= wr || !hrec[a].is_reference || hrec[a].status)
          FAIL(AICP_ERR_HIP, "built-map stream: append plan outside the window");
        const PairDesc& d = B->desc[a];
        rc = map_reserve(ctx, map, d.n_read);
        if (rc) return rc;
        launch_loc_merge(s, (int)d.n_read, ctx->outT.as<float>() + 16 * (size_t)a,
                         B->read_raw.as<float4>() + d.read_off, map->pts.as<float4>() + map->n);
        HIPC(hipGetLastError());
        map->n += d.n_read;
        ++appends;
      }
    }
    if (!status && wr < w) {  // the reading with the empty crop (libpointmatcher throws on an empty cloud)
      aicp_built_map_result& o = out[p + wr];
      std::memset(&o, 0, sizeof(o));
      o.status = o.icp.status = AICP_ERR_INVALID;
      o.map_points = map_n;
      o.icp.overlap_percent = -1.f;
      ident4(out_T + 16 * (p + wr));
      *n_done = p + wr + 1;
      status = AICP_ERR_INVALID;
      empty_crop = true;
    }
    p += wr;
  }
  HIPC(hipEventRecord(L->ev_end, s));
  HIPC(hipStreamSynchronize(s));
  L->last.windows = windows;
  L->last.appends = appends;
  L->last.device_ms = ev_ms(L->ev_begin, L->ev_end);
  L->last.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (status)
    ctx->err = "reading " + std::to_string(*n_done - 1) +
               (empty_crop ? std::string(": empty map crop") : ": status " + std::to_string(status));
  return status;
}

int aicp_hip_last_built_map_timing(const aicp_hip_ctx* ctx, aicp_built_map_timing* out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = ctx->bm ? ctx->bm->last : aicp_built_map_timing{};
  return AICP_OK;
}

}  // extern "C"
