// localization.cpp — App's localization stream on the device-resident prior map
// (aicp_hip_map_sequence_run; localize_against_prior_map, processCloud app.cpp:282-414 with
// setReference app.cpp:37-75 and the map maintenance app.cpp:469-493). Rules: include/aicp_hip.h.
//
// The map changes only when an accepted reading is merged or the map is re-filtered, and both
// depend on the running count of accepted readings alone. Readings between two map changes see
// the same map, so they are independent: they run as one batch (a window), cropped on the device
// straight into the batch's reference array like aicp_hip_map_register_batch. The window ends
// where the next map change would fall if every reading were accepted
// (aicp_hip_localization_window); a dropped reading only postpones the change, so the map is
// still unchanged at the end of the window and the next, shorter window goes on from the count
// reached. Nothing is run twice.
//
// Per window: [host] crop frames -> [device] crop counts -> [host] sizes the batch (one sync, as
// the batch call) -> [device] crop scatter, (debug mode: the reading moved by initialT_), trees,
// normals, ICP loop, finalize (run_batch) -> [device] k_loc_commit: drop test, count, corrected
// origin, initialT_, merge / re-filter flags -> [host] reads the records once -> [device]
// k_loc_merge from the batch's copy of the reading by the device's correction, the map's
// pre-filter. No reading crosses the bus a second time.
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

struct LocBufs {
  DevBuf state;   // LocState
  DevBuf origin;  // prior-pose translations of the window's readings, 3 doubles each
  DevBuf rec;     // LocRec per reading of the window
  PinBuf pin;     // staging: LocState, then the origins, then the records
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;
  aicp_localization_timing last{};
};

void loc_bufs_free(LocBufs* L) {
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

constexpr int kLocFlags = AICP_LOC_MERGE | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN;

bool valid_params(const aicp_localization_params* p) {
  return p && p->reference_update_frequency >= 1 && p->map_refilter_every >= 0 && !(p->flags & ~kLocFlags) &&
         p->max_correction_magnitude == p->max_correction_magnitude;
}

}  // namespace

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

int aicp_hip_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                              const aicp_prefilter_params* pf, aicp_hip_map* map, const aicp_cloud* readings,
                              const float* poses, size_t n, float* out_T, aicp_localization_result* out,
                              size_t* n_done) {
  if (!ctx || !n_done) return AICP_ERR_INVALID;
  *n_done = 0;
  if (!cfg || !prm || !map || (n && (!readings || !poses || !out_T || !out))) return AICP_ERR_INVALID;
  if (!valid_params(prm)) FAIL(AICP_ERR_INVALID, "localization parameters");
  for (size_t i = 0; i < n; ++i) {
    const aicp_cloud& c = readings[i];
    if (!c.pts || c.n == 0 || c.stride < 12 || (c.stride % 4) || c.n > (uint64_t)INT32_MAX)
      FAIL(AICP_ERR_INVALID, "invalid reading " + std::to_string(i));
  }
  const auto t0 = std::chrono::steady_clock::now();
  aicp_prefilter_params pfd;
  if (!pf) {
    aicp_hip_default_prefilter(&pfd);
    pf = &pfd;
  }
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  if (!ctx->loc) ctx->loc = new LocBufs();
  LocBufs* L = ctx->loc;
  L->last = aicp_localization_timing{};
  if (!L->ev_begin) HIPC(hipEventCreate(&L->ev_begin));
  if (!L->ev_end) HIPC(hipEventCreate(&L->ev_end));
  const bool debug = prm->flags & AICP_SEQ_DEBUG;
  LocRules rules{};
  rules.freq = prm->reference_update_frequency;
  rules.refilter_every = prm->map_refilter_every;
  rules.merge = (prm->flags & AICP_LOC_MERGE) ? 1 : 0;
  rules.max_corr = prm->max_correction_magnitude;
  aicp_icp_config c = *cfg;
  c.trimmed_ratio = aicp_hip_autotune_ratio(50.0f);  // octree_overlap_ = 50.0 (app.cpp:123-127)
  int rc = check_cfg(ctx, &c, AICP_RUN_ICP);
  if (rc) return rc;
  const int run_flags = AICP_RUN_ICP | (prm->flags & AICP_RUN_TIME_NN);

  // the stream's state: n_clouds = 0, initialT_ = I
  const size_t wmax = std::min<size_t>(std::max<size_t>(n, 1), (size_t)kMaxPairs);
  const size_t o_org = (sizeof(LocState) + 63) & ~size_t(63), o_rec = o_org + ((wmax * 24 + 63) & ~size_t(63));
  HIPC(ensure(L->state, sizeof(LocState)));
  HIPC(ensure(L->origin, wmax * 24));
  HIPC(ensure(L->rec, wmax * sizeof(LocRec)));
  HIPC(ensure(L->pin, o_rec + wmax * sizeof(LocRec)));
  char* lp = L->pin.as<char>();
  LocState* dS = L->state.as<LocState>();
  {
    LocState* hS = reinterpret_cast<LocState*>(lp);
    std::memset(hS, 0, sizeof(LocState));
    ident4(hS->initT);
    HIPC(hipMemcpyAsync(dS, hS, sizeof(LocState), hipMemcpyHostToDevice, s));
  }
  HIPC(hipEventRecord(L->ev_begin, s));
  std::vector<aicp_icp_stats> stats;
  int windows = 0, merges = 0, refilters = 0, status = AICP_OK;
  uint64_t n_clouds = 0;  // the host's mirror of LocState::n_clouds, from the records
  size_t p = 0;
  bool empty_crop = false;
  while (p < n && !status) {
    const size_t w = aicp_hip_localization_window(n_clouds, prm, n - p);
    const size_t map_n = map->n;
    // every reading's crop, straight into the batch's reference array (as the batch call). An
    // empty crop ends the stream at its reading; the wr readings before it still run
    size_t wr = 0;
    const uint32_t* htot = nullptr;
    rc = map_crop_pairs(ctx, map, prm->crop_min, prm->crop_max, readings + p, poses + 16 * p, w, nullptr, &wr, &htot);
    if (rc) return rc;
    if (wr) {
      aicp_hip_batch* B = ctx->mapbatch;
      double* horg = reinterpret_cast<double*>(lp + o_org);
      for (size_t i = 0; i < wr; ++i)
        for (int k = 0; k < 3; ++k) horg[3 * i + k] = readings[p + i].origin[k];
      HIPC(hipMemcpyAsync(L->origin.p, horg, wr * 24, hipMemcpyHostToDevice, s));
      if (debug) {  // (one reading per window) moved by the device's initialT_, its prior pose too
        launch_loc_move(s, (int)B->desc[0].n_read, dS->initT, L->origin.as<double>(),
                        B->read_raw.as<float4>() + B->desc[0].read_off);
        HIPC(hipGetLastError());
      }
      stats.assign(wr, aicp_icp_stats{});
      for (auto& st : stats) st.status = -1;
      rc = run_batch(ctx, B, &c, 0.0, run_flags, out_T + 16 * p, stats.data(), nullptr);
      if (rc && stats[0].status == -1) return rc;  // the batch did not run to its end (not a reading's status)
      ++windows;
      // App's bookkeeping for the window, on the device; one read-back of its records
      launch_loc_commit(s, (int)wr, ctx->state.as<PairState>(), ctx->outT.as<float>(), L->origin.as<double>(), rules,
                        dS, L->rec.as<LocRec>());
      HIPC(hipGetLastError());
      LocRec* hrec = reinterpret_cast<LocRec*>(lp + o_rec);
      HIPC(hipMemcpyAsync(hrec, L->rec.p, wr * sizeof(LocRec), hipMemcpyDeviceToHost, s));
      HIPC(hipStreamSynchronize(s));
      // the map changes the records ask for, in order (by the window rule: after the last reading)
      for (size_t i = 0; i < wr && !status; ++i) {
        const LocRec& r = hrec[i];
        aicp_localization_result& o = out[p + i];
        std::memset(&o, 0, sizeof(o));
        o.status = r.status;
        o.accepted = r.accepted;
        o.map_points = map_n;
        o.crop_points = htot[i];
        for (int k = 0; k < 3; ++k) o.corrected_origin[k] = r.corrected_origin[k];
        o.icp = stats[i];
        *n_done = p + i + 1;
        if (r.status) {
          status = r.status;
          break;
        }
        n_clouds += r.accepted ? 1 : 0;
        if (r.merged) {
          const PairDesc& d = B->desc[i];
          rc = map_reserve(ctx, map, d.n_read);
          if (rc) return rc;
          launch_loc_merge(s, (int)d.n_read, ctx->outT.as<float>() + 16 * i, B->read_raw.as<float4>() + d.read_off,
                           map->pts.as<float4>() + map->n);
          HIPC(hipGetLastError());
          map->n += d.n_read;
          o.merged = 1;
          ++merges;
        }
        if (r.refiltered) {
          rc = aicp_hip_map_prefilter(ctx, map, pf);
          if (rc) return rc;
          o.refiltered = 1;
          ++refilters;
        }
      }
    }
    if (!status && wr < w) {  // the reading with the empty crop (libpointmatcher throws on an empty cloud)
      aicp_localization_result& o = out[p + wr];
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
  L->last.merges = merges;
  L->last.refilters = refilters;
  L->last.device_ms = ev_ms(L->ev_begin, L->ev_end);
  L->last.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (status)
    ctx->err = "reading " + std::to_string(*n_done - 1) +
               (empty_crop ? std::string(": empty map crop") : ": status " + std::to_string(status));
  return status;
}

int aicp_hip_last_localization_timing(const aicp_hip_ctx* ctx, aicp_localization_timing* out) {
  if (!ctx || !out) return AICP_ERR_INVALID;
  *out = ctx->loc ? ctx->loc->last : aicp_localization_timing{};
  return AICP_OK;
}

}  // extern "C"
