// chain.cpp — the sampled ICP chains: libpointmatcher's data-point filter lists on the
// device and the registration that runs on what they leave.
//
//   aicp_hip_chain_filter    DataPointsFilters::apply of one side's list on one cloud
//   aicp_hip_register_chain  both sides filtered, then the ICP core (run_batch) on the filtered
//                            clouds where they lie; MaxDistOutlierFilter through ChainRun
//
// One side: the cloud is uploaded once (w = input index), SurfaceNormal builds the raw tree of the
// cloud at its position (the tree, kNN and eigen kernels of aicp_hip_normals) and leaves normals
// and densities in that cloud's order; MinDist / RandomSampling / MaxDensity are order-preserving
// compactions (kernels_chain.hip) that carry those descriptors along. The filters' counts stay on
// the device and are read once after the last filter; only a SurfaceNormal behind another filter
// needs its cloud's size earlier, to size its tree.
#include <hip/hip_runtime.h>

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

namespace {

bool knn_served(int knn) { return knn == 10 || knn == 20 || knn == 30; }

// no filter but SurfaceNormal, TrimmedDist: the chain aicp_hip_register serves
bool chain_plain(const aicp_chain& c) {
  if (c.outlier != AICP_OUTLIER_TRIMMED_DIST) return false;
  for (int side = 0; side < 2; ++side)
    for (int q = 0; q < c.n_filters[side]; ++q)
      if (c.filters[side][q].kind != AICP_FILTER_SURFACE_NORMAL) return false;
  return true;
}

int chain_check(aicp_hip_ctx* ctx, const aicp_chain* c) {
  if (!c) FAIL(AICP_ERR_INVALID, "null chain");
  if (c->outlier != AICP_OUTLIER_TRIMMED_DIST && c->outlier != AICP_OUTLIER_MAX_DIST)
    FAIL(AICP_ERR_INVALID, "chain outlier rule");
  // finite: a reading without a match has d2 = inf, which an infinite limit would keep
  if (c->outlier == AICP_OUTLIER_MAX_DIST && !(c->outlier_limit_d2 >= 0.f && std::isfinite(c->outlier_limit_d2)))
    FAIL(AICP_ERR_INVALID, "MaxDist limit must be finite and not negative");
  for (int side = 0; side < 2; ++side) {
    if (c->n_filters[side] < 0 || c->n_filters[side] > AICP_CHAIN_MAX_FILTERS)
      FAIL(AICP_ERR_UNSUPPORTED, "more than 4 data-point filters on a side");
    int sn = 0;
    bool dens = false;
    for (int q = 0; q < c->n_filters[side]; ++q) {
      const aicp_chain_filter& f = c->filters[side][q];
      switch (f.kind) {
        case AICP_FILTER_SURFACE_NORMAL:
          if (++sn > 1) FAIL(AICP_ERR_UNSUPPORTED, "two SurfaceNormal filters on a side");
          dens = f.keep_densities != 0;
          break;
        case AICP_FILTER_MIN_DIST:
          if (f.dim < -1 || f.dim > 2) FAIL(AICP_ERR_INVALID, "MinDist.dim");
          break;
        case AICP_FILTER_RANDOM_SAMPLING:
          if (!(f.prob >= 0.f && f.prob <= 1.f)) FAIL(AICP_ERR_INVALID, "RandomSampling.prob");
          break;
        case AICP_FILTER_MAX_DENSITY:
          if (!(f.max_density > 0.f)) FAIL(AICP_ERR_INVALID, "MaxDensity.maxDensity");
          if (!dens) FAIL(AICP_ERR_INVALID, "MaxDensity without densities (SurfaceNormal keepDensities)");
          break;
        default:
          FAIL(AICP_ERR_INVALID, "chain filter kind");
      }
    }
  }
  return AICP_OK;
}

struct SideRun {
  uint32_t counts[AICP_CHAIN_MAX_FILTERS + 1] = {};  // the cloud as given, then after each filter
  uint32_t kept = 0;
  uint32_t n_sn = 0;        // the cloud's size at the SurfaceNormal that ran (0: none ran)
  uint32_t degenerate = 0;
  int cur = 0;              // the set of ChainBufs that holds the filtered cloud
  bool nrm = false, dens_sn = false;  // normals carried; densities at the SurfaceNormal copied to dens_sn
};

// kd-tree of n points that lie on the device, as upload_tree builds it for aicp_hip_normals
// (bucket 8, raw coordinates, into ctx->bpts / nodes / desc)
int chain_tree(aicp_hip_ctx* ctx, const float4* dpts, size_t n) {
  hipStream_t s = ctx->stream;
  PairDesc d{};
  d.n_ref = (uint32_t)n;
  d.ratio = 0.5f;
  ident4(d.Tin);
  HIPC(ensure(ctx->desc, sizeof(PairDesc)));
  HIPC(hipMemcpyAsync(ctx->desc.p, &d, sizeof(d), hipMemcpyHostToDevice, s));
  int rc = device_trees_begin(ctx->tb[0], ctx->err, s, 1, n, ctx->desc.as<PairDesc>(), dpts, 0, kNormalsBucket,
                              ctx->bpts, ctx->nodes);
  if (rc) return rc;
  return device_trees_end(ctx->tb[0], ctx->err, s, 1, n, ctx->desc.as<PairDesc>(), kNormalsBucket, ctx->bpts,
                          ctx->nodes, 0);
}

// One side's list on one cloud. want_nrm: the kept points' normals are wanted (a SurfaceNormal of
// knn 10 / 20 / 30 on the side); want_dens: the densities at the SurfaceNormal are wanted by the
// caller, beyond what a MaxDensity consumes. A SurfaceNormal whose outputs nobody wants runs nothing.
int chain_side(aicp_hip_ctx* ctx, const aicp_chain* chain, int side, const float* pts, size_t n, size_t stride,
               bool want_nrm, bool want_dens, SideRun* o) {
  hipStream_t s = ctx->stream;
  ChainBufs& cb = ctx->chain[side];
  const int nf = chain->n_filters[side];
  const aicp_chain_filter* fl = chain->filters[side];
  if (n >= (1ull << 28)) FAIL(AICP_ERR_UNSUPPORTED, "cloud too large for a chain");
  ctx->refc.invalidate();  // (ctx->bpts / nodes / bnrm may be rewritten)
  ctx->rdc.valid = false;
  const size_t tiles = chain_tiles(n);
  for (int q = 0; q < 2; ++q) HIPC(ensure(cb.pts[q], n * 16));
  HIPC(ensure(cb.flag, n));
  HIPC(ensure(cb.tile_cnt, tiles * 4));
  HIPC(ensure(cb.tile_off, tiles * 4));
  HIPC(ensure(cb.ctl, sizeof(ChainCtl)));
  HIPC(ensure(ctx->pin_chain, 2 * sizeof(ChainCtl)));
  HIPC(ensure(ctx->pin_io, n * 16));
  pack_xyz4(pts, n, stride, ctx->pin_io.as<float>());
  HIPC(hipMemcpyAsync(cb.pts[0].p, ctx->pin_io.p, n * 16, hipMemcpyHostToDevice, s));
  ChainCtl* ctl = cb.ctl.as<ChainCtl>();
  ChainCtl* hctl = ctx->pin_chain.as<ChainCtl>() + side;
  launch_chain_begin(s, (uint32_t)n, cb.pts[0].as<float4>(), ctl);
  int cur = 0;
  bool have_nrm = false, have_dens = false, sampled = false;
  *o = SideRun{};
  for (int pos = 0; pos < nf; ++pos) {
    const aicp_chain_filter& f = fl[pos];
    if (f.kind == AICP_FILTER_SURFACE_NORMAL) {
      bool later_density = false;
      for (int q = pos + 1; q < nf; ++q) later_density |= fl[q].kind == AICP_FILTER_MAX_DENSITY;
      const bool nrm = want_nrm, dens = f.keep_densities && (later_density || want_dens);
      uint32_t m = (uint32_t)n;
      if ((nrm || dens) && sampled) {  // the tree is sized by the cloud as this filter receives it
        HIPC(hipMemcpyAsync(hctl, ctl, sizeof(ChainCtl), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
        m = hctl->n[pos];
      }
      if ((nrm || dens) && m > 0) {
        if (!knn_served(f.knn)) FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn must be 10, 20 or 30");
        int rc = chain_tree(ctx, cb.pts[cur].as<float4>(), m);
        if (rc) return rc;
        HIPC(ensure(ctx->nbids, (size_t)m * 4 * (size_t)f.knn));
        HIPC(ensure(ctx->ctrs, kCtrWords * 4));
        HIPC(hipMemsetAsync(ctx->ctrs.p, 0, kCtrWords * 4, s));
        if (nrm) {
          HIPC(ensure(ctx->state, sizeof(PairState)));
          HIPC(ensure(ctx->bnrm, (size_t)m * 16));
          for (int q = 0; q < 2; ++q) HIPC(ensure(cb.nrm[q], n * 16));
          launch_init_state(s, 1, ctx->desc.as<PairDesc>(), ctx->state.as<PairState>());
          if (!launch_normals(s, 1, m, ctx->desc.as<PairDesc>(), ctx->state.as<PairState>(), ctx->nodes.as<uint4>(),
                              nullptr, ctx->bpts.as<float4>(), ctx->bnrm.as<float4>(), f.knn, ctx->nbids.as<int32_t>(),
                              ctx->ctrs.as<uint32_t>(), ctx->opt.normals_knn_engine))
            FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn");
        } else if (!launch_knn_ids(s, 1, m, ctx->desc.as<PairDesc>(), ctx->nodes.as<uint4>(), ctx->bpts.as<float4>(),
                                   f.knn, ctx->nbids.as<int32_t>(), ctx->ctrs.as<uint32_t>(), nullptr,
                                   ctx->opt.normals_knn_engine)) {
          FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn");
        }
        if (dens)
          for (int q = 0; q < 2; ++q) HIPC(ensure(cb.dens[q], n * 4));
        launch_chain_sn_out(s, m, f.knn, ctx->bpts.as<float4>(), ctx->nbids.as<int32_t>(), ctx->bnrm.as<float4>(),
                            nrm ? cb.nrm[cur].as<float4>() : nullptr, dens ? cb.dens[cur].as<float>() : nullptr);
        if (dens && want_dens) {
          HIPC(ensure(cb.dens_sn, n * 4));
          HIPC(hipMemcpyAsync(cb.dens_sn.p, cb.dens[cur].p, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
          o->dens_sn = true;
        }
        launch_chain_pass(s, pos, ctl, nrm ? ctx->state.as<PairState>() : nullptr);
        have_nrm = nrm;
        have_dens = dens;
        o->n_sn = m;
      } else {
        launch_chain_pass(s, pos, ctl, nullptr);
      }
      continue;
    }
    ChainFilterArgs a{};
    a.kind = f.kind;
    a.pos = pos;
    a.dim = f.dim;
    a.min_dist = f.min_dist;
    a.prob = f.prob;
    a.max_density = f.max_density;
    a.slot = (uint32_t)(AICP_CHAIN_MAX_FILTERS * side + pos);
    a.seed = chain->seed;
    if (f.kind == AICP_FILTER_MAX_DENSITY && !have_dens) FAIL(AICP_ERR_INVALID, "MaxDensity without densities");
    // the densities travel until the MaxDensity has run
    bool dens_on = false;
    for (int q = pos + 1; q < nf; ++q) dens_on |= fl[q].kind == AICP_FILTER_MAX_DENSITY;
    launch_chain_filter(s, (uint32_t)n, a, ctl, cb.flag.as<uint8_t>(), cb.tile_cnt.as<uint32_t>(),
                        cb.tile_off.as<uint32_t>(), cb.pts[cur].as<float4>(), cb.pts[cur ^ 1].as<float4>(),
                        have_nrm ? cb.nrm[cur].as<float4>() : nullptr, have_nrm ? cb.nrm[cur ^ 1].as<float4>() : nullptr,
                        have_dens ? cb.dens[cur].as<float>() : nullptr,
                        have_dens && dens_on ? cb.dens[cur ^ 1].as<float>() : nullptr);
    if (!dens_on) have_dens = false;
    cur ^= 1;
    sampled = true;
  }
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(hctl, ctl, sizeof(ChainCtl), hipMemcpyDeviceToHost, s));
  HIPC(hipStreamSynchronize(s));
  for (int q = 0; q <= AICP_CHAIN_MAX_FILTERS; ++q) o->counts[q] = hctl->n[q];
  o->kept = hctl->n[nf];
  o->degenerate = hctl->degenerate;
  o->cur = cur;
  o->nrm = have_nrm;
  if (o->kept > n) FAIL(AICP_ERR_HIP, "chain filter count");
  return AICP_OK;
}

}  // namespace

extern "C" {

int aicp_hip_chain_filter(aicp_hip_ctx* ctx, const aicp_chain* chain, int side, const float* pts, size_t n,
                          size_t stride, uint64_t* out_n, uint64_t out_counts[AICP_CHAIN_MAX_FILTERS], int32_t* out_index,
                          float* out_densities, float* out_normals) {
  if (!ctx) return AICP_ERR_INVALID;
  if (!pts || !out_n || n == 0 || stride < 12 || stride % 4 || (side != AICP_CHAIN_REFERENCE && side != AICP_CHAIN_READING))
    FAIL(AICP_ERR_INVALID, "chain_filter arguments");
  HIPC(hipSetDevice(ctx->device));
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
  SideRun r;
  rc = chain_side(ctx, chain, side, pts, n, stride, out_normals != nullptr, out_densities != nullptr, &r);
  if (rc) return rc;
  *out_n = r.kept;
  if (out_counts)
    for (int q = 0; q < AICP_CHAIN_MAX_FILTERS; ++q) out_counts[q] = q < chain->n_filters[side] ? r.counts[q + 1] : 0;
  const ChainBufs& cb = ctx->chain[side];
  std::vector<float> h;
  if (out_index && r.kept) {
    h.resize(4 * (size_t)r.kept);
    HIPC(hipMemcpy(h.data(), cb.pts[r.cur].p, (size_t)r.kept * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r.kept; ++i) std::memcpy(&out_index[i], &h[4 * i + 3], 4);
  }
  if (out_normals && r.kept) {
    if (!r.nrm) FAIL(AICP_ERR_HIP, "chain normals missing");
    h.resize(4 * (size_t)r.kept);
    HIPC(hipMemcpy(h.data(), cb.nrm[r.cur].p, (size_t)r.kept * 16, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < r.kept; ++i)
      for (int k = 0; k < 3; ++k) out_normals[3 * i + k] = h[4 * i + k];
  }
  if (out_densities && r.dens_sn && r.n_sn)
    HIPC(hipMemcpy(out_densities, cb.dens_sn.p, (size_t)r.n_sn * 4, hipMemcpyDeviceToHost));
  return AICP_OK;
}

int aicp_hip_register_chain(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_chain* chain,
                            const aicp_pair* pair, float out_T[16], aicp_icp_stats* stats,
                            aicp_chain_stats* chain_stats) {
  if (!ctx) return AICP_ERR_INVALID;
  if (!pair || !out_T || !valid_pair(*pair)) FAIL(AICP_ERR_INVALID, "register_chain arguments");
  HIPC(hipSetDevice(ctx->device));
  int rc = check_cfg(ctx, cfg, AICP_RUN_ICP);
  if (!rc) rc = chain_check(ctx, chain);
  if (rc) return rc;
  // neither uses nor keeps the reference cache (and the last reading's copy)
  RefCache& rcache = ctx->refc;
  rcache.use = rcache.hit_trees = rcache.hit_ovl = false;
  rcache.invalidate();
  ctx->rdc.hit = false;
  ctx->rdc.valid = false;
  if (!ctx->oneshot) ctx->oneshot = new aicp_hip_batch();
  aicp_hip_batch* B = ctx->oneshot;
  if (chain_stats) {
    std::memset(chain_stats, 0, sizeof(*chain_stats));
    chain_stats->n_in[0] = chain_stats->n_kept[0] = pair->n_ref;
    chain_stats->n_in[1] = chain_stats->n_kept[1] = pair->n_read;
  }
  if (chain_plain(*chain)) {  // aicp_hip_register's path, its cache off
    for (int side = 0; side < 2 && chain_stats; ++side)
      for (int q = 0; q < chain->n_filters[side]; ++q) chain_stats->n_out[side][q] = chain_stats->n_in[side];
    rc = upload_pairs(ctx, pair, 1, B, false, false, false, true);
    if (!rc) rc = run_batch(ctx, B, cfg, 0.0, AICP_RUN_ICP, out_T, stats, nullptr);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  // the reference's normals come from its SurfaceNormal, at that filter's position
  bool ref_sn = false;
  for (int q = 0; q < chain->n_filters[AICP_CHAIN_REFERENCE]; ++q)
    ref_sn |= chain->filters[AICP_CHAIN_REFERENCE][q].kind == AICP_FILTER_SURFACE_NORMAL;
  const bool given = cfg->knn_normals != 0 && ref_sn;
  SideRun rr, rd;
  rc = chain_side(ctx, chain, AICP_CHAIN_REFERENCE, pair->ref, pair->n_ref, pair->ref_stride, given, false, &rr);
  if (!rc) rc = chain_side(ctx, chain, AICP_CHAIN_READING, pair->read, pair->n_read, pair->read_stride, false, false, &rd);
  if (rc) return rc;
  if (chain_stats) {
    for (int q = 0; q < chain->n_filters[0]; ++q) chain_stats->n_out[0][q] = rr.counts[q + 1];
    for (int q = 0; q < chain->n_filters[1]; ++q) chain_stats->n_out[1][q] = rd.counts[q + 1];
    chain_stats->n_kept[0] = rr.kept;
    chain_stats->n_kept[1] = rd.kept;
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->status = AICP_ERR_CONVERGENCE;
    stats->overlap_percent = -1.f;
  }
  if (rr.kept == 0) FAIL(AICP_ERR_CONVERGENCE, "the chain's filters leave no point of the reference");
  if (rd.kept == 0) FAIL(AICP_ERR_CONVERGENCE, "the chain's filters leave no point of the reading");
  // the filtered clouds as a one-pair batch whose points are written on the device
  aicp_pair fp = *pair;
  fp.n_ref = rr.kept;
  fp.n_read = rd.kept;
  rc = upload_pairs(ctx, &fp, 1, B, true, false, true, true);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  launch_chain_rows(s, rr.kept, ctx->chain[0].pts[rr.cur].as<float4>(), B->ref_raw.as<float4>());
  launch_chain_rows(s, rd.kept, ctx->chain[1].pts[rd.cur].as<float4>(), B->read_raw.as<float4>());
  ChainRun run;
  if (given) {
    if (!rr.nrm) FAIL(AICP_ERR_HIP, "chain normals missing");
    run.ref_normals = ctx->chain[0].nrm[rr.cur].as<float4>();
    run.degenerate = (int32_t)rr.degenerate;
  }
  run.max_dist = chain->outlier == AICP_OUTLIER_MAX_DIST;
  run.limit_d2 = chain->outlier_limit_d2;
  rc = run_batch(ctx, B, cfg, 0.0, AICP_RUN_ICP, out_T, stats, nullptr, &run);
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  rcache.invalidate();
  return rc;
}

}  // extern "C"
