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

#include <cstdint>
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

}  // namespace

int aicp::rt::chain_check(aicp_hip_ctx* ctx, const aicp_chain* c) {
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

namespace {

// what the kernels take of the dropping filter at `pos` of a side's list (one rule for the one-pair
// and the batch driver: the slot of the draw is 4 * side + pos)
ChainFilterArgs filter_args(const aicp_chain* chain, int side, int pos) {
  const aicp_chain_filter& f = chain->filters[side][pos];
  ChainFilterArgs a{};
  a.kind = f.kind;
  a.pos = pos;
  a.dim = f.dim;
  a.min_dist = f.min_dist;
  a.prob = f.prob;
  a.max_density = f.max_density;
  a.slot = (uint32_t)(AICP_CHAIN_MAX_FILTERS * side + pos);
  a.seed = chain->seed;
  return a;
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
  bool have_nrm = false, have_dens = false, sampled = false, emptied = false;
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
        emptied = (nrm || dens) && m == 0;
        launch_chain_pass(s, pos, ctl, nullptr);
      }
      continue;
    }
    const ChainFilterArgs a = filter_args(chain, side, pos);
    if (f.kind == AICP_FILTER_MAX_DENSITY && !have_dens) {
      if (!emptied) FAIL(AICP_ERR_INVALID, "MaxDensity without densities");
      launch_chain_pass(s, pos, ctl, nullptr);  // (no point reached the SurfaceNormal: none is left to drop)
      continue;
    }
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

// One side's list over C clouds at once (runtime.hpp). The shape of chain_side: every buffer sized by
// the side's rows as given, the sizes per cloud on the device (ChainCloud), one copy back at the end.
int aicp::rt::chain_batch_side(aicp_hip_ctx* ctx, const aicp_chain* chain, int side, size_t C, const uint32_t* n_in,
                               const float4* dsrc, const uint32_t* src_off, bool want_nrm, bool want_dens,
                               ChainBatchSide* o) {
  hipStream_t s = ctx->stream;
  ChainBufs& cb = ctx->chain[side];
  const int nf = chain->n_filters[side];
  const aicp_chain_filter* fl = chain->filters[side];
  uint64_t total = 0;
  for (size_t c = 0; c < C; ++c) total += n_in[c];
  if (C == 0 || C > (size_t)kMaxPairs || total >= (1ull << 31)) FAIL(AICP_ERR_UNSUPPORTED, "batch too large for a chain");
  ctx->refc.invalidate();  // (ctx->bpts / nodes / bnrm may be rewritten)
  ctx->rdc.valid = false;
  const size_t n = (size_t)total;
  const size_t tiles = chain_tiles(n);
  for (int q = 0; q < 2; ++q) HIPC(ensure(cb.pts[q], n * 16));
  HIPC(ensure(cb.flag, n));
  HIPC(ensure(cb.tile_cnt, tiles * 4));
  HIPC(ensure(cb.tile_off, tiles * 4));
  HIPC(ensure(cb.ctl, sizeof(ChainCtl)));
  HIPC(ensure(cb.clouds, C * sizeof(ChainCloud)));
  HIPC(ensure(cb.src_off, C * 4));
  // pinned: the records, then the upload offsets
  HIPC(ensure(cb.pin_cl, C * (sizeof(ChainCloud) + 4)));
  ChainCloud* hcl = cb.pin_cl.as<ChainCloud>();
  uint32_t* hoff = reinterpret_cast<uint32_t*>(hcl + C);
  std::memset(hcl, 0, C * sizeof(ChainCloud));
  uint32_t off = 0;
  for (size_t c = 0; c < C; ++c) {
    hcl[c].n[0] = n_in[c];
    hcl[c].off[0] = off;
    hcl[c].sn_slot = n_in[c] ? (int32_t)c : -1;
    hoff[c] = src_off[c];
    off += n_in[c];
  }
  ChainCloud* cl = cb.clouds.as<ChainCloud>();
  ChainCtl* ctl = cb.ctl.as<ChainCtl>();
  HIPC(hipMemcpyAsync(cl, hcl, C * sizeof(ChainCloud), hipMemcpyHostToDevice, s));
  HIPC(hipMemcpyAsync(cb.src_off.p, hoff, C * 4, hipMemcpyHostToDevice, s));
  launch_chainb_begin(s, (int)C, cl, (uint32_t)n, dsrc, cb.src_off.as<uint32_t>(), cb.pts[0].as<float4>(), ctl);
  int cur = 0;
  bool have_nrm = false, have_dens = false, sampled = false, emptied = false;
  *o = ChainBatchSide{};
  o->C = C;
  o->total = total;
  o->nf = nf;
  for (int pos = 0; pos < nf; ++pos) {
    const aicp_chain_filter& f = fl[pos];
    if (f.kind == AICP_FILTER_SURFACE_NORMAL) {
      bool later_density = false;
      for (int q = pos + 1; q < nf; ++q) later_density |= fl[q].kind == AICP_FILTER_MAX_DENSITY;
      const bool nrm = want_nrm, dens = f.keep_densities && (later_density || want_dens);
      if ((nrm || dens) && sampled) {  // the trees are sized by the clouds as this filter receives them
        HIPC(hipMemcpyAsync(hcl, cl, C * sizeof(ChainCloud), hipMemcpyDeviceToHost, s));
        HIPC(hipStreamSynchronize(s));
      }
      // the clouds that still have points, laid end to end as they lie: one tree each
      std::vector<PairDesc> td;
      uint64_t m = 0;
      if (nrm || dens)
        for (size_t c = 0; c < C; ++c) {
          // (not sampled: every cloud has points and its slot, its own number, is on the device)
          if (sampled) hcl[c].sn_slot = hcl[c].n[pos] ? (int32_t)td.size() : -1;
          if (!hcl[c].n[pos]) continue;
          PairDesc d{};
          d.ref_off = hcl[c].off[pos];
          d.n_ref = hcl[c].n[pos];
          d.ref_id = (int32_t)td.size();
          d.ratio = 0.5f;
          ident4(d.Tin);
          td.push_back(d);
          m += d.n_ref;
        }
      if ((nrm || dens) && m > 0) {
        if (!knn_served(f.knn)) FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn must be 10, 20 or 30");
        if (m >= (1ull << 28)) FAIL(AICP_ERR_UNSUPPORTED, "clouds too large for a chain's SurfaceNormal");
        const size_t T = td.size();
        if (sampled)  // (the slots the host just chose; the counts are the device's own)
          HIPC(hipMemcpyAsync(cl, hcl, C * sizeof(ChainCloud), hipMemcpyHostToDevice, s));
        HIPC(ensure(cb.pin_desc, T * sizeof(PairDesc)));
        std::memcpy(cb.pin_desc.p, td.data(), T * sizeof(PairDesc));
        HIPC(ensure(ctx->desc, T * sizeof(PairDesc)));
        HIPC(ensure(ctx->state, T * sizeof(PairState)));
        PairDesc* dd = ctx->desc.as<PairDesc>();
        HIPC(hipMemcpyAsync(dd, cb.pin_desc.p, T * sizeof(PairDesc), hipMemcpyHostToDevice, s));
        int rc = device_trees_begin(ctx->tb[0], ctx->err, s, T, m, dd, cb.pts[cur].as<float4>(), 0, kNormalsBucket,
                                    ctx->bpts, ctx->nodes);
        if (!rc) rc = device_trees_end(ctx->tb[0], ctx->err, s, T, m, dd, kNormalsBucket, ctx->bpts, ctx->nodes, 0);
        if (rc) return rc;
        HIPC(ensure(ctx->nbids, (size_t)m * 4 * (size_t)f.knn));
        HIPC(ensure(ctx->ctrs, kCtrWords * 4));
        HIPC(hipMemsetAsync(ctx->ctrs.p, 0, kCtrWords * 4, s));
        if (nrm) {
          HIPC(ensure(ctx->bnrm, (size_t)m * 16));
          for (int q = 0; q < 2; ++q) HIPC(ensure(cb.nrm[q], n * 16));
          launch_init_state(s, (int)T, dd, ctx->state.as<PairState>());
          if (!launch_normals(s, (int)T, (uint32_t)m, dd, ctx->state.as<PairState>(), ctx->nodes.as<uint4>(), nullptr,
                              ctx->bpts.as<float4>(), ctx->bnrm.as<float4>(), f.knn, ctx->nbids.as<int32_t>(),
                              ctx->ctrs.as<uint32_t>(), ctx->opt.normals_knn_engine))
            FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn");
        } else if (!launch_knn_ids(s, (int)T, (uint32_t)m, dd, ctx->nodes.as<uint4>(), ctx->bpts.as<float4>(), f.knn,
                                   ctx->nbids.as<int32_t>(), ctx->ctrs.as<uint32_t>(), nullptr,
                                   ctx->opt.normals_knn_engine)) {
          FAIL(AICP_ERR_UNSUPPORTED, "SurfaceNormal knn");
        }
        if (dens)
          for (int q = 0; q < 2; ++q) HIPC(ensure(cb.dens[q], n * 4));
        launch_chainb_sn_out(s, (int)T, dd, (uint32_t)m, f.knn, ctx->bpts.as<float4>(), ctx->nbids.as<int32_t>(),
                             ctx->bnrm.as<float4>(), nrm ? cb.nrm[cur].as<float4>() : nullptr,
                             dens ? cb.dens[cur].as<float>() : nullptr);
        if (dens && want_dens) {
          HIPC(ensure(cb.dens_sn, n * 4));
          HIPC(hipMemcpyAsync(cb.dens_sn.p, cb.dens[cur].p, (size_t)m * 4, hipMemcpyDeviceToDevice, s));
          o->dens_sn = true;
        }
        launch_chainb_pass(s, pos, (int)C, cl, ctl, nrm ? ctx->state.as<PairState>() : nullptr);
        have_nrm = nrm;
        have_dens = dens;
        o->sn_pos = pos;
      } else {
        emptied = (nrm || dens) && m == 0;
        launch_chainb_pass(s, pos, (int)C, cl, ctl, nullptr);
      }
      continue;
    }
    const ChainFilterArgs a = filter_args(chain, side, pos);
    if (f.kind == AICP_FILTER_MAX_DENSITY && !have_dens) {
      if (!emptied) FAIL(AICP_ERR_INVALID, "MaxDensity without densities");
      launch_chainb_pass(s, pos, (int)C, cl, ctl, nullptr);  // (no point reached the SurfaceNormal)
      continue;
    }
    bool dens_on = false;  // the densities travel until the last MaxDensity has run
    for (int q = pos + 1; q < nf; ++q) dens_on |= fl[q].kind == AICP_FILTER_MAX_DENSITY;
    launch_chainb_filter(s, (uint32_t)n, a, (int)C, cl, ctl, cb.flag.as<uint8_t>(), cb.tile_cnt.as<uint32_t>(),
                         cb.tile_off.as<uint32_t>(), cb.pts[cur].as<float4>(), cb.pts[cur ^ 1].as<float4>(),
                         have_nrm ? cb.nrm[cur].as<float4>() : nullptr, have_nrm ? cb.nrm[cur ^ 1].as<float4>() : nullptr,
                         have_dens ? cb.dens[cur].as<float>() : nullptr,
                         have_dens && dens_on ? cb.dens[cur ^ 1].as<float>() : nullptr);
    if (!dens_on) have_dens = false;
    cur ^= 1;
    sampled = true;
  }
  HIPC(hipGetLastError());
  HIPC(hipMemcpyAsync(hcl, cl, C * sizeof(ChainCloud), hipMemcpyDeviceToHost, s));
  o->cur = cur;
  o->nrm = have_nrm;
  o->cl = hcl;
  return AICP_OK;
}

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
  const int32_t degenerate = (int32_t)rr.degenerate;
  if (given) {
    if (!rr.nrm) FAIL(AICP_ERR_HIP, "chain normals missing");
    run.ref_normals = ctx->chain[0].nrm[rr.cur].as<float4>();
    run.degenerate = &degenerate;
  }
  run.max_dist = chain->outlier == AICP_OUTLIER_MAX_DIST;
  run.limit_d2 = chain->outlier_limit_d2;
  rc = run_batch(ctx, B, cfg, 0.0, AICP_RUN_ICP, out_T, stats, nullptr, &run);
  if (rc) (void)hipStreamSynchronize(ctx->stream);
  rcache.invalidate();
  return rc;
}

int aicp_hip_align_chain_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_chain* chain,
                               const aicp_pair* pairs, size_t n_pairs, double resolution, int flags, float* out_T,
                               aicp_icp_stats* stats, aicp_chain_stats* chain_stats) {
  if (!ctx) return AICP_ERR_INVALID;
  if (!pairs || n_pairs == 0 || !out_T) FAIL(AICP_ERR_INVALID, "align_chain_batch arguments");
  if (flags != AICP_RUN_ICP && flags != (AICP_RUN_ICP | AICP_RUN_OVERLAP))
    FAIL(AICP_ERR_INVALID, "align_chain_batch flags: AICP_RUN_ICP, with or without AICP_RUN_OVERLAP");
  const bool doOvl = (flags & AICP_RUN_OVERLAP) != 0;
  const size_t P = n_pairs;
  for (size_t i = 0; i < P; ++i)
    if (!valid_pair(pairs[i])) FAIL(AICP_ERR_INVALID, "invalid pair " + std::to_string(i));
  if (P > (size_t)kMaxPairs) FAIL(AICP_ERR_UNSUPPORTED, "more than 4096 pairs in one batch");
  HIPC(hipSetDevice(ctx->device));
  int rc = check_cfg(ctx, cfg, flags);
  if (!rc) rc = chain_check(ctx, chain);
  if (rc) return rc;
  if (doOvl && !(resolution > 0)) FAIL(AICP_ERR_INVALID, "resolution");
  // neither uses nor keeps the reference cache (and the last reading's copy)
  RefCache& rcache = ctx->refc;
  rcache.use = rcache.hit_trees = rcache.hit_ovl = false;
  rcache.invalidate();
  ctx->rdc.hit = false;
  ctx->rdc.valid = false;
  if (!ctx->oneshot) ctx->oneshot = new aicp_hip_batch();
  if (!ctx->chainbatch) ctx->chainbatch = new aicp_hip_batch();
  const int nfR = chain->n_filters[0], nfD = chain->n_filters[1];
  if (chain_stats) {
    std::memset(chain_stats, 0, P * sizeof(*chain_stats));
    for (size_t i = 0; i < P; ++i) {
      chain_stats[i].n_in[0] = chain_stats[i].n_kept[0] = pairs[i].n_ref;
      chain_stats[i].n_in[1] = chain_stats[i].n_kept[1] = pairs[i].n_read;
    }
  }
  if (chain_plain(*chain)) {  // aicp_hip_align_batch's path, its cache off
    for (size_t i = 0; i < P && chain_stats; ++i)
      for (int side = 0; side < 2; ++side)
        for (int q = 0; q < chain->n_filters[side]; ++q) chain_stats[i].n_out[side][q] = chain_stats[i].n_in[side];
    rc = upload_pairs(ctx, pairs, P, ctx->oneshot, false, false, false, true);
    if (!rc) rc = run_batch(ctx, ctx->oneshot, cfg, resolution, flags, out_T, stats, nullptr);
    if (rc) (void)hipStreamSynchronize(ctx->stream);
    return rc;
  }
  hipStream_t s = ctx->stream;
  // the clouds as given, uploaded once: they serve the overlap and the filters
  aicp_hip_batch* B0 = ctx->chainbatch;
  rc = upload_pairs(ctx, pairs, P, B0, false, false, false, true);
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  const size_t R = B0->rdesc.size();
  bool ref_sn = false;
  for (int q = 0; q < nfR; ++q) ref_sn |= chain->filters[0][q].kind == AICP_FILTER_SURFACE_NORMAL;
  const bool given = cfg->knn_normals != 0 && ref_sn;
  std::vector<uint32_t> cnt(R + P), off(R + P);
  for (size_t r = 0; r < R; ++r) {
    cnt[r] = B0->rdesc[r].n_ref;
    off[r] = B0->rdesc[r].ref_off;
  }
  for (size_t i = 0; i < P; ++i) {
    cnt[R + i] = B0->desc[i].n_read;
    off[R + i] = B0->desc[i].read_off;
  }
  // the distinct references' list once each, the readings', then one wait for all the counts: the
  // overlap's own, where it runs (on the clouds as given, behind the filters on the same stream)
  ChainBatchSide sr, sd;
  rc = chain_batch_side(ctx, chain, AICP_CHAIN_REFERENCE, R, cnt.data(), B0->ref_raw.as<float4>(), off.data(), given,
                        false, &sr);
  if (!rc)
    rc = chain_batch_side(ctx, chain, AICP_CHAIN_READING, P, cnt.data() + R, B0->read_raw.as<float4>(), off.data() + R,
                          false, false, &sd);
  std::vector<aicp_icp_stats> ost;
  if (!rc && doOvl) {
    ost.resize(P);
    rc = run_batch(ctx, B0, cfg, resolution, AICP_RUN_OVERLAP, nullptr, ost.data(), nullptr);
  } else if (!rc) {
    HIPC(hipStreamSynchronize(s));
  }
  if (rc) {
    (void)hipStreamSynchronize(s);
    return rc;
  }
  // (the records leave the pinned staging: the sides' buffers are written again below)
  const std::vector<ChainCloud> cr(sr.cl, sr.cl + R), cd(sd.cl, sd.cl + P);
  for (size_t r = 0; r < R; ++r)
    if (cr[r].n[nfR] > cr[r].n[0] || cr[r].off[nfR] + (uint64_t)cr[r].n[nfR] > sr.total)
      FAIL(AICP_ERR_HIP, "chain filter count");
  for (size_t i = 0; i < P; ++i)
    if (cd[i].n[nfD] > cd[i].n[0] || cd[i].off[nfD] + (uint64_t)cd[i].n[nfD] > sd.total)
      FAIL(AICP_ERR_HIP, "chain filter count");
  // the pairs that run: both sides kept a point. Their references, numbered as they first appear
  std::vector<size_t> live;
  std::vector<int32_t> new_ref(R, -1);
  std::vector<size_t> live_refs;
  std::vector<int> status(P, AICP_OK);
  for (size_t i = 0; i < P; ++i) {
    const size_t r = (size_t)B0->desc[i].ref_id;
    if (chain_stats) {
      for (int q = 0; q < nfR; ++q) chain_stats[i].n_out[0][q] = cr[r].n[q + 1];
      for (int q = 0; q < nfD; ++q) chain_stats[i].n_out[1][q] = cd[i].n[q + 1];
      chain_stats[i].n_kept[0] = cr[r].n[nfR];
      chain_stats[i].n_kept[1] = cd[i].n[nfD];
    }
    if (cr[r].n[nfR] == 0 || cd[i].n[nfD] == 0) {
      status[i] = AICP_ERR_CONVERGENCE;
      continue;
    }
    if (new_ref[r] < 0) {
      new_ref[r] = (int32_t)live_refs.size();
      live_refs.push_back(r);
    }
    live.push_back(i);
  }
  const size_t L = live.size(), RL = live_refs.size();
  std::vector<float> lT(16 * std::max<size_t>(L, 1));
  std::vector<aicp_icp_stats> lst(std::max<size_t>(L, 1));
  if (L) {
    // the filtered clouds as a batch whose points are written on the device; a reference's identity
    // is its number among those that run
    std::vector<aicp_pair> fp(L);
    std::vector<int32_t> ref_ids(L);
    std::vector<float> ratios(L);
    for (size_t k = 0; k < L; ++k) {
      const size_t i = live[k], r = (size_t)B0->desc[i].ref_id;
      fp[k] = pairs[i];
      fp[k].ref = nullptr;
      fp[k].ref_stride = 16;
      ref_ids[k] = new_ref[r];
      fp[k].n_ref = cr[r].n[nfR];
      fp[k].n_read = cd[i].n[nfD];
      ratios[k] = doOvl ? autotune_ratio_fast(ost[i].overlap_percent) : cfg->trimmed_ratio;
    }
    aicp_hip_batch* B = ctx->oneshot;
    rc = upload_pairs(ctx, fp.data(), L, B, false, true, true, true, ref_ids.data());
    if (rc) return rc;
    if (B->rdesc.size() != RL) FAIL(AICP_ERR_HIP, "chain batch references");
    for (int side = 0; side < 2; ++side) {
      ChainBufs& cb = ctx->chain[side];
      const size_t ns = side ? L : RL;
      HIPC(ensure(cb.pin_seg, ns * sizeof(ChainSeg)));
      HIPC(ensure(cb.segs, ns * sizeof(ChainSeg)));
      ChainSeg* hs = cb.pin_seg.as<ChainSeg>();
      for (size_t k = 0; k < ns; ++k) {
        if (side)
          hs[k] = ChainSeg{B->desc[k].read_off, cd[live[k]].off[nfD], cd[live[k]].n[nfD], 0u};
        else
          hs[k] = ChainSeg{B->rdesc[k].ref_off, cr[live_refs[k]].off[nfR], cr[live_refs[k]].n[nfR], 0u};
      }
      HIPC(hipMemcpyAsync(cb.segs.p, hs, ns * sizeof(ChainSeg), hipMemcpyHostToDevice, s));
      const ChainBatchSide& sb = side ? sd : sr;
      const bool nrm = !side && given;
      if (nrm && !sb.nrm) FAIL(AICP_ERR_HIP, "chain normals missing");
      launch_chainb_rows(s, (int)ns, cb.segs.as<ChainSeg>(), (uint32_t)(side ? B->total_read : B->total_ref),
                         cb.pts[sb.cur].as<float4>(), (side ? B->read_raw : B->ref_raw).as<float4>(),
                         nrm ? cb.nrm[sb.cur].as<float4>() : nullptr, nrm ? cb.nrm[sb.cur ^ 1].as<float4>() : nullptr);
    }
    ChainRun run;
    std::vector<int32_t> degenerate(RL);
    for (size_t k = 0; k < RL; ++k) degenerate[k] = (int32_t)cr[live_refs[k]].degenerate;
    if (given) {
      run.ref_normals = ctx->chain[0].nrm[sr.cur ^ 1].as<float4>();
      run.degenerate = degenerate.data();
    }
    run.max_dist = chain->outlier == AICP_OUTLIER_MAX_DIST;
    run.limit_d2 = chain->outlier_limit_d2;
    run.batch = true;
    run.ratios = ratios.data();
    aicp_icp_config c2 = *cfg;
    if (doOvl) c2.trimmed_ratio = 1.f;  // (not read: every pair has its own)
    rc = run_batch(ctx, B, &c2, 0.0, AICP_RUN_ICP, lT.data(), lst.data(), nullptr, &run);
    rcache.invalidate();
    bool any = false;
    for (size_t k = 0; k < L; ++k) any |= lst[k].status != 0;
    if (rc && !any) {  // not a pair's status: the run itself failed
      (void)hipStreamSynchronize(s);
      return rc;
    }
  }
  // results in the caller's pair order
  for (size_t i = 0; i < P; ++i) {
    ident4(out_T + 16 * i);
    if (stats) {
      std::memset(&stats[i], 0, sizeof(stats[i]));
      stats[i].status = AICP_ERR_CONVERGENCE;
      stats[i].overlap_percent = -1.f;
    }
  }
  for (size_t k = 0; k < L; ++k) {
    const size_t i = live[k];
    std::memcpy(out_T + 16 * i, lT.data() + 16 * k, 64);
    status[i] = lst[k].status;
    if (stats) stats[i] = lst[k];
  }
  if (doOvl)
    for (size_t i = 0; i < P; ++i) {
      if (!stats) break;
      stats[i].overlap_percent = ost[i].overlap_percent;
      for (int k = 0; k < 3; ++k) stats[i].overlap_keys[k] = ost[i].overlap_keys[k];
      stats[i].trimmed_ratio = autotune_ratio_fast(ost[i].overlap_percent);
    }
  for (size_t i = 0; i < P; ++i) {
    if (!status[i]) continue;
    const size_t r = (size_t)B0->desc[i].ref_id;
    if (cr[r].n[nfR] == 0)
      ctx->err = "pair " + std::to_string(i) + ": the chain's filters leave no point of the reference";
    else if (cd[i].n[nfD] == 0)
      ctx->err = "pair " + std::to_string(i) + ": the chain's filters leave no point of the reading";
    else
      ctx->err = "pair " + std::to_string(i) + ": pair status " + std::to_string(status[i]);
    return status[i];
  }
  return AICP_OK;
}

}  // extern "C"
