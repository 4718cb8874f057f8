// kernels.hpp — launch wrappers of the HIP kernels (host-callable).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aicp_common.hpp"

namespace aicp {

// Block -> (pair, first local index) tables for a flat grid over per-pair ranges.
struct BlockMap {
  const int32_t* pair;
  const uint32_t* start;
  uint32_t n_blocks;
};

// ---- ICP ---------------------------------------------------------------------------------
void launch_prepare_read(hipStream_t s, BlockMap m, const PairDesc* pd, const float4* read_raw,
                         float4* read_c);
// Spatial (Morton) order of the reading points of every pair, inside each pair's own range
// (kernels_order.hip). keys*/vals*: total entries each; temp: read_order_temp_bytes.
size_t read_order_temp_bytes(size_t n, int n_pairs);
hipError_t launch_read_order(hipStream_t s, BlockMap m, int n_pairs, const PairDesc* pd, const float4* raw,
                             uint32_t total, uint64_t* keys0, uint64_t* keys1, uint32_t* vals0, uint32_t* vals1,
                             void* temp, size_t temp_bytes, float4* out);
void launch_init_state(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st);
// SurfaceNormal of the reference points (bucket order); ids: scratch of total_ref * knn;
// ctr: kPersistCtrWords work counters (zeroed on s when the persistent engine runs). engine:
// aicp_hip_options::normals_knn_engine.
// Returns false if knn is unsupported.
bool launch_normals(hipStream_t s, int n_pairs, uint32_t total_ref, const PairDesc* pd, PairState* st,
                    const uint4* nodes, const int32_t* parent, const float4* bpts, float4* bnrm, int knn,
                    int32_t* ids, uint32_t* ctr, int engine);
// the kNN of every reference point in its own tree (bucket order in and out: ids are bucket
// positions of the pair's tree, -1 past the cloud size); eps 0, self included. touched
// (nullable, zeroed): += touched points, inner nodes. engine_used (nullable, tests): the engine
// whose kernel was launched: 1 one query per octet of lanes (k_knn_oct), 2 one per lane (k_knn_ids)
bool launch_knn_ids(hipStream_t s, int n_pairs, uint32_t total_ref, const PairDesc* pd, const uint4* nodes,
                    const float4* bpts, int knn, int32_t* ids, uint32_t* ctr, unsigned long long* touched,
                    int engine, int* engine_used = nullptr);
// host_n (nullable): device pointer of mapped host memory that receives the active count;
// done_sig (nullable, signal memory): once no pair is active, the final corrections go to outT
// and *ticket is stored to done_sig (the sequence's next reference waits on it)
void launch_active_list(hipStream_t s, int n_pairs, const PairDesc* pd, const PairState* st,
                        ActiveList* al, uint32_t* ctr, uint32_t* host_n = nullptr, uint64_t* done_sig = nullptr,
                        const uint64_t* ticket = nullptr, float* outT = nullptr, int src_pair = -1);
// Fused ICP iteration: the last workgroup of a
// pair to finish the histogram / compaction / reduction runs that pair's find1 / final select /
// update, and the last pair of the group rebuilds the active list for the next iteration (and,
// when none is left, publishes the corrections and the sequence ticket). Four launches per
// iteration (NN, select x2, reduce) instead of eight. Counters start at zero (icp_sync_words per
// pair group) and reset themselves.
struct IcpIterSync {
  uint32_t* sel1;   // per pair (absolute index): histogram workgroups arrived
  uint32_t* sel2;   // per pair: compaction workgroups arrived
  uint32_t* red;    // per pair: reduction workgroups arrived
  uint32_t* pairs;  // pairs of the group done with this iteration
  int np;           // the group's pairs (pd, st point at its first)
  const PairDesc* pd;
  PairState* st;
  ActiveList* al;
  uint32_t* ctr;
  uint32_t* host_n;    // nullable: the active count for the next iteration (mapped host memory)
  uint64_t* done_sig;  // nullable: see launch_active_list
  const uint64_t* ticket;
  float* outT;
  int src_pair = -1;  // >= 0: bit 31 of host_n says whether this pair (of the group) is still active
};
void tree_prof_dump();  // diagnostic builds (AICP_ITER_PROF): k_tr_mid phase times to stderr
void iter_prof_dump();  // diagnostic builds (AICP_ITER_PROF): per-kernel body / tail times to stderr
inline size_t icp_sync_words(size_t n_pairs) { return 3 * n_pairs + 2; }
// an iteration's IcpIterSync: the sync words laid out for pairs [0, n_pairs) (sel1 | sel2 | red |
// pairs, of whose 2 words the first is used) and the group that iterates, np pairs from pd / st.
// host_n, done_sig / ticket / outT and src_pair are the caller's to set.
IcpIterSync icp_iter_sync(uint32_t* words, size_t n_pairs, int np, const PairDesc* pd, PairState* st, ActiveList* al,
                          uint32_t* ctr);
void launch_icp_select_f(hipStream_t s, BlockMap m, const PairDesc* pd, PairState* st, const float* d2,
                         uint32_t* hist1, uint32_t* cand, uint32_t* cand_cnt, const IcpIterSync& y);
// from the second iteration on: the select in one launch, its compaction on the previous
// iteration's digit-1 bin (same limit; a missed guess is compacted again by the pair's last
// workgroup, counted in PairState::sel_miss)
// the whole select of each pair in one workgroup (batches of many pairs of <= 65536 readings)
void launch_icp_select_pair(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st, const float* d2,
                            uint32_t* cand, const IcpIterSync& y);
// force: aicp_hip_options::select_pair (-1 auto, 0 off, 1 on)
bool sel_pair_fits(size_t n_pairs, uint64_t max_read, int force);
constexpr uint32_t kFinalLds = 8192;  // candidates the final select of a pair copies into LDS
// force_cl (aicp_hip_test_select): 0 = the template by the launch's size, else the candidates the
// final select keeps in LDS, kHistBins or kFinalLds
void launch_icp_select_fused(hipStream_t s, BlockMap m, const PairDesc* pd, PairState* st, const float* d2,
                             uint32_t* hist1, uint32_t* cand, uint32_t* cand_cnt, const IcpIterSync& y,
                             uint32_t force_cl = 0);
// prm.knn_normals == 0: the point-to-point pair of kernels (k_icp_reduce_p2p / k_icp_update_p2p;
// bnrm is not read and may be null), else k_icp_reduce / k_icp_update_f
void launch_icp_reduce_f(hipStream_t s, BlockMap m, const PairDesc* pd, PairState* st, const float4* read_c,
                         const int32_t* match, const float* d2, const uint32_t* touched, const float4* bpts,
                         const float4* bnrm, double* slab, const IcpParams& prm, const IcpIterSync& y);
void launch_icp_nn(hipStream_t s, int grid_items, const PairDesc* pd, const PairState* st,
                   const ActiveList* al, const float4* read_c, const uint4* nodes, const uint4* tl,
                   const int32_t* parent, const float4* bpts, const uint2* ptl, int32_t* match, float* d2,
                   uint32_t* touched, uint32_t* ctr, const IcpParams& prm, hipEvent_t e0 = nullptr,
                   hipEvent_t e1 = nullptr);
// TrimmedDist limit per active pair. m: blocks of kNNBlock * kSelPerThread readings;
// hist1: n_pairs * kHistBins zeroed words, cand: total_read words, cand_cnt: n_pairs zeroed
// words (both left zeroed for the next call).
// m covers pairs p0 .. p0 + n_pairs - 1 (absolute pair indices into pd / st / hist1 / cand_cnt).
void launch_icp_select(hipStream_t s, BlockMap m, int n_pairs, const PairDesc* pd, PairState* st,
                       const float* d2, uint32_t* hist1, uint32_t* cand, uint32_t* cand_cnt, int p0 = 0);
void launch_finalize(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st,
                     float* outT);

// AICP_NN_PROF builds: print and reset the NN kernel's per-phase cycle shares (stderr)
void nn_prof_dump();

// ---- kernel-level entry points ----------------------------------------------------------
bool launch_knn_generic(hipStream_t s, uint32_t nq, const float4* q, const uint4* nodes,
                        const int32_t* parent, const float4* bpts, int k, float maxE2,
                        float maxR2, int32_t* ids, float* d2, unsigned long long* touched,
                        uint32_t* ctr);
void launch_transform(hipStream_t s, int n, const float* T, const float4* in, float4* out);
// kernels_crop.hip: order-preserving oriented box crop (getPointsInOrientedBox).
struct CropBoxArgs {
  float inv[9];  // row-major local-frame rotation (identity when CropBox would skip it)
  float t[3];    // translation subtracted first
  float mn, mx;
};
#ifdef __HIPCC__
// the keep test of every crop kernel and of the sweep accumulator (kernels_accum.hip)
__device__ __forceinline__ bool crop_keep(const CropBoxArgs& a, float4 p) {
  if (!isfinite(p.x) || !isfinite(p.y) || !isfinite(p.z)) return false;
  const float x = __fsub_rn(p.x, a.t[0]), y = __fsub_rn(p.y, a.t[1]), z = __fsub_rn(p.z, a.t[2]);
  float l[3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
    l[r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.inv[3 * r], x), __fmul_rn(a.inv[3 * r + 1], y)),
                               __fmul_rn(a.inv[3 * r + 2], z)),
                     0.f);
  return !(l[0] < a.mn || l[1] < a.mn || l[2] < a.mn || l[0] > a.mx || l[1] > a.mx || l[2] > a.mx);
}
#endif
size_t crop_tiles(size_t n);
void launch_crop_box(hipStream_t s, int n, const float inv[9], const float t[3], float mn, float mx,
                     const float4* pts, uint32_t* tile_cnt, uint32_t* tile_off, uint32_t* total,
                     float4* out);
// the crop's exclusive scan of n_tiles tile counts (one workgroup) and their total, for other
// order-preserving compactions (the FOV filter)
void launch_tile_scan(hipStream_t s, int n_tiles, const uint32_t* cnt, uint32_t* off, uint32_t* total);
// many crops of one map (one per localization reading): args = n_crops packed CropBoxArgs
// (pack_crop_args, crop_args_bytes each); tile_cnt / tile_off: n_crops * crop_tiles(n) words;
// totals: n_crops words. The scatter writes crop c at out + base_of[c], in input order.
size_t crop_args_bytes();
void pack_crop_args(const float inv[9], const float t[3], float mn, float mx, void* dst);
void launch_crop_count_multi(hipStream_t s, int n, int n_crops, const void* args, const float4* pts,
                             uint32_t* tile_cnt, uint32_t* tile_off, uint32_t* totals);
void launch_crop_scatter_multi(hipStream_t s, int n, int n_crops, const void* args, const float4* pts,
                               const uint32_t* tile_off, const uint32_t* base_of, float4* out);
void launch_solve6(hipStream_t s, const double* A, const double* b, double* x, int32_t* path);

// ---- sampled chains (kernels_chain.hip, chain.cpp): data-point filters, MaxDist select -------
constexpr int kChainMaxFilters = 4;  // AICP_CHAIN_MAX_FILTERS
constexpr int kChainMinDist = 2, kChainRandom = 3, kChainMaxDensity = 4;  // AICP_FILTER_*
struct ChainCtl {  // one side's control block on the device
  uint32_t n[kChainMaxFilters + 1];  // points of the cloud as given, then after each filter of the list
  uint32_t max_bits, n_sat;          // MaxDensity: lastDensity (float bits), nbSaturated
  uint32_t degenerate;               // SurfaceNormal's rank-deficient points
};
struct ChainFilterArgs {
  int32_t kind, pos;  // pos: the filter's position in its list (it receives ctl->n[pos] points)
  int32_t dim;
  float min_dist, prob, max_density;
  uint32_t slot;      // of the draw: 4 * side + pos
  uint32_t pad;
  uint64_t seed;
};
size_t chain_tiles(size_t n);
// pts[i].w = i for the n uploaded points; ctl = {n, 0, ...}
void launch_chain_begin(hipStream_t s, uint32_t n, float4* pts, ChainCtl* ctl);
// a filter that keeps every point (SurfaceNormal): ctl->n[pos + 1] = ctl->n[pos]; st (nullable):
// the state launch_normals counted the degenerate points in
void launch_chain_pass(hipStream_t s, int pos, ChainCtl* ctl, const PairState* st);
// One MinDist / RandomSampling / MaxDensity filter on the ctl->n[a.pos] rows of pts: the kept rows
// to out in input order, with their normals and densities (carried where nrm_out / dens_out is
// given, from nrm / dens; dens alone serves the MaxDensity's own test), the kept count to
// ctl->n[a.pos + 1]. cap: the points of the cloud as given (sizes every array; flag: cap bytes;
// tile_cnt / tile_off: chain_tiles(cap) words). MaxDensity reads dens.
void launch_chain_filter(hipStream_t s, uint32_t cap, const ChainFilterArgs& a, ChainCtl* ctl, uint8_t* flag,
                         uint32_t* tile_cnt, uint32_t* tile_off, const float4* pts, float4* out, const float4* nrm,
                         float4* nrm_out, const float* dens, float* dens_out);
// SurfaceNormal's outputs of an n-point cloud's raw tree (bpts; ids: launch_knn_ids / launch_normals;
// bnrm: launch_normals, read only with nrm) into the cloud's order: nrm, dens (each nullable)
bool launch_chain_sn_out(hipStream_t s, uint32_t n, int knn, const float4* bpts, const int32_t* ids, const float4* bnrm,
                         float4* nrm, float* dens);
// bnrm[j] = given[ref_off + input id of bpts[j]] for the n points of the n_refs matcher trees (rd:
// their descriptors, ascending ref_off; given: each reference's normals at its ref_off)
void launch_chain_gather_normals(hipStream_t s, int n_refs, const PairDesc* rd, uint32_t n, const float4* bpts,
                                 const float4* given, float4* bnrm);
// out[i] = (x, y, z, 1) of in[i]: filtered rows as upload_pairs stores a cloud
void launch_chain_rows(hipStream_t s, uint32_t n, const float4* in, float4* out);
// MaxDistOutlierFilter: st[p].limit = limit_d2 for the active pairs (the trimmed select's output)
void launch_chain_select_maxdist(hipStream_t s, int n_pairs, PairState* st, float limit_d2);
// The batch form: one side's clouds concatenated. Cloud c holds n[q] rows at off[q] of the side's
// buffers at stage q (as given, then after each filter); the clouds follow each other without gaps.
struct ChainCloud {
  uint32_t n[kChainMaxFilters + 1], off[kChainMaxFilters + 1];
  uint32_t max_bits, n_sat;  // MaxDensity: the cloud's own lastDensity (float bits) and nbSaturated
  uint32_t degenerate;       // SurfaceNormal's rank-deficient points of the cloud
  int32_t sn_slot;           // the cloud's tree among those SurfaceNormal built (-1: it had no point)
  uint32_t pad[2];
};
struct ChainSeg {  // launch_chainb_rows: n rows from src to dst
  uint32_t dst, src, n, pad;
};
// cl: n[0] / off[0] set by the host, the rest zero. Row i of cloud c from src[src_off[c] + i] (the
// clouds where an upload left them) to pts[off[0] + i], w = i; ctl = {total, 0, ...}
void launch_chainb_begin(hipStream_t s, int n_clouds, const ChainCloud* cl, uint32_t total, const float4* src,
                         const uint32_t* src_off, float4* pts, ChainCtl* ctl);
void launch_chainb_pass(hipStream_t s, int pos, int n_clouds, ChainCloud* cl, ChainCtl* ctl, const PairState* st);
// launch_chain_filter over the concatenation: every cloud filtered by its own indices, counts and
// MaxDensity maximum; cl[c].n / off [a.pos + 1] and ctl->n[a.pos + 1] (the total) written. cap: the
// side's rows as given.
void launch_chainb_filter(hipStream_t s, uint32_t cap, const ChainFilterArgs& a, int n_clouds, ChainCloud* cl,
                          ChainCtl* ctl, uint8_t* flag, uint32_t* tile_cnt, uint32_t* tile_off, const float4* pts,
                          float4* out, const float4* nrm, float4* nrm_out, const float* dens, float* dens_out);
// launch_chain_sn_out over n_trees raw trees (pd: ref_off / n_ref, ascending, tiling [0, total))
bool launch_chainb_sn_out(hipStream_t s, int n_trees, const PairDesc* pd, uint32_t total, int knn, const float4* bpts,
                          const int32_t* ids, const float4* bnrm, float4* nrm, float* dens);
// launch_chain_rows over segments (ascending dst, tiling [0, total)); nrm -> nrm_out beside (nullable)
void launch_chainb_rows(hipStream_t s, int n_segs, const ChainSeg* sg, uint32_t total, const float4* in, float4* out,
                        const float4* nrm, float4* nrm_out);

// ---- sweep accumulator (kernels_accum.hip): VelodyneAccumulatorROS::processLidar ---------------
struct AccumSweep {
  CropBoxArgs box;  // identity frame, crop_min / crop_max (velodyne_accumulator.cpp:59-60)
  float T[16];      // the sweep's pose as transformPointCloud takes it (aicp_hip_accum_pose_matrix)
};
// Sweep j of a reading, two launches: the rows that pass the box (n rows of `stride` bytes on the
// device, 12 or 16, xyz first) are moved by T and appended in input order as float4(x, y, z, 1) at
// out + tails[j]; tails[j + 1] = tails[j] + kept. tile_cnt: crop_tiles(n) words; no write at or past
// out + cap. n = 0 still writes tails[j + 1].
void launch_accum_sweep(hipStream_t s, int n, const void* rows, size_t stride, const AccumSweep& a, uint32_t* tile_cnt,
                        uint32_t* tails, int j, float4* out, uint32_t cap);

// ---- kd-tree construction (kernels_tree.hip) ---------------------------------------------
struct TreeWork {
  float4* W[2];          // points being partitioned (ping-pong), total
  int32_t* segof[2];     // segment of each position at the current / next level, total
  TreeSeg* seg[2];       // segments of the current / next level, max_seg
  uint32_t* flag;        // total + 2
  uint32_t* X1;          // scans, total + 2
  uint32_t* X2;
  uint32_t* posL;        // partner positions, total
  uint32_t* posR;
  NodeEvent* ev;         // 2 * total slots (leaf: first position; inner: total + split position)
  uint8_t* valid;        // 2 * total
  SubSeg* subs;          // wave-subtree segments, max_seg
  SubSeg* mids;          // mid-size segments (kSubMax < count <= kMidMax), max_seg
  uint32_t* ecnt;        // nodes ending at each position, total + 2
  uint64_t* sums;        // 6 per pair (128-bit fixed-point coordinate sums), then 6 per tree_sum_tiles tile
  int32_t* pair_depth;   // per pair
  TreeCtl* ctl;
  void* scan_temp;
  size_t scan_temp_bytes;
  size_t max_seg;
  int n_pairs;
  uint64_t* lb;          // look-back words of the build's scans (lb_bytes), zeroed by launch_tree_prepare
  size_t lb_stride;      // words per scan
  uint32_t mid_max;      // segments up to this size leave the global levels (kMidMax; kSubMax: no mid builder)
  uint32_t lvl_min;      // the level-synchronous subtree builder from this many points (aicp_hip_options)
};
uint32_t tree_mid_max();
hipError_t set_lb_force_stall(int on);  // aicp_hip_test_force_scan_stall
size_t tree_sum_tiles(size_t n);  // k_tr_sum's tiles over n points
size_t tree_scan_temp_bytes(size_t n);
size_t lb_bytes(uint32_t total);
size_t lb_stride_words(uint32_t total);
// centroid (center = 1) + frames in pd, centred points, root segments
// matcher treelets of n_refs trees (rd[r].tl_off / tl_cap set by the host) of the build w (its
// look-back words and control block; cap = 2 * its points + 2): rank: cap + 1 words; errors into
// w.ctl->error (bit 4)
hipError_t launch_treelets(hipStream_t s, int n_refs, uint32_t cap, const PairDesc* rd, const uint4* nodes,
                           int bucket, uint32_t* rank, uint4* tl, uint2* link, const TreeWork& w);
// part 1: only what does not read the points (zeroed work space; frames when center = 0); part 2:
// the rest; 0: all
hipError_t launch_tree_prepare(hipStream_t s, int n_pairs, uint32_t total, PairDesc* pd, const float4* raw,
                               int center, const TreeWork& w, float4* bpts, int bucket, int part = 0);
// one level: nodes at depth `level` are split (their children get depth level + 1)
// last: the final planned level -- children above kSubMax points also go to the subtree
// kernel (its global-memory path) instead of a next level
hipError_t launch_tree_level(hipStream_t s, int level, uint32_t total, const TreeWork& w, float4* bpts,
                             int bucket, bool last);
// mid-size segments, one workgroup each: nodes split in LDS until the pieces fit the subtree builders
hipError_t launch_tree_mid(hipStream_t s, uint32_t total, const TreeWork& w, float4* bpts, int bucket);
// subtrees of the segments with <= kSubMax points, one wave each (grid-stride over the device count)
hipError_t launch_tree_subtrees(hipStream_t s, uint32_t total, const TreeWork& w, float4* bpts,
                                int bucket);
// node records (preorder) and PairDesc node_off / n_nodes / tree_depth
hipError_t launch_tree_finish(hipStream_t s, int n_pairs, uint32_t total, PairDesc* pd, const TreeWork& w,
                              uint4* nodes);

// pairs -> their shared reference's centroid / tree fields (+ T_refMean_dataIn), and its
// SurfaceNormal degenerate count
void launch_pairs_from_refs(hipStream_t s, int n_pairs, PairDesc* pd, const PairDesc* rd);
// normals of the raw-coordinate tree's bucket order -> bnrm in the matcher tree's order
void launch_normals_to_matcher(hipStream_t s, int n_refs, uint32_t total, const PairDesc* rd, const float4* bpts,
                               const float4* bpts_raw, const float4* nrm_raw, uint32_t* inv, float4* bnrm);
void launch_pairs_degenerate(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st, const PairState* rst);
void launch_pairs_degenerate_part(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st, const PairState* rst,
                                  int what);

// ---- overlap ------------------------------------------------------------------------------
// Clouds: the reference side runs over overlap groups (one per distinct reference cloud and
// origin; pd = group descriptors, st = group states), the reading side over pairs.
// sides: 1 = reference origin, 2 = reading origin
void launch_ovl_init(hipStream_t s, int n, const PairDesc* pd, PairState* st, double res, int sides);
void launch_ovl_bbox(hipStream_t s, BlockMap m, const PairDesc* pd, PairState* st,
                     const float4* pts, int side, double res);
// od[i]: the map of entry i (group or pair) of the side being marked; one workgroup per block of m
void launch_ovl_mark(hipStream_t s, BlockMap m, const PairDesc* pd, const OvlDesc* od, PairState* st,
                     const float4* pts, int side, double res, uint8_t* maps, bool filter);
// |A| per group (gst.ovl_counts[0]), |B| and |A∩B| per pair (st.ovl_counts[1], [2])
void launch_ovl_count(hipStream_t s, int n_pairs, int n_groups, const PairDesc* pd, const OvlDesc* od_read,
                      const OvlDesc* od_ref, PairState* st, PairState* gst, const uint8_t* maps, bool wide);
// the parts of launch_ovl_count: |S| of n maps into st[i].ovl_counts[slot]; |A∩B| per pair
// wide: many workgroups per map (the one-shot call of a single pair)
void launch_ovl_popcount(hipStream_t s, int n, const OvlDesc* od, PairState* st, int slot, const uint8_t* maps,
                         bool wide = false);
void launch_ovl_intersect(hipStream_t s, int n_pairs, const PairDesc* pd, const OvlDesc* od_read, const OvlDesc* od_ref,
                          PairState* st, const uint8_t* maps, bool wide = false);
void launch_ovl_finish(hipStream_t s, int n_pairs, const PairDesc* pd, PairState* st, const PairState* gst,
                       int set_ratio);

// ---- sparse overlap (kernels_overlap_sparse.hip): sorted key words instead of voxel maps -------
// One side of an overlap as a key list of `cap` words: the batch's groups then readings (cap = the
// exact key total, read back between the two halves below), or a stream window's readings or its
// reference (cap = a host bound of the keys, no read-back; the tail is padding).
struct OvlKeySide {
  OvlCloud* clouds;            // n_clouds (device)
  int n_clouds;
  const uint32_t* blk_cloud;   // n_blocks blocks of 256 points
  const uint32_t* blk_start;
  uint32_t n_blocks;
  uint32_t n_points;           // count slots (clouds[c].slot + j)
  uint32_t* cnt;               // n_points
  uint64_t* off;               // n_points
  uint64_t cap;
  uint64_t* keys0;             // cap each
  uint64_t* keys1;             // sorted
  void* temp;                  // ovl_keys_temp_bytes
  size_t temp_bytes;
  unsigned long long* per_cloud;  // n_clouds
};
size_t ovl_keys_temp_bytes(size_t n_points, size_t cap, int n_clouds);
// first half: per point key counts (cnt) and their exclusive prefix (off); the points of cloud c
// at (clouds[c].side ? read : ref) + clouds[c].pts_off. origin0 (nullable, 3 device doubles):
// clouds[0].origin := origin0 first. Uses cnt, off, temp; cap and the key arrays not yet.
hipError_t launch_ovl_keys_count(hipStream_t s, const OvlKeySide& k, const double* origin0, const float4* ref,
                                 const float4* read, double res);
// second half: the words, sorted, and |S_c| in k.per_cloud. With st: the words past the true total
// are padded, a cloud whose keys exceed cap reports st[c].ovl_err, and |S_c| goes to
// st[c].ovl_counts[slot] (slot 0 or 1). Without (the batch): cap is the exact total, so there is
// nothing to pad or report, and launch_ovl_keys_intersect writes the counts.
hipError_t launch_ovl_keys_sets(hipStream_t s, const OvlKeySide& k, const float4* ref, const float4* read,
                                double res, PairState* st, int slot);
// both halves in a row (the stream: every cloud of the side in pts)
hipError_t launch_ovl_keys(hipStream_t s, const OvlKeySide& k, const double* origin0, const float4* pts,
                           double res, PairState* st, int slot);
// |A ∩ B| of the readings of rd (its clouds from first_read on) against their groups in ref's list
// into st[p].ovl_counts[2]: group pd[p].ogroup, or cloud 0 without pd. With gst (the batch, rd and
// ref the same side): also |S| of the groups into gst[g].ovl_counts[0] and of the readings into
// st[p].ovl_counts[1], in the same launch.
hipError_t launch_ovl_keys_intersect(hipStream_t s, const OvlKeySide& rd, const OvlKeySide& ref, int first_read,
                                     const PairDesc* pd, unsigned long long* per_pair, PairState* gst,
                                     PairState* st);

// ---- frame-to-reference stream (kernels_sequence.hip) ---------------------------------------
// gd->ref_origin = translation of fromMatrix4fToIsometry3d(T) * prior pose of src (1 thread);
// T (src's correction, written by another stream's kernel) is copied to Tcopy for the transform
// that follows on the same stream
// the next reference: its origin into gd, Tcopy = T, out = T * in (k_transform's arithmetic);
// src_st (nullable): T from the source's state and frames instead (k_finalize's product)
void launch_seq_ref_points(hipStream_t s, int n, PairDesc* gd, const PairDesc* src, const PairState* src_st,
                           const float* T, float* Tcopy, const float4* in, float4* out);
// the window's descriptors, states and corrections into the sequence's arrays (np readings)
void launch_seq_commit(hipStream_t s, int np, const PairDesc* d, const PairState* st, const float* T, PairDesc* gd,
                       PairState* gst, float* gT);
// a[0, na), b[0, nb), c[0, nc) = 0 in one launch
void launch_zero_words3(hipStream_t s, uint32_t* a, size_t na, uint32_t* b, size_t nb, uint32_t* c, size_t nc);
// debug working mode (app.cpp:87-96, 414), one thread each: hist := initT, d's prior origin :=
// translation of initT * prior pose; then outT := d's correction and, if it is accepted,
// initT := correction * initT
void launch_debug_prep(hipStream_t s, PairDesc* d, const float* initT, float* hist);
void launch_debug_post(hipStream_t s, const PairDesc* d, PairState* st, float* outT, float* initT, float max_corr);
// od[i] (min, dim, bytes) from st[i].ovl_bbox; od[i].off preset; bytes > cap[i]: ovl_err, empty map
void launch_ovl_size(hipStream_t s, int n, PairState* st, OvlDesc* od, const uint64_t* cap);
// zero the n maps of od[] (device-side sizes, each at most max_bytes)
void launch_ovl_clear(hipStream_t s, int n, const OvlDesc* od, uint8_t* maps, uint64_t max_bytes);

// ---- App's map localization streams (kernels_map_stream.hip, map_stream.cpp) -----------------
// One window-stream serves the prior map (aicp_hip_map_sequence_run) and the map App builds
// itself (aicp_hip_built_map_sequence_run); `built` selects the rules of the second.
struct StreamState {    // the stream's state on the device
  float initT[16];      // initialT_ (app.cpp:414), column-major
  int32_t count;        // prior map: aligned_clouds_graph_->getNbClouds(); built map: readings
                        // accepted since the last reference (app.cpp:383-391)
  int32_t pad[3];
};
struct StreamRules {    // the stream's parameters as the commit kernel reads them
  int32_t built;        // 0: prior map, 1: built map
  int32_t freq;         // reference_update_frequency
  int32_t refilter_every;  // prior map: map_refilter_every (0: never)
  int32_t merge;        // prior map: AICP_LOC_MERGE
  int32_t overlap;      // built map: the batch ran the overlap, an overlap error fails the reading
  float max_corr;
};
struct StreamRec {      // one reading's decisions (the host reads a window's records once)
  int32_t status;       // AICP_* of its registration; -1: after the reading that ended the stream
  int32_t accepted;
  int32_t append;       // the reading goes to the map's tail (merged / is_reference)
  int32_t refilter;     // the map is pre-filtered after this reading (prior map)
  double corrected_origin[3];
};
// debug working mode (app.cpp:87-96): pts := initialT_ * pts in place (k_transform's expression)
// and origin := translation of initialT_ * prior pose (k_debug_prep's)
// (initT: 16 floats on the device, StreamState::initT)
void launch_loc_move(hipStream_t s, int n, const float* initT, double* origin, float4* pts);
// a raw reading's rows (n rows of `stride` bytes on the device, 16-byte aligned, stride >= 12 and a
// multiple of 4) -> out[i] = float4(x, y, z, 1); initT (nullable, 16 floats on the device): each
// point moved by it (k_transform's expression) and, with origin (nullable), origin := translation
// of initT * prior pose (k_loc_move's)
void launch_stream_ingest(hipStream_t s, int n, const void* rows, size_t stride, const float* initT, double* origin,
                          float4* out);
// one thread walks the window's np readings in order (app.cpp:366-391, 414, 469-493): status, drop
// test, count, corrected origin, initialT_ = correction * initialT_, append / re-filter flags
void launch_stream_commit(hipStream_t s, int np, const PairState* st, const float* T, const double* origin,
                          StreamRules r, StreamState* S, StreamRec* rec);

// ---- live App session (kernels_session.hip, session.cpp) --------------------------------------
struct SessionHeader {  // what describes the session's current reference, beside its points
  uint32_t count;       // points
  int32_t id;           // the process call whose reading it is (-1: the first cloud)
  int32_t pad[2];
  double origin[3];     // its sensor origin (corrected_origin of that reading)
  double pad2;
};
// Behind launch_stream_commit of one reading (np = 1), no host decision in between: if rec->append,
// ref[i] = apply4(T, read[i]) for the n points of the reading as registered (k_transform's
// expression) and hdr = {n, id, rec->corrected_origin}; otherwise nothing is written.
void launch_session_promote(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read, int32_t id,
                            float4* ref, SessionHeader* hdr);
// The live map sessions' append (map_stream.cpp), behind launch_stream_commit of one reading in the
// same way: if rec->append, dst[i] = apply4(T, read[i]) for the n points of the reading as
// registered; otherwise nothing is written. dst: the map's tail, with room for n points.
void launch_session_map_append(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read,
                               float4* dst);
// The risk gate's record in device memory (failure_prediction_mode): the classifier's sample, then
// what k_svm_predict writes for it
struct GateRec {
  float overlap, alignability;
  float raw, ratio;
  double risk;
  int32_t gate, pad;
};
// The gated branch of processCloud (app.cpp:401-411) in the live session, right behind
// launch_svm_predict with no host decision in between. gate->gate == 0: rec->append = 0, nothing
// else. Otherwise the reading as it was filtered is the next reference, unmoved: ref[i] = read[i]
// for its n points (the bytes, not apply4 by the identity), rec = {status 0, accepted 1, append 1,
// corrected_origin = origin (the reading's prior origin, moved in debug mode)}, T = identity,
// S->count = 0 (S->initT stays), hdr = {n, id, origin}.
void launch_session_gate_promote(hipStream_t s, int n, const GateRec* gate, const double* origin, const float4* read,
                                 int32_t id, float4* ref, float* T, StreamState* S, StreamRec* rec,
                                 SessionHeader* hdr);
// launch_session_promote / launch_session_gate_promote for a session that keeps aligned_map_
// (aicp_hip_session_keep_aligned_map; app.cpp:458-468): what they write, and the same n points
// also to dst[i], the map's tail with room for n points; nothing more when nothing is promoted.
void launch_session_promote_map(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read,
                                int32_t id, float4* ref, float4* dst, SessionHeader* hdr);
void launch_session_gate_promote_map(hipStream_t s, int n, const GateRec* gate, const double* origin,
                                     const float4* read, int32_t id, float4* ref, float4* dst, float* T, StreamState* S,
                                     StreamRec* rec, SessionHeader* hdr);
// The gated branch in the live map sessions (aicp_hip_mapsession_create_risk), right behind
// launch_svm_predict in the same way (n > 0: the reading's kept points). gate->gate == 0:
// rec->append = 0, nothing else. Otherwise T = identity, rec = {status 0, accepted 1,
// corrected_origin = origin}, S->initT stays, and
//   r.built: dst[i] = read[i] for the reading's n points (the bytes; dst: the map's tail, with room
//     for n points), rec->append = 1, rec->refilter = 0, S->count = 0;
//   prior map (one block, read / dst not used): c = ++S->count, rec->append = 0, rec->refilter =
//     r.merge && r.refilter_every > 0 && (c - 1) % r.refilter_every == 0.
void launch_session_map_gate(hipStream_t s, int n, const StreamRules& r, const GateRec* gate, const double* origin,
                             const float4* read, float4* dst, float* T, StreamState* S, StreamRec* rec);

// ---- pre-filter (kernels_prefilter.hip): regionGrowingUniformPlaneSegmentationFilter -------
constexpr int kPfMaxNbrs = 16;  // RegionGrowing neighbours per point (edge mask bits)
struct PfCtl {                  // device control block; lo = 0xFFFFFFFF, everything else 0 at start
  uint32_t lo[3], hi[3];        // order-preserving bits of the finite points' min / max
  uint32_t n_fin, n_bad;        // finite / non-finite input points
  int32_t minb[3];              // VoxelGrid min_b_
  uint32_t mul1, mul2;          // divb_mul_[1], divb_mul_[2]
  float inv;                    // inverse leaf size
  uint32_t passthrough;         // PCL's integer-overflow guard fired: the cloud passes unfiltered
  uint32_t n_vox;               // sampled points V
  uint32_t n_inf;               // points left for k_rg_phaseb
  uint32_t n_seg, n_clusters, n_out;
};
struct PfWork {  // scratch, n (+1) words each
  uint32_t *k0, *k1, *v0, *v1, *flag, *scan, *keep, *kpts, *koff;
  void* temp;
  size_t temp_bytes;
};
size_t pf_temp_bytes(size_t n);
// VoxelGrid: ctl->n_vox centroids into sampled (ascending voxel index)
hipError_t launch_pf_voxel(hipStream_t s, uint32_t n, const float4* pts, float inv, PfCtl* ctl, const PfWork& w,
                           float4* sampled);
// NormalEstimation from the kNN of the sampled tree (bucket order); k in {10, 20, 30}
// ids: launch_knn_ids output (bucket positions)
bool launch_pf_normals(hipStream_t s, uint32_t V, int k, int nnb, const float4* bpts, const float4* sampled,
                       const int32_t* ids, uint32_t* inv, const float vp[3], float4* nrm, int32_t* nbp, uint2* kth,
                       uint32_t* ckey, uint32_t* cval);
// seed order, edge masks and initial labels
hipError_t launch_pf_order(hipStream_t s, uint32_t V, int nnb, const PfWork& w, const uint32_t* ckey,
                           const uint32_t* cval, const uint32_t* inv, const float4* bpts, const float4* nrm,
                           const int32_t* nbp, const uint2* kth, float cos_thr, float curv_thr, uint32_t* nob,
                           uint32_t* order_of, uint32_t* em, uint32_t* label);
// union-find over mutual edges (marked in em bits 17..): comp[x] = component root, roots start at their members' minimum
void launch_rg_components(hipStream_t s, uint32_t V, int nnb, const int32_t* nbp, uint32_t* em, uint32_t* comp,
                          uint32_t* label);
void launch_rg_iter(hipStream_t s, uint32_t V, int nnb, const int32_t* nbp, const uint32_t* em, const uint32_t* nob,
                    const uint32_t* comp, uint32_t* label, uint32_t* changed);
void launch_rg_settle(hipStream_t s, uint32_t V, const uint32_t* comp, uint32_t* label);
void launch_rg_count_inf(hipStream_t s, uint32_t V, const uint32_t* label, PfCtl* ctl);
void launch_rg_phaseb(hipStream_t s, uint32_t V, int nnb, const int32_t* nbp, const uint32_t* em, const uint32_t* nob,
                      uint32_t* label);
// clusters of min..max points: out (creation order, ascending index), cluster of every point
hipError_t launch_rg_extract(hipStream_t s, uint32_t V, uint32_t min_size, uint32_t max_size, const uint32_t* label,
                             const uint32_t* inv, const float4* sampled, const PfWork& w, float4* out,
                             int32_t* cluster_of, PfCtl* ctl);

// ---- alignment-risk features (kernels_risk.hip): overlapFilter, alignabilityFilter ----------
struct FovArgs {
  double pinv[12];  // inverse of the other cloud's pose, rows of 3 x 4 (host, double)
  float R[9];       // that pose as float (row-major) and its translation: kept points go back
  float t[3];
  double thresh;    // |theta| bound (degrees), range (metres)
  double range;
};
struct RiskBox {  // a cluster's box as CropBox sees it
  float inv[9];   // row-major local-frame rotation
  float t[3];     // box position
  float half[3];  // min = -half, max = half
  float pad;
};
struct RiskCluster {
  double sum_p[3], sum_n[3], sum_nn[6];  // fp64 sums in the fixed order (xx, xy, xz, yy, yz, zz)
  double centre[3], rot[9], half[3];     // getOBB after overlapBoxFilter's scaling; rot row-major, columns = axes
  RiskBox box;
  uint32_t count, pad;
  // between the cluster kernels: mean (relative to p0) and axes as rows, the cluster's first
  // point, order-preserving bits of the extents' min[3], max[3]
  double frame[12], p0[3];
  unsigned long long ext[6];
};
struct RiskOut {
  double eigenvalues[3];   // normalised, descending
  double eigenvectors[9];  // row-major, column k belongs to eigenvalue k
  double centroid[3];      // of the matched planes of cloud A
  float alignability;
  int32_t n_matches;
};
size_t fov_tiles(size_t n);
// kept points (input order, back in the global frame) to out (capacity n); tile_cnt / tile_off:
// fov_tiles(n) words
void launch_fov_filter(hipStream_t s, uint32_t n, const FovArgs& a, const float4* pts, uint32_t* tile_cnt,
                       uint32_t* tile_off, uint32_t* total, float4* out);
// pf_core's results -> s8 = {x, y, z, curvature, nx, ny, nz, 0} per sampled point, lab = its cluster
void launch_risk_gather(hipStream_t s, uint32_t V, const float4* sampled, const float4* nrm, const uint32_t* inv,
                        const int32_t* cluster_of, float* s8, int32_t* lab);
size_t risk_sort_temp_bytes(size_t n);
size_t risk_partial_bytes(size_t V, size_t nc);
// per cluster c in [0, nc): moments, box. k0, k1, v0, idx: V words; seg: nc + 1 words; partial:
// risk_partial_bytes(V, nc)
hipError_t launch_risk_clusters(hipStream_t s, uint32_t V, uint32_t nc, const float* s8, const int32_t* lab,
                                uint32_t* k0, uint32_t* k1, uint32_t* v0, uint32_t* idx, uint32_t* seg, void* temp,
                                size_t temp_bytes, double* partial, const float scale[3], RiskCluster* out);
// cnt[box_of_Y * ncx + label_of_X_point] += 1 (cnt zeroed by the caller)
void launch_risk_counts(hipStream_t s, uint32_t V, uint32_t ncx, uint32_t ncy, const float* s8, const int32_t* lab,
                        const RiskCluster* boxes, uint32_t* cnt);
// a_in_b: [ncb][nca], b_in_a: [nca][ncb]; best_*: nca, m_*: ncb
void launch_risk_match(hipStream_t s, uint32_t nca, uint32_t ncb, const RiskCluster* ca, const RiskCluster* cb,
                       const uint32_t* a_in_b, const uint32_t* b_in_a, float max_angle, int32_t* best_j,
                       float* best_ov, float* best_d, int32_t* m_idx, float* m_ov, float* m_dist, RiskOut* out);

// ---- the failure-prediction classifier (kernels_svm.hip): svm.cpp's SVM and App's gate ---------
struct SvmEntry {  // one decision-function entry: its support vector (by the file's index), its alpha
  float v0, v1;
  double alpha;
};
struct SvmParams {
  double degree, gamma, coef0, rho;
  double threshold;  // the gate's (read only when a gate is written)
  uint32_t count;    // entries (<= kSvmMaxEntries: staged in LDS)
  uint32_t pad;
};
// sample i = samples[2 i], samples[2 i + 1] (device memory): raw (nullable), risk; gate and ratio
// (nullable): !(risk <= threshold) and autotune_ratio_fast(samples[2 i])
void launch_svm_predict(hipStream_t s, uint32_t n, const SvmParams& prm, const SvmEntry* entries,
                        const float* samples, float* raw, double* risk, int32_t* gate, float* ratio);

// ---- registration quality monitor (kernels_monitor.hip): icpMonitor.cpp's metrics -------------
struct MonSeg {       // one tree/query segment of a 1-NN launch (32 bytes)
  uint32_t slot_off;  // its first slot in the launch's slot space (whole 64-slot chunks per segment)
  uint32_t nq;        // queries
  uint32_t q_off;     // the first of them in the point array
  uint32_t tree;      // descriptor of its tree (node_off, ref_off)
  uint32_t d2_off;    // where its squared distances go
  uint32_t pad[3];
};
// d2 of every segment's queries in its tree (libnabo order, 1-NN, node records); ctr:
// kPersistCtrWords zeroed words. The kernel is in kernels_icp.hip, beside the other searches.
void launch_mon_nn(hipStream_t s, uint32_t slots, const MonSeg* segs, const uint32_t* chunk_seg, const PairDesc* trees,
                   const float4* q, const uint4* nodes, const float4* bpts, float maxE2, float maxR2, float* d2,
                   uint32_t* ctr);
constexpr uint32_t kMonChunk = 16 * 256;  // values per workgroup of the reduction: 16 slabs of 256
struct MonRed {       // one segment of squared distances of the reduction
  uint32_t d2_off, n;
  uint32_t slot0;     // its first chunk slot (partial sums; the slots of a segment are consecutive)
  int32_t lim;        // select state whose limit gates the kept count and sum (paired mean); -1: none
  int32_t knn;        // 1: distancesKNN's valid count and sum
  uint32_t acc;       // its accumulator
  uint32_t pad[2];
};
struct MonAcc {       // integer tallies of a segment (zero at the start): order-free
  uint32_t max_bits;  // the largest finite d2, as the bits of a non-negative float
  uint32_t pad;
  unsigned long long n_valid, kept;
};
struct MonPair {      // where one pair's result comes from
  int32_t red[3];     // reduction segments: out -> ref, ref -> out, paired (-1: none; may be red[0])
  int32_t sel_q[2];   // quantile selects of the two directions
  int32_t sel_p;      // paired select (-1: none)
  int32_t pad[2];
};
struct MonOut {       // aicp_monitor_result's layout (include/aicp_hip.h)
  float hausdorff, hausdorff_quantile;
  float max_d2[2], quantile_d2[2];
  float knn_mean_dist;
  int32_t pad;
  uint64_t knn_valid;
  float paired_mean_dist, paired_limit_d2;
  uint64_t paired_kept;
};
// out cloud i (xf[i] = first point, count) = T[16 i ..] * itself, in k_transform's arithmetic
void launch_mon_transform(hipStream_t s, BlockMap m, const uint2* xf, const float* T, float4* pts);
// pts[0 .. n_ref) = ref, pts[n_ref + j] = T * read[j] (T: 16 floats in device memory, column-major;
// k_transform's arithmetic, w = 1) for j < n_read; n_ref + n_read < 2^32, pts aliases neither input
void launch_mon_stage(hipStream_t s, uint32_t n_ref, uint32_t n_read, const float4* ref, const float4* read,
                      const float* T, float4* pts);
// behind a planned tree build on s (ctl: its control block on the device): if the build left an
// error, segments a[0 .. na) and b[0 .. nb) lose their queries and the 1-NN launches search nothing
void launch_mon_guard(hipStream_t s, const TreeCtl* ctl, MonSeg* a, int na, MonSeg* b, int nb);
// partial[2 slot], [2 slot + 1]: the chunk's sums of sqrt(d2) over the valid / the kept values;
// dist (nullable): sqrt(d2) of every value, at d2's index
void launch_mon_reduce(hipStream_t s, BlockMap m, const MonRed* red, const float* d2, const PairState* lim_st,
                       double max_accepted, MonAcc* acc, double* partial, float* dist);
void launch_mon_finish(hipStream_t s, int n_pairs, const MonPair* mp, const MonRed* red, const MonAcc* acc,
                       const double* partial, const PairState* sel_q, const PairState* sel_p, MonOut* out);

}  // namespace aicp
