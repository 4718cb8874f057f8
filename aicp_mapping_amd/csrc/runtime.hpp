// runtime.hpp — host-side runtime shared by the C-ABI translation units (aicp_hip.cpp, sequence.cpp,
// overlap.cpp, map_stream.cpp, session.cpp, accum.cpp, monitor.cpp, test_entries.cpp):
// device / pinned buffers, kd-tree work space, the context and batch objects, error macros.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "kernels.hpp"

namespace aicp {
namespace rt {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

inline hipError_t ensure(DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return hipSuccess;
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  const size_t nb = std::max<size_t>(256, bytes + bytes / 4);
  const hipError_t e = hipMalloc(&b.p, nb);
  if (e == hipSuccess) b.cap = nb;
  return e;
}
inline hipError_t ensure(PinBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return hipSuccess;
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
  const size_t nb = std::max<size_t>(256, bytes + bytes / 4);
  const hipError_t e = hipHostMalloc(&b.p, nb, hipHostMallocDefault);
  if (e == hipSuccess) b.cap = nb;
  return e;
}
inline void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}
inline void release(PinBuf& b) {
  if (b.p) (void)hipHostFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// A fixed pool of host threads for packing (spawning 16 threads per call costs more than the
// packing of a C2 cloud: the stream's windows and the one-shot calls of a context share one).
class WorkerPool {
 public:
  explicit WorkerPool(unsigned n) {
    for (unsigned i = 0; i < n; ++i) th_.emplace_back([this] { loop(); });
  }
  ~WorkerPool() {
    {
      std::lock_guard<std::mutex> l(mu_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }
  // fn(task) for task in [0, n), on the pool and the calling thread; returns when all are done
  // and no worker is inside the task loop any more (so the next run() may reset the counter)
  void run(size_t n, const std::function<void(size_t)>& fn) {
    if (n == 0) return;
    {
      std::lock_guard<std::mutex> l(mu_);
      fn_ = &fn;
      n_ = n;
      next_.store(0);
      done_ = 0;
      ++gen_;
    }
    cv_.notify_all();
    work();
    std::unique_lock<std::mutex> l(mu_);
    done_cv_.wait(l, [&] { return done_ == n_ && active_ == 0; });
    fn_ = nullptr;
  }

 private:
  void work() {
    for (;;) {
      const size_t i = next_.fetch_add(1);
      if (i >= n_) return;
      (*fn_)(i);
      std::lock_guard<std::mutex> l(mu_);
      if (++done_ == n_) done_cv_.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return stop_ || (gen_ != seen && fn_ != nullptr); });
        if (stop_) return;
        seen = gen_;
        ++active_;
      }
      work();
      std::lock_guard<std::mutex> l(mu_);
      if (--active_ == 0 && done_ == n_) done_cv_.notify_all();
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_, done_cv_;
  const std::function<void(size_t)>* fn_ = nullptr;
  size_t n_ = 0, done_ = 0;
  int active_ = 0;
  std::atomic<size_t> next_{0};
  uint64_t gen_ = 0;
  bool stop_ = false;
};

// Work space of one kd-tree construction (kernels_tree.hip). Two sets: the raw-coordinate
// tree (SurfaceNormal) and the centred matcher tree are built concurrently on two streams.
struct TreeBufs {
  DevBuf W0, W1, segof0, segof1, seg0, seg1, flag, X1, X2, posL, posR, ev, valid, subs, mids, ecnt, sums, pdepth,
      ctl, scan, lb;
  PinBuf pin_ctl;
  TreeWork tw{};    // device_trees_begin -> device_trees_end
  int planned = 0;  // global levels enqueued without host polling (0: polled build)
  int needed = 0;   // global levels the last planned build actually used
  uint32_t lvl_min = 1u << 22;  // aicp_hip_options::tree_lvl_min of the owning context
  bool prof = false;            // aicp_hip_options::profile
  void release_all() {
    for (DevBuf* b : {&W0, &W1, &segof0, &segof1, &seg0, &seg1, &flag, &X1, &X2, &posL, &posR, &ev, &valid, &subs,
                      &mids, &ecnt, &lb, &sums, &pdepth, &ctl, &scan})
      release(*b);
    release(pin_ctl);
  }
};

struct Maps {  // block maps of one flat grid
  std::vector<int32_t> pair;
  std::vector<uint32_t> start;
  void add(int p, uint32_t n, uint32_t per_block) {
    for (uint32_t s = 0; s < n; s += per_block) {
      pair.push_back(p);
      start.push_back(s);
    }
  }
};

// ICP pair groups (1 or 2; AICP_ICP_GROUPS=2 selects two). Two groups measured slower on C2
// (3480 -> 3390 clouds/s): an NN launch over half the pairs takes 62 % of a full one.

// SurfaceNormalDataPointsFilter builds its own libnabo tree with the default bucket size (8),
// whatever bucketSize the chain gives the KDTreeMatcher
constexpr int kNormalsBucket = 8;

struct PackSeg {
  const float* src;
  uint64_t n, stride;
  float* dst4;
};
// Strided xyz -> float4 (w = 1) for many clouds at once, split into equal point ranges over
// up to 16 host threads
void pack_many(const std::vector<PackSeg>& segs, WorkerPool* pool = nullptr);
void pack_xyz4(const float* src, uint64_t n, uint64_t stride_bytes, float* dst4);
bool valid_pair(const aicp_pair& p);
double ev_ms(hipEvent_t a, hipEvent_t b);
// the context options a tree buffer set follows (tree_lvl_min, profile)
void tree_opts(TreeBufs& T, const aicp_hip_options& o);

// Centroid (center = 1) + libnabo-order kd-trees of P clouds on the device (kernels_tree.hip).
// launch = false: allocate the work space only (nothing enqueued; before a stream capture);
// part: launch_tree_prepare's (1: the kernels that do not read the points, 2: the rest, 0: all)
int device_trees_begin(TreeBufs& T, std::string& err, hipStream_t s, size_t P, uint64_t total, PairDesc* dDesc,
                       const float4* raw, int center, int bucket, DevBuf& bpts_out, DevBuf& nodes_out,
                       bool launch = true, int part = 0);
// plan > 0: `plan` global levels with no host read-back; the control block is copied to
// ctl_dst (default T.pin_ctl) at the end of the build unless copy_ctl is false
int device_trees_end(TreeBufs& T, std::string& err, hipStream_t s, size_t P, uint64_t total, PairDesc* dDesc,
                     int bucket, DevBuf& bpts_out, DevBuf& nodes_out, int plan, TreeCtl* ctl_dst = nullptr,
                     bool copy_ctl = true, hipEvent_t levels_done = nullptr);
// errors of a planned build whose control block is in hctl (after its stream completed)
int device_trees_check_ctl(TreeBufs& T, const TreeCtl* hctl, std::string& err);
int device_trees_check(TreeBufs& T, std::string& err);
// force: aicp_hip_options::tree_plan
int plan_levels(uint64_t n_max, const TreeBufs& T, int force, bool lean = false);
int check_cfg(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, int flags);

// ---- the resident form of the quality monitor (monitor.cpp) -----------------------------------
// The monitor's trees over one reference, in buffers of their own: the bucket-8 tree of both exact
// searches and, when the chain matcher's bucket size differs, the matcher's. A live App session
// owns one and keeps it for as long as its reference stays (valid / valid2: the trees were built
// from the current reference); the map sessions' crops change with every pose, so theirs (the
// context's) is rebuilt per reading.
struct MonRefTree {
  DevBuf bpts, nodes, desc;     // bucket 8; desc: the tree's one PairDesc, filled in by the build
  DevBuf bpts2, nodes2, desc2;  // the chain matcher's bucket size
  bool valid = false, valid2 = false;
  int bucket2 = 0;
  void invalidate() { valid = valid2 = false; }
  void release_all() {
    for (DevBuf* b : {&bpts, &nodes, &desc, &bpts2, &nodes2, &desc2}) release(*b);
    invalidate();
  }
};
// monitored readings, bucket-8 trees built, reference-tree reuses, chain-bucket trees built
struct MonCounters {
  uint64_t readings = 0, trees = 0, reuses = 0, trees2 = 0;
};
// One resident pair behind everything enqueued on ctx->stream: d_ref (n_ref float4) and d_read
// (n_read float4) where they lie, d_T the 16 floats of the correction in device memory;
// k_mon_stage, the trees (tree's when it is valid, else built into it), the searches, the selects,
// the reduction, and k_mon_finish writes the 56 bytes to d_result (device memory). Nothing is read
// back and nothing is waited for when the tree levels are planned (plan_levels on ctx->tb_mon, as
// run_batch plans its own; aicp_hip_options::tree_plan = -1 polls, as there). cfg: with
// AICP_MON_PAIRED, the chain. A non-zero return: nothing usable was enqueued (tree->valid is
// cleared). Otherwise, once the stream has been waited for, monitor_resident_check.
int monitor_resident(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg,
                     const float4* d_ref, size_t n_ref, const float4* d_read, size_t n_read, const float* d_T,
                     MonRefTree* tree, MonCounters* cnt, void* d_result);
// After the stream that ran monitor_resident has completed, with the host's copy of its 56 bytes: a
// planned tree deeper than the device stacks (AICP_ERR_UNSUPPORTED) or a direction without a finite
// distance (AICP_ERR_CONVERGENCE), the reason in ctx->err; tree->valid is cleared then.
int monitor_resident_check(aicp_hip_ctx* ctx, MonRefTree* tree, const void* h_result);
int monitor_params_check(aicp_hip_ctx* ctx, const aicp_monitor_params* prm);
// The per-reading monitor of a live session (session.cpp's and map_stream.cpp's): its switch and
// parameters, the counters and the last call's result, with the bodies of the sessions' three
// monitor entry points (monitor.cpp).
struct MonState {
  bool on = false;
  aicp_monitor_params prm{};
  MonCounters cnt;
  aicp_monitor_result last{};
  int32_t valid = 0;
  // this call leaves no result (valid = 0, all zero bytes)
  void none() {
    valid = 0;
    std::memset(&last, 0, sizeof(last));
  }
  int set(aicp_hip_ctx* ctx, const aicp_monitor_params* p);  // p null: off
  int get_last(aicp_monitor_result* out, int32_t* out_valid) const {
    if (!out || !out_valid) return AICP_ERR_INVALID;
    *out = last;
    *out_valid = valid;
    return AICP_OK;
  }
  int counters(uint64_t out[4]) const {
    if (!out) return AICP_ERR_INVALID;
    out[0] = cnt.readings, out[1] = cnt.trees, out[2] = cnt.reuses, out[3] = cnt.trees2;
    return AICP_OK;
  }
  // After the read-back of a reading that went through: ran: monitor_resident was enqueued for it
  // and its 56 bytes are at h_result (checked with monitor_resident_check on `tree`); else err, the
  // reason it was not (empty: the monitor is off), becomes ctx->err. The monitor's own errors leave
  // valid = 0 and the call as it is.
  void take(aicp_hip_ctx* ctx, MonRefTree* tree, bool ran, const void* h_result, const std::string& err);
};

// matcher_trees' treelet step (aicp_hip.cpp), behind the R matcher trees enqueued on s
int matcher_treelets(aicp_hip_ctx* ctx, hipStream_t s, size_t R, uint64_t total_ref, PairDesc* dRdesc, int bucket,
                     std::string& err);
// The matcher's NN engine for R references: their treelet records allotted (rd[r].tl_off / tl_cap;
// kernels_tree.hip: at most 1 + 4 per inner node at even depth), returned as the batch's total, or
// 0 where treelets do not fit and the NN kernel runs on the node records (Trav<1>): leaf slots hold
// a 4-bit count (bucket <= 15), 32-bit byte offsets hold fewer than 2^28 records, the NN kernel's
// LDS frames keep a node id (< 16 * (n_ref + 1)) in 26 bits (n_ref <= 4 M), and
// aicp_hip_options::nn_engine = 1 asks for the node records.
inline uint64_t plan_treelets(PairDesc* rd, size_t R, int bucket, int nn_engine) {
  if (bucket > 15) return 0;
  uint64_t total = 0;
  bool fits = nn_engine != 1;
  for (size_t r = 0; r < R; ++r) {
    rd[r].tl_off = (uint32_t)total;
    rd[r].tl_cap = (uint32_t)(4 * (uint64_t)rd[r].n_ref + 4);
    total += rd[r].tl_cap;
    if (rd[r].n_ref > 4000000u) fits = false;
  }
  return fits && total < (1ull << 28) ? total : 0;
}
// what the ICP kernels take of a chain (prof_slot 0: the NN launches' callers number it)
inline IcpParams icp_params(const aicp_icp_config* cfg) {
  IcpParams ip{};
  ip.maxE2 = (1 + cfg->nn_epsilon) * (1 + cfg->nn_epsilon);
  ip.maxR2 = cfg->nn_max_dist * cfg->nn_max_dist;
  ip.max_iter = cfg->max_iter;
  ip.smooth = cfg->smooth_length;
  ip.min_rot = cfg->min_diff_rot;
  ip.min_trans = cfg->min_diff_trans;
  ip.knn_normals = cfg->knn_normals;
  return ip;
}
WorkerPool* ctx_pool(aicp_hip_ctx* ctx);  // the context's packing threads, created on first use

// The drop-in path's reference cache. App registers reading after reading against one reference
// (app.cpp:72-73, a new one every reference_update_frequency readings, app.cpp:383-391) and calls
// computeOverlap + registerClouds per reading (app.cpp:132-135, 205-210): the reference side of a
// one-shot call (aicp_hip_register / _overlap / _align_batch with one reference array) stays
// resident in the context and is reused while the next call passes the same reference.
struct RefCache {
  // identity: the caller's array (pointer, count, stride), and its points, packed, compared byte
  // for byte on every call (the caller may rewrite the array in place)
  const float* ptr = nullptr;
  uint64_t n = 0, stride = 0;
  std::vector<float> pts;
  // a reference that lives on the device (session.cpp) has no host array: ptr is null, pts empty,
  // and its identity is `owner`, a number the session takes from next_owner for every new
  // reference (0: a caller's host array, the identity above)
  uint64_t owner = 0, next_owner = 1;
  // ctx->bpts, bnrm, nodes, tl, ptl, rdesc, rstate hold its matcher tree, treelets and normals
  bool trees = false;
  int bucket = 0, knn = 0;
  uint64_t tl_total = 0;
  // ctx->bitmap[0, od.bytes) holds its voxel map for (origin, res); gst its group state (|A|, key box)
  bool ovl = false;
  double origin[3] = {0, 0, 0};
  double res = 0;
  OvlDesc od{};
  DevBuf gst;
  // this call
  bool use = false;  // the call may reuse / record (one reference array, a one-shot call)
  bool hit_trees = false, hit_ovl = false;
  uint64_t tree_hits = 0, tree_builds = 0, ovl_hits = 0, ovl_builds = 0;
  void invalidate() {
    trees = ovl = false;
    hit_trees = hit_ovl = use = false;
  }
};

// The reading of the last one-shot call (one pair): App passes the same reading to
// computeOverlap and then to registerClouds (app.cpp:132-135, 205-210), so the second call reuses
// its upload and Morton order (the one-shot batch's read_raw, ctx->read_s) when the array is the
// same and its points are byte-identical.
struct ReadCache {
  const float* ptr = nullptr;
  uint64_t n = 0, stride = 0;
  std::vector<float> pts;
  bool valid = false;
  bool sorted = false;  // its Morton order is in read_s (else the one-shot batch's read_raw serves)
  bool hit = false;  // this call
  uint64_t hits = 0;
};

// aicp_hip_test_overlap's view into the batch's overlap (overlap_maps / overlap_sparse). `on`
// holds for that call alone: the two launch rules and the path take the given values (-1: the
// rule), the ratio is set as a registration sets it, and what ran is recorded with where the key
// path's arrays lie (ctx->ovl_sp / ovl_keys, valid until the next overlap).
struct OvlProbe {
  bool on = false;
  int filter = -1, wide = -1;
  bool keys = false;  // the sorted-key path whatever the maps' size
  int ran_path = 0, ran_filter = 0, ran_wide = 0;  // 1 dense maps, 2 sorted keys
  uint64_t arena_bytes = 0;                        // dense: the map arena as sized
  uint64_t n_points = 0, n_keys = 0;               // keys: per-point slots, words
  const uint32_t* cnt = nullptr;
  const uint64_t* off = nullptr;
  const uint64_t* keys1 = nullptr;
};

struct SeqState;  // sequence.cpp
void seq_state_free(SeqState* s);
struct MapStreamBufs;  // map_stream.cpp
void map_stream_bufs_free(MapStreamBufs* s);

// a caller's cloud as the entry points that take aicp_cloud accept it
inline bool valid_cloud(const aicp_cloud& c) {
  return c.pts && c.n >= 1 && c.n <= (uint64_t)INT32_MAX && c.stride >= 12 && c.stride % 4 == 0;
}

// the batch pipeline (aicp_hip.cpp), for the entry points that compose a batch on the device
int upload_pairs(aicp_hip_ctx* ctx, const aicp_pair* pairs, size_t n, aicp_hip_batch* B, bool refs_on_device,
                 bool skip_refs = false, bool skip_reads = false, bool nosync = false,
                 const int32_t* ref_ids = nullptr);
// What a sampled chain (chain.cpp) adds to a one-pair run_batch; without it run_batch
// does what it did before there were chains.
struct ChainRun {
  // the references' normals, each in its input order at its rdesc ref_off on the device
  // (SurfaceNormal ran earlier in the chain, on the cloud before the later filters): they replace
  // raw tree -> kNN -> k_scatter_normals by one gather through the matcher trees' input index.
  // nullptr: not given
  const float4* ref_normals = nullptr;
  // their rank-deficient counts, one per distinct reference (aicp_icp_stats::degenerate_normals)
  const int32_t* degenerate = nullptr;
  bool max_dist = false;   // MaxDistOutlierFilter: the select step writes limit_d2
  float limit_d2 = 0.f;
  bool batch = false;      // aicp_hip_align_chain_batch: any number of pairs (else one)
  const float* ratios = nullptr;  // per pair, instead of cfg->trimmed_ratio (the overlap's auto-tuned ones)
};
int run_batch(aicp_hip_ctx* ctx, aicp_hip_batch* B, const aicp_icp_config* cfg, double res, int flags, float* outT,
              aicp_icp_stats* stats, float* out_overlap, const ChainRun* chain = nullptr);
// one side's buffers of the sampled chains (chain.cpp): the cloud and its descriptors ping-pong
// between two sets as the filters compact them
struct ChainBufs {
  DevBuf pts[2], nrm[2], dens[2], dens_sn, flag, tile_cnt, tile_off, ctl;
  // the batch form: the clouds' records, where each lies in the upload, the SurfaceNormal trees'
  // descriptors, the segments of the clouds that run; their pinned staging
  DevBuf clouds, src_off, segs;
  PinBuf pin_cl, pin_desc, pin_seg;
  void release_all() {
    for (DevBuf* b : {&pts[0], &pts[1], &nrm[0], &nrm[1], &dens[0], &dens[1], &dens_sn, &flag, &tile_cnt, &tile_off, &ctl,
                      &clouds, &src_off, &segs})
      release(*b);
    for (PinBuf* b : {&pin_cl, &pin_desc, &pin_seg}) release(*b);
  }
};
// One side's filter list over C clouds at once (chain.cpp; DESIGN §4.8, the batch form). The clouds
// lie on the device as an upload left them: cloud c's n_in[c] rows (float4) at dsrc + src_off[c].
// Everything is enqueued on ctx->stream, the records' copy to the host last; nothing is waited for
// unless a SurfaceNormal whose outputs are used sits behind a dropping filter (its trees are sized
// by the counts there). Once the stream has been waited for, o->cl[c] holds cloud c's counts and
// offsets per stage: the kept rows lie at ctx->chain[side].pts[o->cur] + cl[c].off[nf], the normals
// (o->nrm) and, until a MaxDensity consumed them, the densities beside them; dens_sn (o->dens_sn)
// holds the densities at the SurfaceNormal, cloud c's at cl[c].off[o->sn_pos].
struct ChainBatchSide {
  size_t C = 0;
  uint64_t total = 0;
  int nf = 0, cur = 0, sn_pos = -1;
  bool nrm = false, dens_sn = false;
  const ChainCloud* cl = nullptr;  // pinned; valid until the side runs again
};
int chain_batch_side(aicp_hip_ctx* ctx, const aicp_chain* chain, int side, size_t C, const uint32_t* n_in,
                     const float4* dsrc, const uint32_t* src_off, bool want_nrm, bool want_dens, ChainBatchSide* o);
int chain_check(aicp_hip_ctx* ctx, const aicp_chain* c);  // the chain as the registration calls accept it
void free_batch(aicp_hip_batch* B);
// the batch's overlap after its key boxes (overlap.cpp): voxel maps, or sorted key words where they do not fit
int overlap_maps(aicp_hip_ctx* ctx, aicp_hip_batch* B, size_t P, size_t G, PairDesc* dDesc, PairState* dState,
                 PairDesc* dG, PairState* dGst, const float4* readS, double res, bool set_ratio, std::string& err);
// the stream's bound of a cloud's ray keys (overlap.cpp), per-point cap included
extern const uint64_t kMaxRayKeys;
extern const uint64_t kSeqMapBudget;  // bytes of a window's voxel maps beyond which it runs on key lists
uint64_t key_bound(WorkerPool& pool, const aicp_cloud& c, const double* org, double res, bool rigid);

// float AABB of a cloud's points and its sensor origin (the extent bounds its voxel maps)
struct Box {
  float lo[3], hi[3];
  void reset() {
    for (int k = 0; k < 3; ++k) {
      lo[k] = INFINITY;
      hi[k] = -INFINITY;
    }
  }
  void add(float x, float y, float z) {
    const float v[3] = {x, y, z};
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], v[k]);
      hi[k] = std::max(hi[k], v[k]);
    }
  }
  void merge(const Box& b) {
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], b.lo[k]);
      hi[k] = std::max(hi[k], b.hi[k]);
    }
  }
};

// xyz at a byte stride -> float4 (w = 1) and the AABB of each cloud's finite points (sequence.cpp)
void pack_clouds(WorkerPool& pool, const std::vector<PackSeg>& segs, std::vector<Box>& boxes);

// The overlap of one stream window (overlap.cpp): one reference, np readings. The host's part is
// a plan made from the clouds alone; the device's part runs in three steps that the stream puts
// on different streams and aicp_hip_test_overlap one after the other.
struct OvlWinPlan {
  // voxel maps: slot [0] the reference's, [1 + i] reading i's; off preset, the rest sized on the device
  std::vector<OvlDesc> od;
  std::vector<uint64_t> cap;  // the slots' bytes
  uint64_t bm = 0, cap_max = 0;  // all slots together, and the largest
  // key lists (ovl_window_keys): clouds readings 0..np-1 then the reference, their blocks of 256
  // points (cloud, first point; the readings' blocks first), the two lists' capacities
  std::vector<OvlCloud> scl;
  std::vector<uint32_t> sbc, sbs;
  uint64_t cap_r = 0, cap_g = 0;
  std::vector<uint64_t> kb_read;  // each reading's key bound
};
// src_rigid / read_rigid: sized for any rigid motion of that cloud (a corrected reference; debug mode)
void ovl_window_slots(OvlWinPlan& W, const Box& src_box, const double* src_origin, bool src_rigid, const Box* boxes,
                      const aicp_cloud* reads, size_t np, double res, bool read_rigid);
// ref_origin: the origin the reference's rays start from when the host knows it (else 3 zeros, device-written)
void ovl_window_keys(OvlWinPlan& W, WorkerPool& pool, const aicp_cloud& src, const double* ref_origin, bool ref_rigid,
                     const aicp_cloud* reads, const uint32_t* loff, size_t np, double res, bool read_rigid);
// the two key sides on device arrays: dcl / dbc the plan's clouds and block words (sbc then sbs) as
// uploaded, cnt / off one slot per point (readings, then the reference), keys_r / keys_g 2 cap words each
void ovl_window_sides(const OvlWinPlan& W, size_t np, uint64_t nread, uint32_t n_ref, OvlCloud* dcl,
                      const uint32_t* dbc, uint32_t* cnt, uint64_t* off, uint64_t* keys_r, uint64_t* keys_g,
                      void* tmp_r, size_t tmp_rb, void* tmp_g, size_t tmp_gb, unsigned long long* pc, OvlKeySide& kr,
                      OvlKeySide& kg);
struct OvlWinDev {  // where a window's overlap lies on the device
  bool sparse = false;
  size_t np = 0;
  double res = 0;
  const PairDesc* dDesc = nullptr;  // np readings
  PairState* dState = nullptr;
  const PairDesc* dG = nullptr;     // the reference's group
  PairState* dGst = nullptr;
  OvlDesc* dOvl = nullptr;          // np + 1 slots
  const uint64_t* dCap = nullptr;
  uint8_t* bmp = nullptr;
  uint64_t cap_max = 0, cap0 = 0;   // the largest reading slot bound given to the clear; the reference's
  BlockMap m_read{}, m_gref{};
  const OvlKeySide* kr = nullptr;
  const OvlKeySide* kg = nullptr;
  unsigned long long* per_pair = nullptr;
  bool filter = false, wide = false;  // the stream's choice for both: plain stores, narrow counts
};
// side 1: the readings (pts their points), side 0: the reference (origin0, nullable: its origin
// where the device wrote it)
int ovl_window_side(std::string& err, hipStream_t s, const OvlWinDev& D, int side, const double* origin0,
                    const float4* pts);
int ovl_window_counts(std::string& err, hipStream_t s, const OvlWinDev& D);
// the device-resident map (aicp_hip.cpp), for the streams that grow it and crop it into a batch
int map_reserve(aicp_hip_ctx* ctx, aicp_hip_map* map, size_t add);
int map_crop_pairs(aicp_hip_ctx* ctx, const aicp_hip_map* map, float mn, float mx, const aicp_cloud* readings,
                   const float* poses, size_t n, const double* read_origins, size_t* n_ok, const uint32_t** counts,
                   const uint32_t* dev_read_n = nullptr);
// aicp_hip_map_crop with the kept points left on the device, in dst (session.cpp: a start on a map)
int map_crop_resident(aicp_hip_ctx* ctx, const aicp_hip_map* map, float mn, float mx, const float origin[16],
                      DevBuf* dst, uint32_t* kept);
// a raw reading for the raw streams (map_stream.cpp): its rows uploaded, k_stream_ingest into the
// pre-filter's input (d_initT / d_origin: debug mode, nullable), the pre-filter, and the kept
// points copied device-to-device to dst (room for c.n points). Returns with ctx->stream idle up to
// that copy and *kept known.
int stream_prefilter_raw(aicp_hip_ctx* ctx, const aicp_prefilter_params* pf, const aicp_cloud& c, const float* d_initT,
                         double* d_origin, float4* dst, uint32_t* kept);
int stream_prefilter_check(aicp_hip_ctx* ctx, const aicp_prefilter_params* pf);  // pf_check
// a caller's raw rows into ctx->scratch at byte `off`: *drows / *dstride where, and their stride there
int ingest_upload(aicp_hip_ctx* ctx, const float* pts, size_t n, size_t stride, size_t off, const void** drows,
                  size_t* dstride);
// stream_prefilter_raw for rows that may lie on the device already (session.cpp): dpts non-null: n
// float4 rows on the device (the sweep accumulator's cloud, left unchanged; hpts / stride not read),
// else the caller's rows are uploaded. pf null: no pre-filter, the n ingested points go straight to
// dst and *kept = n (nothing is waited for then).
int stream_ingest_rows(aicp_hip_ctx* ctx, const aicp_prefilter_params* pf, const float* hpts, size_t n, size_t stride,
                       const float4* dpts, const float* d_initT, double* d_origin, float4* dst, uint32_t* kept);
// The reference cache's check for a one-pair call whose reference lives on the device under the
// identity `owner` (RefCache::owner): sets what the call reuses and records, as refcache_begin does
// for a host array. The caller clears RefCache::use after its run_batch (and invalidates on an error).
void refcache_begin_resident(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, uint64_t owner, uint64_t n_ref,
                             const double origin[3], double res, int flags);
// The risk gate of aicp_hip_pipeline and of the live session (session.cpp), behind an overlap-only
// run_batch of the same pair on ctx->stream: the batch's overlap into d_gate->overlap, the alignment
// features (alignability into d_gate->alignability, device to device), then k_svm_predict into
// d_gate's raw, risk, gate and ratio. The clouds: the caller's host arrays (ref / read: pts, n,
// stride), or, with d_ref / d_read given, where they lie on the device (float4; then only n is
// read). Nothing of d_gate is read back here. The poses: column-major double[16]. d_overlap (device,
// nullable): the overlap to classify instead of the batch's (the prior map's constant: no batch ran).
int gate_resident(aicp_hip_ctx* ctx, const aicp_risk_params* prm, const aicp_hip_svm* model, double threshold,
                  const aicp_cloud& ref, const aicp_cloud& read, const float4* d_ref, const float4* d_read,
                  const double* ref_pose, const double* read_pose, GateRec* d_gate, float* fov_overlap,
                  const float* d_overlap = nullptr);
// The loop of the two offline App-order entry points (aicp_hip_sequence_run_raw in debug mode,
// aicp_hip_sequence_run_risk; session.cpp): a session private to the call, started on `first` and
// fed the readings one by one into out_T + 16 i, out[i] (and risk->rec[i]); *n_done = i + 1 after
// every reading that ran; the first non-zero return ends the loop and is the call's, with
// ctx->err in the entry points' wording. The arguments are the entry points', already checked.
struct ReplayRisk {  // aicp_hip_sequence_run_risk's part
  const aicp_risk_params* prm;
  const aicp_hip_svm* model;
  double threshold;
  const double* first_pose;
  const double* poses;
  aicp_pipeline_record* rec;
};
int session_replay(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                   const aicp_prefilter_params* pf, const ReplayRisk* risk, const aicp_cloud* first,
                   const aicp_cloud* readings, size_t n, float* out_T, aicp_sequence_result* out, size_t* n_done);
// what a go-back takes from a live session (session.cpp): App's graph count and the device address
// of its initialT_; AICP_ERR_INVALID for a session of another context, not started, or ended
int session_go_back(aicp_hip_ctx* ctx, const aicp_hip_session* s, uint64_t* n_clouds, const float** d_initT);
int risk_params_check(aicp_hip_ctx* ctx, const aicp_risk_params* prm);  // its pre-filter's pf_check
// the gate's pose rules (aicp_hip.cpp: fromMatrix4fToIsometry3d(T) * prior, removePitchRollCorrection)
void pose_moved(const float* T, const double* prior, double* out);
void pose_fix_pitch_roll(const double* corrected, const double* odom, double* out);
// the sweep accumulator's cloud where it lies (accum.cpp): waits for the stream, *n points at *pts
int accum_resident(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const float4** pts, size_t* n);
// aicp_hip_prefilter on n device-resident points (float4, w = 1; left unchanged), moved first by T
// (nullable, host, column-major) as aicp_hip_transform moves them; kept points packed xyz to out
// (capacity cap points). For the sweep accumulator (accum.cpp).
int prefilter_resident(aicp_hip_ctx* ctx, const aicp_prefilter_params* prm, const float4* dpts, size_t n,
                       const float* T, float* out, size_t cap, size_t* out_n);

}  // namespace rt
}  // namespace aicp

struct aicp_hip_batch {
  size_t P = 0;
  std::vector<aicp::PairDesc> desc;
  std::vector<aicp::PairDesc> rdesc;  // one per distinct reference cloud (tree + normals built once)
  std::vector<aicp::PairDesc> gdesc;  // one per overlap group: distinct (reference cloud, origin)
  uint64_t total_ref = 0, total_read = 0;
  uint32_t n_red_total = 0;
  aicp::rt::DevBuf ref_raw, read_raw, maps;
  aicp::BlockMap m_read{}, m_gref{}, m_red{}, m_sel{};
  bool refs_event = false;  // upload_pairs recorded ctx->ev[14] after the references' copy
};

struct aicp_hip_map {  // a device-resident point cloud (float4, w = 1)
  aicp::rt::DevBuf pts;
  size_t n = 0;
};

struct aicp_hip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // raw kd-tree + normals, concurrent with the overlap on `stream`
  hipStream_t stream3 = nullptr;  // centroid + matcher kd-tree, concurrent with both
  std::string err;
  aicp::rt::DevBuf read_c, bpts, bnrm, nodes, match, d2, desc, state, touch, slab, bitmap, outT, scratch, active,
      ctrs, nbids, ref1, sel_hist, sel_cand, sel_cnt, qmap, ovl, rdesc, rstate, rdesc_raw, bpts_raw, nodes_raw,
      nrm_raw, inv, gdesc, gstate, read_s, ord_k0, ord_k1, ord_v0, ord_v1, ord_tmp, tl, ptl,
      tl_rank, pf_a, pf_b, pf_bpts, pf_nodes;  // pf_*: the pre-filter's own (the reference cache keeps bpts / nodes)
  uint64_t tl_total = 0;  // matcher treelet records allotted for this batch (0: no treelets, Trav<1>)
  aicp::rt::TreeBufs tb[2];  // [0] raw-coordinate tree (stream2), [1] centred matcher tree (stream3)
  aicp::rt::PinBuf pin_desc, pin_state, pin_out, pin_io, pin_ovl, pin_rdesc, pin_gdesc, pin_gstate;
  aicp::rt::PinBuf pin_pf;  // pre-filter read-backs (PfHost): outlive any early return of pf_core
  std::vector<hipEvent_t> nn_ev;
  hipEvent_t ev[16] = {};
  int last_nn_launches = 0;
  double last_nn_ms = 0, last_nn_bytes = 0;
  uint64_t last_queries = 0;
  double last_phase[5] = {0, 0, 0, 0, 0};
  aicp_prefilter_stats last_pf{};  // timing and kNN counts of the last pre-filter
  aicp_hip_batch* oneshot = nullptr;  // buffers of aicp_hip_align_batch, kept across calls
  hipEvent_t pf_ev[8] = {};
  aicp::rt::SeqState* seq = nullptr;  // aicp_hip_sequence_run's buffers (sequence.cpp), kept across calls
  aicp::rt::MapStreamBufs* ms = nullptr;  // the map localization streams' buffers (map_stream.cpp), kept across calls
  aicp_hip_batch* mapbatch = nullptr;  // aicp_hip_map_register_batch's batch buffers
  aicp::rt::DevBuf crop_ws;            // its crop work space
  aicp::rt::DevBuf ovl_sp, ovl_keys;   // sparse overlap: clouds, counts, offsets / key words
  aicp::rt::DevBuf isync;              // fused ICP iteration: arrival counters (icp_sync_words)
  aicp::rt::PinBuf pin_crop;
  aicp::rt::PinBuf pin_maps;  // upload_pairs' block maps
  aicp::rt::ChainBufs chain[2];  // the sampled chains' filtered clouds: [reference], [reading] (chain.cpp)
  aicp_hip_batch* chainbatch = nullptr;  // aicp_hip_align_chain_batch: the clouds as given (the filtered ones: oneshot)
  aicp::rt::PinBuf pin_chain;    // their control blocks read back
  aicp::rt::RefCache refc;  // the drop-in path's resident reference (runtime.hpp)
  aicp::rt::OvlProbe ovl_probe;  // aicp_hip_test_overlap (off in every other call)
  aicp::rt::ReadCache rdc;  // and its last reading
  aicp::rt::WorkerPool* pool = nullptr;  // host threads of the one-shot calls (packing, the reference compare)
  uint32_t* poll_host = nullptr;  // the batch loop's active counts (hipHostMalloc, mapped), kBatchPolls words
  uint32_t* poll_dev = nullptr;
  // alignment-risk features: [0], [1] the two clouds (input, accepted points, then the sampled
  // cloud, labels and cluster records: the pre-filter's context buffers are workspace that the next
  // pre-filter rewrites), [2] sort, count and matching work space
  aicp::rt::DevBuf risk[3];
  aicp::rt::PinBuf pin_risk;
  hipEvent_t risk_ev[7] = {};
  aicp_risk_stats last_risk{};
  // the classifier (kernels_svm.hip): the models this context has seen, uploaded once each (keyed
  // by aicp_hip_svm::id), samples / results of a predict call, and the pipeline's gate record
  struct SvmDev {
    uint64_t id = 0;
    aicp::rt::DevBuf entries;
    uint32_t count = 0;
  };
  std::vector<SvmDev> svm_models;
  aicp::rt::DevBuf svm_io;
  aicp::rt::PinBuf pin_svm;
  // registration quality monitor (monitor.cpp): trees and work space of its own (the reference
  // cache keeps bpts / nodes; mon_*2: the chain matcher's trees when its bucket size is not 8)
  aicp::rt::DevBuf mon_bpts, mon_nodes, mon_bpts2, mon_nodes2, mon_ws;
  aicp::rt::PinBuf pin_mon;
  hipEvent_t mon_ev[5] = {};
  aicp_monitor_stats last_mon{};
  // its resident form (monitor_resident): the tree builder's work space and plan of its own (tb[0]'s
  // plan follows run_batch's raw trees), the planned builds' control blocks (reference tree, chain
  // matcher's tree, the reading's tree) and the map sessions' per-reading reference trees
  aicp::rt::TreeBufs tb_mon;
  aicp::rt::PinBuf pin_mon_ctl;
  int mon_planned[3] = {0, 0, 0};  // the levels planned for each control block's build (0: none, or polled)
  aicp::rt::MonRefTree mon_scratch;
  aicp_hip_options opt{};  // aicp_hip_set_options (read by the calls; nothing reads the environment)
};
constexpr int kBatchPolls = 64;

#define HIPC(x)                                                                   \
  do {                                                                            \
    const hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                       \
      ctx->err = std::string(#x) + ": " + hipGetErrorString(e_);                  \
      return AICP_ERR_HIP;                                                        \
    }                                                                             \
  } while (0)

#define FAIL(code, msg)   \
  do {                    \
    ctx->err = (msg);     \
    return (code);        \
  } while (0)

// Tree builders report errors into `err` (they also run on a worker thread, see run_batch).
#define TCHK(x)                                                                   \
  do {                                                                            \
    const hipError_t e_ = (x);                                                    \
    if (e_ != hipSuccess) {                                                       \
      err = std::string(#x) + ": " + hipGetErrorString(e_);                       \
      return AICP_ERR_HIP;                                                        \
    }                                                                             \
  } while (0)
#define TFAIL(code, msg) \
  do {                   \
    err = (msg);         \
    return (code);       \
  } while (0)
