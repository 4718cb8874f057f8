/*
 * aicp_hip.h — C-ABI of the MI355X-native ICP registration core (libaicp_hip.so).
 *
 * This is the drop-in boundary that replaces the in-process C++ virtual interfaces
 * of aicp_core (reference paths relative to zbqq/aicp_mapping):
 *
 *   aicp::AbstractRegistrator   aicp_core/include/aicp_registration/abstract_registrator.hpp:8-19
 *     registerClouds(ref, read, Matrix4f&)   -> aicp_hip_register / aicp_hip_register_batch
 *     getOutputReading(cloud)                -> aicp_hip_transform
 *     updateConfigParams(path)               -> aicp_hip_parse_pm_yaml
 *   aicp::AbstractOverlapper    aicp_core/include/aicp_overlap/abstract_overlapper.hpp:13-19
 *     computeOverlap(...) + getOverlap()     -> aicp_hip_overlap / aicp_hip_overlap_batch
 *   App::computeRegistration ratio auto-tune aicp_core/src/registration/app.cpp:197-205
 *     + replaceRatioConfigFile               aicp_core/src/utils/fileIO.cpp:179-214
 *                                            -> aicp_hip_autotune_ratio,
 *                                               aicp_hip_replace_ratio_config_file,
 *                                               aicp_hip_align_batch (overlap -> ratio -> ICP on device)
 *   SVM::test (failure_prediction_mode)    aicp_core/src/classification/svm.cpp:48-110
 *                                            -> aicp_hip_svm_load, aicp_hip_svm_predict
 *   App::runAicpPipeline with the risk gate  aicp_core/src/registration/app.cpp:218-247, 362-411
 *                                            -> aicp_hip_pipeline, aicp_hip_sequence_run_risk,
 *                                               aicp_hip_session_create_risk (live, one reading per call)
 *
 * Conventions
 *   - Plain C, no exceptions cross this boundary; every entry point returns an AICP_* code.
 *   - Host memory is caller-owned. Point arrays are AoS float x,y,z at a byte stride, so a
 *     pcl::PointXYZ array (16 B per point) passes zero-copy with stride = 16.
 *   - Counts are explicit (the reference uses cloud.width, cloudIO.cpp:83).
 *   - Transforms are column-major float[16], so Eigen::Matrix4f::data() passes through.
 *   - A context owns one HIP stream and a device arena; use one context per host thread
 *     (the reference calls its registrator from a single worker thread, app.cpp:528-550).
 */
#ifndef AICP_HIP_H_
#define AICP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- return codes --------------------------------------------------------------------- */
#define AICP_OK 0
#define AICP_ERR_CONVERGENCE 1  /* maps PM::ConvergenceError ("no outlier to filter",
                                   "no point to minimize", NaN in the differential checker) */
#define AICP_ERR_INVALID 2      /* invalid argument / config (reference: exit(1),
                                   pointmatcher_registration.cpp:60-64,96-100) */
#define AICP_ERR_HIP 3          /* HIP runtime failure or extension unavailable */
#define AICP_ERR_UNSUPPORTED 4  /* chain element or size not supported by this core */
#define AICP_ERR_TRANSFORMATION 5 /* maps PM::TransformationError: a transform applied to the
                                     reading has |1 - det R| > 0.001 (RigidTransformation::
                                     checkParameters; the initial T, every T_iter, the final T) */

typedef struct aicp_hip_ctx aicp_hip_ctx;
typedef struct aicp_hip_batch aicp_hip_batch;

/* The libpointmatcher chain subset of icp_autotuned_default.yaml:9-51, and its point-to-point
 * variant (icp_2Dtesting_cfg.yaml).
 * knn_normals: 10, 20 or 30 run SurfaceNormal on the reference and PointToPlaneErrorMinimizer;
 * 0 means no SurfaceNormal on the reference and PointToPointErrorMinimizer (point-to-plane cannot
 * run without normals, so the value is unambiguous). aicp_hip_parse_pm_yaml sets 0 for a chain
 * whose errorMinimizer is the bare name PointToPointErrorMinimizer, as the reference's chain files
 * write it (the map form "PointToPointErrorMinimizer:" stays AICP_ERR_UNSUPPORTED, as it was). Served by the register / batch / multi /
 * localization-stream calls; aicp_hip_sequence_run and _run_raw return AICP_ERR_UNSUPPORTED. */
typedef struct {
  int32_t knn_normals;    /* SurfaceNormalDataPointsFilter.knn; 0: point-to-point (20) */
  float nn_epsilon;       /* KDTreeMatcher.epsilon                        (3.16) */
  float nn_max_dist;      /* KDTreeMatcher.maxDist                        (inf)  */
  float trimmed_ratio;    /* TrimmedDistOutlierFilter.ratio               (0.70) */
  int32_t max_iter;       /* CounterTransformationChecker.maxIterationCount (20) */
  float min_diff_rot;     /* DifferentialTransformationChecker.minDiffRotErr (1e-3) */
  float min_diff_trans;   /* DifferentialTransformationChecker.minDiffTransErr (1e-2) */
  int32_t smooth_length;  /* DifferentialTransformationChecker.smoothLength (4) */
  int32_t bucket_size;    /* libnabo kd-tree bucketSize                    (8)   */
  int32_t knn_match;      /* KDTreeMatcher.knn; only 1 is supported        (1)   */
} aicp_icp_config;

typedef struct {
  int32_t status;            /* AICP_* code of this pair                          */
  int32_t iterations;        /* ICP iterations executed (IterationsCount)         */
  int32_t converged;         /* 1: differential checker stopped, 0: counter limit */
  int32_t degenerate_normals;/* SurfaceNormal rank-deficient points (reference)   */
  float inlier_ratio;        /* weightedPointUsedRatio of the last iteration      */
  float trimmed_ratio;       /* ratio actually used                               */
  float overlap_percent;     /* octree-equivalent overlap, -1 if not computed     */
  int32_t tree_depth;        /* depth of the matcher kd-tree                      */
  uint64_t nn_points_touched;/* libnabo PointCountTouched over all iterations     */
  uint64_t nn_nodes_touched; /* inner nodes descended over all iterations         */
  uint64_t overlap_keys[3];  /* |S_ref|, |S_read|, |S_ref ∩ S_read|                */
} aicp_icp_stats;

typedef struct {
  const float* ref;      /* reference cloud, x,y,z at ref_stride bytes            */
  uint64_t n_ref;
  uint64_t ref_stride;   /* bytes between points: 12 packed, 16 / 32 / 48 =      */
                         /* pcl::PointXYZ / PointXYZRGB / PointXYZRGBNormal rows   */
  const float* read;     /* reading cloud                                         */
  uint64_t n_read;
  uint64_t read_stride;
  const float* init_T;   /* nullable = identity; column-major 4x4                 */
  double ref_origin[3];  /* sensor origin of the reference (pose translation)     */
  double read_origin[3]; /* sensor origin of the reading                          */
} aicp_pair;

/* One cloud with its sensor origin (the sequence and localization entry points). */
typedef struct {
  const float* pts;      /* x, y, z at `stride` bytes */
  uint64_t n;
  uint64_t stride;
  double origin[3];      /* prior pose translation = sensor origin (octrees_overlap.cpp:229-230) */
} aicp_cloud;

/* flags for aicp_hip_align_batch / aicp_hip_batch_run */
#define AICP_RUN_OVERLAP 1      /* compute overlap and auto-tune the trimmed ratio */
#define AICP_RUN_ICP 2          /* run the ICP registration                        */
#define AICP_RUN_TIME_NN 4      /* record HIP events around every NN launch        */

/* ---- context ---------------------------------------------------------------------------- */
int aicp_hip_create(int device, aicp_hip_ctx** out);
void aicp_hip_destroy(aicp_hip_ctx* ctx);
const char* aicp_hip_last_error(const aicp_hip_ctx* ctx);
const char* aicp_hip_version(void);
/* Provenance of this binary: "src <sha256 prefix of its sources and Makefile> arch <gfx> extra
 * <extra compile flags>" (aicp_mapping_amd/csrc/Makefile); aicp_mapping_amd._lib.source_hash()
 * computes the same hash from a source tree. */
const char* aicp_hip_build_info(void);

/* Context options: the engine and schedule switches the tests and A/B measurements use. The
 * library reads no environment variable; a context starts with aicp_hip_default_options' values
 * (the product path) and keeps what aicp_hip_set_options gives it until the next call. No option
 * changes a result: every engine and schedule gives the same transforms, statistics and counts
 * (the tests compare them). Replaces nothing in the reference. */
typedef struct {
  int32_t profile;            /* 1: host and device phase times (and the counters of the diagnostic
                                 build, -DAICP_DIAG=1) on stderr; the timing events it records
                                 shift the schedule slightly */
  int32_t nn_engine;          /* 0: treelet records where they fit (bucketSize <= 15, <= 4 M
                                 reference points); 1: node records (Trav<1>) always */
  int32_t overlap_path;       /* 0: voxel maps within their memory budget, sorted key lists above;
                                 1: sorted key lists always */
  int32_t normals_knn_engine; /* SurfaceNormal kNN: 0: one octet of lanes per query up to 300 000
                                 queries, one lane above; 1: octets always; 2: one lane always */
  int32_t select_pair;        /* trimmed select: -1: one workgroup per pair from 256 pairs on
                                 (readings <= 65536 each); 0: never; 1: whenever it fits */
  int32_t select_fused_from;  /* ICP iteration from which the chip-wide select runs as one launch
                                 (0: never); 3 */
  int32_t raw_tree_first;     /* batch path: -1: the raw-coordinate tree before the matcher tree
                                 from 4 M reference points on; 0: never; 1: always */
  int32_t raw_first_at;       /* with the raw tree first, the matcher tree starts after the raw
                                 tree's global levels (2) or after the whole raw tree (1); 2 */
  int32_t no_early_exit;      /* 1: every ICP loop enqueues maxIterationCount iterations (tests:
                                 the polled early exit must not change results) */
  int32_t tree_plan;          /* kd-tree global levels: 0: planned from the cloud size; k > 0: k
                                 levels (tests: a too-shallow plan); -1: host-polled build */
  uint32_t tree_lvl_min;      /* the level-synchronous subtree builder from this many points of a
                                 build on; 4194304 */
  int32_t reference_cache;    /* 1: the one-shot calls keep their reference (and last reading)
                                 resident for the next call, identified by a byte compare against a
                                 host copy (aicp_hip_reference_cache_stats); 0: nothing is kept,
                                 copied or compared between calls */
  uint32_t oneshot_keep_mib;  /* device copies of a one-shot call's inputs are kept for the next
                                 call up to this size (MiB), released above it; 4096 */
  int32_t early_reference;    /* stream (non-debug): 1: the next reference starts once its source
                                 reading's registration has stopped, while the window's other
                                 readings still iterate; 0: once the whole window's loop ends; 1 */
  uint64_t read_order_min;    /* Morton order of a batch's readings from this many points on;
                                 200000 */
} aicp_hip_options;
void aicp_hip_default_options(aicp_hip_options* out);
int aicp_hip_set_options(aicp_hip_ctx* ctx, const aicp_hip_options* opt);
int aicp_hip_get_options(const aicp_hip_ctx* ctx, aicp_hip_options* out);
/* Test hook, process-wide on the calling thread's device: on != 0 sends every tile but the first
 * of the kd-tree builds' single-pass scans down the path a stalled look-back takes (the exact
 * prefix recomputed, error 16 reported: the call returns AICP_ERR_HIP and nothing faults). */
int aicp_hip_test_force_scan_stall(int on);

/* ---- configuration (host-only; the reference re-parses the chain per call) -------------- */
void aicp_hip_default_config(aicp_icp_config* out);
/* Parses the libpointmatcher chain subset (pointmatcher_registration.cpp:59-66).
 * Unsupported chain elements yield AICP_ERR_UNSUPPORTED. */
int aicp_hip_parse_pm_yaml(const char* path, aicp_icp_config* out);
/* Text rewrite of "ratio: " + 4 chars, byte-for-byte as fileIO.cpp:179-214. */
int aicp_hip_replace_ratio_config_file(const char* in_path, const char* out_path, float ratio);
/* clamp(overlap/100, .25, .70) (app.cpp:197-202) then the 6-significant-digit text
 * round trip of replaceRatioConfigFile + lexical_cast<float>. */
float aicp_hip_autotune_ratio(float overlap_percent);

/* ---- sampled chains: the data-point filters and the MaxDist outlier rule -------
 * What a chain file holds beside aicp_icp_config: per side an ordered list of data-point filters,
 * and the outlier rule. An all-zero aicp_chain means "no filters, TrimmedDist". Rules are those of
 * libpointmatcher 1.2.x; every filter keeps the order of the points it keeps.
 *   SurfaceNormal   knn in {10, 20, 30} where its output is used (normals of a point-to-plane
 *                   reference, densities of a later MaxDensity); keep_densities as keepDensities
 *   MinDist         dim -1: keep sqrtf((x*x + y*y) + z*z) > fabsf(min_dist); dim 0..2: keep
 *                   fabsf(coord[dim]) > min_dist
 *   RandomSampling  every point draws r; keep r < prob
 *   MaxDensity      density <= max_density: kept without a draw; else keep r < max_density /
 *                   density, times (1 - nbSaturated / nbPointsIn) in integer division for the
 *                   points whose density equals the cloud's maximum
 * The draw is r = aicp_hip_chain_uniform(seed, slot, i): slot = 4 * side + the filter's position
 * in its list, i = the point's index in the cloud as that filter receives it. It is a pure function:
 * the same seed gives the same sample on every call, on the host and on the device; a caller who
 * wants fresh samples changes the seed. (libpointmatcher draws std::rand(), which the reference
 * reseeds from the clock in every pre-filter, so its own samples cannot be reproduced.) */
#define AICP_CHAIN_MAX_FILTERS 4
#define AICP_CHAIN_REFERENCE 0
#define AICP_CHAIN_READING 1
#define AICP_FILTER_NONE 0
#define AICP_FILTER_SURFACE_NORMAL 1
#define AICP_FILTER_MIN_DIST 2
#define AICP_FILTER_RANDOM_SAMPLING 3
#define AICP_FILTER_MAX_DENSITY 4
#define AICP_OUTLIER_TRIMMED_DIST 0 /* limit: the quantile cfg->trimmed_ratio of the finite d2 */
#define AICP_OUTLIER_MAX_DIST 1     /* limit: outlier_limit_d2 */
typedef struct {
  int32_t kind;           /* AICP_FILTER_* */
  int32_t knn;            /* SurfaceNormal.knn                      (5)    */
  int32_t keep_densities; /* SurfaceNormal.keepDensities            (0)    */
  int32_t dim;            /* MinDist.dim: -1 radius, 0 / 1 / 2 axis (-1)   */
  float min_dist;         /* MinDist.minDist                        (1)    */
  float prob;             /* RandomSampling.prob                    (0.75) */
  float max_density;      /* MaxDensity.maxDensity                  (10)   */
  int32_t pad;
} aicp_chain_filter;
typedef struct {
  aicp_chain_filter filters[2][AICP_CHAIN_MAX_FILTERS]; /* [AICP_CHAIN_REFERENCE], [_READING] */
  int32_t n_filters[2];
  int32_t outlier;        /* AICP_OUTLIER_* */
  /* MaxDist: a pair is kept when its squared matcher distance d2 <= outlier_limit_d2. The parser
   * stores MaxDistOutlierFilter.maxDist as written: libpointmatcher 1.2.x compares the matcher's
   * squared distance with the parameter itself. Later versions square the parameter; a caller who
   * wants that rule stores maxDist * maxDist here. */
  float outlier_limit_d2;
  uint64_t seed;          /* of the draws; the parser sets 0 */
} aicp_chain;
typedef struct {
  uint64_t n_in[2];                            /* points of the reference / the reading as given */
  uint64_t n_out[2][AICP_CHAIN_MAX_FILTERS];   /* points after each filter of the side's list   */
  uint64_t n_kept[2];                          /* points the ICP core ran on                     */
} aicp_chain_stats;
/* As aicp_hip_parse_pm_yaml, with the filter lists and the outlier rule in *chain. Accepts every
 * file that call accepts (same aicp_icp_config; the chain then holds at most the SurfaceNormal
 * entries) and MinDist / RandomSampling / MaxDensity data-point filters and MaxDistOutlierFilter.
 * AICP_ERR_INVALID: MaxDensity with no earlier SurfaceNormal with keepDensities: 1 on its side,
 * prob outside [0, 1], maxDensity <= 0, dim outside {-1, 0, 1, 2}, a MaxDistOutlierFilter.maxDist
 * that is negative or not finite (the registration call checks outlier_limit_d2 the same way: a
 * reading without a match has d2 = inf, which an infinite limit would keep). AICP_ERR_UNSUPPORTED: more than
 * 4 filters or two SurfaceNormals on a side, a file with one of the new elements whose used
 * SurfaceNormal has knn outside {10, 20, 30}, and whatever aicp_hip_parse_pm_yaml refuses beyond
 * the elements named here (SamplingSurfaceNormal among them). */
int aicp_hip_parse_pm_chain(const char* path, aicp_icp_config* out, aicp_chain* chain);
/* The filters' draw: k * 2^-24 with k in [0, 2^24), so exact in float and in [0, 1). */
float aicp_hip_chain_uniform(uint64_t seed, uint32_t slot, uint32_t i);
/* DataPointsFilters::apply of one side's list (side: AICP_CHAIN_REFERENCE / _READING) on one
 * cloud. The filtered cloud stays on the device; the host gets the kept count, the count after
 * each filter, and through nullable pointers: the kept points' input indices (ascending; capacity
 * n), the densities at the SurfaceNormal's position in the order of the cloud there (capacity n;
 * only with keep_densities), and the kept points' normals (3 floats each, capacity n; only with a
 * SurfaceNormal of knn 10 / 20 / 30: they are the normals of the cloud at the SurfaceNormal's
 * position, carried through the later filters). A cloud that a filter empties is AICP_OK with
 * *out_n = 0. Invalidates the context's reference cache. */
int aicp_hip_chain_filter(aicp_hip_ctx* ctx, const aicp_chain* chain, int side, const float* pts, size_t n,
                          size_t stride, uint64_t* out_n, uint64_t out_counts[AICP_CHAIN_MAX_FILTERS],
                          int32_t* out_index /* nullable */, float* out_densities /* nullable */,
                          float* out_normals /* nullable */);
/* Filters both clouds of the pair, then runs the ICP core on the filtered clouds where they lie on
 * the device. A reference whose list has a SurfaceNormal hands the core the normals computed at
 * that position (those of the cloud before the later filters); the matcher tree is built over the
 * survivors. stats->inlier_ratio is over the filtered reading. A side left without a point:
 * AICP_ERR_CONVERGENCE, the side named in aicp_hip_last_error. A chain with no filter but
 * SurfaceNormal and the TrimmedDist rule gives aicp_hip_register's bits (reference cache off).
 * The call neither uses nor keeps the reference cache, and drops it. Chains are served here and,
 * for many pairs at once, by aicp_hip_align_chain_batch below; the multi-GPU, stream and session
 * calls take aicp_icp_config alone. */
int aicp_hip_register_chain(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_chain* chain,
                            const aicp_pair* pair, float out_T[16], aicp_icp_stats* stats /* nullable */,
                            aicp_chain_stats* chain_stats /* nullable */);
/* aicp_hip_register_chain for n_pairs pairs in one call: pair i gets exactly what the one-pair
 * call on that pair returns (same seed), out_T bit for bit. flags: AICP_RUN_ICP, or AICP_RUN_ICP |
 * AICP_RUN_OVERLAP; anything else is AICP_ERR_INVALID.
 *   Filters. Every cloud is filtered by its side's list on its own: the draw's index i, MaxDensity's
 *   maximum and saturated count and SurfaceNormal's neighbourhoods are those of the point's own
 *   cloud, never the batch's. Pairs that pass the same reference array (pointer, count, stride)
 *   share it: its filters, its matcher tree and its normals run once.
 *   AICP_RUN_OVERLAP. App's order: the octree overlap is computed on the clouds as given, with the
 *   pair's origins, at `resolution` (not read otherwise); the pair's TrimmedDist ratio is
 *   aicp_hip_autotune_ratio(overlap) and cfg->trimmed_ratio is not read. stats[i].overlap_percent,
 *   overlap_keys and trimmed_ratio are filled as aicp_hip_align_batch fills them, with the MaxDist
 *   rule too (which does not read the ratio).
 *   A pair whose filters leave a side without a point: stats[i].status = AICP_ERR_CONVERGENCE,
 *   the identity in out_T, its chain_stats filled, nothing else of it runs; the other pairs are
 *   not affected. An emptied shared reference ends all its pairs.
 *   Returns the first non-zero pair status in pair order; aicp_hip_last_error names that pair
 *   ("pair 3: ...") and, for an emptied one, the side in aicp_hip_register_chain's words.
 *   stats[i].inlier_ratio is over the filtered reading; degenerate_normals is the count of the cloud
 *   the reference's SurfaceNormal ran on.
 * Limits: 4096 pairs, 2^28 reference points and 2^31 reading points in all (AICP_ERR_UNSUPPORTED).
 * One corner where a pair does not get the one-pair call's answer: a SurfaceNormal whose output is
 * used and whose knn is outside {10, 20, 30} (a chain the parser refuses) ends the whole call with
 * AICP_ERR_UNSUPPORTED as soon as any cloud of the side reaches it with a point, also for a pair that
 * the filters in front of it had emptied (the one-pair call on that pair: AICP_ERR_CONVERGENCE).
 * A chain with no filter but SurfaceNormal and the TrimmedDist rule takes aicp_hip_align_batch's
 * path and gives its bits. The call neither uses nor keeps the reference cache, and drops it. */
int aicp_hip_align_chain_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_chain* chain,
                               const aicp_pair* pairs, size_t n_pairs, double resolution, int flags,
                               float* out_T /* 16 * n_pairs */, aicp_icp_stats* stats /* n_pairs, nullable */,
                               aicp_chain_stats* chain_stats /* n_pairs, nullable */);

/* ---- registration / overlap (host buffers) ---------------------------------------------- */
int aicp_hip_register(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_pair* pair,
                      float out_T[16], aicp_icp_stats* stats /* nullable */);
int aicp_hip_register_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg,
                            const aicp_pair* pairs, size_t n_pairs,
                            float* out_T /* 16*n */, aicp_icp_stats* stats /* n, nullable */);
int aicp_hip_overlap(aicp_hip_ctx* ctx, const aicp_pair* pair, double resolution,
                     float* out_overlap_percent);
int aicp_hip_overlap_batch(aicp_hip_ctx* ctx, const aicp_pair* pairs, size_t n_pairs,
                           double resolution, float* out_overlap_percent /* n */,
                           aicp_icp_stats* stats /* n, nullable: overlap_keys */);
/* Reference cache of the one-shot calls above (register*, overlap*, align_batch). App registers
 * reading after reading against one reference (app.cpp:72-73; a new one every
 * reference_update_frequency readings, app.cpp:383-391) and calls computeOverlap then
 * registerClouds per reading (app.cpp:132-135, 205-210). When every pair of a call passes the same
 * reference array as the previous call -- (pointer, count, stride) equal and the points
 * byte-identical to a copy the context keeps -- the reference's centroid, kd-trees, treelets and
 * normals (ICP), and its voxel map for the same origin and resolution (overlap), stay resident in
 * the context and are reused; the reference is not uploaded again. Any other call that rewrites
 * those buffers (a batch with several references, the kernel-level entry points, the
 * pre-filter) drops the cache. Results are the same as without it.
 * out: tree hits, tree builds, overlap-map hits, overlap-map builds since the context's creation. */
int aicp_hip_reference_cache_stats(const aicp_hip_ctx* ctx, uint64_t out[4]);
/* App::runAicpPipeline hot path (app.cpp:218-247): overlap -> auto-tuned ratio -> ICP,
 * all on device, one launch sequence for the whole batch. cfg->trimmed_ratio is ignored
 * when flags has AICP_RUN_OVERLAP. */
int aicp_hip_align_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg,
                         const aicp_pair* pairs, size_t n_pairs, double resolution, int flags,
                         float* out_T /* 16*n */, aicp_icp_stats* stats /* n, nullable */);
/* ---- several GPUs from one host process (C5) ----------------------------------
 * Independent pairs shard across devices with no data-path exchange: one context and one host
 * thread per device, longest-processing-time shards by n_read * log2(n_ref), and the per-pair
 * results written at the pairs' own indices (the gather). Replaces nothing in the reference,
 * which registers one pair at a time on the CPU (app.cpp:528-550); it is the C++ host's form of
 * bench.py's torch.distributed path. devices = NULL: devices 0..n_devices-1 (n_devices <= 0:
 * every visible device); a device may be listed more than once (several contexts on one GPU). */
typedef struct aicp_hip_multi aicp_hip_multi;
int aicp_hip_multi_create(const int* devices, int n_devices, aicp_hip_multi** out);
void aicp_hip_multi_destroy(aicp_hip_multi* m);
int aicp_hip_multi_size(const aicp_hip_multi* m);
aicp_hip_ctx* aicp_hip_multi_context(aicp_hip_multi* m, int i);
const char* aicp_hip_multi_last_error(const aicp_hip_multi* m);
/* aicp_hip_align_batch over the devices; out_device (n, nullable): the device of each pair */
int aicp_hip_multi_align_batch(aicp_hip_multi* m, const aicp_icp_config* cfg, const aicp_pair* pairs,
                               size_t n_pairs, double resolution, int flags, float* out_T /* 16*n */,
                               aicp_icp_stats* stats /* n, nullable */, int* out_device /* n, nullable */);

/* getOutputReading: out = T * in (float, pad row 1), pointmatcher_registration.cpp:128-131. */
int aicp_hip_transform(aicp_hip_ctx* ctx, const float T[16], const float* in, size_t n,
                       size_t stride, float* out /* packed xyz, 3*n */);

/* Localization-only map crop, getPointsInOrientedBox (aicp_core/src/utils/filteringUtils.cpp:619-637,
 * called at app.cpp:41-51): pcl::CropBox with the cube [min, max]^3, rotation =
 * origin.R.eulerAngles(0,1,2) and translation = origin.t (origin: Matrix4f, col-major). Kept
 * points are written packed xyz in input order to out (capacity n points); *out_n = count.
 * Non-finite points are dropped. rpy_out (nullable) receives the box angles. */
int aicp_hip_crop_box(aicp_hip_ctx* ctx, const float* pts, size_t n, size_t stride, float min,
                      float max, const float origin[16], float* out /* 3*n */, size_t* out_n,
                      float* rpy_out /* 3, nullable */);

/* Pre-filter regionGrowingUniformPlaneSegmentationFilter (aicp_core/src/utils/filteringUtils.cpp:5-45,
 * called at app.cpp:109,295,491 and app_ros.cpp:309; the XYZRGBNormal overload :51-103 adds the
 * viewpoint, the sampled cloud with normals and the clusters): pcl::VoxelGrid (leaf 0.08) ->
 * pcl::NormalEstimation (k 30) -> pcl::RegionGrowing (15 neighbours, 3 deg, curvature 1.0,
 * clusters of 50..1e6 points). Rules for PCL's unspecified orders: DESIGN.md §4.4. */
typedef struct {
  float leaf_size;           /* VoxelGrid leaf, all three axes (0.08) */
  int32_t normal_k;          /* NormalEstimation k: 10, 20 or 30 (30) */
  int32_t neighbours;        /* RegionGrowing neighbours, <= min(16, normal_k) (15) */
  int32_t min_cluster_size;  /* 50 */
  int32_t max_cluster_size;  /* 1000000 */
  float smoothness_rad;      /* 3.0 / 180.0 * M_PI as float */
  float curvature_threshold; /* 1.0 */
  float viewpoint[3];        /* NormalEstimation viewpoint ((0,0,0): the first overload) */
} aicp_prefilter_params;
void aicp_hip_default_prefilter(aicp_prefilter_params* out);
/* out: the clusters' points concatenated (clusters in creation order, each in sampled-cloud
 * order), packed xyz, capacity n points; *out_n = count. Optional (nullable, capacity n):
 * sampled = 8 floats per sampled point {x, y, z, curvature, nx, ny, nz, 0}; labels = cluster of
 * each sampled point (-1: in no kept cluster). A cloud whose voxel grid would overflow 32-bit
 * indices passes unfiltered (as in PCL), which requires finite points (else
 * AICP_ERR_UNSUPPORTED). */
int aicp_hip_prefilter(aicp_hip_ctx* ctx, const aicp_prefilter_params* prm, const float* pts, size_t n,
                       size_t stride, float* out /* 3*n */, size_t* out_n, float* sampled /* 8*n */,
                       int32_t* labels /* n */, size_t* n_sampled /* nullable */,
                       size_t* n_clusters /* nullable */);

/* Timing of the last aicp_hip_prefilter (HIP events on the context stream). */
typedef struct {
  double voxel_ms;          /* VoxelGrid: bounds, keys, sort, centroids */
  double normals_ms;        /* kd-tree of the sampled cloud, kNN, normals */
  double segment_ms;        /* RegionGrowing: seed order, union-find, propagation (with its host
                               round trips), cluster extraction */
  double device_ms;         /* input uploaded -> clusters ready */
  double wall_ms;           /* the whole call: host packing, PCIe both ways */
  double knn_ms;            /* the kNN kernel alone */
  uint64_t knn_queries;     /* sampled points */
  uint64_t knn_points_touched, knn_nodes_touched;
  int32_t propagation_passes;
  int32_t pad;
} aicp_prefilter_stats;
int aicp_hip_last_prefilter_stats(const aicp_hip_ctx* ctx, aicp_prefilter_stats* out);

/* ---- alignment risk (failure_prediction_mode, App::computeAlignmentRisk, app.cpp:143-185) ------
 * The two features App feeds its classifier (app.cpp:179: octree_overlap_, alignability_) and
 * fov_overlap_. The classifier itself, the gate it drives and the gated stream follow below
 * (aicp_hip_svm_*, aicp_hip_pipeline, aicp_hip_sequence_run_risk).
 * Poses are column-major double[16] (Eigen::Isometry3d::data()). Rules and the one deliberate
 * deviation (the clamped cosine): DESIGN.md §4.5. */

/* overlapFilter (aicp_core/src/utils/filteringUtils.cpp:111-193): cloud A is filtered in pose B's
 * frame and cloud B in pose A's: a point is kept when |atan2(y, x)| < 180 - (360 - angular_view)/2
 * degrees and its distance < range; kept points go back to the global frame (float) in input
 * order. *fov_overlap = 100 * kept_A/|A| * kept_B/|B| (float). accepted_a / accepted_b: packed
 * xyz, capacity |A| / |B| points, nullable. An input cloud of 0 points is AICP_ERR_INVALID (the
 * reference divides by zero). */
int aicp_hip_fov_overlap(aicp_hip_ctx* ctx, const aicp_cloud* cloud_a, const aicp_cloud* cloud_b,
                         const double pose_a[16], const double pose_b[16], float range, float angular_view,
                         float* fov_overlap, float* accepted_a /* 3*|A|, nullable */, size_t* n_accepted_a,
                         float* accepted_b /* 3*|B|, nullable */, size_t* n_accepted_b);

typedef struct {
  float range;              /* sensor range, metres (the caller's configuration) */
  float angular_view;       /* field of view, degrees */
  float max_angle_deg;      /* matching: largest angle between mean normals, 20 (filteringUtils.cpp:258) */
  float box_scale[3];       /* overlapBoxFilter's enlargement of the box, (1, 1, 3) (:520-528) */
  aicp_prefilter_params prefilter; /* the viewpoint is overwritten with each pose's translation (:72) */
} aicp_risk_params;
void aicp_hip_default_risk_params(aicp_risk_params* out);

/* One cluster's oriented box: MomentOfInertiaEstimation::getOBB (axes = eigenvectors of the
 * covariance, major / middle = minor x major / minor as columns of rot, row-major) after
 * overlapBoxFilter's scaling; half = the symmetric max point. */
typedef struct {
  double centre[3];
  double rot[9];
  double half[3];
} aicp_risk_box;

/* The matching and PCA of alignabilityFilter (filteringUtils.cpp:222-430) on two pre-filtered
 * clouds in the layout aicp_hip_prefilter returns (sampled: 8 floats per point, labels: cluster or
 * -1; clusters = 1 + the largest label). The kernel-level test surface of the risk kernels.
 * Outputs (each nullable): matching_indeces / matching_overlap / matching_distance per cluster of
 * B (-1: no match); eigenvalues (normalised, descending), eigenvectors (row-major, column k for
 * eigenvalue k), centroid of A's matched planes; boxes per cluster; cnt_a_in_box_b [clusters_B]
 * [clusters_A] and cnt_b_in_box_a [clusters_A][clusters_B]. More than 4096 clusters in a cloud or
 * clusters_A * clusters_B > 2^22: AICP_ERR_UNSUPPORTED. Zero clusters on a side: alignability 0. */
int aicp_hip_cluster_match(aicp_hip_ctx* ctx, const float* sampled_a, const int32_t* labels_a, size_t n_a,
                           const float* sampled_b, const int32_t* labels_b, size_t n_b, float max_angle_deg,
                           const float box_scale[3], float* alignability, int32_t* n_matches,
                           int32_t* matching_indeces, float* matching_overlap, float* matching_distance,
                           double eigenvalues[3], double eigenvectors[9], double centroid[3],
                           aicp_risk_box* boxes_a, aicp_risk_box* boxes_b, uint32_t* cnt_a_in_box_b,
                           uint32_t* cnt_b_in_box_a);

typedef struct {
  float fov_overlap;        /* overlapFilter's value */
  float alignability;       /* alignabilityFilter's value; 0 with no matching planes (:344-348) */
  uint64_t accepted_a, accepted_b; /* points the FOV filter kept */
  uint32_t sampled_a, sampled_b;   /* points of the two sampled clouds */
  int32_t clusters_a, clusters_b;
  int32_t n_matches;
  int32_t pad;
  double eigenvalues[3];    /* normalised, descending */
  double eigenvectors[9];   /* row-major, column k for eigenvalue k */
  double centroid[3];       /* of A's matched planes (the reference's `eigenvectors` cloud, :402-424) */
} aicp_risk_result;

/* computeAlignmentRisk up to the classifier: overlapFilter -> regionGrowingUniformPlane-
 * SegmentationFilter of both accepted clouds (viewpoint = the pose's translation) -> matching
 * and PCA, chained on the device: the accepted clouds, sampled clouds and labels never cross to
 * the host (the host reads the accepted and cluster counts to size launches, and the result).
 * planes_a / planes_b (nullable, capacity planes_cap points of 8 floats: x, y, z, nx, ny, nz,
 * cluster index, 0): the matched planes of both clouds (cloudA_planes / cloudB_planes, :314-315;
 * the index stands where the reference puts a random colour), in matching order. An accepted cloud
 * of 0 points or zero clusters on a side: AICP_OK with alignability 0. */
int aicp_hip_alignment_features(aicp_hip_ctx* ctx, const aicp_risk_params* prm, const aicp_cloud* cloud_a,
                                const aicp_cloud* cloud_b, const double pose_a[16], const double pose_b[16],
                                aicp_risk_result* out, float* planes_a, size_t* n_planes_a, float* planes_b,
                                size_t* n_planes_b, size_t planes_cap);

/* Timing of the last aicp_hip_alignment_features (HIP events on the context stream). */
typedef struct {
  double fov_ms;            /* both FOV filters */
  double prefilter_a_ms, prefilter_b_ms; /* hand-off copy, pre-filter, gather */
  double clusters_ms;       /* moments + boxes of both clouds */
  double counts_ms;         /* both count matrices */
  double match_ms;          /* matching + PCA */
  double device_ms;         /* inputs uploaded -> result ready */
  double wall_ms;           /* the whole call */
} aicp_risk_stats;
int aicp_hip_last_risk_stats(const aicp_hip_ctx* ctx, aicp_risk_stats* out);

/* ---- the classifier of failure_prediction_mode (aicp_core/src/classification/svm.cpp) ------------
 * App's SVM: an OpenCV model file (two classes, two variables: octree overlap in percent and
 * alignability, POLY kernel), evaluated as cv::ml::SVM::predict(..., RAW_OUTPUT) and mapped to a
 * risk in [0, 1] (svm.cpp:82). Per sample x and support vector v, in this order:
 *   s = (double)(v0 * x0) + (double)(v1 * x1), the products in float;
 *   base = (float)(s * gamma + coef0);  K = (float)pow((double)base, degree);
 *   sum = -rho + sum_j alpha[j] * K[index[j]] in double;  raw = (float)sum;
 *   risk = 1.0 - 1.0 / (1.0 + exp(-(double)raw)).
 * The double sum runs in a fixed order (lane l of a wave takes entries l, l + 64, ..., a shuffle
 * tree joins the lanes, -rho is added last): a result depends on its input alone. */
typedef struct aicp_hip_svm aicp_hip_svm;
typedef struct {
  int32_t format;      /* 3: <opencv_ml_svm> with <format>3</format>; 0: the older <my_svm> root */
  int32_t var_count, class_count;
  int32_t sv_total;    /* support vectors in the file */
  int32_t sv_count;    /* entries of the one decision function */
  int32_t has_index;   /* 0: the file has no <index>, which means the identity */
  double degree, gamma, coef0, rho;
} aicp_svm_info;
/* Host only (no device needed), the project's own small reader of the model XML. Read: svmType (or
 * svm_type), kernel/type, degree, gamma, coef0, var_count, class_count, sv_total, support_vectors and
 * of the one decision function sv_count, rho, alpha, index; class_labels and everything else is read
 * past. AICP_ERR_UNSUPPORTED: anything but C_SVC / POLY / 2 classes / var_count 2, or more than 2048
 * decision-function entries; AICP_ERR_INVALID: a file that cannot be read or does not parse, a
 * support-vector count that is not sv_total, sv_count != len(alpha), len(index) != sv_count, an
 * index entry outside [0, sv_total). */
int aicp_hip_svm_load(const char* path, aicp_hip_svm** out);
void aicp_hip_svm_free(aicp_hip_svm* model);
/* the parsed model: support_vectors 2 * sv_total floats, alpha and index sv_count each (nullable) */
int aicp_hip_svm_info(const aicp_hip_svm* model, aicp_svm_info* out, float* support_vectors, double* alpha,
                      int32_t* index);
/* n samples (overlap percent, alignability) in one launch, one wave per sample. The model's arrays
 * are uploaded on a context's first call with that model and stay there (a freed model's copy is
 * dropped with the context). raw (nullable): n floats; risk: n doubles. n = 0 is AICP_OK. */
int aicp_hip_svm_predict(aicp_hip_ctx* ctx, const aicp_hip_svm* model, const float* samples /* 2*n */, size_t n,
                         float* raw /* n, nullable */, double* risk /* n */);

/* App::runAicpPipeline with failure_prediction_mode (app.cpp:218-247) for one pair of pre-filtered
 * clouds: (1) the octree overlap at `resolution` with the poses' translations as sensor origins
 * (App hands the same Isometry3d to both steps: pair->ref_origin / read_origin are not read);
 * (2) aicp_hip_alignment_features on (reference, reading) with (ref_pose, read_pose);
 * (3) the classifier on ((float)overlap, (float)alignability); (4) registerClouds at the auto-tuned
 * ratio when risk <= threshold. Overlap and alignability stay in device memory; one launch of the
 * classifier's kernel reads them there and writes raw, risk, the gate !(risk <= threshold) (a NaN
 * risk gates, as in C++) and the ratio aicp_hip_autotune_ratio(overlap): no host arithmetic stands
 * between the features and the decision, the host reads the record back and enqueues the ICP with the
 * device's ratio, or does not. A gated pair leaves out_T the identity, stats->iterations 0 and
 * stats->status AICP_OK. rec + out_T are aicp_test's result line (aicp_test.cpp:187-198). */
typedef struct {
  uint64_t n_read;        /* points of the (pre-filtered) reading */
  float fov_overlap;      /* overlapFilter's value */
  float octree_overlap;   /* percent */
  float alignability;
  float raw;              /* the decision function's value */
  double risk;
  int32_t registered;     /* 1: risk <= threshold, the ICP ran; 0: gated */
  float trimmed_ratio;    /* aicp_hip_autotune_ratio(octree_overlap), computed on the device */
} aicp_pipeline_record;
int aicp_hip_pipeline(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_risk_params* risk_prm,
                      const aicp_hip_svm* model, double threshold, const aicp_pair* pair, const double ref_pose[16],
                      const double read_pose[16], double resolution, float out_T[16], aicp_pipeline_record* rec,
                      aicp_icp_stats* stats /* nullable */);

/* ---- registration quality monitor (aicp_core/src/utils/icpMonitor.cpp) -------------------------
 * What PointmatcherRegistration would print with pointmatcher.printOutputStatistics
 * (pointmatcher_registration.cpp:138-150, common.hpp:21): how good an alignment is, with no ground
 * truth. ref is the reference, out the reading after alignment; with T (column-major, nullable)
 * out = T * cloud is computed on the device first, in aicp_hip_transform's arithmetic. Trees are
 * built over the coordinates as given (no centring, as aicp_hip_knn). Rules: DESIGN.md §4.6.
 *   hausdorffDistance (:12-81): KDTreeMatcher knn 1, epsilon 0, both directions ([0]: tree on ref,
 *     queries from out; [1]: tree on out, queries from ref); per direction max_d2 =
 *     getDistsQuantile(1.0), quantile_d2 = getDistsQuantile(quantile); hausdorff =
 *     sqrt(max(max_d2[0], max_d2[1])), hausdorff_quantile = sqrt(max(quantile_d2[0], quantile_d2[1])).
 *   distancesKNN(ref, out) (:89-138): d = sqrtf(d2) of direction 0; valid when (double)d <=
 *     max_accepted_dist; knn_mean_dist = sum d / knn_valid (NaN with knn_valid = 0: the reference
 *     divides 0 by 0).
 *   pairedPointsMeanDistance (:146-231), with AICP_MON_PAIRED: the chain's matcher (cfg->nn_epsilon,
 *     nn_max_dist, bucket_size; tree on ref, queries from out) and its TrimmedDist filter:
 *     paired_limit_d2 = getDistsQuantile(cfg->trimmed_ratio), a pair is kept when d2 <= limit,
 *     paired_mean_dist = sum sqrtf(d2) / paired_kept, from the matcher's own d2. Without the flag,
 *     or when the matcher found nothing within nn_max_dist: NaN, NaN and 0.
 * The sums are fp64 in a fixed order: results are byte-identical across runs, contexts and batch
 * compositions. */
typedef struct {
  float quantile;           /* hausdorffDistance's robust quantile, in [0, 1] (0.60) */
  double max_accepted_dist; /* distancesKNN's maxAcceptedDist (0.20) */
  int32_t flags;            /* AICP_MON_PAIRED */
} aicp_monitor_params;
#define AICP_MON_PAIRED 1   /* also the chain-matcher paired mean (needs cfg) */
/* 56 bytes, no implicit padding (pad is 0): two results compare with memcmp */
typedef struct {
  float hausdorff, hausdorff_quantile;   /* metres */
  float max_d2[2], quantile_d2[2];       /* squared metres; [0] out -> ref, [1] ref -> out */
  float knn_mean_dist;
  int32_t pad;
  uint64_t knn_valid;
  float paired_mean_dist, paired_limit_d2;
  uint64_t paired_kept;
} aicp_monitor_result;
void aicp_hip_default_monitor_params(aicp_monitor_params* out);
/* dist_out (|out| floats) / dist_ref (|ref| floats), nullable: sqrtf(d2) per point of out (direction
 * 0) and of ref (direction 1), the values1 / values2 arrays the reference writes to VTK.
 * AICP_ERR_INVALID: a null argument, a cloud of 0 points, a stride below 12 or no multiple of 4, a
 * quantile outside [0, 1], AICP_MON_PAIRED without cfg; AICP_ERR_UNSUPPORTED: a kd-tree deeper than
 * the device stack (48 levels), more than 2^28 points in a call; AICP_ERR_CONVERGENCE: a direction
 * with no finite distance (non-finite coordinates). */
int aicp_hip_monitor(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg /* nullable */,
                     const aicp_cloud* ref, const aicp_cloud* out, const float T[16] /* nullable */,
                     aicp_monitor_result* result, float* dist_out /* nullable */, float* dist_ref /* nullable */);
/* n pairs (ref, read = out or the cloud T moves; init_T and the origins are not read) in one launch
 * sequence: all trees in one device build, one 1-NN launch for the exact searches and one for the
 * chain matcher's, one reduction. T: 16 floats per pair, nullable. At most 4096 pairs. Nothing but
 * the results crosses back to the host. */
int aicp_hip_monitor_batch(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg /* nullable */,
                           const aicp_pair* pairs, size_t n, const float* T /* 16*n, nullable */,
                           aicp_monitor_result* out /* n */);
/* Timing of the last monitor call (HIP events on the context stream). */
typedef struct {
  double trees_ms;          /* transform + every kd-tree */
  double nn_ms;             /* the 1-NN launches */
  double reduce_ms;         /* selects, reduction, results */
  double device_ms;         /* inputs uploaded -> results ready */
  double wall_ms;           /* the whole call */
} aicp_monitor_stats;
int aicp_hip_last_monitor_stats(const aicp_hip_ctx* ctx, aicp_monitor_stats* out);

/* ---- device-resident prior map (localization mode) ------------------------------------------
 * App keeps prior_map_ and, per reading, crops it around the prior pose (setReference,
 * app.cpp:41-51), appends the aligned reference reading every reference_update_frequency clouds
 * (merge_aligned_clouds_to_map, app.cpp:469-483: *merged = *prior_map + *output, output =
 * transformPointCloud(read_prefiltered, correction)) and pre-filters the whole map every 30
 * clouds (app.cpp:485-493). The map stays in HBM: crop, merge and pre-filter run on it without
 * re-uploading it. */
typedef struct aicp_hip_map aicp_hip_map;
int aicp_hip_map_create(aicp_hip_ctx* ctx, const float* pts, size_t n, size_t stride, aicp_hip_map** out);
void aicp_hip_map_free(aicp_hip_ctx* ctx, aicp_hip_map* map);
int aicp_hip_map_size(const aicp_hip_map* map, size_t* n);
/* the map's points, packed xyz (capacity cap points) */
int aicp_hip_map_download(aicp_hip_ctx* ctx, const aicp_hip_map* map, float* out, size_t cap, size_t* out_n);
/* getPointsInOrientedBox on the map (aicp_hip_crop_box semantics), kept points to out */
int aicp_hip_map_crop(aicp_hip_ctx* ctx, const aicp_hip_map* map, float min, float max, const float origin[16],
                      float* out /* 3*cap */, size_t cap, size_t* out_n);
/* Localization-only batch (localize_against_prior_map, app.cpp:41-51,123-127): reading i is
 * registered against the map cropped on the device to [min, max]^3 around its prior pose
 * poses[16 i .. 16 i + 15] (getPointsInOrientedBox, Matrix4f column-major); the crop goes straight
 * into the batch's reference array (no host round trip). The overlap is fixed at 50 %, so the
 * trimmed ratio is aicp_hip_autotune_ratio(50) = 0.5 whatever cfg->trimmed_ratio says.
 * flags: AICP_RUN_TIME_NN only. An empty crop is AICP_ERR_INVALID. */
int aicp_hip_map_register_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_hip_map* map, float min,
                                float max, const aicp_cloud* readings, const float* poses /* 16*n */, size_t n,
                                int flags, float* out_T /* 16*n */, aicp_icp_stats* stats /* n, nullable */);
/* map += T * pts (pcl::transformPointCloud, T column-major float[16]) */
int aicp_hip_map_merge(aicp_hip_ctx* ctx, aicp_hip_map* map, const float* pts, size_t n, size_t stride,
                       const float T[16]);
/* map = regionGrowingUniformPlaneSegmentationFilter(map) (aicp_hip_prefilter on device data) */
int aicp_hip_map_prefilter(aicp_hip_ctx* ctx, aicp_hip_map* map, const aicp_prefilter_params* prm);

/* ---- sweep accumulator: a raw reading assembled in HBM ----------------------------------------
 * VelodyneAccumulatorROS::processLidar (aicp_ros/src/velodyne_accumulator.cpp:31-73) per sweep:
 *   getPointsInOrientedBox(sweep, crop_min, crop_max, Identity): non-finite points dropped, the
 *     cube inclusive;
 *   pcl::transformPointCloud(sweep, pose.translation().cast<float>(),
 *                            Quaternionf(pose.rotation().cast<float>())): x' = r00 x + r01 y +
 *     r02 z + t0 in float, in that order, no FMA (aicp_hip_transform's expression) with the
 *     matrix of aicp_hip_accum_pose_matrix;
 *   accumulated_point_cloud_ += sweep, and after batch_size sweeps the accumulator is finished.
 * A sweep is uploaded when it is pushed and cropped, moved and appended on the device; the raw
 * reading never exists on the host. The counts live on the device: push does not synchronise the
 * host with the device, state / download / prefilter do. One accumulator is driven from one thread
 * at a time, on its context's stream. */
typedef struct aicp_hip_accum aicp_hip_accum;
typedef struct {
  int32_t batch_size;       /* 80 (aicp_ros_node.cpp:40); aicp.launch uses 7 */
  float crop_min, crop_max; /* -30, 30 (velodyne_accumulator.cpp:60) */
} aicp_accum_params;
void aicp_hip_default_accum_params(aicp_accum_params* p);
/* capacity_points: the most input points (kept or not) one reading's sweeps may add up to */
int aicp_hip_accum_create(aicp_hip_ctx* ctx, const aicp_accum_params* prm, size_t capacity_points,
                          aicp_hip_accum** out);
void aicp_hip_accum_free(aicp_hip_ctx* ctx, aicp_hip_accum* acc);
/* One sweep: n rows of `stride` bytes (>= 12, a multiple of 4), xyz first; pose: Isometry3d
 * (inertial <- sensor), column-major double[16]. The rows are copied into a pinned slot of the
 * accumulator before the call returns (rows of 12 or 16 bytes as they are, wider rows packed), the
 * upload and the two kernels are enqueued on the context's stream, and nothing is waited for but a
 * slot's own earlier upload. The host keeps only the sum of every n since the last clear: a push
 * that takes it past capacity_points is AICP_ERR_INVALID and changes nothing. A finished
 * accumulator ignores the push (AICP_OK), as processLidar does; n = 0 counts as a sweep. */
int aicp_hip_accum_push(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const float* pts, size_t n, size_t stride,
                        const double pose[16]);
/* waits for the stream. counter: sweeps taken, finished: counter == batch_size, n_points: the
 * accumulated cloud's size, kept_per_sweep (nullable, batch_size words): each sweep's kept points
 * (0 from `counter` on). Every output is nullable. */
int aicp_hip_accum_state(aicp_hip_ctx* ctx, aicp_hip_accum* acc, int32_t* counter, int32_t* finished,
                         size_t* n_points, uint32_t* kept_per_sweep);
/* clearCloud(): nothing is waited for */
int aicp_hip_accum_clear(aicp_hip_ctx* ctx, aicp_hip_accum* acc);
/* getCloud(): packed xyz (capacity cap points); waits for the stream */
int aicp_hip_accum_download(aicp_hip_ctx* ctx, aicp_hip_accum* acc, float* out, size_t cap, size_t* out_n);
/* regionGrowingUniformPlaneSegmentationFilter of the accumulated cloud where it lies
 * (aicp_hip_prefilter on device data; the accumulator is left as it is). T (nullable, column-major
 * float[16]): the cloud is first moved by it as aicp_hip_transform moves it (setAndFilterReading's
 * debug branch, app.cpp:87-99). out: the kept points, packed xyz, capacity cap points
 * (AICP_ERR_INVALID if they do not fit). aicp_hip_last_prefilter_stats describes the call. */
int aicp_hip_accum_prefilter(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const aicp_prefilter_params* prm,
                             const float T[16], float* out, size_t cap, size_t* out_n);
/* Host only, no device needed. The sweep's float transform (velodyne_accumulator.cpp:62-63):
 * R = Quaternionf(pose.rotation().cast<float>()).toRotationMatrix() (Eigen 3.3: rotation() is the
 * linear part as it stands; Eigen's trace / largest-diagonal branches in float, no normalisation),
 * t = pose.translation().cast<float>(); out_T = [R | t], column-major. */
void aicp_hip_accum_pose_matrix(const double pose[16], float out_T[16]);
/* AppROS::velodyneCallBack's test that the robot moved since the last reading (app_ros.cpp:203-213):
 * with rel = prev_pose^-1 * pose (the Isometry inverse: R^T, -R^T t), 1 if |rel.translation| >
 * min_dist (1.0) or any of |roll|, |pitch|, |yaw| of quat_to_euler(Quaterniond(rel.rotation)) >
 * min_angle_rad (10 degrees), else 0. */
int aicp_hip_motion_gate(const double prev_pose[16], const double pose[16], double min_dist, double min_angle_rad);

/* App's localization stream on the map (localize_against_prior_map: aicp_localization_only.launch,
 * processCloud app.cpp:282-414 with the aligned-cloud graph empty at the start, so the "first
 * cloud" branch app.cpp:286-289 is skipped). State: the map, n_clouds = 0
 * (aligned_clouds_graph_->getNbClouds()), initialT_ = I. For reading i with prior pose P_i:
 *   1. reference = getPointsInOrientedBox(map, crop_min, crop_max, P_i) (app.cpp:41-58), from the
 *      prior pose as given (setReference runs before setAndFilterReading, app.cpp:333, 337);
 *   2. AICP_SEQ_DEBUG only: reading = transformPointCloud(reading, initialT_) (float) and the prior
 *      pose becomes initialT_ * prior pose (app.cpp:87-96); clouds come in pre-filtered, with
 *      aicp_hip_sequence_run's caveat about the filter order;
 *   3. ICP at the ratio aicp_hip_autotune_ratio(50) (the overlap is bypassed at 50 %,
 *      app.cpp:123-127). An empty crop is AICP_ERR_INVALID for that reading. A non-zero status ends
 *      the stream at that reading (app.cpp:210); everything before it stays committed;
 *   4. the reading is dropped when n_clouds != 0 and some |T(k,3)| > max_correction_magnitude
 *      (app.cpp:366-373, float compare); a dropped reading changes nothing;
 *   5. accepted: ++n_clouds, corrected_origin = translation(correction * prior pose) as
 *      aicp_hip_sequence_run computes it, initialT_ = correction * initialT_ (app.cpp:414);
 *   6. with AICP_LOC_MERGE and (n_clouds - 1) % reference_update_frequency == 0:
 *      map += transformPointCloud(reading, correction) (app.cpp:375, 469-483; the moved reading in
 *      debug mode), so the first accepted reading merges;
 *   7. with AICP_LOC_MERGE and (n_clouds - 1) % map_refilter_every == 0:
 *      map = regionGrowingUniformPlaneSegmentationFilter(map), after that reading's merge
 *      (app.cpp:485-493, where the period is 30).
 * Readings between two map changes are independent and run as one batch (a window, see
 * aicp_hip_localization_window); the decisions 4-7 are taken on the device, the merged reading is
 * appended from the batch's device copy by the device's own correction, and the host reads one
 * record per reading once per window. */
#define AICP_LOC_MERGE 16       /* aicp_localization_params.flags: merge_aligned_clouds_to_map */
typedef struct {
  int32_t reference_update_frequency; /* 5 (aicp_localization_only.launch) */
  int32_t map_refilter_every;         /* 30 (app.cpp:485); 0: never */
  float max_correction_magnitude;     /* 1.0 */
  float crop_min, crop_max;           /* -15, 15: the crop cube around the prior pose */
  int32_t flags;                      /* AICP_LOC_MERGE | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN */
} aicp_localization_params;
/* 128 bytes, no implicit padding */
typedef struct {
  int32_t status;          /* AICP_* of this reading's registration */
  int32_t accepted;        /* 0: dropped */
  int32_t merged;          /* 1: appended to the map */
  int32_t refiltered;      /* 1: the map was pre-filtered after this reading */
  uint64_t map_points;     /* size of the map it was cropped from */
  uint64_t crop_points;    /* size of its reference */
  double corrected_origin[3]; /* as aicp_sequence_result (accepted readings) */
  aicp_icp_stats icp;
} aicp_localization_result;
typedef struct {
  int32_t windows;         /* batches run */
  int32_t merges, refilters;
  int32_t pad;
  double wall_ms;          /* the whole call */
  double device_ms;        /* first crop enqueued -> last map change done (HIP events) */
} aicp_localization_timing;
void aicp_hip_default_localization_params(aicp_localization_params* out);
/* Host-only: the length of the next window when n_clouds readings have been accepted and
 * `remaining` are left: debug mode 1; else min(remaining, 4096, k) with k the smallest k >= 1 such
 * that (n_clouds + k - 1) % reference_update_frequency == 0 or (n_clouds + k - 1) %
 * map_refilter_every == 0 (each only with AICP_LOC_MERGE, the second only when the period is not 0;
 * without AICP_LOC_MERGE k is unbounded). If every reading of the window is accepted the map
 * changes exactly after its last one; if some are dropped it does not change and the next window is
 * shorter; nothing is ever run twice. 0 for invalid parameters or remaining = 0. */
size_t aicp_hip_localization_window(uint64_t n_clouds, const aicp_localization_params* prm, size_t remaining);
/* readings: aicp_cloud[n] (origin = the prior pose's translation); poses: 16*n floats, column-major,
 * as aicp_hip_map_register_batch; pf: the re-filter's parameters (nullable: the defaults). The map
 * is updated in place (a failed growth leaves it as it was). out_T / out / n_done as
 * aicp_hip_sequence_run: *n_done = readings processed, the return value the status that ended the
 * stream (at reading *n_done - 1) or AICP_OK. */
int aicp_hip_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                              const aicp_prefilter_params* pf, aicp_hip_map* map, const aicp_cloud* readings,
                              const float* poses /* 16*n */, size_t n, float* out_T /* 16*n */,
                              aicp_localization_result* out /* n */, size_t* n_done);
int aicp_hip_last_localization_timing(const aicp_hip_ctx* ctx, aicp_localization_timing* out);

/* ---- localization against the map App has built itself (localize_against_built_map) ----------
 * The batch: as aicp_hip_map_register_batch (crops straight into the batch's reference array, an
 * empty crop is AICP_ERR_INVALID), but the overlap is not bypassed (app.cpp:123-135). flags:
 * AICP_RUN_OVERLAP | AICP_RUN_TIME_NN (AICP_RUN_ICP is always on). With AICP_RUN_OVERLAP pair i's
 * octree overlap at `resolution` is computed between its device crop (sensor origin
 * poses[16 i + 12 .. 14]) and its reading (sensor origin readings[i].origin), its ratio is
 * aicp_hip_autotune_ratio(overlap), and stats[i].overlap_percent / trimmed_ratio / overlap_keys are
 * filled as aicp_hip_align_batch fills them. Without it the ratio is cfg->trimmed_ratio and
 * overlap_percent is -1. */
int aicp_hip_map_align_batch(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_hip_map* map, float min,
                             float max, const aicp_cloud* readings, const float* poses /* 16*n */, size_t n,
                             double resolution, int flags, float* out_T /* 16*n */,
                             aicp_icp_stats* stats /* n, nullable */);
/* points the map's buffer holds before the next append has to grow it (a map is created with
 * room for its cloud only; a growth copies the map into a buffer of at least twice the size) */
int aicp_hip_map_capacity(const aicp_hip_map* map, size_t* n);

/* App's stream in this mode (processCloud app.cpp:282-414 with setReference app.cpp:60-69). The
 * caller creates the map from App's first cloud, already pre-filtered (app.cpp:293-310:
 * aligned_map_ = first cloud). State: the map, acc = 0 (readings accepted since the last
 * reference), initialT_ = I. For reading i with prior pose P_i:
 *   1. reference = getPointsInOrientedBox(map, crop_min, crop_max, P_i), reference pose P_i as
 *      given (setReference runs before setAndFilterReading, app.cpp:333, 337: in debug mode the
 *      crop and the reference's sensor origin use the unmoved pose). An empty crop is
 *      AICP_ERR_INVALID for that reading;
 *   2. AICP_SEQ_DEBUG only: reading = transformPointCloud(reading, initialT_) (float) and its
 *      sensor origin becomes the translation of initialT_ * prior pose (app.cpp:87-96);
 *   3. with AICP_RUN_OVERLAP the octree overlap at `resolution` between the crop (origin: the
 *      translation of P_i as given) and the reading (origin: its, possibly moved, prior-pose
 *      translation) and the auto-tuned ratio from it (app.cpp:132-135); without, cfg->trimmed_ratio.
 *      Then ICP. A non-zero status ends the stream at that reading (app.cpp:210); everything before
 *      it stays committed;
 *   4. the reading is dropped when some |T(k,3)| > max_correction_magnitude (app.cpp:366-373, float
 *      compare). getNbClouds() != 0 always holds (the graph holds the first cloud), so the first
 *      reading can be dropped too. A dropped reading changes nothing;
 *   5. accepted: corrected_origin as aicp_hip_sequence_run computes it, ++acc; when acc ==
 *      reference_update_frequency the reading becomes a reference (app.cpp:383-391, 458-465):
 *      map += transformPointCloud(reading, correction) (the moved reading in debug mode), acc = 0;
 *      initialT_ = correction * initialT_ (app.cpp:414);
 *   6. the map is never re-filtered (app.cpp:487 is guarded by localize_against_prior_map).
 * Readings between two map changes are independent and run as one window through the batch above
 * (aicp_hip_built_map_window); the decisions 4-5 are taken on the device, the reference reading
 * is appended from the batch's device copy by the device's own correction, and the host reads one
 * record per reading once per window. No reading crosses the bus a second time. */
typedef struct {
  int32_t reference_update_frequency; /* 5 */
  float max_correction_magnitude;     /* 1.0 */
  float crop_min, crop_max;           /* -15, 15: the crop cube around the prior pose */
  double resolution;                  /* 0.2: the overlap's octree */
  int32_t flags;                      /* AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN; default AICP_RUN_OVERLAP */
  int32_t pad;
} aicp_built_map_params;
/* 128 bytes, no implicit padding */
typedef struct {
  int32_t status;          /* AICP_* of this reading's registration */
  int32_t accepted;        /* 0: dropped */
  int32_t is_reference;    /* 1: appended to the map (the reference_update_frequency-th accepted) */
  int32_t pad;
  uint64_t map_points;     /* size of the map it was cropped from */
  uint64_t crop_points;    /* size of its reference */
  double corrected_origin[3]; /* as aicp_sequence_result (accepted readings) */
  aicp_icp_stats icp;
} aicp_built_map_result;
typedef struct {
  int32_t windows;         /* batches run */
  int32_t appends;         /* references appended to the map */
  double wall_ms;          /* the whole call */
  double device_ms;        /* first crop enqueued -> last append done (HIP events) */
} aicp_built_map_timing;
void aicp_hip_default_built_map_params(aicp_built_map_params* out);
/* Host-only: the length of the next window when acc readings have been accepted since the last
 * reference and `remaining` are left: debug mode 1; else min(remaining, 4096,
 * reference_update_frequency - acc). If every reading of the window is accepted the map changes
 * exactly after its last one; if some are dropped it does not change and the next window is
 * shorter; nothing is ever run twice. 0 for invalid parameters, acc >= reference_update_frequency
 * or remaining = 0. */
size_t aicp_hip_built_map_window(uint64_t acc, const aicp_built_map_params* prm, size_t remaining);
/* readings / poses / out_T / out / n_done as aicp_hip_map_sequence_run. The map is updated in place
 * (a failed growth leaves it as it was). */
int aicp_hip_built_map_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_built_map_params* prm,
                                    aicp_hip_map* map, const aicp_cloud* readings, const float* poses /* 16*n */,
                                    size_t n, float* out_T /* 16*n */, aicp_built_map_result* out /* n */,
                                    size_t* n_done);
int aicp_hip_last_built_map_timing(const aicp_hip_ctx* ctx, aicp_built_map_timing* out);

/* Both streams from RAW readings, in App's own order (processCloud calls setAndFilterReading,
 * app.cpp:77-100, for every reading). Every rule of aicp_hip_map_sequence_run /
 * aicp_hip_built_map_sequence_run holds unchanged (the crop by the pose as given, overlap and ratio,
 * the drop test, counts, merge / append, re-filter, the windows, an error ending the stream); only
 * the reading differs:
 *   robot mode:     reading = prefilter(raw);
 *   AICP_SEQ_DEBUG: reading = prefilter(transformPointCloud(raw, initialT_)) with prior pose
 *                   initialT_ * prior pose (app.cpp:87-99). The filtered reading is not moved again.
 * The map append (T * reading) takes this filtered reading (App's read_prefiltered), in debug mode
 * the moved one. pf_read (required) is used as given, viewpoint included, as
 * aicp_hip_sequence_run_raw uses its pf; an unsupported pf_read is refused before anything runs.
 * pf_map: the prior map's re-filter (nullable: the defaults). Per window every raw reading is
 * uploaded (rows of at most 16 bytes as they are, wider rows packed on the host), unpacked and, in
 * debug mode, moved by the device's initialT_ (k_stream_ingest), pre-filtered, and its kept points
 * are handed to the batch on the device: they never come back to the host.
 * A reading the pre-filter empties has status AICP_ERR_INVALID and an identity out_T and ends the
 * stream there, exactly as an empty crop does (the readings before it in the window still run); of
 * an empty crop and an emptied reading in one window the lower reading index ends the stream (at
 * the same reading: the pre-filter's). out_kept (nullable): n counts, the points reading i kept;
 * 0 for the readings behind *n_done. Point-to-point chains as in the pre-filtered streams. */
int aicp_hip_map_sequence_run_raw(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* prm,
                                  const aicp_prefilter_params* pf_map, const aicp_prefilter_params* pf_read,
                                  aicp_hip_map* map, const aicp_cloud* readings /* RAW */,
                                  const float* poses /* 16*n */, size_t n, float* out_T /* 16*n */,
                                  aicp_localization_result* out /* n */, uint32_t* out_kept /* n, nullable */,
                                  size_t* n_done);
int aicp_hip_built_map_sequence_run_raw(aicp_hip_ctx* ctx, const aicp_icp_config* cfg,
                                        const aicp_built_map_params* prm, const aicp_prefilter_params* pf_read,
                                        aicp_hip_map* map, const aicp_cloud* readings /* RAW */,
                                        const float* poses /* 16*n */, size_t n, float* out_T /* 16*n */,
                                        aicp_built_map_result* out /* n */, uint32_t* out_kept /* n, nullable */,
                                        size_t* n_done);

/* ---- device-resident batches (inputs uploaded once, run many times) ----------------------- */
int aicp_hip_batch_upload(aicp_hip_ctx* ctx, const aicp_pair* pairs, size_t n_pairs,
                          aicp_hip_batch** out);
int aicp_hip_batch_run(aicp_hip_ctx* ctx, aicp_hip_batch* batch, const aicp_icp_config* cfg,
                       double resolution, int flags, float* out_T /* 16*n */,
                       aicp_icp_stats* stats /* n, nullable */);
void aicp_hip_batch_free(aicp_hip_ctx* ctx, aicp_hip_batch* batch);
/* Timing of the last batch_run with AICP_RUN_TIME_NN: NN launches, their total duration
 * (HIP events on the context stream), and the algorithmic bytes they moved. */
int aicp_hip_last_nn_timing(const aicp_hip_ctx* ctx, int* n_launches, double* total_ms,
                            double* algorithmic_bytes, uint64_t* queries);
/* Phase times (ms, HIP events) of the last batch_run: [0] overlap (stream 1), [1] raw-
 * coordinate kd-tree + SurfaceNormal (stream 2), [2] centroid + matcher kd-tree (stream 2),
 * [3] icp loop, [4] total wall time. [0] runs concurrently with [1]-[2]. */
int aicp_hip_last_phase_ms(const aicp_hip_ctx* ctx, double out_ms[5]);

/* ---- App's frame-to-reference stream (app.cpp:282-414, robot working mode) ---------------------
 * The first cloud becomes the reference (app.cpp:285-312). Every reading is registered against
 * the current reference (overlap -> auto-tuned ratio -> ICP, app.cpp:218-247); a correction with
 * |t_i| > max_correction_magnitude drops the reading (app.cpp:366-373); an accepted reading is
 * transformed by its correction (pcl::transformPointCloud, float) and, when it is the
 * reference_update_frequency-th accepted reading since the last reference update, it becomes the
 * next reference with the translation of its corrected pose correction * prior pose as sensor
 * origin (app.cpp:375-391, aligned_cloud.cpp:61-70, common.cpp:4-23). A registration error ends
 * the stream, as the uncaught exception ends App's worker (app.cpp:210).
 * Inputs are host buffers (pre-filtered clouds, as App passes read_prefiltered); everything
 * from the upload to the corrections runs on the device, the next reference included. */

/* aicp_sequence_params.flags: App's "debug" working_mode (aicp.launch:36). Each reading is first
 * transformed by initialT_ (pcl::transformPointCloud, float) and its prior pose becomes
 * initialT_ * prior pose (app.cpp:87-96); after each accepted reading initialT_ = correction *
 * initialT_ (app.cpp:414; identity at the start). The readings then depend on each other one by
 * one, so the device registers them one after the other (the reference trees are still built
 * once per window). Without the flag: "robot" mode, the node's default (aicp_ros_node.cpp:14).
 * Filter order: this entry point takes pre-filtered clouds in both modes and moves them by
 * initialT_ afterwards. App moves the RAW reading first and pre-filters the moved cloud
 * (setAndFilterReading, app.cpp:87-99); the 0.08 m VoxelGrid is aligned to the world frame, so the
 * two orders keep different points unless initialT_ is the identity. App's exact order is
 * aicp_hip_sequence_run_raw below (and aicp_hip_map_sequence_run_raw /
 * aicp_hip_built_map_sequence_run_raw above for the two map streams, whose pre-filtered entry
 * points share this caveat); this entry point is the robot-mode fast path. */
#define AICP_SEQ_DEBUG 8

typedef struct {
  int32_t reference_update_frequency; /* 5 (aicp.launch:61) */
  float max_correction_magnitude;     /* 1.0 (aicp.launch:63; aicp_ros_node.cpp:28 default 0.5) */
  double resolution;                  /* octomapResolution (0.2, aicp_config.yaml:21) */
  int32_t flags;                      /* AICP_RUN_OVERLAP: per-reading overlap + auto-tuned ratio
                                         (else cfg->trimmed_ratio); AICP_RUN_TIME_NN; AICP_SEQ_DEBUG */
} aicp_sequence_params;

typedef struct {
  int32_t status;          /* AICP_* of this reading's registration */
  int32_t accepted;        /* 0: dropped, some |t_i| > max_correction_magnitude */
  int32_t reference;       /* cloud it was registered against: -1 the first cloud, else a reading */
  int32_t is_reference;    /* 1: it became the next reference */
  double corrected_origin[3]; /* translation of correction * prior pose (accepted readings; in debug
                                 mode the prior pose is initialT_ * the reading's prior pose) */
  aicp_icp_stats icp;
} aicp_sequence_result;

typedef struct {
  int32_t windows;         /* reference windows run (incl. re-runs after a misprediction) */
  int32_t replans;         /* re-plans after a dropped reading or an error */
  double wall_ms;          /* the whole call: packing, H2D, device work, D2H */
  double device_ms;        /* first upload enqueued -> last correction (HIP events) */
} aicp_sequence_timing;

void aicp_hip_default_sequence_params(aicp_sequence_params* out);
/* out_T: 16 floats per reading (correction, column-major); out: per reading; *n_done = readings
 * processed (all of them unless a registration error ended the stream at reading n_done - 1). */
int aicp_hip_sequence_run(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                          const aicp_cloud* first, const aicp_cloud* readings, size_t n_readings,
                          float* out_T /* 16*n */, aicp_sequence_result* out /* n */, size_t* n_done);
int aicp_hip_last_sequence_timing(const aicp_hip_ctx* ctx, aicp_sequence_timing* out);

/* App's stream from RAW clouds, in App's own order (processCloud, app.cpp:282-414 with
 * setAndFilterReading, app.cpp:77-100): the first cloud is pre-filtered as given (app.cpp:293-297)
 * and becomes the reference. Robot mode: every reading is pre-filtered as given on the device,
 * then the kept points run through aicp_hip_sequence_run. Debug mode (prm->flags AICP_SEQ_DEBUG):
 * reading after reading, the RAW reading is moved by initialT_ on the device
 * (pcl::transformPointCloud, float), the moved cloud is pre-filtered there, its prior pose becomes
 * initialT_ * prior pose, and it is registered against the current reference (overlap ->
 * auto-tuned ratio -> ICP; the reference's trees stay resident across readings); then the drop
 * test, the reference update and initialT_ = correction * initialT_ (app.cpp:362-414). Debug mode
 * is a loop over the live session's reading step (aicp_hip_session_process below) on a session
 * private to the call: the reference, initialT_ and the count stay on the device between readings
 * and no kept cloud comes back to the host. The pre-filter's region growing is host-driven, so
 * debug mode takes host round trips per reading.
 * pf: the pre-filter (aicp_hip_default_prefilter). A reading the pre-filter empties ends the
 * stream with AICP_ERR_INVALID as its status (libpointmatcher throws on an empty cloud).
 * Results as aicp_hip_sequence_run (corrected_origin from initialT_ * prior pose in debug mode);
 * aicp_hip_last_sequence_timing describes robot mode's inner aicp_hip_sequence_run only. */
int aicp_hip_sequence_run_raw(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                              const aicp_prefilter_params* pf, const aicp_cloud* first, const aicp_cloud* readings,
                              size_t n_readings, float* out_T /* 16*n */, aicp_sequence_result* out /* n */,
                              size_t* n_done);

/* App's stream from RAW clouds with failure_prediction_mode (processCloud, app.cpp:282-414 with both
 * branches of the `if` at app.cpp:362): aicp_hip_sequence_run_raw's rules, reading by reading in
 * robot and in debug mode (the features take host round trips per pair), with the pair going through
 * aicp_hip_pipeline's steps against the current reference and its pose. The call is a loop over the
 * gated session's reading step (aicp_hip_session_process_risk below) on a session private to the
 * call, so the clouds stay on the device between the steps and between the readings:
 *   risk <= threshold: the drop test, the correction, the frequency update and initialT_ =
 *     correction * initialT_ as in aicp_hip_sequence_run_raw;
 *   otherwise (app.cpp:401-411): the unmoved pre-filtered reading joins the graph with its prior pose
 *     (debug mode: initialT_ * prior pose) and at once becomes the reference; the count towards
 *     reference_update_frequency restarts; the correction is the identity, so initialT_ stays. It is
 *     reported with status AICP_OK, accepted 1, is_reference 1, corrected_origin = that pose's
 *     translation, out_T the identity and rec[i].registered 0.
 * poses: 16 doubles per reading, column-major (Eigen::Isometry3d::data()); the readings' sensor
 * origins are their translations (readings[i].origin is not read), first_pose the first cloud's.
 * The pose of a reference that is a corrected reading is App's corrected pose, in double on the
 * host: fromMatrix4fToIsometry3d(correction) * prior pose, then removePitchRollCorrection
 * (aligned_cloud.cpp:31-74, common.cpp:4-23, 70-105); its translation is corrected_origin. prm->flags:
 * AICP_SEQ_DEBUG | AICP_RUN_TIME_NN (the overlap always runs: the classifier needs it). rec: n
 * records. The windowed aicp_hip_sequence_run is not involved. */
int aicp_hip_sequence_run_risk(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                               const aicp_prefilter_params* pf, const aicp_risk_params* risk_prm,
                               const aicp_hip_svm* model, double threshold, const aicp_cloud* first,
                               const double first_pose[16], const aicp_cloud* readings /* RAW */,
                               const double* poses /* 16*n */, size_t n_readings, float* out_T /* 16*n */,
                               aicp_sequence_result* out /* n */, aicp_pipeline_record* rec /* n */, size_t* n_done);

/* ---- live App session: one reading per call, the reference resident on the device -------------
 * App::processCloud (app.cpp:282-414) in frame-to-reference mode as the node runs it: a handle keeps
 * App's state between calls, on the device: the current reference (points, sensor origin, id),
 * initialT_, the count towards reference_update_frequency, and the last reading as it was
 * registered. The rules are aicp_hip_sequence_run_raw's:
 *   robot mode: the reading is pre-filtered as given;
 *   debug mode (AICP_SEQ_DEBUG): the RAW reading is moved by the device's initialT_
 *     (pcl::transformPointCloud, float), its origin becomes the translation of initialT_ * prior
 *     pose, then it is pre-filtered;
 *   with AICP_RUN_OVERLAP the octree overlap against the reference gives aicp_hip_autotune_ratio,
 *     otherwise cfg->trimmed_ratio is used;
 *   a reading with some |t_i| > max_correction_magnitude is dropped and leaves every piece of state
 *     as it was, initialT_ included;
 *   the reference_update_frequency-th accepted reading since the last update becomes the reference
 *     (transformPointCloud by its correction in float, no FMA; origin: corrected_origin; the count
 *     restarts), and initialT_ = correction * initialT_ after every accepted reading;
 *   a reading the pre-filter empties has status AICP_ERR_INVALID; it, and any registration error,
 *     ends the session as it ends App's worker (app.cpp:210): further process calls return
 *     AICP_ERR_INVALID until aicp_hip_session_start.
 * pf NULL: the clouds are already App's read_prefiltered (as aicp_hip_sequence_run takes them; debug
 * mode then moves the filtered cloud, that entry point's documented order). pf non-NULL: the clouds
 * are RAW and go through setAndFilterReading in App's order.
 * A point-to-point chain (knn_normals 0) is accepted. A reading crosses the bus at most once (its
 * raw rows), and not at all when it comes from a sweep accumulator, which is left as it is: the
 * caller may aicp_hip_accum_clear as soon as the call returns. The reference's trees, treelets,
 * normals and voxel map stay resident across readings in the context's reference cache; any other
 * registration on the context in between takes the cache, and the session rebuilds them at its next
 * reading with the same results. A session is driven from one thread at a time, on its context's
 * stream; several sessions may share a context. */
typedef struct aicp_hip_session aicp_hip_session;
/* prm->flags: AICP_RUN_OVERLAP | AICP_SEQ_DEBUG | AICP_RUN_TIME_NN. cfg, prm and pf are copied. */
int aicp_hip_session_create(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                            const aicp_prefilter_params* pf /* nullable */, aicp_hip_session** out);
void aicp_hip_session_free(aicp_hip_ctx* ctx, aicp_hip_session* s);
/* The first cloud (app.cpp:285-312): pre-filtered as given when pf is set; it becomes reference -1.
 * Calling start again restarts the session (nothing processed, initialT_ = I, not ended). A first
 * cloud the pre-filter empties is AICP_ERR_INVALID and leaves the session as it was. */
int aicp_hip_session_start(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* first);
int aicp_hip_session_start_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3]);
/* One reading. out_T: its correction (column-major). out->reference: the index of the process call
 * (counted from 0 since start) whose reading is the reference it was registered against, -1: the
 * first cloud. kept (nullable): its points after the pre-filter (pf NULL: its points). */
int aicp_hip_session_process(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* reading, float out_T[16],
                             aicp_sequence_result* out, uint32_t* kept);
int aicp_hip_session_process_accum(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc, const double origin[3],
                                   float out_T[16], aicp_sequence_result* out, uint32_t* kept);
/* Every output is nullable. n_processed: process calls since start (dropped and failed readings
 * count); reference: as aicp_sequence_result.reference for the next reading; initial_T: initialT_,
 * column-major; ended: 1 after a failed reading. */
int aicp_hip_session_state(aicp_hip_ctx* ctx, aicp_hip_session* s, uint64_t* n_processed, int32_t* reference,
                           size_t* reference_points, float initial_T[16], int32_t* ended);
/* The current reference (App's reference_vis_): packed xyz (capacity cap points, AICP_ERR_INVALID if
 * it does not fit) and its sensor origin (nullable). */
int aicp_hip_session_reference(aicp_hip_ctx* ctx, aicp_hip_session* s, float* out, size_t cap, size_t* out_n,
                               double origin[3]);
/* The last process call that registered its reading: the whole call on the host, and from the
 * origin's upload to the promotion on the device (HIP events). Both nullable. */
int aicp_hip_session_last_timing(const aicp_hip_session* s, double* wall_ms, double* device_ms);
/* The quality monitor per reading (aicp_hip_monitor's metrics, above), on the
 * clouds where they lie when the registration returns: ref = the reference the reading was
 * registered against (what aicp_hip_session_reference returned before the call), out = T * the
 * reading as registered, T the correction the call returns, read from device memory. Allowed any
 * time after create, plain and risk sessions alike; prm NULL switches it off (the default), and a
 * process call then enqueues what it enqueues without this entry. AICP_ERR_INVALID: a quantile
 * outside [0, 1]. With AICP_MON_PAIRED the chain is the session's cfg with trimmed_ratio replaced
 * by the reading's own tuned ratio (the result's icp.trimmed_ratio).
 * A process call that registered its reading (accepted, or dropped by max_correction_magnitude)
 * leaves a result with valid = 1; a gated reading of a risk session, a call that ends the session,
 * a call with the monitor off and a session before its first process call leave valid = 0 and a
 * result of all zero bytes. The monitor runs behind the registration and ahead of the commit and
 * the promotion, and its 56 bytes come back in the call's one read-back. An error of its own (a
 * direction without a finite distance, a kd-tree deeper than 48 levels) never ends the session and
 * changes nothing the call returns: valid = 0, the reason in aicp_hip_last_error.
 * The bucket-8 tree over the reference lives in the session and is built on the first monitored
 * reading after start, after a promotion or after set_monitor; later readings against that
 * reference reuse it and build only the tree over out (the chain matcher's tree, when its bucket
 * size is not 8, is kept the same way). */
int aicp_hip_session_set_monitor(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_monitor_params* prm /* NULL: off */);
int aicp_hip_session_last_monitor(const aicp_hip_session* s, aicp_monitor_result* out, int32_t* valid);
/* out[0] monitored readings (valid results), [1] bucket-8 trees built (over references and over
 * out), [2] readings that reused the session's reference tree, [3] chain-bucket trees built. */
int aicp_hip_session_monitor_counters(const aicp_hip_session* s, uint64_t out[4]);

/* The live session with failure_prediction_mode (runAicpPipeline, app.cpp:236-245, and the gated
 * branch of processCloud, app.cpp:401-411): aicp_hip_sequence_run_risk's rules, one reading per call,
 * on the session's resident buffers. Per reading: the raw rows up (not at all from a sweep
 * accumulator), ingest and pre-filter into the session's reading buffer; an overlap-only batch of the
 * resident reference and reading (device to device; the reference's voxel map from the reference
 * cache); the alignment features with the two FOV filters reading both clouds where they lie; the
 * classifier; then k_session_gate_promote, which takes the gated branch on the device: the unmoved
 * reading is copied into the spare reference buffer, the record says accepted / is_reference with the
 * reading's prior origin as corrected_origin, the correction is the identity, the count restarts and
 * initialT_ stays. One read-back (gate record, state, record, header) ends a gated reading, which
 * builds no tree; otherwise an ICP-only batch at the device's ratio follows (device to device, the
 * reference's trees from the reference cache), then the plain session's commit and promotion. After
 * its raw rows no point of a reading or a reference crosses the bus in either direction.
 * Poses are 16 doubles, column-major (Eigen::Isometry3d::data()); the sensor origin is the
 * translation. The overlap always runs (prm->resolution > 0; AICP_RUN_OVERLAP may be left out).
 * The reading's pose in debug mode is fromMatrix4fToIsometry3d(initialT_) * pose. The reference's
 * pose stays on the host in double: removePitchRollCorrection(first_pose, first_pose) after start,
 * removePitchRollCorrection(reading's pose, pose) after a gated reading,
 * removePitchRollCorrection(fromMatrix4fToIsometry3d(T) * reading's pose, pose) after a frequency
 * promotion. A gated reading: AICP_OK, accepted 1, is_reference 1, corrected_origin = its pose's
 * translation, out_T the identity, rec->registered 0, icp.iterations 0.
 * model stays the caller's and must outlive the session; risk_prm is copied. A point-to-point chain
 * is accepted. Any non-zero status (overlap, features, classifier, registration) and an emptied
 * reading end the session until the next start. A session made here takes the _pose / _risk calls
 * below and refuses aicp_hip_session_start / _start_accum / _process / _process_accum with
 * AICP_ERR_INVALID; a session of aicp_hip_session_create refuses the calls below the same way;
 * neither refusal changes any state. state, reference, last_timing and free serve both. */
int aicp_hip_session_create_risk(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_sequence_params* prm,
                                 const aicp_prefilter_params* pf /* nullable */, const aicp_risk_params* risk_prm,
                                 const aicp_hip_svm* model, double threshold, aicp_hip_session** out);
int aicp_hip_session_start_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* first,
                                const double first_pose[16]);
int aicp_hip_session_start_accum_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc,
                                      const double first_pose[16]);
/* One reading with its prior pose (reading->origin is not read). rec: the pipeline's record (n_read:
 * the kept points). out, kept: as aicp_hip_session_process. */
int aicp_hip_session_process_risk(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_cloud* reading,
                                  const double pose[16], float out_T[16], aicp_sequence_result* out,
                                  aicp_pipeline_record* rec, uint32_t* kept);
int aicp_hip_session_process_accum_risk(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_accum* acc,
                                        const double pose[16], float out_T[16], aicp_sequence_result* out,
                                        aicp_pipeline_record* rec, uint32_t* kept);
/* The current reference's pose (column-major). */
int aicp_hip_session_reference_pose(aicp_hip_ctx* ctx, aicp_hip_session* s, double pose[16]);

/* ---- live map sessions: one reading per call on the prior map or on the built map -------------
 * App::processCloud (app.cpp:282-414) in localize_against_prior_map or localize_against_built_map
 * mode as the node runs it: a handle keeps App's state for one of the two policies between calls,
 * on the device: initialT_ and the count (prior map: getNbClouds(); built map: readings accepted
 * since the last reference), the last reading's record and its prior origin. The map stays the
 * caller's aicp_hip_map, as in the streams: it must outlive the session, and between two process
 * calls the caller may use it with the read-only map calls (aicp_hip_map_size, _download, _crop);
 * its size is final when process returns.
 * Reading by reading the rules are the streams', with every window one reading long:
 *   prior map (loc set): rules 1-7 of aicp_hip_map_sequence_run;
 *   built map (bm set):  rules 1-6 of aicp_hip_built_map_sequence_run;
 *   pf_read non-NULL: the readings are RAW and go through setAndFilterReading in App's order, as
 *     the *_run_raw streams treat them (debug mode: the RAW reading is moved by the device's
 *     initialT_, then pre-filtered);
 *   pf_read NULL: the readings are already pre-filtered, as the pre-filtered streams take them
 *     (debug mode then moves the filtered cloud, those entry points' documented order).
 * A dropped reading changes nothing, initialT_ included. An empty crop, a reading the pre-filter
 * empties and a non-zero registration status each end the session: the call returns that status,
 * out is filled as the stream fills the ending reading's record, the map keeps what was committed
 * before, and further process calls return AICP_ERR_INVALID until aicp_hip_map_session_start. So
 * does a map that cannot grow for an append: its error is returned before any state changes and the
 * map is left as it was.
 * The append (rule: merged / is_reference) is decided and done on the device behind the reading's
 * registration; the host makes room in the map beforehand, when the count says the reading would
 * append if accepted, and adds the reading's points to the map's size after the call's one
 * read-back. A point-to-point chain (knn_normals 0) is accepted. A session is driven from one
 * thread at a time, on its context's stream; several sessions may share a context, and a session
 * may alternate with any other call on the context. */
typedef struct aicp_hip_map_session aicp_hip_map_session;
/* Exactly one of loc / bm is non-NULL (both or neither: AICP_ERR_INVALID); their checks and flags
 * are the streams'. pf_read: nullable (above); an unsupported one is refused here. pf_map: the
 * prior map's re-filter (NULL: the defaults); AICP_ERR_INVALID with bm. Everything is copied. */
int aicp_hip_map_session_create(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* loc,
                                const aicp_built_map_params* bm, const aicp_prefilter_params* pf_read,
                                const aicp_prefilter_params* pf_map, aicp_hip_map_session** out);
void aicp_hip_map_session_free(aicp_hip_ctx* ctx, aicp_hip_map_session* s);
/* count = 0, initialT_ = I, not ended, nothing processed, on `map` (built map: the map created from
 * App's first cloud, as for the stream). Calling start again restarts the session. */
int aicp_hip_map_session_start(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_map* map);
/* One reading with its prior pose (16 floats, column-major; reading->origin its sensor origin, as
 * in the streams). out_T: its correction (column-major). out: aicp_localization_result* (prior map)
 * or aicp_built_map_result* (built map), one 128-byte layout. kept (nullable): its points after
 * the pre-filter (pf_read NULL: its points). */
int aicp_hip_map_session_process(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_cloud* reading,
                                 const float pose[16], float out_T[16], void* out, uint32_t* kept);
/* The reading is the sweep accumulator's cloud where it lies (no bus crossing; the accumulator is
 * left as it is); its sensor origin is the pose's translation. Needs pf_read (AICP_ERR_INVALID
 * otherwise). */
int aicp_hip_map_session_process_accum(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_accum* acc,
                                       const float pose[16], float out_T[16], void* out, uint32_t* kept);
/* Every output is nullable. n_processed: process calls since start (dropped and failed readings
 * count); count: the policy's count (above); initial_T: initialT_, column-major; ended: 1 after a
 * reading that ended the session. */
int aicp_hip_map_session_state(aicp_hip_ctx* ctx, aicp_hip_map_session* s, uint64_t* n_processed, int32_t* count,
                               float initial_T[16], int32_t* ended);
/* The last process call that registered its reading: the whole call on the host (map changes
 * included), and from its first enqueue to the append on the device (HIP events). Both nullable. */
int aicp_hip_map_session_last_timing(const aicp_hip_map_session* s, double* wall_ms, double* device_ms);
/* aicp_hip_session_set_monitor's rules for the map sessions: ref = the reading's map crop (what
 * aicp_hip_map_crop returns just before the call at the call's pose; debug mode: at the moved
 * pose), out = T * the reading as registered. The crop changes with every pose, so both trees are
 * built per reading (out[2] of the counters stays 0). A call that ends the session (an emptied
 * reading, an empty crop, a failed registration) leaves valid = 0. (The three are spelled
 * aicp_hip_mapsession_*: the aicp_hip_map_session_* family stays the seven entry points above.) */
int aicp_hip_mapsession_set_monitor(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_monitor_params* prm);
int aicp_hip_mapsession_last_monitor(const aicp_hip_map_session* s, aicp_monitor_result* out, int32_t* valid);
int aicp_hip_mapsession_monitor_counters(const aicp_hip_map_session* s, uint64_t out[4]);

/* ---- live map sessions with failure_prediction_mode: the alignment-risk gate per reading ----------
 * runAicpPipeline's gate (app.cpp:236-245) and both branches of processCloud's `if`
 * (app.cpp:362-411) under the two map policies, as aicp_hip_session_create_risk serves them for the
 * frame-to-reference policy. For a reading with prior pose P (16 doubles, column-major;
 * Eigen::Isometry3d::data()), both policies:
 *  1. The crop is taken at P cast to float (app.cpp:47, 63). The reference pose for the features is
 *     P as given: setReference runs before setAndFilterReading (app.cpp:333, 337), so in debug mode
 *     it is the unmoved P.
 *  2. The reading is pre-filtered in App's order (pf_read as in aicp_hip_map_session_create). In
 *     debug mode the raw reading is moved by initialT_ first and the reading's pose is
 *     fromMatrix4fToIsometry3d(initialT_) * P. The sensor origin is the translation of that pose;
 *     reading->origin is not read.
 *  3. The overlap. Prior map: the constant 50.0 (app.cpp:123-127), no octree is built. Built map:
 *     the octree overlap between the crop and the reading, as the built-map session computes it (the
 *     crop's origin is the translation of the float pose, the reading's its own, moved in debug
 *     mode); it always runs (bm->resolution > 0; AICP_RUN_OVERLAP may be left out).
 *  4. fov_overlap and alignability are overlapFilter's and alignabilityFilter's on (crop, reading as
 *     registered, reference pose, reading pose). The classifier takes ((float)overlap,
 *     (float)alignability); the reading is gated when !(risk <= threshold); the ratio is
 *     aicp_hip_autotune_ratio(overlap).
 *  5. Not gated: ICP at that ratio on the same crop; then the policy's rules apply unchanged (drop
 *     test, count, initialT_, append, the prior map's re-filter), as in a plain session.
 *  6. Gated (app.cpp:401-411, 414, 458-493): the correction is the identity (out_T), initialT_
 *     stays, no drop test is applied, status 0, accepted 1, corrected_origin is the reading's prior
 *     origin (moved in debug mode), rec->registered 0, icp.iterations 0 (icp: overlap_percent and
 *     trimmed_ratio of step 3 and 4, on the built map the overlap's keys; the rest 0). Then
 *       built map: the reading is the reference at once: map += the reading as filtered, unmoved
 *         (its bytes: -0.0f survives), count = 0, is_reference = 1;
 *       prior map: the cloud joins the graph (++count) marked a reference, so the merge of
 *         app.cpp:469-483 is not reached: the map gets no point and merged = 0. The re-filter test
 *         of app.cpp:487-493 stands outside that branch and still applies: refiltered = AICP_LOC_MERGE
 *         && map_refilter_every > 0 && (count - 1) % map_refilter_every == 0 with the new count. A
 *         gated first reading therefore re-filters the map, and after it the count is 1, so later
 *         readings can be dropped.
 * The gated branch is taken on the device (k_session_map_gate, right behind the classifier); on the
 * built map the host makes room for the kept points before every reading's crop, because any
 * reading may be gated. A gated reading ends with one read-back and builds no tree. The crop is taken
 * once per reading, and after its raw rows no point of the reading or the crop crosses the bus.
 * The endings are the plain session's (all reached before the gate: an empty crop, an emptied
 * reading; and a non-zero registration status) and a non-zero status of the overlap, the features or
 * the classifier. The quality monitor: a gated reading leaves valid = 0, a registered reading runs
 * it as in a plain session. model stays the caller's and must outlive the session; risk_prm is
 * copied. A point-to-point chain is accepted.
 * start, state, last_timing (a gated reading: up to its gate), free and the monitor calls serve both
 * kinds of handle. A handle made here refuses aicp_hip_map_session_process / _process_accum with
 * AICP_ERR_INVALID and no state change; a handle of aicp_hip_map_session_create refuses the two
 * calls below the same way. */
int aicp_hip_mapsession_create_risk(aicp_hip_ctx* ctx, const aicp_icp_config* cfg, const aicp_localization_params* loc,
                                    const aicp_built_map_params* bm, const aicp_prefilter_params* pf_read,
                                    const aicp_prefilter_params* pf_map, const aicp_risk_params* risk_prm,
                                    const aicp_hip_svm* model, double threshold, aicp_hip_map_session** out);
/* out, out_T, kept: as aicp_hip_map_session_process. rec: the pipeline's record (n_read: the kept
 * points). */
int aicp_hip_mapsession_process_risk(aicp_hip_ctx* ctx, aicp_hip_map_session* s, const aicp_cloud* reading,
                                     const double pose[16], float out_T[16], void* out, aicp_pipeline_record* rec,
                                     uint32_t* kept);
int aicp_hip_mapsession_process_accum_risk(aicp_hip_ctx* ctx, aicp_hip_map_session* s, aicp_hip_accum* acc,
                                           const double pose[16], float out_T[16], void* out,
                                           aicp_pipeline_record* rec, uint32_t* kept);

/* ---- the mapping session's built map: aligned_map_, the go-back, the start on a loaded map --------
 * App appends every reference to aligned_map_ (app.cpp:310 for the first cloud, app.cpp:458-468
 * after every promotion), the node publishes it, and on a go-back request turns it into the prior
 * map and switches the same App, with its initialT_ and its graph, to localize_against_prior_map
 * (app_ros.cpp:329-357). All of it stays on the device.
 *
 * aicp_hip_session_keep_aligned_map: on != 0: every later start (start, start_accum, start_pose,
 * start_accum_pose, start_on_map) gives the session an aicp_hip_map of its own, made device to
 * device from the bytes of the first cloud's reference (app.cpp:310; a start on a map: empty). A
 * start that fails leaves the old map as it was, one that succeeds replaces it. Default: off; a
 * process call then enqueues what it always did. on == 0: a map the session holds is freed at
 * once. Allowed on plain and risk sessions, after create and before the next start.
 *
 * Append rule (app.cpp:458-468): after a process call whose reading became the reference (the
 * result's is_reference: a frequency promotion, or a risk session's gated reading) the new
 * reference's points lie behind the map in order, the same bytes the call wrote into the reference:
 * the reading as registered moved by its correction (aicp_hip_transform's float expression, w = 1),
 * or, gated, the unmoved bytes. A dropped reading, a reading that ends the session and an accepted
 * reading that is not promoted append nothing. Room is made before the reading is registered, when
 * the count says the reading would be promoted if accepted (a risk session: for every reading); a
 * map that cannot grow is the call's error (AICP_ERR_HIP, or AICP_ERR_INVALID past 2^31 - 1
 * points) with the map and the session as they were, the session not ended. The call ends in the
 * read-backs it always had.
 *
 * aicp_hip_session_aligned_map: a borrowed handle, valid until the session's next start, take or
 * free; between two process calls the read-only map calls (aicp_hip_map_size, _download, _crop,
 * _capacity) may use it. AICP_ERR_INVALID when keeping is off, before the first start with it on,
 * or after a take.
 * aicp_hip_session_take_aligned_map: the map is the caller's (aicp_hip_map_free); nothing is copied.
 * The session keeps running without a map until its next start. */
int aicp_hip_session_keep_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, int on);
int aicp_hip_session_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_map** out);
int aicp_hip_session_take_aligned_map(aicp_hip_ctx* ctx, aicp_hip_session* s, aicp_hip_map** out);
/* The go-back (app_ros.cpp:329-357): aicp_hip_map_session_start on `map` for a prior-map session,
 * with App's state instead of a fresh one: the count starts at from's getNbClouds() (1 for the
 * first cloud, none after aicp_hip_session_start_on_map, plus the readings accepted since its
 * start, gated ones included), and initialT_ is from's, copied device to device in stream order.
 * So the drop test is live from the first localisation reading (app.cpp:366-369) and the merge and
 * re-filter phases follow (n_clouds - 1) % f of App's graph (app.cpp:469-493). Neither handle
 * needs the other afterwards. AICP_ERR_INVALID, with nothing changed: ms was made with the
 * built-map policy; from is not started, or ended (App's worker is dead then); from lives on
 * another context. */
int aicp_hip_mapsession_start_go_back(aicp_hip_ctx* ctx, aicp_hip_map_session* ms, aicp_hip_map* map,
                                      const aicp_hip_session* from);
/* load_map_from_file without localize_against_prior_map (app.cpp:43-59, 392-399), plain sessions
 * only (a risk session: AICP_ERR_INVALID, nothing changed). The reference is `map` cropped to
 * [crop_min, crop_max]^3 around first_pose (column-major; aicp_hip_map_crop's crop, device to
 * device), its id -1, its origin the pose's translation; initialT_ = I, the count 0, nothing
 * processed, the graph empty. An empty crop: AICP_ERR_INVALID, the session as it was. With keeping
 * on the aligned map starts empty (app.cpp:310 is not reached). The first process call after it
 * runs without the drop test (getNbClouds() == 0, app.cpp:366-369) and its accepted reading is the
 * next reference whatever the frequency (app.cpp:383-399); the overlap runs against the crop as
 * against any reference. From the second reading on the session is an ordinary one. `map` is only
 * read, and not needed after the call. */
int aicp_hip_session_start_on_map(aicp_hip_ctx* ctx, aicp_hip_session* s, const aicp_hip_map* map,
                                  const float first_pose[16], float crop_min, float crop_max);

/* ---- kernel-level entry points (parity tests and diagnostics) --------------------------- */
/* kd-tree over pts (as given, no centring) + k-NN of queries: libnabo
 * KDTreeUnbalancedPtInLeavesImplicitBoundsStackOpt order, ALLOW_SELF_MATCH.
 * ids are input indices of pts; unmatched = -1 with dist +inf. */
int aicp_hip_knn(aicp_hip_ctx* ctx, const float* pts, size_t n, size_t stride,
                 const float* queries, size_t nq, size_t qstride, int k, float epsilon,
                 float max_dist, int32_t* out_ids /* k*nq */, float* out_d2 /* k*nq */,
                 uint64_t* out_touched /* nullable */);
/* SurfaceNormal descriptor (knn, keepNormals) of pts in input order. */
int aicp_hip_normals(aicp_hip_ctx* ctx, const float* pts, size_t n, size_t stride, int knn,
                     float* out_normals /* 3*n */, int32_t* out_degenerate /* nullable */);
/* Matches::getDistsQuantile on the device (radix select). */
int aicp_hip_dists_quantile(aicp_hip_ctx* ctx, const float* d2, size_t n, float quantile,
                            float* out_limit);
/* solvePossiblyUnderdeterminedLinearSystem on the device (A row-major 6x6, double). */
int aicp_hip_solve6(aicp_hip_ctx* ctx, const double* A, const double* b, double* out_x,
                    int32_t* out_path /* 0 LLT, 1 QR min-norm, 2 eigen pseudo-inverse */);
/* Test surface: any implementation of the TrimmedDist limit on given distances. Runs n_steps
 * selects, one after another on the same pair states, as successive ICP iterations would. Step s
 * uses variant[s] on d2 + s * total, where total = sum(counts), pair p's slice at its prefix
 * offset. variant: 0 the separate launches (aicp_hip_dists_quantile's), 1 the two launches with
 * tails, 2 the fused launch with the launcher's own choice of template, 3 / 4 the fused launch
 * with 2048 / 8192 candidates in LDS, 5 one workgroup per pair (counts <= 65536). Between steps
 * the entry does the update kernel's part only (the next active list); the digit-1 guess of a
 * fused step is what the previous step left (0 before the first), and a pair that stopped (no
 * finite distance: status 1) or started inactive keeps its outputs. out_dirty: non-zero words
 * left in the select's self-resetting work space after the last step (0 expected).
 * AICP_ERR_INVALID: a null pointer, no pair or more than 4096, no step, a count of 0, a ratio
 * outside [0, 1], an unknown variant, variant 5 with a count above 65536, n_steps * total >= 2^32. */
int aicp_hip_test_select(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* counts, const float* ratios,
                         const uint8_t* active /* nullable: 0 = pair starts inactive */,
                         size_t n_steps, const int32_t* variant, const float* d2,
                         float* out_limit, int32_t* out_status, int32_t* out_n_finite,
                         uint32_t* out_b1, uint32_t* out_miss /* each n_steps * n_pairs */,
                         uint64_t* out_dirty);
/* Test surface: the tail of an ICP iteration, k_icp_reduce and k_icp_update_f as the loop launches
 * them, on given matches. Runs n_steps steps, one after another on the same pair states; each is
 * the active list followed by the production reduce + update launch. Pair p has n_read[p] centred
 * readings (read_c, 3 floats each, the pairs one after another) and gathers reference points and
 * normals at ref_off[p] + match from ref_pts / ref_nrm (3 * total_ref floats each; pairs may share
 * a range). init_T (nullable): 16 floats per pair, column-major, T_iter before the first step
 * (identity by default; the checker ring's entry 0 stays the identity's). Step s writes
 * limit[s * n_pairs + p] into the pair's state (no select runs) and reads match, d2 and touched
 * (low half: touched points, high half: touched nodes) at s * total + the pair's prefix offset,
 * total = sum(n_read). Before every step the slab is filled with doubles of the bit pattern
 * 0x7FF8DEAD7FF8DEAD, so a row nothing wrote is recognisable.
 * Per step: out_slab gets all slab rows (pair p's ceil(n_read[p] / 1024) rows of 30 doubles at its
 * prefix row offset); out_T 16 floats per pair; out_state 6 per pair: kept, iters, status, active,
 * converged, hist_count; out_inlier 1; out_touched 2 (points, nodes; running totals); out_dqdt 2:
 * dq and dt of the ring entry last pushed. out_dirty: non-zero words left in the reduce / pairs
 * arrival counters after the last step (0 expected).
 * AICP_ERR_INVALID, before any device work: a null pointer (init_T and active may be null), no
 * pair or more than 4096, no step, a count of 0, ref_off + n_ref above total_ref, total_ref 0 or
 * >= 2^28, smooth outside [1, 32), a non-finite limit, a match outside [0, n_ref) on a reading
 * with d2 <= limit, sum(n_read) >= 2^31, n_steps * total >= 2^32. */
int aicp_hip_test_step(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* n_read, const uint32_t* n_ref,
                       const uint32_t* ref_off, size_t total_ref, const float* read_c, const float* ref_pts,
                       const float* ref_nrm, const float* init_T /* nullable */,
                       const uint8_t* active /* nullable: 0 = pair starts inactive */, int32_t max_iter,
                       int32_t smooth, float min_rot, float min_trans, size_t n_steps,
                       const float* limit /* n_steps * n_pairs */, const int32_t* match, const float* d2,
                       const uint32_t* touched /* each n_steps * total */, double* out_slab, float* out_T,
                       int32_t* out_state, float* out_inlier, uint64_t* out_touched, double* out_dqdt,
                       uint64_t* out_dirty);
/* The same for the PointToPointErrorMinimizer's kernels, k_icp_reduce_p2p and k_icp_update_p2p:
 * aicp_hip_test_step without ref_nrm (no normals are read). Slab columns: 0..8 sum q_a p_b (3a + b),
 * 9..11 sum p, 12..14 sum q, 15..26 0.0, 27 kept, 28 / 29 touched points / nodes. */
int aicp_hip_test_step_p2p(aicp_hip_ctx* ctx, size_t n_pairs, const uint32_t* n_read, const uint32_t* n_ref,
                           const uint32_t* ref_off, size_t total_ref, const float* read_c, const float* ref_pts,
                           const float* init_T /* nullable */,
                           const uint8_t* active /* nullable: 0 = pair starts inactive */, int32_t max_iter,
                           int32_t smooth, float min_rot, float min_trans, size_t n_steps,
                           const float* limit /* n_steps * n_pairs */, const int32_t* match, const float* d2,
                           const uint32_t* touched /* each n_steps * total */, double* out_slab, float* out_T,
                           int32_t* out_state, float* out_inlier, uint64_t* out_touched, double* out_dqdt,
                           uint64_t* out_dirty);
/* Test surface: the batched kd-tree build as a registration batch runs it for its matcher trees,
 * on given clouds, and everything it wrote. pts: the n_refs clouds one after another, 3 floats per
 * point, counts[r] points each; they are built as one batch (one launch sequence for all clouds),
 * with the global levels planned from the largest cloud, the context's tree_plan / tree_lvl_min
 * options and what the context's previous build used. center 0: trees on the points as given
 * (mean 0); 1: the exact centroid of each cloud and trees on the centred points. bucket: the leaf
 * size (1..4096).
 * Per cloud: out_node_off (its first record in out_nodes), out_n_nodes, out_depth, out_mean (3).
 * out_nodes: 2 * total + 2 records of 4 words, total = sum(counts): an inner node {cut (float
 * bits), cd | right child << 2, parent, depth}, a leaf {point count, 3 | bucket start << 2, parent,
 * depth}; child, parent (0xFFFFFFFF at the root) and bucket start are local to the cloud, the left
 * child is the next record. Records past the last cloud's are not written. out_bpts: total rows
 * (x, y, z, input id within the cloud as integer bits) in bucket order, cloud r's at its prefix
 * offset. out_ctl: AICP_TEST_TREE_CTL_WORDS words of the build's control block: segments per global
 * level [0, 50), then n_small (segments given to the subtree builders), n_mid (to the mid-size
 * builder), n_big (segments above the mid-size limit left over by a plan that was too shallow) and
 * the error bits (1: deeper than 47 levels, 16: a scan took its slow path).
 * The outputs are filled whatever the build reports: AICP_ERR_UNSUPPORTED for a tree deeper than the
 * device stack, AICP_ERR_HIP for any other error bit. Invalidates the context's reference cache.
 * AICP_ERR_INVALID, before any device work: a null pointer, no cloud or more than 4096, a count of
 * 0, total >= 2^28, center outside {0, 1}, bucket outside [1, 4096]. */
#define AICP_TEST_TREE_CTL_WORDS 54
int aicp_hip_test_tree(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* counts, const float* pts,
                       int32_t center, int32_t bucket, uint32_t* out_node_off, uint32_t* out_n_nodes,
                       int32_t* out_depth, float* out_mean /* 3 * n_refs */,
                       uint32_t* out_nodes /* 4 * (2 * total + 2) */, float* out_bpts /* 4 * total */,
                       uint32_t* out_ctl /* AICP_TEST_TREE_CTL_WORDS */);
/* Test surface: the ICP loop's NN search, k_icp_nn as the loop launches it, query by query. The
 * n_refs reference clouds (ref_pts, 3 floats per point, ref_counts[r] points each, one after
 * another) are used as given, with no centring: their trees are built as one batch, as
 * aicp_hip_test_tree builds them, with leaf size `bucket`, then the matcher's treelets where the
 * batch's rule selects them: bucket <= 15, fewer than 2^28 treelet records, no reference above
 * 4 M points, nn_engine 0. Pair p searches reference pair_ref[p] (pairs may share one) for its
 * n_read[p] readings (read_c, 3 floats each, the pairs one after another). Step k writes
 * T[16 (k n_pairs + p) ..] (column-major) into pair p's state as T_iter and active[k n_pairs + p]
 * as its active flag (active null: every pair, every step), then runs the active list and the NN
 * launch with the production grid, epsilon and max_dist as a chain's KDTreeMatcher gives them.
 * A query is ((T0 x + T1 y) + T2 z) + T3 per row in float. Non-finite query coordinates are out of
 * scope: libnabo defines no result for them.
 * Per step and reading, at k * total + the pair's prefix offset, total = sum(n_read): out_match
 * (the bucket position of the match within the pair's reference, -1: none within max_dist),
 * out_d2 (+inf then), out_touched (inner nodes << 16 | bucket points, each saturated at 65535).
 * Before every step the three device arrays are filled with AICP_TEST_NN_SENTINEL (match, d2: a
 * NaN and a position no search gives) and AICP_TEST_NN_TOUCH_SENTINEL (no inner node but more
 * points than a bucket holds), 64 guard words on both sides included: a reading of an inactive
 * pair keeps its sentinels, and out_dirty counts the guard words that changed (0 expected).
 * out_ids: the input id (within its cloud) of every bucket position, reference r's at its prefix
 * offset. out_engine: 0 treelets (Trav2C), 1 node records (Trav<1>).
 * A tree deeper than 47 levels returns AICP_ERR_UNSUPPORTED before any search runs. Invalidates
 * the context's reference cache.
 * AICP_ERR_INVALID, before any device work: a null pointer (active may be null), no reference, pair
 * or step or more than 4096 references or pairs, a count of 0, a pair_ref >= n_refs, bucket outside
 * [1, 4096], sum(ref_counts) or total >= 2^28, a negative or NaN epsilon or max_dist,
 * n_steps * total >= 2^32. */
#define AICP_TEST_NN_SENTINEL 0x7FF8DEADu
#define AICP_TEST_NN_TOUCH_SENTINEL 0x0000DEADu
int aicp_hip_test_nn(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* ref_counts, const float* ref_pts,
                     int32_t bucket, size_t n_pairs, const uint32_t* pair_ref, const uint32_t* n_read,
                     const float* read_c, size_t n_steps, const float* T /* 16 * n_steps * n_pairs */,
                     const uint8_t* active /* n_steps * n_pairs, nullable */, float epsilon, float max_dist,
                     int32_t* out_match, float* out_d2, uint32_t* out_touched /* each n_steps * total */,
                     int32_t* out_ids /* sum(ref_counts) */, int32_t* out_engine, uint64_t* out_dirty);
/* Test surface: the SurfaceNormal chain of a batch's references, launch by launch, and everything
 * it writes. The n_refs clouds (pts, 3 floats per point, counts[r] points each, one after another;
 * total = sum(counts)) go through what a registration batch runs for its references:
 *  1. the raw-coordinate trees as one batch (no centring, leaf size 8), as aicp_hip_test_tree
 *     builds a batch with the plan the registration gives the raw tree;
 *  2. the per-reference state (launch_init_state);
 *  3. launch_normals: the self-kNN of every point (`knn` neighbours, eps 0, self included) on the
 *     engine the context's normals_knn_engine option selects, then k_normals_from_ids;
 *  4. launch_knn_ids once more, into a second id buffer, with the touched counters;
 *  5. the matcher trees (centred, leaf size matcher_bucket);
 *  6. launch_normals_to_matcher: the normals into the matcher trees' bucket order.
 * The two id buffers, the raw normals and the matcher normals live in buffers of this call and are
 * filled with AICP_TEST_NN_SENTINEL before the launches, 64 guard words on both sides included;
 * out_dirty counts the guard words that changed (0 expected).
 * out_ids, out_ids2: knn entries per raw bucket position (reference r's at its prefix offset), in
 * k-best order, each a raw bucket position within the reference, -1 past the cloud's size.
 * out_raw_id, out_matcher_id: the input id (within its cloud) of every raw / matcher bucket
 * position. out_nrm, out_bnrm: 4 floats per raw / matcher bucket position (x, y, z, 0).
 * out_degenerate: per reference, the points whose covariance had rank <= 1 (normal e_y).
 * out_touched: the second kNN launch's bucket points and inner nodes. out_engine: 1 one query per
 * octet of lanes (k_knn_oct), 2 one per lane (k_knn_ids): the kernel step 4 launched.
 * AICP_ERR_INVALID, before any device work: a null pointer, no cloud or more than 4096, a count of
 * 0, total >= 2^28, matcher_bucket outside [1, 4096]. AICP_ERR_UNSUPPORTED: knn outside
 * {10, 20, 30} (before any device work), a tree deeper than 47 levels (before any search).
 * Invalidates the context's reference cache. */
int aicp_hip_test_normals(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* counts, const float* pts, int32_t knn,
                          int32_t matcher_bucket, int32_t* out_ids, int32_t* out_ids2 /* each knn * total */,
                          int32_t* out_raw_id /* total */, float* out_nrm /* 4 * total */,
                          int32_t* out_degenerate /* n_refs */, uint64_t* out_touched /* 2 */,
                          float* out_bnrm /* 4 * total */, int32_t* out_matcher_id /* total */, int32_t* out_engine,
                          uint64_t* out_dirty);
/* Test surface: the octree overlap of a batch, set by set. The n_refs reference clouds (ref_pts, 3
 * floats per point, ref_counts[r] points each, one after another) and the n_pairs readings
 * (read_pts, n_read[p] points each) go through the batch's own overlap, as aicp_hip_align_batch
 * with AICP_RUN_OVERLAP runs it: pair p reads reference pair_ref[p] from ref_origins[3 p ..] and
 * its reading from read_origins[3 p ..]; pairs with the same reference and the same reference
 * origin form one overlap group, in order of first appearance. Clouds are numbered groups first,
 * then readings (n_groups + n_pairs of them, at most 2 n_pairs).
 * path: 0 the batch's own rule, 1 the batch's dense voxel maps, 2 the batch's sorted keys, 3 the
 * stream's voxel maps sized on the device, 4 the stream's capped key lists. A batch whose maps do
 * not fit (a map above 2^34 voxels, or all of them above the arena's budget) runs on sorted keys
 * under 0 and 1 as well; out->path says which ran (1 to 4). Under 3 and 4 every overlap group runs
 * as one window of the frame-to-reference stream (its reference and the readings paired with it),
 * through the stream's own host plan (ovl_window_slots / _keys / _sides) and device steps
 * (ovl_window_side for the readings and for the reference, ovl_window_counts), one window after
 * the other on one stream.
 * filter / wide: -1 the path's rules (batch: the marks' LDS cache from 9 clouds on, the wide count
 * grids for one pair in one group; stream: neither), 0 or 1 to override them for this call;
 * out->filter / out->wide say what was launched (0 on keys). The trimmed ratio is set from the
 * overlap as a registration sets it.
 * cap_mode 0: the stream's own capacities (map_cap of the clouds' extents; key_bound of their
 * rays, the reference's in the form `rigid` selects: 0 as given, 1 for any rigid motion). 1: caps[]
 * gives them per cloud, groups then readings (path 3: bytes of the map slot; path 4: words; the
 * readings of a window share one list of the sum of their capacities). A window whose map slots
 * exceed the stream's 1 GiB budget returns AICP_ERR_UNSUPPORTED under 3 (the stream runs it on
 * key lists).
 * Outputs (caller's arrays in aicp_test_overlap_out, all required):
 *  pair_group[p]; per cloud: cloud_keys (|S|), cloud_err (ovl_err), cloud_bbox (6: key box of its
 *  valid points and origin, min then max; under 4 of the origin alone, the key lists need no box); per pair: pair_counts (3: |A|, |B|, |A ∩ B|),
 *  pair_percent, pair_ratio, pair_err.
 *  Dense maps: desc_min, desc_dim (3 per cloud), desc_off, desc_bytes, and the first
 *  min(arena_cap, arena_bytes) bytes of the map arena in `arena`. Under 3 the windows' arenas
 *  follow one another (desc_off counts from the first), each filled with bytes of 0xA5 before its
 *  window runs: what no kernel wrote (a slot's room beyond its map, a refused slot) still holds them.
 *  Sorted keys: per point (the groups' reference points, then the readings': n_points of them, at
 *  most points_cap) key_counts and the exclusive key_offsets; the sorted words
 *  cloud << 48 | k0 << 32 | k1 << 16 | k2 in `words` (the first min(words_cap, n_words)).
 *  Under 4: per window g two lists, [2 g] its readings' (tagged 0 .. n - 1 in pair order, pad words
 *  n << 48) and [2 g + 1] its reference's (tag 0, pad 1 << 48): list_off (first word in `words`) and
 *  list_cap (all cap words are returned, pads included); key_offsets count within a list;
 *  cloud_bound: the capacity each cloud contributed (the host's bound, or caps[]); under 3 the
 *  bytes of its map slot.
 *  dirty: under 3 and 4 the arena and the key lists are buffers of this call with 64 guard words of
 *  8 bytes on both sides (under 4 around each of the emitted and the sorted array); the guard
 *  words that changed (0 expected).
 * An ovl_err of a cloud is reported in the outputs, not as a return code; a reading's state is its
 * pair's, so its cloud_err also carries its group's error (k_ovl_finish folds it in). Invalidates the context's
 * reference cache.
 * AICP_ERR_INVALID, before any device work: a null pointer (out's arrays included), no reference or
 * pair or more than 4096, a count of 0, a pair_ref >= n_refs, resolution <= 0 or NaN, path outside
 * [0, 4], filter, wide outside {-1, 0, 1}, cap_mode or rigid outside {0, 1}, cap_mode 1 without
 * caps or under a batch path, fewer than n_points points_cap. */
typedef struct {
  int32_t path, filter, wide; /* what ran */
  int32_t n_groups;
  int32_t* pair_group;        /* n_pairs */
  uint64_t* cloud_keys;       /* 2 n_pairs */
  int32_t* cloud_err;         /* 2 n_pairs */
  int32_t* cloud_bbox;        /* 6 * 2 n_pairs */
  uint64_t* pair_counts;      /* 3 n_pairs */
  float* pair_percent;        /* n_pairs */
  float* pair_ratio;          /* n_pairs */
  int32_t* pair_err;          /* n_pairs */
  int32_t* desc_min;          /* 3 * 2 n_pairs */
  int32_t* desc_dim;          /* 3 * 2 n_pairs */
  uint64_t* desc_off;         /* 2 n_pairs */
  uint64_t* desc_bytes;       /* 2 n_pairs */
  uint8_t* arena;
  uint64_t arena_cap, arena_bytes;
  uint32_t* key_counts;       /* points_cap */
  uint64_t* key_offsets;      /* points_cap */
  uint64_t points_cap, n_points;
  uint64_t* words;
  uint64_t words_cap, n_words;
  uint64_t* cloud_bound;      /* 2 n_pairs */
  uint64_t* list_off;         /* 2 n_pairs */
  uint64_t* list_cap;         /* 2 n_pairs */
  uint64_t dirty;
} aicp_test_overlap_out;
int aicp_hip_test_overlap(aicp_hip_ctx* ctx, size_t n_refs, const uint32_t* ref_counts, const float* ref_pts,
                          size_t n_pairs, const uint32_t* pair_ref, const uint32_t* n_read, const float* read_pts,
                          const double* ref_origins /* 3 n_pairs */, const double* read_origins /* 3 n_pairs */,
                          double resolution, int32_t path, int32_t filter, int32_t wide, int32_t cap_mode,
                          const uint64_t* caps /* nullable: n_groups + n_pairs */, int32_t rigid,
                          aicp_test_overlap_out* out);
/* Host only, no device call: the stream's upper bound of the words its key lists hold for a cloud
 * of n points (3 floats each) seen from origin: every key of computeRayKeys(origin, p) and p's own
 * key, duplicates included, each point's share capped at *out_point_cap (3 * 65536 + 8). rigid 0:
 * for the cloud as given; 1: for any rigid motion of cloud and origin together. Returns
 * AICP_ERR_INVALID for a null pointer, n == 0, resolution <= 0 or NaN, rigid outside {0, 1}. */
int aicp_hip_test_key_bound(const float* pts, size_t n, const double origin[3], double resolution, int32_t rigid,
                            uint64_t* out_bound, uint64_t* out_point_cap);
/* Test surface: the raw streams' ingest alone. rows: n rows of `stride` bytes (>= 12, a multiple of
 * 4), xyz first, uploaded as the raw streams upload them (at most 16 bytes: verbatim; wider: packed
 * on the host), then k_stream_ingest: out4[4 i ..] = (x, y, z, 1), moved by T (nullable, column-major
 * float[16]) in aicp_hip_transform's float expression. out4 (nullable: nothing is downloaded). */
int aicp_hip_test_ingest(aicp_hip_ctx* ctx, const float* rows, size_t n, size_t stride,
                         const float* T /* nullable */, float* out4 /* 4*n, nullable */);
/* The quality monitor's resident core as the live sessions run it: ref and read
 * (packed xyz) are placed in guarded device buffers, T (column-major float[16]) in device memory,
 * and the core runs `runs` (1..8) times in a row on them with one reference tree, built by the
 * first run and reused by the others (a session's readings against one reference). result: the last
 * run's 56 bytes, equal to aicp_hip_monitor(ref, read, T)'s. *dirty: guard words that changed
 * around the four buffers, plus 1 for every input that no longer holds what was uploaded (0 when
 * all is well). counters: aicp_hip_session_monitor_counters' four. cfg: nullable without
 * AICP_MON_PAIRED. Errors as aicp_hip_monitor's. */
int aicp_hip_test_monitor_resident(aicp_hip_ctx* ctx, const aicp_monitor_params* prm, const aicp_icp_config* cfg,
                                   const float* ref_xyz, size_t n_ref, const float* read_xyz, size_t n_read,
                                   const float T[16], int32_t runs, aicp_monitor_result* result, uint64_t* dirty,
                                   uint64_t counters[4]);
/* The live session's promotion kernels alone, on a made-up block. block (448 bytes, in and out):
 * the stream state at 0 (initialT_ 16 floats, count int32 at 64), the record at 128 (status,
 * accepted, append, refilter int32; corrected_origin 3 doubles at 144), the reference's header at
 * 192 (count uint32, id int32, origin 3 doubles at 208), the gate's record at 256 (its int32 gate
 * at 280), the correction T at 320 (16 floats), the prior origin at 384 (3 doubles). read4: n
 * float4 points, taken as their bytes. kernel: 0 k_session_promote, 1 k_session_gate_promote,
 * 2 k_session_promote_map, 3 k_session_gate_promote_map, each behind its production launch with
 * the reference id `id`. ref4 (4 n floats out): the reference buffer; map4 (4 (tail + n) floats
 * out): the map with its tail at `tail` points (kernels 0 and 1 are given no map). Both buffers and
 * 64 guard words on each side of them are filled with 0xA5 bytes first; *dirty: guard words that
 * changed, plus 1 when read4's bytes on the device changed. */
int aicp_hip_test_promote_map(aicp_hip_ctx* ctx, int32_t kernel, const float* read4, size_t n, size_t tail,
                              int32_t id, void* block, float* ref4, float* map4, uint64_t* dirty);
/* Test surface: one side's filter list (side: AICP_CHAIN_REFERENCE / _READING) over n_clouds clouds
 * at once, through the kernels aicp_hip_align_chain_batch runs. counts: the clouds' sizes (each >=
 * 1); pts: their points laid end to end, 3 floats each. Out, per cloud c:
 *   out_counts[4 c + q]  points after filter q of the list (0 past the list's end)
 *   out_n[c]             kept points
 *   out_index            the kept points' indices in their own cloud, the clouds' kept points laid
 *                        end to end (cloud c's start at the sum of out_n before it); capacity total
 *   out_normals          nullable: 3 floats per kept point, laid out as out_index (a SurfaceNormal
 *                        of knn 10 / 20 / 30 on the side)
 *   out_densities        nullable: the densities at the SurfaceNormal, in the order of each cloud
 *                        there, the clouds end to end (cloud c holds as many as it had points at
 *                        that position); capacity total (keep_densities on the side)
 * AICP_ERR_INVALID, before any device work: a null pointer, no cloud or more than 4096, a count of
 * 0, total >= 2^28, a wrong side, normals / densities asked of a side that has none, and whatever
 * the chain check refuses. Invalidates the context's reference cache. */
int aicp_hip_test_chain_batch(aicp_hip_ctx* ctx, const aicp_chain* chain, int32_t side, size_t n_clouds,
                              const uint32_t* counts, const float* pts, uint64_t* out_counts /* 4 * n_clouds */,
                              uint64_t* out_n /* n_clouds */, int32_t* out_index /* total */,
                              float* out_normals /* 3 * total, nullable */,
                              float* out_densities /* total, nullable */);

#ifdef __cplusplus
}
#endif

#endif /* AICP_HIP_H_ */
