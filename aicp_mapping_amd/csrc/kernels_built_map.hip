// kernels_built_map.hip — the device side of App's localization stream on the map it has built
// itself (built_map.cpp; localize_against_built_map, app.cpp:60-69, 366-391, 414, 458-465).
//
// A window's readings are registered as one batch (run_batch), each against its own crop of the
// map with its own overlap and ratio. k_bm_commit then walks the window in order and takes App's
// decisions: the drop test (from the first reading on: the graph already holds the first cloud),
// the count of accepted readings since the last reference, the corrected origin, initialT_, and
// which reading becomes a reference, that is, goes to the map's tail (k_loc_merge appends it from
// the batch's copy; k_loc_move moves a debug-mode reading: kernels_localization.hip).
#include <hip/hip_runtime.h>

#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {

// The window's readings in order, one thread (at most kMaxPairs readings, a few hundred flops
// each). st / T: the batch's states and corrections after k_finalize; origin: the readings' prior
// origins (debug mode: moved by k_loc_move). By the window rule (aicp_hip_built_map_window) at
// most one reading of a window becomes a reference, and it is the window's last.
__global__ void k_bm_commit(int np, const PairState* __restrict__ st, const float* __restrict__ T,
                            const double* __restrict__ origin, BmRules r, BmState* S, BmRec* rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int acc = S->acc;
  int append = -1;
  float I[16];
  for (int k = 0; k < 16; ++k) I[k] = S->initT[k];
  bool ended = false;
  for (int i = 0; i < np; ++i) {
    BmRec o;
    o.status = -1;
    o.accepted = o.is_reference = o.pad = 0;
    for (int k = 0; k < 3; ++k) o.corrected_origin[k] = 0.0;
    if (!ended) {
      o.status = st[i].status;
      if (o.status == 0 && r.overlap && st[i].ovl_err) o.status = 3;  // AICP_ERR_HIP, as run_batch reports it
      if (o.status != 0) {
        ended = true;  // the worker ends here (app.cpp:210): nothing after this reading happens
      } else {
        float C[16];
        for (int k = 0; k < 16; ++k) C[k] = T[16 * (size_t)i + k];
        // app.cpp:366-373: getNbClouds() != 0 always holds (the first cloud is in the graph)
        if (!correction_rejected(C, r.max_corr)) {
          o.accepted = 1;
          corrected_origin(C, origin + 3 * (size_t)i, o.corrected_origin);
          if (++acc == r.freq) {  // app.cpp:383-391, 458-465: this reading is the next reference
            o.is_reference = 1;
            append = i;
            acc = 0;
          }
          float N[16];
          mul4(C, I, N);  // initialT_ = correction * initialT_ (app.cpp:414)
          for (int k = 0; k < 16; ++k) I[k] = N[k];
        }
      }
    }
    rec[i] = o;
  }
  S->acc = acc;
  S->append = append;
  for (int k = 0; k < 16; ++k) S->initT[k] = I[k];
}

void launch_bm_commit(hipStream_t s, int np, const PairState* st, const float* T, const double* origin, BmRules r,
                      BmState* S, BmRec* rec) {
  if (np > 0) k_bm_commit<<<1, 64, 0, s>>>(np, st, T, origin, r, S, rec);
}

}  // namespace aicp
