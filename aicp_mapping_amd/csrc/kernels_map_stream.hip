// kernels_map_stream.hip — the device side of App's map localization streams (map_stream.cpp):
// on the prior map (localize_against_prior_map, app.cpp:41-58, 366-373, 414, 469-493) and on the
// map App builds itself (localize_against_built_map, app.cpp:60-69, 366-391, 414, 458-465).
//
// A window's readings are registered as one batch (run_batch). What follows stays on the device:
// k_stream_commit walks the window in order and takes App's decisions (drop, count, corrected
// origin, initialT_, which reading goes to the map's tail, re-filter); the host appends from the
// batch's copy of the reading by the device's own correction (launch_transform). In the debug
// working mode k_loc_move moves the reading by the device-resident initialT_ before it is
// registered. Raw readings (the *_run_raw entry points) enter through k_stream_ingest, which
// unpacks the caller's rows into the pre-filter's input and, in debug mode, moves them first.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {

// setAndFilterReading's debug branch (app.cpp:87-96): every point by initialT_ in
// pcl::transformPointCloud's float order (apply4, as k_transform), in place; thread 0 of block 0
// also makes the prior pose initialT_ * prior pose, of which only the translation is used
// (fromMatrix4fToIsometry3d, common.cpp:4-23: corrected_origin's arithmetic, as k_debug_prep).
__global__ __launch_bounds__(256) void k_loc_move(int n, const float* __restrict__ initT, double* origin,
                                                  float4* pts) {
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = initT[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double o[3];
    corrected_origin(Tl, origin, o);
    for (int k = 0; k < 3; ++k) origin[k] = o[k];
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  float q[3];
  apply4(Tl, p.x, p.y, p.z, q);
  pts[i] = make_float4(q[0], q[1], q[2], 1.f);
}

// A raw reading as the caller's rows were uploaded (n rows of stride_w 32-bit words, xyz first)
// into the pre-filter's input: float4(x, y, z, 1). With initT (debug mode, setAndFilterReading
// app.cpp:90-99: the RAW reading is moved, then pre-filtered) every point goes through apply4, the
// float expression of k_transform / k_loc_move, and thread 0 of block 0 makes origin the
// translation of initialT_ * prior pose as k_loc_move does. One thread per point; a row of 16
// bytes is one 128-bit load, any other stride three 32-bit loads.
__global__ __launch_bounds__(256) void k_stream_ingest(int n, const float* __restrict__ rows, int stride_w,
                                                       const float* __restrict__ initT, double* origin,
                                                       float4* __restrict__ out) {
  float Tl[16];
  if (initT) {
    for (int k = 0; k < 16; ++k) Tl[k] = initT[k];
    if (origin && blockIdx.x == 0 && threadIdx.x == 0) {
      double o[3];
      corrected_origin(Tl, origin, o);
      for (int k = 0; k < 3; ++k) origin[k] = o[k];
    }
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float x, y, z;
  if (stride_w == 4) {
    const float4 p = reinterpret_cast<const float4*>(rows)[i];
    x = p.x;
    y = p.y;
    z = p.z;
  } else {
    const float* p = rows + (size_t)i * (size_t)stride_w;
    x = p[0];
    y = p[1];
    z = p[2];
  }
  if (initT) {
    float q[3];
    apply4(Tl, x, y, z, q);
    x = q[0];
    y = q[1];
    z = q[2];
  }
  out[i] = make_float4(x, y, z, 1.f);
}

// The window's readings in order, one thread (a window holds at most kMaxPairs readings and the
// walk is a few hundred flops each). st / T: the batch's states and corrections after k_finalize;
// origin: the readings' prior origins (debug mode: moved by k_loc_move). By the window rules
// (aicp_hip_localization_window, aicp_hip_built_map_window) the map changes at most after the
// window's last reading.
__global__ void k_stream_commit(int np, const PairState* __restrict__ st, const float* __restrict__ T,
                                const double* __restrict__ origin, StreamRules r, StreamState* S, StreamRec* rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int n = S->count;
  float I[16];
  for (int k = 0; k < 16; ++k) I[k] = S->initT[k];
  bool ended = false;
  for (int i = 0; i < np; ++i) {
    StreamRec o;
    o.status = -1;
    o.accepted = o.append = o.refilter = 0;
    for (int k = 0; k < 3; ++k) o.corrected_origin[k] = 0.0;
    if (!ended) {
      o.status = st[i].status;
      if (o.status == 0 && r.overlap && st[i].ovl_err) o.status = 3;  // AICP_ERR_HIP, as run_batch reports it
      if (o.status != 0) {
        ended = true;  // the worker ends here (app.cpp:210): nothing after this reading happens
      } else {
        float C[16];
        for (int k = 0; k < 16; ++k) C[k] = T[16 * (size_t)i + k];
        // app.cpp:366-373: on the prior map the first cloud of the graph is never dropped
        // (getNbClouds() != 0); on the built map the graph already holds the first cloud
        if (!((r.built || n != 0) && correction_rejected(C, r.max_corr))) {
          ++n;
          o.accepted = 1;
          corrected_origin(C, origin + 3 * (size_t)i, o.corrected_origin);
          float N[16];
          mul4(C, I, N);  // initialT_ = correction * initialT_ (app.cpp:414)
          for (int k = 0; k < 16; ++k) I[k] = N[k];
          if (r.built) {
            if (n == r.freq) {  // app.cpp:383-391, 458-465: this reading is the next reference
              o.append = 1;
              n = 0;
            }
          } else if (r.merge) {
            o.append = (n - 1) % r.freq == 0;                                      // app.cpp:469-483
            o.refilter = r.refilter_every > 0 && (n - 1) % r.refilter_every == 0;  // app.cpp:485-493
          }
        }
      }
    }
    rec[i] = o;
  }
  S->count = n;
  for (int k = 0; k < 16; ++k) S->initT[k] = I[k];
}

void launch_loc_move(hipStream_t s, int n, const float* initT, double* origin, float4* pts) {
  k_loc_move<<<(unsigned)std::max(1, (n + 255) / 256), 256, 0, s>>>(n, initT, origin, pts);
}
void launch_stream_ingest(hipStream_t s, int n, const void* rows, size_t stride, const float* initT, double* origin,
                          float4* out) {
  if (n > 0)
    k_stream_ingest<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, static_cast<const float*>(rows), (int)(stride / 4),
                                                                initT, origin, out);
}
void launch_stream_commit(hipStream_t s, int np,const PairState* st, const float* T, const double* origin,
                          StreamRules r, StreamState* S, StreamRec* rec) {
  if (np > 0) k_stream_commit<<<1, 64, 0, s>>>(np, st, T, origin, r, S, rec);
}

}  // namespace aicp
