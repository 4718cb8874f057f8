// kernels_session.hip — the device side of the live App session (session.cpp): what follows one
// reading's registration without a host decision in between.
//
// k_stream_commit (kernels_map_stream.hip) with np = 1 and the built-map rules states
// app.cpp:366-391, 414 for the frame-to-reference policy too: drop test, count towards
// reference_update_frequency, corrected origin, initialT_ = correction * initialT_, and `append`
// when this reading is the next reference. k_session_promote runs right behind it and does what the
// record says: the reading as it was registered, moved by its correction, becomes the session's
// reference (app.cpp:375-391: pcl::transformPointCloud in float, apply4's expression, no FMA).
//
// k_session_gate_promote is the gated branch of failure_prediction_mode (app.cpp:401-411) for a risk
// session, right behind k_svm_predict: the reading becomes the reference unmoved, by the gate the
// classifier left in device memory.
//
// k_session_promote_map and k_session_gate_promote_map are these two for a session that keeps
// App's aligned_map_ (app.cpp:310, 458-468): every point of the new reference is stored a second
// time, behind the session's map.
//
// k_session_map_append is the same step for the live map sessions (map_stream.cpp): the reading
// goes behind the caller's map instead (prior map: app.cpp:469-483, built map: app.cpp:383-391,
// 458-465), where the host has made room before the reading's crop was enqueued.
//
// k_session_map_gate is the gated branch for the live map sessions made by
// aicp_hip_mapsession_create_risk, right behind k_svm_predict: on the built map the unmoved reading
// goes behind the map and the count restarts, on the prior map the cloud joins the graph without a
// merge and the re-filter rule still applies (app.cpp:401-411, 458-493).
#include <hip/hip_runtime.h>

#include "aicp_common.hpp"
#include "icp_math.hpp"
#include "kernels.hpp"

namespace aicp {

// One point of the reading as it was registered, moved by its correction: one 128-bit load
// (k_transform's expression), and the stores of the value it gives.
__device__ __forceinline__ float4 moved_point(const float (&Tl)[16], const float4* __restrict__ read, int i) {
  const float4 p = read[i];
  float q[3];
  apply4(Tl, p.x, p.y, p.z, q);
  return make_float4(q[0], q[1], q[2], 1.f);
}
// One load, one 128-bit store. The body of k_session_promote and k_session_map_append.
__device__ __forceinline__ void move_point(const float (&Tl)[16], const float4* __restrict__ read,
                                           float4* __restrict__ dst, int i) {
  dst[i] = moved_point(Tl, read, i);
}
// One load, the one value stored twice. The body of k_session_promote_map.
__device__ __forceinline__ void move_point(const float (&Tl)[16], const float4* __restrict__ read,
                                           float4* __restrict__ dst, float4* __restrict__ dst2, int i) {
  const float4 q = moved_point(Tl, read, i);
  dst[i] = q;
  dst2[i] = q;
}

// One point of the reading as it was filtered, unmoved: its bytes, one 128-bit load, one 128-bit
// store (apply4 by the identity would turn -0.0f into +0.0f). The body of the two gate kernels.
__device__ __forceinline__ void copy_point(const float4* __restrict__ read, float4* __restrict__ dst, int i) {
  dst[i] = read[i];
}
// The same bytes stored twice, from one load. The body of k_session_gate_promote_map.
__device__ __forceinline__ void copy_point(const float4* __restrict__ read, float4* __restrict__ dst,
                                           float4* __restrict__ dst2, int i) {
  const float4 p = read[i];
  dst[i] = p;
  dst2[i] = p;
}

// One thread per point of the reading: one 128-bit load, one 128-bit store. Every thread reads the
// record's append flag and the correction from device memory (the same addresses for the whole
// grid: the branch is uniform, the loads are served from the scalar / L2 path). Thread 0 of block 0
// writes the header. ref never aliases read (the session's spare reference buffer).
__global__ __launch_bounds__(256) void k_session_promote(int n, const StreamRec* __restrict__ rec,
                                                         const float* __restrict__ T,
                                                         const float4* __restrict__ read, int32_t id,
                                                         float4* __restrict__ ref, SessionHeader* hdr) {
  if (!rec->append) return;
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = T[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr->count = (uint32_t)n;
    hdr->id = id;
    for (int k = 0; k < 3; ++k) hdr->origin[k] = rec->corrected_origin[k];
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  move_point(Tl, read, ref, i);
}

// k_session_promote for a session that keeps aligned_map_ (app.cpp:458-468: every new reference goes
// behind the map): the same uniform reads, header and per-point value, stored to ref[i] and to the
// map's tail dst[i] (room for n points was reserved before the reading was enqueued): one 128-bit
// load, two 128-bit stores. Neither ref nor dst aliases read or the other.
__global__ __launch_bounds__(256) void k_session_promote_map(int n, const StreamRec* __restrict__ rec,
                                                             const float* __restrict__ T,
                                                             const float4* __restrict__ read, int32_t id,
                                                             float4* __restrict__ ref, float4* __restrict__ dst,
                                                             SessionHeader* hdr) {
  if (!rec->append) return;
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = T[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    hdr->count = (uint32_t)n;
    hdr->id = id;
    for (int k = 0; k < 3; ++k) hdr->origin[k] = rec->corrected_origin[k];
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  move_point(Tl, read, ref, dst, i);
}

// k_session_promote's per-point body with the destination the caller gives (the map's tail,
// map->pts + map->n: room for n points was reserved before the launch) and no header. dst never
// aliases read (the batch's copy of the reading).
__global__ __launch_bounds__(256) void k_session_map_append(int n, const StreamRec* __restrict__ rec,
                                                            const float* __restrict__ T,
                                                            const float4* __restrict__ read,
                                                            float4* __restrict__ dst) {
  if (!rec->append) return;
  float Tl[16];
  for (int k = 0; k < 16; ++k) Tl[k] = T[k];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  move_point(Tl, read, dst, i);
}

// The gated branch (app.cpp:401-411: the unmoved reading joins the graph with its prior pose and is
// the reference at once, the count restarts, initialT_ stays) behind k_svm_predict. Every thread
// reads the gate from device memory (one address for the whole grid: the branch is uniform).
// Gated: one thread per point of the reading copies it with one 128-bit load and one 128-bit store
// (the bytes: apply4 by the identity would turn -0.0f into +0.0f, the host stream's swap does not),
// thread 0 of block 0 writes the record, the identity correction, the count and the header. Not
// gated: thread 0 of block 0 clears rec->append, nothing else is written. ref never aliases read.
__global__ __launch_bounds__(256) void k_session_gate_promote(int n, const GateRec* __restrict__ gate,
                                                              const double* __restrict__ origin,
                                                              const float4* __restrict__ read, int32_t id,
                                                              float4* __restrict__ ref, float* __restrict__ T,
                                                              StreamState* S, StreamRec* rec, SessionHeader* hdr) {
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (!gate->gate) {
    if (first) rec->append = 0;
    return;
  }
  if (first) {
    rec->status = 0;
    rec->accepted = 1;
    rec->append = 1;
    rec->refilter = 0;
    hdr->count = (uint32_t)n;
    hdr->id = id;
    for (int k = 0; k < 3; ++k) {
      const double o = origin[k];
      rec->corrected_origin[k] = o;
      hdr->origin[k] = o;
    }
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    S->count = 0;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  copy_point(read, ref, i);
}

// k_session_gate_promote for a session that keeps aligned_map_: the gated reading's bytes go to
// ref[i] and to the map's tail dst[i] (one 128-bit load, two 128-bit stores); everything thread 0 of
// block 0 writes, and the branch not gated, are k_session_gate_promote's.
__global__ __launch_bounds__(256) void k_session_gate_promote_map(int n, const GateRec* __restrict__ gate,
                                                                  const double* __restrict__ origin,
                                                                  const float4* __restrict__ read, int32_t id,
                                                                  float4* __restrict__ ref, float4* __restrict__ dst,
                                                                  float* __restrict__ T, StreamState* S,
                                                                  StreamRec* rec, SessionHeader* hdr) {
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (!gate->gate) {
    if (first) rec->append = 0;
    return;
  }
  if (first) {
    rec->status = 0;
    rec->accepted = 1;
    rec->append = 1;
    rec->refilter = 0;
    hdr->count = (uint32_t)n;
    hdr->id = id;
    for (int k = 0; k < 3; ++k) {
      const double o = origin[k];
      rec->corrected_origin[k] = o;
      hdr->origin[k] = o;
    }
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
    S->count = 0;
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  copy_point(read, ref, dst, i);
}

// The gated branch for the live map sessions (built: app.cpp:401-411, 458-465; prior map:
// app.cpp:401-411, 469-493) behind k_svm_predict. Every thread reads the gate from device memory
// (one address for the whole grid: the branch is uniform). Not gated: thread 0 of block 0 clears
// rec->append, nothing else is written. Gated, built map (r.built): one thread per point of the
// reading copies it to the map's tail (dst: room for n points was reserved before the launch; it
// never aliases read, the batch's copy of the reading), thread 0 of block 0 writes the record
// (append 1), the identity correction and the count 0. Gated, prior map (one block; n, read and dst
// are not used): the cloud joins the graph marked a reference, so the merge of app.cpp:469-483 is not
// reached (append 0) while the re-filter test of app.cpp:487-493 still applies to the new count.
// S->initT is never written.
__global__ __launch_bounds__(256) void k_session_map_gate(int n, StreamRules r, const GateRec* __restrict__ gate,
                                                          const double* __restrict__ origin,
                                                          const float4* __restrict__ read, float4* __restrict__ dst,
                                                          float* __restrict__ T, StreamState* S, StreamRec* rec) {
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (!gate->gate) {
    if (first) rec->append = 0;
    return;
  }
  if (first) {
    int32_t refilter = 0;
    if (r.built) {
      S->count = 0;
    } else {
      const int32_t c = S->count + 1;  // ++n_clouds
      refilter = r.merge && r.refilter_every > 0 && (c - 1) % r.refilter_every == 0;
      S->count = c;
    }
    rec->status = 0;
    rec->accepted = 1;
    rec->append = r.built ? 1 : 0;
    rec->refilter = refilter;
    for (int k = 0; k < 3; ++k) rec->corrected_origin[k] = origin[k];
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.f : 0.f;
  }
  if (!r.built) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  copy_point(read, dst, i);
}

void launch_session_promote(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read, int32_t id,
                            float4* ref, SessionHeader* hdr) {
  if (n > 0) k_session_promote<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, rec, T, read, id, ref, hdr);
}
void launch_session_gate_promote(hipStream_t s, int n, const GateRec* gate, const double* origin, const float4* read,
                                 int32_t id, float4* ref, float* T, StreamState* S, StreamRec* rec,
                                 SessionHeader* hdr) {
  if (n > 0)
    k_session_gate_promote<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, gate, origin, read, id, ref, T, S, rec, hdr);
}
void launch_session_promote_map(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read,
                                int32_t id, float4* ref, float4* dst, SessionHeader* hdr) {
  if (n > 0) k_session_promote_map<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, rec, T, read, id, ref, dst, hdr);
}
void launch_session_gate_promote_map(hipStream_t s, int n, const GateRec* gate, const double* origin,
                                     const float4* read, int32_t id, float4* ref, float4* dst, float* T, StreamState* S,
                                     StreamRec* rec, SessionHeader* hdr) {
  if (n > 0)
    k_session_gate_promote_map<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, gate, origin, read, id, ref, dst, T, S,
                                                                           rec, hdr);
}
void launch_session_map_append(hipStream_t s, int n, const StreamRec* rec, const float* T, const float4* read,
                               float4* dst) {
  if (n > 0) k_session_map_append<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(n, rec, T, read, dst);
}
void launch_session_map_gate(hipStream_t s, int n, const StreamRules& r, const GateRec* gate, const double* origin,
                             const float4* read, float4* dst, float* T, StreamState* S, StreamRec* rec) {
  // built map: sized by the kept count; prior map: one block (no point is copied)
  const unsigned blocks = r.built ? (unsigned)((n + 255) / 256) : 1u;
  if (n > 0) k_session_map_gate<<<blocks, 256, 0, s>>>(n, r, gate, origin, read, dst, T, S, rec);
}

}  // namespace aicp
