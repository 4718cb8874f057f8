// accum.cpp — the sweep accumulator of include/aicp_hip.h: VelodyneAccumulatorROS (aicp_ros/src/
// velodyne_accumulator.cpp:31-84) with the accumulated cloud in HBM.
//
// A push stages the caller's rows in one of the accumulator's pinned slots (so the caller's buffer
// is free on return), enqueues their upload and the two kernels of kernels_accum.hip on the
// context's stream, and returns. The only thing a push may wait for is the event of the slot it is
// about to reuse, i.e. the upload enqueued kSlots pushes ago. The kept counts stay on the device
// (the tails array); the host tracks the sum of the pushed sizes, an upper bound that keeps every
// append inside the buffer whatever the crop keeps. One staging area on the device serves every
// sweep: the stream runs sweep j's kernels before sweep j + 1's upload.
// Buffers that a larger sweep outgrows are not freed while work may be in flight (a free waits for
// the device): they are set aside and released at the next call that waits for the stream anyway.
#include <cmath>
#include <cstring>

#include "../../include/aicp_hip.h"
#include "aicp_common.hpp"
#include "kernels.hpp"
#include "runtime.hpp"

using namespace aicp;
using namespace aicp::rt;

namespace {
constexpr int kSlots = 4;
constexpr size_t kFirstRows = 65536;         // rows the staging holds before it first grows
constexpr size_t kMaxPoints = size_t(1) << 30;  // (tile and point indices stay far inside int32)
}  // namespace

struct aicp_hip_accum {
  aicp_accum_params prm{};
  size_t cap = 0;       // capacity_points
  size_t bound = 0;     // sum of every n pushed since the last clear (>= the device tail)
  int32_t counter = 0;  // sweeps taken
  DevBuf pts;           // cap float4
  DevBuf tails;         // batch_size + 1 running totals, tails[0] = 0 for good
  DevBuf rows;          // the sweep being taken: row_cap rows of 16 bytes | crop_tiles(row_cap) words
  size_t row_cap = 0;
  struct Slot {
    PinBuf pin;
    hipEvent_t ev = nullptr;  // recorded behind the slot's upload
    bool busy = false;
  } slot[kSlots];
  int next = 0;
  PinBuf pin_tails;
  std::vector<DevBuf> old_dev;  // outgrown, released once the stream has been waited for
  std::vector<PinBuf> old_pin;
};

namespace {

void release_old(aicp_hip_accum* a) {
  for (auto& b : a->old_dev) release(b);
  for (auto& b : a->old_pin) release(b);
  a->old_dev.clear();
  a->old_pin.clear();
}

size_t rows_bytes(size_t row_cap) { return row_cap * 16 + crop_tiles(row_cap) * 4; }

// the tails on the host, the stream idle: the points where the host learns the counts
int sync_tails(aicp_hip_ctx* ctx, aicp_hip_accum* a, const uint32_t** t) {
  HIPC(hipSetDevice(ctx->device));
  const size_t nb = ((size_t)a->prm.batch_size + 1) * 4;
  HIPC(hipMemcpyAsync(a->pin_tails.p, a->tails.p, nb, hipMemcpyDeviceToHost, ctx->stream));
  HIPC(hipStreamSynchronize(ctx->stream));
  for (auto& s : a->slot) s.busy = false;
  release_old(a);
  *t = a->pin_tails.as<uint32_t>();
  if ((*t)[a->counter] > a->bound) FAIL(AICP_ERR_HIP, "accumulator: the device tail exceeds the pushed points");
  return AICP_OK;
}

}  // namespace

namespace aicp {
namespace rt {
int accum_resident(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const float4** pts, size_t* n) {
  const uint32_t* t = nullptr;
  const int rc = sync_tails(ctx, acc, &t);
  if (rc) return rc;
  *pts = acc->pts.as<float4>();
  *n = t[acc->counter];
  return AICP_OK;
}
}  // namespace rt
}  // namespace aicp

extern "C" {

void aicp_hip_default_accum_params(aicp_accum_params* p) {
  if (!p) return;
  p->batch_size = 80;  // aicp_ros_node.cpp:40
  p->crop_min = -30.f;  // velodyne_accumulator.cpp:60
  p->crop_max = 30.f;
}

void aicp_hip_accum_free(aicp_hip_ctx* ctx, aicp_hip_accum* acc) {
  if (!acc) return;
  if (ctx) {
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
  }
  release_old(acc);
  release(acc->pts);
  release(acc->tails);
  release(acc->rows);
  release(acc->pin_tails);
  for (auto& s : acc->slot) {
    release(s.pin);
    if (s.ev) (void)hipEventDestroy(s.ev);
  }
  delete acc;
}

int aicp_hip_accum_create(aicp_hip_ctx* ctx, const aicp_accum_params* prm, size_t capacity_points,
                          aicp_hip_accum** out) {
  if (!ctx || !prm || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  if (prm->batch_size < 1 || prm->batch_size > 65535) FAIL(AICP_ERR_INVALID, "accumulator: batch_size must be 1..65535");
  if (!std::isfinite(prm->crop_min) || !std::isfinite(prm->crop_max) || prm->crop_min > prm->crop_max)
    FAIL(AICP_ERR_INVALID, "accumulator: crop bounds");
  if (capacity_points < 1 || capacity_points > kMaxPoints) FAIL(AICP_ERR_INVALID, "accumulator: capacity must be 1..2^30");
  HIPC(hipSetDevice(ctx->device));
  aicp_hip_accum* a = new aicp_hip_accum();
  a->prm = *prm;
  a->cap = capacity_points;
  a->row_cap = std::min(kFirstRows, capacity_points);
  const size_t tb = ((size_t)prm->batch_size + 1) * 4;
  hipError_t e = ensure(a->pts, capacity_points * 16);
  if (e == hipSuccess) e = ensure(a->tails, tb);
  if (e == hipSuccess) e = ensure(a->rows, rows_bytes(a->row_cap));
  if (e == hipSuccess) e = ensure(a->pin_tails, tb);
  if (e == hipSuccess) e = hipMemset(a->tails.p, 0, tb);
  for (auto& s : a->slot) {
    if (e == hipSuccess) e = ensure(s.pin, a->row_cap * 16);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s.ev, hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    aicp_hip_accum_free(ctx, a);
    HIPC(e);
  }
  *out = a;
  return AICP_OK;
}

int aicp_hip_accum_push(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const float* pts, size_t n, size_t stride,
                        const double pose[16]) {
  if (!ctx || !acc || !pose || (n && !pts) || stride < 12 || (stride % 4)) return AICP_ERR_INVALID;
  if (acc->counter >= acc->prm.batch_size) return AICP_OK;  // if (finished_) return;
  if (n > acc->cap - acc->bound) FAIL(AICP_ERR_INVALID, "accumulator: the sweep does not fit the capacity");
  HIPC(hipSetDevice(ctx->device));
  hipStream_t s = ctx->stream;
  const bool verbatim = stride <= 16;
  const size_t ds = verbatim ? stride : 16;
  if (n > acc->row_cap) {  // a larger sweep than any before: a new staging area, the old one set aside
    const size_t rc = std::min(acc->cap, std::max(n, 2 * acc->row_cap));
    DevBuf nb;
    HIPC(ensure(nb, rows_bytes(rc)));
    acc->old_dev.push_back(acc->rows);
    acc->rows = nb;
    acc->row_cap = rc;
  }
  if (n) {
    aicp_hip_accum::Slot& sl = acc->slot[acc->next];
    if (sl.busy) {  // its own upload, kSlots pushes ago: not the stream
      HIPC(hipEventSynchronize(sl.ev));
      sl.busy = false;
    }
    if (n * 16 > sl.pin.cap) {
      PinBuf nb;
      HIPC(ensure(nb, acc->row_cap * 16));
      acc->old_pin.push_back(sl.pin);
      sl.pin = nb;
    }
    size_t bytes = n * 16;
    if (verbatim) {
      bytes = (n - 1) * stride + 12;  // (the caller's last row may end with its z)
      std::memcpy(sl.pin.p, pts, bytes);
    } else {
      pack_xyz4(pts, n, stride, sl.pin.as<float>());
    }
    HIPC(hipMemcpyAsync(acc->rows.p, sl.pin.p, bytes, hipMemcpyHostToDevice, s));
    HIPC(hipEventRecord(sl.ev, s));
    sl.busy = true;
    acc->next = (acc->next + 1) % kSlots;
  }
  AccumSweep a{};
  a.box.inv[0] = a.box.inv[4] = a.box.inv[8] = 1.f;  // Eigen::MatrixXf::Identity(4, 4)
  a.box.mn = acc->prm.crop_min;
  a.box.mx = acc->prm.crop_max;
  aicp_hip_accum_pose_matrix(pose, a.T);
  uint32_t* tile_cnt = reinterpret_cast<uint32_t*>(acc->rows.as<char>() + acc->row_cap * 16);
  launch_accum_sweep(s, (int)n, acc->rows.p, ds, a, tile_cnt, acc->tails.as<uint32_t>(), acc->counter,
                     acc->pts.as<float4>(), (uint32_t)acc->cap);
  HIPC(hipGetLastError());
  acc->bound += n;
  ++acc->counter;
  return AICP_OK;
}

int aicp_hip_accum_state(aicp_hip_ctx* ctx, aicp_hip_accum* acc, int32_t* counter, int32_t* finished,
                         size_t* n_points, uint32_t* kept_per_sweep) {
  if (!ctx || !acc) return AICP_ERR_INVALID;
  const uint32_t* t = nullptr;
  const int rc = sync_tails(ctx, acc, &t);
  if (rc) return rc;
  if (counter) *counter = acc->counter;
  if (finished) *finished = acc->counter >= acc->prm.batch_size ? 1 : 0;
  if (n_points) *n_points = t[acc->counter];
  if (kept_per_sweep)
    for (int32_t j = 0; j < acc->prm.batch_size; ++j) kept_per_sweep[j] = j < acc->counter ? t[j + 1] - t[j] : 0u;
  return AICP_OK;
}

int aicp_hip_accum_clear(aicp_hip_ctx* ctx, aicp_hip_accum* acc) {
  if (!ctx || !acc) return AICP_ERR_INVALID;
  // (tails[0] stays 0 and sweep 0 starts there: the stream orders the next reading's kernels
  // behind whatever still reads this one)
  acc->bound = 0;
  acc->counter = 0;
  return AICP_OK;
}

int aicp_hip_accum_download(aicp_hip_ctx* ctx, aicp_hip_accum* acc, float* out, size_t cap, size_t* out_n) {
  if (!ctx || !acc || !out_n || (cap && !out)) return AICP_ERR_INVALID;
  *out_n = 0;
  const uint32_t* t = nullptr;
  const int rc = sync_tails(ctx, acc, &t);
  if (rc) return rc;
  const size_t m = t[acc->counter];
  if (m > cap) FAIL(AICP_ERR_INVALID, "accumulator: output capacity too small");
  if (!m) return AICP_OK;
  HIPC(ensure(ctx->pin_io, m * 16));
  float* h = ctx->pin_io.as<float>();
  HIPC(hipMemcpy(h, acc->pts.p, m * 16, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < m; ++i)
    for (int k = 0; k < 3; ++k) out[3 * i + k] = h[4 * i + k];
  *out_n = m;
  return AICP_OK;
}

int aicp_hip_accum_prefilter(aicp_hip_ctx* ctx, aicp_hip_accum* acc, const aicp_prefilter_params* prm,
                             const float T[16], float* out, size_t cap, size_t* out_n) {
  if (!ctx || !acc || !prm || !out_n || (cap && !out)) return AICP_ERR_INVALID;
  *out_n = 0;
  const uint32_t* t = nullptr;
  const int rc = sync_tails(ctx, acc, &t);
  if (rc) return rc;
  return prefilter_resident(ctx, prm, acc->pts.as<float4>(), t[acc->counter], T, out, cap, out_n);
}

}  // extern "C"
