// overlap_keys.hpp — the overlap's key rule and the ray walk's set-up (device), shared by the voxel
// maps (kernels_overlap.hip) and the sorted key lists (kernels_overlap_sparse.hip): one key rule,
// one test of the ray's end keys and one direction / step / tMax / tDelta set-up for both, and
// ray_keys, the walk that visits every key. k_ovl_mark runs its own loop over the same set-up: its
// step carries box-relative coordinates, and every shape of a shared loop tried for it made the C2
// launch slower (profiles/README.md).
#pragma once
#include <hip/hip_runtime.h>

namespace aicp {

constexpr int kKeyMax = 32768;  // octomap's tree_max_val at depth 16

// coordToKeyChecked: the key exists iff floor(c / res) is in [-32768, 32768) (x86 converts NaN
// and out-of-range values to INT_MIN, which octomap's range test rejects; written out here so a
// NaN coordinate is rejected on the device as well, instead of converting to 0)
__device__ __forceinline__ bool ovl_key(double rf, float c, int& key) {
  const double f = floor(rf * (double)c);
  if (!(f >= -(double)kKeyMax && f < (double)kKeyMax)) return false;
  key = (int)f + kKeyMax;
  return true;
}

// The state of computeRayKeys(origin, end) (octomap: Amanatides-Woo, float direction, double tMax /
// tDelta, keys wrapping at 16 bits; the walk ends on the endpoint's key or past the length).
struct RayWalk {
  float o[3], e[3];
  int ko[3], ke[3];  // the origin's and the endpoint's key
  bool okE;          // the endpoint has a key (it is in the set whether or not a walk precedes it)
  int step[3], cur[3];
  double tMax[3], tDelta[3], len;
};

// the end keys; true when a walk lies between them (both exist and differ)
__device__ __forceinline__ bool ray_ends(double res, const double* org, float4 p4, RayWalk& w) {
  w.o[0] = (float)org[0], w.o[1] = (float)org[1], w.o[2] = (float)org[2];
  w.e[0] = p4.x, w.e[1] = p4.y, w.e[2] = p4.z;
  const double rf = 1.0 / res;
  const bool okO = ovl_key(rf, w.o[0], w.ko[0]) && ovl_key(rf, w.o[1], w.ko[1]) && ovl_key(rf, w.o[2], w.ko[2]);
  w.okE = ovl_key(rf, w.e[0], w.ke[0]) && ovl_key(rf, w.e[1], w.ke[1]) && ovl_key(rf, w.e[2], w.ke[2]);
  return okO && w.okE && !(w.ko[0] == w.ke[0] && w.ko[1] == w.ke[1] && w.ko[2] == w.ke[2]);
}

// direction, step, tMax, tDelta and length of a ray with ray_ends() true; cur = the origin's key
__device__ __forceinline__ void ray_setup(double res, RayWalk& w) {
  float dir[3] = {w.e[0] - w.o[0], w.e[1] - w.o[1], w.e[2] - w.o[2]};
  const float nsq = dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2];
  const float length = (float)sqrt((double)nsq);
  for (int i = 0; i < 3; ++i) dir[i] /= length;
  for (int i = 0; i < 3; ++i) {
    w.cur[i] = w.ko[i];
    w.step[i] = dir[i] > 0.0f ? 1 : (dir[i] < 0.0f ? -1 : 0);
    if (w.step[i] != 0) {
      double vb = (double(w.cur[i] - kKeyMax) + 0.5) * res;
      vb += (float)(w.step[i] * res * 0.5);
      w.tMax[i] = (vb - (double)w.o[i]) / (double)dir[i];
      w.tDelta[i] = res / (double)fabsf(dir[i]);
    } else {
      w.tMax[i] = 1.7976931348623157e308;
      w.tDelta[i] = 1.7976931348623157e308;
    }
  }
  w.len = (double)length;
}

// every key of computeRayKeys(origin, end), then the endpoint's key, to visit(k0, k1, k2), in
// k_ovl_mark's order and arithmetic
template <class Visit>
__device__ __forceinline__ void ray_keys(double res, const double* org, float4 p4, Visit&& visit) {
  RayWalk w;
  if (ray_ends(res, org, p4, w)) {
    visit(w.ko[0], w.ko[1], w.ko[2]);
    ray_setup(res, w);
    for (;;) {
      int dim;
      if (w.tMax[0] < w.tMax[1])
        dim = (w.tMax[0] < w.tMax[2]) ? 0 : 2;
      else
        dim = (w.tMax[1] < w.tMax[2]) ? 1 : 2;
#pragma unroll
      for (int i = 0; i < 3; ++i)
        if (i == dim) {
          w.cur[i] = (w.cur[i] + w.step[i]) & 0xFFFF;
          w.tMax[i] += w.tDelta[i];
        }
      if (w.cur[0] == w.ke[0] && w.cur[1] == w.ke[1] && w.cur[2] == w.ke[2]) break;
      const double dfo = fmin(fmin(w.tMax[0], w.tMax[1]), w.tMax[2]);
      if (dfo > w.len) break;
      visit(w.cur[0], w.cur[1], w.cur[2]);
    }
  }
  if (w.okE) visit(w.ke[0], w.ke[1], w.ke[2]);
}

}  // namespace aicp
