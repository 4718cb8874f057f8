// hip_alignability.hpp — overlapFilter / alignabilityFilter of aicp_core's filteringUtils over
// libaicp_hip.so, with the reference's signatures
// (aicp_core/include/aicp_utils/filteringUtils.hpp; aicp_core/src/utils/filteringUtils.cpp:111-193,
// 196-430). App::computeAlignmentRisk (app.cpp:143-185) calls both; with this header its two call
// sites change by a namespace:
//     fov_overlap_  = aicp_hip::overlapFilter(cloudA, cloudB, poseA, poseB, range, view, accA, accB);
//     alignability_ = aicp_hip::alignabilityFilter(accA, accB, poseA, poseB, planesA, planesB, eig);
// Header-only, through the C-ABI of include/aicp_hip.h. tests/shim/risk_main.cpp compiles it against
// stand-ins of the PCL / Eigen types (tests/test_risk_cpu.py).
//
// alignabilityFilter takes the accepted clouds from the host, as the reference does, so it runs
// aicp_hip_prefilter on each and aicp_hip_cluster_match on the results. The path that keeps
// everything between the raw clouds and the two features on the device is
// aicp_hip_alignment_features: a maintainer who can change computeAlignmentRisk's
// body calls that once instead of the two filters.
//
// Behaviour kept from the reference: kept points in input order in the global frame; -1 entries
// for unmatched clusters; "No matching normals left" returns 0 (:344-348); `eigenvectors` holds
// three points at the matched planes' centroid whose normals are the PCA axes (:402-424). The
// matched planes carry the cluster index in rgb where the reference draws a random colour
// (:300-313). The classifier (an OpenCV SVM on the two floats, app.cpp:179) stays with App.
#ifndef AICP_HIP_ALIGNABILITY_HPP_
#define AICP_HIP_ALIGNABILITY_HPP_

#include <Eigen/Geometry>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>

#include <cstdlib>
#include <iostream>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "aicp_hip.h"

namespace aicp_hip {

// The process-wide device context of the two filters (App calls them from its one worker
// thread). Throws std::runtime_error when no HIP device is usable.
inline aicp_hip_ctx* risk_ctx() {
  static std::mutex mu;
  static aicp_hip_ctx* ctx = nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!ctx) {
    const char* dev = std::getenv("AICP_HIP_DEVICE");
    const int rc = aicp_hip_create(dev ? std::atoi(dev) : 0, &ctx);
    if (rc != AICP_OK) {
      ctx = nullptr;
      throw std::runtime_error("aicp_hip_create failed (" + std::to_string(rc) + "): no usable HIP device");
    }
  }
  return ctx;
}

inline void risk_throw_on_error(int rc) {
  if (rc != AICP_OK)
    throw std::runtime_error("aicp_hip error " + std::to_string(rc) + ": " + aicp_hip_last_error(risk_ctx()));
}

inline aicp_cloud risk_cloud(const pcl::PointCloud<pcl::PointXYZ>& c) {
  aicp_cloud o{};
  o.pts = c.points.empty() ? nullptr : &c.points[0].x;
  o.n = c.points.size();
  o.stride = sizeof(pcl::PointXYZ);
  return o;
}

inline float overlapFilter(pcl::PointCloud<pcl::PointXYZ>& cloudA, pcl::PointCloud<pcl::PointXYZ>& cloudB,
                           Eigen::Isometry3d poseA, Eigen::Isometry3d poseB, float range, float angularView,
                           pcl::PointCloud<pcl::PointXYZ>& accepted_pointsA,
                           pcl::PointCloud<pcl::PointXYZ>& accepted_pointsB) {
  const aicp_cloud a = risk_cloud(cloudA), b = risk_cloud(cloudB);
  std::vector<float> ka(3 * a.n + 3), kb(3 * b.n + 3);
  size_t na = 0, nb = 0;
  float overlap = 0.f;
  risk_throw_on_error(aicp_hip_fov_overlap(risk_ctx(), &a, &b, poseA.data(), poseB.data(), range, angularView, &overlap,
                                           ka.data(), &na, kb.data(), &nb));
  for (size_t i = 0; i < na; ++i) {  // push_back, as the reference appends
    pcl::PointXYZ p;
    p.x = ka[3 * i], p.y = ka[3 * i + 1], p.z = ka[3 * i + 2];
    accepted_pointsA.push_back(p);
  }
  for (size_t i = 0; i < nb; ++i) {
    pcl::PointXYZ p;
    p.x = kb[3 * i], p.y = kb[3 * i + 1], p.z = kb[3 * i + 2];
    accepted_pointsB.push_back(p);
  }
  return overlap;
}

inline float alignabilityFilter(pcl::PointCloud<pcl::PointXYZ>& cloudA, pcl::PointCloud<pcl::PointXYZ>& cloudB,
                                Eigen::Isometry3d poseA, Eigen::Isometry3d poseB,
                                pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr cloudA_planes,
                                pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr cloudB_planes,
                                pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr eigenvectors) {
  aicp_hip_ctx* ctx = risk_ctx();
  aicp_risk_params prm;
  aicp_hip_default_risk_params(&prm);
  const aicp_cloud in[2] = {risk_cloud(cloudA), risk_cloud(cloudB)};
  const double* pose[2] = {poseA.data(), poseB.data()};
  std::vector<float> sampled[2];
  std::vector<int32_t> labels[2];
  size_t V[2] = {0, 0}, nc[2] = {0, 0};
  for (int x = 0; x < 2; ++x) {  // regionGrowingUniformPlaneSegmentationFilter(cloud, sampled, pose, clusters)
    aicp_prefilter_params pf = prm.prefilter;
    for (int k = 0; k < 3; ++k) pf.viewpoint[k] = (float)pose[x][12 + k];
    const size_t n = in[x].n;
    std::vector<float> out(3 * n + 3);
    sampled[x].resize(8 * n + 8);
    labels[x].resize(n + 1);
    size_t n_out = 0;
    risk_throw_on_error(aicp_hip_prefilter(ctx, &pf, in[x].pts, n, in[x].stride, out.data(), &n_out, sampled[x].data(),
                                           labels[x].data(), &V[x], &nc[x]));
  }
  std::vector<int32_t> idx(nc[1] + 1, -1);
  float alignability = 0.f;
  int32_t n_matches = 0;
  double ev[3], evec[9], cen[3];
  risk_throw_on_error(aicp_hip_cluster_match(ctx, sampled[0].data(), labels[0].data(), V[0], sampled[1].data(),
                                             labels[1].data(), V[1], prm.max_angle_deg, prm.box_scale, &alignability,
                                             &n_matches, idx.data(), nullptr, nullptr, ev, evec, cen, nullptr, nullptr,
                                             nullptr, nullptr));
  if (n_matches == 0) {
    std::cout << "[Filtering Utils] Error: No matching normals left." << std::endl;
    return 0;
  }
  for (size_t j = 0; j < nc[1]; ++j) {
    if (idx[j] < 0) continue;
    const int32_t want[2] = {idx[j], (int32_t)j};
    pcl::PointCloud<pcl::PointXYZRGBNormal>* dst[2] = {cloudA_planes.get(), cloudB_planes.get()};
    for (int x = 0; x < 2; ++x) {
      if (!dst[x]) continue;
      for (size_t i = 0; i < V[x]; ++i) {
        if (labels[x][i] != want[x]) continue;
        const float* q = &sampled[x][8 * i];
        pcl::PointXYZRGBNormal p;
        p.x = q[0], p.y = q[1], p.z = q[2];
        p.curvature = q[3];
        p.normal_x = q[4], p.normal_y = q[5], p.normal_z = q[6];
        p.rgb = (float)want[0];  // one value per matched pair
        dst[x]->push_back(p);
      }
    }
  }
  if (eigenvectors) {
    eigenvectors->points.resize(3);
    eigenvectors->width = 3;
    eigenvectors->height = 1;
    for (int i = 0; i < 3; ++i) {
      pcl::PointXYZRGBNormal& p = eigenvectors->points[i];
      p.x = (float)cen[0], p.y = (float)cen[1], p.z = (float)cen[2];
      p.normal_x = (float)evec[i], p.normal_y = (float)evec[3 + i], p.normal_z = (float)evec[6 + i];
    }
  }
  return alignability;
}

}  // namespace aicp_hip

#endif  // AICP_HIP_ALIGNABILITY_HPP_
