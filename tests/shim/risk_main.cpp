// Drives integration/hip_alignability.hpp the way App::computeAlignmentRisk does (app.cpp:143-185),
// against the stand-in PCL / Eigen types of stubs/risk.
//   risk_main cpu   no device: the defaults and the argument checks of the C-ABI
//   risk_main gpu   two synthetic clouds of three planes through overlapFilter and alignabilityFilter
#include <cmath>
#include <cstdio>
#include <cstring>

#include "hip_alignability.hpp"

static void plane(pcl::PointCloud<pcl::PointXYZ>& c, int axis, float at, float shift) {
  for (int i = 0; i < 60; ++i)
    for (int j = 0; j < 60; ++j) {
      const float u = 0.05f * i + shift + 0.013f * ((i * 7 + j * 3) % 5), v = 0.05f * j + 0.011f * ((i + j * 5) % 7);
      const float w = at + 0.004f * ((i * 3 + j) % 5);  // a little thickness: the boxes are not flat
      pcl::PointXYZ p;
      if (axis == 0) p.x = w, p.y = u, p.z = v;
      if (axis == 1) p.x = u, p.y = w, p.z = v;
      if (axis == 2) p.x = u, p.y = v, p.z = w;
      c.push_back(p);
    }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "cpu")) {
    aicp_risk_params prm;
    aicp_hip_default_risk_params(&prm);
    if (prm.max_angle_deg != 20.f || prm.box_scale[0] != 1.f || prm.box_scale[1] != 1.f || prm.box_scale[2] != 3.f ||
        prm.prefilter.leaf_size != 0.08f || prm.prefilter.normal_k != 30)
      return 1;
    float ov = 0;
    aicp_cloud none{};
    const double I[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    if (aicp_hip_fov_overlap(nullptr, &none, &none, I, I, 1.f, 360.f, &ov, nullptr, nullptr, nullptr, nullptr) !=
        AICP_ERR_INVALID)
      return 1;
    std::printf("cpu ok: angle %g scale %g %g %g\n", prm.max_angle_deg, prm.box_scale[0], prm.box_scale[1],
                prm.box_scale[2]);
    return 0;
  }
  pcl::PointCloud<pcl::PointXYZ> A, B, accA, accB;
  for (int axis = 0; axis < 3; ++axis) {
    plane(A, axis, 3.f, 0.f);
    plane(B, axis, 3.f, 0.02f);
  }
  Eigen::Isometry3d poseA = Eigen::Isometry3d::Identity(), poseB = Eigen::Isometry3d::Identity();
  poseA(0, 3) = 0.5, poseA(1, 3) = 0.5, poseA(2, 3) = 0.5;
  poseB(0, 3) = 0.6, poseB(1, 3) = 0.4, poseB(2, 3) = 0.5;
  const float fov = aicp_hip::overlapFilter(A, B, poseA, poseB, 50.f, 360.f, accA, accB);
  pcl::PointCloud<pcl::PointXYZRGBNormal>::Ptr planesA(new pcl::PointCloud<pcl::PointXYZRGBNormal>),
      planesB(new pcl::PointCloud<pcl::PointXYZRGBNormal>), eig(new pcl::PointCloud<pcl::PointXYZRGBNormal>);
  const float al = aicp_hip::alignabilityFilter(accA, accB, poseA, poseB, planesA, planesB, eig);
  std::printf("fov %.9g accepted %zu %zu\nalignability %.9g planes %zu %zu eig %zu\n", fov, accA.size(), accB.size(),
              al, planesA->size(), planesB->size(), eig->size());
  return 0;
}
