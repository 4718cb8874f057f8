// Stand-in for <pcl/point_types.h> for integration/hip_alignability.hpp (PCL is not in this image):
// the memory layout and the members the header touches. pcl::PointXYZ is 16 B and
// PointXYZRGBNormal 48 B with x, y, z first, as in PCL 1.8.
#pragma once
namespace pcl {
struct alignas(16) PointXYZ {
  float x = 0, y = 0, z = 0, pad = 1;
};
struct alignas(16) PointXYZRGBNormal {
  float x = 0, y = 0, z = 0, pad = 1;
  float normal_x = 0, normal_y = 0, normal_z = 0, pad3 = 0;
  float rgb = 0, curvature = 0, pad4[2] = {0, 0};
};
static_assert(sizeof(PointXYZ) == 16 && sizeof(PointXYZRGBNormal) == 48, "PCL point layouts");
}  // namespace pcl
