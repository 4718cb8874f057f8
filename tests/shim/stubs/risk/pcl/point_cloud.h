// Stand-in for <pcl/point_cloud.h>: points, width / height, push_back and the shared Ptr of the
// filteringUtils signatures (boost::shared_ptr in PCL 1.8; only get() and -> are used).
#pragma once
#include <stdint.h>

#include <cstddef>
#include <memory>
#include <vector>

namespace pcl {
template <class PointT>
struct PointCloud {
  typedef std::shared_ptr<PointCloud<PointT>> Ptr;
  std::vector<PointT> points;
  uint32_t width = 0, height = 1;
  size_t size() const { return points.size(); }
  void push_back(const PointT& p) {
    points.push_back(p);
    width = (uint32_t)points.size();
    height = 1;
  }
};
}  // namespace pcl
