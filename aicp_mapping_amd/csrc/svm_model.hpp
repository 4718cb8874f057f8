// svm_model.hpp — the failure-prediction classifier's model (aicp_core/src/classification/svm.cpp
// loads it with cv::ml::SVM): what svm_model.cpp parses from the OpenCV model XML and what the
// device entry points (aicp_hip.cpp) read. Host only: no HIP header.
#pragma once
#include <cstdint>
#include <vector>

// decision-function entries the kernel stages in LDS (16 bytes each); more is AICP_ERR_UNSUPPORTED
constexpr int kSvmMaxEntries = 2048;

struct aicp_hip_svm {
  uint64_t id = 0;    // unique per loaded model in this process: the contexts' device copies are keyed by it
  int32_t format = 0; // 3: <opencv_ml_svm> with <format>3</format>; 0: the older <my_svm>
  double degree = 0, gamma = 0, coef0 = 0, rho = 0;
  int32_t var_count = 0, class_count = 0, sv_total = 0, sv_count = 0;
  bool has_index = false;
  std::vector<float> sv;       // var_count * sv_total
  std::vector<double> alpha;   // sv_count
  std::vector<int32_t> index;  // sv_count (the identity when the file has none)
};
