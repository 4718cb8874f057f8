// svm_model.cpp — reader of the OpenCV SVM model XML that App's classifier loads
// (aicp_core/src/classification/svm.cpp, cv::ml::SVM::load; the models under
// aicp_core/data/classification). Host only, like pm_config.cpp: a small scanner for the subset of
// the format those files use, not an XML library. Both root forms are read: <opencv_ml_svm> with
// <format>3</format> (svmType) and the older <my_svm> (svm_type).
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/aicp_hip.h"
#include "svm_model.hpp"

namespace {

struct Span {
  size_t b = 0, e = 0;  // [b, e) of the document
  bool ok = false;
};

// the content of the first <name ...> ... </name> inside `in` (name followed by '>' or a blank)
Span element(const std::string& doc, Span in, const char* name) {
  const std::string open = std::string("<") + name, close = std::string("</") + name + ">";
  size_t p = in.b;
  for (;;) {
    p = doc.find(open, p);
    if (p == std::string::npos || p >= in.e) return {};
    const char c = p + open.size() < in.e ? doc[p + open.size()] : '\0';
    if (c == '>' || c == ' ' || c == '\t' || c == '\n' || c == '\r') break;
    p += open.size();
  }
  const size_t gt = doc.find('>', p);
  if (gt == std::string::npos || gt >= in.e) return {};
  const size_t q = doc.find(close, gt + 1);
  if (q == std::string::npos || q + close.size() > in.e) return {};
  return {gt + 1, q, true};
}

std::string trimmed(const std::string& doc, Span s) {
  size_t b = s.b, e = s.e;
  while (b < e && std::strchr(" \t\r\n", doc[b])) ++b;
  while (e > b && std::strchr(" \t\r\n", doc[e - 1])) --e;
  return doc.substr(b, e - b);
}

// every blank-separated number of the span; false when a token is no number
bool numbers(const std::string& doc, Span s, std::vector<double>* out) {
  const std::string t = doc.substr(s.b, s.e - s.b);
  const char* p = t.c_str();
  for (;;) {
    while (*p && std::strchr(" \t\r\n", *p)) ++p;
    if (!*p) return true;
    char* end = nullptr;
    errno = 0;
    const double v = std::strtod(p, &end);
    if (end == p || (*end && !std::strchr(" \t\r\n", *end))) return false;
    out->push_back(v);
    p = end;
  }
}

bool scalar(const std::string& doc, Span in, const char* name, double* out) {
  const Span s = element(doc, in, name);
  std::vector<double> v;
  if (!s.ok || !numbers(doc, s, &v) || v.size() != 1) return false;
  *out = v[0];
  return true;
}

bool integer(const std::string& doc, Span in, const char* name, int32_t* out) {
  double v;
  if (!scalar(doc, in, name, &v) || v != (double)(int32_t)v) return false;
  *out = (int32_t)v;
  return true;
}

std::atomic<uint64_t> g_next_id{1};

int parse(const std::string& doc, aicp_hip_svm* m) {
  const Span all{0, doc.size(), true};
  Span root = element(doc, all, "opencv_ml_svm");
  m->format = 3;
  if (!root.ok) {
    root = element(doc, all, "my_svm");
    m->format = 0;
  }
  if (!root.ok) return AICP_ERR_INVALID;  // (a truncated file has no closing root tag)
  Span type = element(doc, root, "svmType");
  if (!type.ok) type = element(doc, root, "svm_type");
  const Span kernel = element(doc, root, "kernel");
  if (!type.ok || !kernel.ok) return AICP_ERR_INVALID;
  const Span ktype = element(doc, kernel, "type");
  if (!ktype.ok) return AICP_ERR_INVALID;
  if (!integer(doc, root, "var_count", &m->var_count) || !integer(doc, root, "class_count", &m->class_count) ||
      !integer(doc, root, "sv_total", &m->sv_total))
    return AICP_ERR_INVALID;
  if (trimmed(doc, type) != "C_SVC" || trimmed(doc, ktype) != "POLY" || m->class_count != 2 || m->var_count != 2)
    return AICP_ERR_UNSUPPORTED;
  if (!scalar(doc, kernel, "degree", &m->degree) || !scalar(doc, kernel, "gamma", &m->gamma) ||
      !scalar(doc, kernel, "coef0", &m->coef0))
    return AICP_ERR_INVALID;
  if (m->sv_total < 1) return AICP_ERR_INVALID;
  // support_vectors: sv_total rows <_> v0 v1 </_>
  const Span svs = element(doc, root, "support_vectors");
  if (!svs.ok) return AICP_ERR_INVALID;
  Span rest = svs;
  for (;;) {
    const Span row = element(doc, rest, "_");
    if (!row.ok) break;
    std::vector<double> v;
    if (!numbers(doc, row, &v) || v.size() != (size_t)m->var_count) return AICP_ERR_INVALID;
    // the file holds floats printed with 9 significant digits: strtof's value (one rounding)
    const std::string t = doc.substr(row.b, row.e - row.b);
    const char* p = t.c_str();
    for (int k = 0; k < m->var_count; ++k) {
      char* end = nullptr;
      m->sv.push_back(std::strtof(p, &end));
      p = end;
    }
    rest.b = row.e;
  }
  if (m->sv.size() != (size_t)m->var_count * (size_t)m->sv_total) return AICP_ERR_INVALID;
  // the one decision function of a two-class model
  const Span dfs = element(doc, root, "decision_functions");
  if (!dfs.ok) return AICP_ERR_INVALID;
  const Span df = element(doc, dfs, "_");
  if (!df.ok) return AICP_ERR_INVALID;
  if (!integer(doc, df, "sv_count", &m->sv_count) || !scalar(doc, df, "rho", &m->rho)) return AICP_ERR_INVALID;
  const Span alpha = element(doc, df, "alpha");
  if (!alpha.ok || !numbers(doc, alpha, &m->alpha)) return AICP_ERR_INVALID;
  if (m->sv_count < 1 || m->alpha.size() != (size_t)m->sv_count) return AICP_ERR_INVALID;
  const Span index = element(doc, df, "index");
  m->has_index = index.ok;
  if (index.ok) {
    std::vector<double> v;
    if (!numbers(doc, index, &v) || v.size() != (size_t)m->sv_count) return AICP_ERR_INVALID;
    for (double x : v) {
      if (x != (double)(int32_t)x || x < 0 || x >= (double)m->sv_total) return AICP_ERR_INVALID;
      m->index.push_back((int32_t)x);
    }
  } else {
    if (m->sv_count > m->sv_total) return AICP_ERR_INVALID;
    for (int32_t j = 0; j < m->sv_count; ++j) m->index.push_back(j);
  }
  if (m->sv_count > kSvmMaxEntries) return AICP_ERR_UNSUPPORTED;
  return AICP_OK;
}

}  // namespace

extern "C" {

int aicp_hip_svm_load(const char* path, aicp_hip_svm** out) {
  if (!path || !out) return AICP_ERR_INVALID;
  *out = nullptr;
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return AICP_ERR_INVALID;
  std::string doc;
  char buf[4096];
  size_t k;
  while ((k = std::fread(buf, 1, sizeof(buf), f)) > 0) doc.append(buf, k);
  std::fclose(f);
  aicp_hip_svm* m = new aicp_hip_svm();
  const int rc = parse(doc, m);
  if (rc) {
    delete m;
    return rc;
  }
  m->id = g_next_id.fetch_add(1);
  *out = m;
  return AICP_OK;
}

void aicp_hip_svm_free(aicp_hip_svm* model) { delete model; }

int aicp_hip_svm_info(const aicp_hip_svm* m, aicp_svm_info* out, float* support_vectors, double* alpha,
                      int32_t* index) {
  if (!m || !out) return AICP_ERR_INVALID;
  *out = aicp_svm_info{};
  out->format = m->format;
  out->var_count = m->var_count;
  out->class_count = m->class_count;
  out->sv_total = m->sv_total;
  out->sv_count = m->sv_count;
  out->has_index = m->has_index ? 1 : 0;
  out->degree = m->degree;
  out->gamma = m->gamma;
  out->coef0 = m->coef0;
  out->rho = m->rho;
  if (support_vectors) std::memcpy(support_vectors, m->sv.data(), m->sv.size() * sizeof(float));
  if (alpha) std::memcpy(alpha, m->alpha.data(), m->alpha.size() * sizeof(double));
  if (index) std::memcpy(index, m->index.data(), m->index.size() * sizeof(int32_t));
  return AICP_OK;
}

}  // extern "C"
