// pm_config.cpp — host-side configuration handling of the drop-in boundary.
//
//   aicp_hip_parse_pm_yaml            the libpointmatcher chain subset loaded by
//                                     PointmatcherRegistration::applyConfig
//                                     (pointmatcher_registration.cpp:48-68, icp_.loadFromYaml)
//   aicp_hip_parse_pm_chain           the same files with their data-point filter lists and the
//                                     MaxDist outlier rule
//   aicp_hip_replace_ratio_config_file fileIO.cpp:179-214 (text rewrite, byte for byte)
//   aicp_hip_autotune_ratio           app.cpp:197-205 + the ostream/lexical_cast round trip
//
// yaml-cpp is not available in this image; the chain files only use block maps, block lists,
// plain scalars and comments, which the small parser below covers.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "../../include/aicp_hip.h"
#include "chain_draw.hpp"

namespace {

struct Y {
  enum T { Null, Scalar, Map, List } t = Null;
  std::string s;
  std::vector<std::pair<std::string, Y>> map;
  std::vector<Y> list;
  const Y* get(const std::string& k) const {
    if (t != Map) return nullptr;
    for (auto& kv : map)
      if (kv.first == k) return &kv.second;
    return nullptr;
  }
};

struct Line {
  int indent;
  std::string text;
};

std::string trim(const std::string& s) {
  size_t a = s.find_first_not_of(" \t\r");
  if (a == std::string::npos) return "";
  size_t b = s.find_last_not_of(" \t\r");
  return s.substr(a, b - a + 1);
}

std::string unquote(const std::string& s) {
  if (s.size() >= 2 && ((s.front() == '"' && s.back() == '"') || (s.front() == '\'' && s.back() == '\'')))
    return s.substr(1, s.size() - 2);
  return s;
}

std::vector<Line> lex(std::istream& in) {
  std::vector<Line> out;
  std::string raw;
  while (std::getline(in, raw)) {
    // strip comments ('#' at line start or after whitespace, outside quotes)
    bool sq = false, dq = false;
    size_t cut = std::string::npos;
    for (size_t i = 0; i < raw.size(); ++i) {
      const char c = raw[i];
      if (c == '\'' && !dq) sq = !sq;
      if (c == '"' && !sq) dq = !dq;
      if (c == '#' && !sq && !dq && (i == 0 || raw[i - 1] == ' ' || raw[i - 1] == '\t')) {
        cut = i;
        break;
      }
    }
    if (cut != std::string::npos) raw = raw.substr(0, cut);
    for (auto& ch : raw)
      if (ch == '\t') ch = ' ';
    const std::string t = trim(raw);
    if (t.empty() || t == "---") continue;
    int ind = 0;
    while (ind < (int)raw.size() && raw[ind] == ' ') ++ind;
    out.push_back({ind, t});
  }
  return out;
}

// split "key: value" / "key:" ; returns false if the text has no mapping colon
bool split_kv(const std::string& t, std::string& k, std::string& v) {
  size_t p = std::string::npos;
  for (size_t i = 0; i < t.size(); ++i)
    if (t[i] == ':' && (i + 1 == t.size() || t[i + 1] == ' ')) {
      p = i;
      break;
    }
  if (p == std::string::npos) return false;
  k = unquote(trim(t.substr(0, p)));
  v = trim(t.substr(p + 1));
  return true;
}

Y parse_block(const std::vector<Line>& L, size_t& i, int indent);

Y parse_value_after(const std::vector<Line>& L, size_t& i, int parent_indent, const std::string& v) {
  Y y;
  if (!v.empty()) {
    if (v == "{}" ) {
      y.t = Y::Map;
    } else if (v == "[]") {
      y.t = Y::List;
    } else {
      y.t = Y::Scalar;
      y.s = unquote(v);
    }
    return y;
  }
  if (i < L.size() && L[i].indent > parent_indent) return parse_block(L, i, L[i].indent);
  // a list may sit at the same indent as its key
  if (i < L.size() && L[i].indent == parent_indent && L[i].text.rfind("- ", 0) == 0)
    return parse_block(L, i, L[i].indent);
  return y;  // null
}

Y parse_block(const std::vector<Line>& L, size_t& i, int indent) {
  Y y;
  if (i >= L.size()) return y;
  const bool isList = L[i].text == "-" || L[i].text.rfind("- ", 0) == 0;
  if (isList) {
    y.t = Y::List;
    while (i < L.size() && L[i].indent == indent &&
           (L[i].text == "-" || L[i].text.rfind("- ", 0) == 0)) {
      const std::string item = trim(L[i].text.substr(1));
      const int item_indent = indent + 2;
      ++i;
      std::string k, v;
      if (item.empty()) {
        y.list.push_back(parse_value_after(L, i, indent, ""));
      } else if (split_kv(item, k, v)) {
        Y m;
        m.t = Y::Map;
        m.map.emplace_back(k, parse_value_after(L, i, item_indent, v));
        while (i < L.size() && L[i].indent == item_indent && L[i].text.rfind("- ", 0) != 0) {
          std::string k2, v2;
          if (!split_kv(L[i].text, k2, v2)) break;
          ++i;
          m.map.emplace_back(k2, parse_value_after(L, i, item_indent, v2));
        }
        y.list.push_back(m);
      } else {
        Y s;
        s.t = Y::Scalar;
        s.s = unquote(item);
        y.list.push_back(s);
      }
    }
    return y;
  }
  std::string k, v;
  if (!split_kv(L[i].text, k, v)) {  // bare scalar block ("inspector:\n  NullInspector")
    y.t = Y::Scalar;
    y.s = unquote(L[i].text);
    ++i;
    return y;
  }
  y.t = Y::Map;
  while (i < L.size() && L[i].indent == indent) {
    if (!split_kv(L[i].text, k, v)) break;
    ++i;
    y.map.emplace_back(k, parse_value_after(L, i, indent, v));
  }
  return y;
}

bool to_float(const Y* y, float& out) {
  if (!y || y->t != Y::Scalar) return false;
  const char* s = y->s.c_str();
  char* end = nullptr;
  const float v = std::strtof(s, &end);  // boost::lexical_cast<float>
  if (end == s) return false;
  out = v;
  return true;
}
bool to_int(const Y* y, int32_t& out) {
  float f;
  if (!to_float(y, f)) return false;
  out = (int32_t)f;
  return true;
}

// element of a filter/checker list: a map with one key (class name) -> params map
bool list_items(const Y* y, std::vector<std::pair<std::string, const Y*>>& out) {
  out.clear();
  if (!y || y->t == Y::Null) return true;
  if (y->t != Y::List) return false;
  for (auto& it : y->list) {
    if (it.t == Y::Scalar) {
      out.emplace_back(it.s, nullptr);
    } else if (it.t == Y::Map && it.map.size() == 1) {
      out.emplace_back(it.map[0].first, &it.map[0].second);
    } else {
      return false;
    }
  }
  return true;
}

// A single-key map ("matcher: {KDTreeMatcher: {...}}") or a bare name.
bool single(const Y* y, std::string& name, const Y*& params) {
  if (!y) return false;
  if (y->t == Y::Scalar) {
    name = y->s;
    params = nullptr;
    return true;
  }
  if (y->t == Y::Map && y->map.size() == 1) {
    name = y->map[0].first;
    params = &y->map[0].second;
    return true;
  }
  return false;
}

const Y* param(const Y* params, const char* k) { return params ? params->get(k) : nullptr; }

// One data-point filter of a side's list into the chain (aicp_hip_parse_pm_chain): its values,
// libpointmatcher's defaults where the file names none, and the checks of DESIGN §4.8.
// have_densities: a SurfaceNormal with keepDensities: 1 came earlier on this side.
int chain_filter_item(const std::string& name, const Y* prm, aicp_chain* ch, int side, bool& have_densities) {
  int32_t& n = ch->n_filters[side];
  aicp_chain_filter f;
  std::memset(&f, 0, sizeof(f));
  if (name == "SurfaceNormalDataPointsFilter") {
    for (int q = 0; q < n; ++q)
      if (ch->filters[side][q].kind == AICP_FILTER_SURFACE_NORMAL) return AICP_ERR_UNSUPPORTED;
    f.kind = AICP_FILTER_SURFACE_NORMAL;
    f.knn = 5;
    to_int(param(prm, "knn"), f.knn);
    to_int(param(prm, "keepDensities"), f.keep_densities);
    f.keep_densities = f.keep_densities ? 1 : 0;
    if (f.keep_densities) have_densities = true;
  } else if (name == "MinDistDataPointsFilter") {
    f.kind = AICP_FILTER_MIN_DIST;
    f.dim = -1;
    f.min_dist = 1.f;
    to_int(param(prm, "dim"), f.dim);
    to_float(param(prm, "minDist"), f.min_dist);
    if (f.dim < -1 || f.dim > 2) return AICP_ERR_INVALID;
  } else if (name == "RandomSamplingDataPointsFilter") {
    f.kind = AICP_FILTER_RANDOM_SAMPLING;
    f.prob = 0.75f;
    to_float(param(prm, "prob"), f.prob);
    if (!(f.prob >= 0.f && f.prob <= 1.f)) return AICP_ERR_INVALID;
  } else if (name == "MaxDensityDataPointsFilter") {
    f.kind = AICP_FILTER_MAX_DENSITY;
    f.max_density = 10.f;
    to_float(param(prm, "maxDensity"), f.max_density);
    if (!(f.max_density > 0.f)) return AICP_ERR_INVALID;
    if (!have_densities) return AICP_ERR_INVALID;  // libpointmatcher: InvalidField (no "densities" descriptor)
  } else {
    return AICP_ERR_UNSUPPORTED;
  }
  if (n >= AICP_CHAIN_MAX_FILTERS) return AICP_ERR_UNSUPPORTED;
  ch->filters[side][n++] = f;
  return AICP_OK;
}

int parse_pm_file(const char* path, aicp_icp_config* out, aicp_chain* chain);

}  // namespace

extern "C" {

void aicp_hip_default_config(aicp_icp_config* c) {
  // icp_autotuned_default.yaml:9-51
  c->knn_normals = 20;
  c->nn_epsilon = 3.16f;
  c->nn_max_dist = std::numeric_limits<float>::infinity();
  c->trimmed_ratio = 0.70f;
  c->max_iter = 20;
  c->min_diff_rot = 0.001f;
  c->min_diff_trans = 0.01f;
  c->smooth_length = 4;
  c->bucket_size = 8;
  c->knn_match = 1;
}

int aicp_hip_parse_pm_yaml(const char* path, aicp_icp_config* out) {
  if (!path || !out) return AICP_ERR_INVALID;
  return parse_pm_file(path, out, nullptr);
}

int aicp_hip_parse_pm_chain(const char* path, aicp_icp_config* out, aicp_chain* chain) {
  if (!path || !out || !chain) return AICP_ERR_INVALID;
  return parse_pm_file(path, out, chain);
}

float aicp_hip_chain_uniform(uint64_t seed, uint32_t slot, uint32_t i) { return aicp::chain_uniform(seed, slot, i); }

}  // extern "C"

namespace {

// chain == nullptr: aicp_hip_parse_pm_yaml, which refuses every data-point filter but SurfaceNormal
// and every outlier filter but TrimmedDist
int parse_pm_file(const char* path, aicp_icp_config* out, aicp_chain* chain) {
  std::ifstream f(path);
  if (!f.good()) return AICP_ERR_INVALID;  // "Cannot open config file" -> exit(1)
  std::vector<Line> L = lex(f);
  size_t i = 0;
  Y root = parse_block(L, i, L.empty() ? 0 : L[0].indent);
  if (root.t != Y::Map || i != L.size()) return AICP_ERR_INVALID;
  aicp_icp_config c;
  // libpointmatcher 1.2.x parameter defaults of the chain elements
  c.knn_normals = 5;
  c.nn_epsilon = 0.f;
  c.nn_max_dist = std::numeric_limits<float>::infinity();
  c.trimmed_ratio = 0.85f;
  c.max_iter = 40;
  c.min_diff_rot = 0.001f;
  c.min_diff_trans = 0.001f;
  c.smooth_length = 3;
  c.bucket_size = 8;
  c.knn_match = 1;
  bool haveRefNormals = false, haveCounter = false, haveDifferential = false;
  bool pointToPoint = false, refNormalsDropped = false;
  std::vector<std::pair<std::string, const Y*>> items;
  aicp_chain ch;
  std::memset(&ch, 0, sizeof(ch));
  bool sampled = false;  // the file holds an element that only the chain parser serves

  for (auto& kv : root.map) {
    const std::string& key = kv.first;
    const Y* v = &kv.second;
    if (key == "readingDataPointsFilters" || key == "referenceDataPointsFilters") {
      if (!list_items(v, items)) return AICP_ERR_INVALID;
      const int side = key == "referenceDataPointsFilters" ? AICP_CHAIN_REFERENCE : AICP_CHAIN_READING;
      bool haveDensities = false;
      for (auto& it : items) {
        if (chain) {
          if (const int rc = chain_filter_item(it.first, it.second, &ch, side, haveDensities)) return rc;
          if (it.first != "SurfaceNormalDataPointsFilter") {
            sampled = true;
            continue;
          }
        }
        if (it.first != "SurfaceNormalDataPointsFilter") return AICP_ERR_UNSUPPORTED;
        float eps = 0;
        if (to_float(param(it.second, "epsilon"), eps) && eps != 0.f) return AICP_ERR_UNSUPPORTED;
        int32_t keepNormals = 1;
        to_int(param(it.second, "keepNormals"), keepNormals);
        if (key == "referenceDataPointsFilters") {
          if (!keepNormals) refNormalsDropped = true;  // (refused below unless the minimizer ignores them)
          int32_t knn = 5;
          to_int(param(it.second, "knn"), knn);
          c.knn_normals = knn;
          haveRefNormals = true;
        }
      }
    } else if (key == "readingStepDataPointsFilters") {
      if (!list_items(v, items)) return AICP_ERR_INVALID;
      if (!items.empty()) return AICP_ERR_UNSUPPORTED;
    } else if (key == "matcher") {
      std::string name;
      const Y* p;
      if (!single(v, name, p)) return AICP_ERR_INVALID;
      if (name != "KDTreeMatcher") return AICP_ERR_UNSUPPORTED;
      to_int(param(p, "knn"), c.knn_match);
      to_float(param(p, "epsilon"), c.nn_epsilon);
      to_float(param(p, "maxDist"), c.nn_max_dist);
      int32_t st = 1;
      if (to_int(param(p, "searchType"), st) && st != 1) return AICP_ERR_UNSUPPORTED;
      if (c.knn_match != 1) return AICP_ERR_UNSUPPORTED;
    } else if (key == "outlierFilters") {
      if (!list_items(v, items)) return AICP_ERR_INVALID;
      if (chain && items.size() == 1 && items[0].first == "MaxDistOutlierFilter") {
        float maxDist = 1.f;
        to_float(param(items[0].second, "maxDist"), maxDist);
        // a finite limit: with +inf the readings without a match (d2 = inf) would pass d2 <= limit
        if (!(maxDist >= 0.f) || !std::isfinite(maxDist)) return AICP_ERR_INVALID;
        ch.outlier = AICP_OUTLIER_MAX_DIST;
        ch.outlier_limit_d2 = maxDist;  // libpointmatcher 1.2.x: compared with the squared distance as written
        sampled = true;
        continue;
      }
      if (items.size() != 1 || items[0].first != "TrimmedDistOutlierFilter") return AICP_ERR_UNSUPPORTED;
      to_float(param(items[0].second, "ratio"), c.trimmed_ratio);
    } else if (key == "errorMinimizer") {
      std::string name;
      const Y* p;
      if (!single(v, name, p)) return AICP_ERR_INVALID;
      if (name == "PointToPointErrorMinimizer") {
        // the bare name, as the reference's chain files write it. The map form
        // ("PointToPointErrorMinimizer:", with or without parameters) stays unsupported, as before
        if (p) return AICP_ERR_UNSUPPORTED;
        pointToPoint = true;
      } else {
        if (name != "PointToPlaneErrorMinimizer") return AICP_ERR_UNSUPPORTED;
        int32_t f2d = 0;
        if (to_int(param(p, "force2D"), f2d) && f2d) return AICP_ERR_UNSUPPORTED;
      }
    } else if (key == "transformationCheckers") {
      if (!list_items(v, items)) return AICP_ERR_INVALID;
      for (auto& it : items) {
        if (it.first == "CounterTransformationChecker") {
          to_int(param(it.second, "maxIterationCount"), c.max_iter);
          haveCounter = true;
        } else if (it.first == "DifferentialTransformationChecker") {
          to_float(param(it.second, "minDiffRotErr"), c.min_diff_rot);
          to_float(param(it.second, "minDiffTransErr"), c.min_diff_trans);
          to_int(param(it.second, "smoothLength"), c.smooth_length);
          haveDifferential = true;
        } else {
          return AICP_ERR_UNSUPPORTED;
        }
      }
    } else if (key == "transformations") {
      if (!list_items(v, items)) return AICP_ERR_INVALID;
      for (auto& it : items)
        if (it.first != "RigidTransformation") return AICP_ERR_UNSUPPORTED;
    } else if (key == "inspector" || key == "logger") {
      // observability only
    } else {
      return AICP_ERR_UNSUPPORTED;
    }
  }
  if (pointToPoint) {
    // the reference's SurfaceNormal output is unused, as the reading's is: the filter is optional
    // and ignored; knn_normals = 0 selects the minimizer (include/aicp_hip.h)
    c.knn_normals = 0;
  } else if (!haveRefNormals || refNormalsDropped) {
    return AICP_ERR_UNSUPPORTED;
  }
  if (!haveCounter) return AICP_ERR_UNSUPPORTED;
  if (!haveDifferential) {
    c.min_diff_rot = -1.f;  // never fires
    c.min_diff_trans = -1.f;
    c.smooth_length = 1;
  }
  if (chain && sampled) {
    // a SurfaceNormal whose output is used (a point-to-plane reference's normals, the densities
    // of a later MaxDensity) runs on the device's kNN: knn 10, 20 or 30. A file without the new
    // elements keeps aicp_hip_parse_pm_yaml's answer; the registration calls check its knn.
    for (int side = 0; side < 2; ++side) {
      bool consumed = side == AICP_CHAIN_REFERENCE && !pointToPoint;
      const aicp_chain_filter* sn = nullptr;
      for (int q = 0; q < ch.n_filters[side]; ++q) {
        const aicp_chain_filter& f = ch.filters[side][q];
        if (f.kind == AICP_FILTER_SURFACE_NORMAL) sn = &f;
        if (f.kind == AICP_FILTER_MAX_DENSITY) consumed = true;
      }
      if (sn && consumed && sn->knn != 10 && sn->knn != 20 && sn->knn != 30) return AICP_ERR_UNSUPPORTED;
    }
  }
  *out = c;
  if (chain) *chain = ch;
  return AICP_OK;
}

}  // namespace

extern "C" {

int aicp_hip_replace_ratio_config_file(const char* in_file, const char* out_file, float ratio) {
  if (!in_file || !out_file) return AICP_ERR_INVALID;
  std::ifstream in;
  in.open(in_file, std::fstream::in);
  std::ofstream out;
  out.open(out_file, std::ofstream::out);
  if (!in || !out) return AICP_ERR_INVALID;
  const std::string word = "ratio: ";
  std::stringstream with;
  with << "ratio: " << ratio;
  const std::string replacement = with.str();
  const size_t len = word.length() + 4;
  std::string line;
  while (!in.eof()) {  // the reference's loop, including its extra trailing newline
    std::getline(in, line);
    const size_t pos = line.find(word);
    if (pos != std::string::npos) line.replace(pos, len, replacement);
    out << line << '\n';
  }
  return AICP_OK;
}

float aicp_hip_autotune_ratio(float overlap_percent) {
  float current_ratio = overlap_percent / 100.0;
  if (current_ratio < 0.25)
    current_ratio = 0.25;
  else if (current_ratio > 0.70)
    current_ratio = 0.70;
  std::stringstream ss;
  ss << current_ratio;
  return std::strtof(ss.str().c_str(), nullptr);
}

}  // extern "C"
