// tas_oracle.cpp — CPU restatement of Kueue's TAS evaluation path.
//
// TEST INFRASTRUCTURE ONLY.  This file is the parity oracle (the checker) and
// the CPU baseline ("port") for bench.py.  Only tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg may load it.  The product path
// (kueue_oss_amd/, libkueue_tas.so) never links, loads or calls it.
//
// It restates, line by line and with the reference's own data structures
// (pointer tree, string-keyed ordered maps), the Go code of
//   /root/reference/pkg/cache/scheduler/tas_flavor_snapshot.go   (TASFlavorSnapshot)
//   /root/reference/pkg/cache/scheduler/tas_flavor.go            (snapshot construction)
//   /root/reference/pkg/cache/scheduler/tas_nodes_cache.go       (node filtering)
//   /root/reference/pkg/cache/scheduler/tas_non_tas_pod_cache.go (non-TAS usage)
//   /root/reference/pkg/resources/requests.go                    (CountIn arithmetic)
//   /root/reference/vendor/k8s.io/api/core/v1/toleration.go, taint.go
//   /root/reference/vendor/k8s.io/component-helpers/scheduling/corev1/helpers.go
//   label selectors and required node affinity: k8s_selectors.h
// Each function cites the reference file:line it follows.
//
// Parity pinning: tests/test_oracle_goldens.py checks this oracle against every
// in-scope golden case transcribed from the reference's own table test
// (pkg/cache/scheduler/tas_cache_test.go TestFindTopologyAssignments) by
// tools/extract_goldens.py.  The Go reference itself cannot run here (no Go
// toolchain).
//
// Deterministic choices where Go is not deterministic:
//   * CountInWithLimitingResource with >=2 missing requested keys returns the
//     first missing key in Go map order (random); we return the smallest name.
//   * Requests maps iterate in sorted key order (std::map).
//   * ValidatedSelectorFromSet with >=2 invalid entries reports the first in
//     Go map order (random); we report the smallest key's (k8s_selectors.h).
//   * findIncompleteSliceDomain with >=2 qualifying domains returns the
//     first in Go map order (random); we return the first in assignment order.
//   * TASBalancedPlacement iterates domainsPerLevel and domain.children in
//     Go map order (random); we iterate in lexicographic levelValues order,
//     and sortDomainsByCapacityAndEntropy's ties keep that order.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <limits>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <optional>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "k8s_selectors.h"
#include "mini_json.h"

namespace oracle {

using Requests = std::map<std::string, int64_t>;
static const char* kHostname = "kubernetes.io/hostname";

// ---- Go integer semantics -------------------------------------------------
static inline int32_t w_add(int32_t a, int32_t b) { return int32_t(uint32_t(a) + uint32_t(b)); }
static inline int32_t w_sub(int32_t a, int32_t b) { return int32_t(uint32_t(a) - uint32_t(b)); }
static inline int32_t w_mul(int32_t a, int32_t b) { return int32_t(uint32_t(a) * uint32_t(b)); }
static inline int64_t w_add64(int64_t a, int64_t b) { return int64_t(uint64_t(a) + uint64_t(b)); }
static inline int64_t w_sub64(int64_t a, int64_t b) { return int64_t(uint64_t(a) - uint64_t(b)); }
static inline int64_t w_mul64(int64_t a, int64_t b) { return int64_t(uint64_t(a) * uint64_t(b)); }
struct GoPanic : std::runtime_error { using std::runtime_error::runtime_error; };
static inline int32_t go_div32(int32_t a, int32_t b) {
  if (b == 0) throw GoPanic("integer divide by zero");
  if (a == INT32_MIN && b == -1) return INT32_MIN;
  return a / b;
}
static inline int64_t go_div64(int64_t a, int64_t b) {
  if (b == 0) throw GoPanic("integer divide by zero");
  if (a == INT64_MIN && b == -1) return INT64_MIN;
  return a / b;
}

// resources.Requests.Add / Sub (requests.go:84-94): keys of the operand are
// created in the receiver.
static void req_add(Requests& r, const Requests& o) { for (auto& kv : o) r[kv.first] = w_add64(r[kv.first], kv.second); }
static void req_sub(Requests& r, const Requests& o) { for (auto& kv : o) r[kv.first] = w_sub64(r[kv.first], kv.second); }
static Requests req_scaled_up(const Requests& r, int64_t f) {  // requests.go:53-57, :78-82
  Requests out = r;
  for (auto& kv : out) kv.second = w_mul64(kv.second, f);
  return out;
}

// Requests.CountInWithLimitingResource (requests.go:183-217).
static std::pair<int32_t, std::string> count_in_with_limiting(const Requests& r, const Requests& cap) {
  bool has = false;
  int32_t result = 0;
  std::string lim;
  for (auto& kv : r) {
    const std::string& name = kv.first;
    int64_t rv = kv.second;
    auto it = cap.find(name);
    if (it == cap.end() && rv != 0) return {0, name};
    int64_t capv = it == cap.end() ? 0 : it->second;
    int32_t count;
    if (rv == 0) {
      count = INT32_MAX;
    } else {
      int64_t q = go_div64(capv, rv);
      count = std::max(int32_t(uint32_t(uint64_t(q))), int32_t(0));
    }
    if (!has || count < result || (count == result && name < lim)) {
      result = count;
      lim = name;
      has = true;
    }
  }
  return {has ? result : 0, lim};
}
static int32_t count_in(const Requests& r, const Requests& cap) { return count_in_with_limiting(r, cap).first; }

// ---- k8s core types (subset) ----------------------------------------------
struct Taint { std::string key, value, effect; };
struct Toleration { std::string key, op, value, effect; };

// Taint.ToString (vendor/k8s.io/api/core/v1/taint.go:28-39)
static std::string taint_to_string(const Taint& t) {
  if (t.effect.empty()) {
    if (t.value.empty()) return t.key;
    return t.key + "=" + t.value + ":";
  }
  if (t.value.empty()) return t.key + ":" + t.effect;
  return t.key + "=" + t.value + ":" + t.effect;
}

// content.IsDecimalInteger + strconv.ParseInt (validate/content/decimal_int.go:30-62)
static bool parse_decimal_int(const std::string& v, int64_t* out) {
  size_t n = v.size();
  if (n == 0) return false;
  size_t i = 0;
  bool neg = false;
  if (v[0] == '-') {
    if (n == 1) return false;
    i = 1;
    neg = true;
  }
  if (v[i] == '0') {
    if (n == 1 && i == 0) { *out = 0; return true; }
    return false;
  }
  if (v[i] < '1' || v[i] > '9') return false;
  for (size_t j = i + 1; j < n; j++)
    if (v[j] < '0' || v[j] > '9') return false;
  // ParseInt range check
  unsigned __int128 acc = 0;
  for (size_t j = i; j < n; j++) {
    acc = acc * 10 + unsigned(v[j] - '0');
    if (acc > (unsigned __int128)INT64_MAX + 1) return false;
  }
  if (!neg && acc > (unsigned __int128)INT64_MAX) return false;
  *out = neg ? int64_t(uint64_t(0) - uint64_t(acc)) : int64_t(acc);
  return true;
}

// Toleration.ToleratesTaint (vendor/k8s.io/api/core/v1/toleration.go:52-112)
static bool tolerates_taint(const Toleration& t, const Taint& taint, bool enable_cmp) {
  if (!t.effect.empty() && t.effect != taint.effect) return false;
  if (!t.key.empty() && t.key != taint.key) return false;
  if (t.op.empty() || t.op == "Equal") return t.value == taint.value;
  if (t.op == "Exists") return true;
  if (t.op == "Lt" || t.op == "Gt") {
    if (!enable_cmp) return false;
    int64_t tv, nv;
    if (!parse_decimal_int(t.value, &tv)) return false;
    if (!parse_decimal_int(taint.value, &nv)) return false;
    return t.op == "Lt" ? nv < tv : nv > tv;
  }
  return false;
}

// corev1helpers.FindMatchingUntoleratedTaint with the NoSchedule/NoExecute filter
// (component-helpers/scheduling/corev1/helpers.go:79-102; tas_flavor_snapshot.go:1584-1586)
static const Taint* find_untolerated(const std::vector<Taint>& taints, const std::vector<Toleration>& tols) {
  for (auto& taint : taints) {
    if (!(taint.effect == "NoSchedule" || taint.effect == "NoExecute")) continue;
    bool tolerated = false;
    for (auto& tol : tols)
      if (tolerates_taint(tol, taint, true)) { tolerated = true; break; }
    if (!tolerated) return &taint;
  }
  return nullptr;
}

struct NodeInfo {  // tas_flavor.go:173-190
  std::string name;
  std::map<std::string, std::string> labels;
  std::vector<Taint> taints;
  Requests allocatable;
};

// ---- API types --------------------------------------------------------------
struct SliceConstraint { std::string topology; int32_t size; };
struct TopologyRequest {  // apis/kueue/v1beta2/workload_types.go:165-249
  std::optional<std::string> required, preferred, sliceRequiredTopology;
  std::optional<bool> unconstrained;
  std::optional<int32_t> sliceSize;
  std::vector<SliceConstraint> constraints;
};
struct PodSetRequest {  // TASPodSetRequests (tas_flavor_snapshot.go:356-367)
  std::string name;
  std::optional<TopologyRequest> topologyRequest;
  Requests singlePodRequests;
  int32_t count = 0;
  bool implied = false;
  std::optional<std::string> podSetGroupName;
  std::vector<Toleration> tolerations;
  std::optional<std::map<std::string, std::string>> nodeSelector;
  // affinity.nodeAffinity.requiredDuringSchedulingIgnoredDuringExecution (podset.go:104-144)
  std::optional<k8s::NodeSelector> requiredAffinity;
};
struct DomainAssignment { std::vector<std::string> values; int32_t count; };
struct TopologyAssignment { std::vector<std::string> levels; std::vector<DomainAssignment> domains; };
// TASPodSetRequests.PreviousAssignment (:364-366) of an elastic workload
// slice, in internal form (utiltas.InternalFrom of the v1beta2 value)
struct PreviousAssignments { std::map<std::string, TopologyAssignment> byName; };
struct PodSetResult { std::string name; std::optional<TopologyAssignment> assignment; std::string reason; };
// The parts of kueue.Workload the flavor search reads (WithWorkload,
// tas_flavor_snapshot.go:511-515): Status.UnhealthyNodes and the
// Admission's PodSetAssignments' TopologyAssignment (internal form,
// utiltas.InternalFrom).
struct WorkloadInfo {
  std::vector<std::string> unhealthyNodes;
  std::map<std::string, std::optional<TopologyAssignment>> psa;  // by PodSet name
};

struct Gates {  // pkg/features/kube_features.go:445-448 (TASProfileMixed Beta, default on)
  bool profileMixed = true;
  bool multiLayer = false;
  bool balanced = false;
  bool elastic = false;
};

// ---- snapshot ---------------------------------------------------------------
struct Domain {  // tas_flavor_snapshot.go:51-104 (domain + leafDomain)
  std::string id;
  Domain* parent = nullptr;
  std::vector<Domain*> children;
  int32_t state = 0, sliceState = 0, stateWithLeader = 0, sliceStateWithLeader = 0, leaderState = 0;
  std::vector<std::string> levelValues;
  bool isLeaf = false;
  Requests freeCapacity;
  Requests tasUsage;
  const NodeInfo* node = nullptr;
};

struct ExclusionStats {  // tas_flavor_snapshot.go:423-499
  std::map<std::string, int> taints;
  int nodeSelector = 0, affinity = 0, topologyDomain = 0;
  std::map<std::string, int> resources;
  int totalNodes = 0;
  bool has_exclusions() const {
    return nodeSelector > 0 || affinity > 0 || topologyDomain > 0 || !taints.empty() || !resources.empty();
  }
  std::string format_reasons() const;
};

// Go %q for the ASCII strings that occur here (strconv.Quote).
static std::string go_quote(const std::string& s) {
  std::string out = "\"";
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') { out += '\\'; out += char(c); }
    else if (c == '\n') out += "\\n";
    else if (c == '\t') out += "\\t";
    else if (c == '\r') out += "\\r";
    else if (c < 0x20 || c == 0x7f) { char b[8]; snprintf(b, sizeof b, "\\x%02x", c); out += b; }
    else out += char(c);
  }
  return out + "\"";
}

std::string ExclusionStats::format_reasons() const {
  std::vector<std::string> reasons;
  if (nodeSelector > 0) reasons.push_back("nodeSelector: " + std::to_string(nodeSelector));
  if (affinity > 0) reasons.push_back("affinity: " + std::to_string(affinity));
  if (topologyDomain > 0) reasons.push_back("topologyDomain: " + std::to_string(topologyDomain));
  for (auto& kv : taints) reasons.push_back("taint " + go_quote(kv.first) + ": " + std::to_string(kv.second));
  for (auto& kv : resources) reasons.push_back("resource " + go_quote(kv.first) + ": " + std::to_string(kv.second));
  std::sort(reasons.begin(), reasons.end());
  std::string out;
  for (size_t i = 0; i < reasons.size(); i++) {
    if (i) out += ", ";
    out += reasons[i];
  }
  return out;
}

struct Params {  // topologyAssignmentParameters + state (tas_flavor_snapshot.go:447-464)
  std::map<int, int32_t> sliceSizeAtLevel;
  int32_t sliceSize = 1, count = 0, leaderCount = 0;
  int requestedLevelIdx = 0, sliceLevelIdx = 0;
  bool required = false, unconstrained = false;
  std::vector<SliceConstraint> multiLayerConstraints;
  ExclusionStats stats;
};

struct Requirements {  // topologyAssignmentPodRequirements :434-443
  Requests requests;
  std::optional<Requests> leaderRequests;
  std::map<std::string, Requests>* assumedUsage = nullptr;
  std::vector<Toleration> tolerations;
  std::map<std::string, std::string> selector;  // empty = Everything
  std::optional<k8s::ParsedNodeSelector> affinitySelector;
  bool simulateEmpty = false;
  std::string requiredReplacementDomain;  // :441
};

static std::string domain_id(const std::vector<std::string>& v) {  // util/tas/tas.go:29-31
  std::string out;
  for (size_t i = 0; i < v.size(); i++) {
    if (i) out += ",";
    out += v[i];
  }
  return out;
}

static int compare_values(const std::vector<std::string>& a, const std::vector<std::string>& b) {  // slices.Compare
  size_t n = std::min(a.size(), b.size());
  for (size_t i = 0; i < n; i++) {
    int c = a[i].compare(b[i]);
    if (c != 0) return c < 0 ? -1 : 1;
  }
  if (a.size() == b.size()) return 0;
  return a.size() < b.size() ? -1 : 1;
}
static inline int cmp32(int32_t a, int32_t b) { return a < b ? -1 : (a > b ? 1 : 0); }

class Snapshot {
 public:
  std::string topologyName = "default";
  std::vector<std::string> levelKeys;
  std::map<std::string, Domain*> leaves, roots, domains;
  std::vector<std::map<std::string, Domain*>> domainsPerLevel;
  std::vector<Toleration> tolerations;
  bool isLowestLevelNode = false;
  Gates gates;
  std::deque<Domain> storage;
  std::deque<NodeInfo> nodes;

  Snapshot(const std::vector<std::string>& levels, const std::vector<Toleration>& tols) {  // :139-158
    levelKeys = levels;
    tolerations = tols;
    domainsPerLevel.resize(levels.size());
    isLowestLevelNode = !levels.empty() && levels.back() == kHostname;
  }

  static std::vector<std::string> level_values(const std::vector<std::string>& keys,
                                               const std::map<std::string, std::string>& labels) {
    std::vector<std::string> out;  // util/tas/tas.go:66-72
    for (auto& k : keys) {
      auto it = labels.find(k);
      out.push_back(it == labels.end() ? "" : it->second);
    }
    return out;
  }

  std::string add_node(const NodeInfo* node) {  // :160-195
    std::vector<std::string> levelValues;
    std::string id;
    bool found;
    if (isLowestLevelNode) {
      auto it = node->labels.find(kHostname);
      id = it == node->labels.end() ? "" : it->second;
      found = leaves.count(id) > 0;
      if (!found) levelValues = level_values(levelKeys, node->labels);
    } else {
      levelValues = level_values(levelKeys, node->labels);
      id = domain_id(levelValues);
      found = leaves.count(id) > 0;
    }
    if (!found) {
      storage.emplace_back();
      Domain* d = &storage.back();
      d->id = id;
      d->levelValues = levelValues;
      d->isLeaf = true;
      if (isLowestLevelNode) d->node = node;
      leaves[id] = d;
    }
    req_add(leaves[id]->freeCapacity, node->allocatable);  // addCapacity :243-248
    return id;
  }

  void initialize() {  // :210-217
    for (auto& kv : leaves) {
      Domain* d = kv.second;
      domains[d->id] = d;
      domainsPerLevel[d->levelValues.size() - 1][d->id] = d;
      initialize_helper(d);
    }
  }
  void initialize_helper(Domain* dom) {  // :220-241
    if (dom->levelValues.size() == 1) {
      roots[dom->id] = dom;
      return;
    }
    std::vector<std::string> parentValues(dom->levelValues.begin(), dom->levelValues.end() - 1);
    std::string parentID = domain_id(parentValues);
    Domain* parent;
    auto it = domains.find(parentID);
    if (it == domains.end()) {
      storage.emplace_back();
      parent = &storage.back();
      parent->id = parentID;
      parent->levelValues = parentValues;
      domainsPerLevel[parentValues.size() - 1][parentID] = parent;
      domains[parentID] = parent;
      initialize_helper(parent);
    } else {
      parent = it->second;
    }
    dom->parent = parent;
    parent->children.push_back(dom);
  }
  void add_non_tas_usage(const std::string& id, const Requests& usage) { req_sub(leaves[id]->freeCapacity, usage); }  // :250-255
  void add_tas_usage(const std::string& id, const Requests& usage) {  // :267-279
    auto it = leaves.find(id);
    if (it == leaves.end()) return;
    req_add(it->second->tasUsage, usage);
  }
  void update_tas_usage(const std::string& id, const Requests& usage, bool add, int32_t count) {  // :257-265
    Requests u = usage;
    req_add(u, Requests{{"pods", int64_t(count)}});
    auto it = leaves.find(id);
    if (it == leaves.end()) return;
    if (add) req_add(it->second->tasUsage, u);
    else req_sub(it->second->tasUsage, u);
  }

  // One workload.TopologyDomainRequests record (pkg/workload/workload.go:260-269).
  struct DomainUsage {
    std::vector<std::string> values;
    Requests single;
    int32_t count = 0;
  };
  // ClusterQueueSnapshot.AddUsage / RemoveUsage -> updateTASUsage
  // (clusterqueue_snapshot.go:94-119): TotalRequests = single.ScaledUp(count)
  // (workload.go:267-269), then :257-265 adds pods:count.
  void update_usage(const std::vector<DomainUsage>& us, bool add) {
    for (auto& u : us) update_tas_usage(domain_id(u.values), req_scaled_up(u.single, u.count), add, u.count);
  }
  // TASFlavorSnapshot.Fits (tas_flavor_snapshot.go:401-415): no pods:1 here.
  bool fits(const std::vector<DomainUsage>& us) const {
    for (auto& u : us) {
      auto it = leaves.find(domain_id(u.values));
      if (it == leaves.end()) return false;
      Requests remaining = it->second->freeCapacity;
      req_sub(remaining, it->second->tasUsage);
      if (count_in(u.single, remaining) < u.count) return false;
    }
    return true;
  }

  std::string lowest_level() const { return levelKeys.back(); }
  std::string highest_level() const { return levelKeys.front(); }
  bool use_lfc(bool unconstrained) const { return unconstrained && gates.profileMixed; }  // :1328-1331
  bool use_bf(bool unconstrained) const { return !use_lfc(unconstrained); }               // :1323-1326

  int resolve_level_idx(const std::string& key) const {  // :1104-1110
    for (size_t i = 0; i < levelKeys.size(); i++)
      if (levelKeys[i] == key) return int(i);
    return -1;
  }
  static bool is_slice_topology_only(const std::optional<TopologyRequest>& tr) {  // :1148-1153
    if (!tr || tr->required || tr->preferred) return false;
    return tr->sliceRequiredTopology.has_value() || !tr->constraints.empty();
  }
  std::optional<std::string> level_key(const std::optional<TopologyRequest>& tr) const {  // :1122-1138
    if (!tr) return std::nullopt;
    if (tr->required) return tr->required;
    if (tr->preferred) return tr->preferred;
    if (is_slice_topology_only(tr)) return highest_level();
    if (tr->unconstrained.value_or(false)) return lowest_level();
    return std::nullopt;
  }
  std::optional<std::string> level_key_with_implied_fallback(const PodSetRequest& r) const {  // :1112-1120
    if (auto k = level_key(r.topologyRequest)) return k;
    if (r.implied) return lowest_level();
    return std::nullopt;
  }
  std::string slice_level_key_with_default(const std::optional<TopologyRequest>& tr, const std::string& def) const {  // :1092-1102
    if (tr) {
      if (tr->sliceRequiredTopology) return *tr->sliceRequiredTopology;
      if (!tr->constraints.empty()) return tr->constraints[0].topology;
    }
    return def;
  }
  static std::pair<int32_t, std::string> slice_size_with_single_pod_default(const std::optional<TopologyRequest>& tr) {  // :1162-1180
    if (!tr) return {1, ""};
    if (!tr->constraints.empty()) return {tr->constraints[0].size, ""};
    if (!tr->sliceRequiredTopology) return {1, ""};
    if (!tr->sliceSize) return {0, "slice topology requested, but slice size not provided"};
    return {*tr->sliceSize, ""};
  }

  std::string build_slice_size_at_level(const PodSetRequest& w, int32_t sliceSize, int sliceLevelIdx,
                                        std::map<int, int32_t>& out) const {  // :1018-1063
    out.clear();
    if (!gates.multiLayer || !w.topologyRequest) return "";
    int32_t prevSize = sliceSize;
    int prevLevelIdx = sliceLevelIdx;
    const auto& cs = w.topologyRequest->constraints;
    for (size_t i = 1; i < cs.size(); i++) {
      const auto& layer = cs[i];
      int inner = resolve_level_idx(layer.topology);
      if (inner < 0) return "no requested topology level for additional slice layer: " + layer.topology;
      if (inner <= prevLevelIdx)
        return "additional slice layer topology " + layer.topology + " must be at a lower level than " + levelKeys[prevLevelIdx];
      if (layer.size == 0) throw GoPanic("integer divide by zero");
      if (prevSize % layer.size != 0)
        return "additional slice layer size " + std::to_string(layer.size) + " must evenly divide parent layer size " +
               std::to_string(prevSize);
      for (int lvl = prevLevelIdx + 1; lvl <= inner; lvl++) out[lvl] = layer.size;
      prevSize = layer.size;
      prevLevelIdx = inner;
    }
    return "";
  }

  // ---- phase 1 ----
  void fill_in_counts(const Requirements& rq, Params& st) {  // :1568-1647
    for (auto& kv : domains) {
      Domain* d = kv.second;
      d->state = d->stateWithLeader = d->sliceState = d->sliceStateWithLeader = d->leaderState = 0;
    }
    for (auto& kv : leaves) {
      Domain* leaf = kv.second;
      st.stats.totalNodes++;
      if (isLowestLevelNode) {
        const Taint* t = find_untolerated(leaf->node->taints, rq.tolerations);
        if (t) {
          st.stats.taints[taint_to_string(*t)]++;
          continue;
        }
        bool match = true;
        for (auto& sel : rq.selector) {
          auto it = leaf->node->labels.find(sel.first);
          if (it == leaf->node->labels.end() || it->second != sel.second) { match = false; break; }
        }
        if (!match) {
          st.stats.nodeSelector++;
          continue;
        }
        // required node affinity against leaf.node.toNode() (:1605-1610; tas_flavor.go:196-209)
        if (rq.affinitySelector && !rq.affinitySelector->match(leaf->node->labels, leaf->node->name)) {
          st.stats.affinity++;
          continue;
        }
      }
      // belongsToRequiredDomain (:1613-1617, :1649-1656): DomainID(levelValues) string prefix
      if (!rq.requiredReplacementDomain.empty() &&
          domain_id(leaf->levelValues).compare(0, rq.requiredReplacementDomain.size(), rq.requiredReplacementDomain) != 0) {
        st.stats.topologyDomain++;
        continue;
      }
      Requests remaining = leaf->freeCapacity;
      if (!rq.simulateEmpty) req_sub(remaining, leaf->tasUsage);
      if (rq.assumedUsage) {
        auto it = rq.assumedUsage->find(leaf->id);
        if (it != rq.assumedUsage->end()) req_sub(remaining, it->second);
      }
      auto cl = count_in_with_limiting(rq.requests, remaining);
      leaf->state = cl.first;
      if (leaf->state == 0 && !cl.second.empty()) st.stats.resources[cl.second]++;
      leaf->leaderState = 0;
      if (rq.leaderRequests && count_in(*rq.leaderRequests, remaining) > 0) {
        leaf->leaderState = 1;
        req_sub(remaining, *rq.leaderRequests);
      }
      leaf->stateWithLeader = count_in(rq.requests, remaining);
    }
    for (auto& kv : roots) fill_in_counts_helper(kv.second, st.sliceSize, st.sliceLevelIdx, 0, st.sliceSizeAtLevel, st.leaderCount > 0);
  }

  void fill_in_counts_helper(Domain* d, int32_t sliceSize, int sliceLevelIdx, int level,
                             const std::map<int, int32_t>& sizeAt, bool leaderRequired) {  // :1658-1719
    if (d->children.empty()) {
      if (level == sliceLevelIdx) {
        d->sliceState = go_div32(d->state, sliceSize);
        d->sliceStateWithLeader = go_div32(d->stateWithLeader, sliceSize);
      }
      return;
    }
    int32_t childrenCapacity = 0, sliceCapacity = 0;
    bool hasContributor = false;
    int32_t minDiff = INT32_MAX, minSliceDiff = INT32_MAX, leaderState = 0;
    int childLevel = level + 1;
    auto it = sizeAt.find(childLevel);
    bool hasInner = it != sizeAt.end();
    int32_t innerSize = hasInner ? it->second : 0;
    for (Domain* c : d->children) {
      fill_in_counts_helper(c, sliceSize, sliceLevelIdx, childLevel, sizeAt, leaderRequired);
      int32_t cs = c->state, csw = c->stateWithLeader;
      if (hasInner) {
        cs = w_mul(go_div32(c->state, innerSize), innerSize);
        csw = w_mul(go_div32(c->stateWithLeader, innerSize), innerSize);
      }
      childrenCapacity = w_add(childrenCapacity, cs);
      sliceCapacity = w_add(sliceCapacity, c->sliceState);
      if (!leaderRequired || c->leaderState > 0) {
        hasContributor = true;
        minDiff = std::min(w_sub(cs, csw), minDiff);
        minSliceDiff = std::min(w_sub(c->sliceState, c->sliceStateWithLeader), minSliceDiff);
      }
      leaderState = std::max(c->leaderState, leaderState);
    }
    d->state = childrenCapacity;
    int32_t sswl = 0;
    if (hasContributor) {
      d->stateWithLeader = w_sub(childrenCapacity, minDiff);
      sswl = w_sub(sliceCapacity, minSliceDiff);
    } else {
      d->stateWithLeader = 0;
    }
    d->leaderState = leaderState;
    if (level == sliceLevelIdx) {
      sliceCapacity = go_div32(d->state, sliceSize);
      sswl = go_div32(d->stateWithLeader, sliceSize);
    }
    d->sliceState = sliceCapacity;
    d->sliceStateWithLeader = sswl;
  }

  // ---- phase 2 helpers ----
  std::vector<Domain*> sorted_domains_with_leader(std::vector<Domain*> v, bool unconstrained) const {  // :1511-1535
    bool lfc = use_lfc(unconstrained);
    std::sort(v.begin(), v.end(), [&](Domain* a, Domain* b) {
      int c;
      if (a->leaderState != b->leaderState) c = cmp32(b->leaderState, a->leaderState);
      else if (a->sliceStateWithLeader != b->sliceStateWithLeader)
        c = lfc ? cmp32(a->sliceStateWithLeader, b->sliceStateWithLeader) : cmp32(b->sliceStateWithLeader, a->sliceStateWithLeader);
      else if (a->stateWithLeader != b->stateWithLeader) c = cmp32(a->stateWithLeader, b->stateWithLeader);
      else c = compare_values(a->levelValues, b->levelValues);
      return c < 0;
    });
    return v;
  }
  std::vector<Domain*> sorted_domains(std::vector<Domain*> v, bool unconstrained) const {  // :1544-1564
    bool lfc = use_lfc(unconstrained);
    std::sort(v.begin(), v.end(), [&](Domain* a, Domain* b) {
      int c;
      if (a->sliceState != b->sliceState) c = lfc ? cmp32(a->sliceState, b->sliceState) : cmp32(b->sliceState, a->sliceState);
      else if (a->state != b->state) c = cmp32(a->state, b->state);
      else c = compare_values(a->levelValues, b->levelValues);
      return c < 0;
    });
    return v;
  }
  template <typename F>
  static Domain* find_best_fit_by(const std::vector<Domain*>& ds, size_t from, int32_t needed, F state) {  // :1216-1231
    Domain* best = ds[from];
    int32_t bestState = state(best);
    for (size_t i = from; i < ds.size(); i++) {
      int32_t s = state(ds[i]);
      if (s >= needed && s < bestState) {
        best = ds[i];
        bestState = state(best);
      }
    }
    return best;
  }
  static Domain* find_best_fit(const std::vector<Domain*>& ds, size_t from, int32_t count, int32_t leaderCount) {  // :1186-1196
    if (leaderCount > 0) return find_best_fit_by(ds, from, count, [](Domain* d) { return d->stateWithLeader; });
    return find_best_fit_by(ds, from, count, [](Domain* d) { return d->state; });
  }
  static Domain* find_best_fit_for_slices(const std::vector<Domain*>& ds, size_t from, int32_t n, int32_t leaderCount) {  // :1202-1212
    if (leaderCount > 0) return find_best_fit_by(ds, from, n, [](Domain* d) { return d->sliceStateWithLeader; });
    return find_best_fit_by(ds, from, n, [](Domain* d) { return d->sliceState; });
  }

  std::string not_fit_message(int32_t fit, int32_t total, int32_t sliceSize, const ExclusionStats& stats) const {  // :1721-1741
    std::string unit = sliceSize == 1 ? "pod" : "slice";
    std::string out;
    if (fit == 0)
      out = "topology " + go_quote(topologyName) + " doesn't allow to fit any of " + std::to_string(total) + " " + unit + "(s)";
    else
      out = "topology " + go_quote(topologyName) + " allows to fit only " + std::to_string(fit) + " out of " +
            std::to_string(total) + " " + unit + "(s)";
    if (stats.has_exclusions())
      out += ". Total nodes: " + std::to_string(stats.totalNodes) + "; excluded: " + stats.format_reasons();
    return out;
  }
  static int32_t count_slices_in_subtree(Domain* d, int cur, int target, int32_t sliceSize) {  // :1743-1752
    if (cur == target) return go_div32(d->state, sliceSize);
    int32_t total = 0;
    for (Domain* c : d->children) total = w_add(total, count_slices_in_subtree(c, cur + 1, target, sliceSize));
    return total;
  }
  std::string multi_layer_not_fit_message(int reqLevel, int32_t count, const std::vector<SliceConstraint>& cs,
                                          const ExclusionStats& stats) const {  // :1754-1793
    std::string out = "topology " + go_quote(topologyName) + " doesn't allow to fit";
    Domain* best = nullptr;
    for (auto& kv : domainsPerLevel[reqLevel]) {
      Domain* d = kv.second;
      if (!best || d->sliceState > best->sliceState || (d->sliceState == best->sliceState && d->id < best->id)) best = d;
    }
    if (!best) return out;
    for (auto& c : cs) {
      int t = resolve_level_idx(c.topology);
      if (t < 0) continue;
      int32_t needed = go_div32(count, c.size);
      int32_t fit = count_slices_in_subtree(best, reqLevel, t, c.size);
      out += "; " + std::to_string(fit) + "/" + std::to_string(needed) + " slice(s) fit on level " + c.topology;
    }
    if (stats.has_exclusions())
      out += ". Total nodes: " + std::to_string(stats.totalNodes) + "; excluded: " + stats.format_reasons();
    return out;
  }

  // findLevelWithFitDomains (:1236-1321)
  std::string find_level_with_fit_domains(int searchLevelIdx, Params& st, int* fitLevel, std::vector<Domain*>* out) {
    auto& doms = domainsPerLevel[searchLevelIdx];
    if (doms.empty()) return "no topology domains at level: " + levelKeys[searchLevelIdx];
    std::vector<Domain*> levelDomains;
    for (auto& kv : doms) levelDomains.push_back(kv.second);
    std::vector<Domain*> sorted = sorted_domains_with_leader(levelDomains, st.unconstrained);
    Domain* top = sorted[0];
    int32_t sliceCount = go_div32(st.count, st.sliceSize);
    if (use_bf(st.unconstrained) && top->sliceStateWithLeader >= sliceCount && top->leaderState >= st.leaderCount)
      top = find_best_fit_for_slices(sorted, 0, sliceCount, st.leaderCount);
    auto notFit = [&](int32_t fit, int32_t total) {
      if (!st.multiLayerConstraints.empty())
        return multi_layer_not_fit_message(searchLevelIdx, st.count, st.multiLayerConstraints, st.stats);
      return not_fit_message(fit, total, st.sliceSize, st.stats);
    };
    if (use_lfc(st.unconstrained)) {
      for (Domain* c : sorted)
        if (c->sliceState >= sliceCount) {
          *fitLevel = searchLevelIdx;
          *out = {c};
          return "";
        }
      if (st.required) return notFit(sorted.back()->state, sliceCount);
    }
    if (top->sliceStateWithLeader < sliceCount || top->leaderState < st.leaderCount) {
      if (st.required) return notFit(top->sliceState, sliceCount);
      if (searchLevelIdx > 0 && !st.unconstrained) return find_level_with_fit_domains(searchLevelIdx - 1, st, fitLevel, out);
      std::vector<Domain*> results;
      int32_t remSlices = sliceCount, remLeaders = st.leaderCount;
      size_t idx = 0;
      for (; remLeaders > 0 && idx < sorted.size() && sorted[idx]->leaderState > 0; idx++) {
        Domain* d = sorted[idx];
        if (use_bf(st.unconstrained) && sorted[idx]->sliceStateWithLeader >= remSlices)
          d = find_best_fit_for_slices(sorted, idx, remSlices, remLeaders);
        results.push_back(d);
        remLeaders = w_sub(remLeaders, d->leaderState);
        remSlices = w_sub(remSlices, d->sliceStateWithLeader);
      }
      if (remLeaders > 0) return notFit(w_sub(st.leaderCount, remLeaders), sliceCount);
      std::vector<Domain*> rest(sorted.begin() + idx, sorted.end());
      sorted = sorted_domains(rest, st.unconstrained);
      for (size_t i = 0; remSlices > 0 && i < sorted.size(); i++) {
        Domain* d = sorted[i];
        if (use_bf(st.unconstrained) && sorted[i]->sliceState >= remSlices) d = find_best_fit_for_slices(sorted, i, remSlices, 0);
        results.push_back(d);
        remSlices = w_sub(remSlices, d->sliceState);
      }
      if (remSlices > 0) return notFit(w_sub(sliceCount, remSlices), sliceCount);
      *fitLevel = searchLevelIdx;
      *out = results;
      return "";
    }
    *fitLevel = searchLevelIdx;
    *out = {top};
    return "";
  }

  // consumeWithLeadersGeneric (:1348-1403).  `wl`/`pr` select the fields.
  enum Field { F_STATE, F_SLICE, F_SWL, F_SSWL };
  static int32_t& fld(Domain* d, Field f) {
    switch (f) {
      case F_STATE: return d->state;
      case F_SLICE: return d->sliceState;
      case F_SWL: return d->stateWithLeader;
      default: return d->sliceStateWithLeader;
    }
  }
  Domain* consume_with_leaders(Domain* domain, const std::vector<Domain*>& ds, size_t from, int32_t* remPrimary,
                               int32_t* remLeaders, bool unconstrained, Field wl, Field pr, int32_t sliceSize,
                               bool slices, bool* completed) {
    if (use_bf(unconstrained) && fld(domain, wl) >= *remPrimary && domain->leaderState >= *remLeaders) {
      if (slices) {
        domain = find_best_fit_for_slices(ds, from, *remPrimary, *remLeaders);
        wl = F_SSWL;
        pr = F_SLICE;
      } else {
        domain = find_best_fit(ds, from, *remPrimary, *remLeaders);
        wl = F_SWL;
        pr = F_STATE;
      }
    }
    if (fld(domain, wl) >= *remPrimary && domain->leaderState >= *remLeaders) {
      fld(domain, pr) = *remPrimary;
      domain->leaderState = *remLeaders;
      domain->state = w_mul(*remPrimary, sliceSize);
      *completed = true;
      return domain;
    }
    if (slices) {
      if (fld(domain, wl) > *remPrimary) fld(domain, wl) = *remPrimary;
      if (domain->leaderState > *remLeaders) domain->leaderState = *remLeaders;
      domain->state = w_mul(fld(domain, wl), sliceSize);
      *remLeaders = w_sub(*remLeaders, domain->leaderState);
      *remPrimary = w_sub(*remPrimary, fld(domain, wl));
      *completed = false;
      return domain;
    }
    *remPrimary = w_sub(*remPrimary, fld(domain, wl));
    *remLeaders = w_sub(*remLeaders, domain->leaderState);
    if (fld(domain, wl) > *remPrimary) fld(domain, wl) = *remPrimary;
    if (domain->leaderState > *remLeaders) domain->leaderState = *remLeaders;
    *completed = false;
    return domain;
  }

  // updateCountsToMinimumGeneric (:1405-1469).  Returns false on the
  // "code assumptions violated" path (Go returns nil).
  bool update_counts_to_minimum(const std::vector<Domain*>& ds, int32_t count, int32_t leaderCount, int32_t sliceSize,
                                bool unconstrained, bool slices, std::vector<Domain*>* result) {
    result->clear();
    int32_t remPrimary = slices ? go_div32(count, sliceSize) : count;
    int32_t remLeaders = leaderCount;
    for (size_t i = 0; i < ds.size(); i++) {
      Domain* dom = ds[i];
      if (remLeaders > 0) {
        bool completed = false;
        Domain* d = slices ? consume_with_leaders(dom, ds, i, &remPrimary, &remLeaders, unconstrained, F_SSWL, F_SLICE,
                                                  sliceSize, true, &completed)
                           : consume_with_leaders(dom, ds, i, &remPrimary, &remLeaders, unconstrained, F_SWL, F_STATE, 1,
                                                  false, &completed);
        result->push_back(d);
        if (completed) return true;
        continue;
      }
      if (slices) {
        if (use_bf(unconstrained) && dom->sliceState >= remPrimary) dom = find_best_fit_for_slices(ds, i, remPrimary, 0);
        dom->leaderState = 0;
        if (dom->sliceState >= remPrimary) {
          dom->state = w_mul(remPrimary, sliceSize);
          dom->sliceState = remPrimary;
          result->push_back(dom);
          return true;
        }
        dom->state = w_mul(dom->sliceState, sliceSize);
        remPrimary = w_sub(remPrimary, dom->sliceState);
        result->push_back(dom);
        continue;
      }
      if (use_bf(unconstrained) && dom->state >= remPrimary) dom = find_best_fit(ds, i, remPrimary, 0);
      dom->leaderState = 0;
      if (dom->state >= remPrimary) {
        dom->state = remPrimary;
        result->push_back(dom);
        return true;
      }
      remPrimary = w_sub(remPrimary, dom->state);
      result->push_back(dom);
    }
    result->clear();
    return false;
  }

  TopologyAssignment build_assignment(std::vector<Domain*> ds) const {  // :1490-1501 + :1472-1488
    std::stable_sort(ds.begin(), ds.end(), [](Domain* a, Domain* b) { return compare_values(a->levelValues, b->levelValues) < 0; });
    size_t levelIdx = isLowestLevelNode ? levelKeys.size() - 1 : 0;
    TopologyAssignment ta;
    ta.levels.assign(levelKeys.begin() + levelIdx, levelKeys.end());
    for (Domain* d : ds) {
      if (d->state == 0) continue;
      ta.domains.push_back({std::vector<std::string>(d->levelValues.begin() + levelIdx, d->levelValues.end()), d->state});
    }
    return ta;
  }

  static std::vector<Domain*> lower_level_domains(const std::vector<Domain*>& ds) {  // :1503-1509
    std::vector<Domain*> out;
    for (Domain* d : ds) out.insert(out.end(), d->children.begin(), d->children.end());
    return out;
  }

  // ---- TASBalancedPlacement (pkg/cache/scheduler/tas_balanced_placement.go) ----
  // Where Go iterates a map — domainsPerLevel (:243-246) and every
  // domain.children slice, which initialize (:210-241) fills in the random
  // order of the s.leaves map — this restatement iterates in lexicographic
  // levelValues order (slices.Compare), the order of the other comparators'
  // final tie-break; sortDomainsByCapacityAndEntropy (:211-231, pdqsort with
  // a comparator that ties on equal entropy) is a stable insertion sort.  The
  // product (tas_balanced.h) uses the same rules.  Only inputs with such ties
  // can differ from a given Go run, and those differ between Go runs too.
  std::deque<Domain> clones;  // cloneDomain storage of one find_topology_assignment call
  static std::vector<Domain*> lex_sorted(std::vector<Domain*> v) {
    std::stable_sort(v.begin(), v.end(), [](Domain* a, Domain* b) { return compare_values(a->levelValues, b->levelValues) < 0; });
    return v;
  }
  static std::vector<Domain*> level_domains_lex(const std::map<std::string, Domain*>& m) {
    std::vector<Domain*> v;
    for (auto& kv : m) v.push_back(kv.second);
    return lex_sorted(v);
  }
  Domain* clone_domain(const Domain* d, Domain* parent) {  // :351-359
    clones.push_back(*d);
    Domain* c = &clones.back();
    c->parent = parent;
    c->children.clear();
    for (Domain* k : lex_sorted(d->children)) c->children.push_back(clone_domain(k, c));
    return c;
  }
  std::vector<Domain*> clone_domains(const std::vector<Domain*>& ds) {  // :343-349
    std::vector<Domain*> out;
    for (Domain* d : ds) out.push_back(clone_domain(d, nullptr));
    return out;
  }
  static void clear_state(Domain* d) {  // :323-332
    d->state = d->sliceState = d->stateWithLeader = d->sliceStateWithLeader = d->leaderState = 0;
    for (Domain* c : d->children) clear_state(c);
  }
  static void clear_leader_capacity(Domain* d) {  // :334-341
    d->stateWithLeader = d->sliceStateWithLeader = d->leaderState = 0;
    for (Domain* c : d->children) clear_leader_capacity(c);
  }
  static void prune_node(Domain* d, int32_t threshold, bool leaderRequired) {  // :361-370
    if (d->sliceState < threshold) {
      clear_state(d);
      return;
    }
    if (leaderRequired && d->leaderState > 0 && d->sliceStateWithLeader < threshold) clear_leader_capacity(d);
  }
  void prune_domains(const std::vector<Domain*>& ds, int32_t threshold, int32_t sliceSize, int sliceLevelIdx, int level,
                     bool leaderRequired) {  // :372-382
    for (Domain* d : ds)
      for (Domain* c : d->children) prune_node(c, threshold, leaderRequired);
    for (Domain* d : ds) {
      fill_in_counts_helper(d, sliceSize, sliceLevelIdx, level, std::map<int, int32_t>{}, leaderRequired);
      prune_node(d, threshold, leaderRequired);
    }
  }
  struct Greedy {
    bool fit = false;
    int32_t count = 0;
    Domain* lastWithLeader = nullptr;
    Domain* last = nullptr;
  };
  Greedy evaluate_greedy(const std::vector<Domain*>& ds, int32_t sliceCount, int32_t leaderCount) const {  // :30-63
    Greedy g;
    int32_t remS = sliceCount, remL = leaderCount;
    std::vector<Domain*> withoutLeader;
    size_t idx = 0;
    if (leaderCount > 0) {
      std::vector<Domain*> wl = sorted_domains_with_leader(ds, false);
      for (; remL > 0 && idx < wl.size() && wl[idx]->leaderState > 0; idx++) {
        g.count = w_add(g.count, 1);
        g.lastWithLeader = wl[idx];
        remL = w_sub(remL, wl[idx]->leaderState);
        remS = w_sub(remS, wl[idx]->sliceStateWithLeader);
      }
      withoutLeader = sorted_domains(std::vector<Domain*>(wl.begin() + int64_t(idx), wl.end()), false);
    } else {
      withoutLeader = sorted_domains(ds, false);
    }
    if (remL > 0) return Greedy{};
    for (idx = 0; remS > 0 && idx < withoutLeader.size() && withoutLeader[idx]->sliceState > 0; idx++) {
      g.count = w_add(g.count, 1);
      g.last = withoutLeader[idx];
      remS = w_sub(remS, withoutLeader[idx]->sliceState);
    }
    if (remS > 0) return Greedy{};
    g.fit = true;
    return g;
  }
  // Go's math.Log / math.Log2 (src/math/log.go, log10.go: FreeBSD e_log.c),
  // so entropies and their comparisons round as in the reference.
  static double go_log(double x) {
    const double Ln2Hi = 6.93147180369123816490e-01, Ln2Lo = 1.90821492927058770002e-10;
    const double L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01, L3 = 2.857142874366239149e-01,
                 L4 = 2.222219843214978396e-01, L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
                 L7 = 1.479819860511658591e-01;
    if (std::isnan(x) || std::isinf(x)) return x;
    if (x < 0) return std::nan("");
    if (x == 0) return -std::numeric_limits<double>::infinity();
    int ki;
    double f1 = std::frexp(x, &ki);
    if (f1 < M_SQRT2 / 2) {
      f1 *= 2;
      ki--;
    }
    const double f = f1 - 1, k = double(ki);
    const double s = f / (2 + f), s2 = s * s, s4 = s2 * s2;
    const double t1 = s2 * (L1 + s4 * (L3 + s4 * (L5 + s4 * L7)));
    const double t2 = s4 * (L2 + s4 * (L4 + s4 * L6));
    const double R = t1 + t2, hfsq = 0.5 * f * f;
    return k * Ln2Hi - ((hfsq - (s * (hfsq + R) + k * Ln2Lo)) - f);
  }
  static double go_log2(double x) {
    int e;
    const double frac = std::frexp(x, &e);
    if (frac == 0.5) return double(e - 1);  // exact powers of two
    return go_log(frac) * (1 / 0.693147180559945309417232121458176568) + double(e);
  }
  static double entropy(const Domain* d) {  // calculateEntropy (:186-209) of the children's states
    if (d->children.empty()) return 0.0;
    int32_t total = 0;
    for (Domain* c : d->children) total = w_add(total, c->state);
    if (total == 0) return 0.0;
    double e = 0, tf = double(total);
    for (Domain* c : d->children)
      if (c->state > 0) {
        const double p = double(c->state) / tf;
        e += -p * go_log2(p);
      }
    return e;
  }
  static void sort_by_capacity_and_entropy(std::vector<Domain*>& ds) {  // :211-231
    auto cmp = [](Domain* a, Domain* b) -> int {  // Go's int(b - a) on int32 fields
      if (int32_t r = w_sub(b->leaderState, a->leaderState)) return r;
      if (int32_t r = w_sub(b->sliceStateWithLeader, a->sliceStateWithLeader)) return r;
      const double ea = entropy(a), eb = entropy(b);
      return eb > ea ? 1 : (eb < ea ? -1 : 0);
    };
    for (size_t i = 1; i < ds.size(); i++)  // stable insertion sort
      for (size_t j = i; j > 0 && cmp(ds[j - 1], ds[j]) > 0; j--) std::swap(ds[j - 1], ds[j]);
  }
  // selectOptimalDomainSetToFit (:81-147); nullopt = Go's nil
  std::optional<std::vector<Domain*>> select_optimal_domain_set(std::vector<Domain*>& ds, int32_t sliceCount,
                                                                int32_t leaderCount, int32_t sliceSize, bool byEntropy) {
    const Greedy g = evaluate_greedy(ds, sliceCount, leaderCount);
    if (!g.fit) return std::nullopt;
    if (byEntropy) sort_by_capacity_and_entropy(ds);
    const int32_t opt = g.count;
    // placements[i][leadersLeft][stateLeft]: the first domain list found using i domains
    std::vector<std::map<int32_t, std::map<int32_t, std::vector<Domain*>>>> pl(size_t(std::max(opt, 0)) + 1);
    pl[0][leaderCount][w_mul(sliceCount, sliceSize)] = {};
    for (Domain* d : ds)
      for (int32_t i = opt; i > 0; i--)
        for (auto& lk : pl[size_t(i - 1)])
          for (auto& sk : lk.second) {
            const int32_t beforeLeader = lk.first, beforeState = sk.first;
            if (beforeLeader <= 0 && beforeState <= 0) continue;
            std::vector<Domain*> np = sk.second;
            np.push_back(d);
            if (beforeLeader > 0 && d->leaderState > 0)  // with the leader
              pl[size_t(i)][w_sub(beforeLeader, d->leaderState)].emplace(w_sub(beforeState, d->stateWithLeader), np);
            if (d->sliceState > 0)  // without
              pl[size_t(i)][beforeLeader].emplace(w_sub(beforeState, d->state), np);
          }
    auto it = pl[size_t(std::max(opt, 0))].find(0);
    if (it == pl[size_t(std::max(opt, 0))].end()) return std::nullopt;
    int32_t bestSlice = INT32_MIN;
    const std::vector<Domain*>* best = nullptr;
    for (auto& kv : it->second)
      if (kv.first > bestSlice && kv.first <= 0) {
        bestSlice = kv.first;
        best = &kv.second;
      }
    if (!best) return std::nullopt;
    return *best;
  }
  std::string place_slices_balanced(std::vector<Domain*> ds, int32_t sliceCount, int32_t leaderCount, int32_t sliceSize,
                                    int32_t threshold, std::vector<Domain*>* out) {  // :149-184
    auto res = select_optimal_domain_set(ds, sliceCount, leaderCount, sliceSize, false);
    if (!res) return "TAS Balanced Placement: Cannot find optimal domain set to fit the request";
    if (sliceCount < w_mul(int32_t(res->size()), threshold)) return "TAS Balanced Placement: Not enough slices to meet the threshold";
    std::vector<Domain*> rd = sorted_domains_with_leader(*res, false);
    int32_t extra = w_sub(sliceCount, w_mul(int32_t(rd.size()), threshold));
    int32_t leadersLeft = leaderCount, take = 0;
    for (Domain* d : rd) {
      if (leadersLeft > 0) {
        take = std::min(w_sub(d->sliceStateWithLeader, threshold), extra);
        d->leaderState = 1;
        leadersLeft = w_sub(leadersLeft, 1);
      } else if (extra > 0) {
        take = std::min(w_sub(d->sliceState, threshold), extra);
        d->leaderState = 0;
      } else {
        d->leaderState = 0;
        take = 0;
      }
      d->state = w_mul(w_add(threshold, take), sliceSize);
      d->sliceState = w_add(threshold, take);
      d->sliceStateWithLeader = d->sliceState;
      d->stateWithLeader = w_sub(d->state, d->leaderState);
      extra = w_sub(extra, take);
    }
    if (extra > 0 || leadersLeft > 0) return "TAS Balanced Placement: Not all slices or leaders could be placed";
    *out = rd;
    return "";
  }
  // findBestDomainsForBalancedPlacement (:236-290); returns the threshold, or
  // sets *panic when Go divides by zero (balanceThresholdValue :67 with no
  // domain selected: sliceCount <= 0)
  int32_t find_best_domains_balanced(const Params& st, std::vector<Domain*>* best, bool* panic) {
    const int32_t sliceCount = go_div32(st.count, st.sliceSize);
    std::vector<std::vector<Domain*>> groups;
    if (st.requestedLevelIdx == 0) {
      groups.push_back(level_domains_lex(domainsPerLevel[0]));
    } else {
      for (Domain* h : level_domains_lex(domainsPerLevel[size_t(st.requestedLevelIdx - 1)]))
        groups.push_back(lex_sorted(h->children));
    }
    int32_t bestThreshold = 0, bestCount = 0;
    const bool leaderReq = st.leaderCount > 0;
    for (auto& sib : groups) {
      std::vector<Domain*> cand = clone_domains(sib);
      const std::vector<Domain*> lower = st.requestedLevelIdx < st.sliceLevelIdx ? lower_level_domains(cand) : cand;
      const Greedy g = evaluate_greedy(lower, sliceCount, st.leaderCount);
      if (!g.fit) continue;
      if (g.count == 0) {
        *panic = true;
        return 0;
      }
      int32_t threshold = go_div32(sliceCount, g.count);  // balanceThresholdValue (:66-75)
      if (g.lastWithLeader) threshold = std::min(threshold, g.lastWithLeader->sliceStateWithLeader);
      if (g.last) threshold = std::min(threshold, g.last->sliceState);
      int32_t thrWL = threshold;
      if (st.leaderCount > 0 && g.last) thrWL = std::min(threshold, g.last->sliceStateWithLeader);
      if (threshold < bestThreshold) continue;
      prune_domains(cand, threshold, st.sliceSize, st.sliceLevelIdx, st.requestedLevelIdx, leaderReq);
      Greedy g2 = evaluate_greedy(cand, sliceCount, st.leaderCount);
      if (!g2.fit && thrWL < threshold) {  // retry with a threshold that reserves leader capacity
        if (thrWL <= 0 || thrWL < bestThreshold) continue;
        threshold = thrWL;
        cand = clone_domains(sib);
        prune_domains(cand, threshold, st.sliceSize, st.sliceLevelIdx, st.requestedLevelIdx, leaderReq);
        g2 = evaluate_greedy(cand, sliceCount, st.leaderCount);
      }
      if (!g2.fit) continue;
      if (threshold > bestThreshold || (threshold == bestThreshold && g2.count < bestCount)) {
        bestThreshold = threshold;
        bestCount = g2.count;
        *best = cand;
      }
    }
    return bestThreshold;
  }
  // applyBalancedPlacementAlgorithm (:295-314)
  std::string apply_balanced(const Params& st, int32_t bestThreshold, std::vector<Domain*> cur, std::vector<Domain*>* out,
                             int* fitLevelIdx) {
    const int32_t sliceCount = go_div32(st.count, st.sliceSize);
    if (st.requestedLevelIdx < st.sliceLevelIdx) {
      auto res = select_optimal_domain_set(cur, sliceCount, st.leaderCount, st.sliceSize, true);
      if (!res) return "TAS Balanced Placement: Cannot find optimal domain set to fit the request";
      cur = lower_level_domains(*res);
      *fitLevelIdx = st.requestedLevelIdx + 1;
    } else {
      *fitLevelIdx = st.requestedLevelIdx;
    }
    return place_slices_balanced(cur, sliceCount, st.leaderCount, st.sliceSize, bestThreshold, out);
  }

  // Phase-1 counters as kueue_tas_last_counters lays them out: out[f * S + g],
  // f = state, sliceState, stateWithLeader, sliceStateWithLeader, leaderState,
  // g over the levels from the top, each level in levels_in_order()'s order.
  std::vector<int32_t>* phase1Counters = nullptr;
  std::string phase1Params;  // the prelude's slice parameters of that request (JSON)
  static constexpr const char* kPhase1Stop = "<phase 1 only>";
  std::vector<std::vector<Domain*>> levels_in_order() const {  // lexicographic levelValues (slices.Compare)
    std::vector<std::vector<Domain*>> out;
    for (auto& lvl : domainsPerLevel) {
      std::vector<Domain*> v;
      for (auto& kv : lvl) v.push_back(kv.second);
      std::sort(v.begin(), v.end(), [](Domain* a, Domain* b) { return compare_values(a->levelValues, b->levelValues) < 0; });
      out.push_back(std::move(v));
    }
    return out;
  }
  void dump_counters(std::vector<int32_t>& out) const {
    const auto lv = levels_in_order();
    for (int f = 0; f < 5; f++)
      for (auto& v : lv)
        for (Domain* d : v)
          out.push_back(f == 0 ? d->state : f == 1 ? d->sliceState : f == 2 ? d->stateWithLeader
                        : f == 3 ? d->sliceStateWithLeader : d->leaderState);
  }

  // findTopologyAssignment (:804-999)
  std::string find_topology_assignment(const PodSetRequest& workers, const PodSetRequest* leader,
                                       std::map<std::string, Requests>& assumed, bool simulateEmpty,
                                       std::map<std::string, TopologyAssignment>* assignments,
                                       const std::string& requiredReplacementDomain = "") {
    Requirements rq;
    rq.assumedUsage = &assumed;
    rq.simulateEmpty = simulateEmpty;
    rq.requiredReplacementDomain = requiredReplacementDomain;
    Params st;
    st.count = workers.count;
    rq.requests = workers.singlePodRequests;
    req_add(rq.requests, Requests{{"pods", 1}});
    if (leader) {
      Requests lr = leader->singlePodRequests;
      req_add(lr, Requests{{"pods", 1}});
      rq.leaderRequests = lr;
      st.leaderCount = 1;
    }
    auto ss = slice_size_with_single_pod_default(workers.topologyRequest);
    if (!ss.second.empty()) return ss.second;
    st.sliceSize = ss.first;
    st.required = workers.topologyRequest && workers.topologyRequest->required.has_value();
    st.unconstrained = (workers.topologyRequest && workers.topologyRequest->unconstrained.value_or(false)) ||
                       workers.implied || is_slice_topology_only(workers.topologyRequest);
    auto key = level_key_with_implied_fallback(workers);
    if (!key) return "topology level not specified";
    int req = resolve_level_idx(*key);
    if (req < 0) return "no requested topology level: " + *key;
    st.requestedLevelIdx = req;
    std::string sliceKey = slice_level_key_with_default(workers.topologyRequest, lowest_level());
    int sl = resolve_level_idx(sliceKey);
    if (sl < 0) return "no requested topology level for slices: " + sliceKey;
    st.sliceLevelIdx = sl;
    if (st.requestedLevelIdx > st.sliceLevelIdx)
      return "podset slice topology " + sliceKey + " is above the podset topology " + *key;
    std::string r = build_slice_size_at_level(workers, st.sliceSize, st.sliceLevelIdx, st.sliceSizeAtLevel);
    if (!r.empty()) return r;
    if (gates.multiLayer && !st.sliceSizeAtLevel.empty()) st.multiLayerConstraints = workers.topologyRequest->constraints;
    rq.tolerations = workers.tolerations;
    rq.tolerations.insert(rq.tolerations.end(), tolerations.begin(), tolerations.end());
    if (isLowestLevelNode && workers.nodeSelector) {  // :879-887
      std::string e = k8s::validated_selector_from_set(*workers.nodeSelector);
      if (!e.empty()) return "invalid node selectors: " + k8s::go_map_string(*workers.nodeSelector) + ", reason: " + e;
      rq.selector = *workers.nodeSelector;
    }
    if (workers.requiredAffinity) {  // :889-897
      k8s::ParsedNodeSelector ns;
      std::string e = k8s::new_node_selector(*workers.requiredAffinity, &ns);
      if (!e.empty())
        return "invalid affinity node selectors: " + k8s::node_selector_string(*workers.requiredAffinity) + ", reason: " + e;
      rq.affinitySelector = std::move(ns);
    }

    fill_in_counts(rq, st);
    if (phase1Counters) {  // tas_oracle_counters: stop before phase 2 rewrites the counters in place
      if (phase1Counters->empty()) {
        dump_counters(*phase1Counters);
        phase1Params = "{\"sliceSize\":" + std::to_string(st.sliceSize) + ",\"sliceLevelIdx\":" +
                       std::to_string(st.sliceLevelIdx) + ",\"leader\":" + (st.leaderCount > 0 ? "true" : "false") +
                       ",\"sliceSizeAtLevel\":{";
        bool first = true;
        for (auto& kv : st.sliceSizeAtLevel) {
          phase1Params += std::string(first ? "" : ",") + "\"" + std::to_string(kv.first) + "\":" + std::to_string(kv.second);
          first = false;
        }
        phase1Params += "}}";
      }
      return kPhase1Stop;
    }

    int fitLevelIdx = 0;
    std::vector<Domain*> cur;
    bool useBalanced = false;  // :906-917
    clones.clear();
    if (gates.balanced && !st.required && !st.unconstrained) {
      bool panic = false;
      std::vector<Domain*> best;
      const int32_t thr = find_best_domains_balanced(st, &best, &panic);
      if (panic) return "panic: runtime error: integer divide by zero";
      useBalanced = thr > 0;
      if (useBalanced) {
        r = apply_balanced(st, thr, best, &cur, &fitLevelIdx);
        if (!r.empty()) return r;
      }
    }
    if (!useBalanced) {
      r = find_level_with_fit_domains(st.requestedLevelIdx, st, &fitLevelIdx, &cur);
      if (!r.empty()) return r;
    }
    std::vector<Domain*> next;
    if (!update_counts_to_minimum(cur, st.count, st.leaderCount, st.sliceSize, st.unconstrained, true, &next)) next.clear();
    cur = next;
    int level = fitLevelIdx;
    int L = int(domainsPerLevel.size());
    for (; level < std::min(L - 1, st.sliceLevelIdx) && !useBalanced; level++) {
      auto lower = sorted_domains(lower_level_domains(cur), st.unconstrained);
      if (!update_counts_to_minimum(lower, st.count, st.leaderCount, st.sliceSize, st.unconstrained, true, &next)) next.clear();
      cur = next;
    }
    for (; level < L - 1; level++) {
      int32_t sliceOnLevel = st.sliceSize;
      if (level >= st.sliceLevelIdx) {
        sliceOnLevel = 1;
        auto it = st.sliceSizeAtLevel.find(level + 1);
        if (it != st.sliceSizeAtLevel.end()) sliceOnLevel = it->second;
      }
      std::vector<Domain*> newCur;
      for (Domain* d : cur) {
        auto lower = sorted_domains(d->children, st.unconstrained);
        if (sliceOnLevel > 1)
          for (Domain* c : lower) {
            c->sliceState = go_div32(c->state, sliceOnLevel);
            c->sliceStateWithLeader = go_div32(c->stateWithLeader, sliceOnLevel);
          }
        std::vector<Domain*> add;
        if (!update_counts_to_minimum(lower, d->state, d->leaderState, sliceOnLevel, st.unconstrained, sliceOnLevel > 1, &add))
          add.clear();
        newCur.insert(newCur.end(), add.begin(), add.end());
      }
      cur = newCur;
    }
    if (leader) {
      std::vector<Domain*> leaderFit, workerFit;
      std::deque<Domain> copies;  // `copiedDomain := *domain` (:981-983)
      for (Domain* d : cur) {
        if (d->leaderState > 0) {
          copies.push_back(*d);
          copies.back().state = copies.back().leaderState;
          leaderFit.push_back(&copies.back());
        }
        if (d->state > 0) workerFit.push_back(d);
      }
      (*assignments)[leader->name] = build_assignment(leaderFit);
      cur = workerFit;
    }
    (*assignments)[workers.name] = build_assignment(cur);
    return "";
  }

  // FindTopologyAssignmentsForFlavor (:519-594) — normal (non-replacement,
  // non-elastic) branch.
  // ---- node replacement (:614-678, :680-727, :733-792, :1796-1826) ----
  // IsTopologyAssignmentStale (:736-743)
  std::pair<bool, std::string> is_topology_assignment_stale(const TopologyAssignment& ta) const {
    for (auto& d : ta.domains)
      if (!domains.count(domain_id(d.values))) return {true, d.values.empty() ? "" : d.values[0]};
    return {false, ""};
  }
  // deleteDomain (:746-758): drops the unhealthy node's domains, returns the
  // pods they held (the last match's count)
  static int32_t delete_domain(TopologyAssignment& ta, const std::string& node) {
    int32_t affected = 0;
    std::vector<DomainAssignment> kept;
    for (auto& d : ta.domains) {
      if (!d.values.empty() && d.values.back() == node) affected = d.count;
      else kept.push_back(d);
    }
    ta.domains = kept;
    return affected;
  }
  static bool slices_requested(const std::optional<TopologyRequest>& tr) {  // :1155-1160
    if (!tr) return false;
    return (tr->sliceRequiredTopology && tr->sliceSize) || !tr->constraints.empty();
  }
  // findIncompleteSliceDomain (:760-792).  Go ranges over a map: with more
  // than one qualifying domain its choice is random; here (and in the
  // library) the first qualifying domain in assignment order is taken.
  std::string find_incomplete_slice_domain(const TopologyAssignment& ta, int32_t missing, int32_t sliceSize,
                                           const std::string& topologyKey) const {
    const int sliceLevel = resolve_level_idx(topologyKey);
    if (sliceLevel < 0) return "";
    const int nodeLevel = int(levelKeys.size()) - 1;
    std::vector<std::string> order;
    std::map<std::string, int32_t> usage;
    for (auto& d : ta.domains) {
      auto it = domainsPerLevel[size_t(nodeLevel)].find(domain_id(d.values));
      if (it == domainsPerLevel[size_t(nodeLevel)].end()) continue;
      Domain* dom = it->second;
      for (int i = nodeLevel; i > sliceLevel; i--) dom = dom->parent;
      if (!usage.count(dom->id)) order.push_back(dom->id);
      usage[dom->id] = w_add(usage[dom->id], d.count);
    }
    if (sliceSize == 0) throw GoPanic("runtime error: integer divide by zero");
    for (auto& id : order)
      if (go_mod32(w_add(usage[id], missing), sliceSize) == 0) return id;
    return "";
  }
  static int32_t go_mod32(int32_t a, int32_t b) {
    if (b == 0) throw GoPanic("runtime error: integer divide by zero");
    if (b == -1) return 0;
    return a % b;
  }
  // requiredReplacementDomain (:680-731)
  std::string required_replacement_domain(const PodSetRequest& tr, const TopologyAssignment& ta) const {
    auto key = level_key_with_implied_fallback(tr);
    if (!key) return "";
    const int levelIdx = resolve_level_idx(*key);
    if (levelIdx < 0) return "";
    if (ta.domains.empty()) return "";
    const int32_t sliceSize = slice_size_with_single_pod_default(tr.topologyRequest).first;
    if (slices_requested(tr.topologyRequest) && go_mod32(tr.count, sliceSize) != 0) {
      const auto& cs = tr.topologyRequest->constraints;
      if (cs.size() > 1)
        for (size_t i = cs.size(); i-- > 0;)
          if (go_mod32(tr.count, cs[i].size) != 0) return find_incomplete_slice_domain(ta, tr.count, cs[i].size, cs[i].topology);
      return find_incomplete_slice_domain(ta, tr.count, sliceSize, slice_level_key_with_default(tr.topologyRequest, lowest_level()));
    }
    if (!(tr.topologyRequest && tr.topologyRequest->required)) return "";
    const int nodeLevel = int(levelKeys.size()) - 1;
    const auto& vals = ta.domains[0].values;
    if (vals.empty()) return "";
    auto it = domainsPerLevel[size_t(nodeLevel)].find(domain_id(vals));
    if (it == domainsPerLevel[size_t(nodeLevel)].end()) return "";
    Domain* dom = it->second;
    for (int i = nodeLevel; i > levelIdx; i--) dom = dom->parent;
    return dom->id;
  }
  // mergeTopologyAssignments (:1796-1826): sorted by DomainID of the leaves'
  // levelValues, adjacent equal DomainIDs merged
  TopologyAssignment merge_topology_assignments(const TopologyAssignment& a, const TopologyAssignment& b) const {
    const int nodeLevel = int(levelKeys.size()) - 1;
    std::vector<std::pair<std::string, const DomainAssignment*>> keyed;
    for (auto* ta : {&a, &b})
      for (auto& d : ta->domains) {
        auto it = domainsPerLevel[size_t(nodeLevel)].find(domain_id(d.values));
        if (it == domainsPerLevel[size_t(nodeLevel)].end())
          throw GoPanic("runtime error: invalid memory address or nil pointer dereference");
        keyed.push_back({domain_id(it->second->levelValues), &d});
      }
    std::stable_sort(keyed.begin(), keyed.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    TopologyAssignment out;
    out.levels = a.levels;
    for (auto& kd : keyed) {
      if (!out.domains.empty() && domain_id(out.domains.back().values) == domain_id(kd.second->values))
        out.domains.back().count = w_add(out.domains.back().count, kd.second->count);
      else
        out.domains.push_back(*kd.second);
    }
    return out;
  }
  // findReplacementAssignment (:614-656): (new assignment, replacement, reason)
  std::string find_replacement_assignment(PodSetRequest tr, TopologyAssignment existing, const std::string& node,
                                          std::map<std::string, Requests>& assumed, TopologyAssignment* merged,
                                          TopologyAssignment* replacement) {
    tr.count = delete_domain(existing, node);
    auto stale = is_topology_assignment_stale(existing);
    if (stale.first)
      return "Cannot replace the node, because the existing topologyAssignment is invalid, as it contains the stale domain " +
             stale.second;
    const std::string reqDomain = required_replacement_domain(tr, existing);
    PodSetRequest trCopy = tr;
    const int32_t sliceSize = slice_size_with_single_pod_default(tr.topologyRequest).first;
    if (slices_requested(tr.topologyRequest) && !reqDomain.empty() && go_mod32(tr.count, sliceSize) != 0) {
      // the innermost constraint whose size divides the replacement pods
      int32_t effSize = 1;
      std::optional<std::string> effTopo;
      const auto& cs = tr.topologyRequest->constraints;
      for (size_t i = cs.size(); i-- > 0;)
        if (go_mod32(tr.count, cs[i].size) == 0) {
          effSize = cs[i].size;
          effTopo = cs[i].topology;
          break;
        }
      trCopy.topologyRequest->constraints.clear();
      trCopy.topologyRequest->sliceRequiredTopology = effTopo;
      trCopy.topologyRequest->sliceSize = effSize;
    }
    std::map<std::string, TopologyAssignment> as;
    std::string reason = find_topology_assignment(trCopy, nullptr, assumed, false, &as, reqDomain);
    if (!reason.empty()) return reason;
    auto it = as.find(tr.name);
    if (it == as.end() || it->second.domains.empty())
      return "cannot find replacement assignment for unhealthy node: " + node;
    *replacement = it->second;
    *merged = merge_topology_assignments(it->second, existing);
    return "";
  }

  // ---- elastic workload slices (tas_elastic_workloads.go:35-127) ----
  struct ElasticResult {
    bool applied = false;
    std::vector<PodSetResult> assignments;  // in the order the reference sets them
  };
  static int32_t count_pods(const TopologyAssignment& ta) {  // utiltas.CountPodsInAssignment
    int32_t t = 0;
    for (auto& d : ta.domains) t = w_add(t, d.count);
    return t;
  }
  static TopologyAssignment truncate_assignment(const TopologyAssignment& ta, int32_t n) {  // TruncateAssignment
    TopologyAssignment out;
    out.levels = ta.levels;
    if (n <= 0) return out;
    int32_t remaining = n;
    for (auto& d : ta.domains) {
      if (remaining <= 0) break;
      if (d.count <= remaining) {
        out.domains.push_back(d);
        remaining -= d.count;
      } else {
        out.domains.push_back({d.values, remaining});
        remaining = 0;
      }
    }
    return out;
  }
  static void add_assumed(std::map<std::string, Requests>& assumed, const TopologyAssignment& ta, const PodSetRequest& tr) {
    for (auto& d : ta.domains) req_add(assumed[domain_id(d.values)], req_scaled_up(tr.singlePodRequests, d.count));
  }
  // handleElasticWorkload (:35-69), handleScaleUp (:72-112), handleScaleDown (:115-127)
  ElasticResult handle_elastic(const PodSetRequest& workers, const PodSetRequest* leader,
                               const TopologyAssignment* previous, std::map<std::string, Requests>& assumed,
                               bool simulateEmpty) {
    ElasticResult r;
    if (!previous) return r;
    const TopologyAssignment& prev = *previous;
    if (is_topology_assignment_stale(prev).first) return r;  // fresh placement
    r.applied = true;
    const int32_t prevCount = count_pods(prev);
    if (workers.count > prevCount) {
      PodSetRequest delta = workers;
      delta.count = w_sub(workers.count, prevCount);
      // ComputeUsagePerDomain (util/tas/tas_assignment.go:305-314): single x count + pods:count, per domain (last wins)
      std::map<std::string, Requests> prevUsage;
      for (auto& d : prev.domains) {
        Requests u = req_scaled_up(workers.singlePodRequests, d.count);
        req_add(u, Requests{{"pods", int64_t(d.count)}});
        prevUsage[domain_id(d.values)] = u;
      }
      for (auto& kv : prevUsage) req_add(assumed[kv.first], kv.second);
      std::map<std::string, TopologyAssignment> as;
      std::string reason;
      try {
        reason = find_topology_assignment(delta, leader, assumed, simulateEmpty, &as);
      } catch (const GoPanic& e) {
        reason = std::string("panic: ") + e.what();
      }
      if (!reason.empty()) {
        r.assignments.push_back({workers.name, std::nullopt, reason});
        return r;
      }
      TopologyAssignment merged;
      try {
        merged = merge_topology_assignments(as[workers.name], prev);
      } catch (const GoPanic& e) {
        r.assignments.push_back({workers.name, std::nullopt, std::string("panic: ") + e.what()});
        return r;
      }
      r.assignments.push_back({workers.name, merged, ""});
      if (leader) {
        r.assignments.push_back({leader->name, as[leader->name], ""});
        add_assumed(assumed, as[leader->name], *leader);
      }
      add_assumed(assumed, as[workers.name], workers);
    } else if (workers.count < prevCount) {
      TopologyAssignment t = truncate_assignment(prev, workers.count);
      r.assignments.push_back({workers.name, t, ""});
      add_assumed(assumed, t, workers);
    } else {
      r.assignments.push_back({workers.name, prev, ""});
      add_assumed(assumed, prev, workers);
    }
    return r;
  }

  std::vector<PodSetResult> find_topology_assignments_for_flavor(const std::vector<PodSetRequest>& reqs, bool simulateEmpty,
                                                                 const WorkloadInfo* wl = nullptr,
                                                                 const PreviousAssignments* prevs = nullptr) {
    std::vector<PodSetResult> result;
    std::map<std::string, Requests> assumed;
    std::vector<std::string> order;
    std::map<std::string, std::vector<const PodSetRequest*>> grouped;
    for (size_t idx = 0; idx < reqs.size(); idx++) {
      std::string key = reqs[idx].podSetGroupName ? *reqs[idx].podSetGroupName : std::to_string(idx);
      if (std::find(order.begin(), order.end(), key) == order.end()) order.push_back(key);
      grouped[key].push_back(&reqs[idx]);
    }
    auto set_result = [&](const std::string& name, std::optional<TopologyAssignment> a, const std::string& reason) {
      for (auto& r : result)
        if (r.name == name) { r.assignment = std::move(a); r.reason = reason; return; }
      result.push_back({name, std::move(a), reason});
    };
    for (auto& key : order) {
      auto& trs = grouped[key];
      if (wl && !wl->unhealthyNodes.empty()) {  // HasUnhealthyNodes: node replacement (:546-562)
        for (auto* tr : trs) {
          auto p = wl->psa.find(tr->name);
          if (p == wl->psa.end() || !p->second) continue;
          TopologyAssignment merged, replacement;
          std::string reason;
          try {
            reason = find_replacement_assignment(*tr, *p->second, wl->unhealthyNodes[0], assumed, &merged, &replacement);
          } catch (const GoPanic& e) {
            reason = std::string("panic: ") + e.what();
          }
          if (!reason.empty()) {
            set_result(tr->name, std::nullopt, reason);
            return result;
          }
          set_result(tr->name, merged, "");
          for (auto& d : replacement.domains) {  // addAssumedUsage (:658-666)
            Requests& a = assumed[domain_id(d.values)];
            req_add(a, req_scaled_up(tr->singlePodRequests, d.count));
          }
        }
        continue;
      }
      // findLeaderAndWorkers (:596-609)
      const PodSetRequest* leader = nullptr;
      const PodSetRequest* workers = trs[0];
      if (trs.size() > 1) {
        leader = trs[1];
        if (leader->count > workers->count) { leader = trs[0]; workers = trs[1]; }
      }
      if (gates.elastic) {  // delta-only placement (:567-576)
        const TopologyAssignment* prev = nullptr;
        if (prevs) {
          auto it = prevs->byName.find(workers->name);
          if (it != prevs->byName.end()) prev = &it->second;
        }
        ElasticResult er = handle_elastic(*workers, leader, prev, assumed, simulateEmpty);
        if (er.applied) {
          std::string wreason;
          for (auto& a : er.assignments) {
            set_result(a.name, a.assignment, a.reason);
            if (a.name == workers->name) wreason = a.reason;
          }
          if (!wreason.empty()) return result;
          continue;
        }
      }
      std::map<std::string, TopologyAssignment> assignments;
      std::string reason;
      try {
        reason = find_topology_assignment(*workers, leader, assumed, simulateEmpty, &assignments);
      } catch (const GoPanic& e) {
        reason = std::string("panic: ") + e.what();
      }
      for (auto* tr : trs) {
        auto it = assignments.find(tr->name);
        if (it == assignments.end()) set_result(tr->name, std::nullopt, reason);
        else set_result(tr->name, it->second, reason);
      }
      if (!reason.empty()) return result;
      for (auto* tr : trs) {  // addAssumedUsage (:658-666)
        auto it = assignments.find(tr->name);
        if (it == assignments.end()) continue;
        for (auto& d : it->second.domains) {
          Requests& a = assumed[domain_id(d.values)];
          req_add(a, req_scaled_up(tr->singlePodRequests, d.count));
        }
      }
    }
    return result;
  }
};

// ---- JSON plumbing -------------------------------------------------------------
static Requests parse_requests(const ojson::Value& v) {
  Requests r;
  if (v.kind == ojson::Value::Obj)
    for (auto& kv : v.o) r[kv.first] = kv.second.as_int();
  return r;
}
static std::vector<Toleration> parse_tolerations(const ojson::Value& v) {
  std::vector<Toleration> out;
  for (auto& t : v.a) out.push_back({t.at("key").as_str(), t.at("operator").as_str(), t.at("value").as_str(), t.at("effect").as_str()});
  return out;
}
static Gates parse_gates(const ojson::Value& v) {
  Gates g;
  if (auto p = v.get("TASProfileMixed")) g.profileMixed = p->as_bool();
  if (auto p = v.get("TASMultiLayerTopology")) g.multiLayer = p->as_bool();
  if (auto p = v.get("TASBalancedPlacement")) g.balanced = p->as_bool();
  if (auto p = v.get("ElasticJobsViaWorkloadSlicesWithTAS")) g.elastic = p->as_bool();
  return g;
}

// PodSpec.Affinity.NodeAffinity.RequiredDuringSchedulingIgnoredDuringExecution
// (k8s JSON shape); absent / null at any step -> no required affinity.
static std::optional<k8s::NodeSelector> parse_required_affinity(const ojson::Value& aff) {
  if (aff.kind != ojson::Value::Obj) return std::nullopt;
  const ojson::Value* na = aff.get("nodeAffinity");
  if (!na || na->kind != ojson::Value::Obj) return std::nullopt;
  const ojson::Value* req = na->get("requiredDuringSchedulingIgnoredDuringExecution");
  if (!req || req->kind != ojson::Value::Obj) return std::nullopt;
  k8s::NodeSelector ns;
  auto reqs = [](const ojson::Value* arr) {
    std::vector<k8s::NodeSelectorRequirement> out;
    if (!arr || arr->kind != ojson::Value::Arr) return out;
    for (auto& r : arr->a) {
      k8s::NodeSelectorRequirement q;
      if (auto k = r.get("key")) q.key = k->as_str();
      if (auto o = r.get("operator")) q.op = o->as_str();
      if (auto v = r.get("values"); v && v->kind == ojson::Value::Arr) {
        q.values.emplace();
        for (auto& x : v->a) q.values->push_back(x.as_str());
      }
      out.push_back(std::move(q));
    }
    return out;
  };
  if (auto terms = req->get("nodeSelectorTerms"); terms && terms->kind == ojson::Value::Arr)
    for (auto& t : terms->a) ns.terms.push_back({reqs(t.get("matchExpressions")), reqs(t.get("matchFields"))});
  return ns;
}

static std::vector<PodSetRequest> parse_podsets(const ojson::Value& arr) {
  std::vector<PodSetRequest> out;
  for (auto& ps : arr.a) {
    PodSetRequest r;
    r.name = ps.at("name").as_str();
    const ojson::Value& tr = ps.at("topologyRequest");
    if (!tr.is_null()) {
      TopologyRequest t;
      if (!tr.at("required").is_null()) t.required = tr.at("required").as_str();
      if (!tr.at("preferred").is_null()) t.preferred = tr.at("preferred").as_str();
      if (!tr.at("unconstrained").is_null()) t.unconstrained = tr.at("unconstrained").as_bool();
      if (!tr.at("podSetSliceRequiredTopology").is_null()) t.sliceRequiredTopology = tr.at("podSetSliceRequiredTopology").as_str();
      if (!tr.at("podSetSliceSize").is_null()) t.sliceSize = int32_t(tr.at("podSetSliceSize").as_int());
      for (auto& c : tr.at("podsetSliceRequiredTopologyConstraints").a)
        t.constraints.push_back({c.at("topology").as_str(), int32_t(c.at("size").as_int())});
      r.topologyRequest = t;
    }
    r.implied = tr.is_null();  // harness: tas_cache_test.go:6322-6324
    if (auto im = ps.get("implied")) r.implied = im->as_bool();
    r.singlePodRequests = parse_requests(ps.at("requests"));
    r.count = int32_t(ps.at("count").as_int());
    if (!ps.at("podSetGroupName").is_null()) r.podSetGroupName = ps.at("podSetGroupName").as_str();
    r.tolerations = parse_tolerations(ps.at("tolerations"));
    const ojson::Value& ns = ps.at("nodeSelector");
    if (ns.kind == ojson::Value::Obj) {
      std::map<std::string, std::string> m;
      for (auto& kv : ns.o) m[kv.first] = kv.second.as_str();
      r.nodeSelector = m;
    }
    if (auto aff = ps.get("affinity")) r.requiredAffinity = parse_required_affinity(*aff);
    out.push_back(std::move(r));
  }
  return out;
}

static TopologyAssignment parse_assignment(const ojson::Value& v) {  // internal utiltas.TopologyAssignment
  TopologyAssignment ta;
  for (auto& l : v.at("levels").a) ta.levels.push_back(l.as_str());
  for (auto& d : v.at("domains").a) {
    DomainAssignment da;
    for (auto& x : d.at("values").a) da.values.push_back(x.as_str());
    da.count = int32_t(d.at("count").as_int());
    ta.domains.push_back(std::move(da));
  }
  return ta;
}
// {"unhealthyNodes": [...], "podSetAssignments": [{"name", "topologyAssignment": internal | null}]}
static WorkloadInfo parse_workload(const ojson::Value& w) {
  WorkloadInfo wl;
  if (auto u = w.get("unhealthyNodes"))
    for (auto& n : u->a) wl.unhealthyNodes.push_back(n.as_str());
  if (auto ps = w.get("podSetAssignments"))
    for (auto& p : ps->a) {
      const ojson::Value& ta = p.at("topologyAssignment");
      wl.psa[p.at("name").as_str()] = ta.is_null() ? std::nullopt : std::optional<TopologyAssignment>(parse_assignment(ta));
    }
  return wl;
}

// Build the snapshot exactly like the reference test harness
// (tas_cache_test.go:6270-6300): nodesCache.sync + find, nonTasUsageCache.update,
// TASFlavorCache.snapshot (tas_flavor.go:118-138).
static std::unique_ptr<Snapshot> build_snapshot(const ojson::Value& c) {
  std::vector<std::string> levels;
  for (auto& l : c.at("levels").a) levels.push_back(l.as_str());
  if (levels.empty()) throw std::runtime_error("no levels");
  auto snap = std::make_unique<Snapshot>(levels, parse_tolerations(c.at("flavorTolerations")));
  snap->gates = parse_gates(c.at("featureGates"));
  if (!c.at("topologyName").is_null()) snap->topologyName = c.at("topologyName").as_str();
  std::map<std::string, std::string> flavorLabels;
  for (auto& kv : c.at("nodeLabels").o) flavorLabels[kv.first] = kv.second.as_str();
  std::map<std::string, std::string> nodeToDomain;
  std::set<std::string> seenNames;
  std::vector<const ojson::Value*> kept;
  // nodesCache keyed by name: a later sync of the same name replaces the earlier one.
  std::map<std::string, const ojson::Value*> byName;
  std::vector<std::string> nameOrder;
  for (auto& n : c.at("nodes").a) {
    std::string name = n.at("name").as_str();
    bool ready = false;
    for (auto& cond : n.at("conditions").a)
      if (cond.at("type").as_str() == "Ready") { ready = cond.at("status").as_str() == "True"; break; }
    bool ok = !n.at("unschedulable").as_bool() && ready;  // tas_nodes_cache.go:38-50
    if (ok) {
      if (!byName.count(name)) nameOrder.push_back(name);
      byName[name] = &n;
    } else if (byName.count(name)) {
      byName.erase(name);
      nameOrder.erase(std::find(nameOrder.begin(), nameOrder.end(), name));
    }
  }
  for (auto& name : nameOrder) {
    const ojson::Value& n = *byName[name];
    std::map<std::string, std::string> labels;
    for (auto& kv : n.at("labels").o) labels[kv.first] = kv.second.as_str();
    bool match = true;  // NodeMatchesFlavor (util/tas/node.go:21-33)
    for (auto& kv : flavorLabels) {
      auto it = labels.find(kv.first);
      if ((it == labels.end() ? std::string() : it->second) != kv.second) { match = false; break; }
    }
    for (auto& l : levels)
      if (!labels.count(l)) { match = false; break; }
    if (!match) continue;
    snap->nodes.emplace_back();
    NodeInfo& ni = snap->nodes.back();
    ni.name = name;
    ni.labels = labels;
    for (auto& t : n.at("taints").a) ni.taints.push_back({t.at("key").as_str(), t.at("value").as_str(), t.at("effect").as_str()});
    ni.allocatable = parse_requests(n.at("allocatable"));
    nodeToDomain[name] = snap->add_node(&ni);
  }
  snap->initialize();
  // TAS usage (TASFlavorCache.updateUsage, tas_flavor.go:154-171)
  std::map<std::string, Requests> usage;
  for (auto& u : c.at("tasUsage").a) {
    std::vector<std::string> values;
    for (auto& v : u.at("values").a) values.push_back(v.as_str());
    int64_t cnt = u.at("count").as_int();
    Requests& dst = usage[domain_id(values)];
    req_add(dst, req_scaled_up(parse_requests(u.at("singlePodRequests")), cnt));
    req_add(dst, Requests{{"pods", cnt}});
  }
  for (auto& kv : usage) snap->add_tas_usage(kv.first, kv.second);
  // non-TAS pods (tas_non_tas_pod_cache.go:46-120)
  std::map<std::string, std::pair<std::string, Requests>> podUsage;
  std::map<std::string, Requests> nodeUsage;
  auto remove_node_usage = [&](const std::string& node, const Requests& u) {
    auto it = nodeUsage.find(node);
    if (it == nodeUsage.end()) return;
    req_sub(it->second, u);
    it->second["pods"] = w_sub64(it->second["pods"], 1);
    if (it->second["pods"] <= 0) nodeUsage.erase(it);
  };
  for (auto& p : c.at("pods").a) {
    std::string key = p.at("namespace").as_str() + "/" + p.at("name").as_str();
    std::string phase = p.at("phase").as_str();
    auto old = podUsage.find(key);
    if (phase == "Succeeded" || phase == "Failed") {
      if (old != podUsage.end()) remove_node_usage(old->second.first, old->second.second);
      podUsage.erase(key);
      continue;
    }
    if (old != podUsage.end()) remove_node_usage(old->second.first, old->second.second);
    Requests r = parse_requests(p.at("requests"));
    std::string node = p.at("nodeName").as_str();
    podUsage[key] = {node, r};
    Requests& nu = nodeUsage[node];
    req_add(nu, r);
    nu["pods"] = w_add64(nu["pods"], 1);
  }
  for (auto& kv : nodeUsage) {
    auto it = nodeToDomain.find(kv.first);
    if (it != nodeToDomain.end()) snap->add_non_tas_usage(it->second, kv.second);
  }
  return snap;
}

static void emit_results(std::string& out, const std::vector<PodSetResult>& rs) {
  out += "[";
  for (size_t i = 0; i < rs.size(); i++) {
    if (i) out += ",";
    out += "{\"name\":";
    ojson::quote(out, rs[i].name);
    out += ",\"assignment\":";
    if (!rs[i].assignment) {
      out += "null";
    } else {
      out += "{\"levels\":[";
      auto& a = *rs[i].assignment;
      for (size_t j = 0; j < a.levels.size(); j++) {
        if (j) out += ",";
        ojson::quote(out, a.levels[j]);
      }
      out += "],\"domains\":[";
      for (size_t j = 0; j < a.domains.size(); j++) {
        if (j) out += ",";
        out += "{\"values\":[";
        for (size_t k = 0; k < a.domains[j].values.size(); k++) {
          if (k) out += ",";
          ojson::quote(out, a.domains[j].values[k]);
        }
        out += "],\"count\":" + std::to_string(a.domains[j].count) + "}";
      }
      out += "]}";
    }
    out += ",\"reason\":";
    ojson::quote(out, rs[i].reason);
    out += "}";
  }
  out += "]";
}

// PodSetReducer.Search (pkg/scheduler/flavorassigner/podset_reducer.go:37-86)
// with the fits closure of Scheduler.getInitialAssignments (scheduler.go:
// 720-739) reduced to its TAS part: flvAssigner.Assign(nextCounts) scales every
// PodSet to its count (flavorassigner.go:599-609), WorkloadsTopologyRequests
// skips a count-0 PodSet (tas_flavorassigner.go:52-55) and the assignment
// fits when FindTopologyAssignmentsForWorkload has no failure
// (flavorassigner.go:734-747).  `tas[i]` false: a PodSet outside TAS (its
// counts take part in the index arithmetic only).  The probes are exactly
// sort.Search's (sort.go: h = int(uint(i+j) >> 1)).
struct ReducerResult {
  bool found = false;
  std::vector<int32_t> counts;
  std::vector<PodSetResult> results;
  int64_t probes = 0;
};
static ReducerResult podset_reducer_search(Snapshot& snap, const std::vector<PodSetRequest>& podsets,
                                           const std::vector<int32_t>& minCounts, const std::vector<bool>& tas,
                                           bool simulateEmpty) {
  ReducerResult out;
  const size_t n = podsets.size();
  std::vector<int32_t> full(n), deltas(n);
  int32_t totalDelta = 0;
  for (size_t i = 0; i < n; i++) {  // NewPodSetReducer (:37-53)
    full[i] = podsets[i].count;
    deltas[i] = podsets[i].count - minCounts[i];
    totalDelta += deltas[i];
  }
  if (totalDelta == 0) return out;  // (:71-73)
  auto fill = [&](int32_t up) {     // fillPodSetSizesForSearchIndex (:55-62)
    std::vector<int32_t> c(n);
    for (size_t i = 0; i < n; i++) c[i] = full[i] - int32_t(int64_t(deltas[i]) * int64_t(up) / int64_t(totalDelta));
    return c;
  };
  int lastGoodIdx = 0;
  std::vector<PodSetResult> lastR;
  // sort.Search(int(totalDelta)+1, f) (:76-84)
  int i = 0, j = int(totalDelta) + 1;
  while (i < j) {
    const int h = int(unsigned(i + j) >> 1);
    const std::vector<int32_t> cur = fill(int32_t(h));
    std::vector<PodSetRequest> reqs;
    for (size_t k = 0; k < n; k++)
      if (tas[k] && cur[k] != 0) {
        reqs.push_back(podsets[k]);
        reqs.back().count = cur[k];
      }
    out.probes++;
    std::vector<PodSetResult> rs = reqs.empty() ? std::vector<PodSetResult>{}
                                                : snap.find_topology_assignments_for_flavor(reqs, simulateEmpty);
    bool f = true;
    for (auto& r : rs) f = f && r.reason.empty();  // TASAssignmentsResult.Failure() (:384-391)
    if (f) {
      lastGoodIdx = h;
      lastR = std::move(rs);
    }
    if (!f) i = h + 1;
    else j = h;
  }
  out.found = i == lastGoodIdx;  // (:85)
  if (out.found) {
    out.counts = fill(int32_t(lastGoodIdx));
    out.results = std::move(lastR);
  }
  return out;
}

static char* dup_out(const std::string& s) {
  char* p = static_cast<char*>(malloc(s.size() + 1));
  memcpy(p, s.data(), s.size() + 1);
  return p;
}

}  // namespace oracle

extern "C" {

// Runs one fixture case (schema: tools/extract_goldens.py) and returns
// {"results":[{"name","assignment","reason"}...]} or {"error": "..."}.
int tas_oracle_run_case(const char* case_json, char** out_json) {
  using namespace oracle;
  std::string out;
  try {
    ojson::Value c = ojson::parse(case_json);
    auto snap = build_snapshot(c);
    auto reqs = parse_podsets(c.at("podSets"));
    std::optional<WorkloadInfo> wl;
    if (auto w = c.get("workload")) wl = parse_workload(*w);
    PreviousAssignments prevs;
    for (auto& ps : c.at("podSets").a)
      if (auto pa = ps.get("previousAssignment"))
        if (!pa->is_null()) prevs.byName[ps.at("name").as_str()] = parse_assignment(*pa);
    auto rs = snap->find_topology_assignments_for_flavor(reqs, c.at("simulateEmpty").as_bool(), wl ? &*wl : nullptr,
                                                         &prevs);
    out = "{\"results\":";
    emit_results(out, rs);
    out += "}";
  } catch (const std::exception& e) {
    out = "{\"error\":";
    ojson::quote(out, e.what());
    out += "}";
    *out_json = dup_out(out);
    return -1;
  }
  *out_json = dup_out(out);
  return 0;
}

// Batched evaluation for the CPU baseline: builds the snapshot once from
// `snapshot_json` (same schema, podSets ignored) and evaluates every workload
// of `workloads_json` ({"workloads": [[podset...], ...]}) independently against
// it, as Scheduler.nominate does (pkg/scheduler/scheduler.go:583-619).  Only
// the evaluation loop is timed (*seconds).  `threads` > 1 gives each thread its
// own snapshot copy (the Go snapshot's scratch counters are not reentrant).
int tas_oracle_eval_workloads(const char* snapshot_json, const char* workloads_json, int threads, int emit,
                              double* seconds, char** out_json) {
  using namespace oracle;
  try {
    ojson::Value c = ojson::parse(snapshot_json);
    ojson::Value w = ojson::parse(workloads_json);
    std::vector<std::vector<PodSetRequest>> wls;
    for (auto& wl : w.at("workloads").a) wls.push_back(parse_podsets(wl));
    if (threads < 1) threads = 1;
    std::vector<std::unique_ptr<Snapshot>> snaps;
    for (int t = 0; t < threads; t++) snaps.push_back(build_snapshot(c));
    std::vector<std::vector<PodSetResult>> results(wls.size());
    auto t0 = std::chrono::steady_clock::now();
    if (threads == 1) {
      for (size_t i = 0; i < wls.size(); i++) results[i] = snaps[0]->find_topology_assignments_for_flavor(wls[i], false);
    } else {
      std::vector<std::thread> pool;
      for (int t = 0; t < threads; t++)
        pool.emplace_back([&, t] {
          for (size_t i = t; i < wls.size(); i += threads)
            results[i] = snaps[t]->find_topology_assignments_for_flavor(wls[i], false);
        });
      for (auto& th : pool) th.join();
    }
    auto t1 = std::chrono::steady_clock::now();
    *seconds = std::chrono::duration<double>(t1 - t0).count();
    std::string out = "{\"results\":[";
    if (emit) {
      for (size_t i = 0; i < results.size(); i++) {
        if (i) out += ",";
        emit_results(out, results[i]);
      }
    }
    out += "]}";
    *out_json = dup_out(out);
    return 0;
  } catch (const std::exception& e) {
    std::string out = "{\"error\":";
    ojson::quote(out, e.what());
    out += "}";
    *out_json = dup_out(out);
    return -1;
  }
}

// A scheduling session on one snapshot (the scheduler's admission loop,
// pkg/scheduler/scheduler.go:426-435): `ops_json` = {"ops": [...]} with
//   {"op": "find", "podSets": [...], "simulateEmpty": bool} -> results list
//   {"op": "fits", "usage": [{values, singlePodRequests, count}...]} -> bool
//   {"op": "add" | "remove", "usage": [...]}                         -> null
//   {"op": "admit", "usage": [...]}: fits, then add when it fits     -> bool
//   {"op": "partialAdmission", "podSets": [... "minCount", "tas"], "simulateEmpty": bool}
//       -> {"found", "counts", "results", "probes"} (podset_reducer_search)
// applied in order; returns {"results": [one entry per op]}.
int tas_oracle_session(const char* snapshot_json, const char* ops_json, char** out_json) {
  using namespace oracle;
  std::string out = "{\"results\":[";
  try {
    ojson::Value c = ojson::parse(snapshot_json);
    ojson::Value o = ojson::parse(ops_json);
    auto snap = build_snapshot(c);
    auto parse_usage = [](const ojson::Value& arr) {
      std::vector<Snapshot::DomainUsage> us;
      for (auto& u : arr.a) {
        Snapshot::DomainUsage d;
        for (auto& v : u.at("values").a) d.values.push_back(v.as_str());
        d.single = parse_requests(u.at("singlePodRequests"));
        d.count = int32_t(u.at("count").as_int());
        us.push_back(std::move(d));
      }
      return us;
    };
    bool first = true;
    for (auto& op : o.at("ops").a) {
      if (!first) out += ",";
      first = false;
      const std::string kind = op.at("op").as_str();
      if (kind == "find") {
        auto sim = op.get("simulateEmpty");
        emit_results(out, snap->find_topology_assignments_for_flavor(parse_podsets(op.at("podSets")),
                                                                     sim && sim->as_bool()));
      } else if (kind == "fits") {
        out += snap->fits(parse_usage(op.at("usage"))) ? "true" : "false";
      } else if (kind == "admit") {  // processEntry's TAS half: Fits, then AddUsage (scheduler.go:426-435)
        auto us = parse_usage(op.at("usage"));
        const bool ok = snap->fits(us);
        if (ok) snap->update_usage(us, true);
        out += ok ? "true" : "false";
      } else if (kind == "add" || kind == "remove") {
        snap->update_usage(parse_usage(op.at("usage")), kind == "add");
        out += "null";
      } else if (kind == "partialAdmission") {  // PodSetReducer.Search over the TAS fit
        const ojson::Value& ps = op.at("podSets");
        auto reqs = parse_podsets(ps);
        std::vector<int32_t> minc;
        std::vector<bool> tas;
        for (auto& p : ps.a) {
          auto m = p.get("minCount");
          minc.push_back(m && !m->is_null() ? int32_t(m->as_int()) : int32_t(p.at("count").as_int()));
          auto t = p.get("tas");
          tas.push_back(!(t && !t->is_null() && !t->as_bool()));
        }
        auto sim = op.get("simulateEmpty");
        ReducerResult r = podset_reducer_search(*snap, reqs, minc, tas, sim && sim->as_bool());
        out += std::string("{\"found\":") + (r.found ? "true" : "false") + ",\"counts\":";
        if (!r.found) {
          out += "null,\"results\":null";
        } else {
          out += "[";
          for (size_t k = 0; k < r.counts.size(); k++) out += (k ? "," : "") + std::to_string(r.counts[k]);
          out += "],\"results\":";
          emit_results(out, r.results);
        }
        out += ",\"probes\":" + std::to_string(r.probes) + "}";
      } else {
        throw std::runtime_error("unknown op " + kind);
      }
    }
    out += "]}";
  } catch (const std::exception& e) {
    out = "{\"error\":";
    ojson::quote(out, e.what());
    out += "}";
    *out_json = dup_out(out);
    return -1;
  }
  *out_json = dup_out(out);
  return 0;
}

// Phase-1 counters (fill_in_counts + fill_in_counts_helper, stopped before any
// phase-2 step) of every workload's first PodSet group, each against the
// snapshot as built: {"levels": [[levelValues...] per domain] per level,
// "results": [{"counters": [5 * S ints, kueue_tas_last_counters' layout] or
// null when the prelude fails before phase 1, "reason": that failure,
// "params": the prelude's sliceSize, sliceLevelIdx, leader, sliceSizeAtLevel}]}.
int tas_oracle_counters(const char* snapshot_json, const char* workloads_json, int simulate_empty, char** out_json) {
  using namespace oracle;
  try {
    ojson::Value c = ojson::parse(snapshot_json);
    ojson::Value w = ojson::parse(workloads_json);
    auto snap = build_snapshot(c);
    std::string out = "{\"levels\":[";
    bool firstL = true;
    for (auto& lvl : snap->levels_in_order()) {
      out += firstL ? "[" : ",[";
      firstL = false;
      for (size_t i = 0; i < lvl.size(); i++) {
        out += i ? ",[" : "[";
        // a hostname leaf keeps its levelValues only (:160-195); they end in its id
        for (size_t k = 0; k < lvl[i]->levelValues.size(); k++) {
          if (k) out += ",";
          ojson::quote(out, lvl[i]->levelValues[k]);
        }
        out += "]";
      }
      out += "]";
    }
    out += "],\"results\":[";
    bool first = true;
    for (auto& wl : w.at("workloads").a) {
      std::vector<int32_t> ctr;
      snap->phase1Counters = &ctr;
      auto rs = snap->find_topology_assignments_for_flavor(parse_podsets(wl), simulate_empty != 0);
      snap->phase1Counters = nullptr;
      out += first ? "{\"counters\":" : ",{\"counters\":";
      first = false;
      if (ctr.empty()) {
        out += "null,\"reason\":";
        ojson::quote(out, rs.empty() ? std::string() : rs[0].reason);
      } else {
        out += "[";
        for (size_t i = 0; i < ctr.size(); i++) out += (i ? "," : "") + std::to_string(ctr[i]);
        out += "],\"reason\":\"\",\"params\":" + snap->phase1Params;
      }
      out += "}";
    }
    out += "]}";
    *out_json = dup_out(out);
    return 0;
  } catch (const std::exception& e) {
    std::string out = "{\"error\":";
    ojson::quote(out, e.what());
    out += "}";
    *out_json = dup_out(out);
    return -1;
  }
}

// The reference's unit-test entry points, called as its tests call them:
//   {"op": "countIn", "requests": {...}, "capacity": {...}}
//       -> {"count", "limitingResource"} (count_in_with_limiting)
//   {"op": "sortedDomains", "withLeader": bool, "unconstrained": bool,
//    "profileMixed": bool (default true), "domains": [{"id", "levelValues",
//    and any of the five counters (default 0)}]}
//       -> {"order": [ids]} (sorted_domains_with_leader / sorted_domains on
//          bare domains of a one-level snapshot)
int tas_oracle_unit(const char* op_json, char** out_json) {
  using namespace oracle;
  try {
    ojson::Value op = ojson::parse(op_json);
    const std::string kind = op.at("op").as_str();
    std::string out;
    if (kind == "countIn") {
      auto r = count_in_with_limiting(parse_requests(op.at("requests")), parse_requests(op.at("capacity")));
      out = "{\"count\":" + std::to_string(r.first) + ",\"limitingResource\":";
      ojson::quote(out, r.second);
      out += "}";
    } else if (kind == "sortedDomains") {
      Snapshot snap({"block"}, {});
      if (auto pm = op.get("profileMixed")) snap.gates.profileMixed = pm->as_bool();
      std::deque<Domain> store;
      std::vector<Domain*> ds;
      auto field = [](const ojson::Value& d, const char* k) {
        auto v = d.get(k);
        return v && !v->is_null() ? int32_t(v->as_int()) : int32_t(0);
      };
      for (auto& d : op.at("domains").a) {
        store.emplace_back();
        Domain& x = store.back();
        x.id = d.at("id").as_str();
        for (auto& v : d.at("levelValues").a) x.levelValues.push_back(v.as_str());
        x.state = field(d, "state");
        x.sliceState = field(d, "sliceState");
        x.stateWithLeader = field(d, "stateWithLeader");
        x.sliceStateWithLeader = field(d, "sliceStateWithLeader");
        x.leaderState = field(d, "leaderState");
        ds.push_back(&x);
      }
      const bool unc = op.at("unconstrained").as_bool();
      auto sorted = op.at("withLeader").as_bool() ? snap.sorted_domains_with_leader(ds, unc) : snap.sorted_domains(ds, unc);
      out = "{\"order\":[";
      for (size_t i = 0; i < sorted.size(); i++) {
        if (i) out += ",";
        ojson::quote(out, sorted[i]->id);
      }
      out += "]}";
    } else {
      throw std::runtime_error("unknown op " + kind);
    }
    *out_json = dup_out(out);
    return 0;
  } catch (const std::exception& e) {
    std::string out = "{\"error\":";
    ojson::quote(out, e.what());
    out += "}";
    *out_json = dup_out(out);
    return -1;
  }
}

void tas_oracle_free(char* p) { free(p); }

}  // extern "C"
