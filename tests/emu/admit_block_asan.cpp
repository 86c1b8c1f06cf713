// TEST INFRASTRUCTURE: kueue_tas_admit_block over malformed blocks and tables,
// under AddressSanitizer and UBSan (tests/emu/build_admit_asan.sh: the device
// layer against the CPU SIMT emulator, whose hipMalloc is calloc, so every
// device buffer and the block itself carry redzones).  A pytest process cannot
// show an out-of-bounds write; this program can, and exits non-zero.
//
// Inputs: hand-built blocks with the code each must return (those of
// tests/test_admit_block_malformed.py), admission tables with columns the
// snapshot does not have, and every single-word mutation of one block.  Per
// input: the code is 0, KUEUE_TAS_ELAYOUT or KUEUE_TAS_EINVAL; on an error the
// usage is untouched (kueue_tas_snapshot_usage_changes lists nothing) and the
// out arrays keep their fill; on 0 the ids, verdicts, delta list and usage
// equal a plain loop over the quads that assumes no layout (admit_reference).
//
// What the sanitizer cannot see: the records, their map and the per-workload
// arrays share ONE allocation (the context's admit buffer), so a write past
// the records that stays inside it has no redzone to hit.  The overlapping-run
// cases are therefore caught by the result comparison here and in the pytest
// cases (wrong verdicts, deltas or usage), not by a sanitizer report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kueue_tas.h"
#include "kueue_tas_debug.h"

namespace {
constexpr int N = 4, R = 3, W = 8, CPU = 0, MEM = 1, PODS = 2, HUGE_WL = W - 1;
constexpr int32_t FILL = -7, I32MAX = INT32_MAX, I32MIN = INT32_MIN;
using Quad = std::vector<int32_t>;
using Rows = std::vector<std::vector<Quad>>;

Quad H(int32_t g, int32_t n, int32_t failed = 0) { return {g, -1, failed, n}; }
Quad D(int32_t g, int32_t leaf, int32_t count, int32_t ps = 0) { return {g, ps, leaf, count}; }

int g_failures = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    if (!(cond)) {                              \
      fprintf(stderr, "FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);             \
      fprintf(stderr, "\n");                    \
      g_failures++;                             \
    }                                           \
  } while (0)

struct Term {
  int32_t col;
  int64_t value;
};
// workload -> PodSets -> terms: one PodSet each but workload 1 (two)
std::vector<std::vector<std::vector<Term>>> table() {
  std::vector<std::vector<std::vector<Term>>> t(W);
  for (int g = 0; g < W; g++) t[g] = {{{CPU, 1 + g % 3}, {MEM, 10}}};
  t[1].push_back({{CPU, 2}});
  t[HUGE_WL] = {{{CPU, int64_t(1) << 40}}};
  return t;
}

struct Block {
  std::vector<int32_t> words;  // exactly world x row_words: a read past it meets a redzone
  std::vector<int64_t> lens;
  size_t row_words;
  std::vector<int32_t> quads() const {
    std::vector<int32_t> q;
    for (size_t r = 0; r < lens.size(); r++)
      for (int64_t i = 0; i < lens[r]; i++) q.push_back(words[r * row_words + 1 + size_t(i)]);
    return q;
  }
};
Block make_block(const Rows& rows, size_t cap_extra = 2) {
  Block b;
  size_t longest = 0;
  for (auto& r : rows) longest = std::max(longest, 4 * r.size());
  b.row_words = longest + 1 + cap_extra;
  b.words.assign(rows.size() * b.row_words, 0);
  for (size_t r = 0; r < rows.size(); r++) {
    b.lens.push_back(int64_t(4 * rows[r].size()));
    b.words[r * b.row_words] = int32_t(4 * rows[r].size());
    for (size_t q = 0; q < rows[r].size(); q++)
      for (int k = 0; k < 4; k++) b.words[r * b.row_words + 1 + 4 * q + size_t(k)] = rows[r][q][size_t(k)];
  }
  return b;
}

struct Harness {
  kueue_tas_ctx* ctx = nullptr;
  int64_t free_cap[R][N], usage[R][N];  // the model of the device's snapshot
  std::vector<std::vector<std::vector<Term>>> tab = table();

  int load(int cols) {
    static int32_t sizes[1] = {N}, co[1] = {0};
    static uint32_t fp[N], up[N];
    static int64_t fc[R * N], us[R * N];
    for (int c = 0; c < R; c++)
      for (int i = 0; i < N; i++) {
        free_cap[c][i] = c == CPU ? 8 : c == MEM ? 100 : 110;
        usage[c][i] = 0;
        fc[c * N + i] = free_cap[c][i];
        us[c * N + i] = 0;
      }
    for (int i = 0; i < N; i++) fp[i] = up[i] = (1u << cols) - 1;
    kueue_tas_snapshot_desc d{};
    d.num_levels = 1;
    d.level_sizes = sizes;
    d.child_offsets = co;
    d.num_cols = cols;
    d.free_capacity = fc;
    d.tas_usage = us;
    d.free_present = fp;
    d.usage_present = up;
    d.lowest_is_hostname = 1;
    int rc = kueue_tas_snapshot_load(ctx, &d);
    if (rc == 0) rc = kueue_tas_snapshot_usage_mark(ctx);
    return rc;
  }
  int upload(const std::vector<std::vector<std::vector<Term>>>& t) {
    std::vector<int32_t> base{0}, pst;
    std::vector<kueue_tas_fits_term> terms;
    for (auto& wl : t) {
      for (auto& ps : wl) {
        pst.push_back(int32_t(terms.size()));
        pst.push_back(int32_t(ps.size()));
        for (auto& tm : ps) terms.push_back({tm.value, tm.col, 0});
      }
      base.push_back(int32_t(pst.size() / 2));
    }
    return kueue_tas_admit_table(ctx, base.data(), int32_t(t.size()), pst.data(), terms.data(), terms.size());
  }
  Harness() {
    kueue_tas_config cfg{};
    ctx = kueue_tas_ctx_create(&cfg);
    if (!ctx || load(R) || upload(tab)) {
      fprintf(stderr, "setup failed: %s\n", ctx ? kueue_tas_last_error(ctx) : "no context");
      exit(2);
    }
  }
  ~Harness() { kueue_tas_ctx_destroy(ctx); }

  // The device's usage moved exactly as the model says (absolute values of
  // every (leaf, column) that changed since the last look).
  void check_usage(const char* what, bool expect_none) {
    const kueue_tas_delta* ch = nullptr;
    size_t n = 0;
    CHECK(kueue_tas_snapshot_usage_changes(ctx, &ch, &n) == 0, "%s: %s", what, kueue_tas_last_error(ctx));
    if (expect_none) CHECK(n == 0, "%s: %zu usage values moved on an error", what, n);
    for (size_t i = 0; i < n; i++)
      CHECK(ch[i].leaf >= 0 && ch[i].leaf < N && ch[i].col >= 0 && ch[i].col < R &&
                ch[i].delta == usage[ch[i].col][ch[i].leaf],
            "%s: usage[%d][%d] = %lld", what, ch[i].col, ch[i].leaf, (long long)ch[i].delta);
  }

  // TASFlavorSnapshot.Fits of one record: min over the terms of
  // int32(free - usage) / value, at least 0; no terms: 0.
  bool fits(int32_t leaf, int32_t count, const std::vector<Term>& terms) const {
    int32_t result = 0;
    bool any = false;
    for (auto& t : terms) {
      int32_t c = I32MAX;
      if (t.value != 0) c = std::max(int32_t(uint32_t(uint64_t((free_cap[t.col][leaf] - usage[t.col][leaf]) / t.value))), 0);
      if (!any || c < result) result = c;
      any = true;
    }
    return (any ? result : 0) >= count;
  }

  struct Ref {
    bool error = false;
    std::vector<int32_t> ids, verdicts;
    std::vector<kueue_tas_delta> deltas;
  };
  // kueue_tas_host_admit's reading of the quads, no layout assumed: a workload
  // is present with any quad, failed with any failed header; its records are
  // its domain quads in order; ascending ids, each admitted when every record
  // fits the usage so far, then added (value x count in 128 bits, kept as the
  // low 64 as the library's wrapping product; pods: count).  Updates the model.
  Ref admit_reference(const std::vector<int32_t>& q) {
    Ref ref;
    std::map<int32_t, std::vector<Quad>> recs;
    std::map<int32_t, bool> failed;
    for (size_t i = 0; i + 3 < q.size(); i += 4) {
      const int32_t g = q[i];
      if (g < 0 || g >= W) ref.error = true;
      if (ref.error) continue;
      recs[g];
      if (q[i + 1] < 0) {
        if (q[i + 2] != 0) failed[g] = true;
      } else if (size_t(q[i + 1]) >= tab[size_t(g)].size() || q[i + 2] < 0 || q[i + 2] >= N) {
        ref.error = true;
      } else {
        recs[g].push_back({q[i + 1], q[i + 2], q[i + 3]});
      }
    }
    if (ref.error) return ref;
    for (auto& kv : recs) {
      const int32_t g = kv.first;
      bool ok = !failed[g];
      for (auto& r : kv.second) ok = ok && fits(r[1], r[2], tab[size_t(g)][size_t(r[0])]);
      ref.ids.push_back(g);
      ref.verdicts.push_back(ok ? 1 : 0);
      if (!ok) continue;
      for (auto& r : kv.second) {
        for (auto& t : tab[size_t(g)][size_t(r[0])]) {
          const __int128 p = __int128(t.value) * r[2];
          const int64_t d = int64_t(uint64_t(p));
          ref.deltas.push_back({r[1], t.col, d});
          usage[t.col][r[1]] = int64_t(uint64_t(usage[t.col][r[1]]) + uint64_t(d));
        }
        ref.deltas.push_back({r[1], PODS, r[2]});
        usage[PODS][r[1]] += r[2];
      }
    }
    return ref;
  }

  // One call and its checks; want: the code it must return, or 1 for "any of the three".
  int run(const std::string& name, const Block& b, int want = 1, int32_t pods_col = PODS) {
    int32_t ids[W], adm[W];
    for (int i = 0; i < W; i++) ids[i] = adm[i] = FILL;
    size_t nw = 0, nd = 0;
    const kueue_tas_delta* dl = nullptr;
    const int rc = kueue_tas_admit_block(ctx, b.words.data(), b.row_words, b.lens.data(), int32_t(b.lens.size()),
                                         pods_col, ids, adm, W, &nw, &dl, &nd);
    const char* nm = name.c_str();
    CHECK(rc == 0 || rc == KUEUE_TAS_ELAYOUT || rc == KUEUE_TAS_EINVAL, "%s: code %d", nm, rc);
    if (want != 1) CHECK(rc == want, "%s: code %d, expected %d (%s)", nm, rc, want, kueue_tas_last_error(ctx));
    if (rc != 0) {
      for (int i = 0; i < W; i++) CHECK(ids[i] == FILL && adm[i] == FILL, "%s: out arrays written on an error", nm);
      check_usage(nm, true);
      return rc;
    }
    int64_t before[R][N];
    memcpy(before, usage, sizeof usage);
    const Ref ref = admit_reference(b.quads());
    CHECK(!ref.error, "%s: admitted a block the host path rejects", nm);
    if (ref.error) {
      memcpy(usage, before, sizeof usage);
      reload();
      return rc;
    }
    CHECK(nw == ref.ids.size(), "%s: %zu workloads, expected %zu", nm, nw, ref.ids.size());
    for (size_t k = 0; k < nw && k < ref.ids.size(); k++)
      CHECK(ids[k] == ref.ids[k] && adm[k] == ref.verdicts[k], "%s: workload %zu = (%d, %d), expected (%d, %d)", nm, k,
            ids[k], adm[k], ref.ids[k], ref.verdicts[k]);
    CHECK(nd == ref.deltas.size(), "%s: %zu deltas, expected %zu", nm, nd, ref.deltas.size());
    for (size_t i = 0; i < nd && i < ref.deltas.size(); i++)
      CHECK(dl[i].leaf == ref.deltas[i].leaf && dl[i].col == ref.deltas[i].col && dl[i].delta == ref.deltas[i].delta,
            "%s: delta %zu = (%d, %d, %lld), expected (%d, %d, %lld)", nm, i, dl[i].leaf, dl[i].col,
            (long long)dl[i].delta, ref.deltas[i].leaf, ref.deltas[i].col, (long long)ref.deltas[i].delta);
    check_usage(nm, false);
    reload();
    return rc;
  }
  // every input starts from the empty usage
  void reload() {
    if (load(R)) {
      fprintf(stderr, "reload failed: %s\n", kueue_tas_last_error(ctx));
      exit(2);
    }
  }
};

const Rows GOOD = {{H(0, 2), D(0, 0, 1), D(0, 1, 1), H(1, 2), D(1, 2, 1, 1), D(1, 3, 2), H(2, 1), D(2, 1, 200)},
                   {H(3, 1), D(3, 0, 2), H(5, 0), H(4, 1, 1), D(4, 2, 1)}};
}  // namespace

// With an argument: only the inputs whose name contains it (no mutations).
int main(int argc, char** argv) {
  Harness h;
  const std::string only = argc > 1 ? argv[1] : "";
  auto wanted = [&](const std::string& name) { return only.empty() || name.find(only) != std::string::npos; };
  const int OK = 0, EL = KUEUE_TAS_ELAYOUT, EI = KUEUE_TAS_EINVAL;
  std::vector<Quad> eight;
  for (int g = 0; g < 8; g++) eight.push_back(H(g, 8));
  for (int k = 0; k < 8; k++) eight.push_back(D(7, 0, 1));
  struct HandCase {
    const char* name;
    Rows rows;
    int want;
  };
  const std::vector<HandCase> hand = {
      {"well_formed", GOOD, OK},
      {"overlap_sum_above_quads", {eight}, EL},
      {"overlap_sum_balanced", {{H(0, 2), H(1, 1), D(1, 0, 1), D(1, 1, 1), D(0, 0, 1)}}, EL},
      {"header_inside_run", {{H(0, 2), D(0, 0, 1), H(1, 0), D(0, 1, 1)}}, EL},
      {"orphan_trailing_with_header", {{H(0, 1), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"orphan_trailing_without_header", {{H(0, 1), D(0, 0, 1), D(6, 1, 1)}}, EL},
      {"orphan_leading", {{D(6, 1, 1), H(0, 1), D(0, 0, 1)}}, EL},
      {"orphan_between_runs", {{H(0, 1), D(0, 0, 1), D(6, 1, 1), H(2, 1), D(2, 1, 1)}}, EL},
      {"run_across_rows", {{H(0, 1), D(0, 0, 1), H(2, 1)}, {D(2, 1, 1), H(3, 0)}}, EL},
      {"header_count_-1", {{H(1, 0), H(0, -1), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"header_count_min", {{H(1, 0), H(0, I32MIN), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"header_count_max", {{H(1, 0), H(0, I32MAX), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"header_count_max_minus_q", {{H(1, 0), H(0, I32MAX - 1), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"header_count_nq_minus_q", {{H(1, 0), H(0, 3), D(0, 0, 1), D(0, 1, 1)}}, EL},
      {"header_count_largest_legal", {{H(1, 0), H(0, 2), D(0, 0, 1), D(0, 1, 1)}}, OK},
      {"duplicate_header_one_row", {{H(0, 1), D(0, 0, 1), H(0, 1), D(0, 1, 1)}}, EL},
      {"duplicate_header_two_rows", {{H(0, 1), D(0, 0, 1)}, {H(0, 1), D(0, 1, 1)}}, EL},
      {"failed_header_with_quads", {{H(0, 2, 1), D(0, 0, 1), D(0, 1, 1), H(1, 0)}}, OK},
      {"failed_header_bad_quad", {{H(0, 2, 1), D(0, 0, 1), D(0, N, 1), H(1, 0)}}, EI},
      {"header_without_quads", {{H(0, 0), H(1, 0), H(2, 1), D(2, 0, 1)}}, OK},
      {"header_id_W", {{H(W, 0), H(1, 1), D(1, 0, 1)}}, EL},
      {"header_id_minus_1", {{H(-1, 0), H(1, 1), D(1, 0, 1)}}, EL},
      {"podset_out_of_range", {{H(0, 1), D(0, 0, 1, 1)}}, EI},
      {"second_podset", {{H(1, 2), D(1, 0, 1, 1), D(1, 0, 1, 0)}}, OK},
      {"leaf_N", {{H(1, 1), D(1, N, 1)}}, EI},
      {"leaf_minus_1", {{H(1, 1), D(1, -1, 1)}}, EI},
      {"count_0", {{H(0, 2), D(0, 0, 0), D(0, 1, 1)}}, OK},
      {"count_negative", {{H(0, 2), D(0, 0, -1), D(0, 1, 1), H(1, 1), D(1, 0, 1)}}, OK},
      {"count_max_times_huge_request", {{H(0, 1), D(0, 0, 1), H(HUGE_WL, 1), D(HUGE_WL, 1, I32MAX)}}, OK},
      {"all_rows_empty", {{}, {}, {}}, OK},
  };
  for (auto& c : hand)
    if (wanted(c.name)) h.run(c.name, make_block(c.rows), c.want);
  if (only.empty()) {  // row shapes
    Rows rows16(16);
    rows16[0] = GOOD[0];
    h.run("world_16_fifteen_empty", make_block(rows16), OK);
    h.run("row_words_exact", make_block(GOOD, 0), OK);
    Block b = make_block(GOOD, 0);
    b.lens[0] -= 2;
    h.run("row_length_not_quads", b, EI);
    b = make_block(GOOD, 0);
    b.lens[0] += 4;
    h.run("row_length_above_row_words", b, EI);
    Rows rows20(20);
    rows20[19] = GOOD[1];
    h.run("world_20", make_block(rows20), EL);
  }
  // every single-word mutation of one small block (the length word included)
  const Block base = make_block({{H(0, 1), D(0, 0, 1), H(1, 0)}}, 0);
  size_t outcomes[3] = {0, 0, 0};
  for (size_t r = 0; r < base.lens.size() && only.empty(); r++) {
    const int32_t nq = int32_t(base.lens[r] / 4);
    for (size_t j = 0; j < base.row_words; j++) {
      const int32_t q = std::min(int32_t(j > 0 ? (j - 1) / 4 : 0), nq - 1);
      for (int32_t v : {-1, 0, 1, 2, W - 1, W, N - 1, N, nq - q - 1, nq - q, I32MAX, I32MIN}) {
        Block b = base;
        b.words[r * b.row_words + j] = v;
        const int rc = h.run("mutation row " + std::to_string(r) + " word " + std::to_string(j) + " = " + std::to_string(v), b);
        outcomes[rc == 0 ? 0 : rc == EL ? 1 : 2]++;
      }
    }
  }
  CHECK(!only.empty() || (outcomes[0] && outcomes[1] && outcomes[2]), "mutations: %zu admitted, %zu ELAYOUT, %zu EINVAL", outcomes[0],
        outcomes[1], outcomes[2]);
  // admission tables: columns the snapshot does not have
  const Block two = make_block({{H(0, 1), D(0, 0, 1), H(1, 1), D(1, 1, 1)}});
  for (int32_t col : {R, KUEUE_TAS_MAX_COLS - 1, KUEUE_TAS_MAX_COLS, -2}) {
    if (!wanted("table column " + std::to_string(col))) continue;
    auto t = h.tab;
    t[0][0][0].col = col;
    const int trc = h.upload(t);
    CHECK(trc == EI, "table column %d accepted", col);
    if (trc == OK) {  // (a library that takes it: the call must reject the term)
      h.run("table column " + std::to_string(col) + " in use", two, EI);
      CHECK(h.upload(h.tab) == OK, "%s", kueue_tas_last_error(h.ctx));
      continue;
    }
    h.check_usage("table column", true);
    h.run("after a rejected table", two, OK);  // the table from before is still the context's
  }
  if (wanted("table column -1")) {  // (a resource without a column): the call that uses the term reports it
    auto t = h.tab;
    t[0][0][0].col = -1;
    CHECK(h.upload(t) == OK, "%s", kueue_tas_last_error(h.ctx));
    h.run("table column -1", two, EI);
    h.run("table column -1, term unused", make_block({{H(1, 1), D(1, 1, 1)}}), OK);
    CHECK(h.upload(h.tab) == OK, "%s", kueue_tas_last_error(h.ctx));
  }
  if (wanted("stale table")) {  // a table from before a reload that leaves fewer columns
    auto t = h.tab;
    t[0][0][0].col = R - 1;
    CHECK(h.upload(t) == OK, "%s", kueue_tas_last_error(h.ctx));
    CHECK(h.load(R - 1) == 0, "%s", kueue_tas_last_error(h.ctx));
    h.run("stale table", two, EI, -1);
    h.reload();
  }
  if (g_failures) {
    fprintf(stderr, "admit_block_asan: %d checks failed\n", g_failures);
    return 1;
  }
  printf("admit_block_asan: ok (mutations: %zu admitted, %zu ELAYOUT, %zu EINVAL)\n", outcomes[0], outcomes[1], outcomes[2]);
  return 0;
}
