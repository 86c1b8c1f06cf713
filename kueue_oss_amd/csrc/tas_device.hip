// tas_device.cpp — device layer of libkueue_tas.so: HBM-resident snapshot,
// batch staging and kernel launches behind the C-ABI of include/kueue_tas.h.
//
// Data layout in HBM (per context):
//   snapshot  free_cap[R][N], tas_usage[R][N] (int64 SoA), presence bitmasks
//             [N], taint-profile ids [N], label-value ids [K][N], CSR child
//             offsets per level, DomainID ranks [sum D_l]
//   per batch counters[n][5][sum D_l] int32 (state, sliceState, stateWithLeader,
//             sliceStateWithLeader, leaderState), exclusion counters, phase-2
//             scratch lists, result headers and (leaf, count) entries
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "tas_internal.h"
#include "tas_pool.h"
#include "tas_kernels.hip"

using namespace ktas;

namespace {

constexpr int kEvalsPerFillBlock = kEvalsPerBlock;

// A simple class: no leader, one-pod slices at the leaf level and no inner
// slice rounding, so sliceState == state at every level: its class row keeps
// one field (FillEvalParams::ss_alias, ctr_row).
bool simple_class(const DevEval& ev, int L) {
  bool simple = (ev.flags & KUEUE_TAS_F_LEADER) == 0 && ev.slice_level == L - 1 && ev.slice_size == 1;
  for (int l = 0; l < L && simple; l++) simple = ev.ssal[l] == 0 || ev.ssal[l] == 1;
  return simple;
}

// Device bytes per context (kueue_tas_device_bytes): every DevBuf built
// while a context is constructed links itself into that context's chain.
struct DevBufLink {
  size_t bytes = 0;
  DevBufLink* next = nullptr;
};
thread_local DevBufLink** g_devbuf_chain = nullptr;

template <typename T>
struct DevBuf : DevBufLink {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() {
    if (g_devbuf_chain) {
      next = *g_devbuf_chain;
      *g_devbuf_chain = this;
    }
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    bytes = 0;
    size_t nb = std::max<size_t>(count, 1) * sizeof(T);
    hipError_t e = hipMalloc(&p, nb);
    if (e == hipSuccess) {
      n = std::max<size_t>(count, 1);
      bytes = nb;
    }
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    bytes = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(bytes, o.bytes);
  }
  // ensure with 1/8 headroom when it grows (buffers that grow by a few rows at a time)
  hipError_t reserve(size_t count) { return count <= n && p ? hipSuccess : ensure(count + count / 8); }
};

template <typename T>
struct HostBuf {  // pinned host staging
  T* p = nullptr;
  size_t n = 0;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() { release(); }
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault);
    if (e == hipSuccess) n = std::max<size_t>(count, 1);
    return e;
  }
  // ensure with 1/8 headroom when it grows (a pinned allocation costs a millisecond)
  hipError_t reserve(size_t count) { return count <= n && p ? hipSuccess : ensure(count + count / 8); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    n = 0;
  }
};

// Open-addressing uint64 -> int32 map (linear probing), reset per batch
// without freeing: the phase-1 class lookup of every eval.
struct FlatMap {
  std::vector<uint64_t> keys;
  std::vector<int32_t> vals;  // -1: empty
  size_t mask = 0;
  void reset(size_t n) {
    size_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    if (keys.size() != cap) {
      keys.assign(cap, 0);
      vals.assign(cap, -1);
    } else {
      std::fill(vals.begin(), vals.end(), -1);
    }
    mask = cap - 1;
  }
  static size_t mix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return size_t(k);
  }
  int32_t* find(uint64_t k) {  // the slot's value (-1 if absent)
    for (size_t i = mix(k) & mask;; i = (i + 1) & mask) {
      if (vals[i] < 0 || keys[i] == k) {
        keys[i] = k;
        return &vals[i];
      }
    }
  }
};

// One static part's phase-1 classes (eval_chunk): chains of local classes
// per 64-bit class hash, each local class's first member.
struct alignas(64) PartClasses {  // one per host part, on cache lines of its own
  FlatMap head;
  std::vector<int32_t> rep, next;
  std::vector<uint64_t> hcls, hsig;  // each local class's hashes, contiguous for the merge
};

// libdivide-style u64 magic for exact division by an invariant divisor d >= 1.
// 2^(64 + fl) / d and its remainder for 2^fl < d < 2^(fl + 1): the quotient
// fits 64 bits, so one 128-by-64 divq gives both (two __int128 divisions
// through the runtime library cost ~10x that per term)
static inline uint64_t div_pow2_by(int fl, uint64_t d, uint64_t* rem) {
  uint64_t q, r;
  __asm__("divq %4" : "=a"(q), "=d"(r) : "a"(uint64_t(0)), "d"(uint64_t(1) << fl), "rm"(d));
  *rem = r;
  return q;
}

void compute_magic_uncached(uint64_t d, DevTerm* t) {
  t->magic = 0;
  t->shift = 0;
  t->add = 0;
  t->pow2 = 0;
  int fl = 63 - __builtin_clzll(d);
  if ((d & (d - 1)) == 0) {
    t->pow2 = 1;
    t->shift = uint8_t(fl);
    return;
  }
  uint64_t rem;
  uint64_t proposed = div_pow2_by(fl, d, &rem);
  uint64_t e = d - rem;
  if (e < (uint64_t(1) << fl)) {
    t->shift = uint8_t(fl);
  } else {
    proposed += proposed;
    uint64_t twice = rem + rem;
    if (twice >= d || twice < rem) proposed += 1;
    t->shift = uint8_t(fl);
    t->add = 1;
  }
  t->magic = proposed + 1;
}

// the divisors of a batch repeat (a request shape per workload type): a
// direct-mapped cache of the magic numbers per host part, kept in the
// context (a thread_local here cost a __tls_get_addr call per term)
struct MagicSlot {
  uint64_t d = 0, magic = 0;
  uint8_t shift = 0, add = 0, pow2 = 0;
};
struct alignas(64) MagicCache {
  MagicSlot slot[256];
};
void compute_magic(uint64_t d, DevTerm* t, MagicCache& cache) {
  MagicSlot& c = cache.slot[(d * 0x9e3779b97f4a7c15ull) >> 56];
  if (c.d != d) {
    compute_magic_uncached(d, t);
    c.d = d;
    c.magic = t->magic;
    c.shift = t->shift;
    c.add = t->add;
    c.pow2 = t->pow2;
    return;
  }
  t->magic = c.magic;
  t->shift = c.shift;
  t->add = c.add;
  t->pow2 = c.pow2;
}

// Environment knobs, read once per context at creation (kueue_tas_ctx_create;
// a KUEUE_TAS_CFG_* flag that overrides one writes into the same struct).
struct Knobs {
  int admit_grid_sweeps = 6;  // KTAS_ADMIT_PHASES: window-kernel phases (rejection sweeps over the grid between them); 1: in-kernel
  int admit_step_run = 2 * kAdmitWindow;  // KTAS_ADMIT_STEP_RUN: kueue_tas_admit_targets: target-free runs shorter than this go
                                          // through admit_step_kernel
  int64_t phase2_budget = int64_t(4096) << 20;  // KTAS_PHASE2_BUDGET: bytes of select lists + overlays + tags per slot group
                                                // (tests: a small budget, many groups)
  bool force_scratch_rerun = false;  // KTAS_SCRATCH_TEST_RERUN (set): tests: every chunk re-runs once
  int64_t lcap_test_cap = 0;         // KTAS_SCRATCH_TEST_CAP: tests: bounded lists capped lower (overflows re-run unbounded)
  bool scratch_bounded = true;       // KTAS_SCRATCH_FULL=1 clears it: every slot's lists sized for the widest level
  bool lfc_in_fill = false;    // KTAS_LFC_IN_FILL=1: fast-LFC chunk tables from the pair fill (no lfc_hist_kernel);
                               // off by default: it lengthens the fill on the main chain
                               // by more than it saves the side stream
  bool emit_after_bf = false;  // KTAS_EMIT_MAIN=1: lfc_emit on the main stream after the BestFit select
  int32_t exp_flags = 0;       // KTAS_EXP_FLAGS: diagnostics only (tools/probe_select.py experiments)

  static Knobs from_env() {
    Knobs k;
    auto on = [](const char* name) {
      const char* e = getenv(name);
      return e && atoi(e) != 0;
    };
    if (const char* e = getenv("KTAS_ADMIT_PHASES")) k.admit_grid_sweeps = std::max(1, atoi(e));
    if (const char* e = getenv("KTAS_ADMIT_STEP_RUN")) k.admit_step_run = std::max(0, atoi(e));
    if (const char* e = getenv("KTAS_PHASE2_BUDGET")) k.phase2_budget = std::max<int64_t>(atoll(e), 1);
    k.force_scratch_rerun = getenv("KTAS_SCRATCH_TEST_RERUN") != nullptr;
    if (const char* e = getenv("KTAS_SCRATCH_TEST_CAP")) k.lcap_test_cap = std::max<int64_t>(atoll(e), 1);
    k.scratch_bounded = !on("KTAS_SCRATCH_FULL");
    k.lfc_in_fill = on("KTAS_LFC_IN_FILL");
    k.emit_after_bf = on("KTAS_EMIT_MAIN");
    if (const char* e = getenv("KTAS_EXP_FLAGS")) k.exp_flags = int32_t(atoi(e));
    return k;
  }
};

}  // namespace

struct kueue_tas_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // fast-LFC branch (tables, select, emit) beside the BestFit select
  hipStream_t stream3 = nullptr;  // ExclusionStats branch (staged fill): counts + reduce beside the roll-up/select
  hipEvent_t evs[2] = {};         // ExclusionStats branch: start, end (also the join)
  DevBuf<int8_t> d_fill_lim;
  std::vector<int32_t> cls_pos, cls_cur;
  hipEvent_t ev[8] = {};  // stage boundaries, see eval_chunk
  hipEvent_t evl[4] = {};  // fast-LFC branch: start, end (timing), join, fast select done (emit on the main stream)
  std::string err;
  int list_cap = 1024;
  bool inline_stats = true;   // ExclusionStats counted in the fill (KUEUE_TAS_CFG_SPLIT_STATS: fill_exclusion_kernel)
  bool pair_fill = true;      // fill_pair_kernel for single-run chunks (KUEUE_TAS_CFG_NO_PAIR_FILL clears it)
  bool admit_window = true;   // admit_window_kernel (KUEUE_TAS_CFG_SERIAL_ADMIT: the one-wave chain)
  Knobs knobs;                // the KTAS_* environment knobs (Knobs::from_env at creation)
  bool fused_top = false;    // rollup_top_kernel (KUEUE_TAS_CFG_FUSED_TOP)
  bool cat_fill = true;       // fill_pair_kernel's leaf categories (KUEUE_TAS_CFG_NO_CATEGORY_FILL clears it)
  bool labels16 = false;      // every staged label column's value ids < 2^16 (packed nodeSelector compare)
  int64_t n_loads = 0, n_splices = 0;  // kueue_tas_snapshot_load / _splice calls that succeeded (lifetime)
  bool stage_timing = true;   // record every stage event (else only the fill bracket; kueue_tas_set_stage_timing)
  int max_batch = 1024;
  int entry_cap = 512;  // per-eval device entry capacity (grows on demand)
  // snapshot
  bool loaded = false;
  DevSnap snap{};
  int maxD = 0;
  int rack_fanout = 0;  // see kueue_tas_snapshot_load
  std::vector<int32_t> h_level_sizes;
  DevBuf<int32_t> d_child_off, d_id_rank, d_taint_profile, d_labels;
  DevBuf<uint8_t> d_dead;        // leaves out of the snapshot (kueue_tas_snapshot_set_leaf_live)
  std::vector<uint8_t> h_dead;
  int64_t n_dead = 0;
  DevBuf<int64_t> d_free, d_usage;
  DevBuf<uint32_t> d_free_present, d_usage_present;
  // batch
  DevBuf<int32_t> d_counters;
  // results of a batch, one D2H: out[n] | stats (taint | res | sel counts)
  DevBuf<uint8_t> d_res;
  HostBuf<uint8_t> h_res;
  HostBuf<kueue_tas_eval_out> h_res2;  // the fast-LFC branch's own copy of the result headers (its D2H)
  kueue_tas_eval_out* res_out_h = nullptr;
  int32_t* res_stats_h = nullptr;
  DevBuf<uint64_t> d_scratch;
  DevBuf<kueue_tas_delta> d_deltas;
  DevBuf<uint8_t> d_setfree;  // set_free: leaves | rows | presence
  DevBuf<uint8_t> d_fits;  // kueue_tas_fits: requests | terms | results
  // v1beta2 encoder: parent map (leaf mode), resident names, per-call buffers
  DevBuf<int32_t> d_parent;
  DevBuf<int2> d_wave_tab;       // ragged parents: packed leaf waves (DevSnap::wave_tab)
  DevBuf<int32_t> d_leaf_parent;
  DevBuf<char> d_names;
  DevBuf<int64_t> d_name_off;
  bool names_loaded = false;
  DevBuf<char> d_enc_bytes;
  DevBuf<int64_t> d_enc_stroff, d_enc_off;
  DevBuf<int32_t> d_enc_ids, d_enc_counts, d_enc_same;
  DevBuf<kueue_tas_level_enc> d_enc_out;
  DevBuf<int32_t> d_packed;
  DevBuf<LeafPartial> d_partials;
  DevBuf<int32_t> d_fill_stats;
  HostBuf<uint8_t> h_stage;  // one pinned upload per batch: evals, terms, tables, index lists
  DevBuf<uint8_t> d_stage;
  // phase-1 class computation scratch (kept to avoid reallocation)
  std::vector<int32_t> cls_rep, cls_sig, cls_of, sig_rep, cls_next, sig_next, cls_fastrep, cls_slot, cls_order;
  std::vector<int32_t> sig_base, base_rep, cls_packed, sig_ncls;
  FlatMap cls_head, sig_head;
  DevBuf<int32_t> d_overlay, d_tags;
  DevBuf<int2> d_wave_tab2;     // 128-leaf slots of whole ragged parents (fill_pair_kernel, FC = -1)
  DevBuf<int32_t> d_wide;       // leaf parents wider than a slot (DevSnap::wide_parents)
  DevBuf<uint64_t> d_rack_pos;  // positive-child masks of the leaves' parents (fused fill)  // select's copy-on-write counters and ownership tags
  int32_t tag_epoch = 0;
  // fast-LFC leaf tables (LfcJob, tas_internal.h)
  DevBuf<uint32_t> d_lfc_ch, d_lfc_cp, d_lfc_tot;
  DevBuf<uint64_t> d_lfc_ovs, d_lfc_ovtot;
  DevBuf<uint8_t> d_lfc_u8;
  DevBuf<LfcJob> d_lfc_jobs;
  DevBuf<LfcItem> d_lfc_items;  // [0]: item count, then the items
  DevBuf<int32_t> d_prof;             // profiling build: [n][P_NCAT] select phase ticks
  DevBuf<int32_t> d_fprof;            // profiling build: fill phase stamps [blocks][8]
  std::vector<int32_t> last_fprof;
  DevBuf<int32_t> d_level_max;        // [n][kMaxLevels] level_max_kernel
  std::vector<int32_t> last_prof;
  int num_profiles = 1;
  int64_t stat_fills = 0, stat_evals = 0;  // phase-1 dedup counters (lifetime)
  std::vector<int32_t> last_ticks;    // per-eval select time (100 MHz ticks) of the last batch
  // packed (leaf, count) pairs of the last batch: pinned, device-mapped host
  // memory the pack kernel writes directly (no separate D2H copy or sync)
  int32_t* ent_host = nullptr;
  int32_t* ent_dev = nullptr;
  size_t ent_cap = 0;   // int32 capacity
  size_t ent_used = 0;  // int32 used by the last batch
  // entry tags (kueue_tas_snapshot_set_leaf_tags): per-leaf table in HBM, the
  // per-entry copies in pinned device-mapped host memory beside the entries
  DevBuf<uint64_t> d_leaf_tags;
  HostBuf<int32_t> h_admit;          // kueue_tas_admit's verdicts + its two diagnostics words (pinned D2H)
  int64_t admit_stats[3] = {-1, -1, -1};  // last kueue_tas_admit: window rounds, in-order candidates, candidates
  int64_t admit_launches[3] = {0, 0, 0};  // last kueue_tas_admit(_targets): pass runs, step launches, kernel launches
  // kueue_tas_snapshot_splice: the gather's targets (the resident columns'
  // previous buffers after the swap, reused by the next splice) and its
  // pinned staging (leaf sources and joined rows)
  DevBuf<int64_t> sp_free, sp_usage;
  DevBuf<uint32_t> sp_fp, sp_up;
  DevBuf<int32_t> sp_prof, sp_lab, sp_src;
  DevBuf<uint64_t> sp_tags;
  DevBuf<uint8_t> sp_rows;
  HostBuf<uint8_t> h_load;
  HostBuf<uint8_t> h_tab;  // load_impl's re-derived tables (pinned arena, async copies)
  // host-mirror shadow of the usage columns and presence bits (usage_mark / usage_changes)
  DevBuf<int64_t> d_ushadow;
  DevBuf<uint32_t> d_pshadow;
  DevBuf<kueue_tas_delta> d_uchg;
  DevBuf<int32_t> d_uchg_n;
  HostBuf<int32_t> h_uchg_n;
  std::vector<kueue_tas_delta> uchg;
  bool shadow_ok = false;
  // apply_deltas stages the records in pinned memory (async copy, no sync);
  // the event guards the staging buffer's reuse
  HostBuf<kueue_tas_delta> h_deltas;
  hipEvent_t ev_deltas = nullptr;
  bool leaf_tags_on = false;
  uint64_t* tag_host = nullptr;
  uint64_t* tag_dev = nullptr;
  size_t tag_cap = 0;   // uint64 capacity (entry pairs)
  int32_t ent_stride = 0;              // pairs per eval region of the last chunk
  std::vector<int32_t> ent_count;      // pairs written per eval of the last batch (request order)
  std::vector<int64_t> ent_strided_off;  // their region offsets (pairs) in ent_host
  float last_ms[4] = {0, 0, 0, 0};
  float last_stage_ms[KUEUE_TAS_NUM_STAGES] = {};
  std::vector<MagicCache> magic_cache;  // per host part (compute_magic)
  std::vector<int32_t> h_gsrc;          // a splice's leaf sources (load_impl)
  DevBuf<int32_t> d_adm_ps;             // kueue_tas_admit_table: podset base per workload [W + 1], then (begin, n) per podset
  DevBuf<kueue_tas_fits_term> d_adm_terms;  // and the podsets' single-pod request terms
  int32_t adm_W = -1;                   // workloads of the admission table (-1: none)
  DevBuf<kueue_tas_delta> d_adm_deltas; // kueue_tas_admit_block's delta list
  HostBuf<kueue_tas_delta> h_adm_deltas;
  double admit_block_ms = 0;
  std::vector<int32_t> ctr_row_off;     // last batch: each fill position's class row offset (units of SD)
  std::vector<int32_t> level_maxfan;    // [L] the widest parent's child count per level (last load)
  std::vector<int32_t> sel_groups;      // last batch: BestFit-side slot groups (select launches), bounds
  bool scratch_full = false;            // this chunk re-runs with unbounded select lists (an eval overflowed)
  int64_t scratch_reruns = 0;           // chunks re-run so
  DevBufLink* dev_bufs = nullptr;       // every DevBuf member (kueue_tas_device_bytes)
  bool exact_merge = false;  // the next chunk merges the parts' classes with exact compares (after a collision)
  int64_t merge_reruns = 0;  // chunks re-run after a class hash collision
  size_t lfc_half = 0;        // LFC chunk-table entries per half of d_lfc_ch / d_lfc_ovs
  bool lfc_dirty[2] = {true, true};  // a half not known to be zero
  int lfc_parity = 0;         // the half the next batch with fast-LFC evals uses
  bool collide_test = false; // KUEUE_TAS_CFG_CLASS_COLLIDE

  double trace[24] = {};  // the last chunk's host timeline (wall ms at fixed points, kueue_tas_last_host_trace)
  double host_ms[8] = {};  // last batch host time: compile, classes, enqueue, wait, pack+D2H, copy-out, [6] of compile:
                           // validation pass, [7] of compile: records + hashes pass
  int64_t last_stats[4] = {0, 0, 0, 0};  // fill evals, leaf-partial evals, fill launches, staged columns
  int64_t last_alias_fills = 0;          // fill rows whose sliceState aliases state (FillEvalParams::ss_alias)
  uint32_t fill_paths = 0;               // KUEUE_TAS_PATH_* bits of the last kueue_tas_eval_batch
  uint64_t eval_gen = 0;                 // kueue_tas_eval_batch calls so far (kueue_tas_eval_generation)
  // phase-1 counters of the last device chunk (kueue_tas_last_counters):
  // requests [chunk_base, chunk_base + chunk_rep.size()), their class counter rows
  size_t chunk_base = 0;
  std::vector<int32_t> chunk_rep;
  std::vector<uint8_t> chunk_leader;
  std::vector<uint8_t> chunk_alias;  // the class row's sliceState aliases state (FillEvalParams::ss_alias)
  std::vector<const kueue_tas_eval_req*> req_ptrs;  // kueue_tas_eval_batch's requests as kueue_tas_eval_batch_ptrs takes them
  // eval_chunk's per-request host work (kept between batches)
  std::vector<int64_t> req_term_off;
  std::vector<int32_t> req_chunk_maxt;
  std::vector<std::pair<size_t, std::string>> req_errs;
  std::vector<uint64_t> req_sig_hash, req_cls_hash;
  std::vector<uint8_t> req_fast, req_leaf;
  std::vector<int32_t> req_local_cls, part_map;
  std::vector<size_t> part_base;
  std::vector<PartClasses> part_cls;
  // (behind everything the evaluation path reads: that path's members keep their places)
  // kueue_tas_snapshot_digest: the blocks' partial rows, then the words and chunk words (one D2H);
  // kueue_tas_snapshot_read_leaves: the requested leaves and the gathered staging block (one D2H)
  DevBuf<uint64_t> d_digest;
  HostBuf<uint64_t> h_digest;
  DevBuf<int32_t> d_read_ids;
  DevBuf<uint8_t> d_read;
  HostBuf<uint8_t> h_read;
  hipEvent_t ev_digest[3] = {};  // before the launches, after them, after the D2H (kueue_tas_last_digest_ms)
  float digest_ms[2] = {0, 0};
  // resident removal tables (kueue_tas_removal_tables_build): the build's one
  // upload (target records | list entries | cand_off | set_off), the sets'
  // sorted tables, and the host's copy of what sizes an evaluation's range
  HostBuf<uint8_t> h_rt;
  DevBuf<uint8_t> d_rt;
  DevBuf<kueue_tas_assumed> d_rt_table;
  hipEvent_t ev_rt = nullptr;  // the upload's end (h_rt is rewritten by the next build)
  bool rt_built = false;
  int64_t rt_snap_gen = -1;    // n_loads + n_splices at the build: a load or splice since makes the tables stale
  size_t rt_set_off_at = 0;    // byte offset of set_off in d_rt
  std::vector<int32_t> rt_cand_off, rt_set_off;  // [sets + 1]
  std::vector<int32_t> rt_pos_kept;              // per list entry: its target's records with leaf >= 0
  int64_t rt_stats[4] = {0, 0, 0, 0};            // kueue_tas_removal_stats
  // large sets (KUEUE_TAS_RT_LARGE_SETS), allocated by the first build that has one: the merge
  // passes' two key buffers (a key per record of the large sets) and the segments' position prefixes
  DevBuf<uint64_t> d_rt_keys[2];
  DevBuf<int32_t> d_rt_seg_prefix;               // [segments of all large sets][64]
  std::vector<int32_t> rt_large_seg_off;         // per set: its first row of d_rt_seg_prefix, -1: a small set
  int64_t rt_large_stats[4] = {0, 0, 0, 0};      // kueue_tas_removal_large_stats
  // the chunk's masked evaluations (eval_chunk): each request's job (-1: none) and range length
  std::vector<int32_t> req_job, req_xlen;
};

// The leaf-row scatter kernels write repeated entries in no fixed order:
// the calls that take a leaf list require distinct leaves.
static bool distinct_leaves(const int32_t* leaves, size_t n) {
  std::vector<int32_t> sorted(leaves, leaves + n);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

static int fail(kueue_tas_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(c, x)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (x);                                                                    \
    if (e_ != hipSuccess)                                                                   \
      return fail(c, KUEUE_TAS_EDEVICE, std::string(#x) + ": " + hipGetErrorString(e_));    \
  } while (0)

extern "C" {

static double wall_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int kueue_tas_abi_version(void) { return KUEUE_TAS_ABI_VERSION; }

kueue_tas_ctx* kueue_tas_ctx_create(const kueue_tas_config* cfg) {
  DevBufLink* chain = nullptr;
  g_devbuf_chain = &chain;
  auto* c = new kueue_tas_ctx();
  g_devbuf_chain = nullptr;
  c->dev_bufs = chain;
  c->knobs = Knobs::from_env();
  if (cfg) {
    c->device = cfg->device;
    c->inline_stats = (cfg->flags & KUEUE_TAS_CFG_INLINE_STATS) != 0 || (cfg->flags & KUEUE_TAS_CFG_SPLIT_STATS) == 0;
    c->pair_fill = (cfg->flags & KUEUE_TAS_CFG_NO_PAIR_FILL) == 0;
    c->admit_window = (cfg->flags & KUEUE_TAS_CFG_SERIAL_ADMIT) == 0;
    c->fused_top = (cfg->flags & KUEUE_TAS_CFG_FUSED_TOP) != 0;
    c->cat_fill = (cfg->flags & KUEUE_TAS_CFG_NO_CATEGORY_FILL) == 0;
    c->collide_test = (cfg->flags & KUEUE_TAS_CFG_CLASS_COLLIDE) != 0;
    if (cfg->flags & KUEUE_TAS_CFG_LFC_IN_FILL) c->knobs.lfc_in_fill = true;
    if (cfg->list_cap > 0) {
      int lc = 64;
      while (lc < cfg->list_cap && lc < 1024) lc <<= 1;
      c->list_cap = lc;
    }
    if (cfg->max_batch > 0) c->max_batch = cfg->max_batch;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= c->device) {
    c->err = "no HIP device available";
    delete c;
    return nullptr;
  }
  // priorities: the main stream (fill -> roll-up -> BestFit select, the
  // critical path) and the fast-LFC branch high, the ExclusionStats branch
  // (off the critical path, a full-grid kernel beside select) low, so the
  // dispatcher hands CUs to select's workgroups first
  int prio_lo = 0, prio_hi = 0;
  if (hipSetDevice(c->device) != hipSuccess || hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, prio_hi) != hipSuccess ||
      hipStreamCreateWithPriority(&c->stream3, hipStreamNonBlocking, prio_lo) != hipSuccess) {
    delete c;
    return nullptr;
  }
  // the BestFit select launch declares more than 64 KiB of dynamic LDS
  // (kSelectWaves x kFinalWalkLds; a workgroup may use all 160 KiB of a CU)
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          kSelectWaves * std::max(kFinalWalkLds, c->list_cap * 16)) != hipSuccess) {
    c->err = "select_kernel dynamic LDS attribute";
    delete c;
    return nullptr;
  }
  // the batch's events order its streams and time its stages; the host never
  // reads memory through them (it synchronizes the streams), so no system-scope
  // release: ~1.4 us less device time per record (tools/micro/sync_cost.hip)
  for (auto& e : c->ev) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  for (auto& e : c->evl) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  for (auto& e : c->evs) (void)hipEventCreateWithFlags(&e, hipEventDisableSystemFence);
  return c;
}

void kueue_tas_ctx_destroy(kueue_tas_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  if (c->stream3) (void)hipStreamSynchronize(c->stream3);
  c->d_child_off.release();
  c->d_id_rank.release();
  c->d_taint_profile.release();
  c->d_labels.release();
  c->d_free.release();
  c->d_usage.release();
  c->d_free_present.release();
  c->d_usage_present.release();
  c->d_counters.release();
  c->d_res.release();
  c->h_res.release();
  c->h_res2.release();
  c->d_scratch.release();
  c->d_deltas.release();
  c->d_setfree.release();
  c->d_fits.release();
  c->d_fill_lim.release();
  c->d_parent.release();
  c->d_wave_tab.release();
  c->d_leaf_parent.release();
  c->d_names.release();
  c->d_name_off.release();
  c->d_enc_bytes.release();
  c->d_enc_stroff.release();
  c->d_enc_off.release();
  c->d_enc_ids.release();
  c->d_enc_counts.release();
  c->d_enc_same.release();
  c->d_enc_out.release();
  c->d_packed.release();
  c->d_partials.release();
  c->d_fill_stats.release();
  c->h_stage.release();
  c->d_stage.release();
  c->d_overlay.release();
  c->d_rack_pos.release();
  c->d_tags.release();
  c->d_lfc_ch.release();
  c->d_lfc_cp.release();
  c->d_lfc_tot.release();
  c->d_lfc_ovs.release();
  c->d_lfc_ovtot.release();
  c->d_lfc_u8.release();
  c->d_lfc_jobs.release();
  c->d_lfc_items.release();
  c->d_prof.release();
  c->d_level_max.release();
  if (c->ent_host) (void)hipHostFree(c->ent_host);
  c->ent_host = c->ent_dev = nullptr;
  if (c->tag_host) (void)hipHostFree(c->tag_host);
  c->tag_host = c->tag_dev = nullptr;
  c->d_leaf_tags.release();
  for (auto& e : c->ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->evl)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : c->evs)
    if (e) (void)hipEventDestroy(e);
  if (c->ev_deltas) (void)hipEventDestroy(c->ev_deltas);
  if (c->ev_rt) (void)hipEventDestroy(c->ev_rt);
  for (auto& e : c->ev_digest)
    if (e) (void)hipEventDestroy(e);
  if (c->stream3) (void)hipStreamDestroy(c->stream3);
  if (c->stream2) (void)hipStreamDestroy(c->stream2);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* kueue_tas_last_error(kueue_tas_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

static int load_impl(kueue_tas_ctx* c, const kueue_tas_snapshot_desc* d, const kueue_tas_splice_desc* sp);

int kueue_tas_snapshot_load(kueue_tas_ctx* c, const kueue_tas_snapshot_desc* d) { return load_impl(c, d, nullptr); }

int kueue_tas_snapshot_splice(kueue_tas_ctx* c, const kueue_tas_splice_desc* sp) {
  if (!c || !sp || !sp->topo || !sp->leaf_src) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  const kueue_tas_snapshot_desc* d = sp->topo;
  if (d->num_levels != c->snap.L || d->num_cols != c->snap.R || d->num_label_cols != c->snap.K ||
      d->lowest_is_hostname != c->snap.lowest_is_hostname)
    return fail(c, KUEUE_TAS_EINVAL, "splice: the tree's levels, columns and label columns stay");
  if (d->num_levels < 1 || d->num_levels > KUEUE_TAS_MAX_LEVELS) return fail(c, KUEUE_TAS_EINVAL, "num_levels");
  const int n_new = d->level_sizes[d->num_levels - 1];
  int fresh = 0;
  for (int j = 0; j < n_new; j++) {
    const int32_t x = sp->leaf_src[j];
    if (x >= c->snap.N || x < -1) return fail(c, KUEUE_TAS_EINVAL, "splice: leaf source out of range");
    fresh += x < 0 ? 1 : 0;
  }
  if (fresh != sp->num_new) return fail(c, KUEUE_TAS_EINVAL, "splice: num_new is not the count of joined leaves");
  if (sp->num_new > 0 && (!sp->new_free_capacity || !sp->new_tas_usage || !sp->new_free_present ||
                          !sp->new_usage_present || (c->snap.K > 0 && !sp->new_label_values)))
    return fail(c, KUEUE_TAS_EINVAL, "splice: joined rows missing");
  return load_impl(c, d, sp);
}

static int load_impl(kueue_tas_ctx* c, const kueue_tas_snapshot_desc* d, const kueue_tas_splice_desc* sp) {
  if (!c || !d) return KUEUE_TAS_EINVAL;
  if (d->num_levels < 1 || d->num_levels > KUEUE_TAS_MAX_LEVELS) return fail(c, KUEUE_TAS_EINVAL, "num_levels");
  if (d->num_cols < 0 || d->num_cols > KUEUE_TAS_MAX_COLS) return fail(c, KUEUE_TAS_EINVAL, "num_cols");
  HIPCHK(c, hipSetDevice(c->device));
  DevSnap s{};
  s.L = d->num_levels;
  s.R = d->num_cols;
  s.K = d->num_label_cols;
  s.lowest_is_hostname = d->lowest_is_hostname;
  int64_t off = 0;
  int maxD = 0;
  c->h_level_sizes.assign(d->level_sizes, d->level_sizes + s.L);
  for (int l = 0; l < s.L; l++) {  // level starts 16-byte aligned (vectorized leaf scans)
    s.level_size[l] = d->level_sizes[l];
    s.level_off[l] = int32_t(off);
    off += (int64_t(d->level_sizes[l]) + 3) / 4 * 4;
    maxD = std::max(maxD, d->level_sizes[l]);
  }
  s.level_off[s.L] = int32_t(off);
  s.SD = int32_t(off);
  s.N = d->level_sizes[s.L - 1];
  const size_t N = size_t(s.N);
  s.leaf_dead = nullptr;  // a load describes live leaves only
  s.leaf_tag = nullptr;   // leaf tags describe the previous leaves
  s.tag_out = nullptr;
  s.ent_base = nullptr;
  const bool tags_were_on = c->leaf_tags_on;
  // from here on the context's tables describe the new tree: a failure below
  // leaves it unloaded (every call then reports ENOSNAPSHOT) rather than
  // holding the old snapshot beside the new dead-leaf map
  c->loaded = false;
  c->leaf_tags_on = false;
  s.n_live = s.N;
  // a splice keeps the leaves that had left out: their flags move with them
  std::vector<uint8_t> old_dead;
  const int old_N = c->snap.N;
  if (sp) old_dead.swap(c->h_dead);
  c->h_dead.assign(N, 0);
  c->n_dead = 0;
  std::vector<int32_t>& gsrc = c->h_gsrc;  // (kept: no fresh pages per splice)
  if (sp) {  // sources (joined rows numbered in order) and the dead map, in the host pool's static parts
    gsrc.resize(N);
    ktas_pool::HostPool& pool = ktas_pool::HostPool::get();
    const size_t T = pool.parts();
    std::vector<int32_t> joined(T + 1, 0);
    std::vector<int64_t> dead(T, 0);
    auto part_of = [&](size_t b) {
      size_t t = 0;
      while (t + 1 < T && ktas_pool::HostPool::part_begin(N, t + 1, T) <= b) t++;
      return t;
    };
    pool.run_static(N, [&](size_t b, size_t e) {  // pass 1: joined rows per part
      int32_t k = 0;
      for (size_t j = b; j < e; j++) k += sp->leaf_src[j] < 0 ? 1 : 0;
      joined[part_of(b) + 1] = k;
    });
    for (size_t t = 0; t < T; t++) joined[t + 1] += joined[t];
    pool.run_static(N, [&](size_t b, size_t e) {  // pass 2: the numbering and the dead leaves
      const size_t t = part_of(b);
      int32_t k = joined[t];
      int64_t nd = 0;
      for (size_t j = b; j < e; j++) {
        const int32_t x = sp->leaf_src[j];
        gsrc[j] = x >= 0 ? x : -(++k);
        if (x >= 0 && size_t(x) < old_dead.size() && old_dead[size_t(x)]) {
          c->h_dead[j] = 1;
          nd++;
        }
      }
      dead[t] = nd;
    });
    for (int64_t nd : dead) c->n_dead += nd;
  }
  // the re-derived tables go up through one pinned arena (async copies, one
  // stream synchronization at the end) instead of a synchronous copy each
  HIPCHK(c, c->h_tab.reserve(size_t(off) * 8 + N * 9 + (N + 2) * 16 + 4096));
  size_t arena_pos = 0;
  auto stage = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    if (!bytes) return hipSuccess;
    if (arena_pos + bytes > c->h_tab.n) return hipErrorInvalidValue;  // (the bound above covers every table)
    memcpy(c->h_tab.p + arena_pos, src, bytes);
    const hipError_t e = hipMemcpyAsync(dst, c->h_tab.p + arena_pos, bytes, hipMemcpyHostToDevice, c->stream);
    arena_pos += (bytes + 255) / 256 * 256;
    return e;
  };
  // CSR offsets
  size_t nco = 0;
  for (int l = 0; l + 1 < s.L; l++) {
    s.child_base[l] = int32_t(nco);
    nco += size_t(d->level_sizes[l]) + 1;
  }
  c->level_maxfan.assign(size_t(s.L), 1);  // widest parent per level (select scratch bounds)
  for (int l = 0; l + 1 < s.L; l++) {
    const int32_t* co = d->child_offsets + s.child_base[l];
    int32_t f = 1;
    for (int p = 0; p < d->level_sizes[l]; p++) f = std::max(f, co[p + 1] - co[p]);
    c->level_maxfan[size_t(l)] = f;
  }
  HIPCHK(c, c->d_child_off.reserve(nco));
  if (nco) HIPCHK(c, hipMemcpyAsync(c->d_child_off.p, d->child_offsets, nco * 4, hipMemcpyHostToDevice, c->stream));
  s.child_off = c->d_child_off.p;
  if (sp) {  // the resident leaf columns gathered into the new numbering, the joined rows from the caller
    const int nn = std::max(sp->num_new, 1);
    const bool prof = c->snap.taint_profile != nullptr;
    const bool lab = s.K > 0 && c->snap.label_values != nullptr;
    const bool tags = tags_were_on && sp->new_leaf_tags != nullptr;
    HIPCHK(c, c->sp_free.reserve(size_t(s.R) * N));
    HIPCHK(c, c->sp_usage.reserve(size_t(s.R) * N));
    HIPCHK(c, c->sp_fp.reserve(N));
    HIPCHK(c, c->sp_up.reserve(N));
    if (prof) HIPCHK(c, c->sp_prof.reserve(N));
    if (lab) HIPCHK(c, c->sp_lab.reserve(size_t(s.K) * N));
    if (tags) HIPCHK(c, c->sp_tags.reserve(N));
    HIPCHK(c, c->sp_src.reserve(N));
    // the joined rows: free | usage | free_present | usage_present | profile | labels | tags
    const size_t o_u = size_t(s.R) * nn * 8, o_fp = 2 * o_u, o_up = o_fp + size_t(nn) * 4, o_pr = o_up + size_t(nn) * 4,
                 o_lb = o_pr + size_t(nn) * 4, o_tg = (o_lb + size_t(std::max(s.K, 1)) * nn * 4 + 7) / 8 * 8,
                 rbytes = o_tg + size_t(nn) * 8;
    HIPCHK(c, c->sp_rows.reserve(rbytes));
    // one pinned staging area: leaf sources, then the joined rows
    const size_t o_rows = (N * 4 + 255) / 256 * 256;
    HIPCHK(c, c->h_load.reserve(o_rows + rbytes));
    uint8_t* hl = c->h_load.p;
    if (N) memcpy(hl, gsrc.data(), N * 4);
    uint8_t* hr = hl + o_rows;
    if (sp->num_new > 0) {
      const size_t k = size_t(sp->num_new);
      if (s.R) {
        memcpy(hr, sp->new_free_capacity, size_t(s.R) * k * 8);
        memcpy(hr + o_u, sp->new_tas_usage, size_t(s.R) * k * 8);
      }
      memcpy(hr + o_fp, sp->new_free_present, k * 4);
      memcpy(hr + o_up, sp->new_usage_present, k * 4);
      if (prof && sp->new_taint_profile) memcpy(hr + o_pr, sp->new_taint_profile, k * 4);
      if (lab) memcpy(hr + o_lb, sp->new_label_values, size_t(s.K) * k * 4);
      if (tags) memcpy(hr + o_tg, sp->new_leaf_tags, k * 8);
      for (size_t i = 0; i < k; i++) {
        if (sp->new_taint_profile) c->num_profiles = std::max(c->num_profiles, sp->new_taint_profile[i] + 1);
        for (int q = 0; q < std::min(s.K, kStagedLabels) && sp->new_label_values; q++)
          if (uint32_t(sp->new_label_values[size_t(q) * k + i]) > 0xffffu) c->labels16 = false;
      }
    }
    if (N) HIPCHK(c, hipMemcpyAsync(c->sp_src.p, hl, N * 4, hipMemcpyHostToDevice, c->stream));
    if (sp->num_new > 0) HIPCHK(c, hipMemcpyAsync(c->sp_rows.p, hr, rbytes, hipMemcpyHostToDevice, c->stream));
    const uint8_t* rows = c->sp_rows.p;
    if (N) {
      hipLaunchKernelGGL(splice_leaves_kernel, dim3(unsigned((N + 255) / 256)), dim3(256), 0, c->stream, c->sp_src.p,
                         int(N), old_N, s.R, lab ? s.K : 0, nn, c->d_free.p, c->d_usage.p, c->d_free_present.p,
                         c->d_usage_present.p, prof ? c->d_taint_profile.p : nullptr, lab ? c->d_labels.p : nullptr,
                         reinterpret_cast<const int64_t*>(rows), reinterpret_cast<const int64_t*>(rows + o_u),
                         reinterpret_cast<const uint32_t*>(rows + o_fp), reinterpret_cast<const uint32_t*>(rows + o_up),
                         (prof && sp->new_taint_profile) ? reinterpret_cast<const int32_t*>(rows + o_pr) : nullptr,
                         reinterpret_cast<const int32_t*>(rows + o_lb), c->sp_free.p, c->sp_usage.p, c->sp_fp.p,
                         c->sp_up.p, prof ? c->sp_prof.p : nullptr, lab ? c->sp_lab.p : nullptr,
                         tags ? c->d_leaf_tags.p : nullptr, reinterpret_cast<const uint64_t*>(rows + o_tg),
                         tags ? c->sp_tags.p : nullptr);
      HIPCHK(c, hipGetLastError());
    }
    // the gathered columns go live; the previous ones become the next
    // splice's targets (stream order puts every later kernel after the gather)
    c->d_free.swap(c->sp_free);
    c->d_usage.swap(c->sp_usage);
    c->d_free_present.swap(c->sp_fp);
    c->d_usage_present.swap(c->sp_up);
    if (prof) c->d_taint_profile.swap(c->sp_prof);
    if (lab) c->d_labels.swap(c->sp_lab);
    if (tags) c->d_leaf_tags.swap(c->sp_tags);
    c->leaf_tags_on = tags;
    s.free_cap = c->d_free.p;
    s.tas_usage = c->d_usage.p;
    s.free_present = c->d_free_present.p;
    s.usage_present = c->d_usage_present.p;
    s.taint_profile = prof ? c->d_taint_profile.p : nullptr;
    s.label_values = lab ? c->d_labels.p : nullptr;
    if (c->n_dead > 0) {  // the leaves that had left, at their new indices
      HIPCHK(c, c->d_dead.reserve(N));
      HIPCHK(c, stage(c->d_dead.p, c->h_dead.data(), N));
      s.leaf_dead = c->d_dead.p;
      s.n_live = int32_t(int64_t(N) - c->n_dead);
    }
  } else {  // (leaf columns with headroom: a later splice's gather targets then fit without a reallocation)
  HIPCHK(c, c->d_free.reserve(size_t(s.R) * N));
  HIPCHK(c, c->d_usage.reserve(size_t(s.R) * N));
  if (s.R && N) {
    HIPCHK(c, hipMemcpyAsync(c->d_free.p, d->free_capacity, size_t(s.R) * N * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_usage.p, d->tas_usage, size_t(s.R) * N * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, c->d_free_present.reserve(N));
  HIPCHK(c, c->d_usage_present.reserve(N));
  if (N) {
    HIPCHK(c, hipMemcpyAsync(c->d_free_present.p, d->free_present, N * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_usage_present.p, d->usage_present, N * 4, hipMemcpyHostToDevice, c->stream));
  }
  s.free_cap = c->d_free.p;
  s.tas_usage = c->d_usage.p;
  s.free_present = c->d_free_present.p;
  s.usage_present = c->d_usage_present.p;
  s.taint_profile = nullptr;
  c->num_profiles = 1;
  if (d->taint_profile && N) {
    for (size_t i = 0; i < N; i++) c->num_profiles = std::max(c->num_profiles, d->taint_profile[i] + 1);
    HIPCHK(c, c->d_taint_profile.reserve(N));
    HIPCHK(c, hipMemcpyAsync(c->d_taint_profile.p, d->taint_profile, N * 4, hipMemcpyHostToDevice, c->stream));
    s.taint_profile = c->d_taint_profile.p;
  }
  s.label_values = nullptr;
  c->labels16 = true;
  for (int k = 0; k < std::min(s.K, kStagedLabels) && d->label_values; k++)
    for (size_t i = 0; i < N && c->labels16; i++) c->labels16 = uint32_t(d->label_values[size_t(k) * N + i]) <= 0xffffu;
  if (s.K > 0 && d->label_values && N) {
    HIPCHK(c, c->d_labels.reserve(size_t(s.K) * N));
    HIPCHK(c, hipMemcpyAsync(c->d_labels.p, d->label_values, size_t(s.K) * N * 4, hipMemcpyHostToDevice, c->stream));
    s.label_values = c->d_labels.p;
  }
  }
  s.id_rank = nullptr;
  if (d->domain_id_rank && off) {  // re-laid out on the padded level offsets, in the pinned arena itself
    HIPCHK(c, c->d_id_rank.reserve(size_t(off)));
    const size_t bytes = size_t(off) * 4;
    if (arena_pos + bytes > c->h_tab.n) return fail(c, KUEUE_TAS_EINVAL, "load: staging arena");
    int32_t* ranks = reinterpret_cast<int32_t*>(c->h_tab.p + arena_pos);
    int64_t src = 0;
    for (int l = 0; l < s.L; l++) {
      const int32_t b = s.level_off[l], sz = d->level_sizes[l];
      memcpy(ranks + b, d->domain_id_rank + src, size_t(sz) * 4);
      for (int32_t i = b + sz; i < s.level_off[l + 1]; i++) ranks[i] = 0;
      src += sz;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_id_rank.p, ranks, bytes, hipMemcpyHostToDevice, c->stream));
    arena_pos += (bytes + 255) / 256 * 256;
    s.id_rank = c->d_id_rank.p;
  }
  // leaves' parents with a uniform power-of-two fan-out F <= 64 in leaf order:
  // the staged fill rolls them up itself (one wave holds whole parents)
  c->rack_fanout = 0;
  if (s.L >= 2 && d->level_sizes[s.L - 2] > 0 && d->child_offsets) {
    const int P = d->level_sizes[s.L - 2];
    const int F = s.N / P;
    if (F > 0 && F <= kWave && (F & (F - 1)) == 0 && int64_t(F) * P == s.N) {
      const int32_t* co = d->child_offsets + s.child_base[s.L - 2];
      bool ok = true;
      for (int p = 0; p <= P && ok; p++) ok = co[p] == p * F;
      if (ok) c->rack_fanout = F;
    }
  }
  // otherwise, parents of at most 64 leaves: pack whole parents into waves
  // (first fit in leaf order) so the fill still rolls them up in the wave
  s.wave_tab = nullptr;
  s.n_wave_slots = 0;
  s.leaf_parent = nullptr;
  s.wave_tab2 = nullptr;
  s.n_wave_slots2 = 0;
  s.ragged_max_fan = 0;
  s.wide_parents = nullptr;
  s.n_wide = 0;
  // and the same packing into 128-leaf slots for fill_pair_kernel's two
  // leaves per lane (parents of at most 128 leaves; a wider parent takes
  // slots of its own, one per 128-leaf piece, flagged wide)
  if (c->rack_fanout == 0 && s.L >= 2 && d->level_sizes[s.L - 2] > 0 && d->child_offsets && s.N > 0) {
    const int P = d->level_sizes[s.L - 2];
    const int32_t* co = d->child_offsets + s.child_base[s.L - 2];
    bool ok = co[0] == 0 && co[P] == s.N;
    std::vector<int2> tab;
    std::vector<int32_t> wide;
    int cb = 0, cn = 0, fmax = 0;
    for (int p = 0; p < P && ok; p++) {
      const int f = co[p + 1] - co[p];
      if (f < 1) {
        ok = false;
        break;
      }
      fmax = std::max(fmax, f);
      if (f > 2 * kWave) {  // pieces of their own
        if (cn) tab.push_back(make_int2(cb, cn));
        for (int k = co[p]; k < co[p + 1]; k += 2 * kWave)
          tab.push_back(make_int2(k, std::min(2 * kWave, co[p + 1] - k) | (1 << 16)));
        wide.push_back(p);
        cb = co[p + 1];
        cn = 0;
        continue;
      }
      if (cn + f > 2 * kWave) {
        tab.push_back(make_int2(cb, cn));
        cb = co[p];
        cn = 0;
      }
      cn += f;
    }
    if (ok) {
      if (cn) tab.push_back(make_int2(cb, cn));
      if (!wide.empty()) {
        HIPCHK(c, c->d_wide.reserve(wide.size()));
        HIPCHK(c, stage(c->d_wide.p, wide.data(), wide.size() * 4));
        s.wide_parents = c->d_wide.p;
        s.n_wide = int32_t(wide.size());
      }
      HIPCHK(c, c->d_wave_tab2.reserve(tab.size()));
      HIPCHK(c, stage(c->d_wave_tab2.p, tab.data(), tab.size() * sizeof(int2)));
      HIPCHK(c, c->d_leaf_parent.reserve(N));  // (domain_parents_kernel below)
      s.wave_tab2 = c->d_wave_tab2.p;
      s.n_wave_slots2 = int32_t(tab.size());
      s.leaf_parent = c->d_leaf_parent.p;
      s.ragged_max_fan = fmax;
    }
  }
  if (c->rack_fanout == 0 && s.L >= 2 && d->level_sizes[s.L - 2] > 0 && d->child_offsets && s.N > 0) {
    const int P = d->level_sizes[s.L - 2];
    const int32_t* co = d->child_offsets + s.child_base[s.L - 2];
    bool ok = co[0] == 0 && co[P] == s.N;
    std::vector<int2> tab;
    int cb = 0, cn = 0;
    for (int p = 0; p < P && ok; p++) {
      const int f = co[p + 1] - co[p];
      if (f < 1 || f > kWave) {
        ok = false;
        break;
      }
      if (cn + f > kWave) {
        tab.push_back(make_int2(cb, cn));
        cb = co[p];
        cn = 0;
      }
      cn += f;
    }
    if (ok) {
      tab.push_back(make_int2(cb, cn));
      HIPCHK(c, c->d_wave_tab.reserve(tab.size()));
      HIPCHK(c, stage(c->d_wave_tab.p, tab.data(), tab.size() * sizeof(int2)));
      HIPCHK(c, c->d_leaf_parent.reserve(N));
      s.wave_tab = c->d_wave_tab.p;
      s.n_wave_slots = int32_t(tab.size());
      s.leaf_parent = c->d_leaf_parent.p;
      c->rack_fanout = -1;
    }
  }
  // parent global domain id of every domain (v1beta2 leaf-mode encoder) and
  // the ragged fills' leaf parents, derived on the device from the offsets
  // just uploaded (no O(N) host pass or upload per load / splice)
  HIPCHK(c, c->d_parent.reserve(size_t(std::max<int64_t>(off, 1))));
  if (off > 0) {
    hipLaunchKernelGGL(domain_parents_kernel, dim3(unsigned((off + 255) / 256)), dim3(256), 0, c->stream, s,
                       c->d_parent.p, s.leaf_parent ? c->d_leaf_parent.p : nullptr);
    HIPCHK(c, hipGetLastError());
  }
  c->names_loaded = false;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->snap = s;
  c->maxD = maxD;
  c->loaded = true;
  (sp ? c->n_splices : c->n_loads)++;
  return KUEUE_TAS_OK;
}

int kueue_tas_device_bytes(kueue_tas_ctx* c, int64_t* total, int64_t* phase2) {
  if (!c) return KUEUE_TAS_EINVAL;
  int64_t t = 0;
  for (const DevBufLink* b = c->dev_bufs; b; b = b->next) t += int64_t(b->bytes);
  if (total) *total = t;
  if (phase2) *phase2 = int64_t(c->d_counters.bytes + c->d_overlay.bytes + c->d_tags.bytes + c->d_scratch.bytes);
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_counters(kueue_tas_ctx* c, int64_t* loads, int64_t* splices) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (loads) *loads = c->n_loads;
  if (splices) *splices = c->n_splices;
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_load_names(kueue_tas_ctx* c, const char* bytes, size_t nbytes, const int64_t* offsets) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!offsets || (nbytes && !bytes)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  size_t total = 0;
  for (int l = 0; l < c->snap.L; l++) total += size_t(c->snap.level_size[l]);
  if (offsets[0] != 0 || size_t(offsets[total]) != nbytes) return fail(c, KUEUE_TAS_EINVAL, "name offsets");
  for (size_t i = 0; i < total; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, KUEUE_TAS_EINVAL, "name offsets not monotone");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_names.ensure(nbytes));
  HIPCHK(c, c->d_name_off.ensure(total + 1));
  if (nbytes) HIPCHK(c, hipMemcpy(c->d_names.p, bytes, nbytes, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(c->d_name_off.p, offsets, (total + 1) * 8, hipMemcpyHostToDevice));
  c->names_loaded = true;
  return KUEUE_TAS_OK;
}

static int run_encode(kueue_tas_ctx* c, EncodeArgs& a, size_t n_assign, kueue_tas_level_enc* out, int32_t* same) {
  const size_t nout = n_assign * size_t(a.num_levels);
  HIPCHK(c, c->d_enc_out.ensure(nout));
  HIPCHK(c, c->d_enc_same.ensure(n_assign));
  a.out = c->d_enc_out.p;
  a.same = c->d_enc_same.p;
  a.n_assign = int32_t(n_assign);
  hipLaunchKernelGGL(encode_v1beta2_kernel, dim3(unsigned(n_assign), unsigned(a.num_levels)), dim3(256), 0, c->stream,
                     a);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, a.out, nout * sizeof(kueue_tas_level_enc), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(same, a.same, n_assign * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KUEUE_TAS_OK;
}

int kueue_tas_encode_v1beta2(kueue_tas_ctx* c, const char* bytes, size_t nbytes, const int64_t* str_off,
                             size_t num_strings, const int32_t* ids, const int32_t* counts, const int64_t* off,
                             size_t n_assign, int32_t num_levels, kueue_tas_level_enc* out, int32_t* same_counts) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (n_assign == 0) return KUEUE_TAS_OK;
  if (num_levels < 1 || num_levels > 65535 || !str_off || !off || !out || !same_counts || (nbytes && !bytes))
    return fail(c, KUEUE_TAS_EINVAL, "encode arguments");
  if (n_assign > 0x7fffffff) return fail(c, KUEUE_TAS_EINVAL, "too many assignments");
  // host-side shape checks: every id and offset the kernel will touch
  if (off[0] < 0) return fail(c, KUEUE_TAS_EINVAL, "assignment offsets");
  for (size_t i = 0; i < n_assign; i++)
    if (off[i + 1] < off[i]) return fail(c, KUEUE_TAS_EINVAL, "assignment offsets not monotone");
  const size_t ndom = size_t(off[n_assign]);
  if (ndom && (!ids || !counts)) return fail(c, KUEUE_TAS_EINVAL, "null ids/counts");
  if (str_off[0] < 0 || size_t(str_off[num_strings]) > nbytes) return fail(c, KUEUE_TAS_EINVAL, "string offsets");
  for (size_t i = 0; i < num_strings; i++)
    if (str_off[i + 1] < str_off[i]) return fail(c, KUEUE_TAS_EINVAL, "string offsets not monotone");
  for (size_t i = 0; i < ndom * size_t(num_levels); i++)
    if (ids[i] < 0 || size_t(ids[i]) >= num_strings) return fail(c, KUEUE_TAS_EINVAL, "string id out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_enc_bytes.ensure(nbytes));
  HIPCHK(c, c->d_enc_stroff.ensure(num_strings + 1));
  HIPCHK(c, c->d_enc_off.ensure(n_assign + 1));
  HIPCHK(c, c->d_enc_ids.ensure(ndom * size_t(num_levels)));
  HIPCHK(c, c->d_enc_counts.ensure(ndom));
  if (nbytes) HIPCHK(c, hipMemcpyAsync(c->d_enc_bytes.p, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_enc_stroff.p, str_off, (num_strings + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_enc_off.p, off, (n_assign + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (ndom) {
    HIPCHK(c, hipMemcpyAsync(c->d_enc_ids.p, ids, ndom * size_t(num_levels) * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_enc_counts.p, counts, ndom * 4, hipMemcpyHostToDevice, c->stream));
  }
  EncodeArgs a{};
  a.bytes = c->d_enc_bytes.p;
  a.str_off = c->d_enc_stroff.p;
  a.ids = c->d_enc_ids.p;
  a.counts = c->d_enc_counts.p;
  a.off = c->d_enc_off.p;
  a.num_levels = num_levels;
  return run_encode(c, a, n_assign, out, same_counts);
}

int kueue_tas_encode_v1beta2_leaves(kueue_tas_ctx* c, const int32_t* pairs, const int64_t* off, size_t n_assign,
                                    int32_t first_level, kueue_tas_level_enc* out, int32_t* same_counts) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!c->names_loaded) return fail(c, KUEUE_TAS_EINVAL, "no names loaded (kueue_tas_snapshot_load_names)");
  if (n_assign == 0) return KUEUE_TAS_OK;
  const DevSnap& s = c->snap;
  if (first_level < 0 || first_level >= s.L || !off || !out || !same_counts)
    return fail(c, KUEUE_TAS_EINVAL, "encode arguments");
  if (n_assign > 0x7fffffff) return fail(c, KUEUE_TAS_EINVAL, "too many assignments");
  if (off[0] < 0) return fail(c, KUEUE_TAS_EINVAL, "assignment offsets");
  for (size_t i = 0; i < n_assign; i++)
    if (off[i + 1] < off[i]) return fail(c, KUEUE_TAS_EINVAL, "assignment offsets not monotone");
  const size_t npairs = size_t(off[n_assign]);
  if (npairs && !pairs) return fail(c, KUEUE_TAS_EINVAL, "null pairs");
  for (size_t j = size_t(off[0]); j < npairs; j++)
    if (pairs[2 * j] < 0 || pairs[2 * j] >= s.N) return fail(c, KUEUE_TAS_EINVAL, "leaf out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_enc_counts.ensure(2 * npairs));  // the pairs
  HIPCHK(c, c->d_enc_off.ensure(n_assign + 1));
  if (npairs)
    HIPCHK(c, hipMemcpyAsync(c->d_enc_counts.p, pairs, npairs * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_enc_off.p, off, (n_assign + 1) * 8, hipMemcpyHostToDevice, c->stream));
  EncodeArgs a{};
  a.bytes = c->d_names.p;
  a.str_off = c->d_name_off.p;
  a.pairs = c->d_enc_counts.p;
  a.parent = c->d_parent.p;
  a.off = c->d_enc_off.p;
  a.num_levels = s.L - first_level;
  a.first_level = first_level;
  a.L = s.L;
  int64_t base = 0;
  for (int l = 0; l < s.L; l++) {
    a.level_off[l] = s.level_off[l];
    a.name_base[l] = base;
    base += s.level_size[l];
  }
  return run_encode(c, a, n_assign, out, same_counts);
}

static int apply_deltas_impl(kueue_tas_ctx* c, const kueue_tas_delta* deltas, size_t n,
                             const uint32_t* usage_present_or_null, bool mirrored);
int kueue_tas_snapshot_apply_deltas(kueue_tas_ctx* c, const kueue_tas_delta* deltas, size_t n,
                                    const uint32_t* usage_present_or_null) {
  return apply_deltas_impl(c, deltas, n, usage_present_or_null, false);
}
int kueue_tas_snapshot_apply_deltas_mirrored(kueue_tas_ctx* c, const kueue_tas_delta* deltas, size_t n) {
  return apply_deltas_impl(c, deltas, n, nullptr, true);
}
static int apply_deltas_impl(kueue_tas_ctx* c, const kueue_tas_delta* deltas, size_t n,
                             const uint32_t* usage_present_or_null, bool mirrored) {
  if (!c || !c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot");
  HIPCHK(c, hipSetDevice(c->device));
  if (n) {
    // the records through pinned staging: an async copy, no stream sync (the
    // launches that read the usage follow on the same stream); the previous
    // call's copy must be done before its buffer is rewritten
    if (c->ev_deltas) HIPCHK(c, hipEventSynchronize(c->ev_deltas));
    else HIPCHK(c, hipEventCreateWithFlags(&c->ev_deltas, hipEventDisableTiming));
    HIPCHK(c, c->h_deltas.reserve(n));
    // range check and copy in one pass (a whole batch's admission is ~16k
    // records: over the host pool's static parts when large)
    const int32_t N = c->snap.N, R = c->snap.R;
    kueue_tas_delta* dst = c->h_deltas.p;
    std::atomic<bool> bad{false};
    auto check_copy = [&](size_t i0, size_t i1) {
      bool ok = true;
      for (size_t i = i0; i < i1; i++) {
        const kueue_tas_delta x = deltas[i];
        ok &= x.leaf >= 0 && x.leaf < N && x.col >= 0 && x.col < R;
        dst[i] = x;
      }
      if (!ok) bad.store(true, std::memory_order_relaxed);
    };
    if (n >= 8192) ktas_pool::HostPool::get().run_static(n, check_copy);
    else check_copy(0, n);
    if (bad.load()) return fail(c, KUEUE_TAS_EINVAL, "delta out of range");
    HIPCHK(c, c->d_deltas.ensure(n));
    HIPCHK(c, hipMemcpyAsync(c->d_deltas.p, c->h_deltas.p, n * sizeof(kueue_tas_delta), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_deltas, c->stream));
    int blocks = int((n + 255) / 256);
    const bool sh = mirrored && c->shadow_ok;  // no shadow yet: the next mark copies the usage whole
    hipLaunchKernelGGL(apply_deltas_kernel, dim3(blocks), dim3(256), 0, c->stream, c->d_usage.p, c->d_usage_present.p,
                       c->snap.N, c->d_deltas.p, int(n), sh ? c->d_ushadow.p : nullptr,
                       sh ? c->d_pshadow.p : nullptr);
    HIPCHK(c, hipGetLastError());
  }
  if (usage_present_or_null) {
    HIPCHK(c, hipMemcpyAsync(c->d_usage_present.p, usage_present_or_null, size_t(c->snap.N) * 4, hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the caller's array)
  }
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_usage_mark(kueue_tas_ctx* c) {
  if (!c || !c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t N = size_t(c->snap.N), R = size_t(c->snap.R);
  HIPCHK(c, c->d_ushadow.reserve(N * R));  // (headroom: splices grow N a few leaves at a time)
  HIPCHK(c, c->d_pshadow.reserve(N));
  if (N * R) HIPCHK(c, hipMemcpyAsync(c->d_ushadow.p, c->d_usage.p, N * R * 8, hipMemcpyDeviceToDevice, c->stream));
  if (N) HIPCHK(c, hipMemcpyAsync(c->d_pshadow.p, c->d_usage_present.p, N * 4, hipMemcpyDeviceToDevice, c->stream));
  c->shadow_ok = true;
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_usage_changes(kueue_tas_ctx* c, const kueue_tas_delta** changes, size_t* n) {
  if (!c || !changes || !n) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot");
  if (!c->shadow_ok) return fail(c, KUEUE_TAS_EINVAL, "usage_changes before usage_mark");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t N = size_t(c->snap.N), R = size_t(c->snap.R);
  HIPCHK(c, c->d_uchg.ensure(std::max<size_t>(N * R, 1)));
  HIPCHK(c, c->d_uchg_n.ensure(1));
  HIPCHK(c, c->h_uchg_n.ensure(1));
  HIPCHK(c, hipMemsetAsync(c->d_uchg_n.p, 0, 4, c->stream));
  if (N * R) {
    hipLaunchKernelGGL(usage_diff_kernel, dim3(unsigned((N * R + 255) / 256)), dim3(256), 0, c->stream, c->d_usage.p,
                       c->d_usage_present.p, c->d_ushadow.p, c->d_pshadow.p, int(N), int(R), c->d_uchg.p, c->d_uchg_n.p);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(c->h_uchg_n.p, c->d_uchg_n.p, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const size_t k = size_t(c->h_uchg_n.p[0]);
  c->uchg.resize(k);
  if (k) HIPCHK(c, hipMemcpy(c->uchg.data(), c->d_uchg.p, k * sizeof(kueue_tas_delta), hipMemcpyDeviceToHost));
  *changes = c->uchg.data();
  *n = k;
  return kueue_tas_snapshot_usage_mark(c);
}

int kueue_tas_snapshot_set_free(kueue_tas_ctx* c, const int32_t* leaves, size_t n, const int64_t* rows,
                                const uint32_t* free_present) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (n == 0) return KUEUE_TAS_OK;
  if (!leaves || !rows || !free_present) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  for (size_t i = 0; i < n; i++)
    if (leaves[i] < 0 || leaves[i] >= c->snap.N) return fail(c, KUEUE_TAS_EINVAL, "set_free leaf out of range");
  if (!distinct_leaves(leaves, n)) return fail(c, KUEUE_TAS_EINVAL, "repeated leaf in set_free");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t R = size_t(c->snap.R);
  const size_t rows_off = (n * 4 + 7) / 8 * 8;
  const size_t pres_off = rows_off + n * R * 8;
  HIPCHK(c, c->d_setfree.ensure(pres_off + n * 4));
  uint8_t* d = c->d_setfree.p;
  HIPCHK(c, hipMemcpyAsync(d, leaves, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + rows_off, rows, n * R * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + pres_off, free_present, n * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(set_free_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream, c->d_free.p,
                     c->d_free_present.p, c->snap.N, c->snap.R, reinterpret_cast<const int32_t*>(d),
                     reinterpret_cast<const int64_t*>(d + rows_off), reinterpret_cast<const uint32_t*>(d + pres_off),
                     int(n));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_set_leaf_live(kueue_tas_ctx* c, const int32_t* leaves, size_t n, const int32_t* live) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (n == 0) return KUEUE_TAS_OK;
  if (!leaves || !live) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  for (size_t i = 0; i < n; i++)
    if (leaves[i] < 0 || leaves[i] >= c->snap.N) return fail(c, KUEUE_TAS_EINVAL, "leaf out of range");
  if (!distinct_leaves(leaves, n)) return fail(c, KUEUE_TAS_EINVAL, "repeated leaf in set_leaf_live");
  for (size_t i = 0; i < n; i++) {
    const uint8_t d = live[i] ? 0 : 1;
    c->n_dead += int64_t(d) - int64_t(c->h_dead[size_t(leaves[i])]);
    c->h_dead[size_t(leaves[i])] = d;
  }
  HIPCHK(c, hipSetDevice(c->device));
  c->snap.n_live = int32_t(int64_t(c->snap.N) - c->n_dead);
  const bool was_dense = c->snap.leaf_dead != nullptr;
  if (c->n_dead == 0) {
    c->snap.leaf_dead = nullptr;
    return KUEUE_TAS_OK;
  }
  std::vector<int32_t> lv;  // read by the async copy: lives until the synchronize below
  if (!was_dense) {  // first dead leaf: the whole map (the device copy was dropped while all leaves lived)
    HIPCHK(c, c->d_dead.reserve(size_t(c->snap.N)));
    HIPCHK(c, hipMemcpyAsync(c->d_dead.p, c->h_dead.data(), size_t(c->snap.N), hipMemcpyHostToDevice, c->stream));
  } else {  // scatter the changed leaves
    lv.resize(2 * n);
    for (size_t i = 0; i < n; i++) lv[2 * i] = leaves[i], lv[2 * i + 1] = live[i] ? 1 : 0;
    HIPCHK(c, c->d_setfree.ensure(lv.size() * 4));
    HIPCHK(c, hipMemcpyAsync(c->d_setfree.p, lv.data(), lv.size() * 4, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(set_leaf_dead_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream, c->d_dead.p,
                       reinterpret_cast<const int32_t*>(c->d_setfree.p), int(n));
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->snap.leaf_dead = c->d_dead.p;
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_set_leaf_attrs(kueue_tas_ctx* c, const int32_t* leaves, size_t n, const int32_t* profiles,
                                      const int32_t* labels) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (n == 0) return KUEUE_TAS_OK;
  if (!leaves || !profiles) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  const size_t K = size_t(c->snap.K);
  if (K && !labels) return fail(c, KUEUE_TAS_EINVAL, "labels required (snapshot has label columns)");
  if (!c->snap.taint_profile) return fail(c, KUEUE_TAS_EINVAL, "snapshot has no taint profiles");
  for (size_t i = 0; i < n; i++) {
    if (leaves[i] < 0 || leaves[i] >= c->snap.N) return fail(c, KUEUE_TAS_EINVAL, "leaf out of range");
    if (profiles[i] < 0) return fail(c, KUEUE_TAS_EINVAL, "negative taint profile");
  }
  if (!distinct_leaves(leaves, n)) return fail(c, KUEUE_TAS_EINVAL, "repeated leaf in set_leaf_attrs");
  HIPCHK(c, hipSetDevice(c->device));
  for (size_t i = 0; i < n; i++) c->num_profiles = std::max(c->num_profiles, profiles[i] + 1);
  for (size_t i = 0; i < n && K; i++)  // the packed nodeSelector compare needs 16-bit staged ids
    for (size_t k = 0; k < std::min<size_t>(K, size_t(kStagedLabels)); k++)
      if (uint32_t(labels[i * K + k]) > 0xffffu) c->labels16 = false;
  const size_t prof_off = n * 4, lab_off = 2 * n * 4;
  HIPCHK(c, c->d_setfree.ensure(lab_off + n * K * 4));
  uint8_t* d = c->d_setfree.p;
  HIPCHK(c, hipMemcpyAsync(d, leaves, n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d + prof_off, profiles, n * 4, hipMemcpyHostToDevice, c->stream));
  if (K) HIPCHK(c, hipMemcpyAsync(d + lab_off, labels, n * K * 4, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(set_leaf_attrs_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream,
                     c->d_taint_profile.p, K ? c->d_labels.p : nullptr, c->snap.N, c->snap.K,
                     reinterpret_cast<const int32_t*>(d), reinterpret_cast<const int32_t*>(d + prof_off),
                     reinterpret_cast<const int32_t*>(d + lab_off), int(n));
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KUEUE_TAS_OK;
}

int kueue_tas_fits(kueue_tas_ctx* c, const kueue_tas_fits_req* reqs, size_t n, const kueue_tas_fits_term* terms,
                   size_t num_terms, int32_t* fits) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (n == 0) return KUEUE_TAS_OK;
  if (!reqs || !fits || (num_terms && !terms)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  for (size_t i = 0; i < n; i++) {
    const kueue_tas_fits_req& r = reqs[i];
    if (r.leaf >= c->snap.N || r.num_terms < 0 || r.term_begin < 0 ||
        size_t(r.term_begin) + size_t(r.num_terms) > num_terms)
      return fail(c, KUEUE_TAS_EINVAL, "fits request out of range");
    for (int k = 0; k < r.num_terms; k++)
      if (terms[r.term_begin + k].col >= c->snap.R) return fail(c, KUEUE_TAS_EINVAL, "fits term column out of range");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = n * sizeof(kueue_tas_fits_req) + num_terms * sizeof(kueue_tas_fits_term) + n * 4;
  HIPCHK(c, c->d_fits.ensure(bytes));
  uint8_t* d = c->d_fits.p;
  auto* d_reqs = reinterpret_cast<kueue_tas_fits_req*>(d);
  auto* d_terms = reinterpret_cast<kueue_tas_fits_term*>(d + n * sizeof(kueue_tas_fits_req));
  auto* d_out = reinterpret_cast<int32_t*>(d + n * sizeof(kueue_tas_fits_req) + num_terms * sizeof(kueue_tas_fits_term));
  HIPCHK(c, hipMemcpyAsync(d_reqs, reqs, n * sizeof(kueue_tas_fits_req), hipMemcpyHostToDevice, c->stream));
  if (num_terms)
    HIPCHK(c, hipMemcpyAsync(d_terms, terms, num_terms * sizeof(kueue_tas_fits_term), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(fits_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream, c->snap, d_reqs, int(n),
                     d_terms, d_out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(fits, d_out, n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KUEUE_TAS_OK;
}

static size_t admit_al(size_t b) { return (b + 255) / 256 * 256; }
// kueue_tas_admit's device buffer (c->d_fits): the uploaded part [0, up_bytes)
// (records, terms, workload offsets, record -> workload, phase-1 flags, the
// exact flag, the per-column totals), then the verdicts (+ diagnostics), the
// phase-1 records, the window kernel's lists, the per-leaf minima, the touched
// bitmap and the window phases' state.
struct AdmitLayout {
  size_t o_terms, o_off, o_recwl, o_fit0, o_exact, o_total, up_bytes;
  size_t o_out, o_recs, o_dep, o_todo, o_todor, o_minc, o_bits, o_state, end;
};
static AdmitLayout admit_layout(size_t n, size_t num_terms, size_t n_wl, size_t N) {
  AdmitLayout L{};
  L.o_terms = admit_al(n * sizeof(kueue_tas_fits_req));
  L.o_off = L.o_terms + admit_al(num_terms * sizeof(kueue_tas_fits_term));
  L.o_recwl = L.o_off + admit_al((n_wl + 1) * 8);
  L.o_fit0 = L.o_recwl + admit_al(n * 4);
  L.o_exact = L.o_fit0 + admit_al(n_wl * 4);
  L.o_total = L.o_exact + 256;
  L.up_bytes = L.o_total + KUEUE_TAS_MAX_COLS * 8;
  L.o_out = admit_al(L.up_bytes);
  L.o_recs = L.o_out + admit_al((n_wl + 3) * 4);  // + three diagnostics words (admit_window_kernel)
  L.o_dep = L.o_recs + admit_al(n * sizeof(AdmitRec));
  L.o_todo = L.o_dep + admit_al(n_wl * 4);
  L.o_todor = L.o_todo + admit_al((n_wl + 1) * 4);
  L.o_minc = L.o_todor + admit_al(n_wl * 16);
  L.o_bits = L.o_minc + admit_al(N * 4);
  L.o_state = L.o_bits + admit_al((N + 31) / 32 * 4);  // admit_window_kernel's phase state (AdmitState)
  L.end = L.o_state + 256;
  return L;
}
static int admit_run(kueue_tas_ctx* c, const AdmitLayout& L, uint8_t* d, const kueue_tas_fits_term* d_terms, size_t n,
                     size_t n_wl, int32_t pods_col, bool exact);
// The arrays one pass reads and writes per record and per workload.
struct AdmitView {
  const kueue_tas_fits_req* reqs;  // [n]
  const int32_t* recwl;            // [n] record -> workload
  const int64_t* off;              // [n_wl + 1] workload -> records
  int32_t* fit0;                   // [n_wl] phase-1 flags, 1 on entry
  int32_t* out;                    // [n_wl + 3] verdicts + diagnostics
  AdmitRec* recs;                  // [n]
  int32_t* dep;                    // [n_wl]
};
static int admit_run_view(kueue_tas_ctx* c, const AdmitLayout& L, uint8_t* d, const AdmitView& v,
                          const kueue_tas_fits_term* d_terms, size_t n, size_t n_wl, int32_t pods_col, bool exact);

// kueue_tas_admit_targets' extra arguments (null: kueue_tas_admit).
struct AdmitTargets {
  const kueue_tas_delta* deltas;  // the preemptable workloads' usage records
  const int64_t* off;             // [T + 1] CSR into deltas
  size_t T;
  const int32_t* ids;             // the entries' target lists
  const int64_t* eoff;            // [n_wl + 1] CSR into ids
};
// One stretch of the ordered entry list: a run of target-free entries for the
// pass (admit_run_view), or entries for admit_step_kernel.
struct AdmitSeg {
  bool pass;
  size_t a, b;
};
static int admit_targets_run(kueue_tas_ctx* c, const AdmitLayout& L, const kueue_tas_fits_req* reqs, size_t n,
                             const kueue_tas_fits_term* terms, size_t num_terms, const int64_t* wl_off, size_t n_wl,
                             int32_t pods_col, bool exact, const __int128* total, const AdmitTargets& tg,
                             int32_t* verdict);

static int admit_impl(kueue_tas_ctx* c, const kueue_tas_fits_req* reqs, size_t n, const kueue_tas_fits_term* terms,
                      size_t num_terms, const int64_t* wl_off, size_t n_wl, int32_t pods_col, int32_t* admitted,
                      const AdmitTargets* tg) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (n_wl == 0) return KUEUE_TAS_OK;
  if (!wl_off || !admitted || (n && !reqs) || (num_terms && !terms)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  if (pods_col < -1 || pods_col >= c->snap.R) return fail(c, KUEUE_TAS_EINVAL, "pods column out of range");
  if (wl_off[0] != 0 || size_t(wl_off[n_wl]) != n) return fail(c, KUEUE_TAS_EINVAL, "workload offsets");
  for (size_t w = 0; w < n_wl; w++)
    if (wl_off[w + 1] < wl_off[w]) return fail(c, KUEUE_TAS_EINVAL, "workload offsets not monotone");
  if (tg) {  // the target table and the entries' lists, before anything is enqueued
    if (!tg->eoff || (tg->T && !tg->off)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
    if (tg->T > size_t(INT32_MAX)) return fail(c, KUEUE_TAS_EINVAL, "too many targets");
    if (tg->T && tg->off[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "target offsets");
    for (size_t t = 0; t < tg->T; t++)
      if (tg->off[t + 1] < tg->off[t]) return fail(c, KUEUE_TAS_EINVAL, "target offsets not monotone");
    const size_t nd = tg->T ? size_t(tg->off[tg->T]) : 0;
    if (nd && !tg->deltas) return fail(c, KUEUE_TAS_EINVAL, "null argument");
    for (size_t j = 0; j < nd; j++) {
      const kueue_tas_delta& x = tg->deltas[j];
      if (x.leaf < -1 || x.leaf >= c->snap.N) return fail(c, KUEUE_TAS_EINVAL, "target record leaf out of range");
      if (x.col < 0 || x.col >= c->snap.R) return fail(c, KUEUE_TAS_EINVAL, "target record column out of range");
    }
    if (tg->eoff[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "entry target offsets");
    for (size_t w = 0; w < n_wl; w++)
      if (tg->eoff[w + 1] < tg->eoff[w]) return fail(c, KUEUE_TAS_EINVAL, "entry target offsets not monotone");
    if (tg->eoff[n_wl] && !tg->ids) return fail(c, KUEUE_TAS_EINVAL, "null argument");
    std::vector<int64_t> last(tg->T, -1);  // the entry that listed the target last
    for (size_t w = 0; w < n_wl; w++)
      for (int64_t k = tg->eoff[w]; k < tg->eoff[w + 1]; k++) {
        const int32_t t = tg->ids[k];
        if (t < 0 || size_t(t) >= tg->T) return fail(c, KUEUE_TAS_EINVAL, "target id out of range");
        if (last[size_t(t)] == int64_t(w)) return fail(c, KUEUE_TAS_EINVAL, "target listed twice by one entry");
        last[size_t(t)] = int64_t(w);
      }
    if (tg->eoff[n_wl] == 0) tg = nullptr;  // no entry carries targets: kueue_tas_admit's pass as it is
  }
  // per record on the host pool: the range checks, and for the monotone
  // shortcut (admit_fit0_kernel) the most usage this call can add per column
  // — the shortcut holds only for non-negative values and counts whose totals
  // stay below 2^61 (with every capacity and usage value below 2^61, checked
  // on the device, no int64 arithmetic of the call wraps)
  ktas_pool::HostPool& pool = ktas_pool::HostPool::get();
  const size_t nparts = pool.parts();
  struct alignas(64) AdmitPart {  // one per worker, on cache lines of its own
    __int128 total[KUEUE_TAS_MAX_COLS];
    bool exact;
    int err;  // 0, 1: record out of range, 2: term column out of range
  };
  std::vector<AdmitPart> parts(nparts);
  const int32_t snapN = c->snap.N, snapR = c->snap.R;
  pool.run_static(n, [&](size_t i0, size_t i1) {
    size_t t = 0;
    while (t + 1 < nparts && ktas_pool::HostPool::part_begin(n, t + 1, nparts) <= i0) t++;
    __int128 tot[KUEUE_TAS_MAX_COLS] = {};  // accumulated on the worker's stack, stored once
    bool ex = false;
    int err = 0;
    for (size_t i = i0; i < i1 && !err; i++) {
      const kueue_tas_fits_req& r = reqs[i];
      if (r.leaf >= snapN || r.num_terms < 0 || r.term_begin < 0 || size_t(r.term_begin) + size_t(r.num_terms) > num_terms) {
        err = 1;
        break;
      }
      ex = ex || r.count < 0;
      for (int k = 0; k < r.num_terms; k++) {
        const kueue_tas_fits_term& tm = terms[r.term_begin + k];
        if (tm.col < 0 || tm.col >= snapR) {
          err = 2;
          break;
        }
        ex = ex || tm.value < 0;
        if (tm.col < KUEUE_TAS_MAX_COLS) tot[tm.col] += __int128(tm.value) * r.count;
      }
      if (pods_col >= 0) tot[pods_col] += r.count;
    }
    AdmitPart& ap = parts[t];
    memcpy(ap.total, tot, sizeof tot);
    ap.exact = ex;
    ap.err = err;
  });
  bool exact = false;
  __int128 total[KUEUE_TAS_MAX_COLS] = {};  // per column: the most usage this call can add
  for (size_t t = 0; t < nparts && n > 0; t++) {
    if (parts[t].err == 1) return fail(c, KUEUE_TAS_EINVAL, "admit record out of range");
    if (parts[t].err == 2) return fail(c, KUEUE_TAS_EINVAL, "admit term column out of range");
  }
  for (size_t t = 0; t < nparts && n > 0; t++) {
    exact = exact || parts[t].exact;
    for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++) total[k] += parts[t].total[k];
  }
  for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++) exact = exact || total[k] >= (__int128(1) << 61);
  HIPCHK(c, hipSetDevice(c->device));
  // one pinned upload: records, terms, workload offsets, record -> workload,
  // phase-1 flags (1 = fit) and the exact flag
  const AdmitLayout L = admit_layout(n, num_terms, n_wl, size_t(c->snap.N));
  c->admit_launches[0] = 1;
  c->admit_launches[1] = c->admit_launches[2] = 0;
  if (tg) return admit_targets_run(c, L, reqs, n, terms, num_terms, wl_off, n_wl, pods_col, exact, total, *tg, admitted);
  HIPCHK(c, c->d_fits.ensure(L.end));
  HIPCHK(c, c->h_stage.ensure(L.up_bytes));
  uint8_t* h = c->h_stage.p;
  if (num_terms) memcpy(h + L.o_terms, terms, num_terms * sizeof(kueue_tas_fits_term));
  memcpy(h + L.o_off, wl_off, (n_wl + 1) * 8);
  int32_t* rec_wl = reinterpret_cast<int32_t*>(h + L.o_recwl);
  pool.run_static(n_wl, [&](size_t w0, size_t w1) {  // the records and their workload, per workload range
    if (w1 > w0 && wl_off[w1] > wl_off[w0])
      memcpy(h + size_t(wl_off[w0]) * sizeof(kueue_tas_fits_req), reqs + wl_off[w0],
             size_t(wl_off[w1] - wl_off[w0]) * sizeof(kueue_tas_fits_req));
    for (size_t w = w0; w < w1; w++)
      for (int64_t i = wl_off[w]; i < wl_off[w + 1]; i++) rec_wl[i] = int32_t(w);
  });
  int32_t* fit0 = reinterpret_cast<int32_t*>(h + L.o_fit0);
  for (size_t w = 0; w < n_wl; w++) fit0[w] = 1;
  *reinterpret_cast<int32_t*>(h + L.o_exact) = exact ? 1 : 0;
  for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++)
    reinterpret_cast<int64_t*>(h + L.o_total)[k] = exact ? 0 : int64_t(total[k]);
  uint8_t* d = c->d_fits.p;
  HIPCHK(c, hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, c->stream));
  const int rc = admit_run(c, L, d, reinterpret_cast<const kueue_tas_fits_term*>(d + L.o_terms), n, n_wl, pods_col, exact);
  if (rc) return rc;
  HIPCHK(c, c->h_admit.reserve(n_wl + 3));
  HIPCHK(c, hipMemcpyAsync(c->h_admit.p, d + L.o_out, (n_wl + 3) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(admitted, c->h_admit.p, n_wl * 4);
  c->admit_stats[0] = c->admit_window ? c->h_admit.p[n_wl] : -1;
  c->admit_stats[1] = c->admit_window ? c->h_admit.p[n_wl + 1] : -1;
  c->admit_stats[2] = int64_t(n_wl);
  return KUEUE_TAS_OK;
}

int kueue_tas_admit(kueue_tas_ctx* c, const kueue_tas_fits_req* reqs, size_t n, const kueue_tas_fits_term* terms,
                    size_t num_terms, const int64_t* wl_off, size_t n_wl, int32_t pods_col, int32_t* admitted) {
  return admit_impl(c, reqs, n, terms, num_terms, wl_off, n_wl, pods_col, admitted, nullptr);
}

int kueue_tas_admit_targets(kueue_tas_ctx* c, const kueue_tas_fits_req* reqs, size_t n, const kueue_tas_fits_term* terms,
                            size_t num_terms, const int64_t* wl_off, size_t n_wl, int32_t pods_col,
                            const kueue_tas_delta* target_deltas, const int64_t* target_off, size_t n_targets,
                            const int32_t* entry_targets, const int64_t* entry_target_off, int32_t* verdict) {
  const AdmitTargets tg{target_deltas, target_off, n_targets, entry_targets, entry_target_off};
  return admit_impl(c, reqs, n, terms, num_terms, wl_off, n_wl, pods_col, verdict, &tg);
}

// A validated call in which some entry carries targets.  The ordered list is
// cut into runs of target-free entries, which go through the pass
// (admit_run_view: inside a run the usage only grows, the preempted targets
// staying subtracted), and the stretches between them — the target entries,
// and target-free runs too short to pay for the pass's launches — which one
// admit_step_kernel launch takes in order.  Everything is enqueued on the
// context's stream; admit_restore_kernel puts the preempted targets' usage
// back; one D2H brings the verdicts.
static int admit_targets_run(kueue_tas_ctx* c, const AdmitLayout& L, const kueue_tas_fits_req* reqs, size_t n,
                             const kueue_tas_fits_term* terms, size_t num_terms, const int64_t* wl_off, size_t n_wl,
                             int32_t pods_col, bool exact, const __int128* total, const AdmitTargets& tg,
                             int32_t* verdict) {
  std::vector<AdmitSeg> segs;
  const size_t min_run = size_t(std::max(c->knobs.admit_step_run, 1));
  for (size_t w = 0; w < n_wl;) {
    size_t e = w;
    while (e < n_wl && tg.eoff[e + 1] == tg.eoff[e]) e++;  // [w, e): target-free
    const bool pass = e - w >= min_run;
    if (e == w) e = w + 1;  // a target entry
    if (!pass && !segs.empty() && !segs.back().pass) segs.back().b = e;
    else segs.push_back({pass, w, e});
    w = e;
  }
  size_t n_pass = 0;
  for (const AdmitSeg& sg : segs) n_pass += sg.pass ? 1 : 0;
  // behind the pass's layout: the target table, the entries' lists, the runs'
  // relative offsets (uploaded), the preempted bitmap
  const size_t nd = size_t(tg.off[tg.T]), ne = size_t(tg.eoff[n_wl]), pwords = (tg.T + 31) / 32;
  const size_t x_td = 0, x_toff = x_td + admit_al(nd * sizeof(kueue_tas_delta)), x_etg = x_toff + admit_al((tg.T + 1) * 8),
               x_eoff = x_etg + admit_al(ne * 4), x_roff = x_eoff + admit_al((n_wl + 1) * 8),
               x_up = x_roff + admit_al((n_wl + n_pass + 1) * 8), x_pre = x_up, x_end = x_pre + admit_al(pwords * 4);
  HIPCHK(c, c->d_fits.ensure(L.end + x_end));
  const size_t h_x = admit_al(L.up_bytes);
  HIPCHK(c, c->h_stage.ensure(h_x + x_up));
  uint8_t* h = c->h_stage.p;
  if (n) memcpy(h, reqs, n * sizeof(kueue_tas_fits_req));
  if (num_terms) memcpy(h + L.o_terms, terms, num_terms * sizeof(kueue_tas_fits_term));
  memcpy(h + L.o_off, wl_off, (n_wl + 1) * 8);
  int32_t* rec_wl = reinterpret_cast<int32_t*>(h + L.o_recwl);
  int64_t* roff = reinterpret_cast<int64_t*>(h + h_x + x_roff);
  std::vector<size_t> roff_at(segs.size(), 0);
  size_t ro = 0;
  for (size_t q = 0; q < segs.size(); q++) {  // record -> workload and the offsets, relative to the run
    const AdmitSeg& sg = segs[q];
    if (!sg.pass) continue;
    roff_at[q] = ro;
    for (size_t w = sg.a; w <= sg.b; w++) roff[ro++] = wl_off[w] - wl_off[sg.a];
    for (size_t w = sg.a; w < sg.b; w++)
      for (int64_t i = wl_off[w]; i < wl_off[w + 1]; i++) rec_wl[i] = int32_t(w - sg.a);
  }
  int32_t* fit0 = reinterpret_cast<int32_t*>(h + L.o_fit0);
  for (size_t w = 0; w < n_wl; w++) fit0[w] = 1;
  *reinterpret_cast<int32_t*>(h + L.o_exact) = exact ? 1 : 0;
  for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++)  // the call's total bounds every run's additions
    reinterpret_cast<int64_t*>(h + L.o_total)[k] = exact ? 0 : int64_t(total[k]);
  if (nd) memcpy(h + h_x + x_td, tg.deltas, nd * sizeof(kueue_tas_delta));
  memcpy(h + h_x + x_toff, tg.off, (tg.T + 1) * 8);
  memcpy(h + h_x + x_etg, tg.ids, ne * 4);
  memcpy(h + h_x + x_eoff, tg.eoff, (n_wl + 1) * 8);
  uint8_t* d = c->d_fits.p;
  uint8_t* dx = d + L.end;
  HIPCHK(c, hipMemcpyAsync(d, h, L.up_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(dx, h + h_x, x_up, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(dx + x_pre, 0, admit_al(pwords * 4), c->stream));
  const auto* d_reqs = reinterpret_cast<const kueue_tas_fits_req*>(d);
  const auto* d_terms = reinterpret_cast<const kueue_tas_fits_term*>(d + L.o_terms);
  const auto* d_td = reinterpret_cast<const kueue_tas_delta*>(dx + x_td);
  const auto* d_toff = reinterpret_cast<const int64_t*>(dx + x_toff);
  auto* d_pre = reinterpret_cast<uint32_t*>(dx + x_pre);
  int32_t* d_out = reinterpret_cast<int32_t*>(d + L.o_out);
  for (size_t q = 0; q < segs.size(); q++) {
    const AdmitSeg& sg = segs[q];
    if (sg.pass) {
      const size_t r0 = size_t(wl_off[sg.a]);
      const AdmitView v{d_reqs + r0,
                        reinterpret_cast<const int32_t*>(d + L.o_recwl) + r0,
                        reinterpret_cast<const int64_t*>(dx + x_roff) + roff_at[q],
                        reinterpret_cast<int32_t*>(d + L.o_fit0) + sg.a,
                        d_out + sg.a,
                        reinterpret_cast<AdmitRec*>(d + L.o_recs) + r0,
                        reinterpret_cast<int32_t*>(d + L.o_dep) + sg.a};
      const int rc = admit_run_view(c, L, d, v, d_terms, size_t(wl_off[sg.b]) - r0, sg.b - sg.a, pods_col, exact);
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL(admit_step_kernel, dim3(1), dim3(1024), 0, c->stream, c->snap, c->d_usage.p,
                         c->d_usage_present.p, d_reqs, d_terms, reinterpret_cast<const int64_t*>(d + L.o_off), int(sg.a),
                         int(sg.b), pods_col, d_td, d_toff, reinterpret_cast<const int32_t*>(dx + x_etg),
                         reinterpret_cast<const int64_t*>(dx + x_eoff), d_pre, d_out);
      HIPCHK(c, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(admit_restore_kernel, dim3(unsigned(std::min<size_t>((tg.T + 3) / 4, 1024))), dim3(256), 0, c->stream,
                     c->d_usage.p, c->snap.N, d_td, d_toff, int(tg.T), d_pre);
  HIPCHK(c, hipGetLastError());
  // the diagnostics words are the last run's; a run that ended short of the
  // list's end left its own among the verdicts, which the later entries overwrote
  if (!segs.back().pass) HIPCHK(c, hipMemsetAsync(d_out + n_wl, 0, 12, c->stream));
  HIPCHK(c, c->h_admit.reserve(n_wl + 3));
  HIPCHK(c, hipMemcpyAsync(c->h_admit.p, d_out, (n_wl + 3) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(verdict, c->h_admit.p, n_wl * 4);
  c->admit_stats[0] = c->admit_window ? c->h_admit.p[n_wl] : -1;
  c->admit_stats[1] = c->admit_window ? c->h_admit.p[n_wl + 1] : -1;
  c->admit_stats[2] = int64_t(n_wl);
  c->admit_launches[0] = int64_t(n_pass);
  c->admit_launches[1] = int64_t(segs.size() - n_pass);
  c->admit_launches[2] += int64_t(segs.size() - n_pass) + 1;  // + the passes' (admit_run_view)
  return KUEUE_TAS_OK;
}

int kueue_tas_copy_to_host(kueue_tas_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c || (bytes && (!dst || !src))) return KUEUE_TAS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  if (bytes) HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return KUEUE_TAS_OK;
}

int kueue_tas_admit_table(kueue_tas_ctx* c, const int32_t* ps_base, int32_t num_workloads, const int32_t* ps_terms,
                          const kueue_tas_fits_term* terms, size_t num_terms) {
  if (!c || num_workloads < 0 || !ps_base || (num_terms && !terms)) return KUEUE_TAS_EINVAL;
  const int32_t P = ps_base[num_workloads];
  if (P < 0 || (P && !ps_terms)) return fail(c, KUEUE_TAS_EINVAL, "admit table: podsets");
  for (int32_t w = 0; w < num_workloads; w++)
    if (ps_base[w + 1] < ps_base[w] || ps_base[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "admit table: podset offsets");
  for (int32_t p = 0; p < P; p++)
    if (ps_terms[2 * p] < 0 || ps_terms[2 * p + 1] < 0 || size_t(ps_terms[2 * p]) + size_t(ps_terms[2 * p + 1]) > num_terms)
      return fail(c, KUEUE_TAS_EINVAL, "admit table: term range");
  // -1 (a resource without a column) is the call's to report, for the terms
  // its records use, as kueue_tas_host_admit does; so is a column the
  // snapshot lost in a later reload (admit_block_records_kernel: col >= R)
  const int32_t col_end = c->loaded ? c->snap.R : KUEUE_TAS_MAX_COLS;
  for (size_t t = 0; t < num_terms; t++)
    if (terms[t].col < -1 || terms[t].col >= col_end) return fail(c, KUEUE_TAS_EINVAL, "admit table: term column out of range");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_adm_ps.ensure(size_t(num_workloads) + 1 + 2 * size_t(P)));
  HIPCHK(c, c->d_adm_terms.ensure(std::max<size_t>(num_terms, 1)));
  HIPCHK(c, hipMemcpy(c->d_adm_ps.p, ps_base, (size_t(num_workloads) + 1) * 4, hipMemcpyHostToDevice));
  if (P) HIPCHK(c, hipMemcpy(c->d_adm_ps.p + num_workloads + 1, ps_terms, 2 * size_t(P) * 4, hipMemcpyHostToDevice));
  if (num_terms)
    HIPCHK(c, hipMemcpy(c->d_adm_terms.p, terms, num_terms * sizeof(kueue_tas_fits_term), hipMemcpyHostToDevice));
  c->adm_W = num_workloads;
  return KUEUE_TAS_OK;
}

// kueue_tas_admit_block_targets' extra arguments (null: kueue_tas_admit_block):
// the target table of kueue_tas_admit_targets and the entries' lists keyed by
// workload id.
struct AdmitBlockTargets {
  const kueue_tas_delta* deltas;
  const int64_t* off;  // [T + 1] CSR into deltas
  size_t T;
  const int32_t* entry_ids;      // [E] each id at most once, any order
  const int64_t* entry_off;      // [E + 1] CSR into entry_targets
  const int32_t* entry_targets;  // target ids
  size_t E;
};

// What kueue_tas_admit_targets rejects, and an entry id out of range.  An id
// given twice or without a header in the block shows after the first
// synchronise: on the device's claims (admit_block_entries_kernel), or for
// ids with empty lists only, on the headers' flags.
static int admit_block_targets_check(kueue_tas_ctx* c, const AdmitBlockTargets& bt, int W) {
  if ((bt.T && !bt.off) || (bt.E && (!bt.entry_ids || !bt.entry_off))) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  if (bt.T > size_t(INT32_MAX) || bt.E > size_t(INT32_MAX)) return fail(c, KUEUE_TAS_EINVAL, "too many targets");
  if (bt.T && bt.off[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "target offsets");
  for (size_t t = 0; t < bt.T; t++)
    if (bt.off[t + 1] < bt.off[t]) return fail(c, KUEUE_TAS_EINVAL, "target offsets not monotone");
  const size_t nd = bt.T ? size_t(bt.off[bt.T]) : 0;
  if (nd && !bt.deltas) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  for (size_t j = 0; j < nd; j++) {
    const kueue_tas_delta& x = bt.deltas[j];
    if (x.leaf < -1 || x.leaf >= c->snap.N) return fail(c, KUEUE_TAS_EINVAL, "target record leaf out of range");
    if (x.col < 0 || x.col >= c->snap.R) return fail(c, KUEUE_TAS_EINVAL, "target record column out of range");
  }
  if (!bt.E) return KUEUE_TAS_OK;
  if (bt.entry_off[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "entry target offsets");
  for (size_t e = 0; e < bt.E; e++)
    if (bt.entry_off[e + 1] < bt.entry_off[e]) return fail(c, KUEUE_TAS_EINVAL, "entry target offsets not monotone");
  if (bt.entry_off[bt.E] > int64_t(INT32_MAX)) return fail(c, KUEUE_TAS_EINVAL, "too many targets");
  if (bt.entry_off[bt.E] && !bt.entry_targets) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  std::vector<int64_t> last(bt.entry_off[bt.E] ? bt.T : 0, -1);  // the entry that listed the target last
  for (size_t e = 0; e < bt.E; e++) {
    const int32_t g = bt.entry_ids[e];
    if (g < 0 || g >= W) return fail(c, KUEUE_TAS_EINVAL, "entry id out of range");
    for (int64_t k = bt.entry_off[e]; k < bt.entry_off[e + 1]; k++) {
      const int32_t t = bt.entry_targets[k];
      if (t < 0 || size_t(t) >= bt.T) return fail(c, KUEUE_TAS_EINVAL, "target id out of range");
      if (last[size_t(t)] == int64_t(e)) return fail(c, KUEUE_TAS_EINVAL, "target listed twice by one entry");
      last[size_t(t)] = int64_t(e);
    }
  }
  return KUEUE_TAS_OK;
}

// admit_targets_run over the block path's device arrays: the records, the
// absolute record -> workload map and the offsets are at layout L (`d`), the
// compiled terms in c->d_adm_terms, the target table and the per-position
// lists behind it.  wl_off: the host's copy of the offsets (read when a run
// goes through the pass: its record range sizes the launches).  The pass
// runs' bounds are uploaded and admit_block_runs_kernel writes their relative
// offsets and maps; the verdicts stay on the device for the delta kernels.
static int admit_block_targets_run(kueue_tas_ctx* c, const AdmitLayout& L, uint8_t* d, const std::vector<AdmitSeg>& segs,
                                   size_t n_pass, const int64_t* wl_off, size_t n_wl, int32_t pods_col, bool exact,
                                   size_t T, uint8_t* h_bnd, uint8_t* d_td8, uint8_t* d_toff8, uint8_t* d_etg8,
                                   uint8_t* d_eoff8, uint8_t* d_pre8, size_t pwords, uint8_t* d_bnd8, uint8_t* d_roff8,
                                   uint8_t* d_rel8) {
  const auto* d_reqs = reinterpret_cast<const kueue_tas_fits_req*>(d);
  const kueue_tas_fits_term* d_terms = c->d_adm_terms.p;
  const auto* d_off = reinterpret_cast<const int64_t*>(d + L.o_off);
  const auto* d_td = reinterpret_cast<const kueue_tas_delta*>(d_td8);
  const auto* d_toff = reinterpret_cast<const int64_t*>(d_toff8);
  auto* d_pre = reinterpret_cast<uint32_t*>(d_pre8);
  int32_t* d_out = reinterpret_cast<int32_t*>(d + L.o_out);
  std::vector<size_t> roff_at(segs.size(), 0);
  if (n_pass) {
    int64_t* bnd = reinterpret_cast<int64_t*>(h_bnd);
    size_t ro = 0, k = 0, widest = 1;
    for (size_t q = 0; q < segs.size(); q++) {
      const AdmitSeg& sg = segs[q];
      if (!sg.pass) continue;
      roff_at[q] = ro;
      bnd[3 * k] = int64_t(sg.a);
      bnd[3 * k + 1] = int64_t(sg.b);
      bnd[3 * k + 2] = int64_t(ro);
      ro += sg.b - sg.a + 1;
      k++;
      widest = std::max({widest, sg.b - sg.a + 1, size_t(wl_off[sg.b] - wl_off[sg.a])});
    }
    HIPCHK(c, hipMemcpyAsync(d_bnd8, bnd, n_pass * 24, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(admit_block_runs_kernel, dim3(unsigned(std::min<size_t>((widest + 255) / 256, 64)),
                                                     unsigned(std::min<size_t>(n_pass, 65535))),
                       dim3(256), 0, c->stream, reinterpret_cast<const int64_t*>(d_bnd8), int(n_pass), d_off,
                       reinterpret_cast<const int32_t*>(d + L.o_recwl), reinterpret_cast<int64_t*>(d_roff8),
                       reinterpret_cast<int32_t*>(d_rel8));
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemsetAsync(d_pre, 0, admit_al(pwords * 4), c->stream));
  for (size_t q = 0; q < segs.size(); q++) {
    const AdmitSeg& sg = segs[q];
    if (sg.pass) {
      const size_t r0 = size_t(wl_off[sg.a]);
      const AdmitView v{d_reqs + r0,
                        reinterpret_cast<const int32_t*>(d_rel8) + r0,
                        reinterpret_cast<const int64_t*>(d_roff8) + roff_at[q],
                        reinterpret_cast<int32_t*>(d + L.o_fit0) + sg.a,
                        d_out + sg.a,
                        reinterpret_cast<AdmitRec*>(d + L.o_recs) + r0,
                        reinterpret_cast<int32_t*>(d + L.o_dep) + sg.a};
      const int rc = admit_run_view(c, L, d, v, d_terms, size_t(wl_off[sg.b]) - r0, sg.b - sg.a, pods_col, exact);
      if (rc) return rc;
    } else {
      hipLaunchKernelGGL(admit_step_kernel, dim3(1), dim3(1024), 0, c->stream, c->snap, c->d_usage.p,
                         c->d_usage_present.p, d_reqs, d_terms, d_off, int(sg.a), int(sg.b), pods_col, d_td, d_toff,
                         reinterpret_cast<const int32_t*>(d_etg8), reinterpret_cast<const int64_t*>(d_eoff8), d_pre,
                         d_out);
      HIPCHK(c, hipGetLastError());
    }
  }
  hipLaunchKernelGGL(admit_restore_kernel, dim3(unsigned(std::min<size_t>((T + 3) / 4, 1024))), dim3(256), 0, c->stream,
                     c->d_usage.p, c->snap.N, d_td, d_toff, int(T), d_pre);
  HIPCHK(c, hipGetLastError());
  // the diagnostics words are the last run's (admit_targets_run)
  if (segs.empty() || !segs.back().pass) HIPCHK(c, hipMemsetAsync(d_out + n_wl, 0, 12, c->stream));
  c->admit_launches[0] = int64_t(n_pass);
  c->admit_launches[1] = int64_t(segs.size() - n_pass);
  c->admit_launches[2] += int64_t(segs.size() - n_pass) + 1 + (n_pass ? 1 : 0);  // + the passes' (admit_run_view)
  return KUEUE_TAS_OK;
}

// kueue_tas_admit_block, and with `bt` kueue_tas_admit_block_targets: the
// records, the verdicts' D2H and the delta list are the same; with targets
// the id-keyed lists become per-position ones on the device
// (admit_block_entries_kernel, its bitmap and error bits in the first D2H),
// the host cuts the list into runs as admit_targets_run does, and the runs'
// relative maps come from admit_block_runs_kernel.
static int admit_block_impl(kueue_tas_ctx* c, const int32_t* block, size_t row_words, const int64_t* lens,
                            int32_t world, int32_t pods_col, int32_t* ids, int32_t* admitted, size_t cap,
                            size_t* n_workloads, const kueue_tas_delta** deltas, size_t* n_deltas,
                            const AdmitBlockTargets* bt) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!block || !lens || !ids || !admitted || !n_workloads || !deltas || !n_deltas || world < 1)
    return fail(c, KUEUE_TAS_EINVAL, "null argument");
  if (c->adm_W < 0) return fail(c, KUEUE_TAS_EINVAL, "admit block: no admission table (kueue_tas_admit_table)");
  if (pods_col < -1 || pods_col >= c->snap.R) return fail(c, KUEUE_TAS_EINVAL, "pods column out of range");
  if (bt) {
    const int rc = admit_block_targets_check(c, *bt, c->adm_W);
    if (rc) return rc;
  }
  // some entry lists a target: the targets path; ids given with empty lists
  // only: kueue_tas_admit_block's launches, the ids checked against the headers
  const bool tgt = bt && bt->E && bt->entry_off[bt->E] > 0, chk = bt && bt->E && !tgt;
  AdmitRows rows{};
  rows.row_words = int64_t(row_words);
  rows.world = world;
  size_t Q = 0;
  int32_t maxq = 0;
  for (int r = 0; r < world; r++) {  // every row's, also of a block the fallback reads (EHOSTMEM, more rows than supported)
    if (lens[r] < 0 || lens[r] % 4 || size_t(lens[r]) + 1 > row_words) return fail(c, KUEUE_TAS_EINVAL, "admit block: row length");
    Q += size_t(lens[r] / 4);
  }
  const int W = c->adm_W;
  HIPCHK(c, hipSetDevice(c->device));
  {  // device memory only: kernels must not read a pageable host array
    hipPointerAttribute_t pa{};
    if (hipPointerGetAttributes(&pa, block) != hipSuccess || pa.type != hipMemoryTypeDevice) {
      (void)hipGetLastError();
      return fail(c, KUEUE_TAS_EHOSTMEM, "admit block: not device memory");
    }
  }
  // (after the pointer's type: the fallback copies a device block and reads a host block)
  if (world > kAdmitMaxRows) return fail(c, KUEUE_TAS_ELAYOUT, "admit block: more rows than supported");
  if (Q > size_t(INT32_MAX)) return fail(c, KUEUE_TAS_ELAYOUT, "admit block: more quads than supported");
  for (int r = 0; r < world; r++) {
    rows.nq[r] = int32_t(lens[r] / 4);
    maxq = std::max(maxq, rows.nq[r]);
  }
  // the layout of the host path with the bounds (records <= quads, workloads <= W)
  const AdmitLayout L = admit_layout(std::max<size_t>(Q, 1), 0, size_t(W), size_t(c->snap.N));
  // per id: flag, run position, quad count; hdr: workloads, records, deltas; errors; exact; totals (lo, hi)
  const size_t o_flag = L.end, o_pos = o_flag + admit_al(size_t(W) * 4), o_nd = o_pos + admit_al(size_t(W) * 8),
               o_ids = o_nd + admit_al(size_t(W) * 4), o_hdr = o_ids + admit_al(size_t(W) * 4),
               o_tot = o_hdr + 256, o_blk = o_tot + admit_al(KUEUE_TAS_MAX_COLS * 16),
               nblk = (std::max<size_t>(Q, 1) + 255) / 256, o_dl = o_blk + admit_al(nblk * 4);
  // with targets, behind it: the target table and the id-keyed lists
  // (uploaded), the positions' claims and the carries-targets bitmap (zeroed),
  // the per-position lists, the preempted bitmap, the pass runs' bounds, their
  // relative offsets and record -> workload map
  const size_t T = tgt ? bt->T : 0, E = tgt ? bt->E : 0, ntd = tgt ? size_t(bt->off[T]) : 0,
               ne = tgt ? size_t(bt->entry_off[E]) : 0, pwords = (T + 31) / 32,
               hwords = (size_t(W) + 1023) / 1024 * 32, max_runs = size_t(W) / 2 + 2;
  const size_t x_td = admit_al(o_dl + 16), x_toff = x_td + admit_al(ntd * sizeof(kueue_tas_delta)),
               x_eid = x_toff + admit_al((T + 1) * 8), x_eto = x_eid + admit_al(E * 4),
               x_etl = x_eto + admit_al((E + 1) * 8), x_up = x_etl + admit_al(ne * 4), x_entof = x_up,
               x_has = x_entof + admit_al(size_t(W) * 4), x_eoff = x_has + admit_al(hwords * 4),
               x_etg = x_eoff + admit_al((size_t(W) + 1) * 8), x_pre = x_etg + admit_al(ne * 4),
               x_bnd = x_pre + admit_al(pwords * 4), x_roff = x_bnd + admit_al(max_runs * 24),
               x_rel = x_roff + admit_al((size_t(W) + max_runs + 1) * 8),
               x_end = x_rel + admit_al(std::max<size_t>(Q, 1) * 4);
  HIPCHK(c, c->d_fits.ensure(tgt ? x_end : o_dl + 16));
  uint8_t* d = c->d_fits.p;
  int32_t* hdr = reinterpret_cast<int32_t*>(d + o_hdr);  // [0] workloads [1] records [2] deltas [3] errors [4] negative
                                                         // [5] entry errors (AdmitEntryErr)
  // behind them, per row: the sum of 1 + n over its headers (admit_block_headers_kernel)
  constexpr size_t kRowSumAt = 64, kHdrD2H = kRowSumAt + kAdmitMaxRows * 8;
  static_assert(kHdrD2H <= 256, "the header words and the row sums share the zeroed 256 bytes");
  // pinned host words: the plain call's, then the bitmap, the workload offsets (int64) and, for ids given
  // with empty lists only, the headers' flags
  const size_t a_has = (size_t(W) + 3 + 64 + KUEUE_TAS_MAX_COLS * 4 + 1) / 2 * 2, a_off = a_has + hwords,
               a_flag = a_off + 2 * (size_t(W) + 1), a_end = a_flag + size_t(W);
  HIPCHK(c, c->h_admit.reserve(bt ? a_end : size_t(W) + 3 + 64 + KUEUE_TAS_MAX_COLS * 4));
  // pinned staging: the exact flag and the totals first (below), then the uploads of the targets path
  const size_t hs_x = admit_al(8 + KUEUE_TAS_MAX_COLS * 8);
  if (tgt) HIPCHK(c, c->h_stage.ensure(hs_x + std::max(x_up - x_td, admit_al(max_runs * 24))));
  HIPCHK(c, hipMemsetAsync(d + o_flag, 0, size_t(W) * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(d + o_hdr, 0, 256 + admit_al(KUEUE_TAS_MAX_COLS * 16), c->stream));
  const double t0 = wall_ms();
  if (tgt) {
    uint8_t* h = c->h_stage.p + hs_x;
    if (ntd) memcpy(h, bt->deltas, ntd * sizeof(kueue_tas_delta));
    memcpy(h + (x_toff - x_td), bt->off, (T + 1) * 8);
    memcpy(h + (x_eid - x_td), bt->entry_ids, E * 4);
    memcpy(h + (x_eto - x_td), bt->entry_off, (E + 1) * 8);
    memcpy(h + (x_etl - x_td), bt->entry_targets, ne * 4);
    HIPCHK(c, hipMemcpyAsync(d + x_td, h, x_up - x_td, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d + x_entof, 0, x_eoff - x_entof, c->stream));
  }
  if (maxq > 0) {
    hipLaunchKernelGGL(admit_block_headers_kernel, dim3(unsigned((maxq + 255) / 256), unsigned(world)), dim3(256), 0,
                       c->stream, block, rows, W, reinterpret_cast<int32_t*>(d + o_flag),
                       reinterpret_cast<int64_t*>(d + o_pos), reinterpret_cast<int32_t*>(d + o_nd),
                       reinterpret_cast<unsigned long long*>(d + o_hdr + kRowSumAt), hdr + 3);
    HIPCHK(c, hipGetLastError());
  }
  hipLaunchKernelGGL(admit_block_offsets_kernel, dim3(1), dim3(1024), 0, c->stream, W,
                     reinterpret_cast<const int32_t*>(d + o_flag), reinterpret_cast<const int32_t*>(d + o_nd),
                     reinterpret_cast<int32_t*>(d + o_ids), reinterpret_cast<int64_t*>(d + L.o_off),
                     reinterpret_cast<int32_t*>(d + L.o_fit0), hdr);
  HIPCHK(c, hipGetLastError());
  int32_t* hh = c->h_admit.p;
  if (tgt) {  // the lists by position, their bitmap and error bits: back in the D2H that reads hdr
    hipLaunchKernelGGL(admit_block_entries_kernel, dim3(1), dim3(1024), 0, c->stream, hdr,
                       reinterpret_cast<const int32_t*>(d + o_ids), reinterpret_cast<const int32_t*>(d + x_eid),
                       reinterpret_cast<const int64_t*>(d + x_eto), reinterpret_cast<const int32_t*>(d + x_etl), int(E),
                       reinterpret_cast<int32_t*>(d + x_entof), reinterpret_cast<int64_t*>(d + x_eoff),
                       reinterpret_cast<int32_t*>(d + x_etg), reinterpret_cast<uint32_t*>(d + x_has), hdr + 5);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hh + a_has, d + x_has, hwords * 4, hipMemcpyDeviceToHost, c->stream));
  }
  if (chk) HIPCHK(c, hipMemcpyAsync(hh + a_flag, d + o_flag, size_t(W) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hh, hdr, kHdrD2H, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int32_t n_wl = hh[0], n = hh[1];
  // every row tiled by its headers' runs (with no header twice and, below,
  // every run quad its workload's: no overlap, no quad outside a run), so
  // the records are at most the quads the layout was sized for
  bool tiled = n >= 0 && size_t(n) <= Q;
  uint64_t row_sum[kAdmitMaxRows];
  memcpy(row_sum, reinterpret_cast<const uint8_t*>(hh) + kRowSumAt, sizeof row_sum);
  for (int r = 0; r < world; r++) tiled = tiled && row_sum[r] == uint64_t(rows.nq[r]);
  if ((hh[3] & (ABE_DUP | ABE_LAYOUT | ABE_ID)) || !tiled)
    return fail(c, KUEUE_TAS_ELAYOUT, "admit block: not the assignments layout");
  if (tgt && (hh[5] & AEE_ABSENT)) return fail(c, KUEUE_TAS_EINVAL, "entry id without a header in the block");
  if (tgt && (hh[5] & AEE_DUP)) return fail(c, KUEUE_TAS_EINVAL, "entry id given twice");
  if (chk)
    for (size_t e = 0; e < bt->E; e++) {  // (a flag is 1 or 2 for a header; -1 marks an id seen here)
      int32_t& f = hh[a_flag + size_t(bt->entry_ids[e])];
      if (f < 0) return fail(c, KUEUE_TAS_EINVAL, "entry id given twice");
      if (!f) return fail(c, KUEUE_TAS_EINVAL, "entry id without a header in the block");
      f = -1;
    }
  *n_workloads = size_t(n_wl);
  if (cap < size_t(n_wl)) return KUEUE_TAS_EOVERFLOW;
  const size_t nwl = size_t(n_wl), nr = size_t(n);
  // the ordered list cut as admit_targets_run cuts it, by the positions' bitmap
  std::vector<AdmitSeg> segs;
  size_t n_pass = 0;
  if (tgt) {
    const uint32_t* has = reinterpret_cast<const uint32_t*>(hh + a_has);
    auto carries = [&](size_t w) { return (has[w >> 5] >> (w & 31)) & 1u; };
    const size_t min_run = size_t(std::max(c->knobs.admit_step_run, 1));
    for (size_t w = 0; w < nwl;) {
      size_t e = w;
      while (e < nwl && !carries(e)) e++;  // [w, e): target-free
      const bool pass = e - w >= min_run;
      if (e == w) e = w + 1;  // a target entry
      if (!pass && !segs.empty() && !segs.back().pass) segs.back().b = e;
      else segs.push_back({pass, w, e});
      w = e;
    }
    for (const AdmitSeg& sg : segs) n_pass += sg.pass ? 1 : 0;
  }
  if (nwl) {
    hipLaunchKernelGGL(admit_block_records_kernel, dim3(unsigned((nwl + 3) / 4)), dim3(256), 0, c->stream, block,
                       c->snap.N, W, reinterpret_cast<const int32_t*>(d + o_ids), reinterpret_cast<const int64_t*>(d + L.o_off),
                       reinterpret_cast<const int32_t*>(d + o_flag), reinterpret_cast<const int64_t*>(d + o_pos),
                       reinterpret_cast<const int32_t*>(d + o_nd), c->d_adm_ps.p, c->d_adm_ps.p + W + 1,
                       c->d_adm_terms.p, n_wl, pods_col, c->snap.R, reinterpret_cast<kueue_tas_fits_req*>(d),
                       reinterpret_cast<int32_t*>(d + L.o_recwl), reinterpret_cast<unsigned long long*>(d + o_tot),
                       hdr + 4, hdr + 3);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(hh, hdr, 32, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hh + 8, d + o_tot, KUEUE_TAS_MAX_COLS * 16, hipMemcpyDeviceToHost, c->stream));
  if (n_pass)  // the runs' record ranges (the pass's launch sizes) are the host's to know
    HIPCHK(c, hipMemcpyAsync(hh + a_off, d + L.o_off, (nwl + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int32_t errs = hh[3];
  if (errs & ABE_LAYOUT) return fail(c, KUEUE_TAS_ELAYOUT, "admit block: not the assignments layout");
  if (errs & ABE_RANGE) return fail(c, KUEUE_TAS_EINVAL, "record out of range");
  if (errs & ABE_COL) return fail(c, KUEUE_TAS_EINVAL, "request resource without a column");
  bool exact = hh[4] != 0;
  const uint64_t* tot = reinterpret_cast<const uint64_t*>(hh + 8);
  int64_t tot64[KUEUE_TAS_MAX_COLS];
  for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++) {
    exact = exact || tot[2 * k + 1] != 0 || tot[2 * k] >= (uint64_t(1) << 61);
    tot64[k] = int64_t(tot[2 * k]);
  }
  // the exact flag and the totals, as the host path uploads them
  HIPCHK(c, c->h_stage.ensure(8 + KUEUE_TAS_MAX_COLS * 8));
  int32_t* hx = reinterpret_cast<int32_t*>(c->h_stage.p);
  hx[0] = exact ? 1 : 0;
  HIPCHK(c, hipMemcpyAsync(d + L.o_exact, hx, 4, hipMemcpyHostToDevice, c->stream));
  int64_t* ht = reinterpret_cast<int64_t*>(c->h_stage.p + 8);
  for (int k = 0; k < KUEUE_TAS_MAX_COLS; k++) ht[k] = exact ? 0 : tot64[k];
  HIPCHK(c, hipMemcpyAsync(d + L.o_total, ht, KUEUE_TAS_MAX_COLS * 8, hipMemcpyHostToDevice, c->stream));
  c->admit_launches[0] = 1;
  c->admit_launches[1] = c->admit_launches[2] = 0;
  if (tgt) {
    const int rc = admit_block_targets_run(c, L, d, segs, n_pass, reinterpret_cast<const int64_t*>(hh + a_off), nwl,
                                           pods_col, exact, T, c->h_stage.p + hs_x, d + x_td, d + x_toff, d + x_etg,
                                           d + x_eoff, d + x_pre, pwords, d + x_bnd, d + x_roff, d + x_rel);
    if (rc) return rc;
  } else {
    const int rc = admit_run(c, L, d, c->d_adm_terms.p, nr, nwl, pods_col, exact);
    if (rc) return rc;
  }
  // the admitted workloads' deltas on the device, in the host path's order
  const int32_t* adm_d = reinterpret_cast<const int32_t*>(d + L.o_out);
  const size_t nb = (std::max<size_t>(nr, 1) + 255) / 256;
  int32_t* blk = reinterpret_cast<int32_t*>(d + o_blk);
  if (nr) {
    hipLaunchKernelGGL(admit_delta_blocks_kernel, dim3(unsigned(nb)), dim3(256), 0, c->stream,
                       reinterpret_cast<const kueue_tas_fits_req*>(d), reinterpret_cast<const int32_t*>(d + L.o_recwl),
                       adm_d, n, pods_col, blk);
    hipLaunchKernelGGL(admit_delta_offsets_kernel, dim3(1), dim3(1024), 0, c->stream, blk, int(nb), hdr);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(hh, d + L.o_out, (nwl + 3) * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(hh + nwl + 3, hdr, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(ids, d + o_ids, nwl * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  memcpy(admitted, hh, nwl * 4);
  c->admit_stats[0] = c->admit_window ? hh[nwl] : -1;
  c->admit_stats[1] = c->admit_window ? hh[nwl + 1] : -1;
  c->admit_stats[2] = int64_t(nwl);
  const size_t ndl = nr ? size_t(hh[nwl + 3 + 2]) : 0;
  HIPCHK(c, c->d_adm_deltas.ensure(std::max<size_t>(ndl, 1)));
  HIPCHK(c, c->h_adm_deltas.reserve(std::max<size_t>(ndl, 1)));
  if (ndl) {
    hipLaunchKernelGGL(admit_delta_write_kernel, dim3(unsigned(nb)), dim3(256), 0, c->stream,
                       reinterpret_cast<const kueue_tas_fits_req*>(d), c->d_adm_terms.p,
                       reinterpret_cast<const int32_t*>(d + L.o_recwl), adm_d, n, pods_col, blk, c->d_adm_deltas.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_adm_deltas.p, c->d_adm_deltas.p, ndl * sizeof(kueue_tas_delta),
                             hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  *deltas = c->h_adm_deltas.p;
  *n_deltas = ndl;
  c->admit_block_ms = wall_ms() - t0;
  return KUEUE_TAS_OK;
}

int kueue_tas_admit_block(kueue_tas_ctx* c, const int32_t* block, size_t row_words, const int64_t* lens,
                          int32_t world, int32_t pods_col, int32_t* ids, int32_t* admitted, size_t cap,
                          size_t* n_workloads, const kueue_tas_delta** deltas, size_t* n_deltas) {
  return admit_block_impl(c, block, row_words, lens, world, pods_col, ids, admitted, cap, n_workloads, deltas, n_deltas,
                          nullptr);
}

int kueue_tas_admit_block_targets(kueue_tas_ctx* c, const int32_t* block, size_t row_words, const int64_t* lens,
                                  int32_t world, int32_t pods_col, const kueue_tas_delta* target_deltas,
                                  const int64_t* target_off, size_t n_targets, const int32_t* entry_ids,
                                  const int64_t* entry_target_off, const int32_t* entry_targets, size_t n_entries,
                                  int32_t* ids, int32_t* admitted, size_t cap, size_t* n_workloads,
                                  const kueue_tas_delta** deltas, size_t* n_deltas) {
  const AdmitBlockTargets bt{target_deltas, target_off, n_targets, entry_ids, entry_target_off, entry_targets, n_entries};
  return admit_block_impl(c, block, row_words, lens, world, pods_col, ids, admitted, cap, n_workloads, deltas, n_deltas,
                          &bt);
}

// The admission pass over the records in c->d_fits (layout L): phase 1
// (admit_fit0_kernel), the order-free candidates in parallel unless exact,
// then the in-order pass (admit_window_kernel in phases with grid sweeps, or
// the one-wave chain).  Verdicts at L.o_out.
static int admit_run(kueue_tas_ctx* c, const AdmitLayout& L, uint8_t* d, const kueue_tas_fits_term* d_terms, size_t n,
                     size_t n_wl, int32_t pods_col, bool exact) {
  const AdmitView v{reinterpret_cast<const kueue_tas_fits_req*>(d), reinterpret_cast<const int32_t*>(d + L.o_recwl),
                    reinterpret_cast<const int64_t*>(d + L.o_off), reinterpret_cast<int32_t*>(d + L.o_fit0),
                    reinterpret_cast<int32_t*>(d + L.o_out), reinterpret_cast<AdmitRec*>(d + L.o_recs),
                    reinterpret_cast<int32_t*>(d + L.o_dep)};
  return admit_run_view(c, L, d, v, d_terms, n, n_wl, pods_col, exact);
}

// The pass over the n records / n_wl workloads `v` views: the whole call, or
// one run of target-free entries of kueue_tas_admit_targets (record ->
// workload and the offsets relative to the run).  The lists, the per-leaf
// minima, the touched bitmap and the phase state are the layout's, reset here.
static int admit_run_view(kueue_tas_ctx* c, const AdmitLayout& L, uint8_t* d, const AdmitView& v,
                          const kueue_tas_fits_term* d_terms, size_t n, size_t n_wl, int32_t pods_col, bool exact) {
  const size_t nwords = (size_t(c->snap.N) + 31) / 32;
  // the dynamic bitmaps share the workgroup's 64 KB of LDS with the kernel's
  // static arrays (the window kernel's fit / conflict flags and sweep scan)
  static const size_t static_lds[2] = {
      [] {
        hipFuncAttributes a{};
        return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(admit_kernel)) == hipSuccess ? size_t(a.sharedSizeBytes)
                                                                                                  : size_t(16 * 1024);
      }(),
      [] {
        hipFuncAttributes a{};
        return hipFuncGetAttributes(&a, reinterpret_cast<const void*>(admit_window_kernel)) == hipSuccess
                   ? size_t(a.sharedSizeBytes)
                   : size_t(16 * 1024);
      }()};
  const size_t lds_budget = 64 * 1024 - static_lds[c->admit_window ? 1 : 0];
  const bool lds_bits = nwords * 4 <= lds_budget;
  // the windowed kernel's round bitmap beside the touched one: admission chains within a window
  const bool lds_chain = c->admit_window && 2 * nwords * 4 <= lds_budget;
  HIPCHK(c, hipMemsetAsync(d + L.o_bits, 0, nwords * 4, c->stream));
  HIPCHK(c, hipMemsetAsync(d + L.o_state, 0, 256, c->stream));
  // order-free candidates decided in parallel (admit_minc / dep / indep), unless exact
  const bool indep = c->admit_window && !exact && n > 0;
  if (indep) {
    HIPCHK(c, hipMemsetAsync(d + L.o_minc, 0x7f, size_t(c->snap.N) * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(v.dep, 0, n_wl * 4, c->stream));
  }
  const kueue_tas_fits_req* d_reqs = v.reqs;
  if (n) {
    hipLaunchKernelGGL(admit_fit0_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream, c->snap,
                       c->d_usage.p, c->d_usage_present.p, d_reqs, d_terms,
                       v.recwl, int(n), reinterpret_cast<const int64_t*>(d + L.o_total),
                       v.fit0, v.recs,
                       reinterpret_cast<int32_t*>(d + L.o_exact));
    HIPCHK(c, hipGetLastError());
  }
  if (c->admit_window) {  // independent candidates in parallel, the rest windowed (one 1024-thread workgroup)
    const int32_t* recwl = v.recwl;
    const int32_t* fit0d = v.fit0;
    int32_t* depd = v.dep;
    if (indep) {
      const dim3 g(unsigned((n + 255) / 256));
      hipLaunchKernelGGL(admit_minc_kernel, g, dim3(256), 0, c->stream, d_reqs, recwl, int(n), fit0d, c->snap.N,
                         reinterpret_cast<int32_t*>(d + L.o_minc));
      hipLaunchKernelGGL(admit_dep_kernel, g, dim3(256), 0, c->stream, d_reqs, recwl, int(n), fit0d, c->snap.N,
                         reinterpret_cast<const int32_t*>(d + L.o_minc), depd);
      hipLaunchKernelGGL(admit_indep_kernel, g, dim3(256), 0, c->stream, c->snap, c->d_usage.p, c->d_usage_present.p,
                         d_reqs, d_terms, recwl, int(n), fit0d, depd, pods_col, reinterpret_cast<uint32_t*>(d + L.o_bits));
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(admit_todo_kernel, dim3(1), dim3(1024), 0, c->stream, int(n_wl), fit0d, depd, indep ? 0 : 1,
                       v.out, reinterpret_cast<int32_t*>(d + L.o_todo),
                       v.off, reinterpret_cast<int64_t*>(d + L.o_todor));
    HIPCHK(c, hipGetLastError());
    // the window kernel in phases: each stops at a rejection sweep, which the
    // grid runs (a wave per remaining candidate) before the next phase
    // resumes; the last phase sweeps inside its workgroup.  A finished pass
    // leaves the later launches nothing to do.
    int32_t* st = reinterpret_cast<int32_t*>(d + L.o_state);
    int32_t* todo = reinterpret_cast<int32_t*>(d + L.o_todo);
    int64_t* todor = reinterpret_cast<int64_t*>(d + L.o_todor);
    const int phases = c->knobs.admit_grid_sweeps;
    for (int ph = 0; ph < phases; ph++) {
      if (ph > 0) {
        hipLaunchKernelGGL(admit_sweep_kernel, dim3(1024), dim3(256), 0, c->stream, c->snap, c->d_usage.p,
                           c->d_usage_present.p, d_reqs, d_terms, v.recs, fit0d,
                           reinterpret_cast<const uint32_t*>(d + L.o_bits), v.out, todo,
                           todor, st);
        hipLaunchKernelGGL(admit_compact_kernel, dim3(1), dim3(1024), 0, c->stream, todo, todor, st);
      }
      hipLaunchKernelGGL(admit_window_kernel, dim3(1), dim3(64 * kAdmitWindow),
                         lds_chain ? 2 * nwords * 4 : lds_bits ? nwords * 4 : 0, c->stream, c->snap, c->d_usage.p,
                         c->d_usage_present.p, d_reqs, d_terms, v.recs,
                         v.off, int(n_wl), pods_col,
                         v.fit0, reinterpret_cast<const int32_t*>(d + L.o_exact),
                         reinterpret_cast<uint32_t*>(d + L.o_bits), lds_chain ? 2 : lds_bits ? 1 : 0,
                         v.out, todo, todor, st, ph + 1 < phases ? 1 : 0);
      HIPCHK(c, hipGetLastError());
    }
  } else {  // one wave down the chain
    hipLaunchKernelGGL(admit_kernel, dim3(1), dim3(64), lds_bits ? nwords * 4 : 0, c->stream, c->snap, c->d_usage.p,
                       c->d_usage_present.p, d_reqs, d_terms, v.recs,
                       v.off, int(n_wl),
                       pods_col, v.fit0, reinterpret_cast<const int32_t*>(d + L.o_exact),
                       reinterpret_cast<uint32_t*>(d + L.o_bits), lds_bits ? 1 : 0, v.out);
  }
  HIPCHK(c, hipGetLastError());
  c->admit_launches[2] += (n ? 1 : 0) + (c->admit_window ? (indep ? 3 : 0) + 1 + 3 * c->knobs.admit_grid_sweeps - 2 : 1);
  return KUEUE_TAS_OK;
}

int kueue_tas_last_admit_launches(kueue_tas_ctx* c, int64_t* out3) {
  if (!c || !out3) return KUEUE_TAS_EINVAL;
  memcpy(out3, c->admit_launches, sizeof c->admit_launches);
  return KUEUE_TAS_OK;
}

int kueue_tas_last_admit_stats(kueue_tas_ctx* c, int64_t* out3) {
  if (!c || !out3) return KUEUE_TAS_EINVAL;
  memcpy(out3, c->admit_stats, sizeof c->admit_stats);
  return KUEUE_TAS_OK;
}


// The longest candidate list a BestFit-side walk of `ev` can build (its
// select lists' capacity): every domain of a level at or above its requested
// level (findLevelWithFitDomains sorts whole levels, tas_flavor_snapshot.go:
// 1098-1163), and below it the children of the domains chosen one level up,
// at most one chosen domain per pod (updateCountsToMinimum takes a domain
// only while pods remain, :1236-1321); twice that, as the unbounded capacity
// is twice the widest level.  Unconstrained, multi-layer and replacement
// walks keep the unbounded lists.  An overflow still re-runs the chunk
// unbounded (eval_chunk returns ChunkRerun), so the bound costs memory, never results.
static int64_t scratch_bound(const kueue_tas_ctx* c, const DevSnap& s, const DevEval& ev, int64_t full) {
  if (ev.flags & (KUEUE_TAS_F_UNCONSTRAINED | KUEUE_TAS_F_MULTILAYER | KUEUE_TAS_F_DOMAIN)) return full;
  const int r = ev.requested_level;
  if (r < 0 || r >= s.L || c->level_maxfan.size() < size_t(s.L)) return full;
  const int64_t pods = int64_t(std::max(ev.count, 0)) + ((ev.flags & KUEUE_TAS_F_LEADER) ? 1 : 0);
  int64_t top = 0, below = pods;  // whole levels at or above r (find_level's lists are unchecked there)
  for (int l = 0; l < s.L; l++) {
    if (l <= r) top = std::max<int64_t>(top, s.level_size[l]);
    else
      below = std::max<int64_t>(below, std::min<int64_t>(s.level_size[l], std::min<int64_t>(s.level_size[l - 1], pods) *
                                                                               c->level_maxfan[size_t(l - 1)]));
  }
  int64_t lc = std::min(full, 2 * std::max(top, below) + 64);
  if (c->knobs.lcap_test_cap) lc = std::min(lc, std::max(c->knobs.lcap_test_cap, std::min(full, 2 * top + 64)));  // (descent lists only)
  return lc;
}


// ---- eval_chunk: one device chunk of kueue_tas_eval_batch_ptrs, as a sequence
// of stages over an explicit plan.  The host stages decide the ChunkPlan, the
// enqueue stages consume it; the per-class and per-request vectors the stages
// share stay on the context (kept between batches). ----

// The caller's arrays: filled once per batch, narrowed per chunk.
struct ChunkArgs {
  const kueue_tas_eval_req* const* reqs;
  size_t n;
  const int32_t* taint_table;
  size_t taint_table_len;
  int32_t num_taints;
  const kueue_tas_assumed* assumed;
  size_t num_assumed;
  const kueue_tas_affinity_req* aff;
  size_t num_aff;
  const int32_t* aff_vals;
  size_t num_aff_vals;
  kueue_tas_eval_out* out;
  int64_t* offsets;
  int32_t* taint_counts;
  int32_t* res_counts;
  float* ms;
  float* stage_ms;
  // kueue_tas_eval_batch_removals: the requests' removal sets and masks (null: no request has one)
  const int32_t* rset = nullptr;
  const uint64_t* rmask = nullptr;
};

// Byte offsets of the staging arena's segments (h_stage and d_stage alike).
struct ArenaOffsets {
  size_t evals, terms, taint, assumed, aff, affv;
  size_t fill, fchunks, pairs, rep, frun, slot, lrep, fast, leafsel, pidx, bf;
  size_t moff, mem;  // class members in fill order (CSR)
  size_t top;        // rollup_top_kernel's level maxima (INT32_MIN) and per-class arrival counters (0)
  size_t sel;        // BestFit-side select slots' buffers
  size_t rjobs;      // the masked evaluations' RemovalJob records
  size_t rsegs;      // removal_expand_seg_kernel's blocks (int4 each; none without large sets' evaluations)
  size_t fpos;       // last uploaded: the per-position fill records, up to the batch's nfill
  size_t xassumed;   // device only, addressed from `assumed`: the masked evaluations' expanded ranges
};

struct ChunkPlan {
  ArenaOffsets o{};
  size_t nterms = 0;
  int maxt = 1;  // the widest request's term count
  // fill positions (classes), rep/member pairs, fast-LFC table slots, fast-LFC evals, BestFit-side evals, fill
  // chunks, leaf-level select evals, signature runs, single-run chunks (the first nsingle of nfchunks)
  int nfill = 0, npairs = 0, nslots = 0, nfast = 0, nbf = 0, nfchunks = 0, nleafsel = 0, nruns = 0, nsingle = 0;
  uint32_t umask = 0;  // snapshot columns any request reads
  int ucols = 0;
  int nstat_all = 0;       // ExclusionStats fields per class
  bool lds_stats = false;  // the staged fill counts them in LDS
  int64_t full_lcap = 0;   // a list of any level's domains, twice
  int nchunks = 0;         // LFC leaf chunks
  int nblk = 0;            // leaf partials per eval (one per 64-leaf wave)
  int lfc_cur = 0;         // the half of the LFC chunk tables this chunk uses
  size_t res_bytes = 0, res_off_stats = 0, stats_len = 0;  // d_res / h_res: out[n] | stats
  int njobs = 0;           // masked evaluations: first the small sets' (removal_expand_kernel's grid) ...
  int nsmalljobs = 0;      // ... then the large sets', a workgroup per segment each
  int nsegblocks = 0;      // removal_expand_seg_kernel's grid
  int64_t nexpanded = 0;   // assumed records of their ranges
};

// What the fill-path decision yields (enqueue_fill)
struct FillLaunch {
  bool staged_fill = false, pair = false, ragged_pair = false, gl = false, ts = false, cat = false, wide = false;
  unsigned pgx = 0, sgx = 0;  // the pair and staged kernels' grid.x
  unsigned nblk_fill = 0;     // blocks per fill position (stats partials)
};

// eval_chunk's re-run requests to kueue_tas_eval_batch_ptrs (positive: never a KUEUE_TAS_E* code)
enum ChunkRc : int {
  ChunkGrowEntries = 1,  // an assignment exceeded the per-eval device capacity: grow entry_cap and re-run
  ChunkRerun = 2,        // a class hash collision (exact merge) or a select list overflow (unbounded lists)
};

static void trace(kueue_tas_ctx* c, int k) { c->trace[k] = wall_ms(); }

static size_t part_of(size_t n, size_t nparts, size_t i0) {  // the static part starting at request i0
  size_t t = 0;
  while (t + 1 < nparts && ktas_pool::HostPool::part_begin(n, t + 1, nparts) <= i0) t++;
  return t;
}

// The staging arena's typed views
static DevEval* stage_evals(kueue_tas_ctx* c, const ChunkPlan& p) { return reinterpret_cast<DevEval*>(c->h_stage.p + p.o.evals); }
static DevTerm* stage_terms(kueue_tas_ctx* c, const ChunkPlan& p) { return reinterpret_cast<DevTerm*>(c->h_stage.p + p.o.terms); }
static int32_t* stage_ints(kueue_tas_ctx* c, size_t off) { return reinterpret_cast<int32_t*>(c->h_stage.p + off); }
static const int32_t* dev_ints(kueue_tas_ctx* c, size_t off) { return reinterpret_cast<const int32_t*>(c->d_stage.p + off); }

// Phase-1 class keys: the hashes and exact compares of a request's signature
// (terms, overlay, simulateEmpty, leader) and mask (slice parameters,
// selectors, taint row, affinity) over the compiled records.
struct ClassKeys {
  const DevTerm* hterms;
  const kueue_tas_assumed* assumed;
  const kueue_tas_affinity_req* aff;
  const int32_t* aff_vals;
  const int32_t* taint_table;
  size_t taint_table_len;
  int32_t P;  // taint profiles
  int L;      // levels
  // masked evaluations: the record's assumed range is its expanded range on the
  // device; the signature is the request's own records plus (set, mask)
  const DevEval* hev;
  const int32_t* job_of;  // null: the chunk has none
  const RemovalJob* jobs;
  ClassKeys(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p)
      : hterms(stage_terms(c, p)), assumed(a.assumed), aff(a.aff), aff_vals(a.aff_vals), taint_table(a.taint_table),
        taint_table_len(a.taint_table_len), P(c->num_profiles), L(c->snap.L), hev(stage_evals(c, p)),
        job_of(p.njobs ? c->req_job.data() : nullptr),
        jobs(reinterpret_cast<const RemovalJob*>(c->h_stage.p + p.o.rjobs)) {}

  struct Overlay {
    int32_t begin, end;  // the request's own records
    int32_t set;         // -1: no removal
    uint64_t mask;
  };
  Overlay overlay(const DevEval& e) const {
    const int32_t j = job_of ? job_of[&e - hev] : -1;
    if (j < 0) return {e.assumed_begin, e.assumed_end, -1, 0};
    return {jobs[j].own_begin, jobs[j].own_end, jobs[j].set, jobs[j].mask};
  }

  const int32_t* taint_row(const DevEval& e) const {
    return (taint_table && size_t(e.taint_table) + size_t(P) <= taint_table_len) ? taint_table + e.taint_table
                                                                                  : nullptr;
  }
  uint64_t sig_hash(const DevEval& e) const {
    uint64_t h = 1469598103934665603ull;
    auto add = [&](uint64_t v) {
      h ^= v;
      h *= 1099511628211ull;
      h ^= h >> 31;
    };
    add(e.flags & (KUEUE_TAS_F_LEADER | KUEUE_TAS_F_SIMULATE_EMPTY));
    add(uint64_t(uint32_t(e.nreq)) | (uint64_t(uint32_t(e.nlead)) << 32));
    for (int k = 0; k < e.nreq + e.nlead; k++) {
      const DevTerm& t = hterms[k < e.nreq ? e.term_begin + k : e.lead_begin + (k - e.nreq)];
      add(uint64_t(uint32_t(t.col)));
      add(uint64_t(t.val));
    }
    const Overlay ov = overlay(e);
    for (int a = ov.begin; a < ov.end; a++) {
      add(uint64_t(uint32_t(assumed[a].leaf)) | (uint64_t(uint32_t(assumed[a].col)) << 32));
      add(uint64_t(assumed[a].value));
    }
    if (ov.set >= 0) {
      add(0x5e7u | (uint64_t(uint32_t(ov.set)) << 32));
      add(ov.mask);
    }
    return h;
  }
  uint64_t mask_hash(const DevEval& e) const {
    uint64_t h = 0x9e3779b97f4a7c15ull;
    auto add = [&](uint64_t v) {
      h ^= v;
      h *= 1099511628211ull;
      h ^= h >> 29;
    };
    add(uint64_t(uint32_t(e.slice_size)) | (uint64_t(uint32_t(e.slice_level)) << 32));
    for (int l = 0; l < L; l++) add(uint64_t(uint32_t(e.ssal[l])));  // no kernel reads a level >= L
    add(uint64_t(uint32_t(e.nsel)));
    add(uint64_t(uint32_t(e.dom_begin)) | (uint64_t(uint32_t(e.dom_end)) << 32));
    for (int k = 0; k < e.nsel; k++) add(uint64_t(uint32_t(e.sel_col[k])) | (uint64_t(uint32_t(e.sel_val[k])) << 32));
    if (const int32_t* row = taint_row(e))
      for (int p = 0; p < P; p++) add(uint64_t(uint32_t(row[p])));
    auto add_reqs = [&](int32_t rb, int32_t re) {
      for (int k = rb; k < re; k++) {
        const kueue_tas_affinity_req& q = aff[k];
        add(uint64_t(uint32_t(q.term)) | (uint64_t(uint32_t(q.col)) << 32));
        add(uint64_t(uint32_t(q.negate)) | (uint64_t(uint32_t(q.len)) << 32));
        for (int j = 0; j < q.len; j++) add(uint64_t(uint32_t(aff_vals[q.begin + j])));
      }
    };
    if (e.flags & KUEUE_TAS_F_AFFINITY) {
      add(0xaff1u);
      add_reqs(e.aff_begin, e.aff_end);
    }
    if (e.sx_begin >= 0) {
      add(0x5e1eu);
      add_reqs(e.sx_begin, e.sx_end);
    }
    return h;
  }
  // base signature: what the leaf's remaining capacity depends on (a fill chunk shares it)
  bool same_base(const DevEval& x, const DevEval& y) const {
    if ((x.flags ^ y.flags) & (KUEUE_TAS_F_LEADER | KUEUE_TAS_F_SIMULATE_EMPTY)) return false;
    const Overlay ox = overlay(x), oy = overlay(y);
    if (ox.set != oy.set || ox.mask != oy.mask) return false;
    if (ox.end - ox.begin != oy.end - oy.begin) return false;
    for (int a = 0; a < ox.end - ox.begin; a++) {
      const kueue_tas_assumed& p = assumed[ox.begin + a];
      const kueue_tas_assumed& q = assumed[oy.begin + a];
      if (p.leaf != q.leaf || p.col != q.col || p.value != q.value) return false;
    }
    return true;
  }
  bool same_sig(const DevEval& x, const DevEval& y) const {
    if (x.nreq != y.nreq || x.nlead != y.nlead) return false;
    for (int k = 0; k < x.nreq + x.nlead; k++) {
      const DevTerm& a = hterms[k < x.nreq ? x.term_begin + k : x.lead_begin + (k - x.nreq)];
      const DevTerm& b2 = hterms[k < y.nreq ? y.term_begin + k : y.lead_begin + (k - y.nreq)];
      if (a.col != b2.col || a.val != b2.val) return false;
    }
    return same_base(x, y);
  }
  bool same_mask(const DevEval& x, const DevEval& y) const {
    if (x.slice_size != y.slice_size || x.slice_level != y.slice_level || x.nsel != y.nsel) return false;
    if (x.dom_begin != y.dom_begin || x.dom_end != y.dom_end) return false;
    for (int l = 0; l < L; l++)
      if (x.ssal[l] != y.ssal[l]) return false;
    for (int k = 0; k < x.nsel; k++)
      if (x.sel_col[k] != y.sel_col[k] || x.sel_val[k] != y.sel_val[k]) return false;
    const int32_t *rx = taint_row(x), *ry = taint_row(y);
    if ((rx == nullptr) != (ry == nullptr)) return false;
    if (!(rx == nullptr || rx == ry || memcmp(rx, ry, size_t(P) * 4) == 0)) return false;
    auto same_reqs = [&](int32_t xb, int32_t xe, int32_t yb, int32_t ye) {
      if (xe - xb != ye - yb) return false;
      for (int k = 0; k < xe - xb; k++) {
        const kueue_tas_affinity_req& p = aff[xb + k];
        const kueue_tas_affinity_req& q = aff[yb + k];
        if (p.term != q.term || p.col != q.col || p.negate != q.negate || p.len != q.len) return false;
        if (p.begin != q.begin && memcmp(aff_vals + p.begin, aff_vals + q.begin, size_t(p.len) * 4) != 0) return false;
      }
      return true;
    };
    if ((x.sx_begin >= 0) != (y.sx_begin >= 0)) return false;
    if (x.sx_begin >= 0 && !same_reqs(x.sx_begin, x.sx_end, y.sx_begin, y.sx_end)) return false;
    const bool ax = (x.flags & KUEUE_TAS_F_AFFINITY) != 0, ay = (y.flags & KUEUE_TAS_F_AFFINITY) != 0;
    if (ax != ay) return false;
    if (!ax) return true;
    return same_reqs(x.aff_begin, x.aff_end, y.aff_begin, y.aff_end);
  }
  bool fast_lfc(const DevEval& e, int32_t N) const {
    return (e.flags & KUEUE_TAS_F_LFC) != 0 &&
           (e.flags & (KUEUE_TAS_F_LEADER | KUEUE_TAS_F_REQUIRED | KUEUE_TAS_F_MULTILAYER)) == 0 &&
           e.requested_level == L - 1 && e.slice_level == L - 1 && e.slice_size == 1 && e.count >= 0 && N > 0;
  }
};

// Stage 1: validation and term counts over the worker pool (pass A); an error
// is reported for the lowest request index.  Static parts: the same thread
// handles the same requests in passes A and B (and the host layer's compile
// and decode of the same workloads before and after), so their records stay
// in that core's cache.
static int validate_requests(kueue_tas_ctx* c, const ChunkArgs& a) {
  const DevSnap& s = c->snap;
  const kueue_tas_eval_req* const* reqs = a.reqs;
  const size_t n = a.n, num_aff = a.num_aff, num_aff_vals = a.num_aff_vals, num_assumed = a.num_assumed;
  const kueue_tas_assumed* assumed = a.assumed;
  const kueue_tas_affinity_req* aff = a.aff;
  const int32_t* aff_vals = a.aff_vals;
  ktas_pool::HostPool& pool = ktas_pool::HostPool::get();
  const size_t nparts = pool.parts();
  std::vector<int64_t>& toff = c->req_term_off;  // each request's term count (layout_stage: its first term slot)
  toff.assign(n + 1, 0);
  std::vector<int32_t>& chunk_maxt = c->req_chunk_maxt;
  chunk_maxt.assign(std::max<size_t>(nparts, 1), 1);
  std::vector<std::pair<size_t, std::string>>& errs = c->req_errs;  // per part: (first bad request, message)
  errs.assign(std::max<size_t>(nparts, 1), {SIZE_MAX, std::string()});
  std::vector<int32_t>& xlen = c->req_xlen;  // masked evaluations: the expanded range's length, else -1
  int32_t nsets = 0;
  if (a.rset) {
    if (!c->rt_built) return fail(c, KUEUE_TAS_EINVAL, "no removal tables");
    if (c->rt_snap_gen != c->n_loads + c->n_splices) return fail(c, KUEUE_TAS_EINVAL, "removal tables are stale");
    nsets = int32_t(c->rt_set_off.size()) - 1;
    xlen.assign(n, -1);
  }
  auto validate = [&](size_t i, std::string* msg) -> bool {
    const auto& r = *reqs[i];
    if (r.num_req < 0 || r.num_req > KUEUE_TAS_MAX_COLS || r.num_leader_req < 0 || r.num_leader_req > KUEUE_TAS_MAX_COLS)
      return *msg = "num_req", false;
    if (r.slice_size == 0) return *msg = "slice_size == 0 (integer divide by zero)", false;
    if (r.requested_level < 0 || r.requested_level >= s.L || r.slice_level < 0 || r.slice_level >= s.L)
      return *msg = "level out of range", false;
    if (r.num_selectors < 0 || r.num_selectors > KUEUE_TAS_MAX_SELECTORS) return *msg = "num_selectors", false;
    if (r.num_selectors > 0 && s.K == 0) return *msg = "selectors without label columns", false;
    // host-side shape check of every requirement the fill will read
    auto check_reqs = [&](int32_t rb, int32_t re, bool terms, const char* what) -> bool {
      if (rb < 0 || re < rb || size_t(re) > num_aff || (re > rb && (!aff || !aff_vals)))
        return *msg = std::string(what) + " range", false;
      for (int32_t k = rb; k < re; k++) {
        const kueue_tas_affinity_req& q = aff[k];
        if (q.col < KUEUE_TAS_AFFINITY_LEAF || q.col >= s.K || q.begin < 0 || q.len < 0 ||
            size_t(q.begin) + size_t(q.len) > num_aff_vals || (terms && k > rb && q.term < aff[k - 1].term))
          return *msg = std::string(what) + " requirement", false;
        for (int32_t j = 1; j < q.len; j++)
          if (aff_vals[q.begin + j] <= aff_vals[q.begin + j - 1])
            return *msg = std::string(what) + " values not sorted", false;
      }
      return true;
    };
    if ((r.flags & KUEUE_TAS_F_AFFINITY) && !check_reqs(r.affinity_begin, r.affinity_end, true, "affinity")) return false;
    if (r.flags & KUEUE_TAS_F_SELECTOR_EXT) {
      if (r.num_selectors != KUEUE_TAS_MAX_SELECTORS)
        return *msg = "KUEUE_TAS_F_SELECTOR_EXT needs the inline selector pairs filled", false;
      if (!check_reqs(r.selector_begin, r.selector_end, false, "nodeSelector")) return false;
    }
    if (r.assumed_begin < 0 || r.assumed_end < r.assumed_begin || size_t(r.assumed_end) > num_assumed ||
        (r.assumed_end > r.assumed_begin && !assumed))
      return *msg = "assumed range", false;
    for (int32_t a = r.assumed_begin; a < r.assumed_end; a++) {  // sorted by leaf (the fill's binary search)
      const kueue_tas_assumed& x = assumed[a];
      if (x.leaf < 0 || x.leaf >= s.N || x.col < 0 || x.col >= s.R || x.col >= KUEUE_TAS_MAX_COLS ||
          (a > r.assumed_begin && x.leaf < assumed[a - 1].leaf))
        return *msg = "assumed record out of range or not sorted by leaf", false;
    }
    if ((r.flags & KUEUE_TAS_F_DOMAIN) &&
        (r.domain_begin < 0 || r.domain_end < r.domain_begin || r.domain_end > s.N))
      return *msg = "required domain leaf range", false;
    if (a.rset) {  // the removal's range: the request's own records plus the masked positions' records
      xlen[i] = -1;
      const int32_t set = a.rset[i];
      const uint64_t mask = a.rmask[i];
      if (set < -1 || set >= nsets) return *msg = "removal set out of range", false;
      if (set >= 0 && mask) {
        const int32_t c0 = c->rt_cand_off[size_t(set)], nc = c->rt_cand_off[size_t(set) + 1] - c0;
        if (nc < 64 && (mask >> nc)) return *msg = "removal mask beyond the set's candidates", false;
        int64_t len = int64_t(r.assumed_end) - r.assumed_begin;
        for (uint64_t m = mask; m; m &= m - 1) len += c->rt_pos_kept[size_t(c0 + __builtin_ctzll(m))];
        if (len > INT32_MAX) return *msg = "removal range too long", false;
        xlen[i] = int32_t(len);
      }
    }
    return true;
  };
  pool.run_static(n, [&](size_t i0, size_t i1) {
    const size_t ch = part_of(n, nparts, i0);
    std::string msg;
    int32_t mt = 1;  // this part's widest request, stored once (the parts' slots share a cache line)
    for (size_t i = i0; i < i1; i++) {
      const auto& r = *reqs[i];
      if (errs[ch].first == SIZE_MAX && !validate(i, &msg)) errs[ch] = {i, msg};
      toff[i + 1] = int64_t(std::max(r.num_req, 0)) + int64_t(std::max(r.num_leader_req, 0));
      mt = std::max(mt, std::max(r.num_req, r.num_leader_req));
    }
    chunk_maxt[ch] = mt;
  });
  for (auto& e : errs)
    if (e.first != SIZE_MAX) return fail(c, KUEUE_TAS_EINVAL, e.second);
  return KUEUE_TAS_OK;
}

// Stage 2: the term offsets, the staging arena's layout and allocation, and
// the per-request class scratch pass B fills.
static int layout_stage(kueue_tas_ctx* c, const ChunkArgs& a, ChunkPlan& p) {
  const size_t n = a.n;
  std::vector<int64_t>& toff = c->req_term_off;  // first term slot of each request
  for (size_t i = 0; i < n; i++) toff[i + 1] += toff[i];
  p.nterms = size_t(toff[n]);
  p.maxt = 1;
  for (int32_t m : c->req_chunk_maxt) p.maxt = std::max(p.maxt, m);
  size_t stage_bytes = 0;
  auto seg = [&](size_t bytes) {
    const size_t o = stage_bytes;
    stage_bytes += (bytes + 255) / 256 * 256;
    return o;
  };
  ArenaOffsets& o = p.o;  // (in this order: the upload is one copy of [0, fpos + nfill records))
  o.evals = seg(n * sizeof(DevEval)), o.terms = seg(p.nterms * sizeof(DevTerm));
  o.taint = seg(a.taint_table_len * 4), o.assumed = seg(a.num_assumed * sizeof(kueue_tas_assumed));
  o.aff = seg(a.num_aff * sizeof(kueue_tas_affinity_req)), o.affv = seg(a.num_aff_vals * 4);
  o.fill = seg(n * 4), o.fchunks = seg(n * 8), o.pairs = seg(n * 8), o.rep = seg(n * 4);
  o.frun = seg(n * 4);
  o.slot = seg(n * 4), o.lrep = seg(n * 4), o.fast = seg(n * 4), o.leafsel = seg(n * 4);
  o.pidx = seg(n * 4), o.bf = seg(n * 4);
  o.moff = seg((n + 1) * 4), o.mem = seg(n * 4);
  o.top = seg(n * (kMaxLevels + 1) * 4);
  o.sel = seg(n * sizeof(SelSlot));
  // masked evaluations: a job each, and its range of the device's assumed
  // records behind everything uploaded (the host only knows its length)
  p.njobs = p.nsmalljobs = p.nsegblocks = 0;
  p.nexpanded = 0;
  auto large_row = [&](size_t i) {  // request i's set is a large one: its first row of seg_prefix, else -1
    return c->rt_large_seg_off.empty() ? -1 : c->rt_large_seg_off[size_t(a.rset[i])];
  };
  auto set_segments = [&](int32_t set) {
    const int32_t kept = c->rt_set_off[size_t(set) + 1] - c->rt_set_off[size_t(set)];
    return std::max(1, (kept + kRemovalExpandSegment - 1) / kRemovalExpandSegment);
  };
  if (a.rset) {
    c->req_job.assign(n, -1);
    int64_t nseg = 0;
    int nlarge = 0;
    for (size_t i = 0; i < n; i++)
      if (c->req_xlen[i] >= 0) {
        if (large_row(i) >= 0) nlarge++, nseg += set_segments(a.rset[i]);
        else c->req_job[i] = p.nsmalljobs++;
        p.nexpanded += c->req_xlen[i];
      }
    p.njobs = p.nsmalljobs;
    if (nlarge)
      for (size_t i = 0; i < n; i++)
        if (c->req_xlen[i] >= 0 && c->req_job[i] < 0) c->req_job[i] = p.njobs++;
    if (nseg > INT32_MAX / 2) return fail(c, KUEUE_TAS_EOVERFLOW, "too many segments of large removal sets in a chunk");
    p.nsegblocks = int(nseg);
  }
  o.rjobs = seg(size_t(p.njobs) * sizeof(RemovalJob));
  o.rsegs = seg(size_t(p.nsegblocks) * sizeof(int4));
  o.fpos = seg(n * sizeof(FillPos));
  const size_t host_bytes = stage_bytes;
  o.xassumed = seg(size_t(p.nexpanded) * sizeof(kueue_tas_assumed));
  if ((o.xassumed - o.assumed) / sizeof(kueue_tas_assumed) + size_t(p.nexpanded) > size_t(INT32_MAX))
    return fail(c, KUEUE_TAS_EOVERFLOW, "removal ranges exceed the assumed records' index");
  HIPCHK(c, c->h_stage.ensure(host_bytes));
  HIPCHK(c, c->d_stage.ensure(stage_bytes));
  if (p.njobs) {
    RemovalJob* jobs = reinterpret_cast<RemovalJob*>(c->h_stage.p + o.rjobs);
    int4* segs = reinterpret_cast<int4*>(c->h_stage.p + o.rsegs);
    int64_t at = int64_t((o.xassumed - o.assumed) / sizeof(kueue_tas_assumed));
    for (size_t i = 0; i < n; i++) {
      if (c->req_job[i] < 0) continue;
      if (c->req_job[i] >= p.nsmalljobs)  // a large set: (job, first table record, seg_prefix row, last) per segment
        for (int32_t k = 0, ns = set_segments(a.rset[i]), row = large_row(i); k < ns; k++)
          *segs++ = make_int4(c->req_job[i], k * kRemovalExpandSegment, row + k, k == ns - 1);
      RemovalJob& jb = jobs[c->req_job[i]];
      jb.mask = a.rmask[i];
      jb.set = a.rset[i];
      jb.own_begin = a.reqs[i]->assumed_begin;
      jb.own_end = a.reqs[i]->assumed_end;
      jb.out_begin = int32_t(at);
      jb.out_end = int32_t(at += c->req_xlen[i]);
      jb.pad = 0;
    }
  }
  const size_t nparts = ktas_pool::HostPool::get().parts();
  c->req_sig_hash.resize(n);   // signature hash per request
  c->req_cls_hash.resize(n);   // signature x mask hash per request
  c->req_fast.resize(n);       // fast-LFC eligible (ClassKeys::fast_lfc)
  c->req_leaf.resize(n);       // requested level == the leaf level
  c->req_local_cls.resize(n);  // class within the request's static part
  c->part_cls.resize(nparts);
  for (size_t t = 0; t < nparts; t++) {
    PartClasses& pc = c->part_cls[t];
    pc.head.reset(ktas_pool::HostPool::part_begin(n, t + 1, nparts) - ktas_pool::HostPool::part_begin(n, t, nparts));
    pc.rep.clear();
    pc.next.clear();
    pc.hcls.clear();
    pc.hsig.clear();
  }
  return KUEUE_TAS_OK;
}

// Stage 3: requests to device form over the worker pool (pass B): records,
// division magic, class hashes and each static part's classes.
static int compile_requests(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p) {
  const DevSnap& s = c->snap;
  const kueue_tas_eval_req* const* reqs = a.reqs;
  const size_t n = a.n;
  ktas_pool::HostPool& pool = ktas_pool::HostPool::get();
  const size_t nparts = pool.parts();
  DevEval* hev = stage_evals(c, p);
  DevTerm* hterms = stage_terms(c, p);
  const ClassKeys keys(c, a, p);
  const std::vector<int64_t>& toff = c->req_term_off;
  std::vector<std::pair<size_t, std::string>>& errs = c->req_errs;
  std::vector<uint64_t>& h_sig = c->req_sig_hash;
  std::vector<uint64_t>& h_cls = c->req_cls_hash;
  std::vector<uint8_t>& req_fast = c->req_fast;
  std::vector<uint8_t>& req_leaf = c->req_leaf;
  std::vector<int32_t>& req_local_cls = c->req_local_cls;
  if (c->magic_cache.size() < nparts) c->magic_cache.resize(nparts);
  pool.run_static(n, [&](size_t i0, size_t i1) {
    const size_t ch = part_of(n, nparts, i0);
    MagicCache& mc = c->magic_cache[ch];
    for (size_t i = i0; i < i1; i++) {
      const auto& r = *reqs[i];
      DevEval& e = hev[i];  // every field is assigned below (no memset of the record)
      e.req_mask = e.lead_mask = 0;
      e.flags = r.flags;
      e.count = r.count;
      e.slice_size = r.slice_size;
      e.requested_level = r.requested_level;
      e.slice_level = r.slice_level;
      e.nsel = r.num_selectors;
      e.taint_table = r.taint_table;
      e.assumed_begin = r.assumed_begin;
      e.assumed_end = r.assumed_end;
      if (p.njobs && c->req_job[i] >= 0) {  // the expanded range (removal_expand_kernel writes it)
        e.assumed_begin = keys.jobs[c->req_job[i]].out_begin;
        e.assumed_end = keys.jobs[c->req_job[i]].out_end;
      }
      e.aff_begin = r.affinity_begin;
      e.aff_end = r.affinity_end;
      e.dom_begin = (r.flags & KUEUE_TAS_F_DOMAIN) ? r.domain_begin : -1;
      e.dom_end = (r.flags & KUEUE_TAS_F_DOMAIN) ? r.domain_end : -1;
      const bool sx = (r.flags & KUEUE_TAS_F_SELECTOR_EXT) != 0 && r.selector_end > r.selector_begin;
      e.sx_begin = sx ? r.selector_begin : -1;
      e.sx_end = sx ? r.selector_end : -1;
      e.num_layers = std::min(r.num_layers, KUEUE_TAS_MAX_LAYERS);
      for (int k = 0; k < KUEUE_TAS_MAX_LAYERS; k++) {
        e.layer_level[k] = r.layer_level[k];
        e.layer_size[k] = r.layer_size[k] == 0 ? 1 : r.layer_size[k];
      }
      for (int l = 0; l < KUEUE_TAS_MAX_LEVELS; l++) e.ssal[l] = r.slice_size_at_level[l];
      for (int k = 0; k < KUEUE_TAS_MAX_SELECTORS; k++) {
        e.sel_col[k] = r.sel_col[k];
        e.sel_val[k] = r.sel_val[k];
      }
      int64_t tp = toff[i];
      auto add_terms = [&](const int32_t* cols, const int64_t* vals, int cnt, uint32_t* mask) -> int {
        int prev = -1;
        for (int k = 0; k < cnt; k++) {
          if (cols[k] < 0 || cols[k] >= s.R || cols[k] <= prev) return -1;
          prev = cols[k];
          DevTerm& t = hterms[tp++];
          t.col = cols[k];
          t.val = vals[k];
          t.neg = vals[k] < 0;
          uint64_t mag = vals[k] < 0 ? (0ull - uint64_t(vals[k])) : uint64_t(vals[k]);
          if (mag) {
            compute_magic(mag, &t, mc);
          } else {
            t.magic = 0;
            t.shift = t.add = t.pow2 = 0;
          }
          *mask |= 1u << cols[k];
        }
        return 0;
      };
      e.term_begin = int32_t(tp);
      e.nreq = r.num_req;
      if (add_terms(r.req_col, r.req_val, r.num_req, &e.req_mask)) {
        if (errs[ch].first == SIZE_MAX) errs[ch] = {i, "req columns"};
        continue;
      }
      e.lead_begin = int32_t(tp);
      e.nlead = (r.flags & KUEUE_TAS_F_LEADER) ? r.num_leader_req : 0;
      if (add_terms(r.leader_col, r.leader_val, e.nlead, &e.lead_mask)) {
        if (errs[ch].first == SIZE_MAX) errs[ch] = {i, "leader columns"};
        continue;
      }
      h_sig[i] = keys.sig_hash(e);
      h_cls[i] = h_sig[i] ^ (keys.mask_hash(e) * 0xff51afd7ed558ccdull);
      req_fast[i] = keys.fast_lfc(e, s.N) ? 1 : 0;
      req_leaf[i] = e.requested_level == s.L - 1 ? 1 : 0;
      // this part's classes (first member in request order), exact compare on a hash hit
      PartClasses& pc = c->part_cls[ch];
      int32_t k = -1;
      int32_t* head = pc.head.find(h_cls[i]);
      for (int32_t q = *head; q >= 0; q = pc.next[size_t(q)]) {
        const DevEval& r = hev[pc.rep[size_t(q)]];
        if (keys.same_sig(e, r) && keys.same_mask(e, r)) {
          k = q;
          break;
        }
      }
      if (k < 0) {
        k = int32_t(pc.rep.size());
        pc.rep.push_back(int32_t(i));
        pc.next.push_back(*head);
        pc.hcls.push_back(h_cls[i]);
        pc.hsig.push_back(h_sig[i]);
        *head = k;
      }
      req_local_cls[i] = k;
    }
  });
  for (auto& e : errs)
    if (e.first != SIZE_MAX) return fail(c, KUEUE_TAS_EINVAL, e.second);
  return KUEUE_TAS_OK;
}

// the caller's tables into the staging arena
static void copy_tables(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p) {
  uint8_t* hs = c->h_stage.p;
  if (a.taint_table_len) memcpy(hs + p.o.taint, a.taint_table, a.taint_table_len * 4);
  if (a.num_assumed) memcpy(hs + p.o.assumed, a.assumed, a.num_assumed * sizeof(kueue_tas_assumed));
  if (a.num_aff) memcpy(hs + p.o.aff, a.aff, a.num_aff * sizeof(kueue_tas_affinity_req));
  if (a.num_aff_vals) memcpy(hs + p.o.affv, a.aff_vals, a.num_aff_vals * 4);
}

// Phase-1 classes (stages 4 to 6): evals with identical phase-1 inputs
// (request terms, masks, overlay, slice parameters) get identical counters;
// phase 1 runs once per class (its representative).  Every member's select
// reads the class counters and keeps its mutations in a private overlay;
// duplicates only get the rep's exclusion stats.  A class's request signature
// (terms, overlay, simulateEmpty, leader) decides which classes share a fill
// chunk.

// Stage 4: the parts' classes merged into the chunk's classes and signatures
// (cls_rep, cls_sig, sig_rep) and each eval's class (cls_of): open hash chains
// on the 64-bit (signature, mask) hash, exact compare on the rep.
static void merge_classes(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p) {
  const size_t n = a.n;
  const size_t nparts = ktas_pool::HostPool::get().parts();
  const DevEval* hev = stage_evals(c, p);
  const ClassKeys keys(c, a, p);
  std::vector<int32_t>& cls_rep = c->cls_rep;    // first member of each class
  std::vector<int32_t>& cls_sig = c->cls_sig;    // signature id of each class
  std::vector<int32_t>& cls_of = c->cls_of;      // class of each eval
  std::vector<int32_t>& sig_rep = c->sig_rep;    // first eval of each signature
  cls_rep.clear();
  cls_sig.clear();
  sig_rep.clear();
  cls_of.assign(n, -1);
  FlatMap& cls_head = c->cls_head;
  FlatMap& sig_head = c->sig_head;
  cls_head.reset(n);
  sig_head.reset(n);
  std::vector<int32_t>& cls_next = c->cls_next;  // chain of classes with the same hash
  std::vector<int32_t>& sig_next = c->sig_next;
  cls_next.clear();
  sig_next.clear();
  // the parts' classes merged in part order: a global class is numbered by
  // its first member, as a serial pass over the requests would number it
  std::vector<int32_t>& part_map = c->part_map;  // (part, local class) -> global class
  std::vector<size_t>& part_base = c->part_base;
  part_base.assign(nparts + 1, 0);
  for (size_t t = 0; t < nparts; t++) part_base[t + 1] = part_base[t] + c->part_cls[t].rep.size();
  part_map.assign(part_base[nparts], -1);
  // Speculative merge: parts' classes with equal 64-bit hashes are taken
  // as equal here, and verified exactly while the device runs (verify_merge;
  // the exact compares read other cores' records: ~0.2 us each on the
  // critical path); a hash collision re-runs the chunk with the exact merge
  // below (exact_merge)
  if (!c->exact_merge) {
    for (size_t t = 0; t < nparts; t++) {
      const PartClasses& pc = c->part_cls[t];
      for (size_t j = 0; j < pc.rep.size(); j++) {
        int32_t* head = cls_head.find(c->collide_test ? 0 : pc.hcls[j]);
        int32_t k = *head;
        if (k < 0) {
          k = int32_t(cls_rep.size());
          cls_rep.push_back(pc.rep[j]);
          cls_next.push_back(-1);
          *head = k;
          int32_t* shead = sig_head.find(c->collide_test ? 0 : pc.hsig[j]);
          if (*shead < 0) {
            *shead = int32_t(sig_rep.size());
            sig_rep.push_back(pc.rep[j]);
            sig_next.push_back(-1);
          }
          cls_sig.push_back(*shead);
        }
        part_map[part_base[t] + j] = k;
      }
    }
  }
  for (size_t t = 0; t < nparts && c->exact_merge; t++)
    for (size_t j = 0; j < c->part_cls[t].rep.size(); j++) {
      const size_t i = size_t(c->part_cls[t].rep[j]);
      const DevEval& e = hev[i];
      int32_t k = -1;
      int32_t* head = cls_head.find(c->req_cls_hash[i]);
      for (int32_t q = *head; q >= 0; q = cls_next[size_t(q)]) {
        const DevEval& r = hev[cls_rep[size_t(q)]];
        if (keys.same_sig(e, r) && keys.same_mask(e, r)) {
          k = q;
          break;
        }
      }
      if (k < 0) {
        k = int32_t(cls_rep.size());
        cls_rep.push_back(int32_t(i));
        cls_next.push_back(*head);
        *head = k;
        int32_t sg = -1;
        int32_t* shead = sig_head.find(c->req_sig_hash[i]);
        for (int32_t q = *shead; q >= 0; q = sig_next[size_t(q)])
          if (keys.same_sig(e, hev[sig_rep[size_t(q)]])) {
            sg = q;
            break;
          }
        if (sg < 0) {
          sg = int32_t(sig_rep.size());
          sig_rep.push_back(int32_t(i));
          sig_next.push_back(*shead);
          *shead = sg;
        }
        cls_sig.push_back(sg);
      }
      part_map[part_base[t] + j] = k;
    }
  for (size_t t = 0; t < nparts; t++)
    for (size_t i = ktas_pool::HostPool::part_begin(n, t, nparts); i < ktas_pool::HostPool::part_begin(n, t + 1, nparts); i++)
      cls_of[i] = part_map[part_base[t] + size_t(c->req_local_cls[i])];
}

// Stage 5: each class's representative (the first fast-LFC member if any: its
// class gets an LFC table slot) and the per-eval index lists of the arena.
static void assign_reps_and_slots(kueue_tas_ctx* c, const ChunkArgs& a, ChunkPlan& p) {
  const size_t n = a.n;
  const std::vector<int32_t>& cls_of = c->cls_of;
  const std::vector<uint8_t>& req_fast = c->req_fast;
  const std::vector<uint8_t>& req_leaf = c->req_leaf;
  int32_t* h_pairs = stage_ints(c, p.o.pairs);
  int32_t* h_rep = stage_ints(c, p.o.rep);
  int32_t* h_slot = stage_ints(c, p.o.slot);
  int32_t* h_lrep = stage_ints(c, p.o.lrep);
  int32_t* h_fast = stage_ints(c, p.o.fast);
  int32_t* h_leafsel = stage_ints(c, p.o.leafsel);
  int32_t* h_pidx = stage_ints(c, p.o.pidx);  // eval -> row of its leaf partials, -1
  int32_t* h_bf = stage_ints(c, p.o.bf);      // evals selected on the main stream
  int nslots = 0, nfast = 0, nbf = 0, npairs = 0, nleafsel = 0;
  const int ncls = int(c->cls_rep.size());
  std::vector<int32_t>& rep = c->cls_fastrep;
  rep.assign(size_t(ncls), -1);
  for (size_t i = 0; i < n; i++) {
    const int32_t k = cls_of[i];
    if (rep[size_t(k)] < 0 && req_fast[i]) rep[size_t(k)] = int32_t(i);
  }
  std::vector<int32_t>& slot_of = c->cls_slot;
  slot_of.assign(size_t(ncls), -1);
  for (int k = 0; k < ncls; k++) {
    if (rep[size_t(k)] >= 0) {
      slot_of[size_t(k)] = nslots;
      h_lrep[nslots++] = rep[size_t(k)];
    } else {
      rep[size_t(k)] = c->cls_rep[size_t(k)];
    }
  }
  for (size_t i = 0; i < n; i++) {
    const int32_t k = cls_of[i], r = rep[size_t(k)];
    const bool fast = slot_of[size_t(k)] >= 0 && req_fast[i];
    h_rep[i] = r;
    h_slot[i] = fast ? slot_of[size_t(k)] : -1;
    if (fast) h_fast[nfast++] = int32_t(i);
    else h_bf[nbf++] = int32_t(i);
    if (int32_t(i) != r) {
      h_pairs[2 * npairs] = r;
      h_pairs[2 * npairs + 1] = ~int32_t(i);  // exclusion stats only
      npairs++;
    }
    h_pidx[i] = -1;
    if (req_leaf[i] && !fast) {
      h_pidx[i] = nleafsel;
      h_leafsel[nleafsel++] = int32_t(i);
    }
  }
  p.nslots = nslots;
  p.nfast = nfast;
  p.nbf = nbf;
  p.npairs = npairs;
  p.nleafsel = nleafsel;
}

// Stage 6: fill chunks: classes ordered by (base signature, signature),
// <= kEvalsPerFillBlock per chunk, one base signature each (the leaf's
// remaining capacity is shared); a run of one signature inside a chunk shares
// the CountIn.  Trace points 7 (order) and 8 (member lists) lie inside.
static void order_fill_chunks(kueue_tas_ctx* c, const ChunkArgs& a, ChunkPlan& p) {
  const size_t n = a.n;
  const DevEval* hev = stage_evals(c, p);
  const ClassKeys keys(c, a, p);
  const std::vector<int32_t>& cls_sig = c->cls_sig;
  const std::vector<int32_t>& cls_of = c->cls_of;
  const std::vector<int32_t>& sig_rep = c->sig_rep;
  const std::vector<int32_t>& rep = c->cls_fastrep;
  const std::vector<int32_t>& slot_of = c->cls_slot;
  int32_t* h_fill = stage_ints(c, p.o.fill);
  int32_t* h_fchunks = stage_ints(c, p.o.fchunks);
  int32_t* h_rep = stage_ints(c, p.o.rep);
  int32_t* h_lrep = stage_ints(c, p.o.lrep);
  const int ncls = int(c->cls_rep.size());
  int nfchunks = 0, nruns = 0;
  const int nsig = int(sig_rep.size());
  std::vector<int32_t>& sig_base = c->sig_base;
  sig_base.assign(size_t(nsig), -1);
  {
    std::vector<int32_t>& base_rep = c->base_rep;
    base_rep.clear();
    for (int g = 0; g < nsig; g++) {
      const DevEval& e = hev[sig_rep[size_t(g)]];
      for (size_t q = 0; q < base_rep.size() && sig_base[size_t(g)] < 0; q++)
        if (keys.same_base(e, hev[base_rep[q]])) sig_base[size_t(g)] = int32_t(q);
      if (sig_base[size_t(g)] < 0) {
        sig_base[size_t(g)] = int32_t(base_rep.size());
        base_rep.push_back(sig_rep[size_t(g)]);
      }
      if (base_rep.size() > 64) {  // many distinct bases (assumed usage per eval): no sharing to look for
        for (int h = g + 1; h < nsig; h++) sig_base[size_t(h)] = int32_t(base_rep.size()) + (h - g - 1);
        break;
      }
    }
  }
  std::vector<int32_t>& order = c->cls_order;
  order.resize(size_t(ncls));
  for (int k = 0; k < ncls; k++) order[size_t(k)] = k;
  std::vector<int32_t>& sig_ncls = c->sig_ncls;  // classes per signature: small ones pack together
  sig_ncls.assign(size_t(nsig), 0);
  for (int k = 0; k < ncls; k++) sig_ncls[size_t(cls_sig[size_t(k)])]++;
  auto small = [&](int32_t sg) { return sig_ncls[size_t(sg)] < kEvalsPerFillBlock / 2; };
  std::stable_sort(order.begin(), order.end(), [&](int32_t k1, int32_t k2) {
    const int32_t sa = cls_sig[size_t(k1)], sb = cls_sig[size_t(k2)];
    const int32_t ba = sig_base[size_t(sa)], bb = sig_base[size_t(sb)];
    if (ba != bb) return ba < bb;
    if (small(sa) != small(sb)) return !small(sa);
    return sa < sb;
  });
  trace(c, 7);
  for (int k = 0; k < ncls; k++) h_fill[k] = rep[size_t(order[size_t(k)])];
  p.nfill = ncls;
  {  // members other than the rep, grouped by fill position (stats written by the reduce)
    int32_t* h_moff = stage_ints(c, p.o.moff);
    int32_t* h_mem = stage_ints(c, p.o.mem);
    std::vector<int32_t>& pos = c->cls_pos;
    pos.resize(size_t(ncls));
    for (int k = 0; k < ncls; k++) pos[size_t(order[size_t(k)])] = k;
    for (int k = 0; k <= ncls; k++) h_moff[k] = 0;
    for (size_t i = 0; i < n; i++)
      if (int32_t(i) != rep[size_t(cls_of[i])]) h_moff[pos[size_t(cls_of[i])] + 1]++;
    for (int k = 0; k < ncls; k++) h_moff[k + 1] += h_moff[k];
    std::vector<int32_t>& cur = c->cls_cur;
    cur.assign(h_moff, h_moff + ncls);
    for (size_t i = 0; i < n; i++)
      if (int32_t(i) != rep[size_t(cls_of[i])]) h_mem[cur[size_t(pos[size_t(cls_of[i])])]++] = int32_t(i);
  }
  {  // counters are stored per class, row = fill position: evals and LFC tables refer to their class's row
    const std::vector<int32_t>& pos = c->cls_pos;
    for (size_t i = 0; i < n; i++) h_rep[i] = pos[size_t(cls_of[i])];
    for (int k = 0; k < ncls; k++)
      if (slot_of[size_t(k)] >= 0) h_lrep[slot_of[size_t(k)]] = pos[size_t(k)];
  }
  trace(c, 8);
  int32_t* h_frun = stage_ints(c, p.o.frun);
  // a signature with at least half a chunk of classes gets chunks of its
  // own (one run: CountIn before the eval loop); the smaller ones of a base
  // share packed chunks (several runs).  Single-run chunks first.
  std::vector<int32_t>& packed = c->cls_packed;  // [start, len) signature runs left for packing
  packed.clear();
  for (int k = 0; k < ncls;) {
    const int32_t sg = cls_sig[size_t(order[size_t(k)])];
    int e = k + 1;
    while (e < ncls && cls_sig[size_t(order[size_t(e)])] == sg) e++;
    if (e - k >= kEvalsPerFillBlock / 2) {
      for (int q = k; q < e; q += kEvalsPerFillBlock) {
        h_fchunks[2 * nfchunks] = q;
        h_fchunks[2 * nfchunks + 1] = std::min(kEvalsPerFillBlock, e - q);
        nfchunks++;
        for (int r = q; r < q + h_fchunks[2 * nfchunks - 1]; r++) h_frun[r] = nruns;
        nruns++;
      }
    } else {
      packed.push_back(k);
      packed.push_back(e - k);
    }
    k = e;
  }
  p.nsingle = nfchunks;
  for (size_t i = 0; i < packed.size();) {  // runs of one base, in order, up to a chunk each
    const int32_t k0 = packed[i];
    const int32_t base = sig_base[size_t(cls_sig[size_t(order[size_t(k0)])])];
    int len = 0;
    h_fchunks[2 * nfchunks] = k0;
    while (i < packed.size() && len + packed[i + 1] <= kEvalsPerFillBlock && packed[i] == k0 + len &&
           sig_base[size_t(cls_sig[size_t(order[size_t(packed[i])])])] == base) {
      for (int r = packed[i]; r < packed[i] + packed[i + 1]; r++) h_frun[r] = nruns;
      nruns++;
      len += packed[i + 1];
      i += 2;
    }
    h_fchunks[2 * nfchunks + 1] = len;
    nfchunks++;
  }
  p.nfchunks = nfchunks;
  p.nruns = nruns;
}

// Stage 7: every device buffer the chunk's kernels use, sized by the plan: the
// class counter rows, the select slot groups and tag epoch, the result
// buffers, the LFC tables and the leaf partials (and the chunk's record for
// kueue_tas_last_counters).
static int size_device_buffers(kueue_tas_ctx* c, const ChunkArgs& a, ChunkPlan& p) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  uint8_t* hs = c->h_stage.p;
  const DevEval* hev = stage_evals(c, p);
  const int32_t* h_fill = stage_ints(c, p.o.fill);
  const int32_t* h_rep = stage_ints(c, p.o.rep);
  const int32_t* h_bf = stage_ints(c, p.o.bf);
  const int nfill = p.nfill, nbf = p.nbf, nslots = p.nslots;
  c->chunk_rep.assign(h_rep, h_rep + n);
  c->chunk_leader.resize(n);
  for (size_t i = 0; i < n; i++) c->chunk_leader[i] = (hev[i].flags & KUEUE_TAS_F_LEADER) ? 1 : 0;
  c->chunk_alias.assign(n, 0);  // filled with the fill records (build_fill_records)
  const int64_t SD = s.SD;
  const int64_t full_lcap = p.full_lcap = int64_t(c->maxD) * 2 + 64;
  const int nchunks = p.nchunks = (s.N + kLfcChunk - 1) / kLfcChunk;
  {  // one row per class (fill position), sized by its kind (FillEvalParams::ctr_row)
    c->ctr_row_off.resize(size_t(std::max(nfill, 1)) + 1);
    int64_t at = 0;
    for (int pos = 0; pos < nfill; pos++) {
      const DevEval& ev = hev[h_fill[pos]];
      c->ctr_row_off[size_t(pos)] = int32_t(at);
      at += (ev.flags & KUEUE_TAS_F_LEADER) ? 5 : simple_class(ev, s.L) ? 1 : 2;
    }
    if (at * SD > (int64_t(1) << 40)) return fail(c, KUEUE_TAS_EINVAL, "class rows exceed the device");
    c->ctr_row_off[size_t(nfill)] = int32_t(at);
    HIPCHK(c, c->d_counters.ensure(size_t(std::max<int64_t>(at, 1)) * size_t(SD)));
  }
  // overlay, tags and scratch lists per BestFit-side select slot (fast-LFC
  // evals never mutate or walk lists): each slot's lists bounded by what its
  // walk can reach (scratch_bound), its overlay by its kind (2 fields, 5 with
  // a leader); slots run in groups whose buffers fit Knobs::phase2_budget,
  // reusing one group's buffers (a fresh tag epoch per group)
  SelSlot* hsel = reinterpret_cast<SelSlot*>(hs + p.o.sel);
  std::vector<int32_t>& groups = c->sel_groups;
  groups.assign(1, 0);
  {
    int64_t g_scr = 0, g_ov = 0, max_scr = 2, max_ov = 1;
    int32_t g_tag = 0, max_tag = 1;
    for (int k = 0; k < nbf; k++) {
      const DevEval& ev = hev[h_bf[k]];
      const int64_t lc = (c->scratch_full || !c->knobs.scratch_bounded) ? full_lcap : scratch_bound(c, s, ev, full_lcap);
      const int64_t ovf = (ev.flags & KUEUE_TAS_F_LEADER) ? 5 : 2;
      const int64_t bytes = lc * 48 + (ovf + 1) * SD * 4;
      if (g_tag > 0 && g_scr * 8 + g_ov * 4 + int64_t(g_tag) * SD * 4 + bytes > c->knobs.phase2_budget) {
        groups.push_back(k);
        g_scr = g_ov = 0;
        g_tag = 0;
      }
      hsel[k] = SelSlot{g_scr, g_ov, g_tag, int32_t(lc)};
      g_scr += 6 * lc;
      g_ov += ovf * SD;
      g_tag++;
      max_scr = std::max(max_scr, g_scr);
      max_ov = std::max(max_ov, g_ov);
      max_tag = std::max(max_tag, g_tag);
    }
    groups.push_back(nbf);
    HIPCHK(c, c->d_scratch.ensure(size_t(max_scr)));
    HIPCHK(c, c->d_overlay.ensure(size_t(max_ov)));
    const int ngroups = int(groups.size()) - 1;
    if (c->d_tags.n < size_t(max_tag) * size_t(SD) || c->tag_epoch + ngroups >= 0x7ffffff0) {  // fresh tags: nothing owned
      HIPCHK(c, c->d_tags.ensure(size_t(max_tag) * size_t(SD)));
      HIPCHK(c, hipMemsetAsync(c->d_tags.p, 0, c->d_tags.n * 4, c->stream));
      c->tag_epoch = 0;
    }
  }
  c->tag_epoch++;
  const size_t nt = size_t(std::max(a.num_taints, 0));
  p.stats_len = n * nt + n * size_t(s.R) + 3 * n;  // taints | resources | nodeSelector | affinity | topologyDomain
  p.res_off_stats = (n * sizeof(kueue_tas_eval_out) + 15) / 16 * 16;
  p.res_bytes = p.res_off_stats + p.stats_len * 4;
  HIPCHK(c, c->d_res.ensure(p.res_bytes));
  HIPCHK(c, c->h_res.ensure(p.res_bytes));
  HIPCHK(c, c->h_res2.ensure(n));
  c->res_out_h = reinterpret_cast<kueue_tas_eval_out*>(c->h_res.p);
  c->res_stats_h = reinterpret_cast<int32_t*>(c->h_res.p + p.res_off_stats);
  // ExclusionStats are fully written by the fill's reduce (class reps) and the
  // replication (other members) when the staged fill counts them in LDS
  p.umask = 0;
  for (size_t i = 0; i < n; i++) p.umask |= hev[i].req_mask | hev[i].lead_mask;
  p.ucols = __builtin_popcount(p.umask);
  p.nstat_all = kStatFixed + int(nt) + s.R;
  p.lds_stats = s.N > 0 && p.nfchunks > 0 && p.ucols <= 8 && p.nstat_all <= kMaxFillStats;
  HIPCHK(c, c->d_lfc_jobs.ensure(n));
  HIPCHK(c, c->d_lfc_items.ensure(size_t(std::max(p.nfast, 1)) * size_t(std::max(nchunks, 1)) + 1));
  // chunk counts and overflow sums in two halves used by alternate batches:
  // the fill accumulates into zeroed tables (DevBatch::lfc_fill), and a
  // half's zeroing runs on stream2 during the batch that does not use it
  const size_t lfc_need = size_t(std::max(nslots * nchunks, 1));
  if (lfc_need > c->lfc_half) {
    c->lfc_half = lfc_need + lfc_need / 4;
    HIPCHK(c, c->d_lfc_ch.ensure(2 * c->lfc_half * kLfcBins));
    HIPCHK(c, c->d_lfc_ovs.ensure(2 * c->lfc_half));
    c->lfc_dirty[0] = c->lfc_dirty[1] = true;
  }
  p.lfc_cur = c->lfc_parity;
  HIPCHK(c, c->d_lfc_cp.ensure(size_t(std::max(nslots * nchunks, 1)) * kLfcBins));
  HIPCHK(c, c->d_lfc_tot.ensure(size_t(std::max(nslots, 1)) * kLfcBins));
  HIPCHK(c, c->d_lfc_ovtot.ensure(size_t(std::max(nslots, 1))));
  HIPCHK(c, c->d_lfc_u8.ensure(size_t(std::max(nslots, 1)) * size_t(std::max(nchunks, 1)) * kLfcChunk));
  p.nblk = (s.N + 255) / 256 * 4;
  HIPCHK(c, c->d_partials.ensure(size_t(std::max(p.nleafsel, 1)) * size_t(std::max(p.nblk, 1))));
  if (c->fused_top) {  // rollup_top_kernel's initial level maxima and arrival counters
    int32_t* t = stage_ints(c, p.o.top);
    for (size_t i = 0; i < size_t(nfill) * kMaxLevels; i++) t[i] = INT32_MIN;
    for (size_t i = 0; i < size_t(nfill); i++) t[n * kMaxLevels + i] = 0;
  }
  return KUEUE_TAS_OK;
}

// Stage 8: the per-eval entry regions [n][entry_cap] (leaf, count) pairs in
// pinned, device-mapped host memory: select / lfc_emit write the pairs the
// host reads after the batch's one sync (no offsets/pack kernels, no entries
// D2H); with leaf tags on, one tag per pair in a region of the same layout.
//
// Invariants, in int32 units of ent_host (a pair is two) and uint64 units of
// tag_host (one per pair), with n regions of entry_cap pairs claimed by this
// chunk (claim_entry_regions adds them to ent_used once the chunk is kept):
//   ent_used + n * entry_cap * 2 <= ent_cap
//   (ent_used + n * entry_cap * 2) / 2 <= tag_cap   (tag_cap >= ent_cap / 2)
// A region that grows keeps the batch's earlier chunks' pairs ([0, ent_used)).
static int ensure_entry_regions(kueue_tas_ctx* c, const ChunkArgs& a) {
  const size_t need_ints = c->ent_used + a.n * size_t(c->entry_cap) * 2;
  if (need_ints > c->ent_cap) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t cap = std::max<size_t>(need_ints, 2 * c->ent_cap);
    int32_t* q = nullptr;
    HIPCHK(c, hipHostMalloc(&q, cap * 4, hipHostMallocMapped | hipHostMallocCoherent));
    if (c->ent_used) memcpy(q, c->ent_host, c->ent_used * 4);
    if (c->ent_host) (void)hipHostFree(c->ent_host);
    c->ent_host = q;
    c->ent_cap = cap;
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->ent_dev), q, 0));
  }
  if (c->leaf_tags_on && c->tag_cap < c->ent_cap / 2) {  // one tag per entry pair, same layout
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t cap = c->ent_cap / 2;
    uint64_t* q = nullptr;
    HIPCHK(c, hipHostMalloc(&q, cap * 8, hipHostMallocMapped | hipHostMallocCoherent));
    if (c->ent_used && c->tag_host) memcpy(q, c->tag_host, c->ent_used / 2 * 8);
    if (c->tag_host) (void)hipHostFree(c->tag_host);
    c->tag_host = q;
    c->tag_cap = cap;
    HIPCHK(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->tag_dev), q, 0));
  }
  if (c->leaf_tags_on) c->fill_paths |= KUEUE_TAS_PATH_ENTRY_TAGS;
  c->snap.leaf_tag = c->leaf_tags_on ? c->d_leaf_tags.p : nullptr;
  c->snap.tag_out = c->leaf_tags_on ? c->tag_dev : nullptr;
  c->snap.ent_base = c->ent_dev;
  return KUEUE_TAS_OK;
}

// Stage 9: fill_pair_kernel's per-position records in fill order (FillPos),
// with the packed nodeSelector compare; chunk_alias and last_alias_fills.
static void build_fill_records(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const int32_t* taint_table = a.taint_table;
  const size_t taint_table_len = a.taint_table_len;
  const DevEval* hev = stage_evals(c, p);
  const DevTerm* hterms = stage_terms(c, p);
  const int ucols = p.ucols, nfchunks = p.nfchunks, nfill = p.nfill;
  FillPos* fp = reinterpret_cast<FillPos*>(c->h_stage.p + p.o.fpos);
  const int32_t* h_fill = stage_ints(c, p.o.fill);
  const int32_t* h_fch = stage_ints(c, p.o.fchunks);
  const int32_t* h_frun = stage_ints(c, p.o.frun);
  const int nsw = ucols <= 4 ? 4 : ucols <= 5 ? 5 : 8;  // the launch's NS: worker terms [0, NS), leader terms [NS, 2 NS)
  for (int ch = 0; ch < nfchunks; ch++) {
    const int e0 = h_fch[2 * ch], ne = h_fch[2 * ch + 1];
    const DevEval& base = hev[h_fill[e0]];
    for (int t = 0; t < ne; t++) {
      const int pos = e0 + t;
      const DevEval& ev = hev[h_fill[pos]];
      FillPos& r = fp[pos];
      memset(&r, 0, sizeof r);
      FillEvalParams& P = r.p;
      P.eid = h_fill[pos];
      P.lfc_slot = c->cls_slot[size_t(c->cls_order[size_t(pos)])];  // fast-LFC table slot, -1: none
      P.taint_off = ev.taint_table;
      P.nsel = ev.nsel;
      P.slice_size = ev.slice_size;
      P.slice_level = ev.slice_level;
      P.inner = ev.ssal[s.L - 1];
      const bool aff = (ev.flags & KUEUE_TAS_F_AFFINITY) != 0;
      P.aff_begin = aff ? ev.aff_begin : -1;
      P.aff_end = aff ? ev.aff_end : -1;
      P.dom_begin = ev.dom_begin;
      P.dom_end = ev.dom_end;
      for (int k = 0; k < KUEUE_TAS_MAX_SELECTORS; k++) {
        P.sel_col[k] = ev.sel_col[k];
        P.sel_val[k] = ev.sel_val[k];
        if (k < ev.nsel && ev.sel_col[k] >= kStagedLabels) P.sel_far = 1;
      }
      P.sx_begin = ev.sx_begin;
      P.sx_end = ev.sx_end;
      P.ss_alias = simple_class(ev, s.L) ? 1 : 0;
      P.ctr_row = c->ctr_row_off[size_t(pos)];
      if (ev.sx_begin >= 0) P.sel_far = 1;
      {  // the packed nodeSelector compare (FillEvalParams::sel_fast)
        uint32_t m[2] = {0u, 0u}, w[2] = {0u, 0u};
        bool fast = c->labels16 && !P.sel_far, never = false;
        for (int k = 0; k < ev.nsel && fast; k++) {
          const int col = ev.sel_col[k];
          const uint32_t sh = uint32_t(col & 1) * 16u;
          const uint32_t fm = 0xffffu << sh;
          if (col < 0 || col >= kStagedLabels) {
            fast = false;
            break;
          }
          const int32_t val = ev.sel_val[k];
          if (val < 0 || val > 0xffff) {  // a value no leaf has
            never = true;
            continue;
          }
          const uint32_t fw = uint32_t(val) << sh;
          uint32_t& mm = m[col >> 1];
          uint32_t& ww = w[col >> 1];
          if ((mm & fm) && (ww & fm) != fw) never = true;  // one column, two values
          mm |= fm;
          ww = (ww & ~fm) | fw;
        }
        if (fast && never) {  // want bits outside the mask: no leaf matches
          m[0] = 0u;
          w[0] = 1u;
        }
        P.sel_fast = fast ? 1 : 0;
        P.sel_mlo = m[0];
        P.sel_mhi = m[1];
        P.sel_wlo = w[0];
        P.sel_whi = w[1];
      }
      P.run = h_frun[pos];
      P.sig_new = t == 0 || h_frun[pos - 1] != P.run;
      P.rmask = int32_t(ev.req_mask);
      P.lmask = int32_t(ev.lead_mask);
      P.pad[0] = int32_t(base.flags);  // the chunk's base signature
      P.pad[1] = base.assumed_begin;
      P.pad[2] = base.assumed_end;
      for (int q = 0; q < kStagedProfiles; q++)
        r.taint[q] = q < c->num_profiles && size_t(ev.taint_table + q) < taint_table_len ? taint_table[ev.taint_table + q] : -1;
      for (int j = 0; j < ev.nreq && j < nsw; j++) r.term[j] = hterms[ev.term_begin + j];
      for (int j = 0; j < ev.nlead && j < nsw; j++) r.term[nsw + j] = hterms[ev.lead_begin + j];
    }
  }
  for (size_t i = 0; i < n; i++) c->chunk_alias[i] = uint8_t(fp[c->chunk_rep[i]].p.ss_alias);
  for (int k = 0; k < nfill; k++) c->last_alias_fills += fp[k].p.ss_alias;
}

// g_select_snap is one per device: batches of different contexts must not
// interleave (kueue_tas_eval_batch_ptrs holds the mutex for the whole batch).
// It also guards the cache below: what each device's g_select_snap holds.
static std::mutex select_snap_mu;
static DevSnap select_snap_uploaded[16];
static bool select_snap_valid[16];

// Stage 10: the arena's one H2D copy, the select path's descriptor, and the
// kernels' batch descriptor (DevBatch).  Trace point 12 (upload) lies inside.
static int upload_and_describe(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p, DevBatch& b) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const ArenaOffsets& o = p.o;
  if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->d_stage.p, c->h_stage.p, o.fpos + size_t(p.nfill) * sizeof(FillPos), hipMemcpyHostToDevice,
                           c->stream));
  // the select path's descriptor (g_select_snap), ordered before both select
  // launches: stream2 joins after events recorded later on this stream.
  // Uploaded only when it differs from what the device already holds (the
  // caller serializes batches per process, and every batch drains before
  // eval_batch returns), so a steady stream of batches pays no extra copy.
  {
    const int dev = (c->device >= 0 && c->device < 16) ? c->device : -1;
    if (dev < 0 || !select_snap_valid[dev] || std::memcmp(&select_snap_uploaded[dev], &c->snap, sizeof(DevSnap)) != 0) {
      HIPCHK(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(g_select_snap), &c->snap, sizeof(DevSnap), 0,
                                       hipMemcpyHostToDevice, c->stream));
      if (dev >= 0) {
        std::memcpy(&select_snap_uploaded[dev], &c->snap, sizeof(DevSnap));
        select_snap_valid[dev] = true;
      }
    }
  }
  trace(c, 12);
  const size_t nt = size_t(std::max(a.num_taints, 0));
  kueue_tas_eval_out* d_out = reinterpret_cast<kueue_tas_eval_out*>(c->d_res.p);
  int32_t* d_stats = reinterpret_cast<int32_t*>(c->d_res.p + p.res_off_stats);
  if (!p.lds_stats) HIPCHK(c, hipMemsetAsync(d_stats, 0, p.stats_len * 4, c->stream));
  uint8_t* ds = c->d_stage.p;
  b.evals = reinterpret_cast<const DevEval*>(ds + o.evals);
  b.terms = reinterpret_cast<const DevTerm*>(ds + o.terms);
  b.taint_table = reinterpret_cast<const int32_t*>(ds + o.taint);
  b.assumed = reinterpret_cast<const kueue_tas_assumed*>(ds + o.assumed);
  b.aff = reinterpret_cast<const kueue_tas_affinity_req*>(ds + o.aff);
  b.aff_vals = reinterpret_cast<const int32_t*>(ds + o.affv);
  b.n = int32_t(n);
  b.num_taints = int32_t(nt);
  b.num_profiles = c->num_profiles;
  b.nstat = 0;
  b.nstat_R = s.R;
  b.fill_stats = nullptr;
  b.stats_split = 0;
  b.fill_lim = nullptr;
  b.cls_member_off = nullptr;
  b.cls_members = nullptr;
  b.rack_fanout = 0;
  b.rack_pos = nullptr;
  b.ctr_sd = s.SD;
  b.counters = c->d_counters.p;
  b.overlay = c->d_overlay.p;
  b.tags = c->d_tags.p;
  b.tag_epoch = c->tag_epoch;
  b.taint_counts = d_stats;
  b.res_counts = d_stats + n * nt;
  b.sel_counts = d_stats + n * nt + n * size_t(s.R);
  b.aff_counts = b.sel_counts + n;
  b.dom_counts = b.aff_counts + n;
  b.out = d_out;
  b.entries = c->ent_dev + c->ent_used;
  b.entry_cap = c->entry_cap;
  b.sel_slots = reinterpret_cast<const SelSlot*>(ds + o.sel);
  b.slot_base = 0;
  b.scratch = c->d_scratch.p;
  b.list_cap = c->list_cap;
  b.nblk = p.nblk;
  b.partials = c->d_partials.p;
  b.partial_idx = reinterpret_cast<const int32_t*>(ds + o.pidx);
  b.rep_of = reinterpret_cast<const int32_t*>(ds + o.rep);
  b.lfc_slot = reinterpret_cast<const int32_t*>(ds + o.slot);
  b.lfc_rep = reinterpret_cast<const int32_t*>(ds + o.lrep);
  b.lfc_nslots = p.nslots;
  b.lfc_nchunks = p.nchunks;
  b.lfc_ch = c->d_lfc_ch.p + size_t(p.lfc_cur) * c->lfc_half * kLfcBins;
  b.lfc_u8 = c->d_lfc_u8.p;
  b.exp_flags = c->knobs.exp_flags;
  b.lfc_cp = c->d_lfc_cp.p;
  b.lfc_tot = c->d_lfc_tot.p;
  b.lfc_ovs = c->d_lfc_ovs.p + size_t(p.lfc_cur) * c->lfc_half;
  b.lfc_ovtot = c->d_lfc_ovtot.p;
  b.lfc_jobs = c->d_lfc_jobs.p;
  b.lfc_nitems = reinterpret_cast<int32_t*>(c->d_lfc_items.p);  // item 0's slot holds the count
  b.lfc_items = c->d_lfc_items.p + 1;
  b.prof = nullptr;
  if (KTAS_PROFILE) {
    HIPCHK(c, c->d_prof.ensure(n * P_NCAT));
    HIPCHK(c, hipMemsetAsync(c->d_prof.p, 0, n * P_NCAT * 4, c->stream));
    b.prof = c->d_prof.p;
    HIPCHK(c, c->d_fprof.ensure(size_t(1) << 18));
    HIPCHK(c, hipMemsetAsync(c->d_fprof.p, 0, (size_t(1) << 18) * 4, c->stream));
    b.fill_prof = c->d_fprof.p;
  }
  c->stat_fills += p.nfill;
  c->stat_evals += int64_t(n);
  b.fill_ids = reinterpret_cast<const int32_t*>(ds + o.fill);
  b.nfill = p.nfill;
  b.fill_chunks = reinterpret_cast<const int32_t*>(ds + o.fchunks);
  b.fill_run = reinterpret_cast<const int32_t*>(ds + o.frun);
  b.fill_pos = reinterpret_cast<const FillPos*>(ds + o.fpos);
  // the masked evaluations' assumed ranges, expanded behind the upload and
  // before enqueue_fill records the event both fill streams start from
  if (p.njobs) {
    if (p.nsmalljobs) {
      hipLaunchKernelGGL(removal_expand_kernel, dim3(unsigned(p.nsmalljobs)), dim3(kRemovalThreads), 0, c->stream,
                         reinterpret_cast<const RemovalJob*>(ds + o.rjobs),
                         reinterpret_cast<const int32_t*>(c->d_rt.p + c->rt_set_off_at), c->d_rt_table.p,
                         reinterpret_cast<kueue_tas_assumed*>(ds + o.assumed));
      HIPCHK(c, hipGetLastError());
    }
    if (p.nsegblocks) {  // the large sets' evaluations: a workgroup per segment of the table
      hipLaunchKernelGGL(removal_expand_seg_kernel, dim3(unsigned(p.nsegblocks)), dim3(kRemovalThreads), 0, c->stream,
                         reinterpret_cast<const RemovalJob*>(ds + o.rjobs), reinterpret_cast<const int4*>(ds + o.rsegs),
                         reinterpret_cast<const int32_t*>(c->d_rt.p + c->rt_set_off_at), c->d_rt_table.p,
                         static_cast<const int32_t*>(c->d_rt_seg_prefix.p),
                         reinterpret_cast<kueue_tas_assumed*>(ds + o.assumed));
      HIPCHK(c, hipGetLastError());
      c->rt_large_stats[3] += p.nsegblocks;
    }
    c->rt_stats[3] += p.nexpanded;
  }
  return KUEUE_TAS_OK;
}

// ---- The fill launch.  The instantiated kernels, all of them:
//   fill_pair_kernel<NS, TS, MR, GL, FC>                     NS 4|5|8; TS, MR, GL either; FC -1|0|32
//   fill_pair_kernel<NS, true, false, false, FC, true, LF>   leaf categories: NS 4|5|8; FC -1|0|32; LF either
//   fill_leaves_staged_kernel<NS, TS, MR, GL>                NS 4|5|8; TS, MR, GL either
//   fill_leaves_kernel<MAXT>                                 MAXT 4|8|16|32
// NS: the staged snapshot columns (ucols <= 4, <= 5, <= 8); TS: taint rows in
// LDS (FillLaunch::ts); MR: multi-run chunks; GL: global lookups in the eval
// loop (FillLaunch::gl); FC: -1 ragged pair, 32 for a rack fan-out of 32, else
// 0; LF: DevBatch::lfc_fill.  Every launch names its kernel: a runtime flag
// becomes a template argument only where the table has both values. ----
extern "C++" {

// chunks [first, first + count) of one kind (MR: multi-run) in one launch on `st`
template <int NS, bool TS, bool MR>
static void launch_fill_chunks(kueue_tas_ctx* c, const FillLaunch& f, const DevBatch& b, uint32_t umask, int first,
                               int count, hipStream_t st) {
  if (count <= 0) return;
  const DevSnap& s = c->snap;
  if (!f.pair) {
    const dim3 sg(f.sgx, unsigned(count));
    if (f.gl) hipLaunchKernelGGL((fill_leaves_staged_kernel<NS, TS, MR, true>), sg, dim3(256), 0, st, s, b, umask, first);
    else hipLaunchKernelGGL((fill_leaves_staged_kernel<NS, TS, MR, false>), sg, dim3(256), 0, st, s, b, umask, first);
    return;
  }
  c->fill_paths |= KUEUE_TAS_PATH_PAIR;  // kPairLP leaves per thread
  const dim3 pg(f.pgx, unsigned(count));
  const int fc = f.ragged_pair ? -1 : b.rack_fanout == 32 ? 32 : 0;
#define KTAS_LAUNCH_PAIR(GL, FC) \
  hipLaunchKernelGGL((fill_pair_kernel<NS, TS, MR, GL, FC>), pg, dim3(256), 0, st, s, b, umask, first)
#define KTAS_LAUNCH_CAT(FC, LF) \
  hipLaunchKernelGGL((fill_pair_kernel<NS, true, false, false, FC, true, LF>), pg, dim3(256), 0, st, s, b, umask, first)
  if constexpr (TS && !MR) {  // single-run chunks: leaf categories
    if (f.cat) {
      c->fill_paths |= KUEUE_TAS_PATH_CATEGORY;
      if (b.lfc_fill) {  // (the lean loop's LFC pair lists in LDS)
        if (fc < 0) KTAS_LAUNCH_CAT(-1, true);
        else if (fc == 32) KTAS_LAUNCH_CAT(32, true);
        else KTAS_LAUNCH_CAT(0, true);
      } else if (fc < 0) {
        KTAS_LAUNCH_CAT(-1, false);
      } else if (fc == 32) {
        KTAS_LAUNCH_CAT(32, false);
      } else {
        KTAS_LAUNCH_CAT(0, false);
      }
      return;
    }
  }
  if (f.gl) {
    if (fc < 0) KTAS_LAUNCH_PAIR(true, -1);
    else if (fc == 32) KTAS_LAUNCH_PAIR(true, 32);
    else KTAS_LAUNCH_PAIR(true, 0);
  } else if (fc < 0) {
    KTAS_LAUNCH_PAIR(false, -1);
  } else if (fc == 32) {
    KTAS_LAUNCH_PAIR(false, 32);
  } else {
    KTAS_LAUNCH_PAIR(false, 0);
  }
#undef KTAS_LAUNCH_PAIR
#undef KTAS_LAUNCH_CAT
}

// single-run chunks [0, nsingle) and multi-run chunks [nsingle, nfchunks): one
// launch each.  The multi-run chunks (a few small signatures) run beside the
// single-run chunks on stream2 (idle until the fill is done): their launch's
// ramp and tail overlap the big launch instead of following it
template <int NS, bool TS>
static int launch_staged_fill(kueue_tas_ctx* c, const ChunkPlan& p, const FillLaunch& f, const DevBatch& b) {
  const int nsingle = p.nsingle, nmulti = p.nfchunks - p.nsingle;
  const bool side = nsingle > 0 && nmulti > 0;
  if (side) {
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev[1], 0));
    launch_fill_chunks<NS, TS, true>(c, f, b, p.umask, nsingle, nmulti, c->stream2);
    HIPCHK(c, hipEventRecord(c->evl[2], c->stream2));
  } else {
    launch_fill_chunks<NS, TS, true>(c, f, b, p.umask, nsingle, nmulti, c->stream);
  }
  launch_fill_chunks<NS, TS, false>(c, f, b, p.umask, 0, nsingle, c->stream);
  if (side) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evl[2], 0));
  return KUEUE_TAS_OK;
}

}  // extern "C++"

static int launch_fill(kueue_tas_ctx* c, const ChunkPlan& p, const FillLaunch& f, const DevBatch& b, dim3 grid) {
  const DevSnap& s = c->snap;
  if (p.ucols <= 4) return f.ts ? launch_staged_fill<4, true>(c, p, f, b) : launch_staged_fill<4, false>(c, p, f, b);
  if (p.ucols <= 5) return f.ts ? launch_staged_fill<5, true>(c, p, f, b) : launch_staged_fill<5, false>(c, p, f, b);
  if (p.ucols <= 8) return f.ts ? launch_staged_fill<8, true>(c, p, f, b) : launch_staged_fill<8, false>(c, p, f, b);
  // more than 8 columns: the generic kernel, terms from global memory
  if (p.maxt <= 4) hipLaunchKernelGGL(fill_leaves_kernel<4>, grid, dim3(256), 0, c->stream, s, b);
  else if (p.maxt <= 8) hipLaunchKernelGGL(fill_leaves_kernel<8>, grid, dim3(256), 0, c->stream, s, b);
  else if (p.maxt <= 16) hipLaunchKernelGGL(fill_leaves_kernel<16>, grid, dim3(256), 0, c->stream, s, b);
  else hipLaunchKernelGGL(fill_leaves_kernel<32>, grid, dim3(256), 0, c->stream, s, b);
  return KUEUE_TAS_OK;
}

// Stage 11 (K1): the fill: the path decision (FillLaunch, the KUEUE_TAS_PATH_*
// bits), the buffers only some paths need, and the launches.
static int enqueue_fill(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p, DevBatch& b) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const DevEval* hev = stage_evals(c, p);
  const int nfill = p.nfill, nfchunks = p.nfchunks, ucols = p.ucols;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  c->last_stats[0] += nfill;
  if (s.N > 0 && nfchunks > 0) {
    FillLaunch f;
    const dim3 grid((s.N + 255) / 256, unsigned(nfchunks));
    // the staged kernels take kFillTilesPerBlock leaf tiles per block (with
    // ragged parents a tile is 4 packed wave slots)
    f.staged_fill = ucols <= 8;
    const unsigned stiles = ucols <= 8 && c->rack_fanout < 0 ? unsigned((s.n_wave_slots + 3) / 4) : grid.x;
    f.sgx = (stiles + kFillTilesPerBlock - 1) / kFillTilesPerBlock;
    f.nblk_fill = f.staged_fill ? f.sgx : grid.x;
    c->last_stats[2] += 1;
    c->last_stats[3] = ucols;
    const int nstat = p.nstat_all;
    b.nstat = p.lds_stats ? nstat : 0;
    b.nstat_R = s.R;
    // single-run chunks on fill_pair_kernel (kPairLP leaves per thread): staged
    // columns, uniform fan-out >= 2 or no fused parents; it counts the
    // ExclusionStats itself, so the batch takes the inline-stats path
    // ragged leaf parents of <= 128 leaves on fill_pair_kernel (two leaves per
    // lane, segmented scans over the lanes' pairs): every class without a
    // leader (leader classes keep the one-leaf staged kernel)
    bool any_leader = false;
    for (size_t i = 0; i < n && !any_leader; i++) any_leader = (hev[i].flags & KUEUE_TAS_F_LEADER) != 0;
    f.ragged_pair = c->pair_fill && f.staged_fill && s.wave_tab2 != nullptr && !any_leader;
    f.pair = c->pair_fill && f.staged_fill &&
             (f.ragged_pair || (c->rack_fanout >= 0 && (c->rack_fanout == 0 || c->rack_fanout >= kPairLP)));
    f.pgx = f.ragged_pair ? unsigned((s.n_wave_slots2 + 3) / 4) : unsigned((s.N + kPairTile - 1) / kPairTile);
    if (b.nstat) {
      // sized for the tile grid: fill_exclusion_kernel (split stats) writes one partial per tile
      HIPCHK(c, c->d_fill_stats.ensure(size_t(nfill) * std::max(grid.x, f.nblk_fill) * size_t(nstat)));
      b.fill_stats = c->d_fill_stats.p;
      // the reduce sums every member's stats and stores them for the class's other members
      b.cls_member_off = dev_ints(c, p.o.moff);
      b.cls_members = dev_ints(c, p.o.mem);
    }
    if (b.nstat && !c->inline_stats && !f.pair) {  // staged fill: ExclusionStats by fill_exclusion_kernel on stream3
      HIPCHK(c, c->d_fill_lim.ensure(size_t(p.nruns) * size_t(s.N)));
      b.stats_split = 1;
      b.fill_lim = c->d_fill_lim.p;
    }
    // partial slots per fill position: the exclusion grid (split), else the widest fill grid
    b.nstat_blocks = int32_t(b.stats_split ? grid.x : f.pair ? f.pgx : f.nblk_fill);
    b.rack_fanout = f.ragged_pair ? -1 : ucols <= 8 ? c->rack_fanout : 0;  // the fill fuses the first roll-up level
    if (b.rack_fanout) {
      c->fill_paths |= b.rack_fanout < 0 ? KUEUE_TAS_PATH_RAGGED_ROLLUP : KUEUE_TAS_PATH_UNIFORM_ROLLUP;
      if (f.ragged_pair) c->fill_paths |= KUEUE_TAS_PATH_RAGGED_PAIR;
      // positive-children masks are 64-bit: none when a ragged parent is wider
      if (!f.ragged_pair || s.ragged_max_fan <= kWave) {
        HIPCHK(c, c->d_rack_pos.ensure(size_t(nfill) * size_t(s.level_size[s.L - 2])));
        b.rack_pos = c->d_rack_pos.p;
      }
    }
    f.ts = b.num_profiles <= kStagedProfiles;
    // global lookups in the eval loop: a nodeSelector column beyond the
    // staged label columns, or required node affinity
    for (size_t i = 0; i < n && !f.gl; i++) {
      f.gl = (hev[i].flags & (KUEUE_TAS_F_AFFINITY | KUEUE_TAS_F_SELECTOR_EXT)) != 0;
      for (int k = 0; k < hev[i].nsel; k++) f.gl = f.gl || hev[i].sel_col[k] >= kStagedLabels;
    }
    // leaf parents wider than a slot: zeroed before the ragged pair fill adds
    // its pieces' sums (the fill bracket and stream2's chunks start after it)
    f.wide = f.ragged_pair && s.n_wide > 0;
    if (f.wide) {
      hipLaunchKernelGGL(wide_parents_zero_kernel, dim3(unsigned((s.n_wide + 255) / 256), unsigned(nfill)), dim3(256), 0,
                         c->stream, s, b);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
    }
    // leaf categories in the single-run pair fill: every filter on staged
    // data (no affinity, no far selector column: !gl), taint rows and the
    // ExclusionStats in LDS, label ids packed in 16 bits
    f.cat = c->cat_fill && f.pair && !f.gl && f.ts && b.nstat > 0 && c->labels16;
    // the fast-LFC chunk tables accumulated by the fill itself (every chunk
    // runs on fill_pair_kernel: its lean loop from the block's (category,
    // value) pairs, its per-leaf loop per wave): no lfc_hist_kernel
    // re-reading the slot classes' leaf rows
    b.lfc_fill = (p.nfast > 0 && f.pair && c->knobs.lfc_in_fill) ? 1 : 0;
    if (b.lfc_fill) c->fill_paths |= KUEUE_TAS_PATH_LFC_FILL;
    if (b.lfc_fill && c->lfc_dirty[p.lfc_cur]) {  // (after a reallocation: zeroed before the fill)
      HIPCHK(c, hipMemsetAsync(b.lfc_ch, 0, c->lfc_half * kLfcBins * 4, c->stream));
      HIPCHK(c, hipMemsetAsync(b.lfc_ovs, 0, c->lfc_half * 8, c->stream));
      c->lfc_dirty[p.lfc_cur] = false;
    }
    const int maxt = p.maxt;
    c->fill_paths |= ucols <= 8 ? (f.ts ? KUEUE_TAS_PATH_STAGED : KUEUE_TAS_PATH_STAGED_GLOBAL_TAINTS)
                                : maxt <= 4 ? KUEUE_TAS_PATH_GENERIC4 : maxt <= 8 ? KUEUE_TAS_PATH_GENERIC8
                                : maxt <= 16 ? KUEUE_TAS_PATH_GENERIC16 : KUEUE_TAS_PATH_GENERIC32;
    if (ucols <= 8 && f.gl) c->fill_paths |= KUEUE_TAS_PATH_STAGED_GL;
    if (!p.lds_stats) c->fill_paths |= KUEUE_TAS_PATH_GLOBAL_STATS;
    if (b.stats_split) c->fill_paths |= b.num_profiles <= kStagedProfiles ? KUEUE_TAS_PATH_EXCL : KUEUE_TAS_PATH_EXCL_GLOBAL_TAINTS;
    for (size_t i = 0; i < n; i++)
      if (hev[i].sx_begin >= 0) c->fill_paths |= KUEUE_TAS_PATH_SELECTOR_EXT;
    if (const int rc = launch_fill(c, p, f, b, grid)) return rc;
    HIPCHK(c, hipGetLastError());
    if (f.wide) {
      hipLaunchKernelGGL(wide_parents_finish_kernel, dim3(unsigned((s.n_wide + 255) / 256), unsigned(nfill)), dim3(256),
                         0, c->stream, s, b);
      HIPCHK(c, hipGetLastError());
    }
  }
  return KUEUE_TAS_OK;
}

// Stage 12a: the fill's end (ev[2], what stream2 and stream3 wait for) and the
// ExclusionStats on stream3 beside the roll-up / select, joined before the
// D2H: the reduce of the fill's per-block partials (counted inside the fill),
// or the split path's counting kernel + reduce.
static int enqueue_stats_branch(kueue_tas_ctx* c, const ChunkPlan& p, const DevBatch& b) {
  const DevSnap& s = c->snap;
  const int nfill = p.nfill, nfchunks = p.nfchunks;
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  const bool stats_branch = b.nstat > 0;
  if (stats_branch && !b.stats_split) {
    HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev[2], 0));
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->evs[0], c->stream3));
    hipLaunchKernelGGL(fill_stats_reduce_kernel, dim3(unsigned(nfill)), dim3(256), 0, c->stream3, b, int(b.nstat_blocks));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->evs[1], c->stream3));
  }
  if (b.stats_split) {  // counts, reduce and member stores beside the roll-up / select
    HIPCHK(c, hipStreamWaitEvent(c->stream3, c->ev[2], 0));
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->evs[0], c->stream3));
    dim3 grid((s.N + 255) / 256, unsigned(nfchunks));
    if (b.num_profiles <= kStagedProfiles) hipLaunchKernelGGL(fill_exclusion_kernel<true>, grid, dim3(256), 0, c->stream3, s, b);
    else hipLaunchKernelGGL(fill_exclusion_kernel<false>, grid, dim3(256), 0, c->stream3, s, b);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(fill_stats_reduce_kernel, dim3(unsigned(nfill)), dim3(256), 0, c->stream3, b, int(grid.x));
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->evs[1], c->stream3));
  }
  return KUEUE_TAS_OK;
}

// Stage 12b (K2): the roll-up of the levels the fill did not fuse, and the
// level maxima for the BestFit-side find_level.
static int enqueue_rollup(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p, DevBatch& b) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const int nfill = p.nfill, nbf = p.nbf;
  uint8_t* ds = c->d_stage.p;
  const int upper = s.L - 2 - (b.rack_fanout ? 1 : 0);  // levels [0, upper] left to roll up
  int top_parents = 0;  // parents above level `upper`: the fused launch's last block rolls them up
  for (int l = 0; l < upper; l++) top_parents += s.level_size[l];
  const bool fused_top = c->fused_top && nfill > 0 && upper >= 0 && s.level_size[upper] > 0 && top_parents <= 4096 &&
                         s.level_size[upper + 1] / s.level_size[upper] >= 8;
  if (fused_top) {  // every upper level and the level maxima in one launch
    c->fill_paths |= KUEUE_TAS_PATH_FUSED_TOP;
    b.level_max = nbf > 0 ? reinterpret_cast<int32_t*>(ds + p.o.top) : nullptr;
    const int per_block = 4 * kParentsPerWave;
    dim3 grid((s.level_size[upper] + per_block - 1) / per_block, unsigned(nfill));
    hipLaunchKernelGGL(rollup_top_kernel, grid, dim3(256), 0, c->stream, s, b, upper,
                       reinterpret_cast<int32_t*>(ds + p.o.top) + n * kMaxLevels);
    HIPCHK(c, hipGetLastError());
  }
  // the small top levels (<= kTailParents domains) go to rollup_tail_kernel with the level maxima
  int tail_top = -1;
  if (!fused_top && nfill > 0)
    for (int l = upper; l >= 0 && tail_top < 0; l--)
      if (s.level_size[l] <= kTailParents) tail_top = l;
  for (int l = fused_top ? -1 : upper; l > tail_top; l--) {
    if (s.level_size[l] <= 0) continue;
    const int fanout = s.level_size[l + 1] / s.level_size[l];
    if (fanout >= 8) {  // wave per parent: coalesced child reads
      const int per_block = 4 * kParentsPerWave;
      dim3 grid((s.level_size[l] + per_block - 1) / per_block, unsigned(nfill));
      hipLaunchKernelGGL(rollup_level_wave_kernel, grid, dim3(256), 0, c->stream, s, b, l);
    } else {
      dim3 grid((s.level_size[l] + 255) / 256, unsigned(nfill));
      hipLaunchKernelGGL(rollup_level_kernel, grid, dim3(256), 0, c->stream, s, b, l);
    }
    HIPCHK(c, hipGetLastError());
  }
  if (!fused_top && nfill > 0 && s.L >= 2 && (nbf > 0 || tail_top >= 0)) {
    // the small top levels and the level maxima for the BestFit-side find_level
    b.level_max = nullptr;
    if (nbf > 0) {
      HIPCHK(c, c->d_level_max.ensure(size_t(nfill) * size_t(kMaxLevels)));
      b.level_max = c->d_level_max.p;
    }
    hipLaunchKernelGGL(rollup_tail_kernel, dim3(unsigned(nfill)), dim3(256), 0, c->stream, s, b, tail_top);
    HIPCHK(c, hipGetLastError());
  }
  return KUEUE_TAS_OK;
}

// the class rep's exclusion stats go to the other members by replicate_kernel (global-atomic stats only)
static bool stats_replicated(const ChunkPlan& p, const DevBatch& b) { return p.npairs && !b.nstat; }
// KTAS_EMIT_MAIN: lfc_emit on the main stream after the BestFit select
static bool emit_on_main(const kueue_tas_ctx* c, const ChunkPlan& p) {
  return c->knobs.emit_after_bf && p.nbf > 0 && p.nfast > 0;
}
// select_kernel's per-wave LDS: the sort capacity (list_cap keys); the BestFit
// side also holds lds_level_walk's candidates (kFinalWalkLds per wave)
static int lfc_wave_lds(const kueue_tas_ctx* c) { return c->list_cap * 16; }
static int bf_wave_lds(const kueue_tas_ctx* c) { return std::max(lfc_wave_lds(c), kFinalWalkLds); }

// Stage 12c (K3): the stats replication, the leaf-level selection partials and
// the BestFit-side select (every non-fast eval) on the main stream, one launch
// per slot group.
static int enqueue_bestfit_select(kueue_tas_ctx* c, const ChunkPlan& p, DevBatch& b) {
  const DevSnap& s = c->snap;
  const int npairs = p.npairs, nleafsel = p.nleafsel, nbf = p.nbf;
  if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  const bool replicated = stats_replicated(p, b);
  if (replicated) {
    hipLaunchKernelGGL(replicate_kernel, dim3(1, unsigned(npairs)), dim3(256), 0, c->stream, s, b, dev_ints(c, p.o.pairs),
                       npairs);
    HIPCHK(c, hipGetLastError());
  }
  // an event on the main stream costs ~8 us of its device time (rocprof
  // kernel trace): recorded only when the fast-LFC branch waits for the
  // replication, or for the stage profile
  if (replicated || c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  const int32_t* d_bf = dev_ints(c, p.o.bf);
  const int waves = kSelectWaves;  // the kernel's per-wave LDS state is sized for this
  // leaf-level selection partials (non-fast evals whose requested level is the leaf level)
  if (nleafsel && s.N > 0) {
    c->last_stats[1] += nleafsel;
    dim3 grid((s.N + 255) / 256, unsigned((nleafsel + kEvalsPerFillBlock - 1) / kEvalsPerFillBlock));
    hipLaunchKernelGGL(leaf_partials_kernel, grid, dim3(256), 0, c->stream, s, b, dev_ints(c, p.o.leafsel), nleafsel);
    HIPCHK(c, hipGetLastError());
  }
  if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  if (nbf) {
    b.wave_lds = bf_wave_lds(c);
    const int32_t epoch0 = c->tag_epoch;
    for (size_t gi = 0; gi + 1 < c->sel_groups.size(); gi++) {  // one launch per slot group (one, within budget)
      const int g0 = c->sel_groups[gi], gn = c->sel_groups[gi + 1] - g0;
      b.slot_base = g0;
      b.tag_epoch = epoch0 + int32_t(gi);
      c->tag_epoch = b.tag_epoch;
      hipLaunchKernelGGL(select_kernel, dim3(unsigned((gn + waves - 1) / waves)), dim3(64 * waves),
                         size_t(waves) * size_t(b.wave_lds), c->stream, s, b, d_bf + g0, gn);
      HIPCHK(c, hipGetLastError());
    }
    b.slot_base = 0;
  }
  return KUEUE_TAS_OK;
}

// Stage 12d: the fast-LFC branch on stream2: leaf tables (after the fill),
// select + emit (after the stats replication); the main stream runs the
// BestFit side.  Enqueued after the BestFit select: that launch is on the
// batch's longest chain, and the host's calls for this branch would otherwise
// delay it.
static int enqueue_fast_lfc(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p, DevBatch& b) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const int nfast = p.nfast, nslots = p.nslots, nchunks = p.nchunks, lfc_cur = p.lfc_cur;
  const int waves = kSelectWaves;
  const bool emit_main = emit_on_main(c, p);
  const int emit_grid = int(std::min<int64_t>(int64_t(nfast) * nchunks, 2048));
  if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  if (nfast) {
    if (c->lfc_dirty[lfc_cur ^ 1]) {  // the next batch's half, zeroed while this batch runs
      HIPCHK(c, hipMemsetAsync(c->d_lfc_ch.p + size_t(lfc_cur ^ 1) * c->lfc_half * kLfcBins, 0,
                               c->lfc_half * kLfcBins * 4, c->stream2));
      HIPCHK(c, hipMemsetAsync(c->d_lfc_ovs.p + size_t(lfc_cur ^ 1) * c->lfc_half, 0, c->lfc_half * 8, c->stream2));
      c->lfc_dirty[lfc_cur ^ 1] = false;
    }
    c->lfc_dirty[lfc_cur] = true;  // this batch writes its half
    c->lfc_parity = lfc_cur ^ 1;
    HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev[2], 0));  // fill done
    if (c->stage_timing) HIPCHK(c, hipEventRecord(c->evl[0], c->stream2));
    if (!b.lfc_fill) {
      hipLaunchKernelGGL(lfc_hist_kernel, dim3(unsigned(nchunks), unsigned(nslots)), dim3(256), 0, c->stream2, s, b);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(lfc_total_kernel, dim3(unsigned(nslots)), dim3(kLfcBins), 0, c->stream2, b);
    HIPCHK(c, hipGetLastError());
    // the fast-LFC select reads the leaf counters and the LFC tables only
    // (lfc_fast): it waits for the roll-up only when the replication wrote stats
    if (stats_replicated(p, b)) HIPCHK(c, hipStreamWaitEvent(c->stream2, c->ev[4], 0));
    b.wave_lds = lfc_wave_lds(c);
    const SelSlot* sel = b.sel_slots;
    b.sel_slots = nullptr;  // fast-LFC evals keep no lists or overlay
    hipLaunchKernelGGL(select_kernel, dim3(unsigned((nfast + waves - 1) / waves)), dim3(64 * waves),
                       size_t(waves) * size_t(b.wave_lds), c->stream2, s, b, dev_ints(c, p.o.fast), nfast);
    b.sel_slots = sel;
    HIPCHK(c, hipGetLastError());
    if (emit_main) {
      HIPCHK(c, hipEventRecord(c->evl[3], c->stream2));
    } else {
      hipLaunchKernelGGL(lfc_emit_kernel, dim3(unsigned(emit_grid)), dim3(256), 0, c->stream2, s, b);
      HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipEventRecord(c->evl[1], c->stream2));
    // the branch's result headers come back on its own stream: the host
    // waits for both streams instead of the main stream waiting for this one
    // (a cross-stream hand-off costs ~17 us of device time, sync_cost.hip)
    HIPCHK(c, hipMemcpyAsync(c->h_res2.p, c->d_res.p, n * sizeof(kueue_tas_eval_out), hipMemcpyDeviceToHost, c->stream2));
  }
  if (nfast && emit_main) {  // the emit after the BestFit select on the main stream (its chunk re-reads
    // stall the descents beside it); the fast select's items from stream2
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->evl[3], 0));
    hipLaunchKernelGGL(lfc_emit_kernel, dim3(unsigned(emit_grid)), dim3(256), 0, c->stream, s, b);
    HIPCHK(c, hipGetLastError());
  }
  return KUEUE_TAS_OK;
}

// the join of the ExclusionStats branch and the results' D2H on the main stream
static int enqueue_results_d2h(kueue_tas_ctx* c, const ChunkPlan& p, const DevBatch& b) {
  if (b.nstat > 0) HIPCHK(c, hipStreamWaitEvent(c->stream, c->evs[1], 0));
  if (c->stage_timing) HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_res.p, c->d_res.p, p.res_bytes, hipMemcpyDeviceToHost, c->stream));
  return KUEUE_TAS_OK;
}

// Stage 13: the speculative class merge (merge_classes) verified exactly while
// the device runs; false: a 64-bit class hash collision.
static bool verify_merge(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p) {
  if (c->exact_merge) return true;
  const DevEval* hev = stage_evals(c, p);
  const ClassKeys keys(c, a, p);
  const std::vector<int32_t>& cls_rep = c->cls_rep;
  bool merge_ok = true;
  for (size_t t = 0; t < c->part_cls.size() && merge_ok; t++) {
    const PartClasses& pc = c->part_cls[t];
    for (size_t j = 0; j < pc.rep.size() && merge_ok; j++) {
      const int32_t r = cls_rep[size_t(c->part_map[c->part_base[t] + j])];
      if (r != pc.rep[j]) merge_ok = keys.same_sig(hev[pc.rep[j]], hev[r]) && keys.same_mask(hev[pc.rep[j]], hev[r]);
    }
  }
  for (size_t k = 0; k < cls_rep.size() && merge_ok; k++) {
    const int32_t g = c->sig_rep[size_t(c->cls_sig[k])];
    if (g != cls_rep[k]) merge_ok = keys.same_sig(hev[cls_rep[k]], hev[g]);
  }
  return merge_ok;
}

// Stage 14: the batch's one sync (both streams with fast-LFC evals, whose
// result headers come back on stream2), then the two conditions that re-run
// the chunk as it is; claim_entry_regions holds the third, which grows entry_cap.
static int sync_and_check(kueue_tas_ctx* c, const ChunkPlan& p, bool merge_ok) {
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (p.nfast) {
    HIPCHK(c, hipStreamSynchronize(c->stream2));
    const int32_t* hf = stage_ints(c, p.o.fast);
    for (int k = 0; k < p.nfast; k++) c->res_out_h[hf[k]] = c->h_res2.p[hf[k]];
  }
  if (!merge_ok) {  // a 64-bit class hash collision: the caller re-runs the chunk with the exact merge
    c->exact_merge = true;
    c->merge_reruns++;
    return ChunkRerun;
  }
  if (!c->scratch_full && c->knobs.scratch_bounded) {  // a bounded list overflowed: re-run with unbounded lists
    const int32_t* hb = stage_ints(c, p.o.bf);
    const SelSlot* hq = reinterpret_cast<const SelSlot*>(c->h_stage.p + p.o.sel);
    for (int k = 0; k < p.nbf; k++) {
      const kueue_tas_eval_out& o = c->res_out_h[hb[k]];
      if ((o.status == KUEUE_TAS_ST_INTERNAL && o.num_workers + o.num_leaders <= c->entry_cap && hq[k].lcap < p.full_lcap) ||
          c->knobs.force_scratch_rerun) {
        c->scratch_full = true;
        c->scratch_reruns++;
        return ChunkRerun;
      }
    }
  }
  return KUEUE_TAS_OK;
}

// The chunk's entry regions claimed (see ensure_entry_regions for the sizes):
// the strided offsets, each eval's pair count, ent_used.  An assignment longer
// than entry_cap: nothing claimed, the caller grows entry_cap and re-runs.
static int claim_entry_regions(kueue_tas_ctx* c, const ChunkArgs& a) {
  const size_t n = a.n;
  const int32_t entry_cap = c->entry_cap;
  int32_t need = 0;
  for (size_t i = 0; i < n; i++) need = std::max(need, c->res_out_h[i].num_workers + c->res_out_h[i].num_leaders);
  if (need > entry_cap) return ChunkGrowEntries;
  const int64_t base_pairs = int64_t(c->ent_used / 2);
  for (size_t i = 0; i <= n; i++) a.offsets[i] = base_pairs + int64_t(i) * entry_cap;  // strided regions
  for (size_t i = 0; i < n; i++)
    c->ent_count.push_back(std::min(c->res_out_h[i].num_workers + c->res_out_h[i].num_leaders, entry_cap));
  c->ent_used += n * size_t(entry_cap) * 2;
  c->ent_stride = entry_cap;
  return KUEUE_TAS_OK;
}

// Stage 15a: results and ExclusionStats to the caller's arrays
static int copy_out(kueue_tas_ctx* c, const ChunkArgs& a) {
  const DevSnap& s = c->snap;
  const size_t n = a.n;
  const size_t nt = size_t(std::max(a.num_taints, 0));
  kueue_tas_eval_out* out = a.out;
  memcpy(out, c->res_out_h, n * sizeof(kueue_tas_eval_out));
  {  // nodeSelector / affinity exclusions: counted beside select (stream3), read from the stats region after the join
    const int32_t* sel = c->res_stats_h + n * nt + n * size_t(s.R);
    for (size_t i = 0; i < n; i++) {
      out[i].excl_selector = sel[i];
      out[i].excl_affinity = sel[n + i];
      out[i].excl_topology = sel[2 * n + i];
    }
  }
  if (KTAS_PROFILE) {
    const size_t base = c->last_prof.size();
    c->last_prof.resize(base + n * P_NCAT);
    HIPCHK(c, hipMemcpy(c->last_prof.data() + base, c->d_prof.p, n * P_NCAT * 4, hipMemcpyDeviceToHost));
    c->last_fprof.resize(size_t(1) << 18);
    HIPCHK(c, hipMemcpy(c->last_fprof.data(), c->d_fprof.p, (size_t(1) << 18) * 4, hipMemcpyDeviceToHost));
  }
  for (size_t i = 0; i < n; i++) {
    c->last_ticks.push_back(c->res_out_h[i].reserved[0]);
    c->last_ticks.push_back(c->res_out_h[i].reserved[1]);
  }
  if (a.taint_counts && nt) memcpy(a.taint_counts, c->res_stats_h, n * nt * 4);
  if (a.res_counts && s.R) memcpy(a.res_counts, c->res_stats_h + n * nt, n * size_t(s.R) * 4);
  return KUEUE_TAS_OK;
}

// Stage 15b: the device stage times from the chunk's events, added to the batch's
static void collect_stage_times(kueue_tas_ctx* c, const ChunkArgs& a, const ChunkPlan& p, const DevBatch& b) {
  float* ms = a.ms;
  float* stage_ms = a.stage_ms;
  const int nfast = p.nfast;
  float st[KUEUE_TAS_NUM_STAGES] = {};
  if (!c->stage_timing) {  // only the fill bracket (ev1 -> ev2) was recorded
    (void)hipEventElapsedTime(&st[0], c->ev[1], c->ev[2]);
    for (int k = 0; k < KUEUE_TAS_NUM_STAGES; k++) stage_ms[k] += st[k];
    ms[0] += st[0];
    return;
  }
  for (int k = 0; k < 6; k++) (void)hipEventElapsedTime(&st[k], c->ev[k + 1], c->ev[k + 2]);
  const float partials = st[3];  // ev4 -> ev5: leaf partials; stage [3] reports the concurrent fast-LFC branch
  st[3] = 0.f;
  if (nfast) (void)hipEventElapsedTime(&st[3], c->evl[0], c->evl[1]);
  if (b.nstat > 0) (void)hipEventElapsedTime(&st[2], c->evs[0], c->evs[1]);  // the concurrent stats branch
  (void)hipEventElapsedTime(&st[6], c->ev[0], c->ev[7]);
  if (nfast) {  // the fast-LFC branch may end after the main stream (its results come back on its own stream)
    float tl = 0.f;
    (void)hipEventElapsedTime(&tl, c->ev[0], c->evl[1]);
    st[6] = std::max(st[6], tl);
  }
  for (int k = 0; k < KUEUE_TAS_NUM_STAGES; k++) stage_ms[k] += st[k];
  ms[0] += st[0];                    // fill (+ exclusion stats reduce)
  ms[1] += st[1] + st[2];            // roll-up + replication
  ms[2] += partials + st[4] + st[5]; // leaf partials + select + join with the fast-LFC branch
  ms[3] += st[6];
}

static int eval_chunk(kueue_tas_ctx* c, const ChunkArgs& a) {
  ChunkPlan p;
  DevBatch b{};
  int rc;
  double tm = wall_ms();
  auto lap = [&](int k) {
    const double t = wall_ms();
    c->host_ms[k] += t - tm;
    tm = t;
  };
  trace(c, 0);
  if ((rc = validate_requests(c, a))) return rc;
  c->host_ms[6] += wall_ms() - tm;
  trace(c, 1);
  if ((rc = layout_stage(c, a, p))) return rc;
  trace(c, 2);
  const double t_b = wall_ms();
  if ((rc = compile_requests(c, a, p))) return rc;
  c->host_ms[7] += wall_ms() - t_b;
  trace(c, 3);
  copy_tables(c, a, p);
  lap(0);
  trace(c, 4);
  merge_classes(c, a, p);
  trace(c, 5);
  assign_reps_and_slots(c, a, p);
  trace(c, 6);
  order_fill_chunks(c, a, p);  // (trace points 7, 8)
  lap(1);
  trace(c, 9);
  if ((rc = size_device_buffers(c, a, p))) return rc;
  if ((rc = ensure_entry_regions(c, a))) return rc;
  trace(c, 10);
  build_fill_records(c, a, p);
  trace(c, 11);
  if ((rc = upload_and_describe(c, a, p, b))) return rc;  // (trace point 12)
  if ((rc = enqueue_fill(c, a, p, b))) return rc;
  trace(c, 13);
  if ((rc = enqueue_stats_branch(c, p, b))) return rc;
  if ((rc = enqueue_rollup(c, a, p, b))) return rc;
  trace(c, 14);
  if ((rc = enqueue_bestfit_select(c, p, b))) return rc;
  trace(c, 16);
  if ((rc = enqueue_fast_lfc(c, a, p, b))) return rc;
  trace(c, 15);
  if ((rc = enqueue_results_d2h(c, p, b))) return rc;
  lap(2);
  trace(c, 17);
  const bool merge_ok = verify_merge(c, a, p);
  if ((rc = sync_and_check(c, p, merge_ok))) return rc;
  lap(3);
  trace(c, 18);
  if ((rc = claim_entry_regions(c, a))) return rc;
  lap(4);
  trace(c, 19);
  if ((rc = copy_out(c, a))) return rc;
  collect_stage_times(c, a, p, b);
  lap(5);
  return KUEUE_TAS_OK;
}

int kueue_tas_eval_batch(kueue_tas_ctx* c, const kueue_tas_eval_req* reqs, size_t n, const int32_t* taint_table,
                         size_t taint_table_len, int32_t num_taints, const kueue_tas_assumed* assumed,
                         size_t num_assumed, const kueue_tas_affinity_req* affinity, size_t num_affinity,
                         const int32_t* affinity_values, size_t num_affinity_values, kueue_tas_eval_out* out,
                         int64_t* entry_offsets, int32_t* entries, size_t entries_capacity, int32_t* taint_counts,
                         int32_t* res_counts) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (n && !reqs) return fail(c, KUEUE_TAS_EINVAL, "null requests");
  std::vector<const kueue_tas_eval_req*>& ptrs = c->req_ptrs;
  ptrs.resize(n);
  for (size_t i = 0; i < n; i++) ptrs[i] = reqs + i;
  return kueue_tas_eval_batch_ptrs(c, ptrs.data(), n, taint_table, taint_table_len, num_taints, assumed, num_assumed,
                                   affinity, num_affinity, affinity_values, num_affinity_values, out, entry_offsets,
                                   entries, entries_capacity, taint_counts, res_counts);
}

static int eval_batch_impl(kueue_tas_ctx* c, const kueue_tas_eval_req* const* reqs, size_t n,
                           const int32_t* taint_table, size_t taint_table_len, int32_t num_taints,
                           const kueue_tas_assumed* assumed, size_t num_assumed,
                           const kueue_tas_affinity_req* affinity, size_t num_affinity,
                           const int32_t* affinity_values, size_t num_affinity_values, kueue_tas_eval_out* out,
                           int64_t* entry_offsets, int32_t* entries, size_t entries_capacity, int32_t* taint_counts,
                           int32_t* res_counts, const int32_t* removal_set, const uint64_t* removal_mask);

int kueue_tas_eval_batch_ptrs(kueue_tas_ctx* c, const kueue_tas_eval_req* const* reqs, size_t n,
                              const int32_t* taint_table, size_t taint_table_len, int32_t num_taints,
                              const kueue_tas_assumed* assumed, size_t num_assumed,
                              const kueue_tas_affinity_req* affinity, size_t num_affinity,
                              const int32_t* affinity_values, size_t num_affinity_values, kueue_tas_eval_out* out,
                              int64_t* entry_offsets, int32_t* entries, size_t entries_capacity, int32_t* taint_counts,
                              int32_t* res_counts) {
  return eval_batch_impl(c, reqs, n, taint_table, taint_table_len, num_taints, assumed, num_assumed, affinity,
                         num_affinity, affinity_values, num_affinity_values, out, entry_offsets, entries,
                         entries_capacity, taint_counts, res_counts, nullptr, nullptr);
}

int kueue_tas_eval_batch_removals(kueue_tas_ctx* c, const kueue_tas_eval_req* const* reqs, size_t n,
                                  const int32_t* taint_table, size_t taint_table_len, int32_t num_taints,
                                  const kueue_tas_assumed* assumed, size_t num_assumed,
                                  const kueue_tas_affinity_req* affinity, size_t num_affinity,
                                  const int32_t* affinity_values, size_t num_affinity_values, kueue_tas_eval_out* out,
                                  int64_t* entry_offsets, int32_t* entries, size_t entries_capacity,
                                  int32_t* taint_counts, int32_t* res_counts, const int32_t* removal_set,
                                  const uint64_t* removal_mask) {
  if (!c) return KUEUE_TAS_EINVAL;
  bool any = false;  // no set or no masked position anywhere: the plain batch
  if (removal_set && removal_mask)
    for (size_t i = 0; i < n && !any; i++) any = removal_set[i] != -1 && removal_mask[i] != 0;
  return eval_batch_impl(c, reqs, n, taint_table, taint_table_len, num_taints, assumed, num_assumed, affinity,
                         num_affinity, affinity_values, num_affinity_values, out, entry_offsets, entries,
                         entries_capacity, taint_counts, res_counts, any ? removal_set : nullptr,
                         any ? removal_mask : nullptr);
}

static int eval_batch_impl(kueue_tas_ctx* c, const kueue_tas_eval_req* const* reqs, size_t n,
                           const int32_t* taint_table, size_t taint_table_len, int32_t num_taints,
                           const kueue_tas_assumed* assumed, size_t num_assumed,
                           const kueue_tas_affinity_req* affinity, size_t num_affinity,
                           const int32_t* affinity_values, size_t num_affinity_values, kueue_tas_eval_out* out,
                           int64_t* entry_offsets, int32_t* entries, size_t entries_capacity, int32_t* taint_counts,
                           int32_t* res_counts, const int32_t* removal_set, const uint64_t* removal_mask) {
  std::lock_guard<std::mutex> select_snap_lock(select_snap_mu);
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  HIPCHK(c, hipSetDevice(c->device));
  float ms[4] = {0, 0, 0, 0};
  float stage_ms[KUEUE_TAS_NUM_STAGES] = {};
  c->ent_used = 0;
  c->ent_count.clear();
  c->last_ticks.clear();
  c->last_prof.clear();
  for (auto& v : c->last_stats) v = 0;
  c->last_alias_fills = 0;
  for (auto& v : c->host_ms) v = 0;
  c->fill_paths = 0;
  c->eval_gen++;
  const size_t chunk = size_t(c->max_batch);
  std::vector<int64_t> off;
  entry_offsets[0] = 0;
  ChunkArgs a{reqs,     n,           taint_table,     taint_table_len,     num_taints, assumed, num_assumed,
              affinity, num_affinity, affinity_values, num_affinity_values, out,        nullptr, taint_counts,
              res_counts, ms,         stage_ms};
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    size_t m = std::min(chunk, n - i0);
    off.assign(m + 1, 0);
    c->chunk_base = i0;
    a.reqs = reqs + i0;
    a.n = m;
    a.out = out + i0;
    a.offsets = off.data();
    a.taint_counts = taint_counts ? taint_counts + i0 * size_t(std::max(num_taints, 0)) : nullptr;
    a.res_counts = res_counts ? res_counts + i0 * size_t(c->snap.R) : nullptr;
    a.rset = removal_set ? removal_set + i0 : nullptr;
    a.rmask = removal_set ? removal_mask + i0 : nullptr;
    const size_t keep = c->ent_used;
    auto rewind = [&] {  // what a chunk that re-runs recorded for the batch
      c->ent_used = keep;
      c->ent_count.resize(i0);
      c->last_ticks.resize(2 * i0);
      c->last_prof.resize(KTAS_PROFILE ? i0 * P_NCAT : 0);
    };
    for (;;) {
      int rc = eval_chunk(c, a);
      if (rc == ChunkRerun) {
        rewind();
        continue;
      }
      c->exact_merge = false;
      if (rc == ChunkGrowEntries) {
        rewind();
        int32_t need = 0;
        for (size_t i = 0; i < m; i++) need = std::max(need, c->res_out_h[i].num_workers + c->res_out_h[i].num_leaders);
        int cap = c->entry_cap;
        while (cap < need) cap *= 2;
        c->entry_cap = cap;
        continue;
      }
      if (rc) {
        c->scratch_full = false;
        return rc;
      }
      c->scratch_full = false;
      break;
    }
    for (size_t i = 0; i <= m; i++) entry_offsets[i0 + i] = off[i];
  }
  memcpy(c->last_ms, ms, sizeof ms);
  memcpy(c->last_stage_ms, stage_ms, sizeof stage_ms);
  c->ent_strided_off.assign(entry_offsets, entry_offsets + n + 1);
  if (!entries) return KUEUE_TAS_OK;  // strided offsets into kueue_tas_last_entries()
  // packed layout for the caller
  int64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    entry_offsets[i] = total;
    total += c->ent_count[i];
  }
  entry_offsets[n] = total;
  if (size_t(total) > entries_capacity) return fail(c, KUEUE_TAS_EOVERFLOW, "entries buffer too small");
  return kueue_tas_fetch_entries(c, entries, entries_capacity);
}

// ---- resident removal tables: validation and the positions' record counts on
// the host (they size every evaluation's range without a synchronisation),
// one upload, one removal_table_kernel launch (a workgroup per set).  With
// KUEUE_TAS_RT_LARGE_SETS the sets above kRemovalSetCap records go through the
// large sets' launches behind it, all of them together: the host knows every
// set's raw and kept counts, so it sizes the grids and the merge passes. ----
int kueue_tas_removal_tables_build(kueue_tas_ctx* c, const kueue_tas_delta* target_deltas, const int64_t* target_off,
                                   size_t n_targets, const int32_t* cand, const int64_t* cand_off, size_t n_sets) {
  return kueue_tas_removal_tables_build_flags(c, target_deltas, target_off, n_targets, cand, cand_off, n_sets, 0);
}

int kueue_tas_removal_tables_build_flags(kueue_tas_ctx* c, const kueue_tas_delta* target_deltas,
                                         const int64_t* target_off, size_t n_targets, const int32_t* cand,
                                         const int64_t* cand_off, size_t n_sets, uint32_t flags) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (flags & ~KUEUE_TAS_RT_LARGE_SETS) return fail(c, KUEUE_TAS_EINVAL, "unknown removal table flags");
  const int64_t set_cap = (flags & KUEUE_TAS_RT_LARGE_SETS) ? KUEUE_TAS_REMOVAL_LARGE_SET_CAP : KUEUE_TAS_REMOVAL_SET_CAP;
  if ((n_targets && !target_off) || (n_sets && !cand_off)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  if (n_targets >= size_t(INT32_MAX) || n_sets >= size_t(INT32_MAX)) return fail(c, KUEUE_TAS_EINVAL, "too many targets or sets");
  const int32_t N = c->snap.N, R = c->snap.R;
  if (n_targets && target_off[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "target offsets do not start at 0");
  for (size_t t = 0; t < n_targets; t++)
    if (target_off[t + 1] < target_off[t]) return fail(c, KUEUE_TAS_EINVAL, "target offsets not monotone");
  const int64_t nrec = n_targets ? target_off[n_targets] : 0;
  if (nrec > INT32_MAX / 2 || (nrec && !target_deltas)) return fail(c, KUEUE_TAS_EINVAL, "target records");
  std::vector<int32_t> kept(n_targets, 0);  // per target: records with leaf >= 0
  for (size_t t = 0; t < n_targets; t++)
    for (int64_t k = target_off[t]; k < target_off[t + 1]; k++) {
      const kueue_tas_delta& x = target_deltas[k];
      if (x.leaf < -1 || x.leaf >= N || x.col < 0 || x.col >= R || x.col > kRemovalColMask)
        return fail(c, KUEUE_TAS_EINVAL, "target record out of range");
      kept[t] += x.leaf >= 0;
    }
  if (n_sets && cand_off[0] != 0) return fail(c, KUEUE_TAS_EINVAL, "candidate offsets do not start at 0");
  for (size_t s = 0; s < n_sets; s++) {
    if (cand_off[s + 1] < cand_off[s]) return fail(c, KUEUE_TAS_EINVAL, "candidate offsets not monotone");
    if (cand_off[s + 1] - cand_off[s] > KUEUE_TAS_REMOVAL_MAX_CANDIDATES)
      return fail(c, KUEUE_TAS_EINVAL, "more than 64 candidates in a removal set");
  }
  const int64_t nent = n_sets ? cand_off[n_sets] : 0;
  if (nent && !cand) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  std::vector<int32_t> set_off(n_sets + 1, 0), coff(n_sets + 1, 0), pos_kept(size_t(nent), 0);
  std::vector<RemovalLargeSet> large;  // the large sets, then the totals
  std::vector<int32_t> large_seg_off;  // per set (filled with the first large set)
  int64_t nkeys = 0, nchunks = 0, nsegs = 0, max_chunks = 0, large_kept = 0;
  for (size_t s = 0; s < n_sets; s++) {
    int64_t raw = 0, kp = 0;
    for (int64_t e = cand_off[s]; e < cand_off[s + 1]; e++) {
      if (cand[e] < 0 || size_t(cand[e]) >= n_targets) return fail(c, KUEUE_TAS_EINVAL, "removal candidate out of range");
      raw += target_off[cand[e] + 1] - target_off[cand[e]];
      kp += pos_kept[size_t(e)] = kept[size_t(cand[e])];
    }
    if (raw > set_cap) return fail(c, KUEUE_TAS_EOVERFLOW, "removal set above the record cap");
    coff[s + 1] = int32_t(cand_off[s + 1]);
    if (int64_t(set_off[s]) + kp > INT32_MAX) return fail(c, KUEUE_TAS_EOVERFLOW, "removal tables too large");
    set_off[s + 1] = int32_t(set_off[s] + kp);
    if (raw > KUEUE_TAS_REMOVAL_SET_CAP) {  // a large set: a key per record, a sort per chunk, a prefix row per segment
      if (large.empty()) large_seg_off.assign(n_sets, -1);
      large.push_back({int32_t(s), int32_t(nkeys), int32_t(nchunks), int32_t(nsegs)});
      large_seg_off[s] = int32_t(nsegs);
      const int64_t chunks = (raw + kRemovalSetCap - 1) / kRemovalSetCap;
      nkeys += raw;
      nchunks += chunks;
      nsegs += std::max<int64_t>(1, (kp + kRemovalExpandSegment - 1) / kRemovalExpandSegment);  // (no records: one segment)
      max_chunks = std::max(max_chunks, chunks);
      large_kept += kp;
      if (nkeys > INT32_MAX / 2) return fail(c, KUEUE_TAS_EOVERFLOW, "removal tables too large");
    }
  }
  const size_t nl = large.size();
  if (nl) large.push_back({-1, int32_t(nkeys), int32_t(nchunks), int32_t(nsegs)});
  HIPCHK(c, hipSetDevice(c->device));
  // the upload: target records | list entries | cand_off | set_off
  auto al = [](size_t b) { return (b + 15) / 16 * 16; };
  const size_t o_ent = al(size_t(nrec) * sizeof(kueue_tas_delta)), o_coff = o_ent + al(size_t(nent) * 4);
  const size_t o_soff = o_coff + al((n_sets + 1) * 4);
  const size_t o_large = nl ? al(o_soff + (n_sets + 1) * 4) : 0;  // (a build without large sets: not a byte more)
  const size_t bytes = nl ? o_large + large.size() * sizeof(RemovalLargeSet) : o_soff + (n_sets + 1) * 4;
  if (c->ev_rt) HIPCHK(c, hipEventSynchronize(c->ev_rt));
  else HIPCHK(c, hipEventCreateWithFlags(&c->ev_rt, hipEventDisableTiming));
  c->rt_built = false;  // (valid input: the resident tables are being replaced)
  HIPCHK(c, c->h_rt.reserve(bytes));
  HIPCHK(c, c->d_rt.reserve(bytes));
  HIPCHK(c, c->d_rt_table.reserve(size_t(set_off[n_sets])));
  if (nl) {
    HIPCHK(c, c->d_rt_keys[0].reserve(size_t(nkeys)));
    HIPCHK(c, c->d_rt_keys[1].reserve(size_t(nkeys)));
    HIPCHK(c, c->d_rt_seg_prefix.reserve(size_t(nsegs) * kWave));
  }
  kueue_tas_delta* h_rec = reinterpret_cast<kueue_tas_delta*>(c->h_rt.p);
  int32_t* h_ent = reinterpret_cast<int32_t*>(c->h_rt.p + o_ent);
  if (nrec) memcpy(h_rec, target_deltas, size_t(nrec) * sizeof(kueue_tas_delta));
  for (size_t t = 0; t < n_targets; t++)  // a target's first record carries its record count
    if (target_off[t + 1] > target_off[t])
      h_rec[target_off[t]].col |=
          int32_t(std::min<int64_t>(target_off[t + 1] - target_off[t], set_cap + 1) << kRemovalPosShift);
  for (int64_t e = 0; e < nent; e++)
    h_ent[e] = target_off[cand[e] + 1] > target_off[cand[e]] ? int32_t(target_off[cand[e]]) : -1;
  memcpy(c->h_rt.p + o_coff, coff.data(), (n_sets + 1) * 4);
  memcpy(c->h_rt.p + o_soff, set_off.data(), (n_sets + 1) * 4);
  if (nl) memcpy(c->h_rt.p + o_large, large.data(), large.size() * sizeof(RemovalLargeSet));
  HIPCHK(c, hipMemcpyAsync(c->d_rt.p, c->h_rt.p, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_rt, c->stream));
  if (n_sets) {
    hipLaunchKernelGGL(removal_table_kernel, dim3(unsigned(n_sets)), dim3(kRemovalThreads), 0, c->stream,
                       reinterpret_cast<const kueue_tas_delta*>(c->d_rt.p),
                       reinterpret_cast<const int32_t*>(c->d_rt.p + o_ent),
                       reinterpret_cast<const int32_t*>(c->d_rt.p + o_coff),
                       reinterpret_cast<const int32_t*>(c->d_rt.p + o_soff), c->d_rt_table.p);
    HIPCHK(c, hipGetLastError());
  }
  int passes = 0;
  if (nl) {  // chunk sort | merge passes | store | segment prefix, ordered by the stream alone
    static_assert(kRemovalSetCap == 1 << 12, "removal_merge_kernel's first runs are the sorted chunks");
    const kueue_tas_delta* d_rec = reinterpret_cast<const kueue_tas_delta*>(c->d_rt.p);
    const int32_t* d_ent = reinterpret_cast<const int32_t*>(c->d_rt.p + o_ent);
    const int32_t* d_coff = reinterpret_cast<const int32_t*>(c->d_rt.p + o_coff);
    const RemovalLargeSet* d_large = reinterpret_cast<const RemovalLargeSet*>(c->d_rt.p + o_large);
    hipLaunchKernelGGL(removal_chunk_sort_kernel, dim3(unsigned(nchunks)), dim3(kRemovalThreads), 0, c->stream, d_rec,
                       d_ent, d_coff, d_large, int(nl), c->d_rt_keys[0].p);
    HIPCHK(c, hipGetLastError());
    while ((int64_t(1) << passes) < max_chunks) passes++;
    for (int p = 0; p < passes; p++) {
      hipLaunchKernelGGL(removal_merge_kernel, dim3(unsigned(nchunks)), dim3(kRemovalThreads), 0, c->stream, d_large,
                         int(nl), static_cast<const uint64_t*>(c->d_rt_keys[p & 1].p), c->d_rt_keys[(p + 1) & 1].p,
                         12 + p);
      HIPCHK(c, hipGetLastError());
    }
    hipLaunchKernelGGL(removal_store_kernel, dim3(unsigned(nsegs)), dim3(kRemovalThreads), 0, c->stream, d_rec, d_ent,
                       d_coff, reinterpret_cast<const int32_t*>(c->d_rt.p + o_soff), d_large, int(nl),
                       static_cast<const uint64_t*>(c->d_rt_keys[passes & 1].p), c->d_rt_table.p, c->d_rt_seg_prefix.p);
    HIPCHK(c, hipGetLastError());
    hipLaunchKernelGGL(removal_seg_prefix_kernel, dim3(unsigned(nl)), dim3(kWave), 0, c->stream, d_large,
                       c->d_rt_seg_prefix.p);
    HIPCHK(c, hipGetLastError());
  }
  c->rt_large_seg_off.swap(large_seg_off);
  c->rt_large_stats[0] = int64_t(nl);
  c->rt_large_stats[1] = large_kept;
  c->rt_large_stats[2] = passes;
  c->rt_large_stats[3] = 0;
  c->rt_cand_off.swap(coff);
  c->rt_set_off.swap(set_off);
  c->rt_pos_kept.swap(pos_kept);
  c->rt_set_off_at = o_soff;
  c->rt_snap_gen = c->n_loads + c->n_splices;
  c->rt_built = true;
  c->rt_stats[0] = int64_t(n_sets);
  c->rt_stats[1] = c->rt_set_off[n_sets];
  c->rt_stats[2] = int64_t(bytes);
  c->rt_stats[3] = 0;
  return KUEUE_TAS_OK;
}

int kueue_tas_removal_tables_clear(kueue_tas_ctx* c) {
  if (!c) return KUEUE_TAS_EINVAL;
  c->rt_built = false;
  c->rt_cand_off.clear();
  c->rt_set_off.clear();
  c->rt_pos_kept.clear();
  c->rt_large_seg_off.clear();
  for (auto& v : c->rt_stats) v = 0;
  for (auto& v : c->rt_large_stats) v = 0;
  return KUEUE_TAS_OK;
}

int kueue_tas_removal_stats(kueue_tas_ctx* c, int64_t out[4]) {
  if (!c || !out) return KUEUE_TAS_EINVAL;
  for (int k = 0; k < 4; k++) out[k] = c->rt_stats[k];
  return KUEUE_TAS_OK;
}

int kueue_tas_removal_large_stats(kueue_tas_ctx* c, int64_t out[4]) {
  if (!c || !out) return KUEUE_TAS_EINVAL;
  for (int k = 0; k < 4; k++) out[k] = c->rt_large_stats[k];
  return KUEUE_TAS_OK;
}

int kueue_tas_last_counters(kueue_tas_ctx* c, size_t i, int32_t* out, size_t cap) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!out) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  if (i < c->chunk_base || i >= c->chunk_base + c->chunk_rep.size())
    return fail(c, KUEUE_TAS_EINVAL, "request not in the last device chunk (max_batch)");
  const DevSnap& s = c->snap;
  size_t total = 0;
  for (int l = 0; l < s.L; l++) total += size_t(s.level_size[l]);
  if (cap < 5 * total) return fail(c, KUEUE_TAS_EOVERFLOW, "counters buffer too small");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t k = i - c->chunk_base;
  const int32_t* rep = c->d_counters.p + int64_t(c->ctr_row_off[size_t(c->chunk_rep[k])]) * s.SD;
  const bool leader = c->chunk_leader[k] != 0;
  for (int f = 0; f < 5; f++) {
    // phase 1 writes the leader fields only for leader requests; otherwise
    // they equal state / sliceState and leaderState is 0 (select's Wave::get)
    int src = leader ? f : (f == 2 ? 0 : f == 3 ? 1 : f);
    if (c->chunk_alias[k] && src == 1) src = 0;  // a simple class's sliceState row aliases state
    size_t pos = size_t(f) * total;
    for (int l = 0; l < s.L; l++) {
      const size_t nl = size_t(s.level_size[l]);
      if (!leader && f == 4) std::memset(out + pos, 0, nl * 4);
      else if (nl)
        HIPCHK(c, hipMemcpyAsync(out + pos, rep + int64_t(src) * s.SD + s.level_off[l], nl * 4, hipMemcpyDeviceToHost,
                                 c->stream));
      pos += nl;
    }
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KUEUE_TAS_OK;
}

const int32_t* kueue_tas_last_entries(kueue_tas_ctx* c, size_t* num_pairs) {
  if (!c) return nullptr;
  if (num_pairs) *num_pairs = c->ent_used / 2;
  return c->ent_host;
}

int kueue_tas_snapshot_set_leaf_tags(kueue_tas_ctx* c, const uint64_t* tags, size_t n) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!tags) {
    c->leaf_tags_on = false;
    return KUEUE_TAS_OK;
  }
  if (n != size_t(c->snap.N)) return fail(c, KUEUE_TAS_EINVAL, "leaf tags: n must be the snapshot's leaf count");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_leaf_tags.reserve(std::max<size_t>(n, 1)));
  if (n) HIPCHK(c, hipMemcpyAsync(c->d_leaf_tags.p, tags, n * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  c->leaf_tags_on = true;
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_digest(kueue_tas_ctx* c, uint64_t* words, size_t cap, size_t* len, uint64_t* chunks,
                              size_t chunk_cap, size_t* n_chunks) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  if (!len || (!words && cap) || (chunks && !n_chunks)) return fail(c, KUEUE_TAS_EINVAL, "null argument");
  const DevSnap& s = c->snap;
  const size_t C = size_t(kDigestFixed + 2 * s.R + s.K);
  const size_t nch = (size_t(s.N) + kDigestChunk - 1) / kDigestChunk;
  *len = C;
  if (n_chunks) *n_chunks = nch;
  if (cap < C || (chunks && chunk_cap < nch)) return fail(c, KUEUE_TAS_EOVERFLOW, "digest: capacity");
  size_t seq = 5 + size_t(s.L);  // the topology sequence (digest_topology_value)
  for (int l = 0; l < s.L; l++) seq += size_t(s.level_size[l]) + (l + 1 < s.L ? size_t(s.level_size[l]) + 1 : 0);
  const size_t ntopo = (seq + kDigestChunk - 1) / kDigestChunk;
  const size_t n_part = nch * C + ntopo, n_out = C + nch;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_digest.reserve(n_part + n_out));
  HIPCHK(c, c->h_digest.reserve(n_out));
  const bool timed = c->stage_timing;
  if (timed) {
    for (auto& e : c->ev_digest)
      if (!e) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(c->ev_digest[0], c->stream));
  }
  uint64_t* d_out = c->d_digest.p + n_part;
  hipLaunchKernelGGL(snapshot_digest_kernel, dim3(unsigned(nch + ntopo)), dim3(kDigestThreads), 0, c->stream, s,
                     c->leaf_tags_on ? c->d_leaf_tags.p : nullptr, int(nch), c->d_digest.p);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(snapshot_digest_sum_kernel, dim3(1), dim3(kDigestThreads), 0, c->stream, c->d_digest.p, int(nch),
                     int(ntopo), int(C), d_out);
  HIPCHK(c, hipGetLastError());
  if (timed) HIPCHK(c, hipEventRecord(c->ev_digest[1], c->stream));
  HIPCHK(c, hipMemcpyAsync(c->h_digest.p, d_out, n_out * 8, hipMemcpyDeviceToHost, c->stream));
  if (timed) HIPCHK(c, hipEventRecord(c->ev_digest[2], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (timed) {
    (void)hipEventElapsedTime(&c->digest_ms[0], c->ev_digest[0], c->ev_digest[1]);
    (void)hipEventElapsedTime(&c->digest_ms[1], c->ev_digest[0], c->ev_digest[2]);
  }
  memcpy(words, c->h_digest.p, C * 8);
  if (chunks && nch) memcpy(chunks, c->h_digest.p + C, nch * 8);
  return KUEUE_TAS_OK;
}

int kueue_tas_last_digest_ms(kueue_tas_ctx* c, float* ms2) {
  if (!c || !ms2) return KUEUE_TAS_EINVAL;
  ms2[0] = c->digest_ms[0];
  ms2[1] = c->digest_ms[1];
  return KUEUE_TAS_OK;
}

int kueue_tas_snapshot_read_leaves(kueue_tas_ctx* c, const int32_t* leaves, size_t n, int64_t* free_rows,
                                   uint32_t* free_present, int64_t* usage_rows, uint32_t* usage_present,
                                   int32_t* profiles, int32_t* labels, int32_t* live, uint64_t* tags) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (!c->loaded) return fail(c, KUEUE_TAS_ENOSNAPSHOT, "no snapshot loaded");
  const DevSnap& s = c->snap;
  if (n > size_t(0x7fffffff) || (!leaves && n > size_t(s.N))) return fail(c, KUEUE_TAS_EINVAL, "read_leaves: n");
  for (size_t i = 0; leaves && i < n; i++)
    if (leaves[i] < 0 || leaves[i] >= s.N) return fail(c, KUEUE_TAS_EINVAL, "read_leaves: leaf out of range");
  if (n == 0) return KUEUE_TAS_OK;
  const size_t R = size_t(s.R), K = size_t(s.K);
  // the staging block (read_leaves_kernel): free | usage | tags | free_present | usage_present | profiles | live | labels
  const size_t o_usage = n * R * 8, o_tags = 2 * o_usage, o_fp = o_tags + n * 8, o_up = o_fp + n * 4, o_prof = o_up + n * 4,
               o_live = o_prof + n * 4, o_lab = o_live + n * 4, bytes = o_lab + n * K * 4;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, c->d_read.reserve(bytes));
  HIPCHK(c, c->h_read.reserve(bytes));
  if (leaves) {
    HIPCHK(c, c->d_read_ids.reserve(n));
    HIPCHK(c, hipMemcpyAsync(c->d_read_ids.p, leaves, n * 4, hipMemcpyHostToDevice, c->stream));
  }
  hipLaunchKernelGGL(read_leaves_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, c->stream, s,
                     c->leaf_tags_on ? c->d_leaf_tags.p : nullptr, leaves ? c->d_read_ids.p : nullptr, int(n),
                     c->d_read.p);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(c->h_read.p, c->d_read.p, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));  // (also: the caller's leaf list is read)
  const uint8_t* h = c->h_read.p;
  if (free_rows && R) memcpy(free_rows, h, n * R * 8);
  if (usage_rows && R) memcpy(usage_rows, h + o_usage, n * R * 8);
  if (tags) memcpy(tags, h + o_tags, n * 8);
  if (free_present) memcpy(free_present, h + o_fp, n * 4);
  if (usage_present) memcpy(usage_present, h + o_up, n * 4);
  if (profiles) memcpy(profiles, h + o_prof, n * 4);
  if (live) memcpy(live, h + o_live, n * 4);
  if (labels && K) memcpy(labels, h + o_lab, n * K * 4);
  return KUEUE_TAS_OK;
}

const uint64_t* kueue_tas_last_entry_tags(kueue_tas_ctx* c) {
  return (c && c->leaf_tags_on && c->snap.tag_out) ? c->tag_host : nullptr;
}

int kueue_tas_fetch_entries(kueue_tas_ctx* c, int32_t* entries, size_t entries_capacity) {
  if (!c) return KUEUE_TAS_EINVAL;
  size_t total = 0;
  for (int32_t k : c->ent_count) total += size_t(k);
  if (total > entries_capacity) return fail(c, KUEUE_TAS_EOVERFLOW, "entries buffer too small");
  size_t pos = 0;
  for (size_t i = 0; i < c->ent_count.size(); i++) {
    const size_t k = size_t(c->ent_count[i]);
    if (k) memcpy(entries + 2 * pos, c->ent_host + 2 * size_t(c->ent_strided_off[i]), k * 8);
    pos += k;
  }
  return KUEUE_TAS_OK;
}

int kueue_tas_set_stage_timing(kueue_tas_ctx* c, int32_t on) {
  if (!c) return KUEUE_TAS_EINVAL;
  c->stage_timing = on != 0;
  return KUEUE_TAS_OK;
}

int kueue_tas_last_timings(kueue_tas_ctx* c, float* ms4) {
  if (!c || !ms4) return KUEUE_TAS_EINVAL;
  memcpy(ms4, c->last_ms, sizeof c->last_ms);
  return KUEUE_TAS_OK;
}

int kueue_tas_last_stage_times(kueue_tas_ctx* c, float* ms, int n) {
  if (!c || !ms || n < 0) return KUEUE_TAS_EINVAL;
  for (int k = 0; k < n && k < KUEUE_TAS_NUM_STAGES; k++) ms[k] = c->last_stage_ms[k];
  return KUEUE_TAS_OK;
}

int kueue_tas_last_eval_ticks(kueue_tas_ctx* c, int32_t* ticks, size_t n) {
  if (!c || !ticks) return KUEUE_TAS_EINVAL;
  for (size_t i = 0; i < 2 * n; i++) ticks[i] = i < c->last_ticks.size() ? c->last_ticks[i] : 0;
  return KUEUE_TAS_OK;
}

int64_t kueue_tas_last_fill_profile(kueue_tas_ctx* c, int32_t* out, size_t n) {
  if (!c || !out) return 0;
  const size_t k = std::min(n, c->last_fprof.size());
  if (k) memcpy(out, c->last_fprof.data(), k * 4);
  return int64_t(k);
}

int kueue_tas_last_eval_profile(kueue_tas_ctx* c, int32_t* ticks, size_t n) {
  if (!c || !ticks) return KUEUE_TAS_EINVAL;
  for (size_t i = 0; i < n * P_NCAT; i++) ticks[i] = i < c->last_prof.size() ? c->last_prof[i] : 0;
  return KUEUE_TAS_OK;
}

int64_t kueue_tas_merge_reruns(kueue_tas_ctx* c) { return c ? c->merge_reruns : -1; }

int kueue_tas_select_groups(kueue_tas_ctx* c, int64_t* last_groups, int64_t* scratch_reruns) {
  if (!c) return KUEUE_TAS_EINVAL;
  if (last_groups) *last_groups = c->sel_groups.empty() ? 0 : int64_t(c->sel_groups.size()) - 1;
  if (scratch_reruns) *scratch_reruns = c->scratch_reruns;
  return KUEUE_TAS_OK;
}

int kueue_tas_last_host_trace(kueue_tas_ctx* c, double* ms, int n) {  // ms since the chunk's start, [0, 20)
  if (!c || !ms) return KUEUE_TAS_EINVAL;
  for (int k = 0; k < n && k < 20; k++) ms[k] = c->trace[k] - c->trace[0];
  return KUEUE_TAS_OK;
}

int kueue_tas_last_host_times(kueue_tas_ctx* c, double* ms, int n) {  // copies min(n, 8)
  if (!c || !ms || n < 0) return KUEUE_TAS_EINVAL;
  for (int k = 0; k < n && k < 8; k++) ms[k] = c->host_ms[k];
  return KUEUE_TAS_OK;
}

uint32_t kueue_tas_last_fill_paths(kueue_tas_ctx* c) { return c ? c->fill_paths : 0u; }
uint64_t kueue_tas_eval_generation(kueue_tas_ctx* c) { return c ? c->eval_gen : 0u; }

int64_t kueue_tas_last_alias_fills(kueue_tas_ctx* c) { return c ? c->last_alias_fills : 0; }

int kueue_tas_last_stats(kueue_tas_ctx* c, int64_t* stats4) {
  if (!c || !stats4) return KUEUE_TAS_EINVAL;
  memcpy(stats4, c->last_stats, sizeof c->last_stats);
  return KUEUE_TAS_OK;
}

}  // extern "C"
