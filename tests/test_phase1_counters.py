"""Phase-1 counters compared directly: what the fill and roll-up kernels
compute (fillInCounts + fillInCountsHelper, tas_flavor_snapshot.go:1568-1719)
-- state, sliceState, stateWithLeader, sliceStateWithLeader and leaderState
of every domain of every level -- against the oracle's fill_in_counts
stopped before phase 2 (oracle_lib.counters), for exact equality of all
5 x sum(D_l) integers of every checked request.  The other parity tests see
only assignments and reasons, which a wrong counter on a domain the selection
did not pick leaves unchanged.

The counters of request i of a real multi-request batch are read through
kueue_tas_host_last_counters (TASFlavorSnapshot.last_counters).  The
workload-to-request mapping is proved, not assumed: the C3J configs give
every workload its own request signature, and test_mapping_is_not_shifted
checks that neighbouring workloads' counters differ there, so a shifted index
cannot pass.  Each config asserts the KUEUE_TAS_PATH_* bits it is named after
(kueue_tas_last_fill_paths); test_path_bits_union pins their union.

A request whose prelude fails before phase 1 has no counters and is skipped;
every named config must yield counters for at least three quarters of its
requests and every random generator for at least half.

A pure-Python restatement of CountIn and the roll-up over Python integers
(_ref_counters) guards the oracle and the device against a shared mistake on
snapshots without taints, selectors and affinity: synth.arith_stress_case and
hand-made edge rows (capacity 2^31 * req and (2^31 +- 1) * req, INT64_MAX,
remaining -1, request 0, request 1 against 2^31 - 1 with pods raised)."""
import copy
import ctypes
import random

import numpy as np
import pytest

import oracle_lib
from kueue_oss_amd import TASFlavorSnapshot, abi, synth

FIELDS = ("state", "sliceState", "stateWithLeader", "sliceStateWithLeader", "leaderState")
STAGED, STAGED_GT, G4, G8, G16, G32 = 1, 2, 4, 8, 16, 32
STAGED_GL, GLOBAL_STATS, EXCL, EXCL_GT, SEL_EXT = 64, 128, 256, 512, 1024
RAGGED, UNIFORM, PAIR, ENTRY_TAGS, RAGGED_PAIR, CATEGORY, LFC_FILL = 2048, 4096, 8192, 16384, 32768, 65536, 131072
FUSED_TOP = 262144
HOST, ZONE, BLOCK, RACK, GI = synth.HOST, synth.ZONE, synth.BLOCK, synth.RACK, synth.GI


# ---------------------------------------------------------------------------
# comparison
# ---------------------------------------------------------------------------
def _first_group(podsets):
    """The PodSets of a workload's first PodSet group (the run's only pass)."""
    g = podsets[0].get("podSetGroupName")
    return [podsets[0]] if g is None else [p for p in podsets if p.get("podSetGroupName") == g]


def _describe(name, i, want, got, levels):
    """First differing integer as (config, request, field, level, domain)."""
    S = want.shape[1]
    f, g = np.argwhere(want != got)[0]
    lvl, base = 0, 0
    while g >= base + len(levels[lvl]):
        base += len(levels[lvl])
        lvl += 1
    return (f"{name}: request {i} field {FIELDS[f]} level {lvl} domain {levels[lvl][g - base]}: "
            f"device {got[f, g]} oracle {want[f, g]} ({int((want != got).sum())} of {5 * S} differ)")


def _check_leaf_order(snap, levels, hostname):
    ids = snap.leaf_ids()
    assert ids == [lv[-1] if hostname else ",".join(lv) for lv in levels[-1]]


def _check(make, name, doc, wls, min_share=0.75):
    """Runs the batch on the device and compares every request's counters with
    the oracle's; returns (last_stats, oracle document)."""
    wls = [_first_group(w) for w in wls]
    want = oracle_lib.counters(doc, wls)
    levels = want["levels"]
    S = sum(len(lv) for lv in levels)
    have = [i for i, r in enumerate(want["results"]) if r["counters"] is not None]
    assert len(have) >= min_share * len(wls), (name, len(have), len(wls))
    snap = make(doc)
    try:
        snap.compile(wls)
        snap.run_compiled()
        stats = snap.last_stats()
        _check_leaf_order(snap, levels, doc["levels"][-1] == HOST)
        for i in have:
            w = np.array(want["results"][i]["counters"], dtype=np.int32).reshape(5, S)
            got = snap.last_counters(i, S)
            assert np.array_equal(w, got), _describe(name, i, w, got, levels)
    finally:
        snap.close()
    return stats, want


# ---------------------------------------------------------------------------
# named configs: one per kernel variant
# ---------------------------------------------------------------------------
def _sliced(doc_wls, topo, size, every=2, required=BLOCK):
    """Every `every`-th workload sliced at `topo` with `size` pods per slice."""
    doc, wls = doc_wls
    for k, w in enumerate(wls):
        if k % every == 0:
            tr = w[0].get("topologyRequest") or {}
            w[0]["topologyRequest"] = dict(tr, required=required, preferred=None, unconstrained=None,
                                           podSetSliceRequiredTopology=topo, podSetSliceSize=size,
                                           podsetSliceRequiredTopologyConstraints=[])
            w[0]["count"] = size * max(1, w[0]["count"] // size)
    return doc, wls


def _multilayer():
    """TASMultiLayerTopology: block slices of 8 made of rack slices of 4 made of
    host slices of 2 (fillInCountsHelper's hasInner rounding, :1680-1690)."""
    doc, wls = synth.config_c3(seed=21, n_workloads=48, shape=(2, 2, 4, 8))
    doc = dict(doc, featureGates={"TASMultiLayerTopology": True})
    for k, w in enumerate(wls):
        w[0]["requests"] = {"cpu": 7000 + 1000 * (k % 5), "amd.com/gpu": 1}
        if k % 3 != 2:
            layers = [{"topology": BLOCK, "size": 8}, {"topology": RACK, "size": 4}]
            if k % 3 == 1:
                layers.append({"topology": HOST, "size": 2})
            w[0]["topologyRequest"] = dict(required=ZONE if k % 2 else None, preferred=None, unconstrained=None,
                                           podSetSliceRequiredTopology=None, podSetSliceSize=None,
                                           podsetSliceRequiredTopologyConstraints=layers)
            w[0]["count"] = 8 * (1 + k % 4)
    return doc, wls


def _aggregated():
    """A lowest level that is not the hostname: the leaves are racks, each the
    sum of its nodes (addCapacity :243-248); taints and selectors do not apply."""
    doc, wls = synth.config_c2(seed=22, n_workloads=48, shape=(2, 3, 5, 7))
    doc = dict(doc, levels=[ZONE, BLOCK, RACK])
    doc["tasUsage"] = [dict(u, values=[f"zone-{k % 2}", f"block-{k % 2}-{k % 3}", f"rack-{k % 2}-{k % 3}-{k % 5}"])
                       for k, u in enumerate(doc["tasUsage"][:20])]
    for w in wls:
        tr = w[0].get("topologyRequest")
        if tr:
            for key in ("required", "preferred", "podSetSliceRequiredTopology"):
                if tr.get(key) == HOST:
                    tr[key] = RACK
    return doc, wls


def _narrow_generic(terms):
    """The wide-cols batch (more than 8 request columns in all) with every
    request cut to at most `terms` terms, pods included: the generic fill's
    narrower widths."""
    rng = random.Random(terms)
    doc, wls = synth.wide_case(random.Random(2), "cols", n_nodes=300, n_workloads=24)
    ext = sorted({r for n in doc["nodes"] for r in n["allocatable"] if r.startswith("example.com/")})
    for k, w in enumerate(wls):
        for ps in w:
            ps["requests"] = {r: rng.choice([1, 1, 2]) for r in rng.sample(ext, terms - 1)}
    return doc, wls


def _many_profiles():
    return synth.wide_case(random.Random(0), "profiles", n_nodes=300, n_workloads=24)


NAMED = {
    # name: (TASFlavorSnapshot keywords, builder, bits that must be set, bits that must be clear)
    "pair fan-out 2": ({}, lambda: synth.config_c3(seed=11, n_workloads=64, shape=(2, 4, 16, 2)), PAIR, 0),
    "pair fan-out 4": ({}, lambda: synth.config_c3(seed=6, n_workloads=64, shape=(2, 4, 8, 4)), PAIR, 0),
    "pair fan-out 8": ({}, lambda: synth.config_c3(seed=10, n_workloads=64, shape=(2, 4, 4, 8)), PAIR, 0),
    "pair fan-out 16": ({}, lambda: synth.config_c3(seed=5, n_workloads=64, shape=(2, 2, 4, 16)), PAIR, 0),
    "pair fan-out 32, single-run chunks": ({}, lambda: synth.config_c3(seed=3, n_workloads=384, shape=(2, 2, 4, 32)),
                                           PAIR | CATEGORY, LFC_FILL),
    "pair fan-out 64": ({}, lambda: synth.config_c3(seed=4, n_workloads=64, shape=(2, 2, 2, 64)), PAIR, 0),
    "pair fan-out 101, no fused parents": ({}, lambda: synth.config_c3(seed=7, n_workloads=64, shape=(1, 1, 3, 101)),
                                           PAIR, 0),
    "per-leaf classification": (dict(category_fill=False),
                                lambda: synth.config_c3(seed=3, n_workloads=384, shape=(2, 2, 4, 32)), PAIR, CATEGORY),
    "lfc tables in the fill": (dict(lfc_in_fill=True),
                               lambda: synth.config_c3(seed=3, n_workloads=384, shape=(2, 2, 4, 32)),
                               PAIR | CATEGORY | LFC_FILL, 0),
    "c2 mixed": ({}, lambda: synth.config_c2(seed=8, n_workloads=64, shape=(2, 2, 4, 32)), PAIR, 0),
    "c3j ragged pair, multi-run": ({}, lambda: synth.config_c3j(seed=13, n_workloads=128, shape=(2, 2, 4)),
                                   PAIR | RAGGED_PAIR, 0),
    "c3j ragged pair, parents of 1..64": ({}, lambda: synth.config_c3j(seed=71, n_workloads=24, shape=(2, 2, 3),
                                                                        rack_sizes=(1, 64)), RAGGED_PAIR, 0),
    "c3j ragged pair, a parent in pieces": ({}, lambda: synth.config_c3j(seed=551, n_workloads=12, shape=(1, 1, 3),
                                                                          rack_sizes=(150, 400)), RAGGED_PAIR, 0),
    "c3j ragged staged": (dict(pair_fill=False), lambda: synth.config_c3j(seed=71, n_workloads=24, shape=(2, 2, 3),
                                                                           rack_sizes=(1, 64)),
                          STAGED | RAGGED, PAIR | RAGGED_PAIR),
    "one-leaf staged, uniform roll-up": (dict(pair_fill=False),
                                         lambda: synth.config_c3(seed=5, n_workloads=64, shape=(2, 2, 4, 16)),
                                         STAGED | UNIFORM, PAIR),
    # rollup_top_kernel needs a fan-out of 8 or more at the level above the one the fill fuses
    # (racks per block: 32 / 4, 32 / 4, 128 / 8; hosts per rack, about 16, where the generic fill fuses nothing),
    # and rolls the levels above it up in its last block (zones; zones and blocks); the
    # BestFit half of the C3 mix takes its level maxima
    "one-leaf staged, fused top": (dict(pair_fill=False, fused_top=True),
                                   lambda: synth.config_c3(seed=3, n_workloads=96, shape=(2, 2, 8, 32)),
                                   STAGED | FUSED_TOP, PAIR),
    "pair fan-out 64, fused top": (dict(fused_top=True),
                                   lambda: synth.config_c3(seed=4, n_workloads=64, shape=(2, 2, 8, 64)),
                                   PAIR | FUSED_TOP, 0),
    "pair fan-out 2, fused top": (dict(fused_top=True),
                                  lambda: synth.config_c3(seed=11, n_workloads=64, shape=(2, 4, 16, 2)),
                                  PAIR | FUSED_TOP, 0),
    "generic fill, fused top over unfused racks": (dict(pair_fill=False, split_stats=True, fused_top=True),
                                                   lambda: synth.wide_case(random.Random(0), "cols", n_nodes=300,
                                                                           n_workloads=24),
                                                   G32 | FUSED_TOP, 0),
    # the flag set where no level qualifies (8 racks / 4 blocks): rollup_level_* / rollup_tail_kernel
    "fused top asked, fan-out too small": (dict(fused_top=True),
                                           lambda: synth.config_c3(seed=4, n_workloads=64, shape=(2, 2, 2, 64)),
                                           PAIR, FUSED_TOP),
    "wide cols: generic fill, up to 32 terms": (dict(pair_fill=False, split_stats=True),
                                                lambda: synth.wide_case(random.Random(0), "cols", n_nodes=300,
                                                                        n_workloads=24),
                                                G32 | GLOBAL_STATS | SEL_EXT, 0),
    "wide cols: generic fill, up to 16 terms": (dict(pair_fill=False, split_stats=True),
                                                lambda: synth.wide_case(random.Random(1), "cols", n_nodes=300,
                                                                        n_workloads=24),
                                                G16 | GLOBAL_STATS | SEL_EXT, G32),
    "wide cols: generic fill, 4 terms": (dict(pair_fill=False, split_stats=True), lambda: _narrow_generic(4),
                                         G4 | GLOBAL_STATS, G8 | G16 | G32),
    "wide cols: generic fill, 8 terms": (dict(pair_fill=False, split_stats=True), lambda: _narrow_generic(8),
                                         G8 | GLOBAL_STATS, G16 | G32),
    "wide profiles: split stats": (dict(pair_fill=False, split_stats=True), _many_profiles,
                                   STAGED_GT | EXCL_GT | STAGED_GL | SEL_EXT, 0),
    "wide profiles: pair": ({}, lambda: synth.wide_case(random.Random(0), "profiles", n_nodes=1600, n_workloads=24),
                            STAGED_GT | STAGED_GL | SEL_EXT | PAIR, 0),
    "wide slots: global stats": (dict(pair_fill=False, split_stats=True),
                                 lambda: synth.wide_case(random.Random(1), "slots", n_nodes=300, n_workloads=24),
                                 GLOBAL_STATS | SEL_EXT, 0),
    "split stats": (dict(pair_fill=False, split_stats=True),
                    lambda: synth.config_c3(seed=5, n_workloads=64, shape=(2, 2, 4, 16)), STAGED | EXCL, PAIR),
    "c4 leader groups": ({}, lambda: synth.config_c4(seed=9, n_workloads=8, shape=(2, 2, 4, 16)), PAIR, 0),
    "c4 leader groups, staged": (dict(pair_fill=False),
                                 lambda: synth.config_c4(seed=9, n_workloads=8, shape=(2, 2, 4, 16)), STAGED, PAIR),
    "slices at the leaf level": ({}, lambda: _sliced(synth.config_c3(seed=23, n_workloads=64, shape=(2, 2, 4, 16)),
                                                     HOST, 3), PAIR, 0),
    "slices at an upper level": ({}, lambda: _sliced(synth.config_c3(seed=24, n_workloads=64, shape=(2, 2, 4, 16)),
                                                     RACK, 4), PAIR, 0),
    "slices over ragged wide racks": ({}, lambda: _sliced(synth.config_c3j(seed=5, n_workloads=8, shape=(1, 2, 3),
                                                                            rack_sizes=(100, 300)), RACK, 4),
                                      RAGGED_PAIR, 0),
    "multi-layer inner slices": ({}, _multilayer, PAIR, 0),
    "multi-layer inner slices, staged": (dict(pair_fill=False), _multilayer, STAGED, PAIR),
    "aggregated lowest level": ({}, _aggregated, PAIR | RAGGED_PAIR, 0),
}


def _named(make_with, name):
    kw, build, must, must_not = NAMED[name]
    if not must & FUSED_TOP:
        must_not |= FUSED_TOP
    doc, wls = build()
    stats, want = _check(lambda d: make_with(d, **kw), name, doc, wls)
    paths = stats["fill_paths"]
    assert paths & must == must, (name, hex(paths))
    assert paths & must_not == 0, (name, hex(paths))
    return stats, want, wls


@pytest.mark.parametrize("name", sorted(NAMED))
def test_emulated_counters(emu_lib, name):
    _named(lambda d, **kw: TASFlavorSnapshot(d, lib=emu_lib, **kw), name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(NAMED))
def test_counters_on_gpu(name):
    _named(lambda d, **kw: TASFlavorSnapshot(d, **kw), name)


def test_path_bits_union():
    """The bits the configs assert cover every KUEUE_TAS_PATH_* bit of
    include/kueue_tas_debug.h (ENTRY_TAGS, about the entries and not phase 1,
    is asserted by the mapping test, which runs with RUN_VALUES)."""
    union = ENTRY_TAGS
    for _, _, must, _ in NAMED.values():
        union |= must
    assert union == (1 << 19) - 1, hex(union)


def _mapping(make):
    """C3J: every workload its own request signature.  Neighbouring requests'
    counters differ, so reading request i +- 1 for workload i fails _check."""
    doc, wls = synth.config_c3j(seed=13, n_workloads=128, shape=(2, 2, 4))
    want = oracle_lib.counters(doc, wls)["results"]
    differ = sum(1 for a, b in zip(want, want[1:]) if a["counters"] != b["counters"])
    assert differ >= 0.9 * (len(wls) - 1)
    S = len(want[0]["counters"]) // 5
    snap = make(doc)
    try:
        snap.compile(wls)
        snap.run_compiled(flags=TASFlavorSnapshot.RUN_COMPILE | TASFlavorSnapshot.RUN_VALUES)
        assert snap.last_stats()["fill_paths"] & ENTRY_TAGS
        for i in (0, 1, 63, 64, 126, 127):
            assert snap.last_counters(i, S).reshape(-1).tolist() == want[i]["counters"], i
        with pytest.raises(RuntimeError):
            snap.last_counters(len(wls), S)  # no such workload
        # another batch on the handle's context (a find) replaces the rows: the run's index is refused
        snap.find_topology_assignments_for_flavor(wls[3])
        with pytest.raises(RuntimeError):
            snap.last_counters(0, S)
        snap.run_compiled()
        assert snap.last_counters(0, S).reshape(-1).tolist() == want[0]["counters"]
        # a shard: the index is the workload's position in the run
        snap.set_shard([5, 77, 100])
        snap.run_compiled()
        for k, i in enumerate((5, 77, 100)):
            assert snap.last_counters(k, S).reshape(-1).tolist() == want[i]["counters"], i
        with pytest.raises(RuntimeError):
            snap.last_counters(3, S)
    finally:
        snap.close()


def test_emulated_mapping_is_not_shifted(emu_lib):
    _mapping(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_mapping_is_not_shifted_on_gpu():
    _mapping(lambda d: TASFlavorSnapshot(d))


def _chunks(make):
    """max_batch 16 over 40 requests: the last device chunk holds requests
    32..39; an earlier request's rows are gone and reading them is an error,
    never a stale row."""
    doc, wls = synth.config_c3j(seed=13, n_workloads=40, shape=(2, 2, 4))
    want = oracle_lib.counters(doc, wls)["results"]
    S = len(want[0]["counters"]) // 5
    snap = make(doc)
    try:
        snap.compile(wls)
        snap.run_compiled()
        for i in range(32, 40):
            assert snap.last_counters(i, S).reshape(-1).tolist() == want[i]["counters"], i
        for i in (0, 15, 31):
            with pytest.raises(RuntimeError):
                snap.last_counters(i, S)
    finally:
        snap.close()


def test_emulated_counters_of_the_last_chunk_only(emu_lib):
    _chunks(lambda d: TASFlavorSnapshot(d, lib=emu_lib, max_batch=16))


@pytest.mark.gpu
def test_counters_of_the_last_chunk_only_on_gpu():
    _chunks(lambda d: TASFlavorSnapshot(d, max_batch=16))


# ---------------------------------------------------------------------------
# properties the configs above must really have
# ---------------------------------------------------------------------------
def _fields(want, S):
    return np.array([r["counters"] for r in want["results"] if r["counters"] is not None], dtype=np.int64).reshape(-1, 5, S)


def test_configs_have_the_claimed_properties(emu_lib):
    make = lambda d, **kw: TASFlavorSnapshot(d, lib=emu_lib, **kw)  # noqa: E731
    # aliased simple classes, and non-leader requests (fields 2-4 derived)
    stats, want, _ = _named(make, "pair fan-out 32, single-run chunks")
    assert stats["alias_fills"] > 0 and stats["leader_evals"] == 0
    # leader groups: the leader fields are stored, and differ from the plain ones
    stats, want, wls = _named(make, "c4 leader groups")
    assert stats["leader_evals"] == len(wls)
    S = sum(len(lv) for lv in want["levels"])
    c = _fields(want, S)
    assert (c[:, 0] != c[:, 2]).any() and (c[:, 1] != c[:, 3]).any() and c[:, 4].any()
    # slices: sliceState differs from state at the slice level (leaf / upper)
    for name, lvl in (("slices at the leaf level", 3), ("slices at an upper level", 2)):
        stats, want, _ = _named(make, name)
        S = sum(len(lv) for lv in want["levels"])
        off = sum(len(lv) for lv in want["levels"][:lvl])
        c = _fields(want, S)[:, :, off: off + len(want["levels"][lvl])]
        assert ((c[:, 1] != c[:, 0]) & (c[:, 1] > 0)).any(), name
    # multi-layer: some parent's state is below the plain sum of its children
    stats, want, _ = _named(make, "multi-layer inner slices")
    assert any(r["counters"] is not None and r["params"]["sliceSizeAtLevel"] for r in want["results"])
    rounded = False
    sizes = [len(lv) for lv in want["levels"]]
    S = sum(sizes)
    for r in want["results"]:
        if r["counters"] is None or "3" not in r["params"]["sliceSizeAtLevel"]:
            continue
        st = r["counters"][:S]
        racks = st[sizes[0] + sizes[1]: sizes[0] + sizes[1] + sizes[2]]
        hosts = st[sizes[0] + sizes[1] + sizes[2]:]
        per = len(hosts) // len(racks)
        rounded |= any(racks[k] < sum(hosts[k * per: (k + 1) * per]) for k in range(len(racks)))
    assert rounded


# ---------------------------------------------------------------------------
# seeded random generators
# ---------------------------------------------------------------------------
def _random(make, gen, seed, n, min_share=0.5, want_paths=0):
    rng = random.Random(seed)
    yielded = 0
    paths = 0
    leaders = 0
    for k in range(n):
        case = gen(rng)
        wl = _first_group(case["podSets"])
        want = oracle_lib.counters(case, [wl])
        r = want["results"][0]
        if r["counters"] is None:
            continue
        yielded += 1
        S = sum(len(lv) for lv in want["levels"])
        snap = make(case)
        try:
            snap.compile([wl])
            snap.run_compiled()
            st = snap.last_stats()
            paths |= st["fill_paths"]
            leaders += st["leader_evals"]
            w = np.array(r["counters"], dtype=np.int32).reshape(5, S)
            got = snap.last_counters(0, S)
            assert np.array_equal(w, got), _describe(f"{gen.__name__} seed {seed} case {k}", 0, w, got, want["levels"])
        finally:
            snap.close()
    assert yielded >= min_share * n, (yielded, n)
    assert paths & want_paths == want_paths, hex(paths)
    return leaders


GENERATORS = {"random_case": synth.random_case, "arith_stress_case": synth.arith_stress_case,
              "affinity_case": synth.affinity_case}


@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_emulated_random_counters(emu_lib, gen):
    leaders = _random(lambda d: TASFlavorSnapshot(d, lib=emu_lib), GENERATORS[gen], 101, 60, want_paths=PAIR)
    assert leaders > 0 or gen != "random_case"  # group mode: leader fields stored


@pytest.mark.gpu
@pytest.mark.parametrize("gen", sorted(GENERATORS))
def test_random_counters_on_gpu(gen):
    _random(lambda d: TASFlavorSnapshot(d), GENERATORS[gen], 102, 60, want_paths=PAIR)


# ---------------------------------------------------------------------------
# leaves out of the snapshot after an in-place update_nodes
# ---------------------------------------------------------------------------
def _dead_leaves(make):
    doc, wls = synth.config_c3(seed=12, n_workloads=96, shape=(2, 2, 4, 32))
    gone = [copy.deepcopy(doc["nodes"][k]) for k in range(5, len(doc["nodes"]), 37)]
    for nd in gone:
        nd["conditions"] = [{"type": "Ready", "status": "False"}]
    names = {nd["name"] for nd in gone}
    # the oracle without the nodes has fewer leaves: compare leaf by name, and
    # the dead leaves must read zero in all five fields
    after = dict(doc, nodes=[nd for nd in doc["nodes"] if nd["name"] not in names])
    want = oracle_lib.counters(after, wls)
    full = oracle_lib.counters(doc, wls[:1])["levels"]
    S = sum(len(lv) for lv in full)
    Sw = sum(len(lv) for lv in want["levels"])
    pos = {}
    g = 0
    for lv in full:
        for d in lv:
            pos[tuple(d)] = g
            g += 1
    live = np.array([pos[tuple(d)] for lv in want["levels"] for d in lv])
    dead = np.setdiff1d(np.arange(S), live)
    assert len(dead) == len(gone)
    snap = make(doc)
    try:
        snap.compile(wls)
        assert not snap.update_nodes(gone)  # in place
        snap.run_compiled()
        assert snap.last_stats()["fill_paths"] & PAIR
        n = 0
        for i, r in enumerate(want["results"]):
            if r["counters"] is None:
                continue
            n += 1
            got = snap.last_counters(i, S)
            w = np.array(r["counters"], dtype=np.int32).reshape(5, Sw)
            assert not got[:, dead].any(), (i, got[:, dead])
            assert np.array_equal(got[:, live], w), _describe("dead leaves", i, w, got[:, live], want["levels"])
        assert n >= 0.75 * len(wls)
    finally:
        snap.close()


def test_emulated_dead_leaves_read_zero(emu_lib):
    _dead_leaves(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_dead_leaves_read_zero_on_gpu():
    _dead_leaves(lambda d: TASFlavorSnapshot(d))


# ---------------------------------------------------------------------------
# the raw device layer: simulateEmpty and assumed usage
# ---------------------------------------------------------------------------
def _raw_batch(snap, lib, wls, simulate_empty=False, assumed=None):
    """compile_workload per workload, one kueue_tas_eval_batch over all first
    groups; returns the indices evaluated (request k = the k-th of them)."""
    abi.bind_device_layer(lib)
    recs, tables, idx = [], [], []
    nt = 0
    for i, w in enumerate(wls):
        reqs, ng, taints, ntaints, aff, na, vals, early = snap.compile_workload(w, simulate_empty=simulate_empty)
        if early[0]:
            continue
        assert na == 0 and not (reqs[0].flags & (abi.F_AFFINITY | abi.F_SELECTOR_EXT))
        q = abi.EvalReq.from_buffer_copy(reqs[0])
        row = np.asarray(taints[: len(taints) // max(ng, 1)], dtype=np.int32)
        q.taint_table = sum(len(t) for t in tables)
        tables.append(row)
        nt = ntaints
        if assumed is not None:
            q.assumed_begin, q.assumed_end = 0, len(assumed)
        recs.append(q)
        idx.append(i)
    n = len(recs)
    arr = (abi.EvalReq * n)(*recs)
    tt = np.ascontiguousarray(np.concatenate(tables) if tables and sum(map(len, tables)) else np.full(1, -1), dtype=np.int32)
    outs = (abi.EvalOut * n)()
    offs = (ctypes.c_int64 * (n + 1))()
    ctx = snap.device_ctx()
    rc = lib.kueue_tas_eval_batch(ctx, arr, n, tt.ctypes.data, tt.size, nt,
                                  ctypes.cast(assumed, ctypes.c_void_p) if assumed is not None else None,
                                  len(assumed) if assumed is not None else 0, None, 0, None, 0, outs, offs, None, 0,
                                  None, None)
    assert rc == 0, lib.kueue_tas_last_error(ctx)
    return ctx, idx


def _raw_counters(lib, ctx, k, S):
    out = np.empty(5 * S, dtype=np.int32)
    assert lib.kueue_tas_last_counters(ctx, k, out.ctypes.data, out.size) == 0, lib.kueue_tas_last_error(ctx)
    return out.reshape(5, S)


def _raw(make, lib):
    doc, wls = synth.config_c3j(seed=13, n_workloads=48, shape=(2, 2, 4))
    snap = make(doc)
    try:
        # simulateEmpty: tasUsage ignored (:1622-1624)
        want = oracle_lib.counters(doc, wls, simulate_empty=True)
        plain = oracle_lib.counters(doc, wls)
        assert sum(a["counters"] != b["counters"] for a, b in zip(want["results"], plain["results"])) > len(wls) // 2
        S = sum(len(lv) for lv in want["levels"])
        ctx, idx = _raw_batch(snap, lib, wls, simulate_empty=True)
        assert len(idx) >= 0.75 * len(wls)
        assert lib.kueue_tas_last_fill_paths(ctx) & PAIR
        for k, i in enumerate(idx):
            w = np.array(want["results"][i]["counters"], dtype=np.int32).reshape(5, S)
            got = _raw_counters(lib, ctx, k, S)
            assert np.array_equal(w, got), _describe("simulateEmpty", i, w, got, want["levels"])
        # assumed usage (:1625-1627): gpus taken on a few leaves == the same usage in the document
        ids = snap.leaf_ids()
        picks = list(range(3, len(ids), 11))
        pods_col = _only_col(snap, {})
        q = snap.compile_workload([synth._ps("p", 1, {"amd.com/gpu": 1}, unconstrained=True)])[0][0]
        gpu_col = next(q.req_col[k] for k in range(q.num_req) if q.req_col[k] != pods_col)
        ass = (abi.Assumed * len(picks))(*[abi.Assumed(l, gpu_col, 3) for l in picks])
        doc2 = dict(doc, tasUsage=doc["tasUsage"] + [
            {"values": [ids[l]], "singlePodRequests": {"amd.com/gpu": 3}, "count": 1} for l in picks])
        want = oracle_lib.counters(doc2, wls)  # (its record also adds pods:1 there: 110 pods never bind)
        assert sum(a["counters"] != b["counters"] for a, b in zip(want["results"], plain["results"])) > len(wls) // 2
        ctx, idx = _raw_batch(snap, lib, wls, assumed=ass)
        for k, i in enumerate(idx):
            w = np.array(want["results"][i]["counters"], dtype=np.int32).reshape(5, S)
            got = _raw_counters(lib, ctx, k, S)
            assert np.array_equal(w, got), _describe("assumed usage", i, w, got, want["levels"])
    finally:
        snap.close()


def _only_col(snap, requests):
    """The device column of pods (the one term every request has)."""
    q = snap.compile_workload([synth._ps("p", 1, requests, unconstrained=True)])[0][0]
    assert q.num_req == 1
    return q.req_col[0]


def test_emulated_raw_layer_counters(emu_lib):
    _raw(lambda d: TASFlavorSnapshot(d, lib=emu_lib), emu_lib)


@pytest.mark.gpu
def test_raw_layer_counters_on_gpu():
    from kueue_oss_amd import native
    _raw(lambda d: TASFlavorSnapshot(d), native.load_library())


# ---------------------------------------------------------------------------
# an independent plain reference for the arithmetic (Python integers)
# ---------------------------------------------------------------------------
def _w32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >> 31 else x


def _w64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


def _quo(a, b):  # Go's / truncates toward zero
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _ref_count_in(req, cap):
    """Requests.CountIn (requests.go:174-217)."""
    best = None
    for name, rv in req.items():
        if name not in cap and rv != 0:
            return 0
        if rv == 0:
            count = (1 << 31) - 1
        else:
            count = max(_w32(_quo(cap.get(name, 0), rv)), 0)  # int32(capacity / request), then the clamp
        best = count if best is None else min(best, count)
    return best or 0


def _ref_counters(doc, podsets, params):
    """fillInCounts + fillInCountsHelper for a snapshot without taints,
    selectors and affinity; Ready schedulable nodes; pods of distinct names."""
    levels = doc["levels"]
    hostname = levels[-1] == HOST
    leaves = {}
    node_leaf = {}
    for n in doc["nodes"]:
        ok = not n["unschedulable"] and any(c["type"] == "Ready" and c["status"] == "True" for c in n["conditions"])
        if not ok or any(k not in n["labels"] for k in levels):
            continue
        if any(n["labels"].get(k, "") != v for k, v in (doc.get("nodeLabels") or {}).items()):
            continue
        lv = tuple(n["labels"][k] for k in levels)
        key = lv[-1] if hostname else ",".join(lv)
        leaf = leaves.setdefault(key, {"lv": lv, "free": {}, "used": {}})
        for r, v in n["allocatable"].items():
            leaf["free"][r] = _w64(leaf["free"].get(r, 0) + v)
        node_leaf[n["name"]] = key
    per_node = {}
    for p in doc.get("pods", []):
        if p["phase"] in ("Succeeded", "Failed"):
            continue
        u = per_node.setdefault(p["nodeName"], {})
        for r, v in p["requests"].items():
            u[r] = _w64(u.get(r, 0) + v)
        u["pods"] = u.get("pods", 0) + 1
    for node, u in per_node.items():
        if node in node_leaf:
            f = leaves[node_leaf[node]]["free"]
            for r, v in u.items():
                f[r] = _w64(f.get(r, 0) - v)
    for u in doc.get("tasUsage", []):
        key = ",".join(u["values"])
        if key not in leaves:
            continue
        used = leaves[key]["used"]
        for r, v in u["singlePodRequests"].items():
            used[r] = _w64(used.get(r, 0) + _w64(v * u["count"]))
        used["pods"] = _w64(used.get("pods", 0) + u["count"])
    workers, leader = podsets[0], None
    if len(podsets) > 1:
        leader = podsets[1]
        if leader["count"] > workers["count"]:
            workers, leader = leader, workers
    req = dict(workers["requests"])
    req["pods"] = _w64(req.get("pods", 0) + 1)
    lreq = None
    if leader is not None:
        lreq = dict(leader["requests"])
        lreq["pods"] = _w64(lreq.get("pods", 0) + 1)
    L = len(levels)
    ctr = [{} for _ in range(L)]  # levelValues prefix -> [state, slice, swl, sswl, leader]
    for leaf in leaves.values():
        rem = dict(leaf["free"])
        for r, v in leaf["used"].items():
            rem[r] = _w64(rem.get(r, 0) - v)
        state = _ref_count_in(req, rem)
        ls = 0
        if lreq is not None and _ref_count_in(lreq, rem) > 0:
            ls = 1
            for r, v in lreq.items():
                rem[r] = _w64(rem.get(r, 0) - v)
        ctr[L - 1][leaf["lv"]] = [state, 0, _ref_count_in(req, rem), 0, ls]
    ss, sl = params["sliceSize"], params["sliceLevelIdx"]
    inner = {int(k): v for k, v in params["sliceSizeAtLevel"].items()}
    if sl == L - 1:
        for c in ctr[L - 1].values():
            c[1], c[3] = _w32(_quo(c[0], ss)), _w32(_quo(c[2], ss))
    for lvl in range(L - 2, -1, -1):
        kids = {}
        for lv, c in ctr[lvl + 1].items():
            kids.setdefault(lv[:-1], []).append(c)
        for lv, cs in kids.items():
            state = slices = lead = 0
            diffs, sdiffs = [], []
            for c in cs:
                cstate, cswl = c[0], c[2]
                if lvl + 1 in inner:
                    cstate = _w32(_quo(c[0], inner[lvl + 1]) * inner[lvl + 1])
                    cswl = _w32(_quo(c[2], inner[lvl + 1]) * inner[lvl + 1])
                state = _w32(state + cstate)
                slices = _w32(slices + c[1])
                if not params["leader"] or c[4] > 0:
                    diffs.append(_w32(cstate - cswl))
                    sdiffs.append(_w32(c[1] - c[3]))
                lead = max(lead, c[4])
            swl = _w32(state - min(diffs)) if diffs else 0
            sswl = _w32(slices - min(sdiffs)) if diffs else 0
            if lvl == sl:
                slices, sswl = _w32(_quo(state, ss)), _w32(_quo(swl, ss))
            ctr[lvl][lv] = [state, slices, swl, sswl, lead]
    out = []
    for f in range(5):
        for lvl in range(L):
            out += [ctr[lvl][lv][f] for lv in sorted(ctr[lvl])]
    return out, [[list(lv) for lv in sorted(ctr[lvl])] for lvl in range(L)]


def _plain(case):
    """The case without taints, tolerations, selectors, affinity and repeated hostnames."""
    case = copy.deepcopy(case)
    seen = set()
    nodes = []
    for n in case["nodes"]:
        n["taints"] = []
        h = n["labels"].get(HOST, n["name"])
        if h in seen:
            continue
        seen.add(h)
        nodes.append(n)
    case["nodes"] = nodes
    case["flavorTolerations"] = []
    for ps in case["podSets"]:
        ps["tolerations"] = []
        ps["nodeSelector"] = None
        ps.pop("affinity", None)
    return case


def test_plain_reference_agrees_with_the_oracle_on_arith_stress():
    rng = random.Random(7)
    n = checked = fitting = 0
    for _ in range(300):
        case = _plain(synth.arith_stress_case(rng))
        wl = _first_group(case["podSets"])
        want = oracle_lib.counters(case, [wl])
        r = want["results"][0]
        n += 1
        if r["counters"] is None:
            continue
        got, levels = _ref_counters(case, wl, r["params"])
        assert levels == want["levels"]
        assert got == r["counters"], (case, r["params"])
        checked += 1
        fitting += any(v > 0 for v in got)
    assert checked >= n // 2 and fitting >= checked // 4
    # (the generator's pods allocatable, at most 110, bounds every leaf here:
    # the truncation is reached, a wrapping level sum is not -- the edge rows
    # below raise pods to 2^31 - 1 for that)


I31, I63 = 1 << 31, (1 << 63) - 1


def _edge_rows():
    """(name, allocatable, usage, request, expected leaf state) per leaf row;
    every leaf has pods allocatable 2^31 - 1, so the implicit pods:1 allows
    MaxInt32 and binds nowhere else.  The expected states are worked out by
    hand from requests.go:174-217: int32(capacity / request), clamped at 0."""
    big = "example.com/big"
    P = I31 - 1
    rows = []
    for req in (3, 7, 1 << 20, (1 << 31) + 3):
        rows += [
            (f"2^31 * {req}", {big: I31 * req}, None, {big: req}, 0),            # int32(2^31) = MinInt32
            (f"(2^31 - 1) * {req}", {big: (I31 - 1) * req}, None, {big: req}, P),
            (f"(2^31 + 1) * {req}", {big: (I31 + 1) * req}, None, {big: req}, 0),  # MinInt32 + 1
        ]
        if req < I31:
            rows.append((f"(2^32 + 1) * {req}", {big: (2 * I31 + 1) * req}, None, {big: req}, 1))  # wraps to 1
    rows += [
        ("INT64_MAX / 1", {big: I63}, None, {big: 1}, 0),             # int32(0x7fff...ffff) = -1
        ("INT64_MAX / 7", {big: I63}, None, {big: 7}, 0x49249249),    # 0x1249249249249249
        ("INT64_MAX / 3", {big: I63}, None, {big: 3}, 0),             # 0x2aaa...aaaa: int32 negative
        ("remaining -1", {big: 4}, {big: 5}, {big: 1}, 0),
        ("request 0", {big: 4}, None, {big: 0}, P),
        ("request 0, key missing", {}, None, {big: 0}, P),
        ("key missing", {}, None, {big: 1}, 0),
        ("1 against 2^31 - 1", {big: I31 - 1}, None, {big: 1}, P),
    ]
    return rows


def _edge_doc():
    """Two racks of edge leaves, every row once per rack plus plain leaves, so
    level sums wrap as well."""
    rows = _edge_rows()
    nodes, usage = [], []
    for r in range(2):
        for k, (name, alloc, use, _, _) in enumerate(rows):
            host = f"e{r}-{k:02d}"
            nodes.append(synth._node(host, {RACK: f"r{r}", HOST: host}, dict(alloc, pods=I31 - 1)))
            if use:
                usage.append({"values": [host], "singlePodRequests": dict(use), "count": 1})
    doc = {"levels": [RACK, HOST], "nodes": nodes, "pods": [], "tasUsage": usage, "nodeLabels": {},
           "flavorTolerations": [], "featureGates": {}}
    reqs = []
    for _, _, _, req, _ in rows:
        if req not in reqs:
            reqs.append(req)
    wls = []
    for k, req in enumerate(reqs):
        wls.append([synth._ps(f"w{k}", 4, dict(req), required=RACK)])
        wls.append([synth._ps(f"s{k}", 6, dict(req), required=RACK, slice_topo=HOST if k % 2 else RACK, slice_size=3)])
        wls.append([synth._ps("leader", 1, {"example.com/big": 1}, required=RACK, group="g"),
                    synth._ps("workers", 4, dict(req), required=RACK, group="g")])
    return doc, wls, rows


def test_edge_rows_plain_reference_and_oracle():
    doc, wls, rows = _edge_doc()
    want = oracle_lib.counters(doc, wls)
    assert all(r["counters"] is not None for r in want["results"])
    hosts = [lv[-1] for lv in want["levels"][1]]
    for wl, r in zip(wls, want["results"]):
        got, levels = _ref_counters(doc, wl, r["params"])
        assert levels == want["levels"]
        assert got == r["counters"], wl
        if len(wl) == 1:  # the rows' expected leaf states, written down by hand above
            for k, (name, _, _, req, state) in enumerate(rows):
                if req == wl[0]["requests"]:
                    assert r["counters"][2 + hosts.index(f"e0-{k:02d}")] == state, (name, wl[0]["name"])
    # the rack sums wrapped: 2 x MaxInt32 and more
    assert any(v < 0 for r in want["results"] for v in r["counters"][:2])


def _edge_rows_on_device(make):
    doc, wls, _ = _edge_doc()
    # leader classes take the staged fill over these ragged racks; without them the pair kernel runs
    stats, _ = _check(make, "edge rows", doc, wls, min_share=1.0)
    assert stats["fill_paths"] & STAGED and stats["leader_evals"] > 0
    stats, _ = _check(make, "edge rows, no leaders", doc, [w for w in wls if len(w) == 1], min_share=1.0)
    assert stats["fill_paths"] & PAIR


def test_emulated_edge_rows(emu_lib):
    _edge_rows_on_device(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_edge_rows_on_gpu():
    _edge_rows_on_device(lambda d: TASFlavorSnapshot(d))
