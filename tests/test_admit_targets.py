"""Admission of entries that carry preemption targets
(kueue_tas_admit_targets / kueue_tas_host_admit_targets): processEntry for a
Preempt-mode entry (pkg/scheduler/scheduler.go:419-435, fits() :621-629) —
skipped when a target is already preempted in the cycle, else Fits under
SimulateWorkloadRemoval(preempted + its targets) (snapshot.go:67-84), and on a
fit the targets join the preempted set and the entry's usage is added.

The reference is the oracle session composed per entry: with the preempted
set P tracked here, an overlap gives 2, else `remove` (usage of P + targets),
`admit` (the entry's usage), `add` (the removed usage back).

 * hand cases: the raw device layer (ctypes structs of kueue_oss_amd/abi.py)
   on a two-node snapshot;
 * random cases: the host layer on synth.config_c2, windowed and serial, the
   target-free runs through the pass and through the step kernel."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import oracle_lib
from kueue_oss_amd import TASFlavorSnapshot, abi, native, synth

HOST = "kubernetes.io/hostname"
EINVAL = -1


# ---------------------------------------------------------------------------
# hand cases: nodes x and y, cpu 4 each, A = 4 cpu on x, B = 4 cpu on y
# ---------------------------------------------------------------------------
COLS = ["cpu", "gpu", "pods"]  # sorted resource names; no node has gpu (absent from freeCapacity)
CPU, GPU, PODS = 0, 1, 2
X, Y = 0, 1


def _hand_doc():
    nodes = [{"name": n, "labels": {HOST: n}, "allocatable": {"cpu": 4, "pods": 110}, "taints": [],
              "unschedulable": False, "conditions": [{"type": "Ready", "status": "True"}]} for n in ("x", "y")]
    usage = [{"values": [n], "singlePodRequests": {"cpu": 4}, "count": 1} for n in ("x", "y")]
    return {"levels": [HOST], "nodes": nodes, "tasUsage": usage}


class _Raw:
    """A device context holding the hand snapshot."""

    def __init__(self, lib):
        self.lib = abi.bind_device_layer(lib)
        P = ctypes.POINTER
        N, R = 2, len(COLS)
        self.keep = dict(sizes=np.array([N], dtype=np.int32), co=np.zeros(1, dtype=np.int32),
                         free=np.zeros((R, N), dtype=np.int64), used=np.zeros((R, N), dtype=np.int64),
                         fp=np.zeros(N, dtype=np.uint32), up=np.zeros(N, dtype=np.uint32))
        k = self.keep
        k["free"][CPU, :] = 4
        k["free"][PODS, :] = 110
        k["fp"][:] = (1 << CPU) | (1 << PODS)
        k["used"][CPU, :] = 4
        k["used"][PODS, :] = 1
        k["up"][:] = (1 << CPU) | (1 << PODS)
        d = abi.SnapshotDesc()
        d.num_levels = 1
        d.level_sizes = k["sizes"].ctypes.data_as(P(ctypes.c_int32))
        d.child_offsets = k["co"].ctypes.data_as(P(ctypes.c_int32))
        d.num_cols = R
        d.free_capacity = k["free"].ctypes.data_as(P(ctypes.c_int64))
        d.tas_usage = k["used"].ctypes.data_as(P(ctypes.c_int64))
        d.free_present = k["fp"].ctypes.data_as(P(ctypes.c_uint32))
        d.usage_present = k["up"].ctypes.data_as(P(ctypes.c_uint32))
        d.lowest_is_hostname = 1
        cfg = abi.Config(0, 0, 0, 0)
        self.ctx = self.lib.kueue_tas_ctx_create(ctypes.byref(cfg))
        assert self.ctx, "kueue_tas_ctx_create"
        assert self.lib.kueue_tas_snapshot_load(self.ctx, ctypes.byref(d)) == 0, self.err()

    def err(self):
        return self.lib.kueue_tas_last_error(self.ctx)

    def close(self):
        self.lib.kueue_tas_ctx_destroy(self.ctx)

    @staticmethod
    def _entries(entries):
        """entries: [(leaf, count, {col: value})] one record each."""
        reqs, terms, off = [], [], [0]
        for leaf, count, single in entries:
            reqs.append(abi.FitsReq(leaf, count, len(terms), len(single)))
            terms += [abi.FitsTerm(v, c, 0) for c, v in single.items()]
            off.append(len(reqs))
        return ((abi.FitsReq * max(len(reqs), 1))(*reqs), len(reqs), (abi.FitsTerm * max(len(terms), 1))(*terms),
                len(terms), (ctypes.c_int64 * len(off))(*off))

    def fits(self, leaf, single, count=1):
        reqs, n, terms, nt, _ = self._entries([(leaf, count, single)])
        out = (ctypes.c_int32 * 1)()
        assert self.lib.kueue_tas_fits(self.ctx, reqs, n, terms, nt, out) == 0, self.err()
        return out[0]

    def add(self, leaf, col, delta):
        ds = (abi.Delta * 1)(abi.Delta(leaf, col, delta))
        assert self.lib.kueue_tas_snapshot_apply_deltas(self.ctx, ds, 1, None) == 0, self.err()

    def admit(self, entries):
        reqs, n, terms, nt, off = self._entries(entries)
        out = (ctypes.c_int32 * len(entries))()
        rc = self.lib.kueue_tas_admit(self.ctx, reqs, n, terms, nt, off, len(entries), PODS, out)
        assert rc == 0, self.err()
        return list(out)

    def admit_targets(self, entries, table, lists):
        """table: [[(leaf, col, delta)] per preemptable workload]; lists: target ids per entry."""
        reqs, n, terms, nt, off = self._entries(entries)
        flat = [abi.Delta(*r) for t in table for r in t]
        toff = np.cumsum([0] + [len(t) for t in table]).astype(np.int64)
        ids = [t for l in lists for t in l]
        eoff = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
        out = (ctypes.c_int32 * len(entries))(*([-7] * len(entries)))
        P = ctypes.POINTER
        rc = self.lib.kueue_tas_admit_targets(
            self.ctx, reqs, n, terms, nt, off, len(entries), PODS, (abi.Delta * max(len(flat), 1))(*flat),
            toff.ctypes.data_as(P(ctypes.c_int64)), len(table), (ctypes.c_int32 * max(len(ids), 1))(*ids),
            eoff.ctypes.data_as(P(ctypes.c_int64)), out)
        return rc, list(out)

    def cpu_usage_is(self, leaf, value):
        """tas_usage[cpu][leaf] == value, by probes: full at value - 4 more, one cpu free after one less."""
        self.add(leaf, CPU, 4 - value)  # capacity is 4: usage 4 fits nothing
        full = self.fits(leaf, {CPU: 1}) == 0
        self.add(leaf, CPU, -1)
        one = self.fits(leaf, {CPU: 1}) == 1 and self.fits(leaf, {CPU: 2}) == 0
        self.add(leaf, CPU, value - 3)
        return full and one


A = [(X, CPU, 4), (X, PODS, 1)]  # what RemoveUsage of workload A subtracts
B = [(Y, CPU, 4), (Y, PODS, 1)]


def _hand_1(lib):
    r = _Raw(lib)
    try:
        entries = [(X, 1, {CPU: 4}), (X, 1, {CPU: 4}), (Y, 1, {CPU: 4}), (Y, 1, {CPU: 4}), (Y, 1, {CPU: 1})]
        rc, v = r.admit_targets(entries, [A, B], [[0], [], [0, 1], [1], []])
        assert rc == 0, r.err()
        # e2 overlaps (A is preempted by e0) and must not preempt B: e3 still takes B
        assert v == [1, 0, 2, 1, 0]
        assert r.cpu_usage_is(X, 8) and r.cpu_usage_is(Y, 8)  # every target's usage is back
        assert r.fits(X, {CPU: 1}) == 0 and r.fits(Y, {CPU: 1}) == 0
    finally:
        r.close()


def _hand_2(lib):
    r = _Raw(lib)
    try:
        entries = [(X, 1, {CPU: 2}), (X, 1, {CPU: 2})]
        assert r.fits(X, {CPU: 2}) == 0  # e1 does not fit the starting usage
        rc, v = r.admit_targets(entries, [A, B], [[0], []])
        assert rc == 0, r.err()
        assert v == [1, 1]  # e1 fits only because e0 preempted A: no phase-1 finality across the removal
        assert r.cpu_usage_is(X, 8) and r.cpu_usage_is(Y, 4)
    finally:
        r.close()
    r = _Raw(lib)  # the target-free pass alone rejects both
    try:
        assert r.admit(entries) == [0, 0]
    finally:
        r.close()


def _hand_3(lib):
    r = _Raw(lib)
    try:
        entries = [(X, 1, {CPU: 100}), (X, 1, {CPU: 4}), (X, 1, {CPU: 4})]
        rc, v = r.admit_targets(entries, [A, B], [[0], [], [0]])
        assert rc == 0, r.err()
        # a rejected entry's targets do not leak (e1) and were never preempted (e2 is no overlap)
        assert v == [0, 0, 1]
        assert r.cpu_usage_is(X, 8) and r.cpu_usage_is(Y, 4)
    finally:
        r.close()


def _hand_4(lib):
    """A target whose usage names gpu, a key x's freeCapacity lacks: after
    Requests.Sub the key exists (0 - 2), so remaining gpu = 0 - (-2) = 2."""
    doc = _hand_doc()
    tgt = [{"values": ["x"], "singlePodRequests": {"gpu": 2}, "count": 1}]
    want = []
    for count in (2, 3):
        ent = [{"values": ["x"], "singlePodRequests": {"gpu": 1}, "count": count}]
        res = oracle_lib.session(doc, [{"op": "fits", "usage": ent}, {"op": "remove", "usage": tgt},
                                       {"op": "admit", "usage": ent}, {"op": "add", "usage": tgt}])
        assert res[0] is False  # without the removal the key is absent: CountIn 0
        want.append(1 if res[2] else 0)
    assert want == [1, 0]
    C = [(X, GPU, 2), (X, PODS, 1)]
    for count, w in zip((2, 3), want):
        r = _Raw(lib)
        try:
            assert r.fits(X, {GPU: 1}, count) == 0
            rc, v = r.admit_targets([(X, count, {GPU: 1})], [A, B, C], [[2]])
            assert rc == 0, r.err()
            assert v == [w]
            assert r.cpu_usage_is(X, 4)
        finally:
            r.close()


def _hand_5(lib):
    r = _Raw(lib)
    try:
        entries = [(X, 1, {CPU: 4}), (Y, 1, {CPU: 4})]
        bad_leaf = [(2, CPU, 4)]  # leaf N
        for table, lists, msg in (([A, B], [[2], []], b"target id out of range"),
                                  ([A, B], [[0, 0], []], b"twice"),
                                  ([A, bad_leaf], [[0], []], b"leaf out of range"),
                                  ([A, [(X, 3, 1)]], [[0], []], b"column out of range"),
                                  ([A, B], [[-1], []], b"target id out of range")):
            rc, v = r.admit_targets(entries, table, lists)
            assert rc == EINVAL and msg in r.err(), (rc, r.err())
            assert v == [-7, -7]
            assert r.fits(X, {CPU: 1}) == 0 and r.fits(Y, {CPU: 1}) == 0  # usage unchanged
        assert r.cpu_usage_is(X, 4) and r.cpu_usage_is(Y, 4)
        # offsets that are not monotone
        reqs, n, terms, nt, off = r._entries(entries)
        P = ctypes.POINTER
        flat = (abi.Delta * 2)(*[abi.Delta(*q) for q in A])
        out = (ctypes.c_int32 * 2)()
        for toff, eoff in (([0, 2, 1], [0, 1, 1]), ([0, 2, 2], [0, 1, 0])):
            toff, eoff = np.array(toff, dtype=np.int64), np.array(eoff, dtype=np.int64)
            rc = r.lib.kueue_tas_admit_targets(r.ctx, reqs, n, terms, nt, off, 2, PODS, flat,
                                               toff.ctypes.data_as(P(ctypes.c_int64)), 2, (ctypes.c_int32 * 1)(0),
                                               eoff.ctypes.data_as(P(ctypes.c_int64)), out)
            assert rc == EINVAL and b"monotone" in r.err()
        # a target record with leaf -1 (a domain no longer in the snapshot) is skipped
        rc, v = r.admit_targets(entries, [A + [(-1, CPU, 4)], B], [[0], []])
        assert rc == 0 and v == [1, 0], r.err()
        assert r.cpu_usage_is(X, 8) and r.cpu_usage_is(Y, 4)
    finally:
        r.close()


HAND = [_hand_1, _hand_2, _hand_3, _hand_4, _hand_5]


@pytest.mark.parametrize("case", HAND, ids=lambda f: f.__name__.strip("_"))
def test_emulated_admit_targets_hand(emu_lib, case):
    case(emu_lib)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HAND, ids=lambda f: f.__name__.strip("_"))
def test_admit_targets_hand_on_gpu(case):
    case(native.load_library())


# ---------------------------------------------------------------------------
# random cases through the host layer
# ---------------------------------------------------------------------------
def _assigned(results):
    return all(not r["reason"] for r in results)


@functools.lru_cache(maxsize=None)
def _reference(seed, n, shape, huge, forced=()):
    """The scenario and the oracle composition's answers (computed once per
    scenario, shared by the modes).  `forced`: entry indices that must carry
    targets."""
    rng = random.Random(seed)
    doc, pool_wls = synth.config_c2(seed=seed, n_workloads=max(24, n), shape=shape)
    _, wls = synth.config_c2(seed=seed + 1000, n_workloads=n, shape=shape)
    if huge:  # capacities of 2^62: the limits' preconditions fail, the exact re-check pass runs
        for nd in doc["nodes"]:
            nd["allocatable"]["memory"] = 1 << 62
    # the pool: the first batch's admitted workloads, their usage in the snapshot
    b1 = oracle_lib.session(doc, [{"op": "find", "podSets": w} for w in pool_wls])
    cand = [i for i, r in enumerate(b1) if _assigned(r)]
    setup = [{"op": "admit", "usage": synth.usage_records(pool_wls[i], b1[i])} for i in cand]
    ok = oracle_lib.session(doc, setup)
    pool_ids = [i for i, a in zip(cand, ok) if a]
    pool = [synth.usage_records(pool_wls[i], b1[i]) for i in pool_ids]
    # the second batch is evaluated with a subset of the pool removed, then the subset is back
    subset = sorted(rng.sample(range(len(pool)), max(1, len(pool) // 2)))
    removed = [{"op": "remove", "usage": pool[t]} for t in subset]
    b2 = oracle_lib.session(doc, setup + removed + [{"op": "find", "podSets": w} for w in wls])[len(setup) + len(removed):]
    usage = [synth.usage_records(w, r) if _assigned(r) else None for w, r in zip(wls, b2)]
    targets = {}
    for w in range(n):
        if usage[w] is None:
            continue
        if w in forced or rng.random() < 0.4:
            k = rng.randint(1, 3)
            # mostly from the removed subset (the capacity the entry was placed on), some from the whole pool
            src = subset if rng.random() < 0.7 else range(len(pool))
            targets[w] = sorted(rng.sample(list(src), min(k, len(src))))
    start_fits = oracle_lib.session(doc, setup + [{"op": "fits", "usage": usage[w] or []} for w in range(n)])[len(setup):]
    # processEntry per entry, the op prefix replayed
    prefix, P, verdicts = list(setup), set(), []
    for w in range(n):
        if usage[w] is None:
            verdicts.append(0)  # no assignment: never admitted
            continue
        tg = targets.get(w, [])
        if P & set(tg):
            verdicts.append(2)
            continue
        rem = [r for t in sorted(P | set(tg)) for r in pool[t]]
        step = [{"op": "remove", "usage": rem}, {"op": "admit", "usage": usage[w]}, {"op": "add", "usage": rem}]
        fit = oracle_lib.session(doc, prefix + step)[-2]
        verdicts.append(1 if fit else 0)
        if fit:
            P |= set(tg)
        prefix += step
    after = oracle_lib.session(doc, prefix + [{"op": "find", "podSets": w} for w in wls])[len(prefix):]
    return dict(doc=doc, pool_wls=pool_wls, wls=wls, pool_ids=pool_ids, pool=pool, subset=subset, b1=b1, b2=b2,
                usage=usage, targets=targets, verdicts=verdicts, after=after, start_fits=start_fits)


def _non_vacuous(ref):
    v = ref["verdicts"]
    late = [w for w in range(len(v)) if v[w] == 1 and w not in ref["targets"] and not ref["start_fits"][w]]
    return {0, 1, 2} <= set(v) and bool(late)


def _prepare(make, ref):
    """The snapshot in the state of the call: the pool admitted, the second
    batch evaluated with the subset removed, the subset back."""
    snap = make(ref["doc"])
    snap.compile(ref["pool_wls"])
    snap.run_compiled()
    assert snap.last_results() == ref["b1"]
    adm, _ = snap.admit(snap.last_assignments())
    assert [int(i) for i, a in adm.tolist() if a] == ref["pool_ids"]
    for t in ref["subset"]:
        snap.remove_usage(ref["pool"][t])
    snap.compile(ref["wls"])
    snap.run_compiled()
    assert snap.last_results() == ref["b2"]
    quads = snap.last_assignments()
    for t in ref["subset"]:
        snap.add_usage(ref["pool"][t])
    return snap, quads


def _twin(make, ref):
    """A snapshot holding the usage at the start of the call."""
    twin = make(ref["doc"])
    for u in ref["pool"]:
        twin.add_usage(u)
    return twin


def _random_case(make, seed, n, shape, huge=False, forced=()):
    ref = _reference(seed, n, shape, huge, tuple(forced))
    assert _non_vacuous(ref), "seed does not exercise every verdict"
    for w in forced:
        assert w in ref["targets"]
    snap, quads = _prepare(make, ref)
    pairs, deltas = snap.admit_with_targets(quads, ref["pool"], ref["targets"])
    runs = snap.last_admit_launches()
    snap.run_compiled()
    after = snap.last_results()
    snap.close()
    assert pairs[:, 0].tolist() == list(range(n))
    assert pairs[:, 1].tolist() == ref["verdicts"]
    assert after == ref["after"]
    # the delta list: the verdict-1 entries' updateTASUsage records (single x count per
    # resource + pods:count per domain record), which a replica applies unchanged
    want_n = sum(len(r["singlePodRequests"]) + 1 for w, v in enumerate(ref["verdicts"]) if v == 1
                 for r in ref["usage"][w])
    assert len(deltas) == want_n
    twin = _twin(make, ref)
    late = [w for w, v in enumerate(ref["verdicts"]) if v == 1 and w not in ref["targets"]
            and not twin.fits(ref["usage"][w])]
    assert late  # a target-free entry admitted only because an earlier entry preempted
    twin.compile(ref["wls"])
    twin.apply_deltas(deltas)
    twin.run_compiled()
    assert twin.last_results() == ref["after"]
    twin.close()
    return runs


EMU_SHAPE = (2, 2, 4, 8)
GPU_SHAPE = (2, 4, 8, 16)
# seeds picked on the CPU with the oracle composition alone (_non_vacuous)
EMU_CASES = {15: 4, 16: 4, 17: 4, 33: 4}
EMU_FORCED = (33, 4, (15, 16))
EMU_HUGE = (33, 3)
GPU_CASES = {96: 1}
GPU_HUGE = (96, 1)


class _StepRun:
    """KTAS_ADMIT_STEP_RUN for the contexts created inside: 0 sends every
    target-free run through the pass, the default only the long ones (the
    short ones go through admit_step_kernel)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("KTAS_ADMIT_STEP_RUN")
        if self.value is not None:
            os.environ["KTAS_ADMIT_STEP_RUN"] = self.value

    def __exit__(self, *a):
        os.environ.pop("KTAS_ADMIT_STEP_RUN", None)
        if self.old is not None:
            os.environ["KTAS_ADMIT_STEP_RUN"] = self.old


# the target-free runs through the pass ("0") at the sizes around the window, through the step kernel at all
@pytest.mark.parametrize("n,serial,step_run", [(n, s, None) for n in sorted(EMU_CASES) for s in (False, True)] +
                         [(16, False, "0"), (17, True, "0"), (33, False, "0"), (33, True, "0")])
def test_emulated_admit_targets_random(emu_lib, n, serial, step_run):
    with _StepRun(step_run):
        runs = _random_case(lambda d: TASFlavorSnapshot(d, lib=emu_lib, serial_admit=serial), EMU_CASES[n], n, EMU_SHAPE)
    assert runs[0] > 0 if step_run == "0" else runs[1] > 0


@pytest.mark.parametrize("serial,step_run", [(False, None), (True, None), (False, "0")])
def test_emulated_admit_targets_window_edge(emu_lib, serial, step_run):
    n, seed, forced = EMU_FORCED  # target entries at indices 15 and 16 (kAdmitWindow is 16)
    with _StepRun(step_run):
        _random_case(lambda d: TASFlavorSnapshot(d, lib=emu_lib, serial_admit=serial), seed, n, EMU_SHAPE, forced=forced)


@pytest.mark.parametrize("serial,step_run", [(False, None), (True, None), (False, "0")])
def test_emulated_admit_targets_huge_memory(emu_lib, serial, step_run):
    n, seed = EMU_HUGE
    with _StepRun(step_run):
        _random_case(lambda d: TASFlavorSnapshot(d, lib=emu_lib, serial_admit=serial), seed, n, EMU_SHAPE, huge=True)


@pytest.mark.gpu
@pytest.mark.parametrize("step_run", [None, "0"])
@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("huge", [False, True])
def test_admit_targets_random_on_gpu(huge, serial, step_run):
    n, seed = GPU_HUGE if huge else (96, GPU_CASES[96])
    with _StepRun(step_run):
        _random_case(lambda d: TASFlavorSnapshot(d, serial_admit=serial), seed, n, GPU_SHAPE, huge=huge)


def _no_targets_is_admit(make, seed, n, shape):
    """Every target list empty: the verdicts, the deltas and last_admit_stats
    are admit()'s on a twin snapshot, and so is the kernel sequence (one run,
    no step kernel)."""
    ref = _reference(seed, n, shape, False)
    a, qa = _prepare(make, ref)
    b, qb = _prepare(make, ref)
    assert np.array_equal(qa, qb)
    pa, da = a.admit_with_targets(qa, ref["pool"], {})
    pb, db = b.admit(qb)
    assert pa.tolist() == pb.tolist() and set(pa[:, 1].tolist()) <= {0, 1}
    assert np.array_equal(da, db)
    assert a.last_admit_stats() == b.last_admit_stats()
    assert a.last_admit_launches() == b.last_admit_launches() and a.last_admit_launches()[:2] == (1, 0)
    # and with a table but only empty lists
    a.close()
    a, qa = _prepare(make, ref)
    pa, da = a.admit_with_targets(qa, ref["pool"], {w: [] for w in range(n)})
    assert pa.tolist() == pb.tolist() and np.array_equal(da, db)
    assert a.last_admit_stats() == b.last_admit_stats() and a.last_admit_launches() == b.last_admit_launches()
    a.close()
    b.close()


@pytest.mark.parametrize("serial", [False, True])
def test_emulated_admit_targets_empty_lists(emu_lib, serial):
    _no_targets_is_admit(lambda d: TASFlavorSnapshot(d, lib=emu_lib, serial_admit=serial), EMU_CASES[33], 33, EMU_SHAPE)


@pytest.mark.gpu
def test_admit_targets_empty_lists_on_gpu():
    _no_targets_is_admit(lambda d: TASFlavorSnapshot(d), GPU_CASES[96], 96, GPU_SHAPE)


def test_emulated_admit_targets_host_errors(emu_lib):
    ref = _reference(EMU_CASES[16], 16, EMU_SHAPE, False)
    entry = next(iter(ref["targets"]))
    for targets, msg in (({entry: [len(ref["pool"])]}, "target id out of range"),
                         ({10**6: [0]}, "not in the batch"),
                         ([(entry, [0]), (entry, [1])], "given twice")):
        snap, quads = _prepare(lambda d: TASFlavorSnapshot(d, lib=emu_lib), ref)  # (an error ends the handle)
        with pytest.raises(RuntimeError, match=msg):
            snap.admit_with_targets(quads, ref["pool"], targets)
        snap.close()
    # a target usage record for a domain the snapshot does not know is skipped
    snap, quads = _prepare(lambda d: TASFlavorSnapshot(d, lib=emu_lib), ref)
    pool = [u + [{"values": ["no-such-domain"], "singlePodRequests": {"cpu": 1}, "count": 1}] for u in ref["pool"]]
    pairs, _ = snap.admit_with_targets(quads, pool, ref["targets"])
    assert pairs[:, 1].tolist() == ref["verdicts"]
    snap.close()
