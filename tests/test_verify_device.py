"""kueue_tas_host_snapshot_digest / kueue_tas_host_verify_device: the host
mirror against what the device holds.

 1. seeded sessions on synth.random_case snapshots (<= 64 nodes, ~30
    operations: pod and node events, usage updates, admissions with and
    without preemption targets, other ranks' deltas, requests that add a
    column) stay clean after every operation; after admit_with_targets the
    usage words also equal the numpy digest (test_snapshot_digest's second
    statement of the hash) of the usage read before the call plus the returned
    delta list — the header's "bit for bit";
 2. divergence injected through the raw context behind the mirror's back is
    named by leaf and field, and a later legitimate push of those leaves makes
    the snapshot clean again;
 3. the digest is keyed by name: a request that adds a resource column leaves
    the words of the columns that existed unchanged.

On CPU through the emulated build (tests/emu), on the GPU through libkueue_tas.so."""
import copy
import random

import numpy as np
import pytest

from kueue_oss_amd import TASFlavorSnapshot, abi, synth
from kueue_oss_amd.native import DELTA_DTYPE
from test_snapshot_digest import USAGE, U64, elem
from test_snapshot_events import node_events, pod_events

HOST = "kubernetes.io/hostname"
GI = 1 << 30
READY = [{"type": "Ready", "status": "True"}]


def _clean(snap, what):
    v = snap.verify_device()
    assert v["ok"] and not v["components"] and not v["leaves"] and v["mismatchedLeaves"] == 0, (what, v)


def _usage_words(rows, deltas):
    """{resource: word} of the usage rows read before a call plus its delta list"""
    used = np.ascontiguousarray(rows["usage"].T).view(U64).copy()  # [R, N], wrapping sums
    up = rows["usage_present"].copy()
    for leaf, col, delta in deltas.tolist():
        used[col, leaf] = U64((int(used[col, leaf]) + delta) % (1 << 64))
        up[leaf] |= np.uint32(1 << col)
    idx = np.arange(up.size, dtype=U64)
    out = {}
    for c, name in enumerate(rows["resources"]):
        bit = ((up >> np.uint32(c)) & np.uint32(1)).astype(bool)
        out[name] = "%016x" % int(elem(USAGE, idx[bit], used[c][bit]).sum(dtype=U64)) if bit.any() else "0" * 16
    return out


def _latest(ref):
    latest = {}
    for nd in ref["nodes"]:
        latest[nd["name"]] = nd
    return latest


OPS = ("pods", "nodes", "nodes", "away", "join", "second", "usage", "usage", "remove", "admit", "admit_targets",
       "deltas", "column")


def _session(make, seed, stats):
    rng = random.Random(seed)
    case = synth.random_case(rng, max_nodes=64)
    snap = make(case)
    try:
        ref = copy.deepcopy(case)
        ref.setdefault("pods", [])
        ps = case["podSets"]
        pool = []
        _clean(snap, (seed, "create"))
        for step in range(30):
            op = rng.choice(OPS)
            at = (seed, step, op)
            live = [n for n in _latest(ref).values() if not n.get("unschedulable") and
                    (n.get("conditions") or READY)[0]["status"] == "True"]
            if op == "pods":
                evs = pod_events(rng, ref, rng.randint(1, 4))
                snap.update_pods(evs)
                ref["pods"] += evs
            elif op == "nodes":
                evs = node_events(rng, ref, rng.randint(1, 3))
                if evs:
                    stats["rebuilt" if snap.update_nodes(evs) else "inplace"] += 1
                    ref["nodes"] = ref["nodes"] + evs
            elif op == "away" and live:  # leaves, an event while away, returns
                nd = copy.deepcopy(rng.choice(live))
                gone = dict(nd, conditions=[{"type": "Ready", "status": "False"}])
                snap.update_nodes([gone])
                ref["nodes"] = ref["nodes"] + [gone]
                _clean(snap, at + ("left",))
                ev = [{"namespace": "aw", "name": f"a{step}", "nodeName": nd["name"], "phase": "Running",
                       "requests": {"cpu": 250}}]
                snap.update_pods(ev)
                ref["pods"] += ev
                if HOST in nd["labels"] and case["levels"][-1] == HOST:
                    snap.add_usage([{"values": [nd["labels"][HOST]], "singlePodRequests": {"cpu": 100}, "count": 1}])
                _clean(snap, at + ("while away",))
                nd["conditions"] = READY
                snap.update_nodes([nd])
                ref["nodes"] = ref["nodes"] + [nd]
            elif op in ("join", "second") and live:
                nd = copy.deepcopy(rng.choice(live))
                nd["name"] = f"{op}-{seed}-{step}"
                if op == "join" and HOST in nd["labels"]:  # a new leaf in the middle of the numbering
                    nd["labels"][HOST] = nd["labels"][HOST] + "-j"
                before = snap.snapshot_counters()[1]
                snap.update_nodes([nd])
                stats["splices"] += snap.snapshot_counters()[1] - before
                ref["nodes"] = ref["nodes"] + [nd]
            elif op == "usage":
                u = synth.usage_records(ps, snap.find_topology_assignments_for_flavor(ps))
                if u:
                    snap.add_usage(u)
                    pool.append(u)
            elif op == "remove" and pool:
                snap.remove_usage(pool.pop(rng.randrange(len(pool))))
            elif op == "admit":
                snap.compile([ps] * 3)
                snap.run_compiled()
                adm, deltas = snap.admit(snap.last_assignments())
                stats["admitted"] += int(adm[:, 1].sum())
            elif op == "admit_targets" and pool:
                snap.compile([ps] * 3)
                snap.run_compiled()
                quads = snap.last_assignments()
                targets = pool[: rng.randint(1, min(3, len(pool)))]
                snap.usage_deltas([r for u in targets for r in u])  # every resource a column before the readback
                rows = snap.read_leaves()
                lists = {0: [0], 2: list(range(len(targets)))}
                pairs, deltas = snap.admit_with_targets(quads, targets, lists)
                stats["target_verdicts"] += [int(v) for i, v in pairs.tolist() if i in lists]
                got = snap.snapshot_digest()
                assert list(got["usage"]) == rows["resources"], at
                assert got["usage"] == _usage_words(rows, deltas), at  # usage before + the delta list, bit for bit
            elif op == "deltas":
                d = snap.snapshot_digest()
                if d["leaves"] and d["free"]:
                    recs = [(rng.randrange(d["leaves"]), rng.randrange(len(d["free"])), rng.choice([1, -5, 1 << 40]))
                            for _ in range(rng.randint(1, 4))]
                    snap.apply_deltas(np.array(recs, dtype=DELTA_DTYPE))
            elif op == "column":
                extra = copy.deepcopy(ps)
                extra[0]["requests"] = dict(extra[0]["requests"], **{f"example.com/extra{step}": 1})
                snap.find_topology_assignments_for_flavor(extra)
            _clean(snap, at)
    finally:
        snap.close()


def _sessions(make, seeds):
    stats = dict(rebuilt=0, inplace=0, splices=0, admitted=0, target_verdicts=[])
    for seed in seeds:
        _session(make, seed, stats)
    # the sessions reach every kind of change: rebuilds, in-place events, splices, admissions, admitted entries
    # that preempt (verdict 1 with targets: the usage subtracted and added back)
    assert stats["rebuilt"] and stats["inplace"] and stats["splices"] and stats["admitted"], stats
    assert 1 in stats["target_verdicts"], stats
    return stats


def test_emulated_sessions_stay_clean(emu_lib):
    _sessions(lambda d: TASFlavorSnapshot(d, lib=emu_lib), (302, 304, 308))


@pytest.mark.gpu
def test_sessions_stay_clean_on_gpu():
    _sessions(lambda d: TASFlavorSnapshot(d), range(300, 312))


# ---------------------------------------------------------------------------
# 2. injected divergence
# ---------------------------------------------------------------------------
def _big_doc(n=2100):
    nodes = []
    for i in range(n):
        name = f"h{i:05d}"
        labels = {"block": f"b{i // 700}", "rack": f"r{i // 35:03d}", HOST: name, "zone": "ab"[i % 2]}
        nodes.append({"name": name, "labels": labels, "allocatable": {"cpu": 8000, "memory": 16 * GI, "pods": 110},
                      "taints": [{"key": "k", "value": "v", "effect": "NoSchedule"}] if i % 3 == 0 else [],
                      "unschedulable": False, "conditions": READY})
    return {"levels": ["block", "rack", HOST], "nodes": nodes, "pods": [], "tasUsage": []}


def _report(snap):
    v = snap.verify_device()
    assert v["mismatchedLeaves"] == len(v["leaves"]) <= 64
    return v["ok"], sorted(v["components"]), {(e["leaf"], e["id"]): sorted(e["fields"]) for e in v["leaves"]}


def _injected(make):
    doc = _big_doc()
    snap = make(doc)
    try:
        lib = abi.bind_device_layer(snap._lib)
        ctx = snap.device_ctx()
        ids = snap.leaf_ids()
        assert ids == [n["name"] for n in doc["nodes"]]  # leaf i is node i
        by_name = {n["name"]: n for n in doc["nodes"]}
        _clean(snap, "create")

        def set_free(leaves, change):
            rows = snap.read_leaves(leaves)
            free, fp = rows["free"].copy(), rows["free_present"].copy()
            change(free, fp, rows["resources"])
            ls = np.ascontiguousarray(leaves, dtype=np.int32)
            assert lib.kueue_tas_snapshot_set_free(ctx, ls.ctypes.data, ls.size, free.ctypes.data, fp.ctypes.data) == 0

        def pod_on(leaves, tag):  # a legitimate push of the leaves' free rows
            snap.update_pods([{"namespace": tag, "name": f"p{l}", "nodeName": ids[l], "phase": "Running",
                               "requests": {"cpu": 100}} for l in leaves])

        # one leaf, one value
        def one(free, fp, res):
            free[0, res.index("cpu")] += 1
        set_free([7], one)
        assert _report(snap) == (False, ["free:cpu"], {(7, ids[7]): ["free:cpu"]})
        pod_on([7], "a")
        _clean(snap, "after the push of leaf 7")

        # eight leaves across the two chunks: values in the first, a presence bit in the second
        eight = [3, 700, 1500, 2047, 2048, 2049, 2090, 2099]

        def many(free, fp, res):
            for q, leaf in enumerate(eight):
                if leaf < 2048:
                    free[q, res.index("memory")] ^= 1 << 40
                else:
                    fp[q] &= ~np.uint32(1 << res.index("pods"))
        set_free(eight, many)
        want = {(l, ids[l]): ["free:memory" if l < 2048 else "free:pods"] for l in eight}
        assert _report(snap) == (False, ["free:memory", "free:pods"], want)
        pod_on(eight[:4], "b")
        assert _report(snap) == (False, ["free:pods"], {k: v for k, v in want.items() if k[0] >= 2048})
        pod_on(eight[4:], "c")
        _clean(snap, "after the push of the eight leaves")

        # taint profile and a label id
        rows = snap.read_leaves([11, 2060])
        zone = rows["labelKeys"].index("zone")
        prof, lab = rows["profiles"].copy(), rows["labels"].copy()
        prof[0] = 1 - prof[0]
        lab[1, zone] = 3 - lab[1, zone]  # the two zone values have ids 1 and 2
        assert set(rows["profiles"].tolist()) <= {0, 1} and rows["labels"][1, zone] in (1, 2)
        ls = np.array([11, 2060], dtype=np.int32)
        assert lib.kueue_tas_snapshot_set_leaf_attrs(ctx, ls.ctypes.data, 2, prof.ctypes.data, lab.ctypes.data) == 0
        assert _report(snap) == (False, ["label:zone", "taints"],
                                 {(11, ids[11]): ["taints"], (2060, ids[2060]): ["label:zone"]})
        for l in (11, 2060):  # an in-place node update pushes the leaf's profile and labels
            nd = copy.deepcopy(by_name[ids[l]])
            nd["allocatable"]["cpu"] = 9000
            assert snap.update_nodes([nd]) is False
        _clean(snap, "after the node updates")

        # liveness
        live = np.zeros(1, dtype=np.int32)
        ls = np.array([2051], dtype=np.int32)
        assert lib.kueue_tas_snapshot_set_leaf_live(ctx, ls.ctypes.data, 1, live.ctypes.data) == 0
        assert _report(snap) == (False, sorted(["live", "taints", "free:cpu", "free:memory", "free:pods"] +
                                               ["label:" + k for k in rows["labelKeys"]]),
                                 {(2051, ids[2051]): ["live"]})
        gone = dict(copy.deepcopy(by_name[ids[2051]]), conditions=[{"type": "Ready", "status": "False"}])
        assert snap.update_nodes([gone]) is False  # the node leaves in place: the mirror pushes the leaf out
        _clean(snap, "after the node left")
        assert snap.update_nodes([by_name[ids[2051]]]) is False
        _clean(snap, "after the node returned")
    finally:
        snap.close()


def test_emulated_injected_divergence(emu_lib):
    _injected(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_injected_divergence_on_gpu():
    _injected(lambda d: TASFlavorSnapshot(d))


# ---------------------------------------------------------------------------
# 3. keyed by name
# ---------------------------------------------------------------------------
def _by_name(make):
    doc, wls = synth.config_c1()
    snap = make(doc)
    try:
        a = snap.snapshot_digest()
        assert a["leaves"] == len(snap.leaf_ids()) and a["chunkLeaves"] == 2048
        assert len(a["chunks"]) == (a["leaves"] + 2047) // 2048
        assert set(a["free"]) == set(a["usage"]) and "pods" in a["free"] and list(a["free"]) == sorted(a["free"])
        for w in [a["topology"], a["live"], a["taints"], a["tags"], *a["free"].values(), *a["chunks"]]:
            assert len(w) == 16 and int(w, 16) >= 0
        ps = copy.deepcopy(wls[0])
        ps[0]["requests"] = dict(ps[0]["requests"], **{"aaa.example.com/first": 1})  # sorts before every column
        snap.find_topology_assignments_for_flavor(ps)
        b = snap.snapshot_digest()
        assert list(b["free"])[0] == "aaa.example.com/first" and set(b["free"]) == set(a["free"]) | {"aaa.example.com/first"}
        for kind in ("free", "usage", "labels"):
            for name, w in a[kind].items():
                assert b[kind][name] == w, (kind, name)
        assert b["free"]["aaa.example.com/first"] == b["usage"]["aaa.example.com/first"] == "0" * 16  # on no leaf
        assert (b["live"], b["taints"], b["chunks"]) == (a["live"], a["taints"], a["chunks"])
        assert b["topology"] != a["topology"]  # R is part of the sequence
        _clean(snap, "after the new column")
    finally:
        snap.close()


def test_emulated_digest_keyed_by_name(emu_lib):
    _by_name(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_digest_keyed_by_name_on_gpu():
    _by_name(lambda d: TASFlavorSnapshot(d))
