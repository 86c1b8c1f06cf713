"""The reference's own unit vectors, pinned as data under tests/golden and
run on the oracle and on the device:

* count_in.json -- TestCountIn (8) and TestCountInWithLimitingResource (8),
  pkg/resources/requests_test.go:29-246.  Oracle: count_in_with_limiting
  called verbatim.  Device: a one-node, one-level snapshot per vector whose
  leaf's `state` counter must be the vector's count and, at count 0, whose
  failure message must name the vector's limiting resource.
* reducer_search.json -- TestSearch (9), podset_reducer_test.go:26-150.  The
  test's predicate sum(counts) <= countLimit is built through the real TAS
  fit: one node with `countLimit` of a made-up resource, every PodSet
  unconstrained and asking 1 of it; the PodSets of one find are placed one
  after another with assumed usage, so the find fits exactly when the total
  is within the limit.
* sorted_domains.json -- TestSortedDomainsWithLeader (6),
  tas_flavor_snapshot_test.go:437-517.  Oracle: sorted_domains_with_leader on
  bare domains (and sorted_domains on the same keys without a leader).
  Device: counters cannot be set freely there, so for each criterion, in the
  BestFit and LeastFreeCapacity directions, a small snapshot in which that
  criterion alone decides (checked on the oracle's phase-1 counters), whose
  assignment must equal the oracle's and use the expected prefix of domains."""
import json
import os

import pytest

import oracle_lib
from kueue_oss_amd import TASFlavorSnapshot, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HOST, BLOCK = synth.HOST, synth.BLOCK
MAX_INT32 = (1 << 31) - 1


def _load(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return json.load(fh)["vectors"]


COUNT_IN = _load("count_in.json")
REDUCER = _load("reducer_search.json")
SORTED = _load("sorted_domains.json")


def test_fixture_sizes():
    assert (len(COUNT_IN), len(REDUCER), len(SORTED)) == (16, 9, 6)
    assert sum(v["test"] == "CountIn" for v in COUNT_IN) == 8


def _doc(levels, nodes, usage=()):
    return {"levels": levels, "nodes": nodes, "pods": [], "tasUsage": list(usage), "nodeLabels": {},
            "flavorTolerations": [], "featureGates": {}}


# ---------------------------------------------------------------------------
# B1: CountIn / CountInWithLimitingResource
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("v", COUNT_IN, ids=[v["name"] for v in COUNT_IN])
def test_oracle_count_in(v):
    got = oracle_lib.unit({"op": "countIn", "requests": v["requests"], "capacity": v["capacity"]})
    assert got["count"] == v["count"]
    if v["limitingResource"] is not None:
        assert got["limitingResource"] == v["limitingResource"]


def _count_in_case(v):
    """allocatable = the capacity (an absent key stays absent), a negative
    capacity as usage above allocatable; pods 2^31 - 1 never binds and still
    allows MaxInt32."""
    alloc, use = {"pods": MAX_INT32}, {}
    for r, c in v["capacity"].items():
        alloc[r] = max(c, 0)
        if c < 0:
            use[r] = -c
    usage = [{"values": ["n0"], "singlePodRequests": use, "count": 1}] if use else []
    doc = _doc([HOST], [synth._node("n0", {HOST: "n0"}, alloc)], usage)
    return doc, [synth._ps("main", 1, dict(v["requests"]), unconstrained=True)]


def _count_in(make):
    for v in COUNT_IN:
        doc, podsets = _count_in_case(v)
        want = oracle_lib.counters(doc, [podsets])
        assert want["results"][0]["counters"][0] == v["count"], v["name"]  # the oracle through the snapshot
        snap = make(doc)
        try:
            snap.compile([podsets])
            snap.run_compiled()
            got = snap.last_counters(0, 1)
            assert got[:, 0].tolist() == want["results"][0]["counters"], v["name"]
            assert got[0, 0] == v["count"], v["name"]
            res = snap.find_topology_assignments_for_flavor(podsets)
        finally:
            snap.close()
        assert res == oracle_lib.run_case(dict(doc, podSets=podsets))["results"], v["name"]
        if v["count"] == 0:
            lim = v["limitingResource"]
            if lim is None:  # TestCountIn checks the count only: the limiting resource from the oracle's call
                lim = oracle_lib.unit({"op": "countIn", "requests": v["requests"],
                                       "capacity": v["capacity"]})["limitingResource"]
            assert not v["podsChangesLimitingResource"]
            assert f'excluded: resource "{lim}": 1' in res[0]["reason"], (v["name"], res[0]["reason"])
        else:
            assert res[0]["assignment"]["domains"] == [{"values": ["n0"], "count": 1}], v["name"]


def test_emulated_count_in(emu_lib):
    _count_in(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_count_in_on_gpu():
    _count_in(lambda d: TASFlavorSnapshot(d))


# ---------------------------------------------------------------------------
# B2: PodSetReducer.Search
# ---------------------------------------------------------------------------
SLOT = "example.com/slot"


def _reducer_case(v):
    doc = _doc([HOST], [synth._node("n0", {HOST: "n0"}, {SLOT: v["countLimit"], "pods": MAX_INT32})])
    podsets = [dict(synth._ps(p["name"], p["count"], {SLOT: 1}, unconstrained=True), minCount=p["minCount"])
               for p in v["podSets"]]
    return doc, podsets


def _oracle_search(doc, podsets):
    return oracle_lib.session(doc, [{"op": "partialAdmission", "podSets": podsets, "simulateEmpty": False}])[0]


@pytest.mark.parametrize("v", REDUCER, ids=[v["name"] for v in REDUCER])
def test_oracle_reducer_search(v):
    doc, podsets = _reducer_case(v)
    got = _oracle_search(doc, podsets)
    assert got["found"] == v["found"]
    assert sum(got["counts"] or []) == v["count"]


def _reducer(make, v):
    doc, podsets = _reducer_case(v)
    want = _oracle_search(doc, podsets)
    snap = make(doc)
    try:
        # the host API takes the empty PodSet list and the zero-count PodSet: all nine run on the device
        for mb in (0, 1):
            got = snap.partial_admission_search(podsets, max_batch=mb)
            assert {k: got[k] for k in ("found", "counts", "probes")} == \
                {k: want[k] for k in ("found", "counts", "probes")}, (v["name"], mb)
            assert got["found"] == v["found"] and sum(got["counts"] or []) == v["count"], (v["name"], mb)
    finally:
        snap.close()


@pytest.mark.parametrize("v", REDUCER, ids=[v["name"] for v in REDUCER])
def test_emulated_reducer_search(emu_lib, v):
    # (the two 150,000-pod vectors evaluate sort.Search's whole tree at max_batch 0: 2,047 and 1,169
    # eight-PodSet finds, most of this module's time on the emulator)
    _reducer(lambda d: TASFlavorSnapshot(d, lib=emu_lib), v)


@pytest.mark.gpu
@pytest.mark.parametrize("v", REDUCER, ids=[v["name"] for v in REDUCER])
def test_reducer_search_on_gpu(v):
    _reducer(lambda d: TASFlavorSnapshot(d), v)


# ---------------------------------------------------------------------------
# B3: sortedDomainsWithLeader / sortedDomains
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("v", SORTED, ids=[v["name"] for v in SORTED])
def test_oracle_sorted_domains(v):
    got = oracle_lib.unit({"op": "sortedDomains", "withLeader": True, "unconstrained": v["unconstrained"],
                           "domains": v["domains"]})
    assert got["order"] == v["wantOrder"]
    # sortedDomains (:1544-1564) orders by the same keys without the leader
    # part: the vectors whose domains agree in leaderState, their two leader
    # fields read as sliceState and state, keep their order
    if len({d["leaderState"] for d in v["domains"]}) == 1:
        plain = [{"id": d["id"], "levelValues": d["levelValues"], "sliceState": d["sliceStateWithLeader"],
                  "state": d["stateWithLeader"]} for d in v["domains"]]
        got = oracle_lib.unit({"op": "sortedDomains", "withLeader": False, "unconstrained": v["unconstrained"],
                               "domains": plain})
        assert got["order"] == v["wantOrder"]


W, LEAD = "example.com/w", "example.com/lead"
KEYS = ("leaderState", "sliceStateWithLeader", "stateWithLeader", "levelValues")

# Blocks over hostname leaves; workers ask 1 W per pod in slices of `slice`
# pods at the hostname level, the leader 1 LEAD, which only some nodes carry.
# A block is a list of hosts (W capacity, carries LEAD).  BestFit sorts the
# blocks (preferred block), LeastFreeCapacity the hosts (unconstrained: the
# lowest level), so there every block is one host.  `order` is the expected
# sortedDomainsWithLeader order, written down by hand; `decides` the one
# criterion in which the domains differ (the higher ones equal).
SORT_CASES = [
    # a block no child of which hosts the leader has stateWithLeader = sliceStateWithLeader = 0
    # (:1700-1706), so under BestFit (descending) leaderState cannot be isolated from criterion 2:
    # the case pins that the lower criteria (stateWithLeader ascending, levelValues) would say the opposite
    dict(name="BestFit leaderState", lfc=False, slice=2, decides="leaderState", order=["b", "a"],
         blocks={"a": [(8, False), (8, False)], "b": [(2, True)]}),
    dict(name="BestFit sliceStateWithLeader descending", lfc=False, slice=2, decides="sliceStateWithLeader",
         order=["a", "c", "b"], blocks={"a": [(6, True)], "b": [(2, True)], "c": [(4, True)]}),
    dict(name="BestFit stateWithLeader ascending", lfc=False, slice=4, decides="stateWithLeader",
         order=["b", "c", "a"], blocks={"a": [(6, True), (7, True)], "b": [(4, True), (4, True)],
                                        "c": [(5, True), (5, True)]}),
    dict(name="BestFit levelValues", lfc=False, slice=2, decides="levelValues", order=["a", "b", "c"],
         blocks={"c": [(4, True)], "a": [(4, True)], "b": [(4, True)]}),
    # LeastFreeCapacity alone would put the small host without the leader first
    dict(name="LeastFreeCapacity leaderState", lfc=True, slice=2, decides="leaderState", order=["b", "a"],
         blocks={"a": [(2, False)], "b": [(8, True)]}),
    dict(name="LeastFreeCapacity sliceStateWithLeader ascending", lfc=True, slice=2,
         decides="sliceStateWithLeader", order=["b", "c", "a"],
         blocks={"a": [(10, True)], "b": [(6, True)], "c": [(8, True)]}),
    dict(name="LeastFreeCapacity stateWithLeader ascending", lfc=True, slice=5, decides="stateWithLeader",
         order=["b", "c", "a"], blocks={"a": [(14, True)], "b": [(10, True)], "c": [(12, True)]}),
    dict(name="LeastFreeCapacity levelValues", lfc=True, slice=2, decides="levelValues", order=["a", "b", "c"],
         blocks={"c": [(6, True)], "a": [(6, True)], "b": [(6, True)]}),
]


def _sort_case(c):
    nodes, block_of = [], {}
    for b, hosts in c["blocks"].items():
        for k, (cap, lead) in enumerate(hosts):
            host = f"{b}-h{k}"
            alloc = {W: cap, "pods": 1000}
            if lead:
                alloc[LEAD] = 1
            nodes.append(synth._node(host, {BLOCK: b, HOST: host}, alloc))
            block_of[host] = b
    return _doc([BLOCK, HOST], nodes), block_of


def _sort_podsets(c, count):
    kw = dict(unconstrained=True) if c["lfc"] else dict(preferred=BLOCK)
    return [synth._ps("leader", 1, {LEAD: 1}, group="g", slice_topo=HOST, slice_size=1, **kw),
            synth._ps("workers", count, {W: 1}, group="g", slice_topo=HOST, slice_size=c["slice"], **kw)]


def _sort_keys(c, doc):
    """The sorted domains' five counters from the oracle's phase 1, by domain name."""
    want = oracle_lib.counters(doc, [_sort_podsets(c, c["slice"])])
    sizes = [len(lv) for lv in want["levels"]]
    S = sum(sizes)
    ctr = want["results"][0]["counters"]
    lvl = 1 if c["lfc"] else 0
    off = sum(sizes[:lvl])
    out = {}
    for k, lv in enumerate(want["levels"][lvl]):
        f = [ctr[j * S + off + k] for j in range(5)]
        out[lv[0]] = {"id": lv[0], "levelValues": [lv[0]], "state": f[0], "sliceState": f[1], "stateWithLeader": f[2],
                      "sliceStateWithLeader": f[3], "leaderState": f[4]}
    return out


def _sorted_domains(make):
    for c in SORT_CASES:
        doc, block_of = _sort_case(c)
        keys = _sort_keys(c, doc)
        doms = [keys[b] for b in c["order"]]
        # the relation the case claims: equal in the higher criteria, pairwise different in the one under test
        at = KEYS.index(c["decides"])
        for k in KEYS[:at]:
            if c["name"] == "BestFit leaderState":
                break
            assert len({json.dumps(d[k]) for d in doms}) == 1, (c["name"], k, doms)
        assert len({json.dumps(d[c["decides"]]) for d in doms}) == len(doms), (c["name"], doms)
        if c["name"] == "BestFit leaderState":
            a, b = keys["a"], keys["b"]
            assert (a["leaderState"], a["sliceStateWithLeader"], a["stateWithLeader"]) == (0, 0, 0)
            assert b["leaderState"] == 1 and b["stateWithLeader"] > 0  # ascending stateWithLeader would put a first
        if c["name"] == "LeastFreeCapacity leaderState":
            assert keys["a"]["sliceStateWithLeader"] < keys["b"]["sliceStateWithLeader"]  # ascending: a first
        # the hand-written order is the oracle's sort of those keys
        order = oracle_lib.unit({"op": "sortedDomains", "withLeader": True, "unconstrained": c["lfc"],
                                 "domains": list(keys.values())})["order"]
        assert order == c["order"], c["name"]
        # the leader's domain comes off the sortedDomainsWithLeader order, the
        # others off sortedDomains of the rest (:1291-1316); the cases' rest
        # all host the leader, so that is the same order
        rest = oracle_lib.unit({"op": "sortedDomains", "withLeader": False, "unconstrained": c["lfc"],
                                "domains": [keys[b] for b in c["order"][1:]]})["order"]
        assert rest == c["order"][1:], c["name"]
        slices = [keys[c["order"][0]]["sliceStateWithLeader"]] + [keys[b]["sliceState"] for b in c["order"][1:]]
        snap = make(doc)
        try:
            ran = 0
            for k in range(1, len(doms)):
                count = sum(slices[:k]) * c["slice"]  # needs exactly the first k domains
                if c["lfc"] and k > 1 and sum(slices[:k]) <= max(d["sliceState"] for d in doms):
                    continue  # a single larger host would take it (:1272-1279)
                podsets = _sort_podsets(c, count)
                want = oracle_lib.run_case(dict(doc, podSets=podsets))["results"]
                got = snap.find_topology_assignments_for_flavor(podsets)
                assert got == want, (c["name"], k, got, want)
                by_name = {r["name"]: r for r in got}
                assert not by_name["workers"]["reason"], (c["name"], k, by_name["workers"]["reason"])
                used = {block_of[d["values"][-1]] for d in by_name["workers"]["assignment"]["domains"]}
                assert used == set(c["order"][:k]), (c["name"], k, used)
                lead = {block_of[d["values"][-1]] for d in by_name["leader"]["assignment"]["domains"]}
                assert lead == {c["order"][0]}, (c["name"], k, lead)
                ran += 1
            assert ran >= 1, c["name"]
        finally:
            snap.close()


def test_emulated_sorted_domains(emu_lib):
    _sorted_domains(lambda d: TASFlavorSnapshot(d, lib=emu_lib))


@pytest.mark.gpu
def test_sorted_domains_on_gpu():
    _sorted_domains(lambda d: TASFlavorSnapshot(d))
