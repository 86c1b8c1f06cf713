"""kueue_tas_host_preemption_search_batch with large removal sets, against the
oracle: the cases of test_preemption_batch with every usage record of the
candidates split into m records of the same (leaf, column) whose wrapping sum
is the original delta — negative pieces and +-2^62 pairs among them — with m
chosen so that preemptor 0's set holds more than abi.REMOVAL_SET_CAP records.
The fills sum the records of a (leaf, column), so the oracle's answers for the
unsplit usage are the expected values.  Such a preemptor took the host path
before large sets; now it is built and expanded on the device
(KUEUE_TAS_RT_LARGE_SETS), and large_sets=False routes as before.

On CPU through the emulated build (tests/emu), on the GPU through
libkueue_tas.so; the oracle's answers are those test_preemption_batch caches."""
import random

import numpy as np
import pytest

import oracle_lib
from kueue_oss_amd import abi
from kueue_oss_amd.native import DELTA_DTYPE
from test_preemption_batch import (NOWHERE, _against_oracle, _cases, _decode, _oracle_assignment, _same_answers,
                                   _snap)

CAP = abi.REMOVAL_SET_CAP


def _wrap(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def _split(rng, recs, m):
    """Every record as m records of its (leaf, column) that sum to its delta in wrapping int64."""
    out = np.zeros(len(recs) * m, dtype=DELTA_DTYPE)
    k = 0
    for leaf, col, delta in recs.tolist():
        pieces = []
        while len(pieces) < m - 1:
            if m - 1 - len(pieces) >= 2 and rng.random() < 0.05:
                sign = rng.choice([-1, 1])
                pieces += [sign * (1 << 62), -sign * (1 << 62)]
            else:
                pieces.append(rng.randint(-(1 << 40), 1 << 40))
        pieces.append(_wrap(delta - sum(pieces)))
        assert _wrap(sum(pieces)) == delta and len(pieces) == m
        for d in pieces:
            out[k] = (leaf, col, d)
            k += 1
    return out


def _inflated(snap, c, seed):
    """The case's candidates as split DELTA_DTYPE arrays: preemptor 0 (every candidate) above the small cap."""
    plain = [snap.usage_deltas(u) for u in c["cands"]]
    records = sum(len(p) for p in plain)
    m = max(2, -(-(CAP + 1) // max(records, 1)))
    rng = random.Random(seed)
    split = [_split(rng, p, m) for p in plain]
    if records == 0:  # the candidates name no domain of the snapshot: records that are dropped (leaf -1)
        split[0] = np.array([(-1, 0, 1000)] * (CAP + 1), dtype=DELTA_DTYPE)
    assert sum(len(s) for s in split) >= CAP + 1
    return split


def _search(snap, c, split, **kw):
    return snap.preemption_search_batch([0, 1, 2], split, [order for _, order in c["pres"]], **kw)


def _check(lib, i):
    c = _cases(91, "random_case")[i]
    snap = _snap(c, lib)
    try:
        split = _inflated(snap, c, 1000 + i)
        before = snap.snapshot_digest()
        got = _search(snap, c, split)
        assert snap.snapshot_digest() == before
        _against_oracle(c, got)
        st = got["stats"]
        assert st["deviceSets"] == 3 and st["hostSets"] == 0
        records = sum(len(s) for s in split)
        entries = sum(len(order) for _, order in c["pres"])
        assert st["removalBytesUploaded"] <= 16 * records + 4 * entries + 64 * 3  # linear in the table
        host = _search(snap, c, split, host_overlays=True)
        _same_answers(host, got)
        assert host["stats"]["hostSets"] == 3
        small = _search(snap, c, split, large_sets=False)  # the routing before large sets
        _same_answers(small, got)
        assert small["stats"]["hostSets"] >= 1 and small["stats"]["hostSets"] + small["stats"]["deviceSets"] == 3
        assert snap.snapshot_digest() == before
    finally:
        snap.close()


# Seed 91's first six cases have no fitting prefix behind the first: case 6 (preemptor 1: firstFit 9) is the
# first whose fillBack rounds run over a large set, so the emulator takes seven.
EMU_CASES = 7
GPU_CASES = 16


@pytest.mark.parametrize("limit", [EMU_CASES, GPU_CASES])
def test_coverage(limit):
    want = [w for c in _cases(91, "random_case")[:limit] for w in c["want"]]
    assert any(w["firstFit"] >= 1 for w in want)  # a fillBack round over a large set
    assert any(w["firstFit"] < 0 for w in want) and any(w["firstFit"] == 0 for w in want)


@pytest.mark.parametrize("i", range(EMU_CASES))
def test_emulated_search_large(emu_lib, i):
    _check(emu_lib, i)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(GPU_CASES))
def test_search_large_on_gpu(i):
    _check(None, i)


def _assign(lib):
    """One case with a fitting prefix: the final assignments under large sets, then the admit path."""
    c = next(c for c in _cases(91, "random_case") if c["want"][0]["firstFit"] >= 0)
    snap, twin = _snap(c, lib), _snap(c, lib)
    try:
        split = _inflated(snap, c, 77)
        got = _search(snap, c, split, assign=True)
        _against_oracle(c, got)
        assert got["stats"]["deviceSets"] == 3 and got["stats"]["hostSets"] == 0
        quads = snap.last_assignments()
        dec = _decode(snap, quads, {p: ps for p, (ps, _) in enumerate(c["pres"])})
        results = snap.last_results()
        by_hand = {}
        for p, ((_, order), want) in enumerate(zip(c["pres"], c["want"])):
            tg = None if want["firstFit"] < 0 else [order[q] for q in want["targets"]]
            ref = _oracle_assignment(c, p, tg)
            assert results[p] == ref, (p, tg)
            assert dec[p][0] == any(r["reason"] for r in ref)
            if tg is not None:
                by_hand[p] = tg
        assert by_hand
        block = np.concatenate([[quads.size], quads]).astype(np.int32).reshape(1, -1)
        pairs, deltas = snap.admit_block(block, [quads.size], workloads=split, targets=got["targets"])
        want_pairs, want_deltas = twin.admit_with_targets(quads, c["cands"], by_hand)
        assert pairs.tolist() == want_pairs.tolist()
        assert deltas.tolist() == want_deltas.tolist()
    finally:
        snap.close()
        twin.close()


def test_emulated_assign_and_admit_large(emu_lib):
    _assign(emu_lib)


@pytest.mark.gpu
def test_assign_and_admit_large_on_gpu():
    _assign(None)


def _wide(lib):
    """70 candidates stay on the host path whatever their records; the other two sets are on the device."""
    c = next(c for c in _cases(91, "random_case") if c["want"][0]["firstFit"] >= 0)
    snap = _snap(c, lib)
    try:
        split = _inflated(snap, c, 78)
        k = len(split)
        cands = split + [NOWHERE] * (70 - k)
        order = list(range(70))
        want = oracle_lib.preemption_search(c["case"], c["setup"], c["pres"][0][0],
                                            c["cands"] + [NOWHERE] * (70 - k))
        assert want["firstFit"] >= 0
        got = snap.preemption_search_batch([0, 1, 2], cands, [order] + [o for _, o in c["pres"][1:]])
        assert got["stats"]["hostSets"] == 1 and got["stats"]["deviceSets"] == 2
        assert got["prefixFits"][0] == want["prefixFits"] and int(got["firstFit"][0]) == want["firstFit"]
        assert got["targets"][0] == want["targets"]
        for p in (1, 2):
            assert got["prefixFits"][p] == c["want"][p]["prefixFits"]
            assert int(got["firstFit"][p]) == c["want"][p]["firstFit"]
    finally:
        snap.close()


def test_emulated_more_than_64_candidates_large(emu_lib):
    _wide(emu_lib)


@pytest.mark.gpu
def test_more_than_64_candidates_large_on_gpu():
    _wide(None)
