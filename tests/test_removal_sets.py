"""Removal sets through the raw ABI: kueue_tas_removal_tables_build
(removal_table_kernel) and kueue_tas_eval_batch_removals
(removal_expand_kernel).

The snapshot has 2 x 4 x 8 = 64 leaves and 3 resource columns (cpu, memory,
pods); a few leaves have no memory.  For every case the expected result is
kueue_tas_eval_batch with the overlay merged on the host: the request's own
assumed records plus the negated records (leaf >= 0) of the masked
candidates, sorted by leaf.  kueue_tas_eval_batch_removals must equal it word
for word: kueue_tas_eval_out (but its two reserved words, which hold the
select kernel's clock ticks), the packed entries, the taint and the resource
exclusion counts.

Tile widths the two kernels use, which case_03_tile_widths brackets:
  64    a wave: removal_expand_kernel's ballot, removal_table_kernel's list
  256   removal_expand_kernel's workgroup tile (abi.REMOVAL_EXPAND_TILE) and
        removal_table_kernel's thread stride
  2^k   removal_table_kernel's bitonic sort pads a set to a power of two
  4096  abi.REMOVAL_SET_CAP, the largest set one workgroup sorts

On CPU through the emulated build (tests/emu), on the GPU through
libkueue_tas.so."""
import ctypes
import random

import numpy as np
import pytest

from kueue_oss_amd import abi, native
from test_raw_abi import HOST, GI, _descriptor, _request, emu_lib_path

EINVAL, EOVERFLOW = -1, -5
CLASS_COLLIDE = 256
WAVE = 64
TILE = abi.REMOVAL_EXPAND_TILE
CAP = abi.REMOVAL_SET_CAP
NO_MEMORY = (5, 22, 41)  # leaves (node numbers) without a memory key


def _doc(rng):
    nodes, usage = [], []
    for i in range(64):
        b, r = i // 32, (i // 8) % 4
        alloc = {"cpu": 4000, "memory": 8 * GI, "pods": 110}
        if i in NO_MEMORY:
            del alloc["memory"]
        nodes.append({"name": f"n{i}", "labels": {"block": f"b{b}", "rack": f"b{b}-r{r}", HOST: f"n{i:03d}"},
                      "allocatable": alloc, "taints": [], "unschedulable": False,
                      "conditions": [{"type": "Ready", "status": "True"}]})
        if i not in NO_MEMORY:  # busy: most requests fit only once usage is removed
            usage.append({"values": [f"n{i:03d}"], "singlePodRequests": {"cpu": 1000, "memory": GI},
                          "count": rng.choice([2, 3, 3, 4])})
    return {"levels": ["block", "rack", HOST], "nodes": nodes, "tasUsage": usage}


class _Ctx:
    """One raw context over the 64-leaf snapshot."""

    def __init__(self, lib, seed=1, flags=0, max_batch=0):
        self.lib = abi.bind_device_layer(lib)
        self.rng = random.Random(seed)
        self.desc, self.keep, self.leaves, self.cols = _descriptor(_doc(self.rng))
        assert len(self.leaves) == 64 and self.cols == ["cpu", "memory", "pods"]
        cfg = abi.Config(0, max_batch, 0, flags)
        self.ctx = lib.kueue_tas_ctx_create(ctypes.byref(cfg))
        assert self.ctx, "kueue_tas_ctx_create"
        self.load()

    def load(self):
        assert self.lib.kueue_tas_snapshot_load(self.ctx, ctypes.byref(self.desc)) == 0, self.err()

    def err(self):
        return self.lib.kueue_tas_last_error(self.ctx).decode()

    def close(self):
        self.lib.kueue_tas_ctx_destroy(self.ctx)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def build(self, targets, sets):
        return abi.removal_tables_build(self.lib, self.ctx, targets, sets)

    def requests(self, n):
        """n varied requests (required / preferred / unconstrained, with memory)."""
        rng = self.rng
        return [_request(self.cols, rng.randrange(3), rng.choice(["required", "preferred", "unconstrained"]),
                         rng.choice([1, 2, 5, 9, 17, 40]), rng.choice([500, 1000, 2000]), rng.choice([GI, 2 * GI]))
                for _ in range(n)]

    def _run(self, reqs, assumed, rset=None, rmask=None, rc_want=0):
        n = len(reqs)
        arr = (abi.EvalReq * max(n, 1))(*reqs)
        outs = (abi.EvalOut * max(n, 1))()
        offs = (ctypes.c_int64 * (n + 1))()
        cap = 1 << 14
        ent = np.zeros(2 * cap, dtype=np.int32)
        tt = np.full(1, -1, dtype=np.int32)
        tc = np.full(max(n, 1), -7, dtype=np.int32)
        rcn = np.full(max(n, 1) * len(self.cols), -7, dtype=np.int32)
        ass = (abi.Assumed * max(len(assumed), 1))(*[abi.Assumed(*r) for r in assumed])
        pa = ctypes.cast(ass, ctypes.c_void_p) if assumed else None
        if rset is None:
            rc = self.lib.kueue_tas_eval_batch(self.ctx, arr, n, tt.ctypes.data, 1, 1, pa, len(assumed), None, 0, None,
                                               0, outs, offs, ent.ctypes.data, cap, tc.ctypes.data, rcn.ctypes.data)
        else:
            ptrs = (ctypes.c_void_p * max(n, 1))(*[ctypes.addressof(arr[i]) for i in range(n)])
            rs = np.array(rset, dtype=np.int32)
            rm = np.array(rmask, dtype=np.uint64)
            rc = self.lib.kueue_tas_eval_batch_removals(self.ctx, ptrs, n, tt.ctypes.data, 1, 1, pa, len(assumed), None,
                                                        0, None, 0, outs, offs, ent.ctypes.data, cap, tc.ctypes.data,
                                                        rcn.ctypes.data, rs.ctypes.data, rm.ctypes.data)
        assert rc == rc_want, (rc, self.err())
        if rc:
            return None
        res = []
        for i in range(n):
            o = outs[i]
            # (without `reserved`: the select kernel's clock ticks of this very run)
            res.append((bytes(o)[: abi.EvalOut.reserved.offset], ent[2 * offs[i]: 2 * offs[i + 1]].tolist(), int(tc[i]),
                        rcn[i * len(self.cols): (i + 1) * len(self.cols)].tolist()))
        return res

    def plain(self, reqs, assumed=()):
        return self._run(reqs, list(assumed))

    def removals(self, reqs, assumed, rset, rmask, rc_want=0):
        return self._run(reqs, list(assumed), rset, rmask, rc_want)

    def host_merged(self, reqs, assumed, targets, sets, rset, rmask):
        """kueue_tas_eval_batch over the overlays merged here."""
        merged, out = [], []
        for q, s, m in zip(reqs, rset, rmask):
            recs = list(assumed[q.assumed_begin: q.assumed_end])
            if s >= 0:
                for pos, t in enumerate(sets[s]):
                    if (m >> pos) & 1:
                        recs += [(leaf, col, _wrap(-d)) for leaf, col, d in targets[t] if leaf >= 0]
            recs.sort(key=lambda r: r[0])
            q2 = abi.EvalReq.from_buffer_copy(bytes(q))
            q2.assumed_begin, q2.assumed_end = len(merged), len(merged) + len(recs)
            merged += recs
            out.append(q2)
        return self._run(out, merged)

    def check(self, reqs, assumed, targets, sets, rset, rmask):
        got = self.removals(reqs, assumed, rset, rmask)
        want = self.host_merged(reqs, assumed, targets, sets, rset, rmask)
        for i, (g, w) in enumerate(zip(got, want)):
            assert g == w, (i, rset[i], hex(rmask[i]), _out(g[0]), _out(w[0]), g[1:], w[1:])
        return got


def _wrap(v):
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def _out(b):
    return np.frombuffer(b, dtype=np.int32).tolist()


def _target(rng, nrec, scale=1):
    """A preemptable workload's usage: nrec delta records over the 64 leaves x 3 columns."""
    unit = (1000, 2 * GI, 1)
    return [(leaf, col, unit[col] * rng.randint(1, 3) * scale)
            for leaf, col in (divmod(rng.randrange(192), 3) for _ in range(nrec))]


def _spread(total, parts):
    return [total // parts + (1 if k < total % parts else 0) for k in range(parts)]


def _ok(res):
    return sum(1 for r in res if _out(r[0])[0] == abi.ST_OK)


# ---- the cases (the numbers are the issue's) ----

def case_01_no_removal(lib):
    with _Ctx(lib, 101) as c:
        targets = [_target(c.rng, 12) for _ in range(4)]
        sets = [[0, 1, 2, 3]]
        assert c.build(targets, sets) == 0, c.err()
        reqs = c.requests(10)
        plain = c.plain(reqs)
        assert c.removals(reqs, [], [-1] * 10, [0xFF] * 10) == plain
        assert c.removals(reqs, [], [0] * 10, [0] * 10) == plain
        assert c.removals(reqs, [], [-1, 0] * 5, [3, 0] * 5) == plain
        got = c.check(reqs, [], targets, sets, [0] * 10, [0xF] * 10)
        assert got != plain  # (the removal is visible at all)


def case_02_one_record(lib):
    with _Ctx(lib, 102) as c:
        targets = [[(17, 0, 3000)]]
        sets = [[0]]
        assert c.build(targets, sets) == 0, c.err()
        q = _request(c.cols, 2, "required", 3, 1000, GI)  # three pods on one node: only leaf 17 can take them
        got = c.check([q], [], targets, sets, [0], [1])
        assert _out(got[0][0])[0] == abi.ST_OK and got[0][1] == [17, 3]
        assert _out(c.plain([q])[0][0])[0] != abi.ST_OK


def case_03_tile_widths(lib):
    sizes = [1, WAVE - 1, WAVE, WAVE + 1, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, CAP - 1, CAP]
    with _Ctx(lib, 103) as c:
        targets, sets = [], []
        for k in sizes:  # 7 candidates share the set's k records
            first = len(targets)
            targets += [_target(c.rng, m) for m in _spread(k, 7)]
            sets.append(list(range(first, first + 7)))
        assert c.build(targets, sets) == 0, c.err()
        stats = (ctypes.c_int64 * 4)()
        assert c.lib.kueue_tas_removal_stats(c.ctx, stats) == 0
        assert stats[0] == len(sizes) and stats[1] == sum(sizes)
        assert stats[2] <= 16 * sum(sizes) + 4 * 7 * len(sizes) + 64 * len(sizes)
        base = c.requests(4)
        reqs, rset, rmask = [], [], []
        for s in range(len(sizes)):
            for m in (0x7F, 0x55, 0x42):
                reqs.append(base[(s + m) % 4])
                rset.append(s)
                rmask.append(m)
        got = c.check(reqs, [], targets, sets, rset, rmask)
        assert 0 < _ok(got)
        assert c.lib.kueue_tas_removal_stats(c.ctx, stats) == 0 and stats[3] > 0
        # one record above the cap: refused, the tables stay
        big = targets + [_target(c.rng, CAP + 1)]
        assert c.build(big, sets + [[len(big) - 1]]) == EOVERFLOW
        assert c.removals(reqs, [], rset, rmask) == got


def case_04_candidates_64_65(lib):
    with _Ctx(lib, 104) as c:
        targets = [_target(c.rng, 2) for _ in range(63)] + [[(k, 0, 4000) for k in range(64)]] + [_target(c.rng, 2)]
        sets = [list(range(64)), list(range(63, -1, -1))]
        assert c.build(targets, sets) == 0, c.err()
        reqs = c.requests(6)
        got = c.check(reqs * 2, [], targets, sets, [0] * 6 + [1] * 6, [1 << 63] * 6 + [1 | (1 << 63)] * 6)
        assert c.build(targets, [list(range(65))]) == EINVAL
        assert c.removals(reqs * 2, [], [0] * 6 + [1] * 6, [1 << 63] * 6 + [1 | (1 << 63)] * 6) == got
        # a mask bit at or above the set's candidate count
        assert c.build(targets, [[0, 1, 2]]) == 0
        c.removals(reqs, [], [0] * 6, [8] * 6, rc_want=EINVAL)


def case_05_wrapping_sums(lib):
    with _Ctx(lib, 105) as c:
        big = 1 << 62
        targets = [[(9, 0, big)], [(9, 0, big)], [(9, 0, big), (30, 0, 2000)],  # 3 x 2^62 wraps
                   [(12, 1, 5 * GI)], [(12, 1, -5 * GI)],                        # sums to 0 on a leaf ...
                   [(5, 1, 7 * GI)], [(5, 1, -7 * GI)]]                          # ... and on one without memory
        sets = [[0, 1, 2], [3, 4, 5, 6]]
        assert c.build(targets, sets) == 0, c.err()
        reqs = c.requests(6) + [_request(c.cols, 2, "unconstrained", 64, 500, GI)]
        n = len(reqs)
        c.check(reqs * 4, [], targets, sets, [0] * n + [0] * n + [1] * n + [1] * n,
                [7] * n + [3] * n + [0xF] * n + [0x5] * n)


def case_06_empty_and_unknown(lib):
    with _Ctx(lib, 106) as c:
        t0 = _target(c.rng, 9)
        mixed = []
        for r in t0:  # leaf -1 records between the others
            mixed += [(-1, 0, 1000), r, (-1, 2, 1)]
        targets = [mixed, [], _target(c.rng, 5), [(-1, 0, 1000)] * 3]
        sets = [[0, 1, 2, 3], [], [1], [3, 1]]
        assert c.build(targets, sets) == 0, c.err()
        stats = (ctypes.c_int64 * 4)()
        assert c.lib.kueue_tas_removal_stats(c.ctx, stats) == 0 and stats[1] == 9 + 5
        reqs = c.requests(5)
        rset = [0] * 5 + [0] * 5 + [1] * 5 + [2] * 5 + [3] * 5
        rmask = [0xF] * 5 + [0xA] * 5 + [0] * 5 + [1] * 5 + [3] * 5
        got = c.check(reqs * 5, [], targets, sets, rset, rmask)
        plain = c.plain(reqs)
        # candidates without records, or with leaf -1 records only: nothing is removed
        assert got[5:10] == plain and got[10:15] == plain and got[15:20] == plain and got[20:25] == plain
        assert got[0:5] != plain


def case_07_own_assumed(lib):
    with _Ctx(lib, 107) as c:
        targets = [[(10, 0, 2000), (30, 0, 1000), (20, 1, 2 * GI)], [(20, 0, 3000), (10, 2, 1), (30, 1, GI)]]
        sets = [[0, 1], [1]]
        assert c.build(targets, sets) == 0, c.err()
        # own records before every table leaf, equal to some, between them and behind all
        own = [(0, 0, 500), (5, 0, 500), (10, 0, 1000), (10, 1, GI), (15, 0, 500), (20, 0, 1000), (25, 2, 1),
               (30, 0, 500), (40, 0, 1000), (63, 0, 2000), (63, 1, GI)]
        few = [(20, 0, 500)]
        assumed = own + few
        reqs = []
        for q in c.requests(4):
            for b, e in ((0, len(own)), (len(own), len(assumed)), (3, 7), (0, 0)):
                q2 = abi.EvalReq.from_buffer_copy(bytes(q))
                q2.assumed_begin, q2.assumed_end = b, e
                reqs.append(q2)
        n = len(reqs)
        c.check(reqs * 3, assumed, targets, sets, [0] * n + [0] * n + [1] * n, [3] * n + [2] * n + [1] * n)
        # own records and a table longer than a tile
        t_big = [_target(c.rng, 100) for _ in range(6)]
        assert c.build(t_big, [list(range(6))]) == 0, c.err()
        c.check(reqs, assumed, t_big, [list(range(6))], [0] * n, [0x2D] * n)


def case_08_missing_column(lib):
    with _Ctx(lib, 108) as c:
        leaf = NO_MEMORY[1]
        targets = [[(leaf, 1, 4 * GI)]]  # a removal on the leaf that has no memory key
        sets = [[0]]
        assert c.build(targets, sets) == 0, c.err()
        q = _request(c.cols, 2, "required", 3, 1000, GI)  # three pods on one node: the others have cpu for two
        plain = c.plain([q])[0]
        got = c.check([q], [], targets, sets, [0], [1])[0]
        assert _out(plain[0])[0] != abi.ST_OK and plain[3][1] == len(NO_MEMORY)
        assert _out(got[0])[0] == abi.ST_OK and got[1] == [leaf, 3] and got[3][1] == len(NO_MEMORY) - 1


def _case_09(lib, flags):
    with _Ctx(lib, 109, flags=flags) as c:
        targets = [[(k, 0, 3000) for k in range(0, 8)], [(k, 0, 3000) for k in range(8, 16)]]
        sets = [[0, 1], [1, 0]]
        assert c.build(targets, sets) == 0, c.err()
        q = _request(c.cols, 1, "required", 20, 1000, GI)  # 20 pods in one rack: three per freed node
        other = c.requests(3)
        reqs = [q, q, q, q, q, q] + other + other
        rset = [0, 0, 0, 0, 1, -1] + [0, 0, 0] + [1, 1, 1]
        rmask = [1, 2, 1, 3, 2, 0] + [1, 1, 1] + [2, 2, 2]
        got = c.check(reqs, [], targets, sets, rset, rmask)
        assert got[0] == got[2]                       # the same mask twice
        assert got[0] != got[1]                       # another mask: another rack
        assert got[4] == got[0]                       # set 1 position 1 is target 0 as well
        assert _out(got[5][0])[0] != abi.ST_OK        # no removal: it does not fit
        assert _out(got[0][0])[0] == abi.ST_OK and _out(got[1][0])[0] == abi.ST_OK
        assert got[6:9] == got[9:12]


def case_09_masks_in_one_batch(lib):
    _case_09(lib, 0)


def case_09_masks_class_collide(lib):
    _case_09(lib, CLASS_COLLIDE)


def case_10_second_chunk(lib):
    with _Ctx(lib, 110, max_batch=4) as c:
        targets = [_target(c.rng, 20) for _ in range(5)]
        sets = [[0, 1, 2, 3, 4], [4, 2]]
        assert c.build(targets, sets) == 0, c.err()
        reqs = c.requests(11)
        own = [(3, 0, 500), (44, 0, 500)]
        for q in reqs[5:]:
            q.assumed_begin, q.assumed_end = 0, 2
        rset = [-1, -1, -1, -1, 0, 0, 1, -1, 0, 1, 0]  # the first chunk has none
        rmask = [0, 0, 0, 0, 0x1F, 0x0A, 3, 0, 1, 2, 0x10]
        c.check(reqs, own, targets, sets, rset, rmask)


def case_11_reload_makes_stale(lib):
    with _Ctx(lib, 111) as c:
        targets = [_target(c.rng, 10), _target(c.rng, 10)]
        sets = [[0, 1]]
        reqs = c.requests(4)
        c.removals(reqs, [], [0] * 4, [1] * 4, rc_want=EINVAL)  # no tables yet
        assert c.build(targets, sets) == 0, c.err()
        got = c.check(reqs, [], targets, sets, [0] * 4, [3] * 4)
        c.load()
        c.removals(reqs, [], [0] * 4, [3] * 4, rc_want=EINVAL)
        assert "stale" in c.err()
        assert c.removals(reqs, [], [-1] * 4, [3] * 4) == c.plain(reqs)  # no set named: the plain batch
        assert c.build(targets, sets) == 0, c.err()
        assert c.check(reqs, [], targets, sets, [0] * 4, [3] * 4) == got
        assert c.lib.kueue_tas_removal_tables_clear(c.ctx) == 0
        c.removals(reqs, [], [0] * 4, [3] * 4, rc_want=EINVAL)


def case_12_rejected_tables(lib):
    with _Ctx(lib, 112) as c:
        good = [_target(c.rng, 6), _target(c.rng, 6)]
        assert c.build(good, [[0, 1]]) == 0, c.err()
        reqs = c.requests(4)
        got = c.check(reqs, [], good, [[0, 1]], [0] * 4, [3] * 4)
        for targets, sets in (
                (good, [[0, 2]]),                      # target index out of range
                (good, [[-1]]),
                ([[(64, 0, 1000)]], [[0]]),            # leaf >= N
                ([[(-2, 0, 1000)]], [[0]]),
                ([[(3, 3, 1000)]], [[0]]),             # column >= R
                ([[(3, -1, 1000)]], [[0]]),
                ([[(64, 0, 1000)], good[0]], [[1]])):  # (also in a target no set lists)
            assert c.build(targets, sets) == EINVAL, (targets, sets)
            assert c.removals(reqs, [], [0] * 4, [3] * 4) == got  # the previous tables still stand
        c.removals(reqs, [], [1] * 4, [1] * 4, rc_want=EINVAL)    # set out of range


CASES = [v for k, v in sorted(globals().items()) if k.startswith("case_")]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_emulated(emu_lib, case):
    case(native.load_library(emu_lib_path()))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_on_gpu(case):
    case(native.load_library())
