"""Admission with preemption targets from the gathered device block
(admit_block(..., workloads=, targets=) -> kueue_tas_host_admit_block_targets)
against the only route without it: kueue_tas_copy_to_host of the block's rows,
then admit_with_targets (JSON targets) over the quads.  One evaluated C3 batch
(131,072 nodes) per size: 1,024 candidates in one row and 8,192 in 8 rows
(workloads dealt to the rows by id % 8), the block resident on the device as
the all-gather leaves it.  Three warm-ups, ten timed repeats per leg, the two
sides alternating in one process; median and p10 / p90 of the host wall time
of the call(s), which end in a device synchronise.

Legs: 0 %, 1 % and 10 % of the entries carry 1-2 targets from a pool of
workloads admitted beforehand.  The block side's target table is built once
per leg (usage_deltas per named workload, untimed and reported: a caller
holds those records from the workloads' admission).  In the 0 % leg plain
admit_block of the base library (--base-lib: a build of the parent commit;
default this build) runs as a third side: the block side without targets is
the same launch sequence, and that leg's spread is the run's noise floor;
this build's plain admit_block and a call that names 64 entries with empty
lists (their ids checked against the headers) are timed beside them.
Asserted per repeat: identical verdicts on every side, and that the block
side ran on the device (last_admit_block_path).  Between repeats the admitted
usage is taken out again (apply_deltas of the negated list, untimed).

usage: python tools/admit_block_targets_ab.py [--base-lib PATH] [--out profiles/admit_block_targets.json]
       [--sizes 1024:1,8192:8] [--pool 256] [--repeats 10] [--warmup 3] [--config C3]
       [--lib PATH --shape 2,2,4,8: a rehearsal on another build at a small size]"""
import argparse
import ctypes
import json
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
from admit_targets_ab import assigned, load_base, prepare, stats, undo  # noqa: E402
from kueue_oss_amd import native, synth  # noqa: E402


def dealt_block(quads, world):
    """Rows [len, quads...] of one capacity, workloads dealt by id % world."""
    q4 = np.asarray(quads, dtype=np.int32).reshape(-1, 4)
    rows = [np.ascontiguousarray(q4[q4[:, 0] % world == r]).ravel() for r in range(world)]
    blk = np.zeros((world, max(r.size for r in rows) + 1), dtype=np.int32)
    for r, row in enumerate(rows):
        blk[r, 0] = row.size
        blk[r, 1:1 + row.size] = row
    return blk, np.array([r.size for r in rows], dtype=np.int64)


def rows_to_host(snap, lib, dev, lens):
    """The fallback's copy: each row's quads from the device block (kueue_tas_copy_to_host)."""
    lib.kueue_tas_copy_to_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    ctx = snap.device_ctx()
    out = np.empty(int(lens.sum()), dtype=np.int32)
    at = 0
    for r in range(dev.shape[0]):
        n = int(lens[r])
        row = dev[r].data_ptr() if hasattr(dev, "data_ptr") else dev[r].ctypes.data
        if n and lib.kueue_tas_copy_to_host(ctx, out[at:].ctypes.data, row + 4, n * 4):
            raise RuntimeError("kueue_tas_copy_to_host")
        at += n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--base-lib", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--sizes", default="1024:1,8192:8")
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shape", default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    gen = synth.CONFIGS[a.config]
    kw = {"shape": tuple(int(x) for x in a.shape.split(","))} if a.shape else {}
    new_lib = native.load_library(a.lib) if a.lib else None
    base_lib = load_base(a.base_lib) if a.base_lib else new_lib
    out = {"config": a.config, "pool_requested": a.pool, "repeats": a.repeats, "warmup": a.warmup,
           "base_lib": a.base_lib or "this build", "sizes": [],
           "note": "one GPU, the block resident on the device; rank-0 admission with targets at 8 GPUs was not measured"}
    for size in a.sizes.split(","):
        n, world = (int(x) for x in size.split(":"))
        doc, wls = gen(n_workloads=n, **kw)
        _, pool_wls = gen(seed=4242, n_workloads=a.pool, **kw)
        new, quads, pool, subset, b2 = prepare(doc, pool_wls, wls, new_lib, 1)
        base, quads_b, _, _, _ = prepare(doc, pool_wls, wls, base_lib, 1)
        assert np.array_equal(quads, quads_b)
        blk, lens = dealt_block(quads, world)
        dev = blk if a.lib else torch.from_numpy(blk).to("cuda:0")  # (--lib: the emulator's device memory is the host's)
        if not a.lib:
            torch.cuda.synchronize()
        eligible = [w for w in range(n) if assigned(b2[w])]
        entry = {"entries": n, "rows": world, "block_bytes": int(blk.nbytes), "pool": len(pool), "legs": []}
        for frac in (0.0, 0.01, 0.10):
            rng = random.Random(int(frac * 1000) + 7)
            chosen = sorted(rng.sample(eligible, int(round(frac * n))))
            targets = {w: sorted(rng.sample(subset if rng.random() < 0.7 else range(len(pool)), rng.randint(1, 2)))
                       for w in chosen}
            named = sorted({t for ts in targets.values() for t in ts})
            table = [pool[t] for t in named]  # the JSON side's table
            lists = {w: [named.index(t) for t in ts] for w, ts in targets.items()}
            t0 = time.perf_counter()
            table_d = [new.usage_deltas(u) for u in table]  # the block side's, once per cycle
            table_ms = (time.perf_counter() - t0) * 1e3
            t_blk, t_fall, t_plain, t_own, t_emp = [], [], [], [], []
            for rep in range(a.warmup + a.repeats):
                t0 = time.perf_counter()
                pairs, d_new = new.admit_block(dev, lens, workloads=table_d, targets=lists)
                t1 = time.perf_counter()
                assert new.last_admit_block_path() == "device"
                launches = new.last_admit_launches()
                undo(new, d_new)
                v_new = pairs[:, 1].tolist()
                t2 = time.perf_counter()
                q = rows_to_host(base, base._lib, dev, lens)
                pb, d_base = base.admit_with_targets(q, table, lists)
                t3 = time.perf_counter()
                undo(base, d_base)
                assert pairs[:, 0].tolist() == pb[:, 0].tolist() and v_new == pb[:, 1].tolist(), "the two routes disagree"
                assert len(d_new) == len(d_base)
                if frac == 0.0:
                    t4 = time.perf_counter()
                    pp, d_plain = base.admit_block(dev, lens)
                    t5 = time.perf_counter()
                    undo(base, d_plain)
                    assert pp[:, 1].tolist() == v_new
                    t6 = time.perf_counter()
                    pq, d_own = new.admit_block(dev, lens)  # this build's plain call
                    t7 = time.perf_counter()
                    undo(new, d_own)
                    assert pq[:, 1].tolist() == v_new
                    t8 = time.perf_counter()
                    pe, d_emp = new.admit_block(dev, lens, workloads=table_d, targets={w: [] for w in eligible[:64]})
                    t9 = time.perf_counter()  # ids given with empty lists: checked against the headers, then the plain launches
                    assert new.last_admit_block_path() == "device" and new.last_admit_launches() == launches
                    undo(new, d_emp)
                    assert pe[:, 1].tolist() == v_new
                if rep >= a.warmup:
                    t_blk.append((t1 - t0) * 1e3)
                    t_fall.append((t3 - t2) * 1e3)
                    if frac == 0.0:
                        t_plain.append((t5 - t4) * 1e3)
                        t_own.append((t7 - t6) * 1e3)
                        t_emp.append((t9 - t8) * 1e3)
            leg = {"fraction": frac, "entries_with_targets": len(targets), "targets_named": len(named),
                   "block_ms": stats(t_blk), "fallback_ms": stats(t_fall), "table_build_ms": round(table_ms, 4),
                   "pass_runs": int(launches[0]), "step_launches": int(launches[1]), "kernel_launches": int(launches[2]),
                   "verdicts": [v_new.count(k) for k in (0, 1, 2)]}
            if frac == 0.0:
                leg["plain_admit_block_base_ms"] = stats(t_plain)
                leg["plain_admit_block_ms"] = stats(t_own)
                leg["empty_lists_64_ids_ms"] = stats(t_emp)
                p = leg["plain_admit_block_base_ms"]
                leg["inside_plain_p10_p90"] = bool(p["p10"] <= leg["block_ms"]["median"] <= p["p90"])
            entry["legs"].append(leg)
            print(json.dumps({"entries": n, **leg}), flush=True)
        out["sizes"].append(entry)
        new.close()
        base.close()
        del dev
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
