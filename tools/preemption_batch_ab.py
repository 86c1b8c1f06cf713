"""The preemption search of a cycle, four ways, on one C3 snapshot (131,072
nodes): P preemptors drawn from the bench's workload mix, each with 16
candidates from a shared pool of admitted workloads.  Three warm-ups, ten timed
repeats per variant, the variants alternating; median and p10 / p90 of the
host wall time of the call(s), which end in a device synchronise.

Variants:
 1. per-preemptor: kueue_tas_host_preemption_search once per preemptor (JSON
    in and out, overlays merged on the host) — the parent commit's way;
 2. batch-host: kueue_tas_host_preemption_search_batch with host_overlays;
 3. batch-device: the same call, removal sets expanded on the device, the sets
    above abi.REMOVAL_SET_CAP records built there as large sets;
 4. batch-device-small-only: the same with large_sets=False — sets above
    abi.REMOVAL_SET_CAP records take the host path, the routing before large
    sets: the A/B leg of (3), in the same job on the same box.
All must agree on firstFit and the targets.  The stats blocks of (2)-(4) and
the device layer's large-set stats of (3) are recorded; one extra point at
--extra preemptors (default 512) shows cycle scale for (2)-(4).  Conditions
checked at every point: no set of (3) on the host path, and its upload within
16 bytes per table record + 4 per list entry + 64 per set.

usage: python tools/preemption_batch_ab.py [--out profiles/preemption_batch.json] [--config C3]
       [--preemptors 64] [--candidates 16] [--pool 256] [--extra 512] [--repeats 10] [--warmup 3]
       [--only batch-device: that variant alone, for a kernel trace]
       [--lib PATH --shape 2,2,4,8: a rehearsal on another build at a small size]"""
import argparse
import ctypes
import json
import random
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from kueue_oss_amd import TASFlavorSnapshot, abi, native, synth  # noqa: E402


def stats(ms):
    s = sorted(ms)
    q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
    return {"median": round(q(0.5), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4)}


def overlay_records(candidates, pool_deltas):
    """A lower bound of what the host path merges and uploads per call: the
    records of every prefix's overlay (the fillBack steps' come on top)."""
    return int(sum(sum(len(pool_deltas[t]) for t in cs[: i + 1]) for cs in candidates for i in range(len(cs))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--config", default="C3")
    ap.add_argument("--preemptors", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--pool", type=int, default=256)
    ap.add_argument("--extra", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["per-preemptor", "batch-host", "batch-device", "batch-device-small-only"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--shape", default=None)
    a = ap.parse_args()
    gen = synth.CONFIGS[a.config]
    kw = {"shape": tuple(int(x) for x in a.shape.split(","))} if a.shape else {}
    n_pre = max(a.preemptors, a.extra)
    doc, wls = gen(n_workloads=n_pre, **kw)
    _, pool_wls = gen(seed=4242, n_workloads=a.pool, **kw)
    lib = native.load_library(a.lib) if a.lib else None
    snap = TASFlavorSnapshot(doc, lib=lib) if lib is not None else TASFlavorSnapshot(doc)
    abi.bind_device_layer(snap._lib)  # (kueue_tas_removal_large_stats)
    # the pool: admitted workloads, their usage in the snapshot
    snap.compile(pool_wls)
    snap.run_compiled()
    res = snap.last_results()
    adm, _ = snap.admit(snap.last_assignments())
    pool = [synth.usage_records(pool_wls[i], res[i]) for i, ok in adm.tolist() if ok]
    snap.compile(wls)
    pool_deltas = [snap.usage_deltas(u) for u in pool]
    out = {"config": a.config, "pool": len(pool), "candidates": a.candidates, "repeats": a.repeats, "warmup": a.warmup,
           "points": []}
    for P in sorted({a.preemptors, a.extra} if a.extra else {a.preemptors}):
        rng = random.Random(1000 + P)
        ids = list(range(P))
        cands = [rng.sample(range(len(pool)), min(a.candidates, len(pool))) for _ in ids]
        variants = ["batch-host", "batch-device", "batch-device-small-only"]
        if P == a.preemptors:
            variants.insert(0, "per-preemptor")
        if a.only:
            variants = [a.only]
        times = {v: [] for v in variants}
        answers, blocks, large = {}, {}, None
        for rep in range(a.warmup + a.repeats):
            for v in variants:
                t0 = time.perf_counter()
                if v == "per-preemptor":
                    rs = [snap.preemption_search(wls[p], [pool[t] for t in cands[p]]) for p in ids]
                    ans = ([r["firstFit"] for r in rs],
                           {p: [cands[p][q] for q in r["targets"]] for p, r in zip(ids, rs) if r["firstFit"] >= 0})
                else:
                    r = snap.preemption_search_batch(ids, pool_deltas, cands, host_overlays=(v == "batch-host"),
                                                     large_sets=(v != "batch-device-small-only"))
                    ans = (r["firstFit"].tolist(), r["targets"])
                    blocks[v] = r["stats"]
                t1 = time.perf_counter()
                if v == "batch-device":  # (outside the timed window)
                    lg = (ctypes.c_int64 * 4)()
                    snap._lib.kueue_tas_removal_large_stats(snap.device_ctx(), lg)
                    large = dict(zip(("largeSets", "largeTableRecords", "mergeLaunches", "expandWorkgroups"),
                                     (int(x) for x in lg)))
                answers[v] = ans
                if rep >= a.warmup:
                    times[v].append((t1 - t0) * 1e3)
            first = answers[variants[0]]
            assert all(answers[v] == first for v in variants), "the variants disagree"
        ff = np.array(answers[variants[0]][0])
        table_records = int(sum(len(d) for d in pool_deltas))
        if "batch-device" in blocks:  # the conditions (derivable from the input, so they are asserted)
            st = blocks["batch-device"]
            assert st["hostSets"] == 0 and st["deviceSets"] == P, st
            assert st["removalBytesUploaded"] <= 16 * table_records + 4 * sum(len(cs) for cs in cands) + 64 * P, st
        point = {"preemptors": P, "ms": {v: stats(times[v]) for v in variants}, "stats": blocks, "large_stats": large,
                 "table_records": table_records,
                 "prefix_overlay_records": overlay_records(cands, pool_deltas),
                 "with_fit": int((ff >= 0).sum()), "max_first_fit": int(ff.max()) if ff.size else -1}
        out["points"].append(point)
        print(json.dumps(point), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    snap.close()


if __name__ == "__main__":
    main()
