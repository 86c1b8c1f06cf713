"""kueue_tas_snapshot_digest on the C3 snapshot (131,072 leaves): device time
of warm calls, bracketed by HIP events on the context's stream
(kueue_tas_last_digest_ms), against the kernel's algorithmic bytes.

usage: python tools/probe_digest.py [--calls 20] [--warm 5] [--out profiles/snapshot_digest.json]
                                    [--bench NAME=FILE ...] [--emu]
  --bench: a file holding bench.py's JSON result line, recorded as context
           under "bench" (e.g. parent=..., this=...)
  --emu:   the CPU SIMT emulator build (tests/emu): checks the script, times nothing real
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from kueue_oss_amd import TASFlavorSnapshot, abi, native, synth  # noqa: E402


def _bench_line(path):
    best = None
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith("{") and "ms_per_step" in line:
                best = json.loads(line)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snapshot_digest.json"))
    ap.add_argument("--bench", action="append", default=[])
    ap.add_argument("--emu", action="store_true")
    ap.add_argument("--shape", default="4,16,64,32")
    a = ap.parse_args()
    lib = native.load_library(os.path.join(ROOT, "tests", "emu", "_build", "libkueue_tas_emu.so")) if a.emu \
        else native.load_library()
    abi.bind_device_layer(lib)
    doc, _ = synth.config_c3(n_workloads=8, shape=tuple(int(x) for x in a.shape.split(",")))
    snap = TASFlavorSnapshot(doc, lib=lib)
    d = snap.snapshot_digest()
    assert snap.verify_device()["ok"]
    ctx = snap.device_ctx()
    N, R, K = d["leaves"], len(d["free"]), len(d["labels"])
    tags = int(d["tags"], 16) != 0
    words = np.zeros(4 + 2 * R + K, dtype=np.uint64)
    chunks = np.zeros(max(len(d["chunks"]), 1), dtype=np.uint64)
    n, nc = ctypes.c_size_t(), ctypes.c_size_t()
    ms = (ctypes.c_float * 2)()
    kern, total, wall = [], [], []
    for i in range(a.warm + a.calls):
        t0 = time.perf_counter()
        rc = lib.kueue_tas_snapshot_digest(ctx, words.ctypes.data, words.size, ctypes.byref(n), chunks.ctypes.data,
                                           chunks.size, ctypes.byref(nc))
        t1 = time.perf_counter()
        assert rc == 0, lib.kueue_tas_last_error(ctx)
        lib.kueue_tas_last_digest_ms(ctx, ms)
        if i >= a.warm:
            kern.append(ms[0] * 1e3)
            total.append(ms[1] * 1e3)
            wall.append((t1 - t0) * 1e6)
    assert ["%016x" % int(w) for w in chunks[: nc.value]] == d["chunks"]
    snap.close()
    # N (16 R + 8 + 4 + 4 K + 1 [+ 8 tags]): both capacity columns, the two presence words, the profile,
    # the label columns, the dead map, the tags
    nbytes = N * (16 * R + 8 + 4 + 4 * K + 1 + (8 if tags else 0))

    def stats(v):
        return {"median_us": round(float(np.median(v)), 2), "p10_us": round(float(np.percentile(v, 10)), 2),
                "p90_us": round(float(np.percentile(v, 90)), 2)}

    out = {"config": "C3", "leaves": N, "resource_columns": R, "label_columns": K, "leaf_tags": tags,
           "calls": a.calls, "warm_calls": a.warm, "chunks": int(nc.value),
           "launches_per_call": 2, "d2h_per_call": 1,
           "kernels": stats(kern), "kernels_and_d2h": stats(total), "host_wall": stats(wall),
           "algorithmic_bytes": nbytes,
           "gb_per_s": round(nbytes / (float(np.median(kern)) * 1e-6) / 1e9, 1) if not a.emu else None,
           "bench": {}}
    for spec in a.bench:
        name, path = spec.split("=", 1)
        line = _bench_line(path)
        if line:
            out["bench"][name] = {k: line[k] for k in ("ms_per_step", "value", "config") if k in line}
    print(json.dumps(out, indent=1))
    if not a.emu:
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
