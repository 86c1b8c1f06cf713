"""sharding.verify_replicas: every rank's resident snapshot against rank 0's.

Gloo world 2 on the emulated build (tests/emu), in the style of
test_distributed.py: the same document and two admit_rounds leave the
replicas equal; a request on rank 0 alone that names an extra resource adds
columns there, which is no mismatch (the components are matched by name, the
extra ones listed under "onlyOn"); one extra delta on rank 1 is named by rank,
component and leaf, identically on every rank.  On the GPU a one-rank nccl
group runs the same call (all_gather_object over nccl)."""
import copy
import os
import socket

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from kueue_oss_amd import sharding, synth

HERE = os.path.dirname(os.path.abspath(__file__))
EXTRA = "example.com/only-rank0"


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, lib_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kueue_oss_amd import TASFlavorSnapshot, native
        from kueue_oss_amd.native import DELTA_DTYPE

        lib = native.load_library(lib_path)
        doc, wls = synth.config_c2(n_workloads=24, shape=(2, 2, 8, 16))
        snap = TASFlavorSnapshot(doc, lib=lib)
        snap.compile(wls)
        snap.set_shard(sharding.shard_ids(wls, world, rank))
        out = {}
        admitted = 0
        for _ in range(2):
            snap.run_compiled()
            _, adm, deltas = sharding.admit_round(snap, world, rank, dist)
            admitted += len(deltas)
        out["deltas"] = admitted
        out["same"] = sharding.verify_replicas(snap, dist)
        if rank == 0:  # a request naming a resource no column holds: new columns on this rank only
            ps = copy.deepcopy(wls[0])
            ps[0]["requests"] = dict(ps[0]["requests"], **{EXTRA: 1})
            snap.find_topology_assignments_for_flavor(ps)
        out["only"] = sharding.verify_replicas(snap, dist)
        d = snap.snapshot_digest()
        out["resources"] = list(d["usage"])
        leaf = d["leaves"] - 3
        if rank == 1:  # one delta the other replica never saw
            snap.apply_deltas(np.array([(leaf, list(d["usage"]).index("memory"), 12345)], dtype=DELTA_DTYPE))
        out["diverged"] = sharding.verify_replicas(snap, dist)
        out["leaf"] = leaf
        if rank == 1:
            snap.apply_deltas(np.array([(leaf, list(d["usage"]).index("memory"), -12345)], dtype=DELTA_DTYPE))
        out["healed"] = sharding.verify_replicas(snap, dist)
        out["mirror"] = snap.verify_device()
        snap.close()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_gloo_verify_replicas(emu_lib):
    lib_path = os.path.join(HERE, "emu", "_build", "libkueue_tas_emu.so")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, lib_path)) for r in range(2)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = outs[0], outs[1]
    assert a["deltas"] == b["deltas"] > 0  # the rounds admitted something: the replicas' usage moved
    for key in ("same", "only", "diverged", "healed"):
        assert a[key] == b[key], key  # the same report on every rank
    assert a["same"] == {"ok": True, "ranks": {}, "leaves": [], "onlyOn": {}}
    # rank 0 holds columns rank 1 lacks, numbered in name order: the shared names still agree
    assert EXTRA in a["resources"] and EXTRA not in b["resources"]
    assert a["resources"].index("memory") != b["resources"].index("memory")
    assert a["only"] == {"ok": True, "ranks": {}, "leaves": [],
                         "onlyOn": {f"free:{EXTRA}": [0], f"usage:{EXTRA}": [0]}}
    d = a["diverged"]
    assert d["ok"] is False and d["ranks"] == {1: ["usage:memory"]}
    assert d["leaves"] == [{"rank": 1, "leaf": a["leaf"], "fields": ["usage:memory"]}]
    assert d["onlyOn"] == a["only"]["onlyOn"]
    assert a["healed"] == a["only"]
    assert a["mirror"]["ok"] and b["mirror"]["ok"]


_NCCL_VERIFY = r"""
import os, sys
import numpy as np
import torch
import torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from kueue_oss_amd import TASFlavorSnapshot, sharding, synth

os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
doc, wls = synth.config_c2(n_workloads=64, shape=(2, 4, 8, 16))
snap = TASFlavorSnapshot(doc)
snap.compile(wls)
snap.run_compiled()
_, adm, deltas = sharding.admit_round(snap, 1, 0, dist, "cuda:0")
assert len(deltas) > 0
r = sharding.verify_replicas(snap, dist)
assert r == {"ok": True, "ranks": {}, "leaves": [], "onlyOn": {}}, r
v = snap.verify_device()
assert v["ok"], v
snap.close()
dist.destroy_process_group()
print("verify ok")
"""


@pytest.mark.gpu
def test_verify_replicas_on_rccl():
    """verify_replicas in a one-rank nccl group on the GPU (a child process:
    its own process group), after an admit_round from the device block."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, "-c", _NCCL_VERIFY, os.path.dirname(HERE), str(_free_port())],
                       capture_output=True, text=True, timeout=240,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert r.returncode == 0 and "verify ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
