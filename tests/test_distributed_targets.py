"""The multi-rank round with preemption targets on the CPU (gloo, world 2,
the emulated build; after tests/test_distributed.py): both ranks hold the
snapshot in the state of a test_admit_targets scenario, evaluate their shard
of the cycle's workloads, rank 0 admits the gathered entries with their
targets (sharding.admit_round(..., workloads=, targets=)) and broadcasts the
verdict-1 entries' deltas; both replicas then evaluate the whole list again
and must equal the oracle composition's `after`."""
import os
import socket

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import test_admit_targets as T
from kueue_oss_amd import sharding

HERE = os.path.dirname(os.path.abspath(__file__))
SCENARIO = (T.EMU_CASES[33], 33, T.EMU_SHAPE, False, ())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q, lib_path, ref, as_deltas):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from kueue_oss_amd import TASFlavorSnapshot, native

        lib = native.load_library(lib_path)
        # the replica in the state of the call (test_admit_targets._prepare), its shard of the cycle evaluated
        snap = TASFlavorSnapshot(ref["doc"], lib=lib)
        snap.compile(ref["pool_wls"])
        snap.run_compiled()
        snap.admit(snap.last_assignments())
        for t in ref["subset"]:
            snap.remove_usage(ref["pool"][t])
        snap.compile(ref["wls"])
        ids = sharding.shard_ids(ref["wls"], world, rank)
        snap.set_shard(ids)
        snap.run_compiled()
        out = {"ids": ids, "batch": snap.last_results()}
        for t in ref["subset"]:
            snap.add_usage(ref["pool"][t])
        workloads = targets = None
        if rank == 0:  # only the admitting rank holds the cycle's targets
            workloads = [snap.usage_deltas(u) for u in ref["pool"]] if as_deltas else ref["pool"]
            targets = ref["targets"]
        quads, pairs, deltas = sharding.admit_round(snap, world, rank, dist, workloads=workloads, targets=targets)
        out["pairs"] = pairs.tolist() if pairs is not None else None
        out["deltas"] = deltas.tolist()
        snap.set_shard(list(range(len(ref["wls"]))))
        snap.run_compiled()
        out["after"] = snap.last_results()
        snap.close()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("as_deltas", [False, True], ids=["usage", "deltas"])
def test_gloo_admit_round_with_targets(emu_lib, as_deltas):
    world = 2
    ref = T._reference(*SCENARIO)
    assert T._non_vacuous(ref)
    lib_path = os.path.join(HERE, "emu", "_build", "libkueue_tas_emu.so")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, lib_path, ref, as_deltas)) for r in range(world)]
    for p in procs:
        p.start()
    outs = dict(q.get(timeout=600) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    n = len(ref["wls"])
    assert sorted(i for r in range(world) for i in outs[r]["ids"]) == list(range(n))
    assert all(outs[r]["ids"] for r in range(world))  # both ranks evaluated a part
    batch = {i: rs for r in range(world) for i, rs in zip(outs[r]["ids"], outs[r]["batch"])}
    assert [batch[i] for i in range(n)] == ref["b2"]
    assert outs[1]["pairs"] is None
    assert [i for i, _ in outs[0]["pairs"]] == list(range(n))
    assert [v for _, v in outs[0]["pairs"]] == ref["verdicts"]  # verdict 2 included
    assert outs[0]["deltas"] == outs[1]["deltas"] and outs[0]["deltas"]
    for r in range(world):
        assert outs[r]["after"] == ref["after"]
