"""Worker of tests/test_sharded_exact_gpu.py: one rank of a run whose swipes are
sharded by lecture (rank = distributed.owner(lecture, world)).  Launched by
torch.distributed.run; every rank uses the one GPU.  The rank preloads its
Bloom replica, feeds its share of the swipes -- a part of them delivered twice
-- through a StudentCounts that keeps a row log, and calls the collective
ShardedCounts.exact_insights(), exact_counts() and exact_lecture_rankings();
rank 0 writes what it got.

usage: python -m torch.distributed.run --nproc-per-node W tests/sharded_exact_worker.py OUT.pkl
"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, BATCHES = 3000, 3
OPTS = dict(records="table", records_capacity_log2=13, lecture_counts="lectures", lecture_capacity_log2=10,
            error=0.002, probability=0.01)
WHICH = ("attended", "late", "invalid")


def workload():
    rng = np.random.default_rng(78)
    roster = rng.choice(np.arange(10 ** 7, 10 ** 8), 500, replace=False)
    sids = np.where(rng.random(N) < 0.85, roster[np.minimum(rng.zipf(1.3, N) - 1, 499)],
                    rng.integers(10 ** 7, 10 ** 8, N))
    ids = np.frombuffer("".join(str(int(s)) for s in sids).encode(), np.uint8).reshape(N, 8).copy()
    lectures = ["CS%03d" % l for l in np.minimum(rng.zipf(1.4, N) - 1, 59)]
    days = rng.integers(17, 24, N)
    t0 = int(np.datetime64("2025-03-17T00:00:00").astype("datetime64[s]").astype(np.int64))
    times = t0 + (days - 17) * 86400 + rng.integers(6 * 3600, 14 * 3600, N)
    keys = ["hll:unique:%s:2025-03-%02d" % (l, d) for l, d in zip(lectures, days)]
    return roster, ids, lectures, times, keys


def run_share(pkg, client, dest, rank):
    """This rank's StudentCounts after its share of every batch (dest None:
    all), then of the redelivery: every fifth swipe of the run once more."""
    roster, ids, lectures, times, keys = workload()
    client.execute_command("BF.RESERVE", "bf:students", 0.001, 5000)
    client.bf_madd_packed("bf:students", *pkg.pack_ints(roster))  # replicated preload
    counts = pkg.StudentCounts(client, **OPTS)
    per = N // BATCHES
    for rows in [np.arange(b * per, (b + 1) * per) for b in range(BATCHES)] + [np.arange(0, N, 5)]:
        if dest is not None:
            rows = rows[dest[rows] == rank]
        if rows.size:
            slots = np.asarray([client.key_slot(keys[i]) for i in rows], np.uint32)
            counts.update("bf:students", slots, ids[rows], times[rows], [lectures[i] for i in rows])
    return counts


def answers(sc):
    """what the test compares"""
    return {"insights": sc.exact_insights(), "counts": {w: sc.exact_counts(w) for w in WHICH},
            "rankings": sc.exact_lecture_rankings(4), "by_day": sc.exact_by_day()}


def main():
    import torch
    import torch.distributed as dist
    out = sys.argv[1]
    pkg = ge.load_package()
    from rtsas_amd.distributed import ShardedCounts, route
    torch.cuda.set_device(0)
    if os.environ.get("WORKER_BACKEND", "gloo") == "nccl":
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    client = pkg.SketchClient(decode_responses=True, device=0)
    lectures = workload()[2]
    counts = run_share(pkg, client, route(lectures, world), rank)
    sc = ShardedCounts(counts, rank, world)
    if os.environ.get("WORKER_FORCE_COLLECTIVES") == "1":
        sc.transport.solo = False  # world 1: the collectives are still called
    res = answers(sc)
    res["local_rows"] = counts.records_info()["used"]
    res["processor"] = pkg.AttendanceProcessor(client, counts=sc).insights(exact=True)
    if rank == 0:
        with open(out, "wb") as f:
            pickle.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
