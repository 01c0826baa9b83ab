"""Worker of tests/test_sharded_counts_gpu.py: one rank of a run whose swipes
are routed by lecture-day key (distributed.route).  Launched by
torch.distributed.run; every rank uses the one GPU.  The rank preloads its
Bloom replica, runs its share of the swipes through StudentCounts.update (K1,
the Count-Min adds, the tracks, the profile and the tally) in the batch
sequence of the whole run, and calls the collective ShardedCounts.insights();
rank 0 writes what it got.

usage: python -m torch.distributed.run --nproc-per-node W tests/sharded_counts_worker.py OUT.pkl
"""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

N, BATCHES = 6000, 3
OPTS = dict(track_attended=1, track_invalid=1, capacity_log2=12, late_key="cms:late", track_late=1,
            day_profile="week", lecture_counts="lectures", lecture_capacity_log2=10, error=0.002, probability=0.01)
QUERIES = (dict(), dict(attended_threshold="reference", late_threshold="reference", lecture_k=4),
           dict(attended_threshold=4, invalid_threshold=2, late_threshold=3))


def workload():
    rng = np.random.default_rng(77)
    roster = rng.choice(np.arange(10 ** 7, 10 ** 8), 800, replace=False)
    sids = np.where(rng.random(N) < 0.85, roster[np.minimum(rng.zipf(1.3, N) - 1, 799)],
                    rng.integers(10 ** 7, 10 ** 8, N))
    ids = np.frombuffer("".join(str(int(s)) for s in sids).encode(), np.uint8).reshape(N, 8).copy()
    lectures = ["CS%03d" % l for l in np.minimum(rng.zipf(1.4, N) - 1, 79)]
    days = rng.integers(17, 24, N)
    t0 = int(np.datetime64("2025-03-17T00:00:00").astype("datetime64[s]").astype(np.int64))
    times = t0 + (days - 17) * 86400 + rng.integers(6 * 3600, 14 * 3600, N)
    keys = ["hll:unique:%s:2025-03-%02d" % (l, d) for l, d in zip(lectures, days)]
    return roster, ids, lectures, times, keys


def run_share(pkg, client, dest, rank):
    """This rank's StudentCounts after its share of every batch (dest None: all)."""
    roster, ids, lectures, times, keys = workload()
    client.execute_command("BF.RESERVE", "bf:students", 0.001, 5000)
    client.bf_madd_packed("bf:students", *pkg.pack_ints(roster))  # replicated preload
    counts = pkg.StudentCounts(client, **OPTS)
    per = N // BATCHES
    for b in range(BATCHES):
        rows = np.arange(b * per, (b + 1) * per)
        if dest is not None:
            rows = rows[dest[rows] == rank]
        if rows.size:
            slots = np.asarray([client.key_slot(keys[i]) for i in rows], np.uint32)
            counts.update("bf:students", slots, ids[rows], times[rows], [lectures[i] for i in rows])
    return counts


def answers(sc, client, keys):
    """what the test compares: the insights, then the queries and the tables"""
    out = {"insights": [sc.insights(**q) for q in QUERIES]}
    out["rankings"] = sc.lecture_rankings(5)
    out["hours"] = sc.by_hour_of_week()
    out["tables"] = [client.cms_table(k) for k in keys]
    out["population"] = sc.population("attended")
    return out


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
    keys = workload()[4]
    counts = run_share(pkg, client, route(keys, world), rank)
    sc = ShardedCounts(counts, rank, world)
    if os.environ.get("WORKER_FORCE_COLLECTIVES") == "1":
        sc.transport.solo = False  # world 1: the collectives are still called
    res = answers(sc, client, sc.ops.view_cms_keys())
    res["local_swipes"] = int(counts.by_hour_of_week().sum())
    if rank == 0:
        with open(out, "wb") as f:
            pickle.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
