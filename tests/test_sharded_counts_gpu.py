"""ShardedCounts on the device across processes: W ranks (gloo transport, all on
this box's GPU) each count the swipes routed to them; the insights, rankings,
profile and merged Count-Min tables rank 0 gets from the collective
ShardedCounts.insights() equal those of one context fed the whole workload,
made here in the test process.  RCCL replaces gloo on a multi-GPU node; the
device path (exports, merges) is the same."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def one_context(pkg):
    """the whole workload through one context, once for every launch"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sharded_counts_worker as w
    client = pkg.SketchClient(decode_responses=True, device=0)
    counts = w.run_share(pkg, client, None, 0)
    want = w.answers(counts, client, (counts.attended_key, counts.invalid_key, counts.late_key))
    yield want
    client.flushall()


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (4, "gloo"), (1, "nccl")])
def test_sharded_insights_equal_one_context(one_context, tmp_path, world, backend):
    """backend nccl: RCCL, one rank on the box's one GPU with the collectives
    forced on (all_gather / all_reduce on their RCCL code path; a second RCCL
    rank on the same GPU is refused)."""
    import sharded_counts_worker as w
    out = str(tmp_path / "res.pkl")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WORKER_BACKEND=backend,
               WORKER_FORCE_COLLECTIVES="1" if backend == "nccl" else "0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29700 + world + (10 if backend == "nccl" else 0)),
                        os.path.join(ROOT, "tests", "sharded_counts_worker.py"),
                        out], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out, "rb") as f:
        got = pickle.load(f)
    want = one_context
    assert got["insights"] == want["insights"]
    assert [i["title"] for i in got["insights"][0]] == [
        "Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings", "Most Consistent Attendees",
        "Invalid Attendance Attempts"]
    assert all(i.get("complete", True) for q in got["insights"] for i in q)
    assert got["rankings"] == want["rankings"] and got["rankings"]["complete"]
    assert np.array_equal(got["hours"], want["hours"]) and int(got["hours"].sum()) == w.N
    for (t, c), (wt, wc) in zip(got["tables"], want["tables"]):
        assert np.array_equal(t, wt) and c == wc
    assert got["population"] == want["population"]
    # rank 0 really counted only its share
    assert (got["local_swipes"] == w.N) == (world == 1)
