"""ShardedCounts' exact insights on the device across processes: W ranks (gloo
transport, all on this box's GPU) each keep the rows of the lectures they own
in a row log; the five exact entries, the per-student statistics and the
lecture rankings rank 0 gets from the collective calls equal those of one
context fed every swipe, made here in the test process.  RCCL replaces gloo on
a multi-GPU node; the device path (the group-bys, the merge) is the same."""
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
    import sharded_exact_worker as w
    client = pkg.SketchClient(decode_responses=True, device=0)
    counts = w.run_share(pkg, client, None, 0)
    want = w.answers(counts)
    want["rows"] = counts.records_info()["used"]
    yield want
    client.flushall()


@pytest.mark.parametrize("world,backend", [(2, "gloo"), (4, "gloo"), (1, "nccl")])
def test_sharded_exact_insights_equal_one_context(one_context, tmp_path, world, backend):
    """backend nccl: RCCL, one rank on the box's one GPU with the collectives
    forced on (a second RCCL rank on the same GPU is refused)."""
    import sharded_exact_worker as w
    out = str(tmp_path / "res.pkl")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", WORKER_BACKEND=backend,
               WORKER_FORCE_COLLECTIVES="1" if backend == "nccl" else "0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                        f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
                        "--master-port", str(29740 + world + (10 if backend == "nccl" else 0)),
                        os.path.join(ROOT, "tests", "sharded_exact_worker.py"),
                        out], env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    with open(out, "rb") as f:
        got = pickle.load(f)
    want = one_context
    assert [i["title"] for i in got["insights"]] == [
        "Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings", "Most Consistent Attendees",
        "Invalid Attendance Attempts"]
    # every lecture's rows lay on one rank, every log is complete
    assert all(i["split_lectures"] == 0 and i["complete"] is True for i in got["insights"])
    strip = [{k: v for k, v in i.items() if k != "split_lectures"} for i in got["insights"]]
    assert strip == want["insights"]
    assert all(len(i["data"]) > 0 for i in want["insights"])
    assert got["processor"] == got["insights"]
    for which in w.WHICH:
        g, o = got["counts"][which], want["counts"][which]
        assert g["stats"] == o["stats"], which  # rows, n, sum, sumsq, min, max, the median ranks
        assert g["keys"].dtype == np.int64 and np.array_equal(g["keys"], o["keys"])
        assert np.array_equal(g["counts"], o["counts"]) and g["complete"] is True and g["split_lectures"] == 0
    assert got["rankings"] == dict(want["rankings"], split_lectures=0) and got["rankings"]["complete"] is True
    assert got["by_day"] == want["by_day"]
    # the log held redeliveries, and rank 0 really kept only its share
    assert want["rows"] > want["counts"]["attended"]["stats"]["rows"]
    assert (got["local_rows"] == want["rows"]) == (world == 1)
