"""bench.py's plain run, `--full` and `--dump-outputs`: a plain run carries the
headline figures and none of the legs that take runs of their own; the dumped
arrays are float32 / float64, small, consistent with each other and equal to
the CPU oracle's answers and registers over the same batches."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "stream_1b", "rollup", "host_fed", "check", "cpu_baseline", "secondary")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_full_and_dump_are_off_by_default():
    b = _bench()
    a = b.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = b.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"
    # two sampled float32 arrays, their float64 indices and the float64 key sums
    assert b.DUMP_ELEMS * (4 + 8 + 4 + 8 + 8) <= 64 << 20


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, pkg, orc):
    """C2 (1M swipes per step, the persistent LDS K1), 2 timed steps after 1
    warm-up step: the line, then the dumped answers of step 2 and the
    registers after all 3 steps against the oracle over the same batches."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "c2",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["full"] is False
    assert line["unit"] == "swipes/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
    n = line["config"]["swipes_per_step"]
    assert np.isclose(line["value"], n / (line["ms_per_step"] * 1e-3), rtol=1e-9)
    assert not [k for k in FULL_ONLY if k in line]

    arrs = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrs) == {"answers", "answers_valid", "registers", "registers_key_sums"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    keys = line["config"]["hll_keys_this_gpu"]
    assert arrs["answers"].shape == (n,) and arrs["registers"].shape == (keys * 16384,)
    assert arrs["answers_valid"][0] == arrs["answers"].sum()
    assert np.array_equal(arrs["registers_key_sums"], arrs["registers"].reshape(keys, 16384).sum(1))

    # the oracle over the same three batches (the generator is counter-based)
    from rtsas_amd import synthetic
    from rtsas_amd.engine import SketchEngine
    w = synthetic.WORKLOADS["c2"]
    assert synthetic.key_probs(w) is None and keys == w.n_keys  # uniform keys: no table, slot = key
    eng = SketchEngine(0)
    p = eng.gen_params(w)
    mb = eng.members_batch(p, 0, w.n_members)
    buf, offs, _ = mb.to_host()
    chain = orc.Chain(w.bf_capacity, w.bf_error)
    chain.madd_packed(buf, offs)
    regs = np.zeros((keys, 16384), np.uint8)
    for j in range(3):
        sb = eng.swipe_batch(p, j * n, n)
        buf, offs, slot = sb.to_host()
        want, _, _ = orc.process_swipes(chain, regs, slot.astype(np.uint32), buf, offs)
        sb.free()
    mb.free()
    assert np.array_equal(arrs["answers"], want.astype(np.float32))
    assert np.array_equal(arrs["registers"], regs.reshape(-1).astype(np.float32))
