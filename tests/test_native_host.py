"""Exact probe arithmetic of the kernels (sketch_common.h), checked on the
host: fastmod vs %, incremental probe stepping vs (a + i*b) mod 2^64 mod bits
including 64-bit wraparound, and hllPatLen; and the segmented PFADD's arena
sizing (sketch_seg_plan.h) against a host model of what C1 and D do to the
counters: rows of r2 / o2, chunk-table columns, counted chunk slots, slot
numbers and the window pass's record range, over adversarial and random
bucket patterns."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_arith(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "host_arith.cpp")
    exe = str(tmp_path / "host_arith")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout


def test_seg_capacity(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "seg_capacity.cpp")
    exe = str(tmp_path / "seg_capacity")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
    # the four adversarial patterns still need the rows they were built for
    for line in ("rot nb1 512 sub 3538944: rows 1024 (old maxch 944,", "rot nb1 256 sub 1925120: rows 512 (old maxch 491,",
                 "rot nb1 64 sub 1032192: rows 192 (old maxch 190,", "uniform nb1 512 sub 3932160 seed 0: rows 10"):
        assert line in out.stdout, out.stdout
