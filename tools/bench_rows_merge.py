#!/usr/bin/env python
"""Time the group merge on the GPU (``ske_rows_group_merge``), on
bench_rows.py's data set split by lecture: W in {2, 8} contexts in one process
each hold the rows of the lectures ``rank % W`` gives them (one row in ten a
redelivery of an earlier one, 5000 lectures drawn from a Zipf law; 2^24 rows by
default, half of the 2^25 the one-context benchmarks load, since W + 1 contexts
and the host route share the run).  Per query
-- the late rows, every row and the invalid rows by student, every row by
lecture -- each context's ``ske_rows_group`` leaves its groups on the device;
they are laid out as ``ShardedCounts`` lays the all-gather out (every rank's
keys padded to the largest rank rounded up to 4 entries, then every rank's
counts, pad counts 0), and the one ``ske_rows_group_merge`` call over that
buffer is timed with device events on the destination's stream, median of 5
warmed repeats, outputs on the device.

Beside it, on the host clock, what there was without the call: each context's
``rows_group`` to host arrays, then numpy (``concatenate``,
``unique(return_inverse)``, ``add.at``, ``median``, ``std``).  Every device
answer is checked against the numpy one.

One GPU, no collective running: this is the merge call's cost, not multi-GPU
scaling.

    python tools/bench_rows_merge.py [--n 16777216] [--rounds 5] [--out profiles/NAME.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
from bench_rows import LECTURES, MONDAY, digits  # noqa: E402

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
LATE = 9 * 3600


def ms(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def run_world(torch, world: int, cols, rounds: int) -> list:
    from rtsas_amd import _lib
    from rtsas_amd.engine import DeviceBuffer, SketchEngine, rows_group
    rank, sid, ep, valid = cols
    srcs = [SketchEngine(0) for _ in range(world)]
    dst = SketchEngine(0)
    stream = torch.cuda.Stream()
    dst.ctx.call("ske_set_stream", C.c_void_p(stream.cuda_stream))
    for r, eng in enumerate(srcs):
        mine = np.nonzero(rank % world == r)[0]
        n = int(mine.size)
        bufs = []

        def dev(arr):
            a = np.ascontiguousarray(arr)
            bufs.append(DeviceBuffer(eng.ctx, a.nbytes + 64))
            bufs[-1].from_host(a)
            return C.c_void_p(bufs[-1].ptr)

        eng.rows_init(0, max(8, (max(n, 2) - 1).bit_length()))
        if n:
            eng.ctx.call("ske_rows_append_fixed_async", 0, dev(digits(rank[mine], 8, b"L")),
                         dev((np.arange(n + 1, dtype=np.uint64) * 9).astype(np.uint32)), dev(sid[mine].astype("<i8")),
                         8, dev(ep[mine]), dev(valid[mine]), None, n)
        eng.sync()
        for b in bufs:
            b.free()

    queries = {
        "late_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_VALID_ANY, LATE),
        "every_row_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_VALID_ANY, 0),
        "invalid_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_INVALID_ONLY, 0),
        "by_lecture": (_lib.SKE_ROWS_BY_LECTURE, _lib.SKE_ROWS_VALID_ANY, 0),
    }
    out = []
    for name, (by, vf, sod) in queries.items():
        # the host route, timed: every context's groups to host arrays, then numpy
        t0 = time.perf_counter()
        parts = [rows_group(e.ctx, 0, by, None, I64_MIN, I64_MAX, vf, sod) for e in srcs]
        t1 = time.perf_counter()
        keys = np.concatenate([p[0] for p in parts]).view(np.int64 if by == _lib.SKE_ROWS_BY_STUDENT else np.uint64)
        counts = np.concatenate([p[1] for p in parts])
        uniq, inv = np.unique(keys, return_inverse=True)
        sums = np.zeros(uniq.size, np.uint64)
        np.add.at(sums, inv, counts)
        med, std = float(np.median(sums)), float(np.std(sums.astype(np.float64), ddof=1)) if sums.size > 1 else 0.0
        t2 = time.perf_counter()

        # the gathered buffer: keys of every rank, then counts of every rank, zero padded
        ns = [int(p[0].size) for p in parts]
        nmax = (max(ns) + 3) & ~3
        n_in = world * nmax
        flat = np.zeros(2 * n_in, np.uint64)
        for r, p in enumerate(parts):
            flat[r * nmax:r * nmax + ns[r]] = p[0]
            flat[n_in + r * nmax:n_in + r * nmax + ns[r]] = p[1]
        gathered = DeviceBuffer(dst.ctx, flat.nbytes + 64)
        gathered.from_host(flat)
        d_key, d_count = DeviceBuffer(dst.ctx, n_in * 8 + 64), DeviceBuffer(dst.ctx, n_in * 8 + 64)
        n_out, multi, st = C.c_uint64(), C.c_uint64(), _lib.RowsGroupStats()

        def call():
            dst.ctx.call("ske_rows_group_merge", by, C.c_void_p(gathered.ptr), C.c_void_p(gathered.ptr + n_in * 8),
                         n_in, C.c_void_p(d_key.ptr), C.c_void_p(d_count.ptr), n_in, C.byref(n_out), C.byref(st),
                         C.byref(multi), _lib.SKE_MEM_DEVICE)

        ts = []
        for i in range(rounds + 1):  # the first repeat warms up
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            if i:
                ts.append(a.elapsed_time(b))
        g = int(n_out.value)
        got_k, got_c = d_key.to_host(np.uint64, g), d_count.to_host(np.uint64, g)
        s = np.sort(sums)
        ok = (g == uniq.size and np.array_equal(got_k.view(uniq.dtype), uniq) and np.array_equal(got_c, sums)
              and int(st.sum) == int(sums.sum())
              and int(st.sumsq) == int((sums * sums).sum(dtype=np.uint64))  # the total is below 2^32: no wrap
              and (int(st.med_lo), int(st.med_hi)) == (int(s[(g - 1) // 2]), int(s[g // 2]))
              and (int(st.med_lo) + int(st.med_hi)) / 2 == med
              and int(multi.value) == int((np.bincount(inv, minlength=uniq.size) > 1).sum()))
        row = {"bench": "rows_group_merge", "what": name, "world": world, "entries_in": n_in,
               "entries_per_rank_max": max(ns), "groups_out": g, "multi": int(multi.value), "answers_exact": bool(ok),
               "all_gather_bytes_received_per_rank": (world - 1) * 16 * nmax, "merge_call_device": ms(ts),
               "host_route": {"rows_group_to_host_all_ranks_ms": round((t1 - t0) * 1e3, 3),
                              "numpy_merge_ms": round((t2 - t1) * 1e3, 3), "std_of_sums": round(std, 3)}}
        print(json.dumps(row), flush=True)
        out.append(row)
        for b in (gathered, d_key, d_count):
            b.free()
    for e in srcs:
        e.rows_free(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worlds", default="2,8")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    ge.load_package()
    n = args.n
    rng = np.random.default_rng(2025)
    row = np.arange(n, dtype=np.int64)
    again = np.nonzero(rng.random(n) < 0.1)[0]
    again = again[again > 0]
    row[again] = (rng.random(again.size) * again).astype(np.int64)
    row = row[row]
    rank = (np.minimum(rng.zipf(1.2, n), LECTURES) - 1)[row]
    sid = 10_000_000 + (row * 7919) % 80_000_000
    ep = (MONDAY + row % (7 * 86400)).astype(np.int64)
    valid = (row % 3 != 0).astype(np.uint8)

    results = []
    for world in (int(w) for w in args.worlds.split(",")):
        results += run_world(torch, world, (rank, sid, ep, valid), args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "rows_group_merge", "n_rows": n, "measured_by": "builder",
                       "timing": "device events on the destination's stream around the one ske_rows_group_merge "
                       "call (inputs and outputs on the device), median over warmed repeats; host route on the host "
                       "clock: every context's rows_group to host arrays, then numpy concatenate / "
                       "unique(return_inverse) / add.at / median / std; one GPU, no collective running -- not "
                       "multi-GPU scaling", "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["answers_exact"] for r in results):
        sys.exit("a merge's answer is not numpy's")


if __name__ == "__main__":
    main()
