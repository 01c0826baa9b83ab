#!/usr/bin/env python
"""Time the row log's group-by on the GPU, on bench_rows.py's data set: 2^25
rows resident in a log, one in ten a redelivery of an earlier row, 5000
lectures drawn from a Zipf law.  The reference's five queries
(attendance_analysis.py:65-118) -- the late rows by student, the rows by
weekday (the profile), by lecture, every row by student, the invalid rows by
student -- each as one synchronous call, outputs on the device; beside them the
whole-log select (outputs on the device), the front end they share.

The host route over the same log, in the same run: ``rows_select`` of the whole
log to the host, then numpy ``unique(return_counts=True)`` per query.  Every
device answer is checked against it.

    python tools/bench_rows_group.py [--n 33554432] [--rounds 5] [--out profiles/NAME.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd import _lib
    from rtsas_amd.engine import DeviceBuffer, SketchEngine, rows_select

    eng = SketchEngine(0)
    ctx, n = eng.ctx, args.n
    log2 = max(8, (n - 1).bit_length())
    rng = np.random.default_rng(2025)
    row = np.arange(n, dtype=np.int64)
    again = np.nonzero(rng.random(n) < 0.1)[0]
    again = again[again > 0]
    row[again] = (rng.random(again.size) * again).astype(np.int64)
    row = row[row]
    rank = (np.minimum(rng.zipf(1.2, n), LECTURES) - 1)[row]
    sid = 10_000_000 + (row * 7919) % 80_000_000
    ep = (MONDAY + row % (7 * 86400)).astype(np.int64)

    bufs = []

    def dev(arr):
        a = np.ascontiguousarray(arr)
        bufs.append(DeviceBuffer(ctx, a.nbytes + 64))
        bufs[-1].from_host(a)
        return C.c_void_p(bufs[-1].ptr)

    eng.rows_init(0, log2)
    ctx.call("ske_rows_append_fixed_async", 0, dev(digits(rank, 8, b"L")),
             dev((np.arange(n + 1, dtype=np.uint64) * 9).astype(np.uint32)), dev(sid.astype("<i8")), 8, dev(ep),
             dev((row % 3 != 0).astype(np.uint8)), None, n)
    eng.sync()
    for b in bufs:
        b.free()
    del row, rank, sid, ep

    def timed(call):
        call()  # warm up: the context scratch, the code objects
        ms = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 4), round(min(ms), 4)

    # the yardstick: the whole-log select, outputs on the device
    out = [DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64),
           DeviceBuffer(ctx, n + 64)]
    n_out, complete = C.c_uint64(), C.c_int()
    med, low = timed(lambda: ctx.call("ske_rows_select", 0, None, 0, I64_MIN, I64_MAX,
                                      *[C.c_void_p(b.ptr) for b in out], n, C.byref(n_out), C.byref(complete), 1))
    results = [{"bench": "select", "what": "whole_log", "n": n, "rows_out": int(n_out.value), "ms_median": med,
                "ms_min": low}]
    print(json.dumps(results[-1]), flush=True)
    for b in out[2:]:
        b.free()
    d_key, d_count = out[0], out[1]

    # the host route: the collapsed table to the host once, numpy per query
    t0 = time.perf_counter()
    cols, k, _ = rows_select(ctx, 0, None, I64_MIN, I64_MAX)
    select_host_ms = (time.perf_counter() - t0) * 1e3
    lec, epoch, ids, valid = (c[:k] for c in cols)
    sod = epoch % 86400
    queries = {
        "late_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_VALID_ANY, LATE, lambda: ids[sod >= LATE]),
        "by_lecture": (_lib.SKE_ROWS_BY_LECTURE, _lib.SKE_ROWS_VALID_ANY, 0, lambda: lec),
        "every_row_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_VALID_ANY, 0, lambda: ids),
        "invalid_by_student": (_lib.SKE_ROWS_BY_STUDENT, _lib.SKE_ROWS_INVALID_ONLY, 0, lambda: ids[valid == 0]),
    }
    exact = True
    for name, (by, vf, sod_from, host_col) in queries.items():
        st = _lib.RowsGroupStats()
        med, low = timed(lambda: ctx.call("ske_rows_group", 0, by, None, 0, I64_MIN, I64_MAX, vf, sod_from,
                                          C.c_void_p(d_key.ptr), C.c_void_p(d_count.ptr), n, C.byref(n_out),
                                          C.byref(st), C.byref(complete), 1))
        t0 = time.perf_counter()
        keys, counts = np.unique(host_col(), return_counts=True)
        host_ms = (time.perf_counter() - t0) * 1e3
        g = int(n_out.value)
        got_k, got_c = d_key.to_host(np.uint64, g), d_count.to_host(np.uint64, g)
        s = np.sort(counts)
        ok = (g == keys.size and np.array_equal(got_k.view(keys.dtype), keys) and np.array_equal(got_c, counts)
              and int(st.rows) == k and int(st.sum) == int(counts.sum())
              and int(st.sumsq) == int((counts.astype(object) ** 2).sum())
              and (int(st.med_lo), int(st.med_hi)) == (int(s[(g - 1) // 2]), int(s[g // 2]))
              and (int(st.min), int(st.max)) == (int(s[0]), int(s[-1])))
        exact &= ok
        results.append({"bench": "group", "what": name, "n": n, "rows": k, "groups": g, "answers_exact": ok,
                        "ms_median": med, "ms_min": low,
                        "host_select_then_unique": {"unique_ms": round(host_ms, 1),
                                                    "rows_select_to_host_ms": round(select_host_ms, 1)}})
        print(json.dumps(results[-1]), flush=True)

    bins, rows = np.zeros(168, np.uint64), C.c_uint64()
    med, low = timed(lambda: ctx.call("ske_rows_profile", 0, None, 0, I64_MIN, I64_MAX, _lib.SKE_ROWS_VALID_ANY, 0,
                                      bins.ctypes.data_as(C.c_void_p), C.byref(rows), C.byref(complete)))
    t0 = time.perf_counter()
    want = np.bincount(((epoch // 86400 + 3) % 7) * 24 + sod // 3600, minlength=168)
    host_ms = (time.perf_counter() - t0) * 1e3
    ok = np.array_equal(bins, want.astype(np.uint64)) and int(rows.value) == k
    exact &= ok
    results.append({"bench": "profile", "what": "by_weekday_and_hour", "n": n, "rows": k, "answers_exact": ok,
                    "ms_median": med, "ms_min": low,
                    "host_select_then_bincount": {"bincount_ms": round(host_ms, 1),
                                                  "rows_select_to_host_ms": round(select_host_ms, 1)}})
    print(json.dumps(results[-1]), flush=True)
    eng.rows_free(0)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "rows_group", "timing": "host clock around one synchronous call, median over rounds "
                       "after one warm-up call; group and select outputs on the device, the profile's 168 bins to "
                       "the host; host route: rows_select of the whole log to host arrays once (its time beside "
                       "every query), then numpy per query", "results": results}, f, indent=1)
            f.write("\n")
    if not exact:
        sys.exit("a group-by's answer is not the host's")


if __name__ == "__main__":
    main()
