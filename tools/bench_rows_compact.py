#!/usr/bin/env python
"""Time the row log's compaction on the GPU, on bench_rows.py's data set: 2^25
rows resident in a log, one in ten a redelivery of an earlier row, 5000 lectures
drawn from a Zipf law, the epochs spread over one week.  One synchronous
``ske_rows_compact`` of the whole log -- with nothing expired, and with the
cutoff in the middle of the week -- each round on a freshly loaded log.

Beside it, in the same run: the whole-log select with outputs on the device (the
front end the compaction shares); the host route to the same end (``rows_read``,
numpy, ``rows_reset``, ``ske_rows_append`` from host arrays, ids as text again);
and the whole-log group-by by student before and after, which is what the
compaction buys the readers.  Every answer is checked against the host's.

    python tools/bench_rows_compact.py [--n 33554432] [--rounds 5] [--out profiles/NAME.json]
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


def host_survivors(cols):
    """rows_read's columns -> the positions of each (lec, epoch, id) run's last-appended row, ascending"""
    lec, ep, ids, _ = cols
    order = np.lexsort((ids, ep, lec))  # stable: equal keys stay in position order
    a, b = order[:-1], order[1:]
    last = np.ones(order.size, bool)
    last[:-1] = (lec[a] != lec[b]) | (ep[a] != ep[b]) | (ids[a] != ids[b])
    return np.sort(order[last])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd import _lib
    from rtsas_amd.client_rows import lecture_digest
    from rtsas_amd.engine import DeviceBuffer, SketchEngine, rows_compact, rows_info, rows_read

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

    batch = (dev(digits(rank, 8, b"L")), dev((np.arange(n + 1, dtype=np.uint64) * 9).astype(np.uint32)),
             dev(sid.astype("<i8")), 8, dev(ep), dev((row % 3 != 0).astype(np.uint8)), None, n)
    del row, rank, sid, ep
    eng.rows_init(0, log2)

    def reload():
        eng.rows_reset(0)
        ctx.call("ske_rows_append_fixed_async", 0, *batch)
        eng.sync()

    reload()
    results, exact = [], True

    # the yardstick: the whole-log select, outputs on the device
    out = [DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64),
           DeviceBuffer(ctx, n + 64)]
    outp = [C.c_void_p(b.ptr) for b in out]
    n_out, complete = C.c_uint64(), C.c_int()

    def timed(call, rounds=args.rounds):
        call()  # warm up: the context scratch, the code objects
        ms = []
        for _ in range(rounds):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 4), round(min(ms), 4)

    def select():
        ctx.call("ske_rows_select", 0, None, 0, I64_MIN, I64_MAX, *outp, n, C.byref(n_out), C.byref(complete), 1)

    def group():
        st = _lib.RowsGroupStats()
        ctx.call("ske_rows_group", 0, _lib.SKE_ROWS_BY_STUDENT, None, 0, I64_MIN, I64_MAX, _lib.SKE_ROWS_VALID_ANY, 0,
                 outp[0], outp[1], n, C.byref(n_out), C.byref(st), C.byref(complete), 1)

    def group_answer():
        g = int(n_out.value)
        return out[0].to_host(np.uint64, g), out[1].to_host(np.uint64, g)

    med, low = timed(select)
    results.append({"bench": "select", "what": "whole_log_before", "n": n, "rows_out": int(n_out.value),
                    "ms_median": med, "ms_min": low})
    print(json.dumps(results[-1]), flush=True)
    med, low = timed(group)
    before_groups = group_answer()
    results.append({"bench": "group", "what": "every_row_by_student_before", "used": n, "groups": int(n_out.value),
                    "ms_median": med, "ms_min": low})
    print(json.dumps(results[-1]), flush=True)

    # the host's answer, from the log as rows_read brings it back
    t0 = time.perf_counter()
    cols = rows_read(ctx, 0, 0, n)
    read_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    keep_all = host_survivors(cols)
    numpy_ms = (time.perf_counter() - t0) * 1e3

    # the compaction: each round on a freshly loaded log
    mid = MONDAY + 7 * 43200
    for what, keep_since in (("nothing_expired", I64_MIN), ("cutoff_mid_week", mid)):
        keep = keep_all[cols[1][keep_all] >= keep_since]
        expired = int((cols[1] < keep_since).sum())
        want = dict(before=n, kept=int(keep.size), superseded=n - expired - int(keep.size), expired=expired)
        rows_compact(ctx, 0, keep_since)  # warm up: the context scratch, the code objects
        ms = []
        for _ in range(args.rounds):
            reload()
            t0 = time.perf_counter()
            got = rows_compact(ctx, 0, keep_since)
            ms.append((time.perf_counter() - t0) * 1e3)
            exact &= got == want
        info = rows_info(ctx, 0)
        back = rows_read(ctx, 0, 0, info["used"])
        ok = (got == want and all(np.array_equal(b, c[keep]) for b, c in zip(back, cols))
              and (info["used"], info["taken"], info["dropped"], info["overflow"]) == (keep.size, keep.size, 0, 0))
        exact &= ok
        results.append({"bench": "compact", "what": what, **got, "answers_exact": bool(ok),
                        "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                        "rows_per_s_median": round(n / statistics.median(ms) * 1e3)})
        print(json.dumps(results[-1]), flush=True)
        if keep_since == I64_MIN:  # the readers over the compacted log
            med, low = timed(select)
            results.append({"bench": "select", "what": "whole_log_after", "used": info["used"],
                            "rows_out": int(n_out.value), "ms_median": med, "ms_min": low})
            print(json.dumps(results[-1]), flush=True)
            med, low = timed(group)
            after_groups = group_answer()
            keys, counts = np.unique(cols[2][keep], return_counts=True)
            ok = (all(np.array_equal(a, b) for a, b in zip(before_groups, after_groups))
                  and np.array_equal(after_groups[0].view(np.int64), keys) and np.array_equal(after_groups[1], counts))
            exact &= ok
            results.append({"bench": "group", "what": "every_row_by_student_after", "used": info["used"],
                            "groups": int(n_out.value), "answers_exact": bool(ok), "ms_median": med, "ms_min": low})
            print(json.dumps(results[-1]), flush=True)

    # the host route to the same end, once: the log over the bus twice, the ids as text again.  The log
    # holds digests; the names a host would take from the lecture tally's listing come from the data set here.
    names = digits(np.arange(LECTURES), 8, b"L")
    dig = np.asarray([lecture_digest(x.tobytes()) for x in names], np.uint64)
    by_digest = np.argsort(dig)
    reload()
    t0 = time.perf_counter()
    lec, epo, ids, valid = rows_read(ctx, 0, 0, n)
    keep = host_survivors((lec, epo, ids, valid))
    lec_txt = names[by_digest[np.searchsorted(dig[by_digest], lec[keep])]]
    id_txt = digits(ids[keep], 8)
    k = keep.size
    lec_offs = (np.arange(k + 1, dtype=np.uint64) * 9).astype(np.uint32)
    id_offs = (np.arange(k + 1, dtype=np.uint64) * 8).astype(np.uint32)
    e, v = np.ascontiguousarray(epo[keep]), np.ascontiguousarray(valid[keep])
    eng.rows_reset(0)
    ctx.call("ske_rows_append", 0, _lib.ptr(lec_txt.reshape(-1)), _lib.ptr(lec_offs), _lib.ptr(id_txt.reshape(-1)),
             _lib.ptr(id_offs), _lib.ptr(e), _lib.ptr(v), None, k, _lib.SKE_MEM_HOST)
    route_ms = (time.perf_counter() - t0) * 1e3
    back = rows_read(ctx, 0, 0, rows_info(ctx, 0)["used"])
    ok = all(np.array_equal(b, c[keep_all]) for b, c in zip(back, cols))
    exact &= ok
    results.append({"bench": "host_route", "what": "rows_read, numpy lexsort and last of run, rows_reset, rows_append",
                    "kept": int(k), "answers_exact": bool(ok), "ms": round(route_ms, 1),
                    "of_which": {"rows_read_ms": round(read_ms, 1), "numpy_survivors_ms": round(numpy_ms, 1)}})
    print(json.dumps(results[-1]), flush=True)

    eng.rows_free(0)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "rows_compact", "timing": "host clock around one synchronous call; compact: median "
                       "over rounds, each on a log emptied and loaded again just before (not timed), after one "
                       "warm-up call; select and group: median over rounds after one warm-up call, outputs on the "
                       "device; host route: once, its read and numpy parts as measured on the same log before",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not exact:
        sys.exit("a compaction's counts or log, or a group-by's answer, is not the host's")


if __name__ == "__main__":
    main()
