#!/usr/bin/env python
"""Time the seen-row set on the GPU: the three folds that build the row keys
(lecture, id, epoch) plus ske_seen_add_async, over 2^25 rows resident on the
device, for three populations: all rows distinct; 10 % of the rows redelivered
(copies of earlier rows of the batch); a single row.  Per population the set is
emptied, the batch is timed once into the empty set ("fresh": every distinct row
claims a slot) and then on top of itself ("again": every row is a repeat, the
mean of --reps calls), round by round.  The answers are checked: FIRST as
often as there are distinct rows, then never.

Beside it, in the same run, the host alternative over the same 16-byte keys:
``np.unique`` of the keys the device folded, brought back once.

    python tools/bench_seen.py [--n 33554432] [--rounds 5] [--reps 3] [--capacity-log2 27] [--out profiles/NAME.json]
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
import __graft_entry__ as ge  # noqa: E402

MONDAY = 1742169600  # 2025-03-17T00:00:00 UTC
POPULATIONS = ("all_distinct", "10pct_redelivered", "single_row")


def digits(v: np.ndarray, width: int, lead: bytes = b"") -> np.ndarray:
    """``lead`` + the zero-padded decimal of every value: [n, len(lead) + width] uint8"""
    out = np.empty((v.size, len(lead) + width), np.uint8)
    out[:, :len(lead)] = np.frombuffer(lead, np.uint8)
    x = v.astype(np.uint64)
    for j in range(len(lead) + width - 1, len(lead) - 1, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def rows_of(pop: str, n: int, rng) -> np.ndarray:
    """the row number of every item: equal numbers are one row"""
    if pop == "single_row":
        return np.zeros(n, np.int64)
    row = np.arange(n, dtype=np.int64)
    if pop == "10pct_redelivered":
        again = np.nonzero(rng.random(n) < 0.1)[0]
        again = again[again > 0]
        row[again] = (rng.random(again.size) * again).astype(np.int64)  # an earlier item's row
        row = row[row]  # a copy of a copy is the original's row
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--capacity-log2", type=int, default=27)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd.engine import DeviceBuffer, SketchEngine

    eng = SketchEngine(0)
    ctx, n = eng.ctx, args.n
    rng = np.random.default_rng(2025)
    d_lec, d_id = DeviceBuffer(ctx, n * 9 + 64), DeviceBuffer(ctx, n * 8 + 64)
    d_ep, d_keys, d_out = DeviceBuffer(ctx, n * 8 + 16), DeviceBuffer(ctx, n * 16), DeviceBuffer(ctx, n + 16)
    eng.seen_init(0, args.capacity_log2)

    def fold_and_add():
        keys = C.c_void_p(d_keys.ptr)
        ctx.call("ske_seen_fold_fixed_async", keys, C.c_void_p(d_lec.ptr), 9, n, 1)
        ctx.call("ske_seen_fold_fixed_async", keys, C.c_void_p(d_id.ptr), 8, n, 0)
        ctx.call("ske_seen_fold_epoch_async", keys, C.c_void_p(d_ep.ptr), 1, n, 0)
        eng.seen_add(0, d_keys, n, d_out)

    def timed(reps=1):
        t0 = time.perf_counter()
        for _ in range(reps):
            fold_and_add()
        eng.sync()
        return (time.perf_counter() - t0) / reps * 1e3

    results = []
    for pop in POPULATIONS:
        row = rows_of(pop, n, rng)
        d_lec.from_host(digits(row % 5000, 8, b"L"))
        d_id.from_host(digits(10_000_000 + row // 5000 % 80_000_000, 8))
        d_ep.from_host((MONDAY + row % (7 * 86400)).astype(np.int64))
        eng.seen_reset(0)
        fold_and_add()  # warm up: the context scratch, the code objects
        eng.sync()
        fresh, again = [], []
        first_fresh = first_again = None
        for _ in range(args.rounds):
            # the device is kept busy right up to each timed window (an add, then the reset's
            # memsets; an add on top): a window that opens on an idle device measures its wake-up
            fold_and_add()
            eng.seen_reset(0)
            fresh.append(timed())
            first_fresh = int((d_out.to_host(np.uint8, n) == 0).sum())
            fold_and_add()
            again.append(timed(args.reps))
            first_again = int((d_out.to_host(np.uint8, n) == 0).sum())
        info = eng.seen_info(0)
        keys = d_keys.to_host(np.uint64, 2 * n).view([("k0", "<u8"), ("k1", "<u8")])
        t0 = time.perf_counter()
        distinct = int(np.unique(keys).size)
        host_ms = (time.perf_counter() - t0) * 1e3
        r = {"n": n, "population": pop, "distinct_rows": distinct, "capacity_log2": args.capacity_log2,
             "answers_exact": first_fresh == distinct and first_again == 0 and info["unplaced"] == 0
             and info["used"] == distinct,
             "fold3_add_fresh": {"ms_median": round(statistics.median(fresh), 4), "ms_min": round(min(fresh), 4)},
             "fold3_add_again": {"ms_median": round(statistics.median(again), 4), "ms_min": round(min(again), 4)},
             "host_np_unique_of_the_keys": {"ms": round(host_ms, 1)}}
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.seen_free(0)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "seen_add", "timing": "host clock around the three fold calls and the add, enqueued, "
                       "and one stream synchronise; median over rounds; the set emptied before every fresh add (not "
                       "timed); again: the mean of reps calls behind an untimed one; host: one np.unique over the n "
                       "16-byte keys",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["answers_exact"] for r in results):
        sys.exit("the set's answers are not the distinct rows'")


if __name__ == "__main__":
    main()
