#!/usr/bin/env python
"""Time the time-profile add (ske_tp_add_async) on the GPU.

One add of 2^25 swipe times, per input and in both forms of the kernel: the
aggregated form (the default: a wavefront whose tile falls into one bin adds
it with one LDS atomic) and the plain form (one LDS atomic per lane, always; a
second context opened with SKE_TP_FORM=1).  Three inputs: every swipe in one
(weekday, hour) bin, two adjacent hours of one day mixed, uniform over all 168
bins; each with the bare call (epochs only) and with a mask (85 % set) and the
late output.  Beside
them, the Count-Min masked add of the same n eight-digit ids on the 2000 x 7
table (tools/bench_cms.py's uniform row), the call StudentCounts.update already
enqueues two or three times.  Everything takes turns, round by round, so drift
hits all alike; after the timing both forms' counters must equal the numpy
histogram times the number of adds.

    python tools/bench_tp.py [--n 33554432] [--rounds 7] [--reps 10] [--out profiles/NAME.json]

The input floor is 8 bytes per swipe for the bare call and 10 (8 + a mask byte
+ a late byte) for the full one, at 8 TB/s.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

HBM_BYTES_PER_S = 8e12
MONDAY = 1742169600  # 2025-03-17T00:00:00 UTC
TABLE = (2000, 7)
FORMS = {"aggregated": "0", "plain": "1"}


def digits8(v: np.ndarray) -> np.ndarray:
    out = np.empty((v.size, 8), np.uint8)
    x = v.astype(np.uint32)
    for j in range(7, -1, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def make_times(n: int, kind: str, rng) -> np.ndarray:
    if kind == "one_bin":
        return MONDAY + 2 * 86400 + 9 * 3600 + rng.integers(0, 3600, n)
    if kind == "two_hours":
        return MONDAY + 2 * 86400 + 8 * 3600 + rng.integers(0, 7200, n)
    return MONDAY + rng.integers(0, 7 * 86400, n)


def histogram(epoch: np.ndarray, take=None) -> np.ndarray:
    day, sod = epoch // 86400, epoch % 86400
    bins = ((day + 3) % 7) * 24 + sod // 3600
    return np.bincount(bins if take is None else bins[take], minlength=168).astype(np.uint64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer, SketchEngine

    engines = {}
    for form, v in FORMS.items():
        os.environ["SKE_TP_FORM"] = v
        engines[form] = SketchEngine(0)  # ske_open reads the variable
    os.environ.pop("SKE_TP_FORM", None)

    rng = np.random.default_rng(2025)
    n = args.n
    mask = (rng.random(n) < 0.85).astype(np.uint8)
    main_eng = engines["aggregated"]
    ids = DeviceBatch(main_eng.ctx, n, 8)
    ids.bytes.from_host(digits8(rng.integers(10_000_000, 100_000_000, n, dtype=np.int64)))
    dev = {}
    for form, eng in engines.items():
        m = DeviceBuffer(eng.ctx, n + 16)
        m.from_host(mask)
        dev[form] = (DeviceBuffer(eng.ctx, n * 8), m, DeviceBuffer(eng.ctx, n + 16))
    main_eng.cms_init(0, *TABLE)
    results = []
    for ki, kind in enumerate(("one_bin", "two_hours", "uniform_168")):
        epoch = make_times(n, kind, rng).astype(np.int64)
        for form, eng in engines.items():
            dev[form][0].from_host(epoch)
        for full in (False, True):
            tid = 2 * ki + int(full)

            def tp(form):
                d_e, d_m, d_l = dev[form]
                engines[form].tp_add(tid, d_e, n, mask=d_m if full else None, want=1, late_from=32400,
                                     late=d_l if full else None)

            def cms():
                main_eng.cms_add(0, ids, mask=dev["aggregated"][1], want=1)

            calls = {"aggregated": (engines["aggregated"], lambda: tp("aggregated")),
                     "plain": (engines["plain"], lambda: tp("plain")), "cms_add": (main_eng, cms)}
            for eng in engines.values():
                eng.tp_init(tid)
            for eng, fn in calls.values():  # warm up
                for _ in range(3):
                    fn()
                eng.sync()
            times = {k: [] for k in calls}
            for _ in range(args.rounds):
                for what, (eng, fn) in calls.items():
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn()
                    eng.sync()
                    times[what].append((time.perf_counter() - t0) / args.reps * 1e3)
            adds = 3 + args.rounds * args.reps
            want = histogram(epoch, mask == 1 if full else None) * np.uint64(adds)
            got = {f: e.tp_counts(tid).reshape(-1) for f, e in engines.items()}
            late_ok = True
            if full:
                want_late = (epoch % 86400 >= 32400).astype(np.uint8)
                late_ok = all(np.array_equal(dev[f][2].to_host(np.uint8, n), want_late) for f in engines)
            floor_ms = n * (10 if full else 8) / HBM_BYTES_PER_S * 1e3
            row = {"n": n, "input": kind, "mask_and_late": full, "adds": adds, "bins_hit": int(np.count_nonzero(want)),
                   "counters_exact": bool(all(np.array_equal(g, want) for g in got.values())), "late_exact": late_ok,
                   "floor_ms": round(floor_ms, 4)}
            for f, t in times.items():
                med = statistics.median(t)
                row[f] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4)}
            for f in engines:
                row[f]["floor_fraction"] = round(floor_ms / row[f]["ms_median"], 4)
                row[f]["ratio_to_cms_add"] = round(row[f]["ms_median"] / row["cms_add"]["ms_median"], 3)
            results.append(row)
            print(json.dumps(row), flush=True)
            for eng in engines.values():
                eng.tp_free(tid)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "tp_add", "timing": "host clock around reps enqueued calls + one stream synchronise, "
                       "per call; median over rounds; the two forms (two contexts) and the Count-Min masked add "
                       f"({TABLE[0]} x {TABLE[1]}, uniform eight-digit ids, 85 % of the mask set) alternating",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["counters_exact"] and r["late_exact"] for r in results):
        sys.exit("a form's counters or late bytes are not the restated ones")


if __name__ == "__main__":
    main()
