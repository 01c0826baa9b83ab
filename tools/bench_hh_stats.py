#!/usr/bin/env python
"""Time ske_hh_stats against the listing route on the GPU.

Two sets at half load over the 2000 x 7 table (CMS.INITBYPROB 0.001 0.01):
2^16 slots, the StudentCounts default, and 2^24 slots, the largest -- 2^15 and
2^23 distinct eight-digit ids, every one counted once and a quarter of them a
second time, all tracked at threshold 1.  Over the same set and table, taking
turns round by round so drift hits both alike:

    stats   ske_hh_stats at threshold 1: the struct is all that crosses
    list    what a caller does for the same answer without it: ske_hh_list at
            the same threshold into arrays allocated once, then np.median and
            np.std(ddof=1) of the returned estimates

and, to see what bounds the new call, two more forms of it in the same rounds:

    depth1  the same set against a 2000 x 1 table: one hash per member, not 7
    nopass  threshold above the maximum: the estimate pass reads and hashes
            everything, nothing is compacted, the select's rounds find n == 0

    python tools/bench_hh_stats.py [--log2 16 24] [--rounds 7] [--out profiles/NAME.json]

Timing: the host clock around the synchronous calls, median of the rounds.
The two routes' answers are compared: n, sum, sum of squares, the extremes and
the median must be identical.
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

TABLE = (2000, 7)  # CMS.INITBYPROB 0.001 0.01
HBM_BYTES_PER_S = 8e12
CHUNK = 1 << 22


def digits8(v: np.ndarray) -> np.ndarray:
    out = np.empty((v.size, 8), np.uint8)
    x = v.astype(np.uint32)
    for j in range(7, -1, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def distinct_ids(m: int) -> np.ndarray:
    """m distinct eight-digit ids: 7919 is coprime to the 9 * 10^7 of them"""
    return digits8(10_000_000 + (np.arange(m, dtype=np.int64) * 7919) % 90_000_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[16, 24])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd import _lib
    from rtsas_amd.client_hh import derive_stats
    from rtsas_amd.engine import DeviceBatch, SketchEngine, hh_stats

    eng = SketchEngine(0)
    ctx = eng.ctx
    width, depth = TABLE
    results = []
    for k, log2 in enumerate(args.log2):
        m = 1 << (log2 - 1)
        cid, cid1, hid = 2 * k, 2 * k + 1, k
        eng.cms_init(cid, width, depth)
        eng.cms_init(cid1, width, 1)
        eng.hh_init(hid, log2)
        ids = distinct_ids(m)
        for at in range(0, m, CHUNK):  # every id once, every fourth twice; then all join
            part = ids[at:at + CHUNK]
            batches = []
            for sel in (part, part[::4]):
                b = DeviceBatch(ctx, len(sel), 8)
                b.bytes.from_host(np.ascontiguousarray(sel))
                for c in (cid, cid1):
                    eng.cms_add(c, b)
                batches.append(b)
            eng.hh_track(hid, cid, batches[0], 1)
            eng.sync()
            for b in batches:
                b.free()
        del ids
        info = eng.hh_info(hid)
        out_ids = np.zeros((m, _lib.SKE_HH_ID_BYTES), np.uint8)
        out_len, out_est = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
        n_out, done = C.c_uint64(0), C.c_int(1)

        def listing():
            ctx.call("ske_hh_list", hid, cid, 1, out_ids.ctypes.data_as(C.c_void_p),
                     out_len.ctypes.data_as(C.c_void_p), out_est.ctypes.data_as(C.c_void_p), m, C.byref(n_out),
                     C.byref(done))
            est = out_est[:int(n_out.value)]
            return est, float(np.median(est)), float(np.std(est, ddof=1))

        est, med, std = listing()
        top = int(est.max())
        forms = {"stats": lambda: hh_stats(ctx, hid, cid, 1), "list": listing,
                 "depth1": lambda: hh_stats(ctx, hid, cid1, 1), "nopass": lambda: hh_stats(ctx, hid, cid, top + 1)}
        for fn in forms.values():  # warm: scratch sized, code loaded
            fn()
        times = {f: [] for f in forms}
        for r in range(args.rounds):
            for f, fn in forms.items():
                t0 = time.perf_counter()
                fn()
                times[f].append((time.perf_counter() - t0) * 1e3)
            print(f"# log2 {log2} round {r}: " + " ".join(f"{f} {times[f][-1]:.3f}" for f in forms), flush=True)
        raw = hh_stats(ctx, hid, cid, 1)
        s = derive_stats(raw)
        ints = est.astype(np.uint64)
        assert top < 1 << 20  # so numpy's u64 sums below are exact: 2^23 squares of 40 bits
        same = bool(s["n"] == len(ints) and s["sum"] == int(ints.sum()) and s["sumsq"] == int((ints * ints).sum())
                    and (s["min"], s["max"]) == (int(ints.min()), top) and s["median"] == med
                    and abs(s["std"] - std) <= 1e-9 * std)
        row = {"capacity_log2": log2, "members": info["used"], "members_expected": m, "width": width, "depth": depth,
               "complete": bool(raw["complete"]) and info["overflow"] == 0, "routes_agree": same,
               "n": s["n"], "min": s["min"], "max": s["max"], "median": s["median"], "mean": round(s["mean"], 6),
               "std": round(s["std"], 6),
               "read_floor_ms": round((1 << log2) * 28 / HBM_BYTES_PER_S * 1e3, 5),
               "list_bytes_to_host": 24 * s["n"], "stats_bytes_to_host": 112}
        for f, t in times.items():
            row[f] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                      "ms_max": round(max(t), 4)}
        row["list_over_stats"] = round(row["list"]["ms_median"] / row["stats"]["ms_median"], 2)
        results.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "hh_stats_vs_listing", "timing": "host clock around each synchronous call; median over "
                       "rounds; ske_hh_stats, the listing route (ske_hh_list into arrays allocated once + np.median + "
                       "np.std(ddof=1)), ske_hh_stats against a depth-1 table and ske_hh_stats with no member passing, "
                       "alternating", "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["routes_agree"] and r["members"] == r["members_expected"] for r in results):
        sys.exit("the two routes disagree, or the set is not the expected one")


if __name__ == "__main__":
    main()
