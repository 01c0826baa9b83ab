#!/usr/bin/env python
"""Time the heavy-hitter track (ske_hh_track_fixed_async) on the GPU.

One masked track of 2^25 eight-digit ids on the 2000 x 7 table (the form
StudentCounts.update enqueues behind the two adds), uniform ids and one id at
10 %, in both forms: the table copied into LDS by every workgroup, and read
from memory (two contexts, SKE_HH_LDS_CELLS set for each).  The Count-Min
masked add over the same buffers (tools/bench_cms.py's measurement, into a
table of its own so the tracked table stays as it is) runs in the same rounds
as the yardstick.  The three take turns, round by round, so drift hits all
alike; afterwards the two forms' sets must be identical.

    python tools/bench_hh.py [--n 33554432] [--rounds 7] [--reps 10] [--out profiles/NAME.json]

The track threshold is twice the table's noise (n * 0.85 / width per cell), so
no uniform id passes and the hot id does: the insert path runs for a tenth of
the batch and ends at its plain load.  The input floor is 9 bytes per swipe
(8 id bytes + 1 mask byte) at 8 TB/s.
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
TABLE = (2000, 7)  # CMS.INITBYPROB 0.001 0.01
LDS_CELLS = 152 * 1024 // 4


def digits8(v: np.ndarray) -> np.ndarray:
    out = np.empty((v.size, 8), np.uint8)
    x = v.astype(np.uint32)
    for j in range(7, -1, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def make_ids(n: int, dist: str, rng) -> np.ndarray:
    v = rng.integers(10_000_000, 100_000_000, n, dtype=np.int64)
    if dist == "zipf10":  # one id takes a tenth of the swipes
        v[rng.random(n) < 0.10] = 20251003
    return digits8(v)


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
    for form, cells in (("lds", LDS_CELLS), ("memory", 0)):
        os.environ["SKE_HH_LDS_CELLS"] = str(cells)
        engines[form] = SketchEngine(0)  # ske_open reads the variable
    os.environ.pop("SKE_HH_LDS_CELLS", None)

    rng = np.random.default_rng(2025)
    n = args.n
    width, depth = TABLE
    floor_ms = n * 9 / HBM_BYTES_PER_S * 1e3
    mask = (rng.random(n) < 0.85).astype(np.uint8)
    threshold = int(2 * n * 0.85 / width)
    results = []
    for di, dist in enumerate(("uniform", "zipf10")):
        ids = make_ids(n, dist, rng)
        cid, add_cid, hid = 2 * di, 2 * di + 1, di
        dev = {}
        for form, eng in engines.items():
            b = DeviceBatch(eng.ctx, n, 8)
            b.bytes.from_host(ids)
            m = DeviceBuffer(eng.ctx, n + 16)
            m.from_host(mask)
            dev[form] = (b, m)
            eng.cms_init(cid, width, depth)
            eng.cms_init(add_cid, width, depth)
            eng.hh_init(hid, 16)
            eng.cms_add(cid, b, mask=m, want=1)  # the batch's own add: the table the track reads
            for _ in range(3):
                eng.hh_track(hid, cid, b, threshold, mask=m, want=1)
                eng.cms_add(add_cid, b, mask=m, want=1)
            eng.sync()
        times = {"lds": [], "memory": [], "add": []}
        for _ in range(args.rounds):
            for what in times:
                eng = engines["lds" if what == "add" else what]
                b, m = dev["lds" if what == "add" else what]
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    if what == "add":
                        eng.cms_add(add_cid, b, mask=m, want=1)
                    else:
                        eng.hh_track(hid, cid, b, threshold, mask=m, want=1)
                eng.sync()
                times[what].append((time.perf_counter() - t0) / args.reps * 1e3)
        lists = {f: e.hh_list(hid, cid, threshold) for f, e in engines.items()}
        infos = {f: e.hh_info(hid) for f, e in engines.items()}
        same = bool(lists["lds"][0] == lists["memory"][0] and np.array_equal(lists["lds"][1], lists["memory"][1])
                    and infos["lds"] == infos["memory"])
        row = {"n": n, "dist": dist, "width": width, "depth": depth, "threshold": threshold,
               "members": infos["lds"]["used"], "complete": lists["lds"][2], "sets_identical": same,
               "members_expected": 0 if dist == "uniform" else 1, "floor_ms": round(floor_ms, 4)}
        for f, t in times.items():
            med = statistics.median(t)
            row[f] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                      "floor_fraction": round(floor_ms / med, 4)}
        for f in ("lds", "memory"):
            row[f]["ratio_to_add"] = round(row[f]["ms_median"] / row["add"]["ms_median"], 3)
        results.append(row)
        print(json.dumps(row), flush=True)
        for b, m in dev.values():
            b.free()
            m.free()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "hh_masked_track", "timing": "host clock around reps enqueued calls + one stream "
                       "synchronise, per call; median over rounds; the two track forms and the Count-Min masked "
                       "add (LDS form) alternating", "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["sets_identical"] and r["members"] == r["members_expected"] and r["complete"] for r in results):
        sys.exit("the two forms disagree, or the set is not the expected one")


if __name__ == "__main__":
    main()
