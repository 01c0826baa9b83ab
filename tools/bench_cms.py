#!/usr/bin/env python
"""Time the Count-Min Sketch bulk add (ske_cms_add_fixed_async) on the GPU.

One masked add of 2^25 eight-digit ids (the form StudentCounts.update
enqueues behind K1), per table and id distribution, in both bulk forms: the
LDS form (what the table size selects) and the global form (a second context
opened with SKE_CMS_LDS_CELLS=0).  The two contexts take turns, round by
round, so drift hits both alike; after the timing the two tables must be
identical.

    python tools/bench_cms.py [--n 33554432] [--rounds 7] [--reps 10] [--out profiles/NAME.json]

The input floor is 9 bytes per swipe (8 id bytes + 1 mask byte) at 8 TB/s.
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
TABLES = [(2000, 7), (200, 10), (4864, 8)]  # 0.001/0.01, 0.01/0.001, the largest LDS-form table


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
    for form, cells in (("lds", None), ("global", "0")):
        if cells is None:
            os.environ.pop("SKE_CMS_LDS_CELLS", None)
        else:
            os.environ["SKE_CMS_LDS_CELLS"] = cells
        engines[form] = SketchEngine(0)  # ske_open reads the variable
    os.environ.pop("SKE_CMS_LDS_CELLS", None)

    rng = np.random.default_rng(2025)
    n = args.n
    floor_ms = n * 9 / HBM_BYTES_PER_S * 1e3
    mask = (rng.random(n) < 0.85).astype(np.uint8)
    results = []
    for dist in ("uniform", "zipf10"):
        ids = make_ids(n, dist, rng)
        dev = {}
        for form, eng in engines.items():
            b = DeviceBatch(eng.ctx, n, 8)
            b.bytes.from_host(ids)
            m = DeviceBuffer(eng.ctx, n + 16)
            m.from_host(mask)
            dev[form] = (b, m)
        for ti, (width, depth) in enumerate(TABLES):
            cid = ti + (0 if dist == "uniform" else len(TABLES))
            times = {f: [] for f in engines}
            for form, eng in engines.items():
                eng.cms_init(cid, width, depth)
                for _ in range(3):
                    eng.cms_add(cid, dev[form][0], mask=dev[form][1], want=1)
                eng.sync()
            for _ in range(args.rounds):
                for form, eng in engines.items():
                    b, m = dev[form]
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        eng.cms_add(cid, b, mask=m, want=1)
                    eng.sync()
                    times[form].append((time.perf_counter() - t0) / args.reps * 1e3)
            tabs = {f: e.cms_table(cid) for f, e in engines.items()}
            same = bool(np.array_equal(tabs["lds"][0], tabs["global"][0]) and tabs["lds"][1] == tabs["global"][1])
            adds = 3 + args.rounds * args.reps
            row = {"n": n, "dist": dist, "width": width, "depth": depth, "adds": adds,
                   "count": int(tabs["lds"][1]), "count_expected": adds * int(mask.sum()),
                   "tables_identical": same, "floor_ms": round(floor_ms, 4)}
            for f in engines:
                med = statistics.median(times[f])
                row[f] = {"ms_median": round(med, 4), "ms_min": round(min(times[f]), 4),
                          "ms_max": round(max(times[f]), 4), "floor_fraction": round(floor_ms / med, 4)}
            results.append(row)
            print(json.dumps(row), flush=True)
        for b, m in dev.values():
            b.free()
            m.free()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "cms_masked_add", "timing": "host clock around reps enqueued adds + one "
                       "stream synchronise, per add; median over rounds, the two forms alternating",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["tables_identical"] and r["count"] == r["count_expected"] for r in results):
        sys.exit("the two forms disagree")


if __name__ == "__main__":
    main()
