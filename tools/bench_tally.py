#!/usr/bin/env python
"""Time the tally add (ske_tally_add_packed_async) and its readers on the GPU.

One add of 2^25 packed 9-byte keys with a mask (85 % set), per population and
per variant of the kernel, each variant a context of its own (ske_open reads
SKE_TALLY_FORM / SKE_TALLY_LDS_LOG2): form 0 (a hash table in each workgroup's
LDS, flushed at the end) with 2^12, 2^11 and 2^10 LDS slots, and form 1 (one
insert-or-add in memory per item).  Three populations: one key; Zipf(1.1) over
5000 keys; uniform over 2^20 keys.  Beside them, on the same key bytes in the
same session, the Count-Min masked packed add (2000 x 7 table) and the time
profile add of as many epochs.  Everything takes turns, round by round, so
drift hits all alike; after the timing every variant's listing must equal the
numpy group-by times the number of adds.

Then the readers over the tallies the adds left (5000 and 2^20 entries):
``tally_top(3)`` and ``tally_list`` against listing everything and ordering it
with numpy on the host.

    python tools/bench_tally.py [--n 33554432] [--rounds 5] [--reps 2] [--out profiles/NAME.json]
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

MONDAY = 1742169600  # 2025-03-17T00:00:00 UTC
TABLE = (2000, 7)
VARIANTS = {"form0_lds12": ("0", "12"), "form0_lds11": ("0", "11"), "form0_lds10": ("0", "10"),
            "form1": ("1", "12")}
POPULATIONS = {"one_key": 1, "zipf1.1_5000": 5000, "uniform_2^20": 1 << 20}


def keys9(v: np.ndarray) -> np.ndarray:
    """b"L%08d" of every value: [n, 9] uint8"""
    out = np.empty((v.size, 9), np.uint8)
    out[:, 0] = ord("L")
    x = v.astype(np.uint32)
    for j in range(8, 0, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def draw(pop: str, n: int, rng) -> np.ndarray:
    k = POPULATIONS[pop]
    if k == 1:
        return np.zeros(n, np.int64)
    if pop.startswith("zipf"):
        p = 1.0 / np.arange(1, k + 1) ** 1.1
        return rng.choice(k, n, p=p / p.sum())
    return rng.integers(0, k, n)


def timed(fn, sync, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer, SketchEngine

    engines = {}
    for name, (form, lds) in VARIANTS.items():
        os.environ["SKE_TALLY_FORM"], os.environ["SKE_TALLY_LDS_LOG2"] = form, lds
        engines[name] = SketchEngine(0)
    os.environ.pop("SKE_TALLY_FORM", None)
    os.environ.pop("SKE_TALLY_LDS_LOG2", None)
    main_eng = engines["form0_lds12"]

    rng = np.random.default_rng(2025)
    n = args.n
    mask = (rng.random(n) < 0.85).astype(np.uint8)
    d_mask = DeviceBuffer(main_eng.ctx, n + 16)
    d_mask.from_host(mask)
    d_epoch = DeviceBuffer(main_eng.ctx, n * 8)
    d_epoch.from_host((MONDAY + rng.integers(0, 7 * 86400, n)).astype(np.int64))
    batch = DeviceBatch(main_eng.ctx, n, 9)
    batch.width = 0  # the packed form: bytes + offsets
    batch.offs.from_host((np.arange(n + 1, dtype=np.uint64) * 9).astype(np.uint32))
    main_eng.cms_init(0, *TABLE)
    main_eng.tp_init(0)
    results, readers = [], []
    for pi, pop in enumerate(POPULATIONS):
        which = draw(pop, n, rng)
        batch.bytes.from_host(keys9(which))
        log2 = 22 if POPULATIONS[pop] > 5000 else 14
        calls = {}
        for name, eng in engines.items():
            eng.tally_init(pi, log2)
            calls[name] = (eng, lambda e=eng: e.tally_add(pi, batch, mask=d_mask))
        calls["cms_add_packed"] = (main_eng, lambda: main_eng.cms_add(0, batch, mask=d_mask, want=1))
        calls["tp_add"] = (main_eng, lambda: main_eng.tp_add(0, d_epoch, n, mask=d_mask, want=1, late_from=86400))
        for eng, fn in calls.values():  # warm up
            fn()
            eng.sync()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for what, (eng, fn) in calls.items():
                times[what].append(timed(fn, eng.sync, args.reps))
        adds = 1 + args.rounds * args.reps
        ev = np.bincount(which, minlength=POPULATIONS[pop]) * adds
        va = np.bincount(which[mask == 1], minlength=POPULATIONS[pop]) * adds
        want = sorted((bytes(k), int(e), int(v)) for k, e, v in zip(keys9(np.arange(POPULATIONS[pop])), ev, va) if e)
        exact = True
        for name, eng in engines.items():
            keys, ge_, gv, complete = eng.tally_list(pi)
            exact &= complete and sorted(zip(keys, ge_.tolist(), gv.tolist())) == want
        row = {"n": n, "population": pop, "keys": len(want), "adds": adds, "counts_exact": bool(exact)}
        for f, t in times.items():
            row[f] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                      "ms_max": round(max(t), 4)}
        results.append(row)
        print(json.dumps(row), flush=True)
        if POPULATIONS[pop] > 1:  # the readers, over what the adds left
            r = {"entries": len(want)}
            for what, fn in (("tally_top3", lambda: main_eng.tally_top(pi, 3)),
                             ("tally_list", lambda: main_eng.tally_list(pi))):
                fn()
                t = [timed(fn, lambda: None, 1) for _ in range(5)]
                r[what] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4)}
            keys, ge_, gv, _ = main_eng.tally_list(pi)
            karr = np.asarray(keys)
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                order = np.lexsort((karr, ~ge_))
                t.append((time.perf_counter() - t0) * 1e3)
            assert [keys[i] for i in order[:3]] == main_eng.tally_top(pi, 3)[0][0]
            r["numpy_lexsort_of_the_listing"] = {"ms_median": round(statistics.median(t), 4),
                                                 "ms_min": round(min(t), 4)}
            readers.append(r)
            print(json.dumps(r), flush=True)
        for eng in engines.values():
            eng.tally_free(pi)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "tally_add", "timing": "host clock around reps enqueued calls + one stream "
                       "synchronise, per call; median over rounds; the variants (a context each), the Count-Min "
                       f"masked packed add ({TABLE[0]} x {TABLE[1]}) and the time-profile add alternating; readers: "
                       "host clock around one synchronous call, best and median of five",
                       "results": results, "readers": readers}, f, indent=1)
            f.write("\n")
    if not all(r["counts_exact"] for r in results):
        sys.exit("a variant's listing is not the restated group-by")


if __name__ == "__main__":
    main()
