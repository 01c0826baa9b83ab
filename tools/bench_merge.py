#!/usr/bin/env python
"""Time the device merge calls behind distributed.ShardedCounts on one GPU.

`world` contexts in one process stand for the ranks (world 2 and 8); a further
context is the destination.  Per context: a 2000 x 7 Count-Min table, a
heavy-hitter set of 2^16 and of 2^20 members (neighbouring contexts share half
of theirs) and a tally of 5000 keys.  The sources' exports are laid behind one
another in device memory, as an all-gather leaves them, and each merge call is
timed with device events around warmed repeats on the destination's stream:

  cms_sum     ske_cms_sum_dev over the `world` tables, one call
  hh_merge    ske_hh_merge_dev, one call per source, into an empty set
  tally_merge ske_tally_merge_dev, one call per source, into an empty tally

Beside each, on the host clock, what the library offered for the same job
before these calls: for Count-Min, cms_table of every source + a numpy sum +
ske_cms_import; for the tally, tally_list of every source + tally_import; for
the sets nothing ("none").  The exports (ske_hh_export_dev,
ske_tally_export_dev: they return when done) are timed on the host clock.

These are device-call times on one GPU, not multi-GPU scaling: no collective
runs here.  After the timing every merged structure must equal the host sum.

    python tools/bench_merge.py [--worlds 2,8] [--reps 5] [--out profiles/NAME.json]
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

TABLE = (2000, 7)
SET_SIZES = (1 << 16, 1 << 20)
TALLY_KEYS = 5000


def ms(ts):
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4)}


def host_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ms(ts)


class OnStream:
    """The destination's calls run on a torch stream, so torch events time them."""

    def __init__(self, torch, client):
        self.torch, self.client = torch, client
        self.stream = torch.cuda.Stream()
        client.ctx.call("ske_set_stream", C.c_void_p(self.stream.cuda_stream))

    def device_ms(self, fn, reps, before=None):
        ts = []
        for i in range(reps + 1):  # the first repeat warms up
            if before is not None:
                before()
            a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            a.record(self.stream)
            fn()
            b.record(self.stream)
            b.synchronize()
            if i:
                ts.append(a.elapsed_time(b))
        return ms(ts)


def set_entries(first: int, n: int):
    """ids b"%016x" of first .. first + n - 1 as the export's arrays"""
    v = np.arange(first, first + n, dtype=np.uint64)
    ids = np.empty((n, 16), np.uint8)
    for j in range(16):
        d = ((v >> np.uint64(4 * (15 - j))) & np.uint64(15)).astype(np.uint8)
        ids[:, j] = np.where(d < 10, 48 + d, 87 + d)
    return ids, np.full(n, 16, np.uint32)


def run_world(pkg, torch, world: int, reps: int) -> list:
    dev = torch.device("cuda", 0)
    srcs = [pkg.SketchClient(decode_responses=True, device=0) for _ in range(world)]
    dst = pkg.SketchClient(decode_responses=True, device=0)
    on = OnStream(torch, dst)
    rng = np.random.default_rng(world)
    rows = []

    def u8(nbytes):
        return torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=dev)

    # ---- Count-Min: world tables of 2000 x 7
    width, depth = TABLE
    ncells = width * depth
    stride = (ncells + 3) & ~3
    want = np.zeros(ncells, np.uint64)
    counts = []
    for s in srcs + [dst]:
        s.cms_initbydim("k", width, depth)
    for s in srcs:
        cells = rng.integers(0, 1 << 30, ncells, dtype=np.uint64).astype(np.uint32)
        cnt = int(cells.astype(np.uint64).sum()) // depth
        s.ctx.call("ske_cms_import", s.cms_cid("k"), cells.ctypes.data_as(C.c_void_p), ncells, cnt)
        want += cells
        counts.append(cnt)
    tables = u8(world * stride * 4)
    torch.cuda.synchronize()
    for k, s in enumerate(srcs):
        p, _ = s.cms_table_dev("k")
        dst.ctx.call("ske_memcpy", C.c_void_p(tables.data_ptr() + k * stride * 4), C.c_void_p(p), stride * 4, 2)
    dev_t = on.device_ms(lambda: dst.cms_sum_dev("k", tables, stride, counts), reps)
    exact = np.array_equal(dst.cms_table("k")[0].reshape(-1), np.minimum(want, 0xFFFFFFFF).astype(np.uint32))

    def cms_host():
        acc = np.zeros((depth, width), np.uint64)
        total = 0
        for s in srcs:
            t, c = s.cms_table("k")
            acc += t
            total += c
        cells = np.minimum(acc, 0xFFFFFFFF).astype(np.uint32)
        dst.ctx.call("ske_cms_import", dst.cms_cid("k"), cells.ctypes.data_as(C.c_void_p), ncells, total)
    host_t = host_ms(cms_host, reps)
    rows.append({"world": world, "what": "cms_sum", "table": list(TABLE), "device_call": dev_t,
                 "host_composition": host_t, "host_over_device": round(host_t["ms_median"] / dev_t["ms_median"], 1),
                 "exact": bool(exact)})

    # ---- heavy-hitter sets: per context n members, half shared with the next context
    for n in SET_SIZES:
        log2 = int(n).bit_length() + 1          # sources at a quarter load
        union = (world + 1) * (n // 2)
        dlog2 = min(int(union - 1).bit_length() + 1, 24)
        ids_all, lens_all = u8(world * n * 16), u8(world * n * 4)
        export_t = []
        for r, s in enumerate(srcs):
            s.hh_create("s%d" % n, "k", log2)
            ids, lens = set_entries(r * (n // 2), n)
            d_ids = torch.from_numpy(ids.reshape(-1)).to(dev)
            d_lens = torch.from_numpy(lens.view(np.uint8)).to(dev)
            torch.cuda.synchronize()
            s.hh_merge_dev("s%d" % n, d_ids, d_lens, n)
            s.ctx.call("ske_sync")
            assert s.hh_info("s%d" % n) == {"capacity": 1 << log2, "used": n, "overflow": 0}
            seg_ids, seg_lens = ids_all[r * n * 16:(r + 1) * n * 16], lens_all[r * n * 4:(r + 1) * n * 4]
            t0 = time.perf_counter()
            got, ov = s.hh_export_dev("s%d" % n, seg_ids, seg_lens, n)
            export_t.append((time.perf_counter() - t0) * 1e3)
            assert (got, ov) == (n, 0)
        name = "d%d" % n
        dst.hh_create(name, "k", dlog2)

        def merge_all():
            for r in range(world):
                dst.hh_merge_dev(name, ids_all[r * n * 16:(r + 1) * n * 16], lens_all[r * n * 4:(r + 1) * n * 4], n)
        dev_t = on.device_ms(merge_all, reps, before=lambda: dst.hh_reset(name))
        info = dst.hh_info(name)
        rows.append({"world": world, "what": "hh_merge", "members_per_context": n, "union": union,
                     "capacity_log2": dlog2, "device_calls": dev_t, "per_call_ms": round(dev_t["ms_median"] / world, 4),
                     "export_call_host_clock": ms(export_t), "host_composition": "none",
                     "exact": info["used"] == union and info["overflow"] == 0})
        for s in srcs:
            s.hh_free("s%d" % n)
        dst.hh_free(name)
        del ids_all, lens_all

    # ---- tallies: 5000 keys per context, the same keys everywhere
    keys = [b"L%08d" % i for i in range(TALLY_KEYS)]
    kb = np.zeros((TALLY_KEYS, 32), np.uint8)
    kb[:, :9] = np.frombuffer(b"".join(keys), np.uint8).reshape(TALLY_KEYS, 9)
    lens = np.full(TALLY_KEYS, 9, np.uint32)
    total_ev = np.zeros(TALLY_KEYS, np.uint64)
    n = TALLY_KEYS
    packed = u8(world * n * 52)
    segs = []
    for r, s in enumerate(srcs):
        s.tally_create("t", 14)
        ev = rng.integers(1, 1 << 20, TALLY_KEYS).astype(np.uint64)
        s.tally_import("t", keys, ev, ev // 2)
        total_ev += ev
        base = packed[r * n * 52:(r + 1) * n * 52]
        seg = (base[:32 * n], base[48 * n:], base[32 * n:40 * n], base[40 * n:48 * n])
        torch.cuda.synchronize()
        assert s.tally_export_dev("t", *seg, n) == n
        segs.append(seg)
    dst.tally_create("t", 14)

    def tally_all():
        for seg in segs:
            dst.tally_merge_dev("t", *seg, n)
    dev_t = on.device_ms(tally_all, reps, before=lambda: dst.tally_reset("t"))
    got = dst.tally_list("t")
    exact = got[3] and dict(zip(got[0], got[1].tolist())) == dict(zip(keys, total_ev.tolist()))

    def tally_host():
        dst.tally_reset("t")
        for s in srcs:
            k, e, v, _ = s.tally_list("t")
            dst.tally_import("t", k, e, v)
    host_t = host_ms(tally_host, reps)
    rows.append({"world": world, "what": "tally_merge", "keys_per_context": TALLY_KEYS, "device_calls": dev_t,
                 "host_composition": host_t, "host_over_device": round(host_t["ms_median"] / dev_t["ms_median"], 1),
                 "exact": bool(exact)})
    for c in srcs + [dst]:
        c.flushall()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="2,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = ge.load_package()
    import torch
    results = []
    for world in [int(w) for w in args.worlds.split(",")]:
        for row in run_world(pkg, torch, world, args.reps):
            results.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "counts_merge", "timing": "device events on the destination's stream around the "
                       "merge calls of one repeat, median over warmed repeats (set and tally resets outside the "
                       "events); host compositions and exports on the host clock; one GPU, no collective",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["exact"] for r in results):
        sys.exit("a merged structure is not the host sum")


if __name__ == "__main__":
    main()
