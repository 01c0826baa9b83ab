#!/usr/bin/env python
"""Time the bulk HLL dump / load against the per-key loop on the GPU.

For each size: that many day keys filled as C5 fills them (about 17 ids a key,
one PFADD batch), plus ``--dense`` keys whose registers force the dense
encoding.  Over the same keys, round by round:

    sizes      ske_hll_dump_sizes, every array on the device (one read of the rows)
    dump       ske_hll_dump, every array on the device (its own sizes launch,
               then the strings: two reads of the rows)
    dump_hlls  the facade: the strings as host bytes
    load_hlls  the facade: the same strings back into their keys
    loop_dump  [dump_hll(k) for k in keys]   -- one key a call, encoded on the host
    loop_load  load_hll(k, s) for every key  -- the code as it was before the bulk calls

    python tools/bench_hll_dump.py [--log2 12 16] [--dense 2048] [--rounds 7] [--loop-rounds 3]
                                   [--out profiles/NAME.json]

Timing: the host clock around the synchronous calls, median of the rounds
after one warm-up of every form.  The bulk strings must equal the loop's.
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

STREAM_BYTES_PER_S = 6.29e12  # the slab streamed once
IDS_PER_KEY = 17
ROW = 16384


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=[12, 16])
    ap.add_argument("--dense", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    pkg = ge.load_package()
    from rtsas_amd.engine import DeviceBuffer, SketchEngine

    results = []
    for log2 in args.log2:
        client = pkg.SketchClient(decode_responses=True, device=0)
        eng = SketchEngine(ctx=client.ctx)
        ctx = client.ctx
        nsparse, ndense = 1 << log2, args.dense
        rng = np.random.default_rng(log2)
        names = [f"hll:unique:L{i:06d}:2025-03-19" for i in range(nsparse)] + [f"hll:dense:{i}" for i in range(ndense)]
        slots = np.asarray([client.key_slot(n) for n in names], np.uint32)
        n = slots.size
        ids = rng.integers(10_000_000, 100_000_000, nsparse * IDS_PER_KEY)
        buf, offs = pkg.pack_ints(ids)
        client.pfadd_packed(np.repeat(slots[:nsparse], IDS_PER_KEY), buf, offs)
        if ndense:  # rows with registers above 32, written straight into the slab (the slots are consecutive)
            rows = rng.integers(0, 40, (ndense, ROW)).astype(np.uint8)
            assert (np.diff(slots[nsparse:].astype(np.int64)) == 1).all()
            p, nb = C.c_void_p(), C.c_uint64()
            ctx.call("ske_hll_slab", C.byref(p), C.byref(nb))
            ctx.call("ske_memcpy", C.c_void_p(p.value + int(slots[nsparse]) * ROW), rows.ctypes.data_as(C.c_void_p),
                     rows.nbytes, 0)

        dslots, doffs = DeviceBuffer(ctx, 4 * n), DeviceBuffer(ctx, 4 * n + 4)
        dslots.from_host(slots)
        eng.hll_dump_sizes(dslots, n, doffs)
        total = int(doffs.to_host(np.uint32, n + 1)[-1])
        dout = DeviceBuffer(ctx, total)
        strings = client.dump_hlls(names)
        assert sum(map(len, strings)) == total
        pairs = list(zip(names, strings))

        def loop_dump():
            return [client.dump_hll(k) for k in names]

        def loop_load():
            for k, s in pairs:
                client.load_hll(k, s)

        fast = {"sizes": lambda: eng.hll_dump_sizes(dslots, n, doffs), "dump": lambda: eng.hll_dump(dslots, n, dout, doffs),
                "dump_hlls": lambda: client.dump_hlls(names), "load_hlls": lambda: client.load_hlls(pairs)}
        slow = {"loop_dump": loop_dump, "loop_load": loop_load}
        times = {f: [] for f in list(fast) + list(slow)}
        for fn in fast.values():  # warm: scratch and staging sized, code loaded
            fn()
        same = loop_dump() == strings  # the loop's warm-up, and the check
        loop_load()
        for r in range(args.rounds):
            for f, fn in fast.items():
                times[f].append(timed(fn)[0])
            if r < args.loop_rounds:
                for f, fn in slow.items():
                    times[f].append(timed(fn)[0])
            print(f"# log2 {log2} round {r}: " + " ".join(f"{f} {t[-1]:.3f}" for f, t in times.items() if len(t) > r),
                  flush=True)
        same = same and client.dump_hlls(names) == strings  # the loads put back what was there
        row = {"sparse_keys": nsparse, "dense_keys": ndense, "ids_per_key": IDS_PER_KEY, "string_bytes": total,
               "row_bytes": n * ROW, "strings_equal": bool(same)}
        for f, t in times.items():
            row[f] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4),
                      "ms_max": round(max(t), 4), "rounds": len(t)}
        row["loop_dump_over_dump_hlls"] = round(row["loop_dump"]["ms_median"] / row["dump_hlls"]["ms_median"], 2)
        row["loop_load_over_load_hlls"] = round(row["loop_load"]["ms_median"] / row["load_hlls"]["ms_median"], 2)
        for f, reads in (("sizes", 1), ("dump", 2)):
            rate = reads * n * ROW / (row[f]["ms_median"] * 1e-3)
            row[f + "_read_TBps"] = round(rate / 1e12, 4)
            row[f + "_read_over_stream"] = round(rate / STREAM_BYTES_PER_S, 4)
        results.append(row)
        print(json.dumps(row), flush=True)
        for b in (dslots, doffs, dout):
            b.free()
        client.flushall()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "hll_dump_bulk_vs_loop", "timing": "host clock around each synchronous call; median over "
                       "rounds after a warm-up of every form; the loop forms are dump_hll / load_hll per key",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not all(r["strings_equal"] for r in results):
        sys.exit("the bulk strings differ from the loop's")


if __name__ == "__main__":
    main()
