#!/usr/bin/env python
"""Time the row log on the GPU: appends of 2^25 rows resident on the device in
the three forms (packed id text, parse-column spans, fixed 8-byte ids), each
into an emptied log; then, over the log the last append left, the select of one
lecture out of 5000 (the lectures drawn from a Zipf law, the most and a
middling frequent one) and of the whole log, outputs on the device.  One row in
ten is a redelivery of an earlier row of the batch, so the selects collapse.
The answers are checked: the log's counts, and the selects' row counts against
the host's.

Beside each select, in the same run, the host alternative over the same log:
``rows_read``, a numpy mask, ``np.lexsort``, last of each run.

    python tools/bench_rows.py [--n 33554432] [--rounds 5] [--out profiles/NAME.json]
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
LECTURES = 5000
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def digits(v: np.ndarray, width: int, lead: bytes = b"") -> np.ndarray:
    """``lead`` + the zero-padded decimal of every value: [n, len(lead) + width] uint8"""
    out = np.empty((v.size, len(lead) + width), np.uint8)
    out[:, :len(lead)] = np.frombuffer(lead, np.uint8)
    x = v.astype(np.uint64)
    for j in range(len(lead) + width - 1, len(lead) - 1, -1):
        out[:, j] = 48 + x % 10
        x //= 10
    return out


def host_select(cols, digest):
    """rows_read's columns -> the rows a select returns: mask, lexsort, last of each run"""
    lec, ep, ids, valid = cols
    at = np.arange(lec.size) if digest is None else np.nonzero(lec == digest)[0]
    keys = (at, ids[at], ep[at]) if digest is not None else (at, ids[at], ep[at], lec[at])
    order = at[np.lexsort(keys)]
    a, b = order[:-1], order[1:]
    last = np.ones(order.size, bool)
    last[:-1] = (lec[a] != lec[b]) | (ep[a] != ep[b]) | (ids[a] != ids[b])
    keep = order[last]
    return lec[keep], ep[keep], ids[keep], valid[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 25)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    ge.load_package()
    from rtsas_amd.client_rows import lecture_digest
    from rtsas_amd.engine import DeviceBuffer, SketchEngine, rows_read

    eng = SketchEngine(0)
    ctx, n = eng.ctx, args.n
    log2 = max(8, (n - 1).bit_length())
    rng = np.random.default_rng(2025)

    # the rows: one in ten repeats an earlier row of the batch
    row = np.arange(n, dtype=np.int64)
    again = np.nonzero(rng.random(n) < 0.1)[0]
    again = again[again > 0]
    row[again] = (rng.random(again.size) * again).astype(np.int64)
    row = row[row]
    rank = np.minimum(rng.zipf(1.2, n), LECTURES) - 1  # lecture 0 the most frequent
    rank = rank[row]
    sid = 10_000_000 + (row * 7919) % 80_000_000  # 8 digits, no leading zero: canonical
    ep = (MONDAY + row % (7 * 86400)).astype(np.int64)
    lec_txt, id_txt = digits(rank, 8, b"L"), digits(sid, 8)
    distinct = int(np.unique(row).size)

    up = {}

    def dev(name, arr):
        a = np.ascontiguousarray(arr)
        up[name] = DeviceBuffer(ctx, a.nbytes + 64)
        up[name].from_host(a)
        return C.c_void_p(up[name].ptr)

    lec = dev("lec", lec_txt)
    lec_offs = dev("lec_offs", (np.arange(n + 1, dtype=np.uint64) * 9).astype(np.uint32))
    ids = dev("ids", id_txt)
    id_offs = dev("id_offs", (np.arange(n + 1, dtype=np.uint64) * 8).astype(np.uint32))
    fixed = dev("fixed", sid.astype("<i8"))
    blob = dev("blob", np.concatenate([lec_txt, id_txt], axis=1))  # each row's lecture, then its id
    starts = (np.arange(n, dtype=np.uint64) * 17).astype(np.uint32)
    lec_start, id_start = dev("lec_start", starts), dev("id_start", starts + np.uint32(9))
    lec_len, id_len = dev("lec_len", np.full(n, 9, np.uint32)), dev("id_len", np.full(n, 8, np.uint32))
    status = dev("status", np.zeros(n, np.uint8))
    d_ep, valid = dev("ep", ep), dev("valid", (row % 3 != 0).astype(np.uint8))
    del lec_txt, id_txt, starts

    eng.rows_init(0, log2)
    forms = {
        "packed": lambda: ctx.call("ske_rows_append_packed_async", 0, lec, lec_offs, ids, id_offs, d_ep, valid, None, n),
        "spans": lambda: ctx.call("ske_rows_append_spans_async", 0, blob, lec_start, lec_len, id_start, id_len, status,
                                  d_ep, valid, None, n),
        "fixed": lambda: ctx.call("ske_rows_append_fixed_async", 0, lec, lec_offs, fixed, 8, d_ep, valid, None, n),
    }
    results, exact = [], True
    for form, call in forms.items():
        call()  # warm up: the context scratch, the code objects
        eng.sync()
        ms = []
        for _ in range(args.rounds):
            call()  # the device busy right up to the timed window
            eng.rows_reset(0)
            t0 = time.perf_counter()
            call()
            eng.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        info = eng.rows_info(0)
        ok = (info["used"], info["taken"], info["refused_ids"], info["dropped"]) == (n, n, 0, 0)
        exact &= ok
        r = {"bench": "append", "form": form, "n": n, "counts_exact": ok,
             "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
             "rows_per_s_median": round(n / statistics.median(ms) * 1e3)}
        results.append(r)
        print(json.dumps(r), flush=True)

    t0 = time.perf_counter()
    cols = rows_read(ctx, 0, 0, n)
    read_ms = (time.perf_counter() - t0) * 1e3
    out = [DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64), DeviceBuffer(ctx, n * 8 + 64),
           DeviceBuffer(ctx, n + 64)]
    outp = [C.c_void_p(b.ptr) for b in out]
    for name, lecture in (("lecture_rank_0", b"L00000000"), ("lecture_rank_500", b"L00000500"), ("whole_log", None)):
        n_out, complete = C.c_uint64(), C.c_int()

        def select():
            ctx.call("ske_rows_select", 0, None if lecture is None else C.c_char_p(lecture),
                     0 if lecture is None else len(lecture), I64_MIN, I64_MAX, *outp, n, C.byref(n_out),
                     C.byref(complete), 1)

        select()
        ms = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            select()
            ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = host_select(cols, None if lecture is None else np.uint64(lecture_digest(lecture)))
        host_ms = (time.perf_counter() - t0) * 1e3
        k = int(n_out.value)
        got = [b.to_host(w.dtype, k) for b, w in zip(out, want)]
        ok = k == want[0].size and all(np.array_equal(g, w) for g, w in zip(got, want)) and bool(complete.value)
        if lecture is None:
            ok = ok and k == distinct
        exact &= ok
        r = {"bench": "select", "what": name, "n": n, "rows_out": k, "answers_exact": ok,
             "ms_median": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
             "host_mask_lexsort_last": {"ms": round(host_ms, 1), "rows_read_ms": round(read_ms, 1)}}
        results.append(r)
        print(json.dumps(r), flush=True)
    eng.rows_free(0)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"bench": "rows", "timing": "host clock around the enqueued call(s) and one stream synchronise; "
                       "median over rounds; an append goes into a log emptied just before (not timed); a select is "
                       "the whole synchronous call, outputs on the device; host: numpy over the columns rows_read "
                       "brought back once (its time beside)",
                       "results": results}, f, indent=1)
            f.write("\n")
    if not exact:
        sys.exit("the log's counts or a select's rows are not the host's")


if __name__ == "__main__":
    main()
