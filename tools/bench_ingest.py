"""Ingest throughput: raw JSON payloads in host memory ->
BF.EXISTS answers + PFADDs, through ``SketchClient.ingest`` (device JSON
decode, device key table, fused K1), against the reference's per-event
Python loop (attendance_processor.py:100-137: json.loads, fromisoformat,
BF.EXISTS, PFADD) over the CPU oracle on a sample of the same messages.

Messages follow the reference generator's schema (data_generator.py:112-118):
{"student_id": <5-digit int>, "timestamp": "<ISO>", "lecture_id":
"LECTURE_<YYYYMMDD>", "is_valid": ..., "event_type": ...}, C2-sized: 100k
students (10 % invalid swipes), 50 lecture days.  The timed region includes
the host-side packing and the H2D copy of the payloads (PCIe), so the rate is
end to end.

"insight_stages" times what ``StudentCounts.update_messages`` adds behind the
ingest, over the same batch in one session: the device stages one by one
(host clock around calls that end in a stream synchronise, ``--inner`` calls
per timing, best and median of ``--reps``) beside the two ingest kernels
they follow, ske_ingest_parse and ske_ingest_swipes; the whole
``update_messages_packed`` call; and the host alternative, ``count_packed``
fed by per-message json.loads + fromisoformat, on the CPU sample.
usage: python tools/bench_ingest.py [--messages N] [--reps R]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def make_messages(rng, n, members, invalid):
    days = rng.integers(0, 50, n)
    bad = rng.random(n) < 0.10
    ids = np.where(bad, rng.choice(invalid, n), rng.choice(members, n))
    hh, mm = rng.integers(8, 18, n), rng.integers(0, 60, n)
    out = []
    for i in range(n):
        d = 1 + int(days[i]) % 28
        mo = 3 + int(days[i]) // 28
        ts = f"2025-{mo:02d}-{d:02d}T{int(hh[i]):02d}:{int(mm[i]):02d}:00"
        out.append(('{"student_id": %d, "timestamp": "%s", "lecture_id": "LECTURE_2025%02d%02d", '
                    '"is_valid": %s, "event_type": "entry"}' % (ids[i], ts, mo, d,
                                                                  "false" if bad[i] else "true")).encode())
    return out


def timed(fn, sync, reps, inner):
    """best and median seconds of one fn() call followed through to the device's end"""
    fn()
    sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / inner)
    return {"best_s": min(out), "median_s": float(np.median(out))}


def insight_stages(pkg, client, msgs, blob, moffs, reps, inner, cpu_messages):
    """The stages behind the ingest that turn the decoded messages into the
    counters of ``StudentCounts`` (every option on), each over the whole batch."""
    from datetime import datetime
    from rtsas_amd._lib import IngestDense
    n = len(msgs)
    sc = pkg.StudentCounts(client, track_attended=40, track_invalid=5, late_key="cms:late", track_late=20,
                           day_profile="week")
    valid, status = sc.update_messages_packed("bf:students", blob, moffs)  # warm: buffers, keys
    ctx, fid = client.ctx, client.keys.fid[b"bf:students"]
    run = client._ingest_batch("bf:students", blob, moffs, "hll:unique:", "readme")[2]
    B, cols = run.B, run.cols
    d = sc._packed_buffers("dense", n, B["msgs"].nbytes)
    msgs_p, moffs_p = C.c_void_p(B["msgs"].ptr), C.c_void_p(B["moffs"].ptr)
    out = IngestDense(*[C.c_void_p(d[k].ptr) for k in ("ids", "offs", "epoch", "valid", "at")])
    nd, nb, taken = C.c_uint64(), C.c_uint64(), C.c_uint64()

    def sync():
        ctx.call("ske_sync")

    def dense():
        ctx.call("ske_ingest_dense", msgs_p, C.byref(cols), n, C.c_void_p(B["valid"].ptr),
                 C.c_void_p(d["epoch_all"].ptr), C.byref(out), d["nbytes"], C.byref(nd), C.byref(nb))
    stages = {
        "ske_ingest_parse": lambda: ctx.call("ske_ingest_parse", msgs_p, moffs_p, n, 1, C.byref(cols)),
        "ske_ingest_swipes": lambda: ctx.call("ske_ingest_swipes", fid, msgs_p, C.byref(cols), n,
                                              C.c_void_p(B["valid"].ptr), C.byref(taken)),
        "ske_ingest_times": lambda: ctx.call("ske_ingest_times", msgs_p, C.byref(cols), n,
                                             C.c_void_p(d["epoch_all"].ptr)),
        "ske_ingest_dense": dense,
    }
    res = {k: timed(f, sync, reps, inner) for k, f in stages.items()}
    ndense = int(nd.value)
    res["packed_adds_and_tracks"] = timed(
        lambda: sc._enqueue_packed(d["ids"], d["offs"], ndense, d["valid"], d["epoch"], d["late"]), sync, reps, inner)
    res["packed_adds_and_tracks"]["calls"] = "3 ske_cms_add_packed_async, ske_tp_add_async, 3 ske_hh_track_packed_async"
    res["update_messages_packed"] = timed(lambda: sc.update_messages_packed("bf:students", blob, moffs),
                                          sync, reps, 1)
    res["ingest_packed"] = timed(lambda: client.ingest_packed("bf:students", blob, moffs), sync, reps, 1)
    # the host alternative: every message decoded by Python, then count_packed
    sample = msgs[:cpu_messages]
    t0 = time.perf_counter()
    ids, tss = [], []
    for m in sample:
        data = json.loads(m.decode())
        ids.append(pkg.encode(data["student_id"]))
        tss.append(datetime.fromisoformat(data["timestamp"]))
    t_decode = time.perf_counter() - t0
    buf, offs = pkg.pack(ids)
    cp = timed(lambda: sc.count_packed(buf, offs, valid[:len(sample)], tss), sync, reps, 1)
    res["host_alternative"] = {"sample": len(sample), "decode_s": t_decode, "count_packed": cp,
                               "messages_per_s": len(sample) / (t_decode + cp["best_s"])}
    return {"messages": n, "dense": ndense, "dense_id_bytes": int(nb.value), "inner": inner, "stages": res,
            "update_messages_per_s": n / res["update_messages_packed"]["best_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-messages", type=int, default=50_000)
    ap.add_argument("--inner", type=int, default=20, help="calls per timing of one device stage")
    args = ap.parse_args()
    pkg = ge.load_package()
    orc = ge.load_oracle()
    rng = np.random.default_rng(20251003)
    members = rng.choice(np.arange(10000, 100000), 20_000, replace=False)
    invalid = np.setdiff1d(np.arange(100000, 200000), members)[:50]
    msgs = make_messages(rng, args.messages, members, invalid)
    client = pkg.SketchClient(decode_responses=True)
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 100000)
    client.bf_madd_packed("bf:students", *pkg.pack_ints(members))
    client.ingest("bf:students", msgs[:1000])  # warm: key table, buffers
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        valid, status = client.ingest("bf:students", msgs)
        times.append(time.perf_counter() - t0)
    best = min(times)
    # the same payloads already laid end to end (what a network consumer fills)
    blob = np.frombuffer(b"".join(msgs), np.uint8)
    moffs = np.zeros(len(msgs) + 1, np.uint32)
    np.cumsum(np.fromiter(map(len, msgs), np.uint32, count=len(msgs)), out=moffs[1:])
    ptimes = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        valid_p, _ = client.ingest_packed("bf:students", blob, moffs)
        ptimes.append(time.perf_counter() - t0)
    assert np.array_equal(valid_p, valid)
    # the reference's per-event loop over the oracle, on a sample
    chain = orc.Chain(100000, 0.01)
    for m in members:
        chain.add(str(int(m)).encode())
    hlls = {}
    from datetime import datetime
    sample = msgs[:args.cpu_messages]
    t0 = time.perf_counter()
    for m in sample:
        data = json.loads(m.decode())
        sid = str(data["student_id"]).encode()
        ts = datetime.fromisoformat(data["timestamp"])
        if chain.exists(sid):
            hlls.setdefault(f"hll:unique:{data['lecture_id']}:{ts.date().isoformat()}",
                            orc.HLL()).add(sid)
    cpu_s = time.perf_counter() - t0
    stages = insight_stages(pkg, client, msgs, blob, moffs, args.reps, args.inner, args.cpu_messages)
    print(json.dumps({
        "metric": "ingested swipes/s (packed JSON payloads in host memory -> answers + PFADD), end to end",
        "messages": args.messages, "payload_bytes": int(sum(len(m) for m in msgs)),
        "value": args.messages / min(ptimes), "best_s": min(ptimes),
        "list_of_bytes": {"value": args.messages / best, "best_s": best,
                          "note": "includes b''.join / lengths of the Python message list"},
        "device_decoded_frac": float((status == 0).mean()), "valid_frac": float(valid.mean()),
        "cpu_reference_loop": {"value": len(sample) / cpu_s, "unit": "swipes/s", "cores": 1,
                               "sample": f"{len(sample)} messages, json.loads + fromisoformat + "
                                         "oracle BF.EXISTS / PFADD per event"},
        "insight_stages": stages,
    }), flush=True)


if __name__ == "__main__":
    main()
