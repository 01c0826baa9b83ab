"""Insights from the message stream, the parts that need no GPU: the timestamp
arithmetic of sketch_common.h (``iso_epoch``; a stand-alone program,
tests/native/iso_host.cpp) against ``epoch_seconds(datetime.fromisoformat(...))``,
the argument checks that come before any device call, the header against the
ctypes prototypes, and over a context stub the native call sequences of
``StudentCounts.count_packed`` / ``update_messages`` and of
``AttendanceProcessor.process_batch`` with and without a ``StudentCounts``.

The program can also be built by hand with the host sanitizers:
    hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \\
        -o iso_host tests/native/iso_host.cpp && ./iso_host 2025 3 19 9 0 0 0 0 0
"""
import ctypes as C
import json
import os
import re
import subprocess
from datetime import datetime, timedelta

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOT = ("ske_device_alloc", "ske_memcpy", "ske_device_free")
NEW = ("ske_ingest_times", "ske_ingest_dense", "ske_cms_add_packed_async", "ske_hh_track_packed_async")

ISO = re.compile(r"(\d{4})-(\d\d)-(\d\d)(?:.(\d\d):(\d\d):(\d\d)(?:\.(?:\d{3}|\d{6}))?(?:([+-])(\d\d):(\d\d))?)?$",
                 re.S)


def iso_fields(text):
    """The nine fields iso_host takes, of a fast-path timestamp."""
    m = ISO.match(text)
    assert m, text
    y, mo, d, hh, mi, ss, sg, oh, om = m.groups()
    return [int(y), int(mo), int(d), int(hh or 0), int(mi or 0), int(ss or 0),
            0 if sg is None else (1 if sg == "+" else -1), int(oh or 0), int(om or 0)]


@pytest.fixture(scope="module")
def iso_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "iso_host.cpp")
    exe = str(tmp_path_factory.mktemp("iso") / "iso_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)

    def run(texts):
        args = [str(v) for t in texts for v in iso_fields(t)]
        out = subprocess.run([exe] + args, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        got = [int(line) for line in out.stdout.splitlines()]
        assert len(got) == len(texts)
        return got
    return run


def by_datetime(pkg, text):
    return int(pkg.epoch_seconds([datetime.fromisoformat(text)])[0])


PINS = {
    "2025-03-19T08:59:59": 1742374799, "2025-03-19T09:00:00": 1742374800,
    "1969-12-31T23:59:58.250": -2, "0001-01-01": -62135596800, "9999-12-31T23:59:59": 253402300799,
    "1970-01-01": 0, "1970-01-01 00:00:00.000000": 0,
    # offsets across a day and a year boundary
    "2025-03-19T02:10:00+05:30": 1742330400, "2025-03-19T23:30:00-02:00": 1742434200,
    "2025-01-01T00:00:00+23:59": 1735689600 - 86340, "2024-12-31T23:59:59-23:59": 1735689599 + 86340,
    "1970-01-01T00:00:00+00:01": -60, "1969-12-31T23:59:59.999-00:01": 59,
    # leap days
    "2000-02-29T12:00:00": 951825600, "2024-02-29": 1709164800, "2000-03-01": 951868800,
}


def test_pins(pkg, iso_host):
    texts = list(PINS)
    for t, got in zip(texts, iso_host(texts)):
        assert by_datetime(pkg, t) == PINS[t], t  # the pins themselves
        assert got == PINS[t], (t, got)


def test_against_datetime(pkg, iso_host):
    rng = np.random.default_rng(19700101)
    lo, hi = datetime(2, 1, 1), datetime(9998, 12, 31, 23, 59, 59)
    span = int((hi - lo).total_seconds())
    texts = []
    for k in range(1000):
        t = lo + timedelta(seconds=int(rng.integers(0, span, endpoint=True)))
        form = k % 6
        if form == 0:
            texts.append(t.date().isoformat())
            continue
        text = t.isoformat(sep="T _"[k % 3])
        if form in (2, 4):
            text += ".%03d" % rng.integers(0, 1000)
        if form in (3, 5):
            text += ".%06d" % rng.integers(0, 1000000)
        if form >= 4 or k % 7 == 0:
            text += "%s%02d:%02d" % ("+-"[int(rng.integers(0, 2))], rng.integers(0, 24), rng.integers(0, 60))
        texts.append(text)
    assert len({len(t) for t in texts}) == 7  # every length the fast path accepts
    got = iso_host(texts)
    for t, g in zip(texts, got):
        assert g == by_datetime(pkg, t), (t, g)


def header_prototypes():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sketch.h")).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(",")]
            for m in re.finditer(r"\bint (ske_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def test_header_and_prototypes_agree(pkg):
    from rtsas_amd import _lib
    protos = header_prototypes()
    for name in NEW:
        args = protos[name]
        res, types = _lib.SIGNATURES[name]
        assert res is C.c_int and len(types) == len(args), name
        for a, t in zip(args, types):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a)
            elif a.startswith("uint64_t"):
                assert t is C.c_uint64, (name, a)
            elif a.startswith("uint32_t"):
                assert t is C.c_uint32, (name, a)
            else:
                assert a.startswith("int ") and t is C.c_int, (name, a)
    # ske_ingest_dense_t field by field
    hdr = open(os.path.join(ROOT, "include", "sketch.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} ske_ingest_dense_t;", hdr).group(1)
    assert re.findall(r"\*(\w+);", body) == [f[0] for f in _lib.IngestDense._fields_]
    assert C.sizeof(_lib.IngestDense) == 5 * C.sizeof(C.c_void_p)
    # the cols struct keeps its layout
    assert [f[0] for f in _lib.IngestCols._fields_] == ["status", "id_start", "id_len", "lec_start", "lec_len",
                                                        "ts_start", "ts_len", "day", "kh"]
    # the capture comment names the enqueue-only newcomers
    cap = re.search(r"---- stream capture \(HIP graphs\) ----(.*?)\*/", hdr, re.S).group(1)
    for name in ("ske_cms_add_packed_async", "ske_hh_track_packed_async"):
        assert name in cap


def test_null_context_is_rejected(pkg):
    from rtsas_amd import _lib
    lib = pkg.load_library()
    cols, out = _lib.IngestCols(), _lib.IngestDense()
    nd, nb = C.c_uint64(7), C.c_uint64(7)
    assert lib.ske_ingest_times(None, None, C.byref(cols), 0, None) == -1
    assert lib.ske_ingest_dense(None, None, C.byref(cols), 0, None, None, C.byref(out), 0, C.byref(nd),
                                C.byref(nb)) == -1
    assert lib.ske_cms_add_packed_async(None, 0, None, None, 0, None, None, 1) == -1
    assert lib.ske_hh_track_packed_async(None, 0, 0, None, None, 0, None, 1, 1) == -1


def make_client(pkg, hooks=None):
    ctx = StubContext(pkg.load_library())
    ctx.hooks.update(hooks or {})
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    return cl, ctx


def cold(ctx):
    return [c for c in ctx.log if c[0] not in HOT]


OPTIONS = [
    dict(),
    dict(day_profile="week"),
    dict(late_key="cms:late"),
    dict(late_key="cms:late", track_late=2),
    dict(track_attended=3, track_invalid=2, capacity_log2=12),
    dict(late_key="cms:late", day_profile="week", track_attended=3, track_invalid=2, capacity_log2=12),
    dict(late_key="cms:late", track_late=3, day_profile="week", track_attended=3, track_invalid=2,
         capacity_log2=12),
]


def counting_calls(cl, sc, n):
    """What ``_enqueue_packed`` makes over n packed ids, in ``update``'s order."""
    opt_late, timed = sc.late_key is not None, sc.timed
    want = [["ske_cms_add_packed_async", cl.cms_cid(sc.attended_key), "*", "*", n, None, "*", 1],
            ["ske_cms_add_packed_async", cl.cms_cid(sc.invalid_key), "*", "*", n, None, "*", 0]]
    if timed:
        want.append(["ske_tp_add_async", cl.tp_tid(sc._profile), "*", n, None, 1, sc.late_from,
                     "*" if opt_late else None])
    if opt_late:
        want.append(["ske_cms_add_packed_async", cl.cms_cid(sc.late_key), "*", "*", n, None, "*", 1])
    for name, thr, w in sc._tracks + ([sc._late_track] if sc._late_track else []):
        hid, cid = cl._hh_entry(name)
        want.append(["ske_hh_track_packed_async", hid, cid, "*", "*", n, "*", w, thr])
    return want


@pytest.mark.parametrize("opts", OPTIONS)
def test_count_packed_call_sequence(pkg, opts):
    cl, ctx = make_client(pkg)
    sc = pkg.StudentCounts(cl, late_from=8 * 3600, **opts)
    buf, offs = pkg.pack([10001, "", b"abcdefghijklmnopq"])
    times = np.asarray([0, 8 * 3600, -1], np.int64) if sc.timed else None
    ctx.log.clear()
    assert sc.count_packed(buf, offs, [True, False, True], times) is None
    assert cold(ctx) == counting_calls(cl, sc, 3) + [["ske_sync"]]  # no swipe call
    # what is uploaded: ids, offs, valid bytes [, epochs]
    ups = [c for c in ctx.log if c[0] == "ske_memcpy"]
    assert [c[3] for c in ups] == [buf.size, 16, 3] + ([24] if sc.timed else [])
    ctx.log.clear()
    sc.count_packed(np.zeros(0, np.uint8), np.zeros(1, np.uint32), [], np.zeros(0, np.int64) if sc.timed else None)
    assert ctx.log == []


def test_count_packed_value_errors(pkg):
    cl, ctx = make_client(pkg)
    plain = pkg.StudentCounts(cl)
    timed = pkg.StudentCounts(cl, "a2", "i2", day_profile="week")
    late = pkg.StudentCounts(cl, "a3", "i3", late_key="l3")
    buf, offs = pkg.pack([1, 22, 333, 4444])
    ctx.calls.clear()
    with pytest.raises(ValueError):
        plain.count_packed(buf, offs, [1, 1, 0, 0], np.zeros(4, np.int64))  # times without a use for them
    with pytest.raises(ValueError):
        plain.count_packed(buf, offs, [1, 1, 0])  # one answer per id
    for sc in (timed, late):
        with pytest.raises(ValueError):
            sc.count_packed(buf, offs, [1, 1, 0, 0])  # times missing
        for n in (3, 5):
            with pytest.raises(ValueError):
                sc.count_packed(buf, offs, [1, 1, 0, 0], np.zeros(n, np.int64))
    assert ctx.calls == []  # refused before any native call


MESSAGES = [json.dumps({"student_id": 10000 + i, "lecture_id": "L1",
                        "timestamp": "2025-03-19T09:00:0%d" % i}).encode() for i in range(5)]


def status_hook(host):
    """The parse leaves every message to the device but those in ``host``: the
    first n-byte read-back after ske_ingest_parse is the status column."""
    state = {"armed": False}

    def parse(*a):
        state["armed"] = True

    def memcpy(dst, src, nbytes, kind):
        if state["armed"] and kind == 1 and nbytes == len(MESSAGES):
            state["armed"] = False
            st = (C.c_uint8 * nbytes).from_address(dst.value)
            for m in host:
                st[m] = 1
    return {"ske_ingest_parse": parse, "ske_memcpy": memcpy}


@pytest.mark.parametrize("host", [(), (1, 3)])
@pytest.mark.parametrize("opts", OPTIONS)
def test_update_messages_call_sequence(pkg, opts, host):
    # ingest's own calls over the same batch
    cl0, ctx0 = make_client(pkg, status_hook(host))
    ctx0.log.clear()
    valid0, status0 = cl0.ingest("bf", MESSAGES)
    ingest_calls = cold(ctx0)
    assert [c[0] for c in ingest_calls][:4] == ["ske_ingest_parse", "ske_keytab_clear", "ske_keytab_lookup",
                                                "ske_ingest_swipes"]
    assert status0.tolist() == [1 if m in host else 0 for m in range(5)]

    hooks = status_hook(host)
    ndense = 5 - len(host)

    def dense(msgs, cols, n, valid, epoch, out, cap, nd, nb):
        nd._obj.value, nb._obj.value = ndense, 5 * ndense
    hooks["ske_ingest_dense"] = dense
    cl, ctx = make_client(pkg, hooks)
    sc = pkg.StudentCounts(cl, late_from=8 * 3600, **opts)
    ctx.log.clear()
    valid, status = sc.update_messages("bf", MESSAGES)
    assert np.array_equal(valid, valid0) and np.array_equal(status, status0)
    want = list(ingest_calls)
    if sc.timed:
        want.append(["ske_ingest_times", "*", "*", 5, "*"])
    want.append(["ske_ingest_dense", "*", "*", 5, "*", "*" if sc.timed else None, "*", "*", "*", "*"])
    want += counting_calls(cl, sc, ndense) + [["ske_sync"]]
    if host:  # the host-decoded messages: count_packed
        want += counting_calls(cl, sc, len(host)) + [["ske_sync"]]
    got = cold(ctx)
    got[len(ingest_calls) + sc.timed][7] = "*"  # the dense capacity: the payload buffer's size
    assert got == want
    # the packed twin makes the same calls
    ctx.log.clear()
    blob = np.frombuffer(b"".join(MESSAGES), np.uint8)
    moffs = np.cumsum([0] + [len(m) for m in MESSAGES]).astype(np.uint32)
    sc.update_messages_packed("bf", blob, moffs)
    got = cold(ctx)
    ctx0.log.clear()
    cl0.ingest("bf", MESSAGES)  # ingest's calls the second time round
    assert [c[0] for c in got] == [c[0] for c in cold(ctx0)] + [c[0] for c in want[len(ingest_calls):]]
    # an empty batch makes no call
    ctx.log.clear()
    sc.update_messages("bf", [])
    assert ctx.log == []


def test_update_messages_without_filter_passes_no_valid(pkg):
    """BF.EXISTS of a missing key answers 0: the dense batch gets no valid column."""
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    sc = pkg.StudentCounts(cl)
    ctx.log.clear()
    sc.update_messages("bf:none", MESSAGES)
    got = cold(ctx)
    assert "ske_ingest_swipes" not in [c[0] for c in got]
    dense = [c for c in got if c[0] == "ske_ingest_dense"]
    assert len(dense) == 1 and dense[0][4] is None and dense[0][5] is None
    assert got[-1][0] == "ske_ingest_dense"  # the stub reports nothing dense: no add, no wait


@pytest.mark.parametrize("opts", [OPTIONS[0], OPTIONS[-1]])
def test_process_batch_with_and_without_counts(pkg, opts):
    batch = MESSAGES + [b"not json", json.dumps({"student_id": True, "lecture_id": "L1",
                                                 "timestamp": "2025-03-19T09:00:00"}).encode()]
    cfg = pkg.AttendanceConfig(bloom_filter_key="bf")
    cl0, ctx0 = make_client(pkg)
    p0 = pkg.AttendanceProcessor(cl0, cfg)
    ctx0.log.clear()
    rows0 = p0.process_batch(batch)
    plain = cold(ctx0)
    assert [c[0] for c in plain] == ["ske_hll_reserve", "ske_swipes"]  # what it makes today
    assert len(rows0) == 5 and (p0.acked, p0.nacked) == (5, 2)
    with pytest.raises(ValueError):
        p0.insights()

    cl, ctx = make_client(pkg)
    sc = pkg.StudentCounts(cl, **opts)
    p = pkg.AttendanceProcessor(cl, cfg, counts=sc)
    ctx.log.clear()
    rows = p.process_batch(batch)
    assert rows == rows0
    assert cold(ctx) == plain + counting_calls(cl, sc, 5) + [["ske_sync"]]  # the nacked ones are not counted
    ctx.log.clear()
    assert p.process_batch([b"junk"]) == [] and ctx.log == []
    titles = [i["title"] for i in p.insights(keys=["hll:unique:L1:2025-03-19"])]
    timed = (["Habitual Latecomers", "Attendance by Day"] if sc.timed else [])
    assert titles == timed + ["Lecture Attendance Rankings"] + \
        (["Most Consistent Attendees", "Invalid Attendance Attempts"] if sc._tracks else [])
    assert [i["title"] for i in p.insights()] == [i["title"] for i in sc.insights()]
