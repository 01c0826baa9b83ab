"""Row logs, the parts that need no GPU: the id rule and the lecture digest of
sketch_common.h (a stand-alone program, tests/native/rows_host.cpp, built with
``-Xarch_host -fsanitize=address,undefined``) against ``client_rows.parse_id``
and ``keyhash.murmur64a``; the error texts and constants; ``rows_oracle``
itself; and over a context stub: the facade's registry of named logs,
``FLUSHALL``, and what ``StudentCounts(records=...)`` enqueues and where."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOOM_SEED = 0xC6A4A7935BD1E995

ID_TEXTS = [b"", b"-", b"0", b"-0", b"00", b"01", b"+1", b" 1", b"1 ", b"1.0", b"1e3",
            b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809",
            b"12345678901234567890", b"1" * 32, b"12\xc3\xa9", b"\x80", b"7", b"-1", b"10", b"-10",
            b"2147483648", b"-2147483649", b"1234567890123456789", b"-123456789012345678", b"0x10", b"1-", b"--1"]
# what the rule says of each, written out: int64 or None
ID_WANT = [None, None, 0, None, None, None, None, None, None, None, None,
           2 ** 63 - 1, None, -2 ** 63, None,
           None, None, None, None, 7, -1, 10, -10,
           2147483648, -2147483649, 1234567890123456789, -123456789012345678, None, None, None]


@pytest.fixture(scope="module")
def rows_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "rows_host.cpp")
    exe = str(tmp_path_factory.mktemp("rows") / "rows_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "runtime error" not in out.stderr, out.stderr
        return out.stdout.splitlines()
    return run


def test_id_rule(pkg, rows_host):
    from rtsas_amd.client_rows import parse_id
    assert len(ID_TEXTS) == len(ID_WANT)
    lines = rows_host("id", *[t.hex() or "-" for t in ID_TEXTS])
    assert len(lines) == len(ID_TEXTS)
    for t, want, line in zip(ID_TEXTS, ID_WANT, lines):
        assert parse_id(t) == want, t
        assert line == ("refused" if want is None else f"ok {want}"), (t, line)
    # every length 1..20 of digits, both signs: the words' boundaries at 8 and 16
    texts = [(b"-" if neg else b"") + b"1234567890123456789"[:k] for neg in (0, 1) for k in range(1, 20)]
    for t, line in zip(texts, rows_host("id", *[t.hex() for t in texts])):
        assert line == f"ok {int(t)}" and parse_id(t) == int(t), t


def test_lecture_digest(pkg, rows_host, orc):
    from rtsas_amd.client_rows import lecture_digest
    from rtsas_amd.keyhash import murmur64a
    lectures = [bytes((37 * n + 11 * j + 1) & 0xFF for j in range(n)) for n in (0, 1, 7, 8, 9, 32, 33, 100)]
    lectures += [b"CS101-L01", "Ünï".encode()]
    lines = rows_host("digest", *[x.hex() or "-" for x in lectures])
    for x, line in zip(lectures, lines):
        want = murmur64a(x, BLOOM_SEED) or 1
        assert int(line) == want == lecture_digest(x), x
        assert murmur64a(x, BLOOM_SEED) == orc.murmur64a(x, BLOOM_SEED)
    assert lecture_digest(42) == lecture_digest("42") == lecture_digest(b"42")
    # the 0 -> 1 map: 0 names no partition
    assert rows_host("word", 0, 1, 2, 2 ** 64 - 1) == ["1", "1", "2", str(2 ** 64 - 1)]


def test_error_texts_and_constants(pkg):
    from rtsas_amd import _lib
    want = {-42: ("SKE_EROWSNOLOG", "ERR row log does not exist"),
            -43: ("SKE_EROWSEXISTS", "ERR row log already exists"),
            -44: ("SKE_EROWSCAP", "ERR row log capacity out of range"),
            -45: ("SKE_EROWSSPACE", "ERR row log selection does not fit the output")}
    txt = open(_lib.HEADER_PATH).read()
    for code, (name, text) in want.items():
        assert getattr(_lib, name) == code and _lib.strerror(code) == text
        assert re.search(rf"#define {name} {code}\b", txt), name
    assert _lib.strerror(-41) == "ERR unknown" and _lib.strerror(-46) == "ERR unknown"
    consts = {"SKE_MAX_ROWS": 8, "SKE_ROWS_MIN_LOG2": 8, "SKE_ROWS_MAX_LOG2": 28, "SKE_ROWS_BLOCK": 256,
              "SKE_ROWS_ROW_BYTES": 25}
    for name, value in consts.items():
        m = re.search(rf"#define {name} (\d+)", txt)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    assert _lib.SKE_ROWS_MAX_LOG2 <= min(28, _lib.SKE_SEEN_MAX_LOG2) and _lib.SKE_ROWS_MIN_LOG2 >= _lib.SKE_SEEN_MIN_LOG2
    assert C.sizeof(_lib.RowsInfo) == 48
    for name in ("ske_rows_append_packed_async", "ske_rows_append_spans_async", "ske_rows_append_fixed_async"):
        assert name in txt.split("---- stream capture")[1], name  # listed among the capturable calls


def test_argument_checks_before_any_device_call(pkg):
    lib = pkg.load_library()
    assert lib.ske_rows_init(None, 0, 10) == -1
    assert lib.ske_rows_free(None, 0) == -1 and lib.ske_rows_reset(None, 0) == -1
    assert lib.ske_rows_info(None, 0, None) == -1
    assert lib.ske_rows_append_packed_async(None, 0, None, None, None, None, None, None, None, 0) == -1
    assert lib.ske_rows_append_spans_async(None, 0, None, None, None, None, None, None, None, None, None, 0) == -1
    assert lib.ske_rows_append_fixed_async(None, 0, None, None, None, 8, None, None, None, 0) == -1
    assert lib.ske_rows_append(None, 0, None, None, None, None, None, None, None, 0, 0) == -1
    assert lib.ske_rows_read(None, 0, 0, 0, None, None, None, None) == -1
    assert lib.ske_rows_select(None, 0, None, 0, 0, 0, None, None, None, None, 0, None, None, 0) == -1


def test_oracle_rules(pkg):
    from rtsas_amd.client_rows import lecture_digest, rows_oracle
    # two lectures whose digests differ in the top bit
    names = [f"L{i}" for i in range(64)]
    lo = next(x for x in names if lecture_digest(x) < 2 ** 63)
    hi = next(x for x in names if lecture_digest(x) >= 2 ** 63)
    b1 = ([hi, lo, lo, lo, lo, hi], ["5", "-3", "2", "x", "2", "9"], [10, -7, 10, 11, 10, 12], [1, 1, 0, 1, 1, 0],
          [1, 1, 1, 1, 1, 0])
    b2 = ([lo, lo], ["-3", "2"], [-7, 20], None, None)
    o = rows_oracle([b1, b2])
    assert (o["taken"], o["refused_ids"], o["dropped"]) == (7, 1, 0)
    lec, ep, ids, valid = o["log"]
    assert ids.tolist() == [5, -3, 2, 2, -3, 2] and ep.tolist() == [10, -7, 10, 10, -7, 20]  # arrival order
    assert valid.tolist() == [1, 1, 0, 1, 0, 0]
    # digest-major (unsigned), then (epoch, id) signed; the last write wins, is_valid included
    d, ep, ids, valid = o["select"]
    assert d.tolist() == [lecture_digest(lo)] * 3 + [lecture_digest(hi)]
    assert list(zip(ep.tolist(), ids.tolist(), valid.tolist())) == [(-7, -3, 0), (10, 2, 1), (20, 2, 0), (10, 5, 1)]
    # one lecture, the half-open range
    for since, until, want in ((None, None, [-7, 10, 20]), (10, None, [10, 20]), (None, 10, [-7]), (10, 20, [10]),
                               (-7, -6, [-7]), (11, 20, [])):
        assert rows_oracle([b1, b2], lecture=lo, since=since, until=until)["select"][1].tolist() == want
    assert rows_oracle([b1, b2], lecture="none")["select"][0].size == 0
    # ids order numerically, not as text; negative before positive
    o = rows_oracle([(["a"] * 4, ["10", "9", "-1", "-10"], [0] * 4, None, None)], lecture="a")
    assert o["select"][2].tolist() == [-10, -1, 9, 10]
    # a capacity keeps the batch's prefix
    o = rows_oracle([b1, b2], capacity=4)
    assert o["log"][2].tolist() == [5, -3, 2, 2] and o["dropped"] == 2
    assert o["log"][0].size + o["refused_ids"] + o["dropped"] == o["taken"]


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    return cl, ctx


def test_registry_and_flushall(pkg, stub_client):
    cl, ctx = stub_client
    ctx.log.clear()
    rid = cl.rows_create("table", 10)
    assert ctx.log == [["ske_rows_init", rid, 10]] and cl.rows_rid("table") == rid
    with pytest.raises(pkg.ResponseError, match="ERR row log already exists"):
        cl.rows_create("table", 10)
    for bad in (7, 29):
        with pytest.raises(pkg.ResponseError, match="ERR row log capacity out of range"):
            cl.rows_create("other", bad)
    for call in (cl.rows_info, cl.rows_reset, cl.rows_select, cl.rows_read):
        with pytest.raises(pkg.ResponseError, match="ERR row log does not exist"):
            call("nope")
    other = cl.rows_create(b"other")
    assert other != rid and ctx.log[-1] == ["ske_rows_init", other, 22]
    assert cl.exists("table") == 0 and cl.type("table") == "none" and cl.delete("table") == 0  # no Redis key
    assert list(cl.scan_iter()) == ["bf"]
    assert cl.rows_drop("other") and not cl.rows_drop("other")
    assert cl.rows_create("again", 8) == other  # the id is free again
    for i in range(6):
        cl.rows_create(f"more{i}", 8)
    with pytest.raises(pkg.ResponseError, match="too many row logs"):
        cl.rows_create("ninth", 8)
    ctx.log.clear()
    cl.flushall()
    assert sorted(c[1] for c in ctx.log if c[0] == "ske_rows_free") == list(range(8))
    assert not cl._rows
    ctx.log.clear()
    cl.flushall()
    assert not [c for c in ctx.log if c[0].startswith("ske_rows")]


def rows_calls(ctx):
    return [c for c in ctx.log if c[0].startswith("ske_rows")]


MESSAGES = [json.dumps({"student_id": 10000 + i, "lecture_id": "L%d" % (i % 2),
                        "timestamp": "2025-03-19T09:00:0%d" % i}).encode() for i in range(5)]


def message_hooks(host):
    """The parse leaves every message to the device but those in ``host`` (the
    first n-byte read-back after ske_ingest_parse is the status column); the
    dense call reports the others."""
    state = {"armed": False}

    def parse(*a):
        state["armed"] = True

    def memcpy(dst, src, nbytes, kind):
        if state["armed"] and kind == 1 and nbytes == len(MESSAGES):
            state["armed"] = False
            st = (C.c_uint8 * nbytes).from_address(dst.value)
            for m in host:
                st[m] = 1

    def dense(msgs, cols, n, valid, epoch, out, cap, nd, nb):
        nd._obj.value, nb._obj.value = len(MESSAGES) - len(host), 5 * (len(MESSAGES) - len(host))
    return {"ske_ingest_parse": parse, "ske_memcpy": memcpy, "ske_ingest_dense": dense}


def test_no_records_no_rows_call(pkg):
    """a StudentCounts without ``records`` makes no ske_rows_* call on any entry point"""
    ctx = StubContext(pkg.load_library())
    ctx.hooks.update(message_hooks((1,)))
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    ids = np.frombuffer(b"12345678" * 3, np.uint8).reshape(3, 8)
    buf, offs = pkg.pack([1, 22, 333])
    for opts in (dict(), dict(dedup="seen", lecture_counts="lectures", day_profile="week")):
        sc = pkg.StudentCounts(cl, **opts)
        extra = dict(times=[1, 2, 3], lectures=["a", "b", "c"]) if opts else {}
        sc.update("bf", np.zeros(3, np.uint32), ids, **extra)
        sc.count_packed(buf, offs, [1, 0, 1], **extra)
        sc.update_messages("bf", MESSAGES)
        proc = pkg.AttendanceProcessor(cl, counts=sc)
        proc.process_batch(MESSAGES)
        assert "attendance_records" not in proc.get_attendance_stats("L0")
        assert not sc.keeps_records
        for call in (sc.records, sc.records_info, proc.fetch_attendance_data):
            with pytest.raises(ValueError):
                call()
        cl.flushall()
        cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    assert rows_calls(ctx) == [] and not cl._rows


def test_records_options(pkg, stub_client):
    cl, ctx = stub_client
    ctx.log.clear()
    sc = pkg.StudentCounts(cl, records="table", records_capacity_log2=12)
    assert ["ske_rows_init", cl.rows_rid("table"), 12] in ctx.log
    assert sc.keeps_records and sc.needs_times and sc.needs_lectures
    assert not sc.timed and not sc.counts_lectures and not sc.dedup  # their meaning is kept
    ctx.log.clear()
    pkg.StudentCounts(cl, "a2", "i2", records="table")  # an existing log is taken as it is
    assert not rows_calls(ctx)
    ids8 = np.frombuffer(b"12345678", np.uint8).reshape(1, 8)
    for call in (lambda: sc.update("bf", np.zeros(1, np.uint32), ids8),
                 lambda: sc.update("bf", np.zeros(1, np.uint32), ids8, times=[0]),
                 lambda: sc.count_packed(np.zeros(4, np.uint8), np.asarray([0, 4], np.uint32), [1], lectures=["L"])):
        with pytest.raises(ValueError):  # a row needs its time and its lecture
            call()
    # an id of the fixed form is 4 or 8 bytes: refused before any native call
    ctx.calls.clear()
    for width in (5, 1, 16):
        with pytest.raises(ValueError, match="4- or 8-byte"):
            sc.update("bf", np.zeros(2, np.uint32), np.zeros((2, width), np.uint8), times=[0, 1], lectures=["a", "b"])
    assert ctx.calls == []
    # without a tally the whole table has no lecture names
    proc = pkg.AttendanceProcessor(cl, counts=sc)
    with pytest.raises(ValueError, match="lecture_counts"):
        proc.fetch_attendance_data()


@pytest.mark.parametrize("dedup", [None, "seen"])
def test_update_and_count_packed_append_every_row(pkg, stub_client, dedup):
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, records="table", dedup=dedup)
    rid = cl.rows_rid("table")
    for width in (4, 8):
        ids = np.zeros((3, width), np.uint8)
        ctx.log.clear()
        sc.update("bf", np.zeros(3, np.uint32), ids, times=[1, 2, 3], lectures=["a", "b", "c"])
        names = [c[0] for c in ctx.log]
        assert rows_calls(ctx) == [["ske_rows_append_fixed_async", rid, "*", "*", "*", width, "*", "*", None, 3]]
        at = names.index("ske_rows_append_fixed_async")
        assert names.index("ske_swipes_fixed") < at  # K1's answers are the valid column
        if dedup:  # every row, before the repeats leave
            assert at < names.index("ske_seen_add_async")
    buf, offs = pkg.pack([1, 22, 333])
    ctx.log.clear()
    sc.count_packed(buf, offs, [1, 0, 1], times=[1, 2, 3], lectures=["a", "b", "c"])
    names = [c[0] for c in ctx.log]
    assert rows_calls(ctx) == [["ske_rows_append_packed_async", rid, "*", "*", "*", "*", "*", "*", None, 3]]
    if dedup:
        assert names.index("ske_rows_append_packed_async") < names.index("ske_seen_add_async")
    assert names.index("ske_rows_append_packed_async") < names.index("ske_cms_add_packed_async")


@pytest.mark.parametrize("host", [(), (1, 3)])
@pytest.mark.parametrize("dedup", [None, "seen"])
def test_update_messages_appends_from_the_parse_columns(pkg, host, dedup):
    """the spans append reads the parse's own status, before the dedup calls
    replace it by the set's answers; host-decoded messages arrive through count_packed"""
    seqs = []
    for records in (None, "table"):
        ctx = StubContext(pkg.load_library())
        ctx.hooks.update(message_hooks(host))
        status_ptrs = []
        ctx.hooks["ske_ingest_times"] = lambda msgs, cols, n, ep: status_ptrs.append(cols._obj.status)
        cl = pkg.SketchClient(decode_responses=True, context=ctx)
        cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
        sc = pkg.StudentCounts(cl, records=records, dedup=dedup)
        ctx.log.clear()
        valid, status = sc.update_messages("bf", MESSAGES)
        assert status.tolist() == [1 if m in host else 0 for m in range(5)]
        seqs.append((cl, [c for c in ctx.log if c[0] not in ("ske_memcpy", "ske_device_alloc", "ske_device_free")],
                     status_ptrs))
    (_, off, _), (cl, on, status_ptrs) = seqs
    rid = cl.rows_rid("table")
    spans = [c for c in on if c[0] == "ske_rows_append_spans_async"]
    assert len(spans) == 1 and spans[0][1] == rid and spans[0][-1] == 5
    assert spans[0][7] == status_ptrs[0] and spans[0][9] == "*" and spans[0][10] is None  # parse status, K1's valid
    names = [c[0] for c in on]
    at = names.index("ske_rows_append_spans_async")
    assert names.index("ske_ingest_times") < at < names.index("ske_ingest_dense")
    if dedup:
        assert at < names.index("ske_seen_fold_spans_async") and at < names.index("ske_seen_add_async")
    packed = [c for c in on if c[0] == "ske_rows_append_packed_async"]
    assert [c[-1] for c in packed] == ([len(host)] if host else [])
    if dedup:  # without dedup the times call itself is new: records asks for it
        rest = [c[0] for c in on if not c[0].startswith("ske_rows")]
        assert rest == [c[0] for c in off]  # every other call is the one made today


def test_processor_readers(pkg, stub_client):
    from rtsas_amd.client_rows import lecture_digest
    from datetime import datetime
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, records="table", lecture_counts="lectures")
    proc = pkg.AttendanceProcessor(cl, counts=sc)
    rows = [(lecture_digest("L1"), 1742374800, 7, 1), (lecture_digest("L1"), 1742374801, -2, 0)]

    def select(rid, lec, llen, since, until, o_lec, o_ep, o_id, o_valid, cap, n_out, complete, mem):
        n_out._obj.value, complete._obj.value = len(rows), 1
        if cap < len(rows):
            return
        for ptr, typ, col in ((o_lec, C.c_uint64, 0), (o_ep, C.c_int64, 1), (o_id, C.c_int64, 2),
                              (o_valid, C.c_uint8, 3)):
            arr = (typ * len(rows)).from_address(ptr.value)
            for j, r in enumerate(rows):
                arr[j] = r[col]

    ctx.hooks["ske_rows_select"] = select
    stats = proc.get_attendance_stats("L1")
    assert stats["attendance_records"] == [{"student_id": 7, "timestamp": datetime(2025, 3, 19, 9, 0, 0)},
                                           {"student_id": -2, "timestamp": datetime(2025, 3, 19, 9, 0, 1)}]
    assert [c for c in ctx.calls if c == "ske_rows_select"] == ["ske_rows_select"] * 2  # the count, then the rows
    rec = sc.records("L1")
    assert rec["student_id"].tolist() == [7, -2] and rec["is_valid"].tolist() == [1, 0] and rec["complete"]
    assert ctx.calls.count("ske_rows_select") == 3  # the grown buffer is reused
