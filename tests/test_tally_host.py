"""Tallies, the parts that need no GPU: the digest, probe start and list order
of sketch_common.h (a stand-alone program, tests/native/tally_host.cpp, which
can also be built by hand with ``hipcc -O1 -g -std=c++17 -Xarch_host
-fsanitize=address,undefined tests/native/tally_host.cpp -o tally_host``)
against a Python restatement pinned by the oracle's MurmurHash64A; the error
texts and constants; the argument checks that come before any device call; and
over a context stub: the facade's registry of named tallies, ``FLUSHALL``,
``StudentCounts``' native call sequence with ``lecture_counts`` on, off and
combined with every other option, the ``lectures`` ValueErrors and
``AttendanceProcessor.insights``' three ``rank_by`` cases.  With pandas, the
reference's own expression over the rows the GPU tests restate in plain Python."""
import ctypes as C
import json
import os
import re
import subprocess
from collections import Counter

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOOM_SEED = 0xC6A4A7935BD1E995
HOT = ("ske_device_alloc", "ske_memcpy", "ske_device_free")


def digest(orc, key: bytes) -> int:
    return orc.murmur64a(key, BLOOM_SEED) or 1


@pytest.fixture(scope="module")
def tally_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "tally_host.cpp")
    exe = str(tmp_path_factory.mktemp("tally") / "tally_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        return out.stdout.splitlines()
    return run


def test_digest_and_start(tally_host, orc):
    keys = [b"", bytes(1), bytes(8), bytes(32), b"A", b"A\0", b"CS101-L01", b"\xff" * 32, b"LECTURE_20250317"]
    keys += [bytes((7 * i + j) & 0xFF for j in range(n)) for n in range(1, 33) for i in (1, 29)]
    assert digest(orc, bytes(1)) == 1  # the seed is the multiplier: one zero byte hashes to 0, mapped to 1
    assert digest(orc, b"A") != digest(orc, b"A\0")  # the length takes part
    for log2 in (8, 16, 24):
        lines = tally_host("digest", log2, *[k.hex() or "-" for k in keys])
        assert len(lines) == len(keys)
        for k, line in zip(keys, lines):
            d = digest(orc, k)
            assert line == f"{k.hex() or '-'} {d} {d & ((1 << log2) - 1)}", (k, line)
    assert tally_host("digest", 8, "00") == ["00 1 1"]


def test_list_order(tally_host):
    rng = np.random.default_rng(3)
    keys = [b"", b"\0", b"A", b"A\0", b"A\0\0", b"A\0B", b"A\x01", b"AB", b"B", b"\xff", bytes(32), bytes(31) + b"\x01",
            b"x" * 32, b"x" * 31, b"CS101-L01", b"CS101-L02", b"CS101-L1"]
    rows = [(int(rng.integers(1, 4)), k) for k in keys] + [(2 ** 63, b"big"), (2 ** 64 - 1, b"bigger")]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    want = sorted(rows, key=lambda r: (-r[0], r[1]))
    got = tally_host("order", *[f"{c}:{k.hex() or '-'}" for c, k in rows])
    assert got == [f"{c}:{k.hex() or '-'}" for c, k in want]
    assert [k for _, k in want[:2]] == [b"bigger", b"big"]  # counts compare as unsigned 64-bit
    same = [k for c, k in want if c == 1]
    assert len(same) > 3 and same == sorted(same)  # a prefix before its extensions


def test_error_texts_and_constants(pkg):
    from rtsas_amd import _lib
    want = {-32: ("SKE_ETALLYNOSET", "ERR tally does not exist"), -33: ("SKE_ETALLYEXISTS", "ERR tally already exists"),
            -34: ("SKE_ETALLYCAP", "ERR tally capacity out of range"),
            -35: ("SKE_ETALLYSPACE", "ERR tally list does not fit the output")}
    txt = open(_lib.HEADER_PATH).read()
    for code, (name, text) in want.items():
        assert getattr(_lib, name) == code and _lib.strerror(code) == text
        assert re.search(rf"#define {name} {code}\b", txt), name
    assert _lib.strerror(-28) == "ERR unknown" and _lib.strerror(-31) == "ERR unknown"
    assert _lib.strerror(-36) == "ERR unknown"
    assert not re.search(r"#define SKE_\w+ -(28|31)\b", txt)
    consts = {"SKE_MAX_TALLY": 256, "SKE_TALLY_KEY_BYTES": 32, "SKE_TALLY_MIN_LOG2": 8, "SKE_TALLY_MAX_LOG2": 24,
              "SKE_TALLY_MAX_PROBES": 128, "SKE_TALLY_LOAD_DEN": 2, "SKE_TALLY_MAX_TOP": 16}
    for name, value in consts.items():
        m = re.search(rf"#define {name} (\d+)", txt)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    assert C.sizeof(_lib.TallyInfo) == 48


def test_null_context_is_rejected(pkg):
    lib = pkg.load_library()
    n, done = C.c_uint64(), C.c_int()
    assert lib.ske_tally_init(None, 0, 10) == -1
    assert lib.ske_tally_free(None, 0) == -1
    assert lib.ske_tally_reset(None, 0) == -1
    assert lib.ske_tally_info(None, 0, None) == -1
    assert lib.ske_tally_add_packed_async(None, 0, None, None, 0, None) == -1
    assert lib.ske_tally_add_fixed_async(None, 0, None, 8, 0, None) == -1
    assert lib.ske_tally_add_spans_async(None, 0, None, None, None, 0, None, None) == -1
    assert lib.ske_tally_add(None, 0, None, None, 0, None, 0) == -1
    assert lib.ske_tally_query(None, 0, None, None, 0, None, None, 0) == -1
    assert lib.ske_tally_list(None, 0, 0, None, None, None, None, 0, C.byref(n), C.byref(done)) == -1
    assert lib.ske_tally_top(None, 0, 3, 0, *([None] * 8), C.byref(n), C.byref(done)) == -1
    assert lib.ske_tally_import(None, 0, None, None, None, None, 0) == -1


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    return cl, ctx


def cold(ctx):
    return [c for c in ctx.log if c[0] not in HOT]


def test_registry(pkg, stub_client):
    cl, ctx = stub_client
    ex = cl.execute_command
    ctx.log.clear()
    a, b = cl.tally_create("lectures"), cl.tally_create(b"gates", 10)
    assert a != b and ctx.log == [["ske_tally_init", a, 16], ["ske_tally_init", b, 10]]
    with pytest.raises(pkg.ResponseError, match="ERR tally already exists"):
        cl.tally_create("lectures")
    for bad in (7, 25):
        with pytest.raises(pkg.ResponseError, match="ERR tally capacity out of range"):
            cl.tally_create("x", bad)
    for call in (cl.tally_info, cl.tally_reset, cl.tally_list, cl.tally_top, lambda n: cl.tally_add(n, ["a"]),
                 lambda n: cl.tally_query(n, ["a"]), lambda n: cl.tally_import(n, [], [], [])):
        with pytest.raises(pkg.ResponseError, match="ERR tally does not exist"):
            call("nosuch")
    # no key kind: the generic key commands do not see a tally
    assert ex("TYPE", "lectures") == "none" and ex("EXISTS", "lectures") == 0 and list(cl.scan_iter()) == ["bf"]
    ctx.calls.clear()
    assert ex("DEL", "lectures") == 0 and ctx.calls == []
    # the host add: encoded as redis-py would, one synchronous native call
    ctx.log.clear()
    cl.tally_add("lectures", ["CS101", 7, 2.5, b"raw"], valid=[1, 0, 1, 1])
    assert ctx.log == [["ske_tally_add", a, "*", "*", 4, "*", 0]]
    ctx.log.clear()
    cl.tally_add("lectures", [])
    assert ctx.log == []
    with pytest.raises(ValueError):
        cl.tally_add("lectures", ["a", "b"], valid=[1])
    ev, va = cl.tally_query("lectures", ["CS101", "x"])
    assert ev.tolist() == [0, 0] and ev.dtype == np.uint64 and va.dtype == np.uint64
    keys, ev, va, complete = cl.tally_list("lectures")
    assert keys == [] and complete is True
    head, tail, complete = cl.tally_top("lectures", 3, by="valid")
    assert head[0] == [] and tail[0] == [] and ctx.log[-1][:4] == ["ske_tally_top", a, 3, 1]
    for bad in (dict(k=0), dict(k=17), dict(by="unique")):
        with pytest.raises(ValueError):
            cl.tally_top("lectures", **bad)
    with pytest.raises(ValueError):
        cl.tally_import("lectures", [b"x" * 33], [1], [0])
    ctx.log.clear()
    cl.tally_import("lectures", ["CS101", b"B"], [3, 2], [1, 0])
    assert ctx.log == [["ske_tally_import", a, "*", "*", "*", "*", 2]]
    # free and recycle
    ctx.log.clear()
    assert cl.tally_free("lectures") is True and cl.tally_free("lectures") is False
    assert ctx.log == [["ske_tally_free", a]]
    assert cl.tally_create("again") == a
    ctx.log.clear()
    assert ex("FLUSHALL") == "OK"
    assert sorted(c[0] for c in ctx.log) == ["ske_bf_free", "ske_tally_free", "ske_tally_free"]
    assert cl._tally == {} and len(cl._tally_free_ids) == 256
    ctx.calls.clear()
    assert ex("FLUSHALL") == "OK" and ctx.calls == []
    for i in range(256):
        cl.tally_create(f"t{i}")
    with pytest.raises(pkg.ResponseError, match="too many tallies"):
        cl.tally_create("one more")


OPTIONS = [
    dict(),
    dict(day_profile="week"),
    dict(late_key="cms:late", track_late=2),
    dict(track_attended=3, track_invalid=2, capacity_log2=12),
    dict(late_key="cms:late", track_late=3, day_profile="week", track_attended=3, track_invalid=2, capacity_log2=12),
]


@pytest.mark.parametrize("opts", OPTIONS)
def test_update_call_sequence(pkg, stub_client, opts):
    """the option adds one enqueue before the one wait, and nothing when off"""
    cl, ctx = stub_client
    ids = np.full((4, 5), 49, np.uint8)
    slots = np.zeros(4, np.uint32)
    off = pkg.StudentCounts(cl, "a0", "i0", **{k: (v + ":0" if isinstance(v, str) else v) for k, v in opts.items()})
    ctx.log.clear()
    on = pkg.StudentCounts(cl, lecture_counts="lectures", lecture_capacity_log2=9, **opts)
    made = [c for c in ctx.log if c[0] == "ske_tally_init"]
    assert made == [["ske_tally_init", cl.tally_tid("lectures"), 9]] and not off.counts_lectures and on.counts_lectures
    times = np.asarray([0, 32399, 32400, -1], np.int64) if on.timed else None
    ctx.log.clear()
    off.update("bf", slots, ids, times)
    base = [c[0] for c in cold(ctx)]
    assert base[-1] == "ske_sync" and not any("tally" in c for c in base)
    ctx.log.clear()
    on.update("bf", slots, ids, times, lectures=["L1", "L2", 3.5, b"L1"])
    got = cold(ctx)
    assert [c[0] for c in got] == base[:-1] + ["ske_tally_add_packed_async", "ske_sync"]
    assert got[-2] == ["ske_tally_add_packed_async", cl.tally_tid("lectures"), "*", "*", 4, "*"]
    ups = [c[3] for c in ctx.log if c[0] == "ske_memcpy" and c[4] == 0]
    assert ups[-2:] == [len(b"L1L23.5L1"), 20]  # the lecture bytes and their five offsets, after the rest
    # the packed form of the argument, and count_packed
    buf, offs = pkg.pack(["L1", "L2", "3.5", "L1"])
    ctx.log.clear()
    on.update("bf", slots, ids, times, lectures=(buf, offs))
    assert cold(ctx) == got
    ibuf, ioffs = pkg.pack([10001, "", b"abc", 7])
    ctx.log.clear()
    off.count_packed(ibuf, ioffs, [1, 0, 1, 1], times)
    base = cold(ctx)
    ctx.log.clear()
    on.count_packed(ibuf, ioffs, [1, 0, 1, 1], times, lectures=["L1", "L2", 3.5, b"L1"])
    got = cold(ctx)
    assert [c[0] for c in got] == [c[0] for c in base[:-1]] + ["ske_tally_add_packed_async", "ske_sync"]
    assert got[-2] == ["ske_tally_add_packed_async", cl.tally_tid("lectures"), "*", "*", 4, "*"]
    # an existing tally is used as it is
    ctx.log.clear()
    pkg.StudentCounts(cl, "a5", "i5", lecture_counts="lectures")
    assert not [c for c in ctx.log if c[0] == "ske_tally_init"]
    titles = [i["title"] for i in on.insights()]
    at = sum(t in ("Habitual Latecomers", "Attendance by Day") for t in titles)
    assert titles[at] == "Lecture Attendance Rankings" and titles[:at] + titles[at + 1:] == \
        [i["title"] for i in off.insights()]
    assert on.insights()[at] == {"title": "Lecture Attendance Rankings", "complete": True,
                                 "description": "Most and least attended lectures",
                                 "data": {"most_attended": {}, "least_attended": {}}}


def test_lectures_value_errors(pkg, stub_client):
    cl, ctx = stub_client
    ids = np.full((4, 5), 49, np.uint8)
    slots = np.zeros(4, np.uint32)
    plain = pkg.StudentCounts(cl)
    lec = pkg.StudentCounts(cl, "a2", "i2", lecture_counts="lectures")
    buf, offs = pkg.pack([1, 22, 333, 4444])
    ctx.calls.clear()
    with pytest.raises(ValueError):
        plain.update("bf", slots, ids, lectures=["a"] * 4)  # lectures without a use for them
    with pytest.raises(ValueError):
        plain.count_packed(buf, offs, [1, 1, 0, 0], lectures=["a"] * 4)
    with pytest.raises(ValueError):
        lec.update("bf", slots, ids)  # lectures missing
    with pytest.raises(ValueError):
        lec.count_packed(buf, offs, [1, 1, 0, 0])
    for n in (3, 5):
        with pytest.raises(ValueError):
            lec.update("bf", slots, ids, lectures=["a"] * n)
        with pytest.raises(ValueError):
            lec.count_packed(buf, offs, [1, 1, 0, 0], lectures=pkg.pack(["a"] * n))
    assert ctx.calls == []  # refused before any native call
    for call in (plain.lecture_rankings, lambda: plain.lecture_events(["a"])):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        lec.lecture_rankings(by="unique")
    with pytest.raises(ValueError):
        lec.lecture_rankings(k=17)


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


@pytest.mark.parametrize("host", [(), (1, 3)])
@pytest.mark.parametrize("opts", [OPTIONS[0], OPTIONS[-1]])
def test_update_messages_call_sequence(pkg, opts, host):
    """the spans add reads the parse columns in place, beside the other adds and
    before the one wait; the host-decoded messages carry their lectures to count_packed"""
    seqs = []
    for lecture_counts in (None, "lectures"):
        ctx = StubContext(pkg.load_library())
        ctx.hooks.update(message_hooks(host))
        cl = pkg.SketchClient(decode_responses=True, context=ctx)
        cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
        sc = pkg.StudentCounts(cl, lecture_counts=lecture_counts, **opts)
        ctx.log.clear()
        valid, status = sc.update_messages("bf", MESSAGES)
        assert status.tolist() == [1 if m in host else 0 for m in range(5)]
        seqs.append((cl, cold(ctx)))
    (_, off), (cl, on) = seqs
    tid = cl.tally_tid("lectures")
    spans = [c for c in on if c[0] == "ske_tally_add_spans_async"]
    assert len(spans) == 1 and spans[0][1] == tid and spans[0][5] == 5 and spans[0][7] == "*"  # n; masked by BF.EXISTS
    at = on.index(spans[0])
    assert on[at + 1] == ["ske_sync"] and on[at - 1][0] != "ske_sync"
    rest = on[:at] + on[at + 1:]
    if host:
        assert rest[-2] == ["ske_tally_add_packed_async", tid, "*", "*", len(host), "*"] and rest[-1] == ["ske_sync"]
        rest = rest[:-2] + rest[-1:]
    assert [c[0] for c in rest] == [c[0] for c in off]  # every other call is the one made today


def test_update_messages_without_filter_passes_no_mask(pkg):
    ctx = StubContext(pkg.load_library())
    ctx.hooks.update(message_hooks(()))
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    sc = pkg.StudentCounts(cl, lecture_counts="lectures")
    ctx.log.clear()
    sc.update_messages("bf:none", MESSAGES)
    spans = [c for c in cold(ctx) if c[0] == "ske_tally_add_spans_async"]
    assert len(spans) == 1 and spans[0][7] is None  # BF.EXISTS of a missing key answers 0: nothing is valid


@pytest.mark.parametrize("opts", [OPTIONS[0], OPTIONS[-1]])
def test_processor_rank_by(pkg, stub_client, opts):
    cl, ctx = stub_client
    cfg = pkg.AttendanceConfig(bloom_filter_key="bf")
    batch = MESSAGES + [b"not json"]
    off = pkg.AttendanceProcessor(cl, cfg, counts=pkg.StudentCounts(cl, "a0", "i0", **{
        k: (v + ":0" if isinstance(v, str) else v) for k, v in opts.items()}))
    on = pkg.AttendanceProcessor(cl, cfg, counts=pkg.StudentCounts(cl, lecture_counts="lectures", **opts))
    ctx.log.clear()
    rows0 = off.process_batch(batch)
    base = [c for c in cold(ctx) if c[0] != "ske_hll_reserve"]  # the first batch makes the HLL keys
    ctx.log.clear()
    rows = on.process_batch(batch)
    got = cold(ctx)
    assert rows == rows0 and len(rows) == 5
    assert [c[0] for c in got] == [c[0] for c in base[:-1]] + ["ske_tally_add_packed_async", "ske_sync"]
    assert got[-2][4] == 5  # the acknowledged rows' lectures, the nacked one's not
    keys = ["hll:unique:L1:2025-03-19"]
    cl.pfadd(keys[0], "10001")  # the stub answers no swipe valid: make the key the PFCOUNT form ranks
    title = "Lecture Attendance Rankings"

    def entries(ins):
        return [i for i in ins if i["title"] == title]

    # keys given, rank_by None or "unique": the PFCOUNT entry exactly as today
    ctx.log.clear()
    uniq = on.insights(keys=keys)
    assert "ske_hll_pfcount_each" in ctx.calls and not [c for c in ctx.log if c[0] == "ske_tally_top"]
    assert uniq == on.insights(keys=keys, rank_by="unique") and len(entries(uniq)) == 1
    assert entries(uniq) == entries(off.insights(keys=keys)) and "complete" not in entries(uniq)[0]
    # rank_by="events", or no keys with a tally on: the tally's entry, never both
    for kw in (dict(), dict(rank_by="events"), dict(keys=keys, rank_by="events")):
        ctx.log.clear()
        ctx.calls.clear()
        ins = on.insights(k=2, **kw)
        tops = [c for c in ctx.log if c[0] == "ske_tally_top"]
        assert len(tops) == 1 and tops[0][1:4] == [cl.tally_tid("lectures"), 2, 0]
        assert "ske_hll_pfcount_each" not in ctx.calls
        assert len(entries(ins)) == 1 and entries(ins)[0]["complete"] is True
        assert [i["title"] for i in ins] == [i["title"] for i in uniq]  # at the reference's place
    assert entries(off.insights()) == []
    for bad in (dict(rank_by="rows"), dict(rank_by="unique")):
        with pytest.raises(ValueError):
            on.insights(**bad)
    with pytest.raises(ValueError):
        off.insights(rank_by="events")
    # get_attendance_stats: the record counts only with a tally
    assert set(off.get_attendance_stats("L1")) == {"unique_attendees"}
    assert on.get_attendance_stats("L1") == {"unique_attendees": 0, "attendance_record_count": 0,
                                             "invalid_record_count": 0}
    assert on.get_attendance_stats("L1", day="2025-03-19")["attendance_record_count"] == 0


def test_reference_expression_agrees_with_the_restatement():
    """df.groupby('lecture_id').size().sort_values(ascending=False), .head(3) /
    .tail(3) (attendance_analysis.py:87-97) over rows whose counts are untied
    at both cuts -- pandas leaves ties in quicksort order -- is the plain-Python
    restatement the GPU tests trust"""
    pd = pytest.importorskip("pandas")
    rng = np.random.default_rng(12)
    lectures = ["CS%d-L%02d" % (100 + j, j) for j in range(12)]
    sizes = [701, 356, 187, 159, 137, 92, 81, 70, 59, 56, 52, 23]
    rows = [lec for lec, c in zip(lectures, sizes) for _ in range(c)]
    rows = [rows[j] for j in rng.permutation(len(rows))]
    df = pd.DataFrame({"lecture_id": rows, "is_valid": rng.random(len(rows)) < 0.85})
    ranked = df.groupby("lecture_id").size().sort_values(ascending=False)
    counts = Counter(rows)
    full = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0].encode()))
    assert ranked.head(3).to_dict() == dict(full[:3]) and list(ranked.head(3).index) == [k for k, _ in full[:3]]
    assert ranked.tail(3).to_dict() == dict(full[-3:]) and list(ranked.tail(3).index) == [k for k, _ in full[-3:]]
