"""Time profiles, the parts that need no GPU: the weekday / hour / second-of-day
arithmetic of sketch_common.h (a stand-alone program, tests/native/tp_host.cpp,
which can also be built by hand with ``-Xarch_host
-fsanitize=address,undefined``) against Python's datetime and numpy floor
arithmetic, the error texts and constants, the argument checks that come before
any device call, and over a context stub: the facade's registry of named
profiles, ``StudentCounts.update``'s native call sequence with each combination
of the time options, its ValueErrors, and ``epoch_seconds``."""
import ctypes as C
import os
import re
import subprocess
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
DT_LO, DT_HI = -62135596800, 253402300799  # 0001-01-01T00:00:00 .. 9999-12-31T23:59:59
# epoch -> (dow, hour, sod); Monday = 0
PINS = {-1: (2, 23, 86399), 0: (3, 0, 0), 1742374799: (2, 8, 32399), 1742374800: (2, 9, 32400),
        DT_LO: (0, 0, 0), DT_HI: (4, 23, 86399)}


@pytest.fixture(scope="module")
def tp_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "tp_host.cpp")
    exe = str(tmp_path_factory.mktemp("tp") / "tp_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)

    def run(epochs):
        out = subprocess.run([exe] + [str(int(e)) for e in epochs], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        rows = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(epochs)
        return rows
    return run


def by_datetime(e):
    t = datetime(1970, 1, 1) + timedelta(seconds=int(e))
    return t.weekday(), t.hour, t.hour * 3600 + t.minute * 60 + t.second


def test_pins(tp_host):
    got = tp_host(list(PINS) + [INT64_MIN])
    for (e, want), row in zip(PINS.items(), got):
        assert by_datetime(e) == want, e  # the pins themselves
        assert row == want + (want[0] * 24 + want[1],), (e, row)
    assert got[-1][0] == 6


def test_against_datetime_and_floor_arithmetic(tp_host):
    rng = np.random.default_rng(168)
    epochs = [int(e) for e in rng.integers(DT_LO, DT_HI, 1000, endpoint=True)]
    for e, row in zip(epochs, tp_host(epochs)):
        dow, hour, sod = by_datetime(e)
        assert row == (dow, hour, sod, dow * 24 + hour), (e, row)
    # the int64 extremes, the day boundaries around zero and seeded values of the whole range
    wide = np.concatenate([np.asarray([INT64_MIN, INT64_MAX, INT64_MIN + 1, -86401, -86400, -86399, 86399, 86400]),
                           rng.integers(INT64_MIN, INT64_MAX, 1000, endpoint=True)]).astype(np.int64)
    day, sod = wide // 86400, wide % 86400
    dow, hour = (day + 3) % 7, sod // 3600
    got = np.asarray(tp_host(wide))
    assert np.array_equal(got, np.stack([dow, hour, sod, dow * 24 + hour], axis=1))


def test_error_texts_and_constants(pkg):
    from rtsas_amd import _lib
    assert (_lib.SKE_ETPNOSET, _lib.SKE_ETPEXISTS) == (-29, -30)
    assert _lib.strerror(-29) == "ERR time profile does not exist"
    assert _lib.strerror(-30) == "ERR time profile already exists"
    assert _lib.strerror(-28) == "ERR unknown" and _lib.strerror(-31) == "ERR unknown"
    txt = open(_lib.HEADER_PATH).read()
    for name in ("SKE_MAX_TP", "SKE_TP_BINS", "SKE_ETPNOSET", "SKE_ETPEXISTS"):
        m = re.search(rf"#define {name} (-?\d+)", txt)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert (_lib.SKE_MAX_TP, _lib.SKE_TP_BINS) == (256, 168)
    assert not re.search(r"#define SKE_\w+ -28\b", txt)


def test_null_context_is_rejected(pkg):
    lib = pkg.load_library()
    buf = (C.c_uint64 * 168)()
    assert lib.ske_tp_init(None, 0) == -1
    assert lib.ske_tp_free(None, 0) == -1
    assert lib.ske_tp_reset(None, 0) == -1
    assert lib.ske_tp_read(None, 0, buf) == -1
    assert lib.ske_tp_import(None, 0, buf) == -1
    assert lib.ske_tp_add_async(None, 0, None, 0, None, 1, 32400, None) == -1


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def test_registry(pkg, stub_client):
    cl, ctx = stub_client
    ex = cl.execute_command
    ex("CMS.INITBYDIM", "c", 100, 5)
    a, b = cl.tp_create("week"), cl.tp_create(b"week:2")
    assert a != b and ctx.log[-2:] == [["ske_tp_init", a], ["ske_tp_init", b]]
    with pytest.raises(pkg.ResponseError, match="ERR time profile already exists"):
        cl.tp_create("week")
    for call in (cl.tp_counts, cl.tp_reset, lambda n: cl.tp_add(n, [0])):
        with pytest.raises(pkg.ResponseError, match="ERR time profile does not exist"):
            call("nosuch")
    assert cl.tp_counts("week").shape == (7, 24) and cl.tp_counts("week").dtype == np.uint64
    # no key kind: the generic key commands do not see a profile
    assert ex("TYPE", "week") == "none" and ex("EXISTS", "week") == 0 and list(cl.scan_iter()) == ["c"]
    ctx.calls.clear()
    assert ex("DEL", "week") == 0 and ctx.calls == []
    # the host-array add: upload, one enqueue (no late bytes), one wait
    ctx.log.clear()
    cl.tp_add("week", [datetime(2025, 3, 19, 9)], mask=[1], want=1)
    got = [c for c in ctx.log if c[0] not in ("ske_device_alloc", "ske_memcpy", "ske_device_free")]
    assert got == [["ske_tp_add_async", a, "*", 1, "*", 1, 86400, None], ["ske_sync"]]
    with pytest.raises(ValueError):
        cl.tp_add("week", [0, 1], mask=[1])
    # free and recycle
    ctx.log.clear()
    assert cl.tp_free("week") is True and cl.tp_free("week") is False
    assert ctx.log == [["ske_tp_free", a]]
    assert cl.tp_create("again") == a
    ctx.log.clear()
    assert ex("FLUSHALL") == "OK"
    assert sorted(c[0] for c in ctx.log) == ["ske_cms_free", "ske_tp_free", "ske_tp_free"]
    assert cl._tp == {} and len(cl._tp_free_ids) == 256
    ctx.calls.clear()
    assert ex("FLUSHALL") == "OK" and ctx.calls == []
    # all 256 ids, then none
    for i in range(256):
        cl.tp_create(f"p{i}")
    with pytest.raises(pkg.ResponseError, match="too many time profiles"):
        cl.tp_create("one more")


HOT = ("ske_device_alloc", "ske_memcpy", "ske_device_free")
BASE = ["ske_swipes_fixed", "ske_cms_add_fixed_async", "ske_cms_add_fixed_async"]


@pytest.mark.parametrize("late_key,track_late,day_profile,tracked", [
    (None, None, None, False),
    (None, None, "week", False),
    ("cms:late", None, None, False),
    ("cms:late", 2, None, False),
    ("cms:late", None, "week", True),
    ("cms:late", 3, "week", True),
])
def test_update_call_sequence(pkg, stub_client, late_key, track_late, day_profile, tracked):
    cl, ctx = stub_client
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    ids = np.full((4, 5), 49, np.uint8)
    slots = np.zeros(4, np.uint32)
    times = np.asarray([0, 32399, 32400, -1], np.int64)
    extra = dict(track_attended=3, track_invalid=2, capacity_log2=12) if tracked else {}
    ctx.log.clear()
    sc = pkg.StudentCounts(cl, late_key=late_key, late_from=8 * 3600, track_late=track_late,
                           day_profile=day_profile, **extra)
    made = [c[0] for c in ctx.log]
    timed = late_key is not None or day_profile is not None
    assert made.count("ske_cms_init") == 2 + (late_key is not None)
    assert made.count("ske_tp_init") == (1 if timed else 0)
    assert made.count("ske_hh_init") == 2 * tracked + (track_late is not None)
    assert set(cl._tp) == ({b"week"} if day_profile else {b"tp:cms:late"} if late_key else set())
    ctx.log.clear()
    sc.update("bf", slots, ids, times if timed else None)
    got = [c for c in ctx.log if c[0] not in HOT]
    want = list(BASE)
    if timed:
        want.append("ske_tp_add_async")
    if late_key:
        want.append("ske_cms_add_fixed_async")
    want += ["ske_hh_track_fixed_async"] * (2 * tracked + (track_late is not None)) + ["ske_sync"]
    assert [c[0] for c in got] == want
    if timed:
        tp = got[3]  # tid, epoch, n, mask, want, late_from, late
        assert tp[1:] == [cl._tp[sc._profile], "*", 4, None, 1, 8 * 3600, "*" if late_key else None]
    if late_key:
        assert got[4][1:] == [cl.cms_cid("cms:late"), "*", 5, 4, None, "*", 1]  # masked by the late bytes
    if track_late is not None:
        assert got[-2][5:] == [4, "*", 1, track_late]  # n, mask, want, threshold
    titles = [i["title"] for i in sc.insights()]
    want_titles = (["Habitual Latecomers"] if track_late is not None else []) + \
                  (["Attendance by Day"] if day_profile else []) + \
                  (["Most Consistent Attendees", "Invalid Attendance Attempts"] if tracked else [])
    assert titles == want_titles


def test_update_value_errors(pkg, stub_client):
    cl, ctx = stub_client
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    ids = np.full((4, 5), 49, np.uint8)
    slots = np.zeros(4, np.uint32)
    plain = pkg.StudentCounts(cl)
    timed = pkg.StudentCounts(cl, "a2", "i2", day_profile="week")
    late = pkg.StudentCounts(cl, "a3", "i3", late_key="l3")
    ctx.calls.clear()
    with pytest.raises(ValueError):
        plain.update("bf", slots, ids, np.zeros(4, np.int64))  # times without a use for them
    for sc in (timed, late):
        with pytest.raises(ValueError):
            sc.update("bf", slots, ids)  # times missing
        for n in (3, 5):
            with pytest.raises(ValueError):
                sc.update("bf", slots, ids, np.zeros(n, np.int64))
    assert ctx.calls == []  # refused before any native call
    for call in (plain.by_day, plain.by_hour_of_week, plain.top_late, timed.top_late, late.top_late,
                 lambda: plain.late([b"1"]), lambda: timed.late([b"1"])):
        with pytest.raises(ValueError):
            call()
    for bad in (dict(track_late=2), dict(late_key="l4", late_from=86401), dict(late_key="l4", late_from=-1),
                dict(late_key="l4", track_late=0)):
        with pytest.raises(ValueError):
            pkg.StudentCounts(cl, "a4", "i4", **bad)


def test_by_day_order_and_median_rule(pkg, stub_client):
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, late_key="cms:late", track_late=1, day_profile="week")
    counts = np.zeros((7, 24), np.uint64)
    counts[0, 9], counts[2, 8], counts[2, 23], counts[4, 0], counts[6, 12] = 5, 2, 1, 7, 3

    def read(tid, out):
        C.memmove(out, counts.ctypes.data, counts.nbytes)
    ctx.hooks["ske_tp_read"] = read
    assert np.array_equal(sc.by_hour_of_week(), counts)
    assert list(sc.by_day().items()) == [("Friday", 7), ("Monday", 5), ("Sunday", 3), ("Wednesday", 3)]
    listed = [(b"10001", 9), (b"10002", 4), (b"10003", 4), (b"10004", 1)]  # median 4: only 9 is above

    def hh_info(hid, info):
        info._obj.used = len(listed)

    def hh_list(hid, cid, thr, ids, lens, est, room, n, complete):
        ids_a = np.ctypeslib.as_array(C.cast(ids, C.POINTER(C.c_uint8)), (room * 16,)).reshape(room, 16)
        lens_a = np.ctypeslib.as_array(C.cast(lens, C.POINTER(C.c_uint32)), (room,))
        est_a = np.ctypeslib.as_array(C.cast(est, C.POINTER(C.c_uint32)), (room,))
        keep = [e for e in listed if e[1] >= thr]
        for i, (s, e) in enumerate(keep):
            ids_a[i, :len(s)] = np.frombuffer(s, np.uint8)
            lens_a[i], est_a[i] = len(s), e
        n._obj.value, complete._obj.value = len(keep), 1
    ctx.hooks["ske_hh_info"], ctx.hooks["ske_hh_list"] = hh_info, hh_list
    first = sc.insights()[0]
    assert first == {"title": "Habitual Latecomers", "complete": True, "data": {"10001": 9},
                     "description": "Found 1 students who frequently arrive after 9:00 AM"}
    assert sc.insights(late_threshold=4)[0]["data"] == {"10001": 9, "10002": 4, "10003": 4}
    assert sc.insights()[1] == {"title": "Attendance by Day", "data": sc.by_day(),
                                "description": "Distribution of attendance across different days"}


def test_epoch_seconds(pkg):
    es = pkg.epoch_seconds
    a = np.asarray([INT64_MIN, -1, 0, 1742374800], np.int64)
    assert es(a).dtype == np.int64 and np.array_equal(es(a), a)
    ms = np.asarray(["1969-12-31T23:59:59.500", "2025-03-19T08:59:59.999", "2025-03-19T09:00:00.000"],
                    "datetime64[ms]")
    assert es(ms).tolist() == [-1, 1742374799, 1742374800]
    assert es(ms.astype("datetime64[ns]")).tolist() == [-1, 1742374799, 1742374800]
    assert es(np.asarray(["2025-03-19"], "datetime64[D]")).tolist() == [1742342400]
    naive = datetime(2025, 3, 19, 9, 0, 0)
    west = datetime(2025, 3, 19, 9, 0, 0, tzinfo=timezone(timedelta(hours=-2)))
    east = datetime(2025, 3, 19, 9, 0, 0, tzinfo=timezone(timedelta(hours=5, minutes=30)))
    before = datetime(1969, 12, 31, 23, 59, 58, 250000)  # a fraction before 1970 floors away from zero
    got = es([naive, west, east, before])
    assert got.dtype == np.int64
    assert got.tolist() == [1742374800, 1742374800 + 7200, 1742374800 - 19800, -2]
    assert es([]).shape == (0,) and es([5, -5]).tolist() == [5, -5]
    with pytest.raises(TypeError):
        es(["2025-03-19"])
    with pytest.raises(TypeError):
        es([1.5])
