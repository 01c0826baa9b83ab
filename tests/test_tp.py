"""Time profiles on the GPU (csrc/sketch_tp.hip, ske_tp_*): the 168 weekday x
hour counters and the late bytes of a batch of swipe times, compared exactly
with numpy floor arithmetic written here (``epoch // 86400``, ``% 86400``);
then behind K1 in a recorded graph, and ``StudentCounts`` end to end against a
plain-Python group-by of the same rows."""
import ctypes as C
import os
from datetime import datetime, timedelta

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
DT_LO, DT_HI = -62135596800, 253402300799  # 0001-01-01T00:00:00 .. 9999-12-31T23:59:59
MONDAY = 1742169600    # 2025-03-17T00:00:00, a Monday
WED_9 = 1742374800     # 2025-03-19T09:00:00
SIZES = (0, 1, 63, 64, 65, 1025, 100003)
KINDS = ("one", "two", "week", "range", "extremes")
DAY_NAMES = ("Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday", "Sunday")
GUARD = 0xA5


# ---------------------------------------------------------------- the restatement
def restate(epoch, mask=None, want=1, late_from=32400):
    """(counts[168] uint64, late[n] uint8) by numpy floor arithmetic"""
    e = np.asarray(epoch, np.int64)
    day, sod = e // 86400, e % 86400
    bins = ((day + 3) % 7) * 24 + sod // 3600
    take = np.ones(e.size, bool) if mask is None else np.asarray(mask) == want
    return (np.bincount(bins[take], minlength=168).astype(np.uint64),
            (sod >= late_from).astype(np.uint8))


def test_pins(eng):
    """the restatement itself against datetime (every test below trusts it), then the pins on the device"""
    for e, (dow, hour) in {-1: (2, 23), 0: (3, 0), WED_9 - 1: (2, 8), WED_9: (2, 9), DT_LO: (0, 0),
                           DT_HI: (4, 23), MONDAY: (0, 0)}.items():
        t = datetime(1970, 1, 1) + timedelta(seconds=e)
        assert (t.weekday(), t.hour) == (dow, hour)
        counts, late = restate([e])
        assert counts[dow * 24 + hour] == 1 and counts.sum() == 1 and late[0] == (hour >= 9)
    with Profile(eng) as tid:
        check_add(eng, tid, np.zeros(168, np.uint64),
                  np.asarray([-1, 0, WED_9 - 1, WED_9, DT_LO, DT_HI, INT64_MIN, INT64_MAX], np.int64))
        got = eng.tp_counts(tid)
        assert got[2, 23] == got[3, 0] == got[2, 8] == got[2, 9] == got[0, 0] == got[4, 23] == 1
        assert got[6].sum() == 2 and got.sum() == 8


def times(kind, n, seed=0):
    rng = np.random.default_rng(1000 * len(kind) + n + seed)
    if kind == "one":  # one bin
        return WED_9 + rng.integers(0, 3600, n)
    if kind == "two":  # two adjacent hours of one day, mixed
        return WED_9 - 3600 + rng.integers(0, 7200, n)
    if kind == "week":  # uniform over the 168 bins
        return MONDAY + rng.integers(0, 7 * 86400, n)
    if kind == "range":  # the whole datetime range, negatives included
        return rng.integers(DT_LO, DT_HI, n, endpoint=True)
    edge = np.asarray([INT64_MIN, INT64_MAX, INT64_MIN + 1, INT64_MAX - 1, -1, 0, 1, -86400, -86401, 86399, 86400,
                       DT_LO, DT_HI, INT64_MIN + 86400, INT64_MAX - 86400], np.int64)
    return edge[rng.integers(0, edge.size, n)] if n > edge.size else edge[:n]


def mask_of(kind, n, seed=0):
    rng = np.random.default_rng(77 + n + seed)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    return (rng.random(n) < 0.85).astype(np.uint8)


# ---------------------------------------------------------------- device helpers
def make_engine(grid=None, form=None):
    """a context opened with SKE_TP_GRID / SKE_TP_FORM (ske_open reads them)"""
    ge.load_package()
    from rtsas_amd.engine import SketchEngine
    for name, v in (("SKE_TP_GRID", grid), ("SKE_TP_FORM", form)):
        if v is not None:
            os.environ[name] = str(v)
    try:
        return SketchEngine(0)
    finally:
        os.environ.pop("SKE_TP_GRID", None)
        os.environ.pop("SKE_TP_FORM", None)


@pytest.fixture(scope="module")
def eng():
    return make_engine()


class Profile:
    """tid of a fresh profile for the length of a test"""

    def __init__(self, engine, tid=0):
        self.engine, self.tid = engine, tid

    def __enter__(self):
        self.engine.tp_init(self.tid)
        return self.tid

    def __exit__(self, *exc):
        self.engine.tp_free(self.tid)
        return False


def add(engine, tid, epoch, mask=None, want=1, late_from=32400, late=True, e_off=0, m_off=0, l_off=0):
    """One ske_tp_add_async + sync over host arrays placed at the given element
    (epoch) and byte (mask, late) offsets of their allocations.  Returns the late
    bytes (None without).  The bytes around the late range must stay as they were."""
    from rtsas_amd.engine import DeviceBuffer
    e = np.ascontiguousarray(epoch, np.int64)
    n = e.size
    bufs = []
    d_e = DeviceBuffer(engine.ctx, (n + e_off) * 8 + 16)
    bufs.append(d_e)
    d_e.from_host(np.concatenate([np.zeros(e_off, np.int64), e]))
    p_m = p_l = None
    if mask is not None:
        d_m = DeviceBuffer(engine.ctx, n + m_off + 16)
        bufs.append(d_m)
        d_m.from_host(np.concatenate([np.full(m_off, 7, np.uint8), np.asarray(mask, np.uint8)]))
        p_m = C.c_void_p(d_m.ptr + m_off)
    if late:
        room = l_off + n + 16
        d_l = DeviceBuffer(engine.ctx, room)
        bufs.append(d_l)
        d_l.from_host(np.full(room, GUARD, np.uint8))
        p_l = C.c_void_p(d_l.ptr + l_off)
    engine.ctx.call("ske_tp_add_async", tid, C.c_void_p(d_e.ptr + 8 * e_off), n, p_m, want, late_from, p_l)
    engine.sync()
    out = None
    if late:
        raw = d_l.to_host(np.uint8, room)
        assert np.all(raw[:l_off] == GUARD) and np.all(raw[l_off + n:] == GUARD), "a late byte outside the batch"
        out = raw[l_off:l_off + n]
    for b in bufs:
        b.free()
    return out


def check_add(engine, tid, total, epoch, **kw):
    """add, then compare the late bytes and the accumulated counters (total is updated)"""
    late = add(engine, tid, epoch, **kw)
    counts, want_late = restate(epoch, kw.get("mask"), kw.get("want", 1), kw.get("late_from", 32400))
    total += counts
    if late is not None:
        assert np.array_equal(late, want_late)
    got = engine.tp_counts(tid)
    assert got.shape == (7, 24) and got.dtype == np.uint64
    assert np.array_equal(got.reshape(-1), total)


# ---------------------------------------------------------------- the add
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_and_inputs(eng, kind, n):
    with Profile(eng) as tid:
        total = np.zeros(168, np.uint64)
        e = times(kind, n)
        check_add(eng, tid, total, e)
        assert total.sum() == n
        if kind == "one" and n:
            assert np.count_nonzero(total) == 1
        if kind == "two" and n >= 63:
            assert np.count_nonzero(total) == 2
        if kind == "week" and n == 100003:
            assert np.count_nonzero(total) == 168


@pytest.mark.parametrize("mkind,want", [(None, 1), ("most", 0), ("most", 1), ("zeros", 0), ("zeros", 1),
                                        ("ones", 0), ("ones", 1)])
def test_masks(eng, mkind, want):
    """late ignores the mask; the counters follow it"""
    with Profile(eng) as tid:
        total = np.zeros(168, np.uint64)
        for n in (1, 65, 1025, 100003):
            for kind in ("one", "week"):
                m = None if mkind is None else mask_of(mkind, n)
                check_add(eng, tid, total, times(kind, n, seed=1), mask=m, want=want)


@pytest.mark.parametrize("late_from", [0, 32400, 86399, 86400])
def test_late_from(eng, late_from):
    e = np.concatenate([times("range", 1025), times("extremes", 15),
                        MONDAY + np.asarray([0, 32399, 32400, 86399, 86400 + 32400])])
    with Profile(eng) as tid:
        total = np.zeros(168, np.uint64)
        check_add(eng, tid, total, e, late_from=late_from)
        want = restate(e, late_from=late_from)[1]
        assert want.all() if late_from == 0 else not want.any() if late_from == 86400 else 0 < want.sum() < e.size
        check_add(eng, tid, total, e, late_from=late_from, late=False)  # no late output


def test_alignment(eng):
    """epoch from an even and an odd element, mask and late from every byte
    offset, every n & 3: the head, the wide body and the tail of each"""
    with Profile(eng) as tid:
        total = np.zeros(168, np.uint64)
        k = 0
        for e_off in (0, 1):
            for r in range(4):
                for m_off in range(8):
                    l_off = (3 * m_off + r + e_off) % 8
                    n = 4 * (257 + m_off) + r  # a few hundred groups of four, two tiles
                    k += 1
                    check_add(eng, tid, total, times("week", n, seed=k), mask=mask_of("most", n, seed=k),
                              want=k & 1, e_off=e_off, m_off=m_off, l_off=l_off)
        for off in range(8):  # one of the two byte arrays alone decides the head
            for r in range(4):
                n, k = 260 + r, k + 1
                check_add(eng, tid, total, times("range", n, seed=k), mask=mask_of("most", n, seed=k),
                          late=False, e_off=off & 1, m_off=off)
                check_add(eng, tid, total, times("range", n, seed=k), e_off=(off >> 1) & 1, l_off=off)
        for e_off in (0, 1):  # the epochs alone
            for n in (1, 2, 3, 4, 5, 6, 7, 8, 9, 4099):
                k += 1
                check_add(eng, tid, total, times("two", n, seed=k), late=False, e_off=e_off)


@pytest.mark.parametrize("grid", [1, 3])
def test_grid_stride_loop(grid):
    """100 003 swipes through one and three workgroups: dozens of tiles each"""
    engine = make_engine(grid=grid)
    with Profile(engine) as tid:
        total = np.zeros(168, np.uint64)
        for kind in ("two", "week", "extremes"):
            n = 100003
            check_add(engine, tid, total, times(kind, n), mask=mask_of("most", n), want=1, e_off=1, m_off=1, l_off=2)
        check_add(engine, tid, total, times("one", 100003))


def test_forms_identical():
    """SKE_TP_FORM 0 (a wavefront whose tile holds one bin adds it once) and 1 (one add per lane)"""
    engines = [make_engine(form=0), make_engine(form=1)]
    totals = [np.zeros(168, np.uint64) for _ in engines]
    for engine, total in zip(engines, totals):
        engine.tp_init(3)
        for kind in KINDS:
            for n in (65, 1025, 100003):
                check_add(engine, 3, total, times(kind, n), mask=mask_of("most", n), want=1)
                check_add(engine, 3, total, times(kind, n))
    assert np.array_equal(engines[0].tp_counts(3), engines[1].tp_counts(3))
    assert np.array_equal(totals[0], totals[1]) and totals[0].sum() > 0


def test_accumulate_reset_import(eng):
    with Profile(eng, 5) as tid:
        total = np.zeros(168, np.uint64)
        for seed, kind in enumerate(("week", "two", "week")):
            check_add(eng, tid, total, times(kind, 1025, seed=seed))
        assert total.sum() == 3 * 1025
        eng.tp_reset(tid)
        assert not eng.tp_counts(tid).any()
        rng = np.random.default_rng(5)
        saved = rng.integers(0, 2 ** 64 - 1, 168, dtype=np.uint64, endpoint=True)
        eng.tp_import(tid, saved.reshape(7, 24))
        assert np.array_equal(eng.tp_counts(tid).reshape(-1), saved)
        with pytest.raises(ValueError):
            eng.tp_import(tid, saved[:167])
        # the flush carries into the upper word
        start = np.zeros(168, np.uint64)
        start[2 * 24 + 9] = 2 ** 32 - 1
        eng.tp_import(tid, start)
        add(eng, tid, times("one", 1025), late=False)
        got = eng.tp_counts(tid)
        assert int(got[2, 9]) == 2 ** 32 + 1024 and int(got.sum()) == 2 ** 32 + 1024


def test_errors(eng, pkg):
    from rtsas_amd import _lib
    from rtsas_amd.engine import DeviceBuffer

    def code(name, *args):
        with pytest.raises(pkg.SketchLibError) as e:
            eng.ctx.call(name, *args)
        return e.value.code

    buf = (C.c_uint64 * 168)()
    d = DeviceBuffer(eng.ctx, 64)
    ep = C.c_void_p(d.ptr)
    for name, args in (("ske_tp_free", ()), ("ske_tp_reset", ()), ("ske_tp_read", (buf,)), ("ske_tp_import", (buf,)),
                       ("ske_tp_add_async", (ep, 4, None, 1, 32400, None))):
        assert code(name, 9, *args) == _lib.SKE_ETPNOSET, name  # a free tid
        assert code(name, _lib.SKE_MAX_TP, *args) == _lib.SKE_EINVAL, name
    assert code("ske_tp_init", _lib.SKE_MAX_TP) == _lib.SKE_EINVAL
    eng.tp_init(9)
    assert code("ske_tp_init", 9) == _lib.SKE_ETPEXISTS
    assert code("ske_tp_add_async", 9, ep, 4, None, 1, 86401, None) == _lib.SKE_EINVAL
    assert code("ske_tp_add_async", 9, ep, 4, None, 2, 32400, None) == _lib.SKE_EINVAL
    assert code("ske_tp_add_async", 9, ep, 4, None, -1, 32400, None) == _lib.SKE_EINVAL
    assert code("ske_tp_add_async", 9, ep, 2 ** 32 - 1, None, 1, 32400, None) == _lib.SKE_EINVAL
    assert code("ske_tp_add_async", 9, None, 4, None, 1, 32400, None) == _lib.SKE_EINVAL
    # n == 0 does nothing, but still checks its arguments
    eng.ctx.call("ske_tp_add_async", 9, None, 0, None, 1, 86400, None)
    assert code("ske_tp_add_async", 9, None, 0, None, 2, 32400, None) == _lib.SKE_EINVAL
    assert code("ske_tp_add_async", 9, None, 0, None, 1, 86401, None) == _lib.SKE_EINVAL
    assert code("ske_tp_read", 9, None) == _lib.SKE_EINVAL
    assert not eng.tp_counts(9).any()
    eng.tp_free(9)
    assert code("ske_tp_read", 9, buf) == _lib.SKE_ETPNOSET
    eng.tp_init(9)  # the id is free again
    eng.tp_free(9)
    d.free()


# ---------------------------------------------------------------- behind K1
def _swipes(n=6007):
    """1000 members of 5-digit ids, n swipes of which about a tenth are not
    members, over a fortnight between 07:00 and 11:00"""
    rng = np.random.default_rng(29)
    members = rng.choice(np.arange(10000, 100000), 1000, replace=False)
    others = np.setdiff1d(np.arange(10000, 100000), members)
    ids = np.where(rng.random(n) < 0.9, rng.choice(members[:60], n), rng.choice(others[:12], n))
    when = MONDAY + rng.integers(0, 14, n) * 86400 + rng.integers(7 * 3600, 11 * 3600, n)
    return members, ids, rng.integers(0, 4, n), when.astype(np.int64)


def test_capture(pkg, engine):
    """swipes, the two adds, the profile add, the late add and the late track
    recorded once and replayed three times: three direct updates"""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    members, ids, key_of, when = _swipes()
    n = len(ids)
    engine.reserve(0, 0.01, 1000)
    engine.hll_reserve(4)
    mbuf, moffs = pkg.pack_ints(members)
    engine.ctx.call("ske_bf_madd", 0, mbuf.ctypes.data_as(C.c_void_p), moffs.ctypes.data_as(C.c_void_p),
                    len(members), None, 0)
    sbuf, _ = pkg.pack_ints(ids)
    b = DeviceBatch(engine.ctx, n, 5)
    b.bytes.from_host(sbuf)
    b.slot.from_host(key_of.astype(np.uint32))
    valid, late = DeviceBuffer(engine.ctx, n + 16), DeviceBuffer(engine.ctx, n + 16)
    d_when = DeviceBuffer(engine.ctx, n * 8)
    d_when.from_host(when)
    for i in range(6):
        engine.cms_init(i, 2000, 7)
    for i in range(2):
        engine.hh_init(i, 12)
        engine.tp_init(i)
    thr = 100  # a member's late swipes pass it at the third update, no other id's do

    def step(k):  # k = 0: direct, 1: recorded
        engine.swipes_fixed_async(0, b, valid)
        engine.cms_add(3 * k, b, mask=valid, want=1)
        engine.cms_add(3 * k + 1, b, mask=valid, want=0)
        engine.tp_add(k, d_when, n, late_from=32400, late=late)
        engine.cms_add(3 * k + 2, b, mask=late, want=1)
        engine.hh_track(k, 3 * k + 2, b, thr, mask=late, want=1)

    for _ in range(3):
        step(0)
        engine.sync()
    counts, want_late = restate(when)
    assert np.array_equal(engine.tp_counts(0).reshape(-1), 3 * counts)
    assert np.array_equal(late.to_host(np.uint8, n), want_late) and 0 < want_late.sum() < n
    assert engine.cms_table(2)[1] == 3 * int(want_late.sum())
    direct = engine.hh_list(0, 2, thr)
    assert 0 < len(direct[0]) < len(set(ids.tolist())) and direct[2] is True

    g = engine.capture(lambda: step(1))
    assert not engine.tp_counts(1).any() and engine.hh_info(1)["used"] == 0  # recording ran nothing
    for _ in range(3):
        g.launch()
    engine.sync()
    assert np.array_equal(engine.tp_counts(1), engine.tp_counts(0))
    for i in range(3):
        a, c = engine.cms_table(i), engine.cms_table(3 + i)
        assert np.array_equal(a[0], c[0]) and a[1] == c[1]
    got = engine.hh_list(1, 5, thr)
    assert got[0] == direct[0] and np.array_equal(got[1], direct[1]) and got[2] is True
    with pytest.raises(pkg.SketchLibError) as e:  # a recorded graph points to the profile
        engine.tp_free(1)
    assert e.value.code == -13
    g.free()
    engine.tp_free(1)


# ---------------------------------------------------------------- StudentCounts
def murmur2_32(data: bytes, seed: int) -> int:
    m, mask = 0x5BD1E995, 0xFFFFFFFF
    h = (seed ^ len(data)) & mask
    nblk = len(data) // 4
    for j in range(nblk):
        k = int.from_bytes(data[4 * j:4 * j + 4], "little")
        k = k * m & mask
        k ^= k >> 24
        k = k * m & mask
        h = (h * m & mask) ^ k
    tail = data[4 * nblk:]
    if tail:
        h ^= int.from_bytes(tail, "little")
        h = h * m & mask
    h ^= h >> 13
    h = h * m & mask
    return h ^ (h >> 15)


def cms_estimates(rows, width=2000, depth=7):
    """the Count-Min estimate of every distinct id of ``rows`` (a list of id
    bytes, one per counted swipe), restated: cell = MurmurHash2(id, seed = row) % width"""
    table = np.zeros((depth, width), np.int64)
    cells = {s: [murmur2_32(s, r) % width for r in range(depth)] for s in set(rows)}
    for s in rows:
        for r, c in enumerate(cells[s]):
            table[r, c] += 1
    return {s: min(int(table[r, c]) for r, c in enumerate(cs)) for s, cs in cells.items()}


def test_student_counts(pkg, client):
    assert [murmur2_32(b"12345", r) % 2000 for r in range(4)] == [18, 136, 1146, 1175]
    members, ids, key_of, when = _swipes(3001)
    n = len(ids)
    keys = [f"hll:unique:CS10{k}:2025-03-17" for k in range(4)]
    mbuf, moffs = pkg.pack_ints(members)
    sbuf, _ = pkg.pack_ints(ids)
    id_mat = sbuf.reshape(n, 5)
    rows = [bytes(r) for r in id_mat]
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 1000)
    client.bf_madd_packed("bf:students", mbuf, moffs)
    slots = np.asarray([client.key_slot(k) for k in keys], np.uint32)[key_of]

    # the plain-Python group-bys of the same rows (the reference's, attendance_analysis.py:65-85)
    stamps = [datetime(1970, 1, 1) + timedelta(seconds=int(t)) for t in when]
    true_late, true_day = {}, {}
    for s, t in zip(rows, stamps):
        if t.hour >= 9:
            true_late[s] = true_late.get(s, 0) + 1
        true_day[DAY_NAMES[t.weekday()]] = true_day.get(DAY_NAMES[t.weekday()], 0) + 1
    # precondition, decided by the restatement alone: no collision touches an estimate
    assert cms_estimates([s for s, t in zip(rows, stamps) if t.hour >= 9]) == true_late
    assert len(true_late) > 20 and len(set(true_late.values())) > 3

    plain = pkg.StudentCounts(client, "cms:a0", "cms:i0", track_attended=30, track_invalid=5, capacity_log2=12)
    sc = pkg.StudentCounts(client, track_attended=30, track_invalid=5, capacity_log2=12, late_key="cms:late",
                           track_late=1, day_profile="week")
    cut = 1234
    as_dt64 = when.astype("datetime64[s]")  # the second batch's times in another input form
    valid = []
    for lo, hi, tm in ((0, cut, when[:cut]), (cut, n, as_dt64[cut:])):
        v0 = plain.update("bf:students", slots[lo:hi], id_mat[lo:hi])
        v1 = sc.update("bf:students", slots[lo:hi], id_mat[lo:hi], tm)
        assert np.array_equal(v0, v1)
        valid.append(v1)
    valid = np.concatenate(valid).astype(np.uint8)
    assert 0 < valid.sum() < n

    assert sc.by_day() == true_day and list(sc.by_day()) == sorted(true_day)
    assert np.array_equal(sc.by_hour_of_week().reshape(-1), restate(when)[0])
    assert np.array_equal(client.tp_counts("week"), sc.by_hour_of_week())
    everyone = sorted(set(rows))
    assert sc.late(everyone).tolist() == [true_late.get(s, 0) for s in everyone]
    order = sorted(true_late.items(), key=lambda kv: (-kv[1], kv[0]))
    ids_l, est, complete = sc.top_late()
    assert complete and list(zip(ids_l, (int(e) for e in est))) == order
    assert sc.top_late(k=3)[0] == [s for s, _ in order[:3]]
    med = float(np.median(list(true_late.values())))
    frequent = {s.decode(): c for s, c in true_late.items() if c > med}
    ins = sc.insights()
    assert [i["title"] for i in ins] == ["Habitual Latecomers", "Attendance by Day", "Most Consistent Attendees",
                                         "Invalid Attendance Attempts"]
    assert ins[0]["data"] == frequent and 0 < len(frequent) < len(true_late) and ins[0]["complete"] is True
    assert ins[0]["description"] == f"Found {len(frequent)} students who frequently arrive after 9:00 AM"
    assert ins[1]["data"] == true_day
    at = sorted(set(true_late.values()))[-3]
    assert sc.insights(late_threshold=at)[0]["data"] == {s.decode(): c for s, c in true_late.items() if c >= at}
    # the two existing insights and their counters are what they are without the new options
    assert ins[2:] == plain.insights() and len(ins[2]["data"]) > 0 and len(ins[3]["data"]) > 0
    for key, other in (("cms:attended", "cms:a0"), ("cms:invalid", "cms:i0")):
        assert np.array_equal(client.cms_table(key)[0], client.cms_table(other)[0])
    # the host-array add of the facade, with a mask, into a profile of its own
    client.tp_create("valid only")
    client.tp_add("valid only", stamps, mask=valid, want=1)
    assert np.array_equal(client.tp_counts("valid only").reshape(-1), restate(when, valid, 1)[0])
    assert client.tp_free("valid only") is True
    # FLUSHALL (the fixture's) frees the rest
