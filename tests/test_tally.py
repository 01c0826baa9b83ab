"""Tallies on the GPU (csrc/sketch_tally.hip, ske_tally_*): exact event counts
per key, compared exactly with ``collections.Counter`` and ``sorted(...,
key=(-count, key))`` written here; the three async forms, the tuning contexts
that reach the LDS table's overflow and the stride loop at small n, capacity,
``top`` against the ends of ``list``, a recorded graph behind K1, and
``StudentCounts`` / ``AttendanceProcessor`` end to end against a plain-Python
group-by of the same messages."""
import ctypes as C
import json
import os
from collections import Counter

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1025, 100003)
POPULATIONS = ("one", "two", "zipf37", "k5000", "distinct")
GUARD = 0xA5


# ---------------------------------------------------------------- inputs and the restatement
def keys_of(pop, n, seed=0):
    """n keys (bytes) of a population"""
    rng = np.random.default_rng(1000 * len(pop) + n + seed)
    if pop == "one":
        return [b"CS101-L01"] * n
    if pop == "two":
        return [(b"CS101-L01", b"CS101-L02")[j] for j in rng.integers(0, 2, n)]
    if pop == "zipf37":
        p = 1.0 / np.arange(1, 38) ** 1.1
        return [b"LECT%05d" % j for j in rng.choice(37, n, p=p / p.sum())]
    if pop == "k5000":
        return [b"LECT%05d" % j for j in rng.integers(0, 5000, n)]
    return [b"K%08d" % j for j in rng.permutation(n)]


def mask_of(kind, n, seed=0):
    if kind is None:
        return None
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    return (np.random.default_rng(77 + n + seed).random(n) < 0.85).astype(np.uint8)


def ordered(events, valid=None, by=0):
    """the listing of two Counters: [(key, events, valid)] by count descending, key bytes ascending"""
    valid = valid or Counter()
    rows = [(k, e, valid.get(k, 0)) for k, e in events.items()]
    return sorted(rows, key=lambda r: (-r[1 + by], r[0]))


class Want:
    """the running group-by of everything added to one tally"""

    def __init__(self):
        self.events, self.valid, self.taken = Counter(), Counter(), 0

    def add(self, keys, mask=None, take=None):
        for i, k in enumerate(keys):
            if take is not None and not take[i]:
                continue
            self.taken += 1
            self.events[k] += 1
            if mask is not None and mask[i] == 1:
                self.valid[k] += 1


def listing(engine, tid, min_events=0):
    keys, ev, va, complete = engine.tally_list(tid, min_events)
    return [(k, int(e), int(v)) for k, e, v in zip(keys, ev, va)], complete


def check(engine, tid, want):
    """the whole tally against the running group-by"""
    got, complete = listing(engine, tid)
    assert complete is True
    assert got == ordered(want.events, want.valid)
    info = engine.tally_info(tid)
    assert info["used"] == len(want.events) and info["overflow"] == 0 and info["taken"] == want.taken
    assert info["dropped_events"] == 0 and info["dropped_valid"] == 0
    assert sum(r[1] for r in got) == want.taken


# ---------------------------------------------------------------- device helpers
def make_engine(grid=None, form=None, lds_log2=None):
    """a context opened with SKE_TALLY_GRID / SKE_TALLY_FORM / SKE_TALLY_LDS_LOG2 (ske_open reads them)"""
    ge.load_package()
    from rtsas_amd.engine import SketchEngine
    names = (("SKE_TALLY_GRID", grid), ("SKE_TALLY_FORM", form), ("SKE_TALLY_LDS_LOG2", lds_log2))
    for name, v in names:
        if v is not None:
            os.environ[name] = str(v)
    try:
        return SketchEngine(0)
    finally:
        for name, _ in names:
            os.environ.pop(name, None)


@pytest.fixture(scope="module")
def eng():
    return make_engine()


class Tally:
    """tid of a fresh tally for the length of a test"""

    def __init__(self, engine, log2=14, tid=0):
        self.engine, self.log2, self.tid = engine, log2, tid

    def __enter__(self):
        self.engine.tally_init(self.tid, self.log2)
        return self.tid

    def __exit__(self, *exc):
        self.engine.tally_free(self.tid)
        return False


def add(engine, tid, keys, mask=None, form="packed", status=None, seed=0):
    """One async add + sync of host keys through one of the three forms.  The
    spans form scatters the keys over a byte buffer at every start & 7, with
    guard bytes between and behind them that must stay as they were."""
    from rtsas_amd.engine import DeviceBuffer
    n = len(keys)
    bufs = []

    def dev(arr, extra=16):
        a = np.ascontiguousarray(arr)
        d = DeviceBuffer(engine.ctx, a.nbytes + extra)
        bufs.append(d)
        d.from_host(a)
        return d

    p_m = None
    if mask is not None:
        p_m = C.c_void_p(dev(np.asarray(mask, np.uint8)).ptr)
    if form == "packed":
        lens = np.fromiter((len(k) for k in keys), np.int64, n)
        offs = np.zeros(n + 1, np.uint32)
        offs[1:] = np.cumsum(lens)
        raw = np.frombuffer(b"".join(keys), np.uint8)
        d_b, d_o = dev(raw), dev(offs)
        engine.ctx.call("ske_tally_add_packed_async", tid, C.c_void_p(d_b.ptr), C.c_void_p(d_o.ptr), n, p_m)
    elif form == "fixed":
        w = len(keys[0]) if n else 1
        assert all(len(k) == w for k in keys)
        d_b = dev(np.frombuffer(b"".join(keys), np.uint8))
        engine.ctx.call("ske_tally_add_fixed_async", tid, C.c_void_p(d_b.ptr), w, n, p_m)
    else:
        rng = np.random.default_rng(5 + n + seed)
        gaps = rng.integers(0, 8, n)
        lens = np.fromiter((len(k) for k in keys), np.int64, n)
        start = np.zeros(n, np.int64)
        pos = int(rng.integers(0, 8))
        for i in range(n):
            pos += int(gaps[i])
            start[i] = pos
            pos += int(lens[i])
        total = (pos + 7) // 8 * 8  # nothing behind the 8-byte boundary is the batch's
        raw = np.full(total + 64, GUARD, np.uint8)
        for i, k in enumerate(keys):
            raw[start[i]:start[i] + len(k)] = np.frombuffer(k, np.uint8)
        d_b = dev(raw, extra=0)
        d_s, d_l = dev(start.astype(np.uint32)), dev(lens.astype(np.uint32))
        p_st = C.c_void_p(dev(np.asarray(status, np.uint8)).ptr) if status is not None else None
        engine.ctx.call("ske_tally_add_spans_async", tid, C.c_void_p(d_b.ptr), C.c_void_p(d_s.ptr),
                        C.c_void_p(d_l.ptr), n, p_st, p_m)
        engine.sync()
        assert np.array_equal(d_b.to_host(np.uint8, raw.size), raw), "the batch's bytes changed"
    engine.sync()
    for b in bufs:
        b.free()


# ---------------------------------------------------------------- the add
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pop", POPULATIONS)
def test_sizes_and_populations(eng, pop, n):
    with Tally(eng, 18) as tid:
        want = Want()
        keys = keys_of(pop, n)
        m = mask_of("most", n)
        add(eng, tid, keys, m)
        want.add(keys, m)
        check(eng, tid, want)
        if pop in ("one", "distinct"):
            assert len(want.events) == (min(n, 1) if pop == "one" else n)
        if pop == "k5000" and n == 100003:
            assert len(want.events) == 5000  # more keys than a workgroup's LDS table holds


LENGTH_KEYS = [bytes(range(65, 65 + w)) for w in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32)]
PAIRS = [bytes(32), bytes(31) + b"\x01",                      # differ only in byte 31
         b"x" * 16 + b"a" + b"y" * 7, b"x" * 16 + b"b" + b"y" * 7,  # differ only behind byte 16
         b"A\0", b"A\0\0", b"\0"]                            # beside LENGTH_KEYS' b"A" and b""


@pytest.mark.parametrize("form", ["packed", "spans"])
def test_key_lengths(eng, form):
    rng = np.random.default_rng(32)
    pool = LENGTH_KEYS + PAIRS
    assert len(set(pool)) == len(pool)
    keys = [pool[j] for j in rng.integers(0, len(pool), 4099)]
    m = mask_of("most", len(keys))
    with Tally(eng) as tid:
        want = Want()
        add(eng, tid, keys, m, form=form)
        want.add(keys, m)
        check(eng, tid, want)
        assert len(want.events) == len(pool)
        # the listing's order puts a prefix before its extensions
        got = [r[0] for r in listing(eng, tid)[0]]
        assert got == [r[0] for r in ordered(want.events, want.valid)]
        ev, va = eng.tally_query(tid, *pack(pool + [b"absent", b"A\0\0\0"]))
        assert ev.tolist() == [want.events[k] for k in pool] + [0, 0]
        assert va.tolist() == [want.valid[k] for k in pool] + [0, 0]


def pack(keys):
    offs = np.zeros(len(keys) + 1, np.uint32)
    offs[1:] = np.cumsum([len(k) for k in keys])
    return np.frombuffer(b"".join(keys), np.uint8), offs


@pytest.mark.parametrize("form", ["packed", "fixed", "spans"])
def test_too_long_key_is_dropped(eng, form):
    """33 bytes: not grouped, counted as dropped, overflow set, the sums still meet taken"""
    n = 1025
    if form == "fixed":
        keys = [b"L" * 33] * n
    else:
        keys = [b"L" * 33 if i % 5 == 0 else b"CS101" for i in range(n)]
    m = mask_of("most", n)
    nlong = sum(len(k) == 33 for k in keys)
    with Tally(eng) as tid:
        add(eng, tid, keys, m, form=form)
        got, complete = listing(eng, tid)
        info = eng.tally_info(tid)
        assert complete is False and info["overflow"] != 0 and info["taken"] == n
        assert info["dropped_events"] == nlong
        assert info["dropped_valid"] == sum(int(m[i]) for i, k in enumerate(keys) if len(k) == 33)
        assert sum(r[1] for r in got) + info["dropped_events"] == info["taken"]
        assert sum(r[2] for r in got) + info["dropped_valid"] == int(m.sum())
        assert got == ([] if form == "fixed" else [(b"CS101", n - nlong, int(m.sum()) - info["dropped_valid"])])
        eng.tally_reset(tid)
        assert listing(eng, tid) == ([], True) and eng.tally_info(tid)["taken"] == 0


@pytest.mark.parametrize("mkind", [None, "zeros", "ones", "most"])
def test_masks(eng, mkind):
    with Tally(eng) as tid:
        want = Want()
        for n in (1, 65, 1025, 100003):
            for pop in ("one", "zipf37"):
                keys, m = keys_of(pop, n, seed=1), mask_of(mkind, n)
                add(eng, tid, keys, m)
                want.add(keys, m)
        check(eng, tid, want)
        nvalid = sum(want.valid.values())
        assert nvalid == want.taken if mkind == "ones" else nvalid == 0 if mkind != "most" else 0 < nvalid < want.taken


@pytest.mark.parametrize("form", ["packed", "fixed", "spans"])
def test_forms(eng, form):
    with Tally(eng) as tid:
        want = Want()
        for n in (1, 64, 1025, 20011):
            for pop in ("one", "zipf37", "k5000"):
                keys, m = keys_of(pop, n, seed=2), mask_of("most", n, seed=2)
                add(eng, tid, keys, m, form=form)
                want.add(keys, m)
        check(eng, tid, want)


def test_spans_status_holes(eng):
    """a status column with holes: only status 0 is taken; every start & 7 occurs"""
    n = 4099
    keys = keys_of("zipf37", n, seed=3)
    status = (np.random.default_rng(9).random(n) < 0.3).astype(np.uint8)
    status[::7] = 255  # the parser's -1
    m = mask_of("most", n, seed=3)
    with Tally(eng) as tid:
        want = Want()
        add(eng, tid, keys, m, form="spans", status=status)
        want.add(keys, m, take=status == 0)
        add(eng, tid, keys, None, form="spans", status=np.ones(n, np.uint8))  # nothing taken
        check(eng, tid, want)
        assert 0 < want.taken < n


@pytest.mark.parametrize("grid,form,lds_log2", [(1, 0, 4), (3, 0, 4), (3, 0, None), (None, 1, None), (1, 1, 4)])
def test_tuning_contexts(grid, form, lds_log2):
    """16 LDS slots and one or three workgroups: 1025 items overflow the LDS
    table into the insert-or-add in memory and walk the stride loop; form 1 is
    that path alone.  The counts do not change."""
    engine = make_engine(grid=grid, form=form, lds_log2=lds_log2)
    with Tally(engine, 17) as tid:
        want = Want()
        for n in (65, 1025, 20011):
            for pop in POPULATIONS:
                for f in ("packed", "spans"):
                    keys, m = keys_of(pop, n, seed=4), mask_of("most", n, seed=4)
                    add(engine, tid, keys, m, form=f)
                    want.add(keys, m)
        check(engine, tid, want)


def test_batches_import_query(eng):
    """several batches into one tally; its listing imported into a second, twice"""
    with Tally(eng, 14, 1) as a, Tally(eng, 13, 2) as b:
        want = Want()
        for seed, pop in enumerate(("zipf37", "k5000", "two", "zipf37")):
            keys, m = keys_of(pop, 1025, seed=seed), mask_of("most", 1025, seed=seed)
            add(eng, a, keys, m)
            want.add(keys, m)
        check(eng, a, want)
        keys, ev, va, complete = eng.tally_list(a)
        eng.tally_import(b, keys, ev, va)
        assert listing(eng, b) == listing(eng, a)
        assert eng.tally_info(b)["taken"] == want.taken
        eng.tally_import(b, keys[:10], ev[:10], va[:10])  # insert-or-ADD
        got = dict((r[0], r[1:]) for r in listing(eng, b)[0])
        for i, k in enumerate(keys):
            f = 2 if i < 10 else 1
            assert got[k] == (f * int(ev[i]), f * int(va[i]))
        some = keys[:5] + [b"nobody", b""]
        qe, qv = eng.tally_query(a, *pack(some))
        assert qe.tolist() == [want.events[k] for k in some[:5]] + [0, 0]
        assert qv.tolist() == [want.valid[k] for k in some[:5]] + [0, 0]
        assert eng.tally_list(a, min_events=int(ev[3]))[0] == [k for k, e in zip(keys, ev) if e >= ev[3]]


# ---------------------------------------------------------------- capacity
def test_capacity_overflow(eng):
    """2^8 slots take 128 claims (SKE_TALLY_LOAD_DEN, a condition of the design):
    300 distinct keys cannot all be held"""
    n = 3000
    rng = np.random.default_rng(300)
    keys = [b"ROOM-%03d" % j for j in rng.integers(0, 300, n)]
    assert len(set(keys)) == 300
    m = mask_of("most", n)
    true_e, true_v = Counter(keys), Counter(k for k, v in zip(keys, m) if v)
    with Tally(eng, 8) as tid:
        add(eng, tid, keys, m)
        got, complete = listing(eng, tid)
        info = eng.tally_info(tid)
        assert complete is False and info["overflow"] != 0
        assert 0 < info["used"] <= 256 and info["used"] == len(got) and info["capacity"] == 256
        for k, e, v in got:
            assert 0 < e <= true_e[k] and v <= true_v[k]
        assert info["taken"] == n and info["dropped_events"] > 0
        assert sum(r[1] for r in got) + info["dropped_events"] == n
        assert sum(r[2] for r in got) + info["dropped_valid"] == int(m.sum())


def test_capacity_fits(eng):
    """100 distinct keys in 2^8 slots stay complete and exact"""
    n = 3000
    keys = [b"ROOM-%03d" % j for j in np.random.default_rng(100).integers(0, 100, n)]
    m = mask_of("most", n)
    with Tally(eng, 8) as tid:
        want = Want()
        add(eng, tid, keys, m)
        want.add(keys, m)
        check(eng, tid, want)
        assert len(want.events) == 100


# ---------------------------------------------------------------- top
def _top_rows(end):
    return [(k, int(e), int(v)) for k, e, v in zip(*end)]


@pytest.mark.parametrize("nkeys", [0, 2, 40])
def test_top_is_the_ends_of_list(eng, nkeys):
    """ties across the cut (many keys share a count), fewer than k entries, an empty tally"""
    rng = np.random.default_rng(40 + nkeys)
    keys = []
    for j in range(nkeys):
        keys += [b"LEC-%02d" % j] * (1 + j // 4)  # four keys per count: every cut crosses a tie
    keys = [keys[j] for j in rng.permutation(len(keys))]
    m = mask_of("most", len(keys))
    with Tally(eng) as tid:
        want = Want()
        add(eng, tid, keys, m)
        want.add(keys, m)
        check(eng, tid, want)
        for by in (0, 1):
            full = ordered(want.events, want.valid, by)
            for k in (1, 3, 16):
                head, tail, complete = eng.tally_top(tid, k, by)
                assert complete is True
                assert _top_rows(head) == full[:k]
                assert _top_rows(tail) == (full[-k:] if full else [])


def test_errors(eng, pkg):
    from rtsas_amd import _lib
    from rtsas_amd.engine import DeviceBuffer

    def code(name, *args):
        with pytest.raises(pkg.SketchLibError) as e:
            eng.ctx.call(name, *args)
        return e.value.code

    d = DeviceBuffer(eng.ctx, 64)
    p = C.c_void_p(d.ptr)
    info = _lib.TallyInfo()
    for name, args in (("ske_tally_free", ()), ("ske_tally_reset", ()), ("ske_tally_info", (C.byref(info),)),
                       ("ske_tally_add_packed_async", (p, p, 1, None)),
                       ("ske_tally_add_fixed_async", (p, 4, 1, None)),
                       ("ske_tally_add_spans_async", (p, p, p, 1, None, None))):
        assert code(name, 9, *args) == _lib.SKE_ETALLYNOSET, name
        assert code(name, _lib.SKE_MAX_TALLY, *args) == _lib.SKE_EINVAL, name
    assert code("ske_tally_init", 9, 7) == _lib.SKE_ETALLYCAP
    assert code("ske_tally_init", 9, 25) == _lib.SKE_ETALLYCAP
    eng.tally_init(9, 8)
    assert code("ske_tally_init", 9, 8) == _lib.SKE_ETALLYEXISTS
    assert code("ske_tally_add_fixed_async", 9, p, 0, 1, None) == _lib.SKE_EINVAL
    assert code("ske_tally_add_packed_async", 9, p, p, 2 ** 32 - 1, None) == _lib.SKE_EINVAL
    assert code("ske_tally_add_packed_async", 9, None, p, 1, None) == _lib.SKE_EINVAL
    eng.ctx.call("ske_tally_add_packed_async", 9, None, None, 0, None)  # n == 0 does nothing
    buf, offs = pack([b"ok", b"L" * 33])
    assert code("ske_tally_add", 9, buf.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), 2, None,
                0) == _lib.SKE_ETOOLONG
    assert eng.tally_info(9)["taken"] == 0  # refused before anything was counted
    n, complete = C.c_uint64(), C.c_int()
    buf, offs = pack([b"a", b"b", b"c"])
    eng.ctx.call("ske_tally_add", 9, buf.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), 3, None, 0)
    assert code("ske_tally_list", 9, 0, None, None, None, None, 0, C.byref(n), C.byref(complete)) == \
        _lib.SKE_ETALLYSPACE and n.value == 3
    with pytest.raises(pkg.SketchLibError):
        eng.tally_top(9, 17, 0)
    with pytest.raises(pkg.SketchLibError):
        eng.tally_top(9, 3, 2)
    eng.tally_free(9)
    d.free()


# ---------------------------------------------------------------- behind K1
def test_capture(pkg, engine):
    """swipes and a tally add masked by K1's answers, recorded once and replayed
    twice: twice one batch's counts"""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    rng = np.random.default_rng(29)
    n = 6007
    members = rng.choice(np.arange(10000, 100000), 1000, replace=False)
    others = np.setdiff1d(np.arange(10000, 100000), members)
    ids = np.where(rng.random(n) < 0.9, rng.choice(members[:60], n), rng.choice(others[:12], n))
    engine.reserve(0, 0.01, 1000)
    engine.hll_reserve(4)
    mbuf, moffs = pkg.pack_ints(members)
    engine.ctx.call("ske_bf_madd", 0, mbuf.ctypes.data_as(C.c_void_p), moffs.ctypes.data_as(C.c_void_p),
                    len(members), None, 0)
    sbuf, _ = pkg.pack_ints(ids)
    b = DeviceBatch(engine.ctx, n, 5)
    b.bytes.from_host(sbuf)
    b.slot.from_host(rng.integers(0, 4, n).astype(np.uint32))
    lec = keys_of("zipf37", n)
    lb = DeviceBatch(engine.ctx, n, 9)
    lb.bytes.from_host(np.frombuffer(b"".join(lec), np.uint8))
    valid = DeviceBuffer(engine.ctx, n + 16)
    engine.tally_init(0, 10)
    engine.tally_init(1, 10)

    def step(tid):
        engine.swipes_fixed_async(0, b, valid)
        engine.tally_add(tid, lb, mask=valid)

    step(0)
    engine.sync()
    v = valid.to_host(np.uint8, n)
    want = Want()
    want.add(lec, v)
    check(engine, 0, want)
    assert 0 < v.sum() < n
    g = engine.capture(lambda: step(1))
    assert engine.tally_info(1)["taken"] == 0  # recording ran nothing
    g.launch()
    g.launch()
    engine.sync()
    want.add(lec, v)
    check(engine, 1, want)
    with pytest.raises(pkg.SketchLibError) as e:  # a recorded graph points to the tally
        engine.tally_free(1)
    assert e.value.code == -13
    g.free()
    engine.tally_free(1)
    engine.tally_free(0)


# ---------------------------------------------------------------- end to end
LECTURES = ["CS%d-L%02d" % (100 + j, j) for j in range(11)]
GHOST = "GHOST-L99"  # only ids off the roster reach it
ALL_OPTS = dict(track_attended=3, track_invalid=2, capacity_log2=12, late_key="cms:late", track_late=1,
                day_profile="week")
TITLES = ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings", "Most Consistent Attendees",
          "Invalid Attendance Attempts"]


def message_stream(seed=12):
    """About 2000 payloads of the reference generator's schema over 12 lectures
    and 3 days, their counts Zipf-skewed; ids off the roster among them, one
    lecture that only those reach, host-path payloads (an escaped string, a
    float lecture_id) and undecodable ones; in two batches."""
    rng = np.random.default_rng(seed)
    roster = [int(x) for x in rng.choice(np.arange(10000, 100000), 400, replace=False)]
    off = [int(x) for x in np.setdiff1d(np.arange(10000, 100000), roster)[:3000:60]]
    p = 1.0 / np.arange(1, len(LECTURES) + 1) ** 1.1
    out = []
    for _ in range(1950):
        lec = LECTURES[int(rng.choice(len(LECTURES), p=p / p.sum()))]
        bad = rng.random() < 0.15
        ts = "2025-03-%02dT%02d:%02d:00" % (17 + int(rng.integers(0, 3)), int(rng.integers(8, 12)),
                                            int(rng.integers(0, 60)))
        out.append(json.dumps({"student_id": int(rng.choice(off if bad else roster)), "timestamp": ts,
                               "lecture_id": lec, "is_valid": not bad, "event_type": "entry"}).encode())
    for j in range(23):
        out.append(json.dumps({"student_id": off[j % 7], "timestamp": "2025-03-18T10:%02d:00" % j,
                               "lecture_id": GHOST, "is_valid": False, "event_type": "entry"}).encode())
    host = [b'{"student_id": %d, "lecture_id": "LAB\\u002d7", "timestamp": "2025-03-17T09:30:00"}' % roster[0],
            b'{"student_id": %d, "lecture_id": 3.5, "timestamp": "2025-03-18T08:15:00"}' % roster[1],
            b'{"student_id": 123.5, "lecture_id": "LAB\\u002d7", "timestamp": "2025-03-19T10:00:00"}',
            b'{"student_id": "\\u0031\\u0032345", "lecture_id": "CS100-L00", "timestamp": "2025-03-17T10:00:00"}']
    junk = [b"not json", b'{"student_id": 1}', b'{"student_id": true, "lecture_id": "L", "timestamp": "2025-03-17"}',
            b'{"student_id": 12345, "lecture_id": "L", "timestamp": "yesterday"}']
    for m in (host + junk) * 3:
        out.insert(int(rng.integers(0, len(out))), m)
    cut = len(out) // 2 + 7
    return roster, [out[:cut], out[cut:]]


def acknowledged(pkg, batch):
    """(index, lecture text) of the messages the reference's loop acknowledges
    (cassandra_row_types off): json, the three fields, fromisoformat, encode"""
    from datetime import datetime
    rows = []
    for i, m in enumerate(batch):
        try:
            d = json.loads(m.decode())
            datetime.fromisoformat(d["timestamp"])
            pkg.encode(d["student_id"])
            rows.append((i, str(d["lecture_id"])))
        except Exception:
            pass
    return rows


def rankings_of(events, k=3):
    full = [(key, e) for key, e, _ in ordered(events)]
    return {"most_attended": dict(full[:k]), "least_attended": dict(full[-k:])}


def test_messages_end_to_end(pkg, client):
    roster, batches = message_stream()
    assert sum(len(b) for b in batches) > 1950
    mbuf, moffs = pkg.pack_ints(roster)
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 10000)
    client.bf_madd_packed("bf:students", mbuf, moffs)
    only = pkg.StudentCounts(client, "a1", "i1", lecture_counts="lectures", lecture_capacity_log2=8)
    every = pkg.StudentCounts(client, "a2", "i2", lecture_counts="lectures:2", **ALL_OPTS)
    older = pkg.StudentCounts(client, "a3", "i3", **dict(ALL_OPTS, late_key="cms:late3", day_profile="week3"))
    events, valid_of, seen = Counter(), Counter(), Counter()
    for batch in batches:
        valid, status = only.update_messages("bf:students", batch)
        for sc in (every, older):
            v, s = sc.update_messages("bf:students", batch)
            assert np.array_equal(v, valid) and np.array_equal(s, status)
        rows = acknowledged(pkg, batch)
        assert np.array_equal(np.nonzero(status != -1)[0], np.asarray([r[0] for r in rows]))
        assert (status == 0).sum() > 900 and (status == 1).sum() >= 1 and (status == -1).sum() >= 1
        seen.update(status.tolist())
        for i, lec in rows:
            events[lec] += 1
            valid_of[lec] += int(valid[i])
    n_rows = sum(events.values())
    assert seen[1] == 12 and seen[-1] == 12  # the host-decoded and the undecodable payloads, three times each
    # the inputs are what the test is about: 12 lectures and the host-decoded two, untied at both cuts
    assert set(events) == set(LECTURES) | {GHOST, "LAB-7", "3.5"} and events["LAB-7"] == 6 and events["3.5"] == 3
    counts = sorted(events.values())
    assert len(set(counts[:4])) == 4 and len(set(counts[-4:])) == 4
    assert events[GHOST] == 23 and valid_of[GHOST] == 0
    assert client.exists(*["hll:unique:%s:2025-03-18" % GHOST]) == 0  # no valid swipe reached it: no HLL key
    want = {k.encode(): v for k, v in events.items()}
    want_valid = {k.encode(): v for k, v in valid_of.items() if v}
    for sc, name in ((only, "lectures"), (every, "lectures:2")):
        keys, ev, va, complete = client.tally_list(name)
        assert complete and [(k, int(e), int(v)) for k, e, v in zip(keys, ev, va)] == ordered(want, want_valid)
        info = client.tally_info(name)
        assert info["taken"] == n_rows and info["dropped_events"] == 0
        assert sc.lecture_rankings() == dict(rankings_of(events), complete=True)
        ask = sorted(events) + ["nobody"]
        ev, va = sc.lecture_events(ask)
        assert ev.tolist() == [events[x] for x in ask[:-1]] + [0]
        assert va.tolist() == [valid_of[x] for x in ask[:-1]] + [0]
    by_valid = only.lecture_rankings(k=2, by="valid")
    full = [(key, v) for key, _, v in ordered({k: events[k] for k in events}, dict(valid_of), by=1)]
    assert by_valid == {"most_attended": dict(full[:2]), "least_attended": dict(full[-2:]), "complete": True}
    ins = every.insights()
    assert [i["title"] for i in ins] == TITLES
    assert ins[2] == {"title": "Lecture Attendance Rankings", "description": "Most and least attended lectures",
                      "data": rankings_of(events), "complete": True}
    # the four older insights are what they are without the option
    assert [i for i in ins if i["title"] != TITLES[2]] == older.insights()
    assert [i["title"] for i in only.insights()] == [TITLES[2]]

    # the same messages through the drop-in processor
    pc = pkg.StudentCounts(client, "a4", "i4", lecture_counts="lectures:p",
                           **dict(ALL_OPTS, late_key="cms:late4", day_profile="week4"))
    proc = pkg.AttendanceProcessor(client, pkg.AttendanceConfig(cassandra_row_types=False), counts=pc)
    p_valid = Counter()
    for batch in batches:
        for r in proc.process_batch(batch):
            p_valid[str(r["lecture_id"])] += r["is_valid"]
    assert proc.acked == n_rows and +p_valid == +valid_of
    pins = proc.insights()  # no key list from the caller
    assert [i["title"] for i in pins] == TITLES and pins[2] == ins[2]
    assert pins == proc.insights(rank_by="events") == proc.insights(keys=["x"], rank_by="events")
    day_keys = ["hll:unique:%s:2025-03-%02d" % (lec, d) for lec in LECTURES[:3] for d in (17, 18, 19)]
    uniq = proc.insights(keys=day_keys)
    assert [i["title"] for i in uniq] == TITLES and "complete" not in uniq[2]
    assert set(uniq[2]["data"]["most_attended"]) <= set(day_keys)
    assert uniq == proc.insights(keys=day_keys, rank_by="unique")
    for lec in (LECTURES[0], GHOST, "LAB-7", "never"):
        stats = proc.get_attendance_stats(lec)
        assert stats["attendance_record_count"] == events[lec]
        assert stats["invalid_record_count"] == events[lec] - valid_of[lec]
        assert stats["unique_attendees"] <= max(valid_of[lec], 0)
    plain = pkg.AttendanceProcessor(client, pkg.AttendanceConfig(cassandra_row_types=False), counts=older)
    assert set(plain.get_attendance_stats(LECTURES[0])) == {"unique_attendees"}
    assert [i["title"] for i in plain.insights()] == [t for t in TITLES if t != TITLES[2]]
    with pytest.raises(ValueError):
        plain.insights(rank_by="events")
