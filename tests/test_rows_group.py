"""The row log's group-by on the device (``ske_rows_group``, ``ske_rows_profile``;
csrc/sketch_rows.hip) against ``client_rows.rows_group_oracle`` and
``rows_profile_oracle``: exact equality everywhere.  Sizes around the tile
(``SKE_ROWS_BLOCK``), the scan's second pass and the grid; one group over every
tile, groups of one, group boundaries on tile and wave boundaries; signed id
order; the upsert before the count; every filter; windows and lectures; the
median over the count sets of the host test; the capacity protocol; the
profile; and ``StudentCounts.exact_insights`` end to end."""
import ctypes as C
import json

import numpy as np
import pytest

import __graft_entry__ as ge
from rows_group_cases import COUNT_SETS, DAY0, LATE, hand_batches
from test_rows import Dev, make_client

pytestmark = pytest.mark.gpu

ge.load_package()
from rtsas_amd import _lib  # noqa: E402

B = _lib.SKE_ROWS_BLOCK
SCAN = 1024  # kRowsScanBlock: tiles one pass of the scan covers
EBUSY, EROWSSPACE, EINVAL = -13, -45, -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SODS = (0, LATE, 86399)
STAT_KEYS = ("rows", "n", "sum", "sumsq", "min", "max", "med_lo", "med_hi")


@pytest.fixture(scope="module")
def cl():
    c = make_client()
    yield c
    c.flushall()


@pytest.fixture(scope="module")
def small():
    """two workgroups: more than two tiles repeat every grid-stride loop"""
    c = make_client(2)
    yield c
    c.flushall()


def load(cl, name, batches, log2=None):
    n = sum(len(b[1]) for b in batches)
    for other in list(cl._rows):  # a module-wide client: the earlier tests' logs go
        cl.rows_drop(other)
    cl.rows_create(name, log2 or max(8, int(n).bit_length()))
    for lectures, ids, epochs, valid, take in batches:
        assert take is None
        cl.rows_append(name, lectures, ids, np.asarray(epochs, np.int64), valid)
    return name


def check_group(cl, name, batches, **kw):
    """rows_group == the oracle: keys, counts, every statistic; rows == rows_select's n"""
    from rtsas_amd.client_rows import rows_group_oracle
    want = rows_group_oracle(batches, **kw)
    got = cl.rows_group(name, **kw)
    assert got["keys"].dtype == want["keys"].dtype and got["counts"].dtype == np.uint64
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"]), kw
    assert {k: got["stats"][k] for k in STAT_KEYS} == {k: want["stats"][k] for k in STAT_KEYS}, kw
    assert got["stats"]["median"] == want["stats"]["median"] and got["complete"]
    sel = {k: kw[k] for k in ("lecture", "since", "until") if k in kw}
    assert got["stats"]["rows"] == cl.rows_select(name, **sel)["epoch"].size
    return got


def check_profile(cl, name, batches, **kw):
    from rtsas_amd.client_rows import rows_profile_oracle
    got = cl.rows_profile(name, **kw)
    assert got.dtype == np.uint64 and np.array_equal(got, rows_profile_oracle(batches, **kw)), kw
    return got


def random_batch(n, seed, nids=None, lectures=("a", "bb", "CS101-L01")):
    """n rows with repeats: ids of both signs and the extremes, epochs on the
    filters' boundaries (32399, 32400, -1) and around, either validity"""
    rng = np.random.default_rng(seed)
    pool = np.asarray([I64_MIN, -1, 0, I64_MAX] + rng.integers(-(1 << 62), 1 << 62, (nids or max(n // 5, 1))).tolist(),
                      dtype=object)
    ids = [str(int(v)) for v in pool[rng.integers(0, pool.size, n)]]
    marks = np.asarray([LATE - 1, LATE, -1, 86399, 86400, DAY0 + LATE, DAY0 + LATE - 1, -86400 - 1])
    ep = np.where(rng.random(n) < 0.5, marks[rng.integers(0, marks.size, n)], rng.integers(-200000, 200000, n))
    return ([lectures[j] for j in rng.integers(0, len(lectures), n)], ids, ep.astype(np.int64).tolist(),
            rng.integers(0, 2, n).tolist(), None)


@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17])
def test_sizes(cl, n):
    batches = [random_batch(n, n)]
    load(cl, "sizes", batches)
    for by in ("student", "lecture"):
        check_group(cl, "sizes", batches, by=by)
        check_group(cl, "sizes", batches, by=by, valid=True, late_from=LATE)
    check_profile(cl, "sizes", batches)


def test_scan_second_pass(cl):
    """more tiles than one pass of the scan covers, over the rows and over the groups"""
    n = SCAN * B + 1
    rng = np.random.default_rng(3)
    ids = rng.permutation(n) - n // 2  # every group of size 1: as many groups as rows
    ep = rng.integers(0, 86400, n)
    batches = [(["L"] * n, [str(int(v)) for v in ids], ep.tolist(), (ids % 3 == 0).astype(int).tolist(), None)]
    load(cl, "big", batches, 19)
    got = check_group(cl, "big", batches, by="student")
    assert got["stats"]["n"] == n and got["stats"]["max"] == 1
    check_group(cl, "big", batches, by="student", valid=False, late_from=LATE)
    got = check_group(cl, "big", batches, by="lecture")
    assert got["counts"].tolist() == [n]  # one group over every tile
    cl.rows_drop("big")


@pytest.mark.parametrize("which", ["cl", "small"])
@pytest.mark.parametrize("shape", ["one_group", "all_ones", "tiles", "waves", "mixed"])
def test_group_shapes(request, which, shape):
    c = request.getfixturevalue(which)
    n = 5 * B + 3 if which == "small" else 2 * B + 17
    i = np.arange(n)
    ids = {"one_group": np.zeros(n, np.int64), "all_ones": i, "tiles": i // B, "waves": i // 64,
           "mixed": np.where(i < B, i // 64, np.where(i < 2 * B, 1000, i))}[shape]
    # distinct (epoch, id): no row collapses, so a group's run in sorted order is its rows
    batches = [(["L"] * n, [str(int(v)) for v in ids], (DAY0 + i * 37).tolist(), (i % 2).tolist(), None)]
    load(c, "shape", batches)
    got = check_group(c, "shape", batches, by="student")
    if shape == "one_group":
        assert got["counts"].tolist() == [n]
    if shape == "all_ones":
        assert got["stats"]["n"] == n and got["stats"]["sumsq"] == n
    if shape == "tiles":
        assert got["counts"].tolist()[:2] == [B, B]
    check_group(c, "shape", batches, by="student", valid=True)
    check_group(c, "shape", batches, by="student", valid=False, late_from=LATE)
    check_group(c, "shape", batches, by="lecture")
    check_profile(c, "shape", batches, valid=True)


def test_grid_two_random(small):
    batches = [random_batch(5 * B + 3, 77), random_batch(B + 1, 78)]
    load(small, "grid2", batches)
    for by in ("student", "lecture"):
        for valid in (None, True, False):
            check_group(small, "grid2", batches, by=by, valid=valid, late_from=LATE)
    check_group(small, "grid2", batches, by="student", lecture="bb")
    check_profile(small, "grid2", batches, late_from=LATE)


def test_signed_order(cl):
    ids = [I64_MAX, 0, -1, I64_MIN, 5, -5, I64_MIN, I64_MAX, -1]
    batches = [(["L"] * len(ids), [str(v) for v in ids], list(range(len(ids))), [1] * len(ids), None)]
    load(cl, "signed", batches)
    got = check_group(cl, "signed", batches, by="student")
    assert got["keys"].tolist() == [I64_MIN, -5, -1, 0, 5, I64_MAX] and got["counts"].tolist() == [2, 1, 2, 1, 1, 2]


def test_collapse_before_count(cl):
    """a redelivered row counts once, under the validity of its last write"""
    first = (["L", "L", "M", "L"], ["7", "8", "7", "7"], [10, 10, 10, 11], [1, 1, 1, 0], None)
    batches = [first]
    load(cl, "flip", batches)
    assert check_group(cl, "flip", batches, by="student", valid=True)["counts"].tolist() == [2, 1]
    assert check_group(cl, "flip", batches, by="student", valid=False)["counts"].tolist() == [1]
    again = (["L", "L"], ["7", "8"], [10, 10], [0, 1], None)  # (L, 10, 7) flips to invalid; (L, 10, 8) repeats
    batches = [first, again]
    cl.rows_append("flip", *again[:4])
    got = check_group(cl, "flip", batches, by="student")
    assert got["counts"].tolist() == [3, 1] and got["stats"]["rows"] == 4 and cl.rows_info("flip")["used"] == 6
    valid = check_group(cl, "flip", batches, by="student", valid=True)
    invalid = check_group(cl, "flip", batches, by="student", valid=False)
    assert (valid["keys"].tolist(), valid["counts"].tolist()) == ([7, 8], [1, 1])
    assert (invalid["keys"].tolist(), invalid["counts"].tolist()) == ([7], [2])
    assert check_group(cl, "flip", batches, by="lecture", valid=False)["counts"].tolist() == [2]


def test_filters(cl):
    batches = hand_batches()
    edge = (["edge"] * 6, ["1", "2", "3", "1", "2", "4"], [LATE - 1, LATE, -1, DAY0 + LATE - 1, DAY0 + LATE, 86399],
            [1, 0, 1, 0, 1, 1], None)
    batches.append(edge)
    load(cl, "filters", batches)
    ns = set()
    for valid in (None, True, False):
        for sod in SODS:
            for by in ("student", "lecture"):
                got = check_group(cl, "filters", batches, by=by, valid=valid, late_from=sod)
                ns.add((by, got["stats"]["n"]))
            check_group(cl, "filters", batches, by="student", lecture="edge", valid=valid, late_from=sod)
            check_profile(cl, "filters", batches, valid=valid, late_from=sod)
            check_profile(cl, "filters", batches, lecture="edge", valid=valid, late_from=sod)
    assert len({n for by, n in ns if by == "student"}) > 2  # filters empty some groups: n shrinks
    # epoch -1 is second 86399 of its day: the only rows that pass the last second
    got = cl.rows_group("filters", lecture="edge", late_from=86399)
    assert (got["keys"].tolist(), got["counts"].tolist()) == ([3, 4], [1, 1])
    # a filter that empties every group
    allvalid = [(["L"] * 70, [str(i % 9) for i in range(70)], list(range(70)), [1] * 70, None)]
    load(cl, "allvalid", allvalid)
    got = check_group(cl, "allvalid", allvalid, by="student", valid=False)
    assert got["keys"].size == 0 and got["stats"] == dict(rows=70, n=0, sum=0, sumsq=0, min=0, max=0, med_lo=0,
                                                          med_hi=0, median=0.0)
    assert not check_profile(cl, "allvalid", allvalid, valid=False).any()


def test_windows_and_lectures(cl):
    batches = hand_batches()
    load(cl, "win", batches)
    for kw in (dict(lecture="CS101"), dict(lecture="solo"), dict(lecture="pair"), dict(lecture="nobody"), dict(),
               dict(since=DAY0 + 86400, until=DAY0 + 3 * 86400), dict(lecture="MA201", until=DAY0 + LATE),
               dict(since=DAY0 + 8 * 86400), dict(since=-1, until=0)):
        for by in ("student", "lecture"):
            got = check_group(cl, "win", batches, by=by, **kw)
            if by == "lecture" and "lecture" in kw:
                assert got["keys"].size == (0 if kw["lecture"] == "nobody" else 1)  # a single group
        check_profile(cl, "win", batches, **kw)
    cl.rows_reset("win")
    got = check_group(cl, "win", [], by="student")
    assert got["stats"]["rows"] == 0 and got["keys"].size == 0
    assert not check_profile(cl, "win", []).any()


@pytest.mark.parametrize("name", sorted(COUNT_SETS))
def test_median(cl, name):
    counts = COUNT_SETS[name]
    ids = np.repeat(np.arange(len(counts)) * 3 - 4, counts)
    rng = np.random.default_rng(len(counts))
    order = rng.permutation(ids.size)
    n = ids.size
    batches = [(["L"] * n, [str(int(v)) for v in ids[order]], np.arange(n).tolist(), (order % 2).tolist(), None)]
    load(cl, "median", batches)
    got = check_group(cl, "median", batches, by="student")
    assert got["counts"].tolist() == counts
    s = sorted(counts)
    assert (got["stats"]["med_lo"], got["stats"]["med_hi"]) == (s[(len(s) - 1) // 2], s[len(s) // 2])
    cl.rows_drop("median")


def raw_group(cl, name, by=0, vf=0, sod=0, cap=0, device=False, lecture=None, n_keys=0):
    """ske_rows_group with the return code: (rc, n_out, stats, complete, keys, counts)"""
    keys, counts = np.full(max(n_keys, 1), 0xABCD, np.uint64), np.full(max(n_keys, 1), 0xABCD, np.uint64)
    d = Dev(cl.ctx)
    ptrs = [d.up(keys), d.up(counts)] if device else [a.ctypes.data_as(C.c_void_p) for a in (keys, counts)]
    if cap == 0 and n_keys == 0:
        ptrs = [None, None]
    n_out, complete, st = C.c_uint64(77), C.c_int(77), _lib.RowsGroupStats(*([77] * 8))
    lec = None if lecture is None else C.c_char_p(lecture)
    rc = cl.ctx.lib.ske_rows_group(cl.ctx.ptr, cl.rows_rid(name), by, lec, 0 if lecture is None else len(lecture),
                                   I64_MIN, I64_MAX, vf, sod, *ptrs, cap, C.byref(n_out), C.byref(st),
                                   C.byref(complete), 1 if device else 0)
    if device:
        cl.ctx.call("ske_sync")
        keys, counts = d.bufs[0].to_host(np.uint64, keys.size), d.bufs[1].to_host(np.uint64, counts.size)
    d.free()
    return rc, int(n_out.value), {k: int(getattr(st, k)) for k in STAT_KEYS}, int(complete.value), keys, counts


def test_capacity_protocol(cl):
    from rtsas_amd.client_rows import rows_group_oracle
    batches = hand_batches()
    load(cl, "cap", batches)
    want = rows_group_oracle(batches, "student")
    n = want["stats"]["n"]
    stats = {k: want["stats"][k] for k in STAT_KEYS}
    for device in (False, True):
        rc, n_out, st, complete, _, _ = raw_group(cl, "cap", cap=0)
        assert (rc, n_out, st, complete) == (EROWSSPACE, n, stats, 1)  # the statistics alone
        rc, n_out, st, complete, keys, counts = raw_group(cl, "cap", cap=n - 1, device=device, n_keys=n)
        assert (rc, n_out, st, complete) == (EROWSSPACE, n, stats, 1)
        assert (keys == 0xABCD).all() and (counts == 0xABCD).all()  # no output array touched
        rc, n_out, st, complete, keys, counts = raw_group(cl, "cap", cap=n, device=device, n_keys=n)
        assert (rc, n_out, st, complete) == (0, n, stats, 1)
        assert np.array_equal(keys.view(np.int64), want["keys"]) and np.array_equal(counts, want["counts"])
    # nothing listed: cap = 0 succeeds
    rc, n_out, st, complete, _, _ = raw_group(cl, "cap", lecture=b"nobody")
    assert (rc, n_out, complete) == (0, 0, 1) and not any(st.values())
    for kw in (dict(by=2), dict(by=-1), dict(vf=3), dict(vf=-1), dict(sod=86400)):
        assert raw_group(cl, "cap", **kw)[0] == EINVAL, kw
    bins, rows, complete = np.zeros(168, np.uint64), C.c_uint64(), C.c_int()
    for vf, sod in ((3, 0), (0, 86400)):
        assert cl.ctx.lib.ske_rows_profile(cl.ctx.ptr, cl.rows_rid("cap"), None, 0, I64_MIN, I64_MAX, vf, sod,
                                           bins.ctypes.data_as(C.c_void_p), C.byref(rows), C.byref(complete)) == EINVAL
    # an overflowed log answers from what it kept, complete = 0
    cl.rows_drop("full")
    cl.rows_create("full", 8)
    rows_in = (["L"] * 300, [str(i % 7) for i in range(300)], list(range(300)), [1] * 300, None)
    cl.rows_append("full", *rows_in[:4])
    got = cl.rows_group("full")
    kept = rows_group_oracle([rows_in], "student", capacity=256)
    assert not got["complete"] and np.array_equal(got["counts"], kept["counts"]) and got["stats"]["rows"] == 256
    assert raw_group(cl, "full")[3] == 0
    cl.rows_drop("full")


def test_busy_under_capture(pkg, engine):
    """both calls wait for the stream: refused while a capture records, and nothing runs"""
    ctx = engine.ctx
    cl = pkg.SketchClient(context=ctx)
    cl.rows_create("rec", 10)
    rid = cl.rows_rid("rec")
    n = 40
    ids = np.arange(n, dtype=np.int64).view(np.uint8).reshape(n, 8)
    ep = np.arange(n, dtype=np.int64)
    lectures = pkg.pack(["L"] * n)
    cl.rows_enqueue(rid, lectures, ep, fixed_ids=ids)  # a direct call first: it sizes the scratch the recording pins
    ctx.call("ske_sync")
    b = cl._rows_bufs
    busy, g = [], None
    n_out, complete, st = C.c_uint64(), C.c_int(), _lib.RowsGroupStats()
    bins, rows = np.zeros(168, np.uint64), C.c_uint64()
    try:
        g = engine.capture(lambda: (
            ctx.call("ske_rows_append_fixed_async", rid, C.c_void_p(b["lec"].ptr), C.c_void_p(b["lec_offs"].ptr),
                     C.c_void_p(b["ids"].ptr), 8, C.c_void_p(b["epoch"].ptr), None, None, n),
            busy.append(ctx.lib.ske_rows_group(ctx.ptr, rid, 0, None, 0, I64_MIN, I64_MAX, 0, 0, None, None, 0,
                                               C.byref(n_out), C.byref(st), C.byref(complete), 0)),
            busy.append(ctx.lib.ske_rows_profile(ctx.ptr, rid, None, 0, I64_MIN, I64_MAX, 0, 0,
                                                 bins.ctypes.data_as(C.c_void_p), C.byref(rows),
                                                 C.byref(complete)))))
        assert busy == [EBUSY, EBUSY]
        assert cl.rows_info("rec")["used"] == n  # recording ran nothing
        assert cl.rows_group("rec")["stats"]["n"] == n  # and the call works again once the capture ended
    finally:
        if g is not None:
            g.free()
        cl.flushall()


def test_profile_bins(cl):
    # every weekday and hour once, then twice; one bin holding every row
    hours = np.arange(168)
    ep = np.concatenate([DAY0 + hours * 3600 + 59, DAY0 - 7 * 86400 + hours * 3600, DAY0 + 7 * 86400 + hours * 3600])
    n = ep.size
    batches = [(["L"] * n, [str(i % 5) for i in range(n)], ep.tolist(), (np.arange(n) % 2).tolist(), None)]
    load(cl, "bins", batches)
    got = check_profile(cl, "bins", batches)
    assert (got == 3).all()
    for valid in (None, True, False):
        for sod in SODS:
            check_profile(cl, "bins", batches, valid=valid, late_from=sod)
    n = 3 * B + 1
    one = [(["L"] * n, [str(i) for i in range(n)], [DAY0 + 2 * 86400 + 13 * 3600 + i for i in range(n)], None, None)]
    load(cl, "bins", one)
    got = check_profile(cl, "bins", one)
    assert got[2, 13] == n and got.sum() == n


def oracle_insights(batches, names, late_from, k):
    """the five entries from the oracles alone"""
    from rtsas_amd.analysis import DAY_NAMES, reference_rule
    from rtsas_amd.client_rows import lecture_digest, rows_group_oracle, rows_profile_oracle
    late = rows_group_oracle(batches, "student", late_from=late_from)
    twice = late["stats"]["med_lo"] + late["stats"]["med_hi"]
    late_data = {k_: c for k_, c in zip(late["keys"].tolist(), late["counts"].tolist()) if 2 * c > twice}
    per_day = rows_profile_oracle(batches).sum(axis=1)
    lec = rows_group_oracle(batches, "lecture")
    by_digest = {lecture_digest(x): x for x in names}
    ranked = sorted((-c, by_digest[d]) for d, c in zip(lec["keys"].tolist(), lec["counts"].tolist()))
    att = rows_group_oracle(batches, "student")
    thr = reference_rule(att["stats"], "median+std")
    inv = rows_group_oracle(batches, "student", valid=False)
    return [late_data, {d: int(per_day[i]) for d, i in sorted((d, i) for i, d in enumerate(DAY_NAMES)) if per_day[i]},
            {"most_attended": {x: -c for c, x in ranked[:k]}, "least_attended": {x: -c for c, x in ranked[-k:]}},
            {k_: c for k_, c in zip(att["keys"].tolist(), att["counts"].tolist()) if thr is not None and c >= thr},
            dict(zip(inv["keys"].tolist(), inv["counts"].tolist()))]


def test_exact_insights_end_to_end(pkg, client):
    from test_seen_counts import row_of, setup_bloom, stream
    roster, msgs = stream(seed=41, n_students=80)
    setup_bloom(pkg, client, roster)
    sc = pkg.StudentCounts(client, "x:att", "x:inv", records="table", records_capacity_log2=13,
                           lecture_counts="x:lectures", lecture_capacity_log2=10)
    batches, names = [], set()
    for batch in (msgs, msgs[len(msgs) // 3:], msgs[::4]):  # redelivered in part, twice
        valid, status = sc.update_messages("bf:students", batch)
        rows = [(row_of(pkg, m), ok) for m, ok, st in zip(batch, valid, status) if st != -1]
        batches.append(([r[0] for r, _ in rows], [r[2] for r, _ in rows], [r[1] for r, _ in rows],
                        [int(ok) for _, ok in rows], None))
        names |= {r[0].decode() for r, _ in rows}
    before = sc.records()
    assert sc.records_info()["used"] > before["epoch"].size > 200  # the log holds the redeliveries
    got = sc.exact_insights(lecture_k=3)
    want = oracle_insights(batches, sorted(names), sc.late_from, 3)
    assert [i["title"] for i in got] == ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings",
                                         "Most Consistent Attendees", "Invalid Attendance Attempts"]
    assert [i["data"] for i in got] == want and all(i["complete"] for i in got)
    assert len(want[0]) > 0 and len(want[3]) > 0 and len(want[4]) > 0 and len(want[1]) >= 3
    assert got[0]["description"] == f"Found {len(want[0])} students who frequently arrive after 9:00 AM"
    proc = pkg.AttendanceProcessor(client, counts=sc)
    assert proc.insights(exact=True) == got
    # the select shares the group-by's scratch: the same answer before and after
    after = sc.records()
    for col in ("lecture_digest", "epoch", "student_id", "is_valid"):
        assert np.array_equal(before[col], after[col]), col
    lec = sorted(names)[0]
    one = sc.records(lec)
    assert client.rows_group("table", by="lecture", lecture=lec)["counts"].tolist() == [one["epoch"].size]
    assert np.array_equal(sc.records(lec)["student_id"], one["student_id"])
    assert json.dumps(got[0]["data"]) and all(isinstance(k_, int) for k_ in got[4]["data"])
