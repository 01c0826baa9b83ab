"""The group merge on the device (``ske_rows_group_merge``; csrc/sketch_rows.hip,
"group merge") against ``client_rows.rows_group_merge_oracle``: exact equality
of keys, counts, every statistic and ``multi``.  Sizes around the wave and the
tile (``SKE_ROWS_BLOCK``), the scan's second pass and a grid of two workgroups;
one key over every tile, all keys distinct, group boundaries on and beside wave
and tile boundaries, zero-count entries anywhere in a group; signed and
unsigned key order; counts and totals at the 2^32 - 1 bound and the refusals
past it; the median over the count sets of the host test; the capacity
protocol; identity and order-freedom over a real log's group-by; and the merge
of a by-lecture split's group-bys against the group-by of one log."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from rows_group_cases import COUNT_SETS
from rows_merge_cases import FILTERS, merge_entries, random_batch, split_by_lecture
from test_rows import Dev, make_client

pytestmark = pytest.mark.gpu

ge.load_package()
from rtsas_amd import _lib  # noqa: E402

B = _lib.SKE_ROWS_BLOCK
SCAN = 1024  # kRowsScanBlock: tiles one pass of the scan covers
EBUSY, EROWSSPACE, EINVAL = -13, -45, -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U32_MAX = (1 << 32) - 1
STAT_KEYS = ("rows", "n", "sum", "sumsq", "min", "max", "med_lo", "med_hi")
BY = {"student": 0, "lecture": 1}
SENTINEL = 0xABCD


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


def typed(keys, by):
    k = np.ascontiguousarray(keys)
    return k.view(np.int64) if by == "student" else k.view(np.uint64)


def merge(c, by, keys, counts, device=False):
    """engine.rows_group_merge with the arrays on the host or on the device: rows_group_merge's dict"""
    from rtsas_amd.engine import DeviceBuffer, rows_group_merge
    k = np.ascontiguousarray(keys).view(np.uint64)
    v = np.ascontiguousarray(counts, dtype=np.uint64)
    if not device:
        ok, ov, stats, multi = rows_group_merge(c.ctx, BY[by], k, v, k.size, _lib.SKE_MEM_HOST)
    else:
        d, made = Dev(c.ctx), []

        def alloc(n):
            made.extend([DeviceBuffer(c.ctx, n * 8), DeviceBuffer(c.ctx, n * 8)])
            return (made[0], made[1]), (made[0].ptr, made[1].ptr)
        kp, vp = d.up(k), d.up(v)
        ok, ov, stats, multi = rows_group_merge(c.ctx, BY[by], kp.value, vp.value, k.size, _lib.SKE_MEM_DEVICE, True,
                                                alloc)
        c.ctx.call("ske_sync")
        n = stats["n"]
        ok, ov = (np.zeros(0, np.uint64),) * 2 if ok is None else (ok.to_host(np.uint64, n), ov.to_host(np.uint64, n))
        for b in made:
            b.free()
        d.free()
    return {"keys": typed(ok, by), "counts": ov, "stats": stats, "multi": multi}


def check(c, by, keys, counts, device=False):
    """the device's merge == the oracle's: keys, counts, every statistic, multi"""
    from rtsas_amd.client_rows import rows_group_merge_oracle
    want = rows_group_merge_oracle([{"keys": typed(keys, by), "counts": np.asarray(counts, np.uint64)}], by)
    got = merge(c, by, keys, counts, device)
    assert got["keys"].dtype == want["keys"].dtype and got["counts"].dtype == np.uint64
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"])
    assert {k: got["stats"][k] for k in STAT_KEYS} == {k: want["stats"][k] for k in STAT_KEYS}
    assert got["stats"]["rows"] == 0 and got["multi"] == want["multi"]
    return got


def check_all(c, keys, counts):
    for by in BY:
        for device in (False, True):
            check(c, by, keys, counts, device)


@pytest.mark.parametrize("which", ["cl", "small"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17])
def test_sizes(request, which, n):
    c = request.getfixturevalue(which)
    rng = np.random.default_rng(n)
    pool = rng.integers(I64_MIN, I64_MAX, n // 3 + 1, dtype=np.int64)
    keys = pool[rng.integers(0, pool.size, n)]
    counts = rng.integers(0, 6, n).astype(np.uint64)  # zeros among them
    check_all(c, keys, counts)


def shape_entries(shape):
    """(keys int64, counts) in key order: the sort is stable, so an entry's place in its run is the one given"""
    rng = np.random.default_rng(len(shape))
    if shape == "one_key":
        n = 3 * B + 5
        return np.full(n, -7, np.int64), rng.integers(0, 4, n)
    if shape == "distinct":
        n = 2 * B + 17
        return np.arange(n, dtype=np.int64) * 3 - n, rng.integers(0, 3, n)
    if shape == "waves":  # every run ends on a wave boundary
        n = 3 * B
        return np.arange(n, dtype=np.int64) // 64, rng.integers(0, 5, n)
    if shape == "tiles":  # every run ends on a tile boundary
        n = 3 * B
        return np.arange(n, dtype=np.int64) // B, rng.integers(1, 5, n)
    if shape == "straddle":  # runs of 65, 63, B + 1, B - 1: an end one past and one before each boundary
        runs = [65, 63, 65, 63, B + 1, B - 1, 1, 64, 1]
        return np.repeat(np.arange(len(runs), dtype=np.int64), runs), rng.integers(0, 5, sum(runs))
    if shape == "zeros":  # a zero at a group's start, middle, end; whole groups of zeros, first and last too
        groups = [[0, 0], [0, 3, 4], [2, 0, 5], [6, 1, 0], [0], [7], [0, 0, 0, 9, 0, 0], [1, 1], [0, 0, 0]] * 70
        counts = np.asarray([v for g in groups for v in g])
        return np.repeat(np.arange(len(groups), dtype=np.int64) - 300, [len(g) for g in groups]), counts
    raise KeyError(shape)


@pytest.mark.parametrize("which", ["cl", "small"])
@pytest.mark.parametrize("shape", ["one_key", "distinct", "waves", "tiles", "straddle", "zeros"])
def test_shapes(request, which, shape):
    c = request.getfixturevalue(which)
    keys, counts = shape_entries(shape)
    counts = counts.astype(np.uint64)
    got = check(c, "student", keys, counts)
    check(c, "lecture", keys, counts, device=True)
    if shape == "one_key":
        assert got["counts"].tolist() == [int(counts.sum())] and got["multi"] == 1
    if shape == "tiles":
        assert got["stats"]["n"] == 3 and got["multi"] == 3
    if shape == "zeros":
        assert got["stats"]["n"] == 6 * 70  # the all-zero groups are not listed
    # the same entries in another order: the same answer
    order = np.random.default_rng(5).permutation(keys.size)
    again = check(c, "student", keys[order], counts[order], device=True)
    assert np.array_equal(again["keys"], got["keys"]) and np.array_equal(again["counts"], got["counts"])
    assert again["stats"] == got["stats"] and again["multi"] == got["multi"]


@pytest.mark.parametrize("which", ["cl", "small"])
def test_signed_and_unsigned_order(request, which):
    c = request.getfixturevalue(which)
    keys = np.asarray([I64_MAX, 0, -1, I64_MIN, 0, -1, I64_MIN, I64_MAX, -1], np.int64)
    counts = np.asarray([1, 2, 3, 4, 5, 6, 7, 8, 0], np.uint64)
    for device in (False, True):
        got = check(c, "student", keys, counts, device)
        assert got["keys"].tolist() == [I64_MIN, -1, 0, I64_MAX] and got["counts"].tolist() == [11, 9, 7, 9]
        got = check(c, "lecture", keys, counts, device)  # the same bit patterns, compared unsigned
        assert got["keys"].tolist() == [0, I64_MAX, 1 << 63, (1 << 64) - 1] and got["counts"].tolist() == [7, 9, 11, 9]
        assert got["multi"] == 4


def test_scan_second_pass(cl):
    """more tiles than one pass of the scan covers, over the entries and over the groups"""
    n = SCAN * B + 1
    rng = np.random.default_rng(3)
    keys = (rng.permutation(n) - n // 2).astype(np.int64)  # as many groups as entries
    got = check(cl, "student", keys, np.ones(n, np.uint64))
    assert got["stats"]["n"] == n and got["stats"]["max"] == 1 and got["multi"] == 0
    keys = rng.integers(-3, 4, n).astype(np.int64)  # 7 keys: few groups, long runs over many tiles
    got = check(cl, "lecture", keys, rng.integers(0, 4, n).astype(np.uint64), device=True)
    assert got["stats"]["n"] == 7 and got["multi"] == 7


def raw_merge(c, by, keys, counts, cap, device=False, n_keys=0, n_in=None):
    """ske_rows_group_merge with the return code: (rc, n_out, stats, multi, keys, counts); the outputs
    are prefilled with a sentinel"""
    k = np.ascontiguousarray(keys).view(np.uint64)
    v = np.ascontiguousarray(counts, dtype=np.uint64)
    ok, ov = np.full(max(n_keys, 1), SENTINEL, np.uint64), np.full(max(n_keys, 1), SENTINEL, np.uint64)
    d = Dev(c.ctx)
    if device:
        ins, outs = [d.up(k), d.up(v)], [d.up(ok), d.up(ov)]
    else:
        ins, outs = [a.ctypes.data_as(C.c_void_p) for a in (k, v)], [a.ctypes.data_as(C.c_void_p) for a in (ok, ov)]
    if cap == 0 and n_keys == 0:
        outs = [None, None]
    n_out, multi, st = C.c_uint64(77), C.c_uint64(77), _lib.RowsGroupStats(*([77] * 8))
    rc = c.ctx.lib.ske_rows_group_merge(c.ctx.ptr, by, *ins, k.size if n_in is None else n_in, *outs, cap,
                                        C.byref(n_out), C.byref(st), C.byref(multi), 1 if device else 0)
    if device:
        c.ctx.call("ske_sync")
        ok, ov = d.bufs[2].to_host(np.uint64, ok.size), d.bufs[3].to_host(np.uint64, ov.size)
    d.free()
    return rc, int(n_out.value), {s: int(getattr(st, s)) for s in STAT_KEYS}, int(multi.value), ok, ov


def test_values_at_the_bound(cl, small):
    for c in (cl, small):
        # one entry of 2^32 - 1
        got = check(c, "student", np.asarray([4, 9], np.int64), np.asarray([U32_MAX, 0], np.uint64))
        assert got["counts"].tolist() == [U32_MAX] and got["stats"]["sumsq"] == U32_MAX * U32_MAX
        # many entries over three tiles summing to exactly 2^32 - 1, in one key and in many
        n = 2 * B + 9
        counts = np.full(n, U32_MAX // n, np.uint64)
        counts[-1] += U32_MAX - int(counts.sum())
        assert int(counts.sum()) == U32_MAX
        for keys in (np.zeros(n, np.int64), np.arange(n, dtype=np.int64) % 5 - 2):
            for device in (False, True):
                got = check(c, "student", keys, counts, device)
                assert got["stats"]["sum"] == U32_MAX
        # past it: refused, nothing written
        over = counts.copy()
        over[3] += 1
        wide = np.asarray([1, 1 << 32, 0, 2], np.uint64)
        huge = np.asarray([(1 << 64) - 1, 1, (1 << 64) - 1, 2], np.uint64)  # a 64-bit total would wrap to a small one
        for keys, bad, by in ((np.arange(n, dtype=np.int64) % 5, over, 0), (np.arange(4, dtype=np.int64), wide, 1),
                              (np.arange(4, dtype=np.int64), huge, 0), (np.arange(4, dtype=np.int64), wide // 2, 2),
                              (np.arange(4, dtype=np.int64), wide // 2, -1)):
            for device in (False, True):
                rc, n_out, st, multi, ok, ov = raw_merge(c, by, keys, bad, cap=8, device=device, n_keys=8)
                assert rc == EINVAL, (by, device)
                assert (ok == SENTINEL).all() and (ov == SENTINEL).all()  # no output array touched
                assert n_out == 0 and multi == 0 and not any(st.values())
        # and the call works again afterwards
        check(c, "lecture", np.arange(4, dtype=np.int64), wide // 2)


@pytest.mark.parametrize("name", sorted(COUNT_SETS))
def test_median(cl, name):
    sums = COUNT_SETS[name]
    rng = np.random.default_rng(len(sums) + sums[0])
    keys, counts = [], []
    for j, total in enumerate(sums):  # each merged count split at random into 1 to 4 entries
        cuts = sorted(rng.integers(0, total + 1, int(rng.integers(0, 4))).tolist())
        pieces = np.diff([0] + cuts + [total]).tolist()
        keys += [j * 3 - 4] * len(pieces)
        counts += pieces
    order = rng.permutation(len(keys))
    got = check(cl, "student", np.asarray(keys, np.int64)[order], np.asarray(counts, np.uint64)[order])
    assert got["counts"].tolist() == sums
    s = sorted(sums)
    assert (got["stats"]["med_lo"], got["stats"]["med_hi"]) == (s[(len(s) - 1) // 2], s[len(s) // 2])


def test_capacity_protocol(cl):
    from rtsas_amd.client_rows import rows_group_merge_oracle
    rng = np.random.default_rng(9)
    keys = rng.integers(-40, 40, 3 * B + 1).astype(np.int64)
    counts = rng.integers(0, 3, keys.size).astype(np.uint64)
    want = rows_group_merge_oracle([{"keys": keys, "counts": counts}], "student")
    n = want["stats"]["n"]
    stats = {k: want["stats"][k] for k in STAT_KEYS}
    for device in (False, True):
        rc, n_out, st, multi, _, _ = raw_merge(cl, 0, keys, counts, cap=0, device=device)
        assert (rc, n_out, st, multi) == (EROWSSPACE, n, stats, want["multi"])  # the statistics alone
        rc, n_out, st, multi, ok, ov = raw_merge(cl, 0, keys, counts, cap=n - 1, device=device, n_keys=n)
        assert (rc, n_out, st, multi) == (EROWSSPACE, n, stats, want["multi"])
        assert (ok == SENTINEL).all() and (ov == SENTINEL).all()  # no output array touched
        rc, n_out, st, multi, ok, ov = raw_merge(cl, 0, keys, counts, cap=n, device=device, n_keys=n)
        assert (rc, n_out, st, multi) == (0, n, stats, want["multi"])
        assert np.array_equal(ok.view(np.int64), want["keys"]) and np.array_equal(ov, want["counts"])
        # nothing listed: cap = 0 succeeds
        rc, n_out, st, multi, _, _ = raw_merge(cl, 0, keys, np.zeros(keys.size, np.uint64), cap=0, device=device)
        assert (rc, n_out, multi) == (0, 0, 0) and not any(st.values())
        # no entry at all: everything zero, the pointers are not looked at
        rc, n_out, st, multi, ok, ov = raw_merge(cl, 1, keys, counts, cap=4, device=device, n_keys=4, n_in=0)
        assert (rc, n_out, multi) == (0, 0, 0) and not any(st.values()) and (ok == SENTINEL).all()
    lib, ptr = cl.ctx.lib, cl.ctx.ptr
    n_out, multi, st = C.c_uint64(), C.c_uint64(), _lib.RowsGroupStats()
    kp, vp = keys.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)
    assert lib.ske_rows_group_merge(ptr, 0, None, None, 0, None, None, 0, C.byref(n_out), C.byref(st),
                                    C.byref(multi), 0) == 0
    for args in ((0, None, vp, 5, None, None, 0, C.byref(n_out), C.byref(st), C.byref(multi), 0),
                 (0, kp, None, 5, None, None, 0, C.byref(n_out), C.byref(st), C.byref(multi), 0),
                 (0, kp, vp, 5, None, None, 0, None, C.byref(st), C.byref(multi), 0),
                 (0, kp, vp, 5, None, None, 0, C.byref(n_out), None, C.byref(multi), 0),
                 (0, kp, vp, 5, None, None, 0, C.byref(n_out), C.byref(st), None, 0),
                 (0, kp, vp, 5, None, None, 3, C.byref(n_out), C.byref(st), C.byref(multi), 0),
                 (0, kp, vp, (1 << 28) + 1, None, None, 0, C.byref(n_out), C.byref(st), C.byref(multi), 0)):
        assert lib.ske_rows_group_merge(ptr, *args) == EINVAL, args[:4]


def test_busy_under_capture(pkg, engine):
    """the call waits for the stream: refused while a capture records, and it works again afterwards"""
    ctx = engine.ctx
    c = pkg.SketchClient(context=ctx)
    c.rows_create("rec", 10)
    rid = c.rows_rid("rec")
    n = 40
    ids = np.arange(n, dtype=np.int64).view(np.uint8).reshape(n, 8)
    ep = np.arange(n, dtype=np.int64)
    c.rows_enqueue(rid, pkg.pack(["L"] * n), ep, fixed_ids=ids)  # a direct call first: it sizes the scratch the recording pins
    ctx.call("ske_sync")
    b = c._rows_bufs
    keys, counts = np.asarray([3, 1, 3], np.int64), np.asarray([1, 2, 3], np.uint64)
    busy, g = [], None
    n_out, multi, st = C.c_uint64(), C.c_uint64(), _lib.RowsGroupStats()
    try:
        g = engine.capture(lambda: (
            ctx.call("ske_rows_append_fixed_async", rid, C.c_void_p(b["lec"].ptr), C.c_void_p(b["lec_offs"].ptr),
                     C.c_void_p(b["ids"].ptr), 8, C.c_void_p(b["epoch"].ptr), None, None, n),
            busy.append(ctx.lib.ske_rows_group_merge(ctx.ptr, 0, keys.ctypes.data_as(C.c_void_p),
                                                     counts.ctypes.data_as(C.c_void_p), 3, None, None, 0,
                                                     C.byref(n_out), C.byref(st), C.byref(multi), 0))))
        assert busy == [EBUSY] and n_out.value == 0
    finally:
        if g is not None:
            g.free()
    try:
        got = c.rows_group_merge("student", keys, counts)
        assert (got["keys"].tolist(), got["counts"].tolist(), got["multi"]) == ([1, 3], [2, 4], 1)
    finally:
        c.flushall()


def load(c, name, batches):
    n = sum(len(b[1]) for b in batches)
    c.rows_create(name, max(8, int(n).bit_length()))
    for lectures, ids, epochs, valid, take in batches:
        c.rows_append(name, lectures, ids, np.asarray(epochs, np.int64), valid)
    return name


def drop_logs(c):
    for other in list(c._rows):  # a module-wide client: the earlier tests' logs go
        c.rows_drop(other)


@pytest.mark.parametrize("which", ["cl", "small"])
def test_identity_and_order_freedom(request, which):
    """the merge of one rows_group output alone is that output; shuffled, the same"""
    c = request.getfixturevalue(which)
    drop_logs(c)
    load(c, "one", [random_batch(2 * B + 17, 31)])
    for by in BY:
        for kw in ({}, dict(valid=False), dict(late_from=FILTERS["late"]["late_from"])):
            g = c.rows_group("one", by=by, **kw)
            got = c.rows_group_merge(by, g["keys"], g["counts"])
            assert got["keys"].dtype == g["keys"].dtype
            assert np.array_equal(got["keys"], g["keys"]) and np.array_equal(got["counts"], g["counts"])
            assert got["stats"] == dict(g["stats"], rows=0) and got["multi"] == 0
            order = np.random.default_rng(2).permutation(g["keys"].size)
            again = c.rows_group_merge(by, g["keys"][order], g["counts"][order])
            assert np.array_equal(again["keys"], got["keys"]) and np.array_equal(again["counts"], got["counts"])
            assert again["stats"] == got["stats"] and again["multi"] == 0
    drop_logs(c)


@pytest.mark.parametrize("world", [2, 4])
def test_against_the_group_by_of_one_log(cl, world):
    """W logs hold a by-lecture split, a further one everything: the merge of the W group-bys is its group-by"""
    drop_logs(cl)
    batches = [random_batch(4 * B + 3, 40 + world)]
    parts = split_by_lecture(batches, world, lambda lec, w: sum(str(lec).encode()) % w)
    assert sum(1 for p in parts if p) >= 2
    for r, p in enumerate(parts):
        load(cl, "part%d" % r, p)  # a part without rows is an empty log
    load(cl, "all", batches)
    for by in BY:
        for which, kw in FILTERS.items():
            gs = [cl.rows_group("part%d" % r, by=by, **kw) for r in range(world)]
            want = cl.rows_group("all", by=by, **kw)
            keys, counts = merge_entries(gs)
            got = cl.rows_group_merge(by, typed(keys, by), counts)
            assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"]), (by, which)
            rows = sum(g["stats"]["rows"] for g in gs)
            assert dict(got["stats"], rows=rows) == want["stats"], (by, which)
            if by == "lecture":
                assert got["multi"] == 0  # no lecture lies in two logs
    drop_logs(cl)
