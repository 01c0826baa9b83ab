"""Row log compaction on the device (``ske_rows_compact``, csrc/sketch_rows.hip)
against ``client_rows.rows_compact_oracle``: sizes around the tile, the wave and
the scan's pass on the default grid and on two workgroups; survivor patterns in
position order; columns whose halves cannot be confused; the cutoff's edges;
the reads before and after; the log's life after a compaction; errors; and
``StudentCounts(records_compact=True)``.  The conventions are tests/test_rows.py's."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge
from rows_compact_cases import Rows, patterned, wild
from test_rows import B, LECTURES, PATTERNS, SIZES, Batch, Dev, append, log_of, make_client, packed, same, take_of

pytestmark = pytest.mark.gpu

ge.load_package()
from rtsas_amd import _lib  # noqa: E402

EBUSY, EINVAL, ENOLOG = -13, -1, -42
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
COLS = ("lecture_digest", "epoch", "student_id", "is_valid")


def load(cl, name, rows):
    """the log emptied, then the rows through the fixed form"""
    cl.rows_reset(name)
    if rows.n:
        append(cl, name, "fixed", rows)


def head(info):
    return {k: info[k] for k in ("used", "taken", "refused_ids", "dropped", "overflow")}


def check_compact(cl, name, full_log, keep_since, refused=0):
    """compact ``name`` (which holds ``full_log``) and check the counts, the log and the head"""
    from rtsas_amd.client_rows import rows_compact_oracle
    want = rows_compact_oracle(full_log, keep_since)
    return check_against(cl, name, want, len(full_log[0]), keep_since, refused)


def check_against(cl, name, want, before, keep_since, refused=0):
    got = cl.rows_compact(name, keep_since)
    assert got == {"before": before, "kept": want["kept"], "superseded": want["superseded"],
                   "expired": want["expired"]}, (got, want["kept"])
    assert got["before"] == got["kept"] + got["superseded"] + got["expired"]
    assert same(log_of(cl, name), want["log"])
    info = cl.rows_info(name)
    assert head(info) == dict(used=want["kept"], taken=want["kept"] + refused, refused_ids=refused, dropped=0,
                              overflow=0), info
    assert info["used"] + info["refused_ids"] + info["dropped"] == info["taken"]
    return got


@pytest.fixture(scope="module")
def cl():
    c = make_client()
    yield c
    c.flushall()


@pytest.fixture(scope="module")
def small():
    """two workgroups: every kernel's grid-stride loop repeats from the third tile on"""
    c = make_client(2)
    yield c
    c.flushall()


# ---- sizes

SIZE_CUTOFF = -2


@pytest.fixture(scope="module")
def sized():
    """per size: rows over a key space small enough that many are written again,
    epochs on both sides of the cutoff, and the oracle's answer (computed once)"""
    from rtsas_amd.client_rows import rows_compact_oracle
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(300 + n)
        ids, _ = wild(rng.integers(0, max(n // 32, 1), n))
        rows = Rows([LECTURES[j] for j in rng.integers(0, len(LECTURES), n)], ids, rng.integers(-4, 4, n),
                    rng.integers(0, 2, n))
        out[n] = (rows, rows_compact_oracle(rows.log(), SIZE_CUTOFF))
    big = out[SIZES[-1]][1]
    assert big["superseded"] > B and big["expired"] > B and big["kept"] > 1024 * B // 4
    return out


@pytest.mark.parametrize("grid", ["default", "two"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes(cl, small, sized, n, grid):
    c = cl if grid == "default" else small
    rows, want = sized[n]
    if b"sizes" not in c._rows:
        c.rows_create("sizes", 19)  # 2^19 rows hold the largest log
    c.rows_reset("sizes")
    bad = Rows([b"x"] * 3, [0] * 3, [0] * 3, [0] * 3)
    bad.ids = [b"abc", b"", b"01"]
    append(c, "sizes", "packed", bad)  # three refused ids: the head's other counts are not the compaction's
    if n:
        append(c, "sizes", "fixed", rows)
    assert c.rows_info("sizes")["used"] == n
    check_against(c, "sizes", want, n, SIZE_CUTOFF, refused=3)


# ---- survivor patterns

@pytest.mark.parametrize("grid", ["default", "two"])
@pytest.mark.parametrize("kind", PATTERNS)
def test_patterns(cl, small, kind, grid):
    c = cl if grid == "default" else small
    if b"pat" not in c._rows:
        c.rows_create("pat", 12)
    n, cutoff = 5 * B + 3, -70000
    keep = take_of(kind, n)
    rows = patterned(keep, cutoff, seed=PATTERNS.index(kind))
    if kind == "none":  # a cutoff above every epoch
        rows = patterned(np.ones(n, bool), cutoff)
        cutoff = int(rows.ep.max()) + 1
    load(c, "pat", rows)
    got = check_compact(c, "pat", rows.log(), cutoff)
    assert got["kept"] == int(keep.sum())
    if kind == "none":
        assert got == dict(before=n, kept=0, superseded=0, expired=n)
    if kind in ("alternating", "one_per_wave", "last"):  # both ways of leaving are there
        assert got["superseded"] > 0 and got["expired"] > 0


def test_long_run_and_tile_edge(cl):
    """one row written 600 times with is_valid alternating -- a run longer than
    two tiles whose survivor carries the last write's byte -- and a run that
    begins in the last lane of one tile and ends in the first lane of the next"""
    cl.rows_create("run", 12)
    try:
        for last_valid in (0, 1):
            valid = [(j + 1 + last_valid) % 2 for j in range(600)]
            assert valid[-1] == last_valid
            other = Rows([b"o"] * 10, range(10), [5] * 10, [1] * 10)
            rows = Rows([b"o"] * 5 + [b"r"] * 600 + [b"o"] * 5, other.idv[:5].tolist() + [77] * 600 +
                        other.idv[5:].tolist(), [5] * 610, [1] * 5 + valid + [1] * 5)
            load(cl, "run", rows)
            got = check_compact(cl, "run", rows.log(), None)
            assert got == dict(before=610, kept=11, superseded=599, expired=0)
            assert cl.rows_read("run")["is_valid"].tolist() == [1] * 5 + [last_valid] + [1] * 5
        n = 2 * B + 9
        ids, lo = wild(np.arange(n))
        ids[B - 1] = ids[B]  # the run: positions B - 1 and B
        rows = Rows([b"edge"] * n, ids, [3] * n, [1] * (B - 1) + [0, 1] + [1] * (n - B - 1))
        load(cl, "run", rows)
        got = check_compact(cl, "run", rows.log(), None)
        assert got == dict(before=n, kept=n - 1, superseded=1, expired=0)
        r = cl.rows_read("run")
        assert r["student_id"][B - 1] == ids[B] and r["is_valid"][B - 1] == 1 and r["student_id"][B] == ids[B + 1]
    finally:
        cl.rows_drop("run")


# ---- columns

@pytest.mark.parametrize("r", range(8))
def test_columns_cannot_be_confused(cl, r):
    """ids and epochs whose 32-bit halves differ and are unique per row, the
    extreme ids among them, lectures of the eight lengths; ``kept & 7 == r``
    (the byte column's tail)"""
    n = B + 16
    ids, lo = wild(np.arange(n))
    ids[3], ids[n - 1] = I64_MIN, I64_MAX
    ep = ((np.arange(n, dtype=np.int64) - 100) << 32) | lo
    gone = np.zeros(n, bool)
    gone[5:5 + (8 - r)] = True  # below the cutoff
    ep[gone] = ((-1000 - np.arange(n, dtype=np.int64)[gone]) << 32) | lo[gone]
    cutoff = -100 << 32
    assert (ep[~gone] >= cutoff).all() and (ep[gone] < cutoff).all() and (ep < 0).any() and (ids < 0).any()
    assert len(set(ids.tolist())) == n and len(set(ep.tolist())) == n
    assert all((v >> 32) & 0xFFFFFFFF != v & 0xFFFFFFFF for v in ids.tolist() + ep.tolist())
    valid = (np.arange(n) * 7 // 3 % 2).astype(np.uint8)
    rows = Rows([LECTURES[i % len(LECTURES)] for i in range(n)], ids, ep, valid)
    if b"cols" not in cl._rows:
        cl.rows_create("cols", 10)
    load(cl, "cols", rows)
    got = check_compact(cl, "cols", rows.log(), cutoff)
    assert got["kept"] & 7 == r and got["expired"] == 8 - r and got["superseded"] == 0


# ---- the cutoff

def test_cutoff_edges(cl):
    n = 2 * B + 17
    rng = np.random.default_rng(5)
    ep = rng.integers(-6, 7, n)
    rows = Rows([LECTURES[j] for j in rng.integers(0, 3, n)], rng.integers(0, 40, n), ep, rng.integers(0, 2, n))
    cl.rows_create("cut", 12)
    try:
        for keep_since in (None, I64_MIN, 0, -3, 6, 7, I64_MAX):
            load(cl, "cut", rows)
            got = check_compact(cl, "cut", rows.log(), keep_since)
            r = cl.rows_read("cut")
            lo = I64_MIN if keep_since is None else keep_since
            assert got["expired"] == int((ep < lo).sum())
            assert (r["epoch"] >= lo).all()
            present = set(ep[ep >= lo].tolist())
            assert set(r["epoch"].tolist()) == present  # rows at keep_since stay, rows at keep_since - 1 go
            if keep_since in (None, I64_MIN):
                assert got["expired"] == 0 and got["superseded"] > 0
        # a superseded row below the cutoff counts as expired: the counts sum to `before`
        rows = Rows([b"a"] * 6, [7, 7, 8, 7, 8, 9], [-1, -1, 0, 0, 0, -1], [0, 1, 0, 1, 1, 1])
        load(cl, "cut", rows)
        assert check_compact(cl, "cut", rows.log(), 0) == dict(before=6, kept=2, superseded=1, expired=3)
        assert cl.rows_read("cut")["student_id"].tolist() == [7, 8]
    finally:
        cl.rows_drop("cut")


# ---- the reads before and after

def test_reads_are_unchanged(cl):
    """over a log with redeliveries that flip is_valid: every read of a window
    at or above keep_since answers after the compaction what it answered before"""
    n = 3 * B + 5
    a = Batch(n, 61, lectures=[b"one", b"two", b"three"])
    b = Batch(n, 61, lectures=[b"one", b"two", b"three"])
    flip = take_of("alternating", n)
    b.valid = np.where(flip, 1 - a.valid, a.valid).astype(np.uint8)
    redelivered = take_of("one_per_wave", n) | flip
    keep_since = -200
    cl.rows_create("eq", 12)
    try:
        append(cl, "eq", "packed", a)
        append(cl, "eq", "spans", b, mask=redelivered)

        def reads():
            out = []
            for lecture in (None, b"two"):
                for since, until in ((keep_since, None), (keep_since + 150, None), (keep_since, 300), (0, 1)):
                    sel = cl.rows_select("eq", lecture, since, until)
                    out.append([sel[k].tolist() for k in COLS])
                    for by in ("student", "lecture"):
                        for valid in (None, True, False):
                            for late in (None, 500):
                                g = cl.rows_group("eq", by, lecture, since, until, valid, late)
                                out.append((g["keys"].tolist(), g["counts"].tolist(), g["stats"]))
                    out.append(cl.rows_profile("eq", lecture, since, until, None, 500).tolist())
                    out.append(cl.rows_profile("eq", lecture, since, until, True).tolist())
            return out

        before = reads()
        got = cl.rows_compact("eq", keep_since)
        assert got["superseded"] > 64 and got["expired"] > B and got["kept"] > B
        assert len(before[0][0]) > B  # the windows hold rows
        assert reads() == before
    finally:
        cl.rows_drop("eq")


# ---- life after

def test_append_after_and_second_compact(cl):
    from rtsas_amd.client_rows import rows_compact_oracle
    n = 2 * B + 17
    a = patterned(take_of("alternating", n), -50)
    cl.rows_create("life", 12)
    try:
        load(cl, "life", a)
        first = check_compact(cl, "life", a.log(), -50)
        kept = rows_compact_oracle(a.log(), -50)["log"]
        # nothing is left to remove: the counts say so and no byte changes
        again = cl.rows_compact("life", -50)
        assert again == dict(before=first["kept"], kept=first["kept"], superseded=0, expired=0)
        assert same(log_of(cl, "life"), kept) and cl.rows_info("life")["used"] == first["kept"]
        # an append lands at `kept`; it still wins over the rows before it
        b = Rows(a.lectures[1:B:2], a.idv[1:B:2], a.ep[1:B:2], 1 - a.valid[1:B:2])
        append(cl, "life", "fixed", b)
        whole = tuple(np.concatenate([x, y]) for x, y in zip(kept, b.log()))
        assert same(log_of(cl, "life"), whole)
        assert cl.rows_info("life")["used"] == first["kept"] + b.n
        got = check_compact(cl, "life", whole, -50)
        assert got["superseded"] == b.n
        # an empty log
        cl.rows_reset("life")
        assert cl.rows_compact("life") == dict(before=0, kept=0, superseded=0, expired=0)
    finally:
        cl.rows_drop("life")


def test_recorded_append_replays_at_the_new_used(pkg, engine):
    cl = pkg.SketchClient(context=engine.ctx)
    n = B + 17
    bt = Batch(n, 41, bad=False)
    cl.rows_create("direct", 12)
    cl.rows_create("replayed", 12)
    g, d, busy = None, None, []
    try:
        append(cl, "direct", "packed", bt)  # a direct call first: it sizes the scratch the recording pins
        append(cl, "replayed", "packed", bt)
        append(cl, "replayed", "packed", bt)
        d = Dev(cl.ctx)
        lb, lo = packed(bt.lectures)
        ib, io = packed(bt.ids)
        args = [d.up(lb), d.up(lo), d.up(ib), d.up(io), d.up(bt.ep), d.up(bt.valid), None, n]
        out = _lib.RowsCompact()
        g = engine.capture(lambda: (
            cl.ctx.call("ske_rows_append_packed_async", cl.rows_rid("replayed"), *args),
            busy.append(engine.ctx.lib.ske_rows_compact(engine.ctx.ptr, cl.rows_rid("replayed"), I64_MIN,
                                                        C.byref(out)))))
        assert busy == [EBUSY]  # the compaction waits for the stream: not while a capture records
        before = log_of(cl, "replayed")
        assert before[0].size == 2 * n  # and it did nothing
        one = log_of(cl, "direct")
        got = cl.rows_compact("replayed")
        assert got["before"] == 2 * n and got["superseded"] >= n
        kept = log_of(cl, "replayed")
        g.launch()
        engine.sync()
        assert cl.rows_info("replayed")["used"] == got["kept"] + n
        assert same(log_of(cl, "replayed"), tuple(np.concatenate([x, y]) for x, y in zip(kept, one)))
    finally:
        if g is not None:
            g.free()
        if d is not None:
            d.free()
        cl.rows_drop("direct")
        cl.rows_drop("replayed")


def test_full_log_recovers_and_stays_incomplete(cl):
    cap = 1 << 8
    a = Batch(200, 71, bad=False)
    cl.rows_create("full", 8)
    try:
        append(cl, "full", "packed", a)
        append(cl, "full", "packed", a)  # the redelivery finds 56 free rows
        info = cl.rows_info("full")
        assert head(info) == dict(used=cap, taken=400, refused_ids=0, dropped=144, overflow=1)
        full = log_of(cl, "full")
        from rtsas_amd.client_rows import rows_compact_oracle
        want = rows_compact_oracle(full, None)
        got = cl.rows_compact("full")
        assert got["kept"] == want["kept"] <= 200 and got["superseded"] >= 56
        assert same(log_of(cl, "full"), want["log"])
        info = cl.rows_info("full")
        assert head(info) == dict(used=got["kept"], taken=got["kept"] + 144, refused_ids=0, dropped=144, overflow=1)
        nxt = Batch(cap - got["kept"], 72, bad=False)  # the next batch fits, to the last row
        append(cl, "full", "packed", nxt)
        info = cl.rows_info("full")
        assert head(info) == dict(used=cap, taken=cap + 144, refused_ids=0, dropped=144, overflow=1)
        assert cl.rows_select("full")["complete"] is False  # the dropped rows are still lost
    finally:
        cl.rows_drop("full")


def test_two_logs(cl):
    a = patterned(take_of("one_per_wave", 3 * B), 0, seed=1)
    b = patterned(take_of("alternating", 2 * B + 1), 0, seed=2)
    cl.rows_create("a", 10)
    cl.rows_create("b", 10)
    try:
        append(cl, "a", "fixed", a)
        append(cl, "b", "fixed", b)
        info_b = cl.rows_info("b")
        check_compact(cl, "a", a.log(), 0)
        assert same(log_of(cl, "b"), b.log()) and cl.rows_info("b") == info_b
    finally:
        cl.rows_drop("a")
        cl.rows_drop("b")


def test_errors(cl):
    lib, ptr = cl.ctx.lib, cl.ctx.ptr
    out = _lib.RowsCompact()
    assert lib.ske_rows_compact(ptr, 7, 0, C.byref(out)) == ENOLOG
    assert lib.ske_rows_compact(ptr, 8, 0, C.byref(out)) == EINVAL
    cl.rows_create("e", 8)
    try:
        assert lib.ske_rows_compact(ptr, cl.rows_rid("e"), 0, None) == EINVAL
        assert lib.ske_rows_compact(None, cl.rows_rid("e"), 0, C.byref(out)) == EINVAL
        assert lib.ske_rows_compact(ptr, cl.rows_rid("e"), 0, C.byref(out)) == 0
    finally:
        cl.rows_drop("e")


# ---- StudentCounts(records_compact=True)

def test_auto_compact(pkg, client):
    """batches whose redeliveries would overflow a 2^8-row log: with
    records_compact the log never drops a row and the exact counts are the
    oracle's; the same feed with the default overflows"""
    from rtsas_amd.client_rows import rows_group_oracle
    rng = np.random.default_rng(9)
    pool = [(b"L%d" % (k % 4), 1000 + k // 2, 1742374800 + k % 7, k % 3 != 0) for k in range(120)]
    feeds = []
    for _ in range(8):
        pick = rng.integers(0, len(pool), 90)
        feeds.append(([pool[j][0] for j in pick], [pool[j][1] for j in pick], [pool[j][2] for j in pick],
                      [pool[j][3] for j in pick]))
    batches = [(lec, [str(i).encode() for i in ids], ep, valid, None) for lec, ids, ep, valid in feeds]
    for name, auto in (("auto", True), ("plain", False)):
        sc = pkg.StudentCounts(client, "a:" + name, "i:" + name, records=name, records_capacity_log2=8,
                               records_compact=auto)
        for lec, ids, ep, valid in feeds:
            buf, offs = pkg.pack(ids)
            sc.count_packed(buf, offs, valid, times=np.asarray(ep, np.int64), lectures=lec)
        info = sc.records_info()
        assert info["overflow"] == (0 if auto else 1), info
        if auto:
            assert info["dropped"] == 0 and info["used"] <= 256
            for which, kw in (("attended", dict()), ("invalid", dict(valid=False))):
                got, want = sc.exact_counts(which), rows_group_oracle(batches, "student", **kw)
                assert got["complete"] and got["keys"].tolist() == want["keys"].tolist()
                assert got["counts"].tolist() == want["counts"].tolist()
    with pytest.raises(ValueError):
        pkg.StudentCounts(client, "a:none", "i:none").compact_records()
