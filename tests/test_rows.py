"""Row logs on the device (csrc/sketch_rows.hip) against the Python restatement
``client_rows.rows_oracle``: the append's stable placement over sizes around
the tile (``SKE_ROWS_BLOCK``), the scan's pass and the grid; statuses and masks
in patterns with refused ids interleaved; the three append forms; capacity;
the select's match, order, upsert and capacity protocol; a recorded append
replayed; reset; two logs side by side."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

ge.load_package()
from rtsas_amd import _lib  # noqa: E402

B = _lib.SKE_ROWS_BLOCK  # items per tile of an append: the shapes below are derived from it
SCAN = 1024  # threads of the one workgroup that scans the tile counts (kRowsScanBlock)
SIZES = (0, 1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 17, SCAN * B + 1)
PATTERNS = ("all", "none", "alternating", "one_per_wave", "first", "last")
LECTURES = [b"", b"L", b"CS101-L", b"CS101-L0", b"CS101-L01", b"x" * 32, b"y" * 33, "Ünï-7".encode()]
BAD_IDS = [b"", b"-", b"-0", b"00", b"01", b"+1", b" 1", b"1 ", b"1.0", b"1e3", b"9223372036854775808",
           b"-9223372036854775809", b"12345678901234567890", b"1" * 32, b"12\xc3\xa9", b"abc"]
EBUSY, EROWSSPACE, EINVAL = -13, -45, -1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def make_client(grid=None):
    """a client on a context opened with SKE_ROWS_GRID (ske_open reads it)"""
    pkg = ge.load_package()
    if grid is not None:
        os.environ["SKE_ROWS_GRID"] = str(grid)
    try:
        return pkg.SketchClient(context=pkg.Context(0))
    finally:
        os.environ.pop("SKE_ROWS_GRID", None)


@pytest.fixture(scope="module")
def cl():
    c = make_client()
    yield c
    c.flushall()


@pytest.fixture(scope="module")
def small():
    """two workgroups: a batch of more than two tiles repeats the grid-stride loop"""
    c = make_client(2)
    yield c
    c.flushall()


def take_of(kind, n):
    i = np.arange(n)
    return {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 1,
            "one_per_wave": i % 64 == 37, "first": i == 0, "last": i == n - 1}[kind]


class Batch:
    """n rows: lectures of eight lengths, integer ids of every magnitude as
    text with a refused text at every fifth row, epochs on both sides of 0."""

    def __init__(self, n, seed, bad=True, lo=-(1 << 62), hi=1 << 62, lectures=LECTURES):
        rng = np.random.default_rng(seed)
        self.n = n
        self.lectures = [lectures[j] for j in rng.integers(0, len(lectures), n)]
        mags = rng.integers(0, 63, n)
        vals = (rng.integers(lo, hi, n) >> mags) if n else np.zeros(0, np.int64)
        self.ids = [str(int(v)).encode() for v in vals]
        if bad:
            for i in range(3, n, 5):
                self.ids[i] = BAD_IDS[(i // 5) % len(BAD_IDS)]
        self.ep = rng.integers(-1000, 1000, n).astype(np.int64)
        self.valid = rng.integers(0, 2, n).astype(np.uint8)

    def oracle_rows(self, take=None):
        return (self.lectures, self.ids, self.ep.tolist(), self.valid.tolist(), None if take is None else take.tolist())

    def ok(self):
        from rtsas_amd.client_rows import parse_id
        return np.asarray([parse_id(i) is not None for i in self.ids], bool)


def packed(items, align=0):
    blob = bytes(align) + b"".join(items)
    offs = np.zeros(len(items) + 1, np.uint32)
    offs[1:] = np.cumsum(np.asarray([len(x) for x in items], np.int64))
    return np.frombuffer(blob + bytes(8), np.uint8), offs + np.uint32(align)


class Dev:
    """device copies of host arrays, freed together"""

    def __init__(self, ctx):
        from rtsas_amd.engine import DeviceBuffer
        self.ctx, self.bufs, self.DeviceBuffer = ctx, [], DeviceBuffer

    def up(self, arr):
        if arr is None:
            return None
        a = np.ascontiguousarray(arr)
        b = self.DeviceBuffer(self.ctx, a.nbytes + 64)
        b.from_host(a)
        self.bufs.append(b)
        return C.c_void_p(b.ptr)

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def u8(mask):
    return None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)


def append(cl, name, form, bt, mask=None, status=None, align=0, width=8):
    """one batch through one of the three forms; mask: rows with 1, status: rows with 0"""
    d, rid, n = Dev(cl.ctx), cl.rows_rid(name), bt.n
    try:
        ep, valid, m = d.up(bt.ep), d.up(bt.valid), d.up(u8(mask))
        if form == "spans":
            # one blob, each row's lecture then its id, as the parse leaves its columns
            ll = np.asarray([len(x) for x in bt.lectures], np.uint32)
            il = np.asarray([len(x) for x in bt.ids], np.uint32)
            blob = bytes(align) + b"".join(a + b for a, b in zip(bt.lectures, bt.ids)) + bytes(8)
            ends = np.cumsum(ll.astype(np.int64) + il.astype(np.int64))
            ls = (ends - il - ll + align).astype(np.uint32)
            is_ = (ends - il + align).astype(np.uint32)
            cl.ctx.call("ske_rows_append_spans_async", rid, d.up(np.frombuffer(blob, np.uint8)), d.up(ls), d.up(ll),
                        d.up(is_), d.up(il), d.up(u8(status)), ep, valid, m, n)
        else:
            assert status is None
            lb, lo = packed(bt.lectures, align)
            if form == "packed":
                ib, io = packed(bt.ids, (align * 3) % 8)
                cl.ctx.call("ske_rows_append_packed_async", rid, d.up(lb), d.up(lo), d.up(ib), d.up(io), ep, valid,
                            m, n)
            else:
                vals = np.asarray([int(i) for i in bt.ids], np.int64).astype("<i8" if width == 8 else "<i4")
                raw = np.frombuffer(bytes(align) + vals.tobytes() + bytes(8), np.uint8)
                if align:  # an id column that starts off a word boundary
                    b = d.DeviceBuffer(cl.ctx, raw.nbytes + 64)
                    b.from_host(raw)
                    d.bufs.append(b)
                    ids = C.c_void_p(b.ptr + align)
                else:
                    ids = d.up(raw)
                cl.ctx.call("ske_rows_append_fixed_async", rid, d.up(lb), d.up(lo), ids, width, ep, valid, m, n)
        cl.ctx.call("ske_sync")
    finally:
        d.free()


def log_of(cl, name):
    r = cl.rows_read(name)
    return r["lecture_digest"], r["epoch"], r["student_id"], r["is_valid"]


def same(got, want):
    return all(np.array_equal(g, w) and g.dtype == w.dtype for g, w in zip(got, want))


def check_info(info, used, taken, refused, dropped=0):
    assert (info["used"], info["taken"], info["refused_ids"], info["dropped"]) == (used, taken, refused, dropped), info
    assert info["used"] + info["refused_ids"] + info["dropped"] == info["taken"]
    assert info["overflow"] == (1 if dropped else 0)


@pytest.fixture(scope="module")
def sized():
    """per size: the batch, which ids parse, and the oracle's log of the whole batch (computed once)"""
    from rtsas_amd.client_rows import rows_oracle
    out = {}
    for n in SIZES:
        bt = Batch(n, 100 + n)
        out[n] = (bt, bt.ok(), rows_oracle([bt.oracle_rows()])["log"])
    return out


@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_patterns(cl, sized, n):
    """the log after one append equals the oracle's arrival-order log, for every
    pattern as a mask (packed) and as a status column (spans)"""
    bt, ok, full = sized[n]
    if b"sizes" not in cl._rows:
        cl.rows_create("sizes", 19)  # 2^19 rows hold the largest batch
    for kind in PATTERNS:
        take = take_of(kind, n)
        want = tuple(col[take[ok]] for col in full)  # the oracle's rows of the taken, parseable items, in order
        for form, kw in (("packed", dict(mask=take)), ("spans", dict(status=~take))):
            cl.rows_reset("sizes")
            append(cl, "sizes", form, bt, **kw)
            assert same(log_of(cl, "sizes"), want), (kind, form)
            check_info(cl.rows_info("sizes"), int((take & ok).sum()), int(take.sum()), int((take & ~ok).sum()))
    # status and mask together: both must let the row through
    st, mk = take_of("alternating", n), take_of("one_per_wave", n) | take_of("first", n) | (np.arange(n) % 3 == 0)
    cl.rows_reset("sizes")
    append(cl, "sizes", "spans", bt, status=st, mask=mk)
    take = ~st & mk
    assert same(log_of(cl, "sizes"), tuple(col[take[ok]] for col in full))


@pytest.mark.parametrize("n", [2 * B + 17, 5 * B + 3])
def test_small_grid(small, n):
    """more tiles than workgroups: the grid-stride loop repeats, in all three kernels' forms"""
    from rtsas_amd.client_rows import rows_oracle
    small.rows_create("g", 12)
    try:
        bt = Batch(n, 7 + n)
        take = take_of("alternating", n) | take_of("one_per_wave", n)
        want = rows_oracle([bt.oracle_rows(take), bt.oracle_rows()])
        append(small, "g", "packed", bt, mask=take)
        append(small, "g", "spans", bt)
        assert same(log_of(small, "g"), want["log"])
        info = small.rows_info("g")
        check_info(info, want["log"][0].size, want["taken"], want["refused_ids"])
        for lecture in (None, LECTURES[2]):
            got = small.rows_select("g", lecture)
            assert same((got["lecture_digest"], got["epoch"], got["student_id"], got["is_valid"]),
                        rows_oracle([bt.oracle_rows(take), bt.oracle_rows()], lecture=lecture)["select"])
    finally:
        small.rows_drop("g")


def test_three_forms_identical(cl):
    """the same rows through packed, spans and fixed give the same log; spans at
    every start alignment, packed ids of every length 1..20, fixed ids of both widths"""
    from rtsas_amd.client_rows import rows_oracle
    n = 2 * B + 17
    cl.rows_create("forms", 12)
    try:
        for width, lo, hi in ((8, -(1 << 62), 1 << 62), (4, -(1 << 31), 1 << 31)):
            bt = Batch(n, 11 + width, bad=False, lo=lo, hi=hi)
            edge = [I64_MIN, I64_MAX, 0, -1] if width == 8 else [-(1 << 31), (1 << 31) - 1, 0, -1]
            bt.ids[:4] = [str(v).encode() for v in edge]
            want = rows_oracle([bt.oracle_rows()])["log"]
            mask = take_of("alternating", n)
            for align in range(8):
                for form in ("spans", "packed", "fixed"):
                    cl.rows_reset("forms")
                    append(cl, "forms", form, bt, align=align, width=width)
                    assert same(log_of(cl, "forms"), want), (form, align, width)
            cl.rows_reset("forms")
            for form in ("spans", "packed", "fixed"):
                append(cl, "forms", form, bt, mask=mask, width=width)
            got = log_of(cl, "forms")
            k = int(mask.sum())
            assert got[0].size == 3 * k
            assert all(np.array_equal(c[:k], c[k:2 * k]) and np.array_equal(c[:k], c[2 * k:]) for c in got)
        # ids of every length 1..20, both signs, at every alignment of the packed column
        ids = [b"1234567890123456789"[:k] for k in range(1, 20)] + [b"-" + b"1234567890123456789"[:k]
                                                                     for k in range(1, 20)]
        ids += [b"9223372036854775807", b"-9223372036854775808", b"0"]
        bt = Batch(len(ids), 3, bad=False)
        bt.ids = ids
        want = rows_oracle([bt.oracle_rows()])["log"]
        assert want[2].tolist() == [int(i) for i in ids]
        for align in range(8):
            for form in ("packed", "spans"):
                cl.rows_reset("forms")
                append(cl, "forms", form, bt, align=align)
                assert same(log_of(cl, "forms"), want), (form, align)
        # widths other than 4 and 8 are refused
        d = Dev(cl.ctx)
        p = d.up(np.zeros(64, np.uint8))
        for width in (0, 1, 5, 16):
            assert cl.ctx.lib.ske_rows_append_fixed_async(cl.ctx.ptr, cl.rows_rid("forms"), p, p, p, width, p, None,
                                                          None, 1) == EINVAL
        d.free()
    finally:
        cl.rows_drop("forms")


def test_capacity(cl):
    """the smallest log: a batch that ends exactly at capacity, one that crosses
    it in the middle of a wavefront, one that arrives when it is full"""
    from rtsas_amd.client_rows import rows_oracle
    cap = 1 << 8
    cl.rows_create("cap", 8)
    try:
        a, b = Batch(100, 1, bad=False), Batch(cap - 100, 2, bad=False)
        append(cl, "cap", "packed", a)
        append(cl, "cap", "spans", b)
        check_info(cl.rows_info("cap"), cap, cap, 0)  # full, nothing dropped
        assert same(log_of(cl, "cap"), rows_oracle([a.oracle_rows(), b.oracle_rows()])["log"])
        assert cl.rows_select("cap")["complete"]
        cl.rows_reset("cap")
        batches = [Batch(200, 3), Batch(150, 4), Batch(10, 5)]  # refused ids among them
        kept = [sum(bt.ok()[:k]) for bt, k in zip(batches, (200, 150, 10))]
        assert kept[0] < cap < kept[0] + kept[1] and (cap - kept[0]) % 64  # the crossing falls inside a wavefront
        for bt in batches:
            append(cl, "cap", "packed", bt)
        want = rows_oracle([bt.oracle_rows() for bt in batches], capacity=cap)
        assert same(log_of(cl, "cap"), want["log"])  # the prefix that fits, in order
        info = cl.rows_info("cap")
        check_info(info, cap, want["taken"], want["refused_ids"], want["dropped"])
        assert info["dropped"] == sum(kept) - cap and info["overflow"] == 1
        sel = cl.rows_select("cap")
        assert sel["complete"] is False
        assert same((sel["lecture_digest"], sel["epoch"], sel["student_id"], sel["is_valid"]),
                    rows_oracle([bt.oracle_rows() for bt in batches], capacity=cap)["select"])
        cl.rows_reset("cap")  # overflow is sticky until a reset
        assert cl.rows_info("cap")["overflow"] == 0 and cl.rows_select("cap")["complete"]
    finally:
        cl.rows_drop("cap")


def raw_select(cl, name, lecture, since, until, cap, device=False):
    """ske_rows_select itself: (rc, n_out, complete, the four arrays as they are afterwards)"""
    cols = [np.full(max(cap, 1) * np.dtype(t).itemsize, 0xAB, np.uint8).view(t)
            for t in (np.uint64, np.int64, np.int64, np.uint8)]
    d = Dev(cl.ctx)
    ptrs = [d.up(c) for c in cols] if device else [c.ctypes.data_as(C.c_void_p) for c in cols]
    if cap == 0:
        ptrs = [None] * 4
    n_out, complete = C.c_uint64(77), C.c_int(77)
    lec = None if lecture is None else C.c_char_p(lecture)
    rc = cl.ctx.lib.ske_rows_select(cl.ctx.ptr, cl.rows_rid(name), lec, 0 if lecture is None else len(lecture),
                                    since, until, *ptrs, cap, C.byref(n_out), C.byref(complete), 1 if device else 0)
    if device and cap:
        cl.ctx.call("ske_sync")
        cols = [b.to_host(c.dtype, c.size) for b, c in zip(d.bufs, cols)]
    d.free()
    return rc, int(n_out.value), int(complete.value), cols


@pytest.fixture(scope="module")
def table(cl):
    """a log of three batches: a lecture present only in the first tile and one
    only in the last, ids and epochs at the edges, and rows written again --
    inside one wavefront, across tiles of one batch and across calls -- with
    another is_valid"""
    from rtsas_amd.client_rows import lecture_digest
    names = [b"T%d" % i for i in range(64)]
    lo = next(x for x in names if lecture_digest(x) < 2 ** 63)
    hi = next(x for x in names if lecture_digest(x) >= 2 ** 63)
    n = 3 * B + 5
    a = Batch(n, 21, lectures=[lo, hi, b"mid"])
    a.lectures[:B] = [b"first-only" if i % 3 == 0 else x for i, x in enumerate(a.lectures[:B])]
    a.lectures[-B // 2:] = [b"last-only" if i % 2 == 0 else x for i, x in enumerate(a.lectures[-B // 2:])]
    edges = [0, -1, 1, (1 << 31) - 1, 1 << 31, -(1 << 31), -(1 << 31) - 1, 1 << 62, -(1 << 62), I64_MAX, I64_MIN]
    for j, v in enumerate(edges):  # one lecture, one second: the id order decides
        a.lectures[10 + j], a.ids[10 + j], a.ep[10 + j] = lo, str(v).encode(), -5
    for j, e in enumerate((-3, -2, -1, 0, 1, 2)):  # one id, seconds around 0
        a.lectures[40 + j], a.ids[40 + j], a.ep[40 + j] = hi, b"77", e

    def again(bt, src, dst, flip=True):
        bt.lectures[dst], bt.ids[dst], bt.ep[dst] = a.lectures[src], a.ids[src], a.ep[src]
        bt.valid[dst] = 1 - a.valid[src] if flip else a.valid[src]
    again(a, 64, 70)            # in one wavefront
    again(a, 70, 75, flip=False)  # three writes of one row: the last one's value stays
    again(a, 12, 2 * B + 100)   # across tiles
    again(a, 300, 3 * B + 4)    # the batch's last row
    b = Batch(B + 9, 22, lectures=[lo, hi, b"mid"])
    for src, dst in ((12, 0), (41, 65), (3 * B + 4, B + 8)):  # across calls
        again(b, src, dst)
    c = Batch(5, 23, lectures=[b"mid"])
    again(c, 12, 4, flip=False)  # and once more: the third write wins
    cl.rows_create("table", 12)
    for bt, form in ((a, "packed"), (b, "spans"), (c, "packed")):
        append(cl, "table", form, bt)
    yield [a.oracle_rows(), b.oracle_rows(), c.oracle_rows()], lo, hi
    cl.rows_drop("table")


def test_select(cl, table):
    from rtsas_amd.client_rows import lecture_digest, rows_oracle
    batches, lo, hi = table
    cases = [(None, None, None), (lo, None, None), (hi, None, None), (b"first-only", None, None),
             (b"last-only", None, None), (b"absent", None, None), (b"mid", None, None),
             (lo, -5, -4), (lo, -5, -5), (lo, -4, None), (lo, None, -5), (hi, -2, 2), (hi, -3, -2), (hi, 2, 3),
             (hi, 3, 2), (None, -5, 1), (None, 0, None), (None, None, 0), (None, I64_MIN, I64_MAX),
             (lo, I64_MIN, I64_MAX)]
    for lecture, since, until in cases:
        want = rows_oracle(batches, lecture=lecture, since=since, until=until)["select"]
        got = cl.rows_select("table", lecture, since, until)
        assert same((got["lecture_digest"], got["epoch"], got["student_id"], got["is_valid"]), want), \
            (lecture, since, until)
        assert got["complete"]
    # what the cases rely on is there: a collapse, the edges in signed order, the top-bit digests in unsigned order
    whole = rows_oracle(batches)
    assert whole["select"][0].size < whole["log"][0].size
    d = whole["select"][0]
    assert lecture_digest(lo) < 2 ** 63 <= lecture_digest(hi) and (np.diff(d.astype(object)) >= 0).all()
    edge = cl.rows_select("table", lo, -5, -4)["student_id"].tolist()
    assert edge[0] == I64_MIN and edge[-1] == I64_MAX and edge == sorted(edge) and 0 in edge and -(1 << 31) - 1 in edge
    assert rows_oracle(batches, lecture=b"absent")["select"][0].size == 0
    assert rows_oracle(batches, lecture=b"first-only")["select"][0].size > 0
    # one lecture alone in a log: every row matches
    cl.rows_create("one", 10)
    try:
        bt = Batch(B + 3, 31, lectures=[b"only"])
        append(cl, "one", "packed", bt)
        got = cl.rows_select("one", b"only")
        want = rows_oracle([bt.oracle_rows()], lecture=b"only")["select"]
        assert same((got["lecture_digest"], got["epoch"], got["student_id"], got["is_valid"]), want)
        assert same(tuple(cl.rows_select("one")[k] for k in ("lecture_digest", "epoch", "student_id", "is_valid")), want)
    finally:
        cl.rows_drop("one")


def test_select_capacity_protocol(cl, table):
    from rtsas_amd.client_rows import rows_oracle
    batches, lo, hi = table
    for lecture in (None, lo):
        want = rows_oracle(batches, lecture=lecture)["select"]
        n = want[0].size
        assert n > 2
        for device in (False, True):
            rc, n_out, complete, _ = raw_select(cl, "table", lecture, I64_MIN, I64_MAX, 0, device)
            assert (rc, n_out, complete) == (EROWSSPACE, n, 1)  # cap = 0 is the count
            rc, n_out, complete, cols = raw_select(cl, "table", lecture, I64_MIN, I64_MAX, n - 1, device)
            assert (rc, n_out, complete) == (EROWSSPACE, n, 1)
            assert all((c.view(np.uint8) == 0xAB).all() for c in cols)  # nothing written
            rc, n_out, complete, cols = raw_select(cl, "table", lecture, I64_MIN, I64_MAX, n, device)
            assert (rc, n_out, complete) == (0, n, 1) and same(tuple(cols), want)  # host and device outputs
            rc, n_out, complete, cols = raw_select(cl, "table", lecture, I64_MIN, I64_MAX, n + 7, device)
            assert (rc, n_out) == (0, n) and same(tuple(c[:n] for c in cols), want)
            assert all((c[n:].view(np.uint8) == 0xAB).all() for c in cols)
    # nothing matches: cap = 0 succeeds
    assert raw_select(cl, "table", b"absent", I64_MIN, I64_MAX, 0)[:3] == (0, 0, 1)
    assert raw_select(cl, "table", lo, 5000, 6000, 0)[:3] == (0, 0, 1)


def test_graph_replay_appends_again(pkg, engine):
    """a recorded append launched twice appends twice: the head lives on the device"""
    from rtsas_amd.client_rows import rows_oracle
    cl = pkg.SketchClient(context=engine.ctx)
    n = B + 17
    bt = Batch(n, 41)
    cl.rows_create("direct", 12)
    cl.rows_create("replayed", 12)
    g, held, busy = None, [], []
    try:
        append(cl, "direct", "packed", bt)  # a direct call first: it sizes the context scratch the recording pins

        # the uploads are synchronous copies: they come before the capture begins
        d = Dev(cl.ctx)
        lb, lo = packed(bt.lectures)
        ib, io = packed(bt.ids)
        args = [d.up(lb), d.up(lo), d.up(ib), d.up(io), d.up(bt.ep), d.up(bt.valid), None, n]
        held.append(d)
        g = engine.capture(lambda: (
            cl.ctx.call("ske_rows_append_packed_async", cl.rows_rid("replayed"), *args),
            busy.append(engine.ctx.lib.ske_rows_select(engine.ctx.ptr, cl.rows_rid("replayed"), None, 0, I64_MIN,
                                                       I64_MAX, None, None, None, None, 0, C.byref(C.c_uint64()),
                                                       C.byref(C.c_int()), 0)),
            busy.append(engine.ctx.lib.ske_rows_free(engine.ctx.ptr, cl.rows_rid("replayed")))))
        assert busy == [EBUSY, EBUSY]  # select and free wait for the stream: not while a capture records
        assert cl.rows_info("replayed")["used"] == 0  # recording ran nothing
        one = rows_oracle([bt.oracle_rows()])
        k = one["log"][0].size
        g.launch()
        engine.sync()
        assert cl.rows_info("replayed")["used"] == k and same(log_of(cl, "replayed"), one["log"])
        g.launch()
        engine.sync()
        two = rows_oracle([bt.oracle_rows(), bt.oracle_rows()])
        info = cl.rows_info("replayed")
        check_info(info, 2 * k, two["taken"], two["refused_ids"])
        assert same(log_of(cl, "replayed"), two["log"])  # arrival order repeats
        assert engine.ctx.lib.ske_rows_free(engine.ctx.ptr, cl.rows_rid("replayed")) == EBUSY  # a graph is alive
    finally:
        if g is not None:
            g.free()
        for d in held:
            d.free()
        cl.rows_drop("direct")
        cl.rows_drop("replayed")


def test_reset_two_logs_and_restore(cl):
    """reset empties a log; two logs do not touch each other; the host append
    of a log's read-back, ids as text, restores it"""
    from rtsas_amd.client_rows import rows_oracle
    a, b = Batch(B + 1, 51), Batch(2 * B, 52)
    cl.rows_create("a", 10)
    cl.rows_create("b", 10)
    try:
        append(cl, "a", "packed", a)
        append(cl, "b", "spans", b)
        append(cl, "a", "spans", a, mask=take_of("alternating", a.n))
        wa = rows_oracle([a.oracle_rows(), a.oracle_rows(take_of("alternating", a.n))])
        wb = rows_oracle([b.oracle_rows()])
        assert same(log_of(cl, "a"), wa["log"]) and same(log_of(cl, "b"), wb["log"])
        cl.rows_reset("a")
        info = cl.rows_info("a")
        assert {k: info[k] for k in ("used", "taken", "refused_ids", "dropped", "overflow")} == \
            dict(used=0, taken=0, refused_ids=0, dropped=0, overflow=0)
        assert cl.rows_select("a")["epoch"].size == 0 and cl.rows_read("a")["epoch"].size == 0
        assert same(log_of(cl, "b"), wb["log"])
        # the facade's host append: the same rule, and the restore of a checkpoint
        cl.rows_append("a", b.lectures, b.ids, b.ep, b.valid)
        assert same(log_of(cl, "a"), wb["log"])
        check_info(cl.rows_info("a"), wb["log"][0].size, wb["taken"], wb["refused_ids"])
        sa, sb = cl.rows_select("a"), cl.rows_select("b")
        assert all(np.array_equal(sa[k], sb[k]) for k in ("lecture_digest", "epoch", "student_id", "is_valid"))
    finally:
        cl.rows_drop("a")
        cl.rows_drop("b")


def test_errors(cl, pkg):
    lib, ptr = cl.ctx.lib, cl.ctx.ptr
    info = _lib.RowsInfo()
    assert lib.ske_rows_reset(ptr, 7) == -42 and lib.ske_rows_free(ptr, 7) == -42
    assert lib.ske_rows_reset(ptr, 8) == EINVAL and lib.ske_rows_init(ptr, 8, 10) == EINVAL
    assert lib.ske_rows_init(ptr, 7, 7) == -44 and lib.ske_rows_init(ptr, 7, 29) == -44
    cl.rows_create("e", 8)
    try:
        rid = cl.rows_rid("e")
        assert lib.ske_rows_init(ptr, rid, 8) == -43
        assert lib.ske_rows_read(ptr, rid, 0, 1, None, None, None, None) == EINVAL  # past `used`
        assert lib.ske_rows_append_packed_async(ptr, rid, None, None, None, None, None, None, None, 0) == 0
        assert lib.ske_rows_append_packed_async(ptr, rid, None, None, None, None, None, None, None, 1) == EINVAL
        assert lib.ske_rows_append_packed_async(ptr, rid, None, None, None, None, None, None, None,
                                                0xFFFFFFFF) == EINVAL
        assert lib.ske_rows_info(ptr, rid, C.byref(info)) == 0 and info.capacity == 256
    finally:
        cl.rows_drop("e")
