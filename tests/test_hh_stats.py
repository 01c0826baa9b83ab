"""Statistics of a heavy-hitter set's estimates on the GPU
(csrc/sketch_hh_stats.hip through the C-ABI, the engine, the facade and
analysis.StudentCounts) against a restatement written here: the Count-Min
table, the digests and the set of test_hh.py (copied, not imported), and numpy
over ``RefSet.listing(table, threshold)`` for the expected values.

Every integer field is compared exactly (n, sum, both words of the sum of
squares, min, max, the two median order statistics, complete, and every
selected rank against ``np.sort``).  ``mean``, ``std`` and ``hh_quantile`` are
compared with numpy to 1e-12 relative: two float64 roundings of exact integers
against numpy's summation of at most 2^17 values.

Tables are written with ske_cms_import from the restatement's cells, so a case
costs no add; ids join through ske_hh_track (packed, from the host), which
takes every length from 0 to 16.  Wherever the set is compared the
restatement's set stays within the load limit (capacity / 2): asserted first.
Only the overflow case goes past it."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
BLOOM_SEED = 0xC6A4A7935BD1E995
LDS_TABLE = (2003, 7)
GLOBAL_TABLE = (50021, 5)
TABLES = {"lds": LDS_TABLE, "global": GLOBAL_TABLE}
LOAD_DEN = 2
MAX_RANKS = 16
REL = 1e-12


# ---------------------------------------------------------------- reference
def mm2(mat: np.ndarray, seed: int) -> np.ndarray:
    """MurmurHash2 (32-bit) of every row of a [m, L] uint8 matrix."""
    M = np.uint64(0x5BD1E995)
    mask = np.uint64(U32)
    m, L = mat.shape
    b = mat.astype(np.uint64)
    h = np.full(m, (seed ^ L) & U32, np.uint64)
    for j in range(L // 4):
        k = b[:, 4 * j] | b[:, 4 * j + 1] << np.uint64(8) | b[:, 4 * j + 2] << np.uint64(16) | \
            b[:, 4 * j + 3] << np.uint64(24)
        k = k * M & mask
        k ^= k >> np.uint64(24)
        k = k * M & mask
        h = h * M & mask
        h ^= k
    rem, at = L & 3, L & ~3
    if rem:
        for j in range(rem):
            h ^= b[:, at + j] << np.uint64(8 * j)
        h = h * M & mask
    h ^= h >> np.uint64(13)
    h = h * M & mask
    h ^= h >> np.uint64(15)
    return h.astype(np.uint32)


def cells_of(items: list, width: int, depth: int) -> np.ndarray:
    """[depth, n]: the cell of every item in every row."""
    out = np.zeros((depth, len(items)), np.int64)
    lens = np.fromiter(map(len, items), np.int64, count=len(items))
    for L in np.unique(lens):
        idx = np.flatnonzero(lens == L)
        mat = np.frombuffer(b"".join(items[i] for i in idx), np.uint8).reshape(len(idx), int(L))
        for r in range(depth):
            out[r, idx] = mm2(mat, r) % np.uint32(width)
    return out


class RefTable:
    def __init__(self, width, depth):
        self.width, self.depth = width, depth
        self.t = np.zeros((depth, width), np.uint64)

    def add(self, items, counts=None):
        """every item once, or counts[i] times"""
        if not items:
            return
        cs = cells_of(items, self.width, self.depth)
        w = np.ones(len(items), np.uint64) if counts is None else np.asarray(counts, np.uint64)
        for r in range(self.depth):
            np.add.at(self.t[r], cs[r], w)
        np.minimum(self.t, np.uint64(U32), out=self.t)

    def query(self, items):
        if not items:
            return np.zeros(0, np.uint32)
        cs = cells_of(items, self.width, self.depth)
        return self.t[np.arange(self.depth)[:, None], cs].min(axis=0).astype(np.uint32)


class RefSet:
    """digest -> id"""

    def __init__(self, orc, capacity_log2):
        self.orc, self.capacity = orc, 1 << capacity_log2
        self.members = {}

    def digest(self, item: bytes) -> int:
        return self.orc.murmur64a(item, BLOOM_SEED) or 1

    def track(self, table: RefTable, items, threshold):
        """the batch's ids (already added to the table) that reach the threshold join"""
        uniq = sorted(set(items))
        for it, est in zip(uniq, table.query(uniq)):
            if est >= threshold:
                d = self.digest(it)
                assert self.members.setdefault(d, it) == it  # no two test ids share a digest
        assert len(self.members) <= self.capacity // LOAD_DEN, "the case must stay within the load limit"

    def listing(self, table: RefTable, threshold):
        ids = list(self.members.values())
        rows = [(int(e), i) for i, e in zip(ids, table.query(ids)) if e >= threshold]
        rows.sort(key=lambda r: (-r[0], r[1]))
        return [r[1] for r in rows], [r[0] for r in rows]


# ---------------------------------------------------------------- inputs and the device side
def make_ids(m: int, seed: int) -> list:
    """m distinct ids of every length from 0 to 16: the one-byte id 00 (digest 0
    mapped to 1) first, then the empty id, then lengths 2 .. 16 in turn"""
    rng = np.random.default_rng(seed)
    ids, seen = [b"\x00", b""], {b"\x00", b""}
    while len(ids) < m:
        L = 2 + (len(ids) - 2) % 15
        i = rng.integers(0, 256, L, dtype=np.uint8).tobytes()
        if i not in seen:
            seen.add(i)
            ids.append(i)
    return ids[:m]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def packed(items):
    buf = np.frombuffer(b"".join(items) + bytes(8), np.uint8).copy()
    offs = np.zeros(len(items) + 1, np.uint32)
    offs[1:] = np.cumsum([len(i) for i in items])
    return buf, offs


class Rig:
    """one table (cid) and one set (hid) of a context, beside their restatement"""

    def __init__(self, ctx, orc, table, log2, cid=0, hid=0, init=True):
        self.ctx, self.cid, self.hid = ctx, cid, hid
        self.ref, self.rset = RefTable(*table), RefSet(orc, log2)
        if init:
            ctx.call("ske_cms_init", cid, *table)
            ctx.call("ske_hh_init", hid, log2)

    def write_table(self):
        """the restatement's cells onto the device"""
        cells = np.ascontiguousarray(self.ref.t, np.uint32)
        self.ctx.call("ske_cms_import", self.cid, _p(cells), cells.size, int(self.ref.t[0].sum()))

    def track(self, items, threshold=1):
        self.rset.track(self.ref, items, threshold)
        if items:
            buf, offs = packed(items)
            self.ctx.call("ske_hh_track", self.hid, self.cid, _p(buf), _p(offs), len(items), threshold, 0)

    def fill(self, m, seed, threshold=1):
        """m ids with zipf counts in the table, all tracked"""
        ids = make_ids(m, seed)
        counts = np.minimum(np.random.default_rng(seed + 1).zipf(1.3, m), 200)
        self.ref.add(ids, counts)
        self.write_table()
        self.track(ids, threshold)
        assert len(self.rset.members) == m
        return ids

    def estimates(self):
        """every member's estimate, ascending: computed once, filtered per threshold"""
        return np.sort(np.asarray(self.rset.listing(self.ref, 0)[1], np.uint64))

    def stats(self, threshold):
        from rtsas_amd.engine import hh_stats
        return hh_stats(self.ctx, self.hid, self.cid, threshold)

    def select(self, threshold, ranks):
        from rtsas_amd.engine import hh_select
        return hh_select(self.ctx, self.hid, self.cid, threshold, ranks)

    def select_code(self, threshold, ranks, nranks=None, sentinel=0xDEADBEEF):
        """the raw call: (return code, n_out, out)"""
        r = np.asarray(ranks, np.uint64)
        out = np.full(max(len(r), 1), sentinel, np.uint32)
        n = C.c_uint64(12345)
        lib = self.ctx.lib
        rc = lib.ske_hh_select(self.ctx.ptr, self.hid, self.cid, threshold, _p(r),
                               len(r) if nranks is None else nranks, _p(out), C.byref(n))
        return rc, n.value, out


def check_stats(rig, all_est, threshold, complete=True):
    """every field of ske_hh_stats against numpy over the passing estimates"""
    from rtsas_amd.client_hh import derive_stats
    v = all_est[all_est >= threshold]
    ints = [int(x) for x in v]
    n = len(ints)
    raw = rig.stats(threshold)
    assert raw["n"] == n and raw["sum"] == sum(ints)
    assert raw["sq_lo"] == sum((x * x) & U32 for x in ints) and raw["sq_hi"] == sum((x * x) >> 32 for x in ints)
    assert raw["min"] == (ints[0] if n else 0) and raw["max"] == (ints[-1] if n else 0)
    assert raw["med_lo"] == (ints[(n - 1) // 2] if n else 0) and raw["med_hi"] == (ints[n // 2] if n else 0)
    assert raw["complete"] == int(complete)
    s = derive_stats(raw)
    assert s["sumsq"] == sum(x * x for x in ints)
    if n:
        f = v.astype(np.float64)
        assert s["median"] == np.median(f)
        assert s["mean"] == pytest.approx(f.mean(), rel=REL, abs=0)
    if n >= 2:
        assert s["std"] == pytest.approx(f.std(ddof=1), rel=REL, abs=0)
    else:
        assert math.isnan(s["std"])
    return v


def check_select(rig, v, threshold, every=True, seed=0):
    """ranks against the sorted passing estimates: all of them in batches of 16, or a
    sample; then one shuffled batch with repeats"""
    n = len(v)
    if n == 0:
        rc, n_out, out = rig.select_code(threshold, [0])
        assert (rc, n_out) == (-1, 0) and out[0] == 0xDEADBEEF
        return
    rng = np.random.default_rng(seed + n)
    if every:
        ranks = np.arange(n)
    else:
        ends = np.clip([0, 1, (n - 1) // 2, n // 2, n - 2, n - 1], 0, n - 1)
        ranks = np.unique(np.concatenate([ends, rng.integers(0, n, 26)]))
    for at in range(0, len(ranks), MAX_RANKS):
        r = ranks[at:at + MAX_RANKS]
        assert np.array_equal(rig.select(threshold, r), v[r].astype(np.uint32)), (threshold, at)
    r = rng.integers(0, n, MAX_RANKS)
    r[3] = r[11] = r[0]  # repeats
    assert np.array_equal(rig.select(threshold, r), v[r].astype(np.uint32))


def thresholds_of(all_est, track=1):
    """0, the track threshold, a value with members on both sides, the maximum, one above it"""
    if len(all_est) == 0:
        return [0, track, 5]
    mx = int(all_est[-1])
    mid = int(all_est[len(all_est) // 2]) + 1  # above the lower half; below the maximum unless all are equal
    return [0, track, min(mid, mx), mx, mx + 1]


# ---------------------------------------------------------------- shapes
@pytest.mark.parametrize("members", [0, 1, 2, 3, 63, 64, 65, 128])
@pytest.mark.parametrize("tname", list(TABLES))
def test_one_workgroup(engine, orc, tname, members):
    """2^8 slots: one workgroup of the estimate pass, up to the load limit"""
    rig = Rig(engine.ctx, orc, TABLES[tname], 8)
    rig.fill(members, 100 + members)
    est = rig.estimates()
    assert len(est) == members
    for thr in thresholds_of(est):
        v = check_stats(rig, est, thr)
        check_select(rig, v, thr)
    if members == 0:  # an empty set: all-zero stats, and any select is refused
        assert rig.stats(0) == {k: (1 if k == "complete" else 0) for k in rig.stats(0)}
        for ranks in ([0], [0, 1, 2], [5] * MAX_RANKS):
            assert rig.select_code(0, ranks)[:2] == (-1, 0)


@pytest.mark.parametrize("tname", list(TABLES))
def test_several_workgroups(engine, orc, tname):
    """2^10 slots, 300 members: four workgroups' atomics and compaction"""
    rig = Rig(engine.ctx, orc, TABLES[tname], 10)
    rig.fill(300, 7)
    est = rig.estimates()
    ths = thresholds_of(est)
    assert 0 < (est >= ths[2]).sum() < 300
    for thr in ths:
        v = check_stats(rig, est, thr)
        check_select(rig, v, thr)


@pytest.mark.parametrize("tname", list(TABLES))
def test_many_workgroups(engine, orc, tname):
    """2^17 slots, 40 000 members: 512 workgroups flush, and the compacted array is
    longer than one histogram workgroup's span (64 workgroups stride over it)"""
    rig = Rig(engine.ctx, orc, TABLES[tname], 17)
    m = 40000
    rig.fill(m, 11)
    est = rig.estimates()
    assert len(est) == m and m > (1 << 17) // (8 * 256) * 256
    ths = thresholds_of(est)
    assert 0 < (est >= ths[2]).sum() < m
    for thr in ths:
        v = check_stats(rig, est, thr)
        check_select(rig, v, thr, every=False)


@pytest.mark.parametrize("log2,members", [(18, 3000), (19, 50000), (21, 5000)])
def test_slots_per_thread(engine, orc, log2, members):
    """past 2^18 slots a thread of the estimate pass takes 2, 4, .. slots (kHhsEstGrid): the last
    capacity with one, the first with two (about 50 members per workgroup, in both steps), and 8"""
    rig = Rig(engine.ctx, orc, LDS_TABLE, log2)
    rig.fill(members, log2)
    est = rig.estimates()
    for thr in thresholds_of(est):
        v = check_stats(rig, est, thr)
        check_select(rig, v, thr, every=False)


# ---------------------------------------------------------------- digits, saturation, all equal
DIGIT_VALUES = [0, 1, 255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24, 1 << 31, U32]


def unique_cell_ids(width, m, seed):
    """m ids (lengths 0 .. 16) whose cells in a depth-1 table of this width are all different"""
    ids, cells, taken = [], cells_of(make_ids(4 * m, seed), width, 1)[0], set()
    for i, c in zip(make_ids(4 * m, seed), cells):
        if int(c) not in taken:
            taken.add(int(c))
            ids.append(i)
    assert len(ids) >= m
    return ids[:m]


def test_digits(engine, orc):
    """a depth-1 table whose cells are chosen values: every digit position decides somewhere"""
    width, m = 4099, 100
    rig = Rig(engine.ctx, orc, (width, 1), 8)
    ids = unique_cell_ids(width, m, 3)
    rig.ref.t[:] = 1  # every id joins at threshold 1; then the cells get their values
    rig.write_table()
    rig.track(ids)
    rng = np.random.default_rng(4)
    vals = np.asarray(DIGIT_VALUES + list(rng.choice(DIGIT_VALUES, m - len(DIGIT_VALUES))), np.uint64)
    rig.ref.t[:] = 0
    rig.ref.t[0, cells_of(ids, width, 1)[0]] = vals
    rig.write_table()
    est = rig.estimates()
    assert np.array_equal(est, np.sort(vals)) and len(set(vals.tolist())) == len(DIGIT_VALUES) < m
    for thr in (0, 1, 256, 65536, 1 << 24, (1 << 31) + 1, U32):
        v = check_stats(rig, est, thr)
        assert 0 < len(v) <= m
        check_select(rig, v, thr, seed=thr & 0xFF)


def test_saturation(engine, orc):
    """every cell 0xffffffff, 100 members: the largest sums a member can add"""
    rig = Rig(engine.ctx, orc, LDS_TABLE, 8)
    ids = make_ids(100, 5)
    rig.ref.t[:] = U32
    rig.write_table()
    rig.track(ids)
    for thr in (0, U32):
        raw = rig.stats(thr)
        assert raw["n"] == 100 and raw["sum"] == 100 * U32
        assert raw["sq_hi"] * 2 ** 32 + raw["sq_lo"] == 100 * U32 * U32
        assert raw["min"] == raw["max"] == raw["med_lo"] == raw["med_hi"] == U32
    est = rig.estimates()
    v = check_stats(rig, est, 7)
    check_select(rig, v, 7)


def test_all_equal(engine, orc):
    from rtsas_amd.client_hh import derive_stats
    rig = Rig(engine.ctx, orc, GLOBAL_TABLE, 10)
    ids = make_ids(300, 6)
    rig.ref.t[:] = 37
    rig.write_table()
    rig.track(ids)
    est = rig.estimates()
    assert set(est.tolist()) == {37}
    v = check_stats(rig, est, 0)
    check_select(rig, v, 0)
    s = derive_stats(rig.stats(37))
    assert s["std"] == 0.0 and s["mean"] == 37.0 == s["median"] and s["n"] == 300
    assert rig.stats(38)["n"] == 0


# ---------------------------------------------------------------- behaviour
def test_reads_only_and_repeats(engine, orc):
    """neither call changes the set or the table; two calls give the same answer; reset empties"""
    rig = Rig(engine.ctx, orc, LDS_TABLE, 10)
    rig.fill(300, 8)
    before = (engine.hh_list(0, 0, 1), engine.hh_info(0), engine.cms_table(0))
    a, ra = rig.stats(2), rig.select(2, [0, 5, 3, 3])
    b, rb = rig.stats(2), rig.select(2, [0, 5, 3, 3])
    assert a == b and np.array_equal(ra, rb) and a["n"] > 5
    after = (engine.hh_list(0, 0, 1), engine.hh_info(0), engine.cms_table(0))
    assert before[0][0] == after[0][0] and np.array_equal(before[0][1], after[0][1])
    assert before[1] == after[1] and np.array_equal(before[2][0], after[2][0]) and before[2][1] == after[2][1]
    engine.hh_reset(0)
    assert rig.stats(0) == {k: (1 if k == "complete" else 0) for k in a}
    assert rig.select_code(0, [0])[:2] == (-1, 0)


def test_overflow_clears_complete(engine, orc):
    """5000 distinct passing ids into the smallest capacity (test_hh.py's overflow recipe)"""
    from rtsas_amd import _lib
    rig = Rig(engine.ctx, orc, LDS_TABLE, _lib.SKE_HH_MIN_LOG2)
    vals = np.random.default_rng(19).choice(np.arange(10000, 100000), 5000, replace=False)
    items = [b"%d" % v for v in vals]
    rig.ref.add(items)
    rig.write_table()
    buf, offs = packed(items)
    engine.ctx.call("ske_hh_track", 0, 0, _p(buf), _p(offs), len(items), 1, 0)
    ids, est, done = engine.hh_list(0, 0, 1)
    assert done is False
    raw = rig.stats(1)
    assert raw["complete"] == 0 and raw["n"] == len(ids) == engine.hh_info(0)["used"]
    ints = sorted(int(e) for e in est)  # what the set does hold is still counted exactly
    assert raw["sum"] == sum(ints) and (raw["min"], raw["max"]) == (ints[0], ints[-1])
    assert raw["med_lo"] == ints[(len(ints) - 1) // 2] and raw["med_hi"] == ints[len(ints) // 2]


def test_errors(engine, orc, pkg):
    from rtsas_amd import _lib
    rig = Rig(engine.ctx, orc, LDS_TABLE, 8)
    rig.fill(10, 9)
    n = rig.stats(0)["n"]
    assert n == 10
    # a rank equal to n: refused, the count comes back, the output is untouched
    rc, n_out, out = rig.select_code(0, [0, n, 1])
    assert (rc, n_out) == (_lib.SKE_EINVAL, n) and (out == 0xDEADBEEF).all()
    rc, n_out, out = rig.select_code(0, [n - 1])
    assert (rc, n_out) == (0, n) and out[0] == rig.stats(0)["max"]
    assert rig.select_code(0, [0], nranks=0)[0] == _lib.SKE_EINVAL
    assert rig.select_code(0, [0] * 17)[0] == _lib.SKE_EINVAL
    lib, ptr = engine.ctx.lib, engine.ctx.ptr
    assert lib.ske_hh_stats(ptr, 0, 0, 0, None) == _lib.SKE_EINVAL
    assert lib.ske_hh_select(ptr, 0, 0, 0, None, 1, None, None) == _lib.SKE_EINVAL

    def code(fn, *args):
        with pytest.raises(pkg.SketchLibError) as e:
            fn(*args)
        return e.value.code

    assert code(engine.hh_stats, 5, 0, 0) == _lib.SKE_EHHNOSET  # a free hid
    assert code(engine.hh_select, 5, 0, 0, [0]) == _lib.SKE_EHHNOSET
    assert code(engine.hh_stats, 0, 7, 0) == _lib.SKE_ECMSNOKEY
    engine.ctx.call("ske_cms_free", 0)  # a freed table is an error at the next call
    assert code(engine.hh_stats, 0, 0, 0) == _lib.SKE_ECMSNOKEY
    assert code(engine.hh_select, 0, 0, 0, [0]) == _lib.SKE_ECMSNOKEY
    engine.hh_free(0)
    assert code(engine.hh_stats, 0, 0, 0) == _lib.SKE_EHHNOSET


def test_refused_inside_a_capture(engine, orc, pkg):
    """both calls wait for the stream: refused while recording, and the recording survives"""
    from rtsas_amd import _lib
    from rtsas_amd.engine import DeviceBatch
    rig = Rig(engine.ctx, orc, LDS_TABLE, 8)
    items = [b"%05d" % i for i in range(40)]
    b = DeviceBatch(engine.ctx, len(items), 5)
    b.bytes.from_host(np.frombuffer(b"".join(items), np.uint8))
    b.offs.from_host((np.arange(len(items) + 1) * 5).astype(np.uint32))
    codes = []

    def step():
        engine.cms_add(0, b)
        for fn, args in ((engine.hh_stats, (0, 0, 0)), (engine.hh_select, (0, 0, 0, [0]))):
            with pytest.raises(pkg.SketchLibError) as e:
                fn(*args)
            codes.append(e.value.code)
        engine.hh_track(0, 0, b, 1)

    g = engine.capture(step)
    assert codes == [_lib.SKE_EBUSY] * 2
    g.launch()
    engine.sync()
    rig.ref.add(items)
    rig.rset.track(rig.ref, items, 1)
    est = rig.estimates()
    v = check_stats(rig, est, 1)
    check_select(rig, v, 1)
    g.free()


# ---------------------------------------------------------------- the facade and StudentCounts
def test_facade_quantiles(client, orc):
    client.execute_command("CMS.INITBYDIM", "cms:q", *GLOBAL_TABLE)
    client.hh_create("hh:q", "cms:q", 12)
    hid, cid = client._hh_entry("hh:q")
    rig = Rig(client.ctx, orc, GLOBAL_TABLE, 12, cid=cid, hid=hid, init=False)
    rig.fill(1000, 12)
    est = rig.estimates()
    for thr in (0, 2):
        v = est[est >= thr].astype(np.float64)
        s = client.hh_stats("hh:q", thr)
        assert s["n"] == len(v) and s["median"] == np.median(v) and s["complete"] is True
        assert s["mean"] == pytest.approx(v.mean(), rel=REL, abs=0)
        assert s["std"] == pytest.approx(v.std(ddof=1), rel=REL, abs=0)
        for q in (0.0, 0.01, 0.25, 0.5, 0.75, 0.9, 0.999, 1.0):
            assert client.hh_quantile("hh:q", q, thr) == pytest.approx(np.quantile(v, q), rel=REL, abs=0), q
    ranks = np.random.default_rng(1).integers(0, len(est), 40)  # split over three calls
    assert np.array_equal(client.hh_select("hh:q", ranks), est[ranks].astype(np.uint32))
    assert math.isnan(client.hh_quantile("hh:q", 0.5, int(est[-1]) + 1))


def test_insights_by_the_references_rules(pkg, client):
    """about 3000 swipes of about 200 students with times: the device's lists are the
    reference's two rules applied in numpy to the true counts"""
    rng = np.random.default_rng(31)
    students = rng.choice(np.arange(10000, 100000), 200, replace=False)
    n = 3000
    draw = np.minimum(rng.zipf(1.3, n) - 1, rng.integers(0, 200, n))
    sid = students[draw]
    ids = np.frombuffer(b"".join(b"%05d" % s for s in sid), np.uint8).reshape(n, 5)
    times = 1_700_000_000 + rng.integers(0, 14 * 86400, n)
    late = (times % 86400) >= 9 * 3600
    client.execute_command("BF.RESERVE", "bf:s", 0.001, 1000)
    mbuf, moffs = pkg.pack_ints(students)
    client.bf_madd_packed("bf:s", mbuf, moffs)
    slots = np.full(n, client.key_slot("hll:unique:CS101:2025-10-03"), np.uint32)
    sc = pkg.StudentCounts(client, error=0.00002, probability=0.001, track_attended=1, track_late=1,
                           late_key="cms:late", capacity_log2=12)
    half = n // 2
    valid = np.concatenate([sc.update("bf:s", slots[:half], ids[:half], times[:half]),
                            sc.update("bf:s", slots[half:], ids[half:], times[half:])])
    assert valid.all()  # every student is a member: attended counts are the swipe counts

    def true_counts(sel):
        u, c = np.unique(sid[sel], return_counts=True)
        return {str(int(k)): int(v) for k, v in zip(u, c)}

    att, lat = true_counts(np.ones(n, bool)), true_counts(late)
    assert 100 < len(att) <= 200 and len(lat) > 50
    # the table is wide enough that the estimates are the true counts
    keys = sorted(att)
    assert np.array_equal(sc.attended([k.encode() for k in keys]), [att[k] for k in keys])
    assert np.array_equal(sc.late([k.encode() for k in sorted(lat)]), [lat[k] for k in sorted(lat)])

    pop = sc.population("attended")
    a = np.asarray(list(att.values()), np.float64)
    assert pop["n"] == len(att) and pop["sum"] == n and pop["median"] == np.median(a)
    assert pop["std"] == pytest.approx(a.std(ddof=1), rel=REL, abs=0)

    ins = {i["title"]: i for i in sc.insights(attended_threshold="reference", late_threshold="reference")}
    bound = np.median(a) + a.std(ddof=1)
    want = {k: v for k, v in att.items() if v > bound}
    assert 0 < len(want) < len(att) and all(abs(v - bound) > 1e-6 for v in att.values())
    assert ins["Most Consistent Attendees"]["data"] == want and ins["Most Consistent Attendees"]["complete"]
    assert sc.reference_threshold("attended", "median+std") == math.floor(bound) + 1
    la = np.asarray(list(lat.values()), np.float64)
    want_late = {k: v for k, v in lat.items() if v > np.median(la)}
    assert 0 < len(want_late) < len(lat)
    assert ins["Habitual Latecomers"]["data"] == want_late
    today = {i["title"]: i for i in sc.insights()}  # late_threshold=None: the host-side median
    assert today["Habitual Latecomers"]["data"] == want_late
    assert today["Habitual Latecomers"]["description"] == ins["Habitual Latecomers"]["description"]
