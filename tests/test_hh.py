"""Heavy-hitter sets on the GPU (csrc/sketch_hh.hip through the C-ABI, the
engine, the facade and analysis.StudentCounts) against a restatement written
here: a Count-Min table as in test_cms.py (copied, not imported), the oracle's
MurmurHash64A for the digests, a dict as the set.

The rule restated: after a batch's adds, every id of the batch (that the mask
lets through) whose estimate is at least the track threshold is in the set from
then on; ids are judged only at the batches they occur in.  A list is every
member whose current estimate is at least the list threshold, sorted by estimate
descending, then id bytes ascending.  Every comparison is of the whole sorted
list (ids with their lengths, estimates), ``used`` and ``complete``.

Wherever the set is compared, the restatement's set stays within the load limit
(capacity / 2): the test asserts that first.  Only test_overflow goes past it."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
BLOOM_SEED = 0xC6A4A7935BD1E995
LDS_CELLS = 152 * 1024 // 4          # kCmsLdsCells
LDS_TABLE = (2003, 7)
GLOBAL_TABLE = (50021, 5)
BELOW = (4864, 8)                    # 38912 cells: the largest table a track copies into LDS
ABOVE = (12971, 3)                   # 38913 cells: the smallest it reads from memory
TABLES = {"lds": LDS_TABLE, "global": GLOBAL_TABLE, "below": BELOW, "above": ABOVE}
SIZES = [1, 63, 64, 65, 1025, 100003]
WIDTHS = [1, 5, 8, 9, 13, 16]
MAX_PROBES, LOAD_DEN = 128, 2
assert BELOW[0] * BELOW[1] == LDS_CELLS and ABOVE[0] * ABOVE[1] == LDS_CELLS + 1


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

    def add(self, items):
        if not items:
            return
        cs = cells_of(items, self.width, self.depth)
        for r in range(self.depth):
            np.add.at(self.t[r], cs[r], np.uint64(1))
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


# ---------------------------------------------------------------- inputs
def skewed(n: int, width: int, seed: int) -> list:
    """n ids of `width` bytes drawn with a heavy skew from a pool of random
    byte strings (the all-zero id among them), so counts run from 1 to many"""
    rng = np.random.default_rng(100 * seed + width)
    pool = max(2, min(n // 3, 256 ** min(width, 2)))
    ids = rng.integers(0, 256, (pool, width), dtype=np.uint8)
    ids[0] = 0
    ids = np.unique(ids, axis=0)
    draw = np.minimum(rng.zipf(1.4, n) - 1, rng.integers(0, len(ids), n))
    return [bytes(r) for r in ids[draw]]


def fixed_batch(engine, items, width):
    from rtsas_amd.engine import DeviceBatch
    b = DeviceBatch(engine.ctx, len(items), width)
    b.bytes.from_host(np.frombuffer(b"".join(items), np.uint8))
    b.offs.from_host((np.arange(len(items) + 1) * width).astype(np.uint32))
    return b


def dev_u8(engine, arr):
    from rtsas_amd.engine import DeviceBuffer
    a = np.ascontiguousarray(arr, np.uint8)
    d = DeviceBuffer(engine.ctx, a.nbytes + 16)
    d.from_host(a)
    return d


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def make_engine(form=None):
    """form "lds": tables up to kCmsLdsCells cells are copied into LDS by a
    track; "memory": none is; None: the build's default."""
    ge.load_package()
    from rtsas_amd.engine import SketchEngine
    if form is not None:
        os.environ["SKE_HH_LDS_CELLS"] = str(LDS_CELLS if form == "lds" else 0)
    try:
        return SketchEngine(0)  # ske_open reads the variable
    finally:
        os.environ.pop("SKE_HH_LDS_CELLS", None)


def batch(engine, cid, hid, items, width, threshold, mask=None, want=1):
    """one batch as StudentCounts enqueues it: the add, then the track, one sync"""
    b = fixed_batch(engine, items, width)
    dm = None if mask is None else dev_u8(engine, mask)
    engine.cms_add(cid, b, mask=dm, want=want)
    engine.hh_track(hid, cid, b, threshold, mask=dm, want=want)
    engine.sync()
    b.free()
    if dm:
        dm.free()


def check(engine, hid, cid, table: RefTable, rset: RefSet, threshold, complete=True):
    ids, est, done = engine.hh_list(hid, cid, threshold)
    want_ids, want_est = rset.listing(table, threshold)
    info = engine.hh_info(hid)
    assert info["used"] == len(rset.members) and info["capacity"] == rset.capacity
    assert done is complete and bool(info["overflow"]) is not complete
    assert [len(i) for i in ids] == [len(i) for i in want_ids]
    assert ids == want_ids
    assert [int(e) for e in est] == want_est
    return ids, est


def threshold_for(n, table):
    """above the table's noise (a cell holds about n / width per batch), so
    that the skew's head passes and its tail does not"""
    return 1 if n == 1 else 3 + 4 * n // table[0]


def two_batches(engine, orc, table, n, width):
    ref, rset = RefTable(*table), RefSet(orc, 16)
    engine.cms_init(0, *table)
    engine.hh_init(0, 16)
    threshold = threshold_for(n, table)
    seen = set()
    for seed in (1, 2):  # the second batch meets a table and a set that are not empty
        items = skewed(n, width, 10 * n + seed)
        batch(engine, 0, 0, items, width, threshold)
        ref.add(items)
        rset.track(ref, items, threshold)
        check(engine, 0, 0, ref, rset, threshold)
        seen |= set(items)
    if n >= 63 and width > 1:  # skewed: some ids pass, not all
        assert 0 < len(rset.members) < len(seen)
    return ref, rset


# ---------------------------------------------------------------- track and list
@pytest.mark.parametrize("ni", range(len(SIZES)), ids=[f"n{n}" for n in SIZES])
@pytest.mark.parametrize("tname", list(TABLES))
def test_track_sizes_and_tables(orc, tname, ni):
    """every batch size on every table (the LDS copy up to kCmsLdsCells cells,
    memory above), the widths rotating so that each table meets each width"""
    width = WIDTHS[(ni + list(TABLES).index(tname)) % len(WIDTHS)]
    two_batches(make_engine("lds"), orc, TABLES[tname], SIZES[ni], width)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("form", ["lds", "memory", None])
def test_track_widths_both_forms(orc, form, width):
    """every width in both forms of the 2003 x 7 table and in the default one"""
    two_batches(make_engine(form), orc, LDS_TABLE, 1025, width)


def test_batch_boundaries(engine, orc):
    """three batches into a 7 x 2 table: collisions raise the cells of early
    ids after their last occurrence; they are not added then"""
    rng = np.random.default_rng(41)
    pool = [b"%05d" % v for v in rng.choice(np.arange(10000, 100000), 60, replace=False)]
    b1 = pool[:20]                                    # once each: low estimates
    b2 = [p for p in pool[20:40] for _ in range(3)]   # 60 items
    b3 = pool[40:] + pool[20:25]
    threshold = 8
    ref, rset = RefTable(7, 2), RefSet(orc, 8)
    engine.cms_init(0, 7, 2)
    engine.hh_init(0, 8)
    for items in (b1, b2, b3):
        order = [items[i] for i in rng.permutation(len(items))]  # the order inside a batch is free
        batch(engine, 0, 0, order, 5, threshold)
        ref.add(items)
        rset.track(ref, items, threshold)
        check(engine, 0, 0, ref, rset, threshold)
    late = [i for i, e in zip(b1, ref.query(b1)) if e >= threshold and rset.digest(i) not in rset.members]
    assert late and rset.members  # the case the rule is about did occur
    ids, _, _ = engine.hh_list(0, 0, threshold)
    assert not set(late) & set(ids)


@pytest.mark.parametrize("tname", ["lds", "global"])
def test_mask(orc, tname):
    engine = make_engine("lds")
    table = TABLES[tname]
    items = skewed(20011, 8, 7)
    mask = (np.random.default_rng(3).random(len(items)) < 0.85).astype(np.uint8)
    for cid, want in ((0, 1), (1, 0), (2, None)):
        ref, rset = RefTable(*table), RefSet(orc, 16)
        engine.cms_init(cid, *table)
        engine.hh_init(cid, 16)
        take = items if want is None else [items[i] for i in np.flatnonzero(mask == want)]
        thr = threshold_for(len(items), table)
        for _ in range(2):
            batch(engine, cid, cid, items, 8, thr, None if want is None else mask, 1 if want is None else want)
            ref.add(take)
            rset.track(ref, take, thr)
            check(engine, cid, cid, ref, rset, thr)
        assert 0 < len(rset.members) < len(set(take))
    # an all-masked batch changes nothing
    before = engine.hh_list(0, 0, 4)
    b = fixed_batch(engine, items, 8)
    engine.hh_track(0, 0, b, 1, mask=dev_u8(engine, np.zeros(len(items), np.uint8)), want=1)
    engine.sync()
    after = engine.hh_list(0, 0, 4)
    assert before[0] == after[0] and np.array_equal(before[1], after[1])


@pytest.mark.parametrize("form", ["lds", "memory"])
def test_concurrent_claims(orc, form):
    """100 003 distinct ids, all passing at threshold 1, into 2^18 slots"""
    engine = make_engine(form)
    vals = np.random.default_rng(9).choice(np.arange(10_000_000, 100_000_000), 100003, replace=False)
    items = [b"%d" % v for v in vals]
    engine.cms_init(0, *LDS_TABLE)
    engine.hh_init(0, 18)
    assert len(items) <= (1 << 18) // LOAD_DEN
    batch(engine, 0, 0, items, 8, 1)
    ids, est, done = engine.hh_list(0, 0, 1)
    assert done and engine.hh_info(0) == {"capacity": 1 << 18, "used": 100003, "overflow": 0}
    assert len(ids) == 100003 and set(ids) == set(items)
    ref = RefTable(*LDS_TABLE)
    ref.add(items)
    order = sorted(zip((-ref.query(items).astype(np.int64)).tolist(), items))
    assert ids == [i for _, i in order] and [-int(e) for e in est] == [e for e, _ in order]


@pytest.mark.parametrize("form", ["lds", "memory"])
def test_one_hot_id(orc, form):
    """one id takes half of 200 000 items: one entry"""
    engine = make_engine(form)
    rng = np.random.default_rng(13)
    items = [b"%d" % v for v in rng.integers(10_000_000, 100_000_000, 200000)]
    for i in rng.choice(200000, 100000, replace=False):
        items[i] = b"20251003"
    ref, rset = RefTable(*LDS_TABLE), RefSet(orc, 10)
    engine.cms_init(0, *LDS_TABLE)
    engine.hh_init(0, 10)
    for _ in range(2):
        batch(engine, 0, 0, items, 8, 5000)
        ref.add(items)
        rset.track(ref, items, 5000)
        ids, est = check(engine, 0, 0, ref, rset, 5000)
        assert ids == [b"20251003"] and engine.hh_info(0)["used"] == 1


def test_thresholds_and_ordering(engine, orc):
    """a list threshold above the track threshold filters; estimates are
    ske_cms_query's; equal estimates come in id order (a prefix before its
    extension); the all-zero id of width 8 is a member"""
    ref, rset = RefTable(*GLOBAL_TABLE), RefSet(orc, 12)
    engine.cms_init(0, *GLOBAL_TABLE)
    engine.hh_init(0, 12)
    rng = np.random.default_rng(17)
    pool = [bytes(8)] + [bytes(r) for r in rng.integers(0, 256, (299, 8), dtype=np.uint8)]
    counts = [5 + i % 4 for i in range(len(pool))]  # 75 ids per count: ties at every estimate
    items8 = [p for p, c in zip(pool, counts) for _ in range(c)]
    items8 = [items8[i] for i in rng.permutation(len(items8))]
    rare = [bytes(r) for r in rng.integers(0, 256, (50, 8), dtype=np.uint8)]  # once each: below the threshold
    batches = [(items8 + rare, 8), ([b"ab"] * 6 + [b"a\x00"] * 6, 2), ([b"ab\x00"] * 6 + [b"a\x00\x00"] * 6, 3),
               ([b"a"] * 6 + [b"\x00"] * 6, 1)]  # one zero byte: the id whose hash is 0 (claim word 1)
    for items, width in batches:
        batch(engine, 0, 0, items, width, 5)
        ref.add(items)
        rset.track(ref, items, 5)
    for threshold in (5, 6, 7, 8, 9):
        ids, est = check(engine, 0, 0, ref, rset, threshold)
        assert (threshold == 9) == (ids == [])
        if ids:
            from rtsas_amd.engine import DeviceBatch
            buf = np.frombuffer(b"".join(ids), np.uint8).copy()
            offs = np.zeros(len(ids) + 1, np.uint32)
            offs[1:] = np.cumsum([len(i) for i in ids])
            q = np.zeros(len(ids), np.uint32)
            engine.ctx.call("ske_cms_query", 0, _p(buf), _p(offs), len(ids), _p(q), 0)
            assert np.array_equal(q, est)
    ids, est, _ = engine.hh_list(0, 0, 5)
    assert bytes(8) in ids and not set(rare) & set(ids)
    six = [i for i, e in zip(ids, est) if e == 6]
    assert six == sorted(six)
    short = [i for i in six if len(i) < 8]
    assert short == [b"\x00", b"a", b"a\x00", b"a\x00\x00", b"ab", b"ab\x00"]
    assert orc.murmur64a(b"\x00", BLOOM_SEED) == 0
    # the packed form from the host, into a second set: the same members
    engine.hh_init(1, 12)
    for items, _ in batches:
        buf = np.frombuffer(b"".join(items), np.uint8).copy()
        offs = np.zeros(len(items) + 1, np.uint32)
        offs[1:] = np.cumsum([len(i) for i in items])
        engine.ctx.call("ske_hh_track", 1, 0, _p(buf), _p(offs), len(items), 5, 0)
    got = engine.hh_list(1, 0, 5)
    assert got[0] == ids and np.array_equal(got[1], est) and got[2]


def test_overflow_and_reset(engine, orc):
    """5000 distinct passing ids into the smallest capacity"""
    from rtsas_amd import _lib
    log2 = _lib.SKE_HH_MIN_LOG2
    vals = np.random.default_rng(19).choice(np.arange(10000, 100000), 5000, replace=False)
    items = [b"%d" % v for v in vals]
    engine.cms_init(0, *LDS_TABLE)
    engine.hh_init(0, log2)
    batch(engine, 0, 0, items, 5, 1)
    ids, est, done = engine.hh_list(0, 0, 1)
    info = engine.hh_info(0)
    assert done is False and info["overflow"] != 0
    assert 0 < info["used"] <= info["capacity"] == 1 << log2
    assert len(ids) == info["used"] == len(set(ids))
    assert set(ids) <= set(items)  # every one of them passes in the restatement (threshold 1)
    ref = RefTable(*LDS_TABLE)
    ref.add(items)
    assert [int(e) for e in est] == [int(e) for e in ref.query(ids)]
    engine.hh_reset(0)
    assert engine.hh_info(0) == {"capacity": 1 << log2, "used": 0, "overflow": 0}
    ids, est, done = engine.hh_list(0, 0, 1)
    assert ids == [] and len(est) == 0 and done is True
    rset = RefSet(orc, log2)
    batch(engine, 0, 0, items[:100], 5, 1)
    ref.add(items[:100])
    rset.track(ref, items[:100], 1)
    check(engine, 0, 0, ref, rset, 1)


def test_errors(engine, pkg):
    from rtsas_amd import _lib

    def code(name, *args):
        with pytest.raises(pkg.SketchLibError) as e:
            engine.ctx.call(name, *args)
        return e.value.code

    engine.cms_init(0, *LDS_TABLE)
    engine.hh_init(0, 10)
    items = [b"%017d" % i for i in range(4)]
    b17 = fixed_batch(engine, items, 17)
    ids = C.c_void_p(b17.bytes.ptr)
    assert code("ske_hh_track_fixed_async", 0, 0, ids, 17, 4, None, 1, 1) == _lib.SKE_ETOOLONG
    assert code("ske_hh_track_fixed_async", 0, 0, ids, 16, 4, None, 1, 0) == _lib.SKE_EINVAL
    assert code("ske_hh_track_fixed_async", 0, 0, ids, 0, 4, None, 1, 1) == _lib.SKE_EINVAL
    assert code("ske_hh_track_fixed_async", 0, 0, ids, 16, 4, None, 2, 1) == _lib.SKE_EINVAL
    assert code("ske_hh_track_fixed_async", 5, 0, ids, 16, 4, None, 1, 1) == _lib.SKE_EHHNOSET
    assert code("ske_hh_track_fixed_async", 0, 7, ids, 16, 4, None, 1, 1) == _lib.SKE_ECMSNOKEY
    assert code("ske_hh_init", 0, 10) == _lib.SKE_EHHEXISTS
    assert code("ske_hh_init", 1, _lib.SKE_HH_MIN_LOG2 - 1) == _lib.SKE_EHHCAP
    assert code("ske_hh_init", 1, _lib.SKE_HH_MAX_LOG2 + 1) == _lib.SKE_EHHCAP
    assert code("ske_hh_init", _lib.SKE_MAX_HH, 10) == _lib.SKE_EINVAL
    for name in ("ske_hh_free", "ske_hh_reset"):
        assert code(name, 3) == _lib.SKE_EHHNOSET
    # the packed form: an id of 17 bytes, from the host (nothing is tracked) and on the device
    buf = np.frombuffer(b"abc" + items[0], np.uint8).copy()
    offs = np.asarray([0, 3, 20], np.uint32)
    engine.ctx.call("ske_cms_incrby", 0, _p(buf), _p(offs), 2, None, None, 0)
    assert code("ske_hh_track", 0, 0, _p(buf), _p(offs), 2, 1, 0) == _lib.SKE_ETOOLONG
    assert engine.hh_info(0)["used"] == 0
    assert code("ske_hh_track", 0, 0, ids, C.c_void_p(b17.offs.ptr), 4, 1, 1) == _lib.SKE_ETOOLONG
    assert code("ske_hh_track", 0, 0, _p(buf), _p(offs), 2, 0, 0) == _lib.SKE_EINVAL
    assert engine.hh_info(0) == {"capacity": 1024, "used": 0, "overflow": 0}
    engine.ctx.call("ske_hh_track", 0, 0, _p(buf), _p(offs[:2]), 1, 1, 0)
    assert engine.hh_list(0, 0, 1)[0] == [b"abc"]
    # an output too small: the count comes back, nothing else
    n, done = C.c_uint64(), C.c_int()
    assert code("ske_hh_list", 0, 0, 1, None, None, None, 0, C.byref(n), C.byref(done)) == _lib.SKE_EHHSPACE
    assert n.value == 1 and done.value == 1
    # a freed table is an error at the next call, and so is a freed set
    engine.ctx.call("ske_cms_free", 0)
    assert code("ske_hh_track_fixed_async", 0, 0, ids, 16, 4, None, 1, 1) == _lib.SKE_ECMSNOKEY
    assert code("ske_hh_list", 0, 0, 1, None, None, None, 0, C.byref(n), C.byref(done)) == _lib.SKE_ECMSNOKEY
    engine.hh_free(0)
    assert code("ske_hh_info", 0, C.byref(_lib.HhInfo())) == _lib.SKE_EHHNOSET
    engine.hh_init(0, 10)  # the id is free again


# ---------------------------------------------------------------- behind K1
def _c1_inputs():
    """C1-sized: BF.RESERVE 0.01 / 1000, 5-digit ids, 4 HLL keys, 6007 swipes
    of which about a tenth are not members, a handful of them repeat offenders"""
    rng = np.random.default_rng(23)
    members = rng.choice(np.arange(10000, 100000), 1000, replace=False)
    others = np.setdiff1d(np.arange(10000, 100000), members)
    n = 6007
    bad = rng.choice(others, n)
    offenders = rng.choice(others, 6, replace=False)
    pick = rng.random(n) < 0.3
    bad[pick] = rng.choice(offenders, int(pick.sum()))
    ids = np.where(rng.random(n) < 0.9, rng.choice(members[:300], n), bad)
    return members, ids, rng.integers(0, 4, n)


def test_capture(pkg, engine, orc):
    """swipes, two adds and two tracks recorded into one graph and replayed
    twice: the result of running the step twice eagerly"""
    from rtsas_amd.engine import DeviceBuffer
    members, ids, key_of = _c1_inputs()
    n = len(ids)
    engine.reserve(0, 0.01, 1000)
    engine.hll_reserve(4)
    mbuf, moffs = pkg.pack_ints(members)
    engine.ctx.call("ske_bf_madd", 0, _p(mbuf), _p(moffs), len(members), None, 0)
    sbuf, _ = pkg.pack_ints(ids)
    items = [bytes(r) for r in sbuf.reshape(n, 5)]
    b = fixed_batch(engine, items, 5)
    b.slot.from_host(key_of.astype(np.uint32))
    valid = DeviceBuffer(engine.ctx, n + 16)
    for i in range(4):
        engine.cms_init(i, *LDS_TABLE)
        engine.hh_init(i, 12)
    thr = (45, 10)  # attended, invalid

    def step(att, inv):
        engine.swipes_fixed_async(0, b, valid)
        engine.cms_add(att, b, mask=valid, want=1)
        engine.cms_add(inv, b, mask=valid, want=0)
        engine.hh_track(att, att, b, thr[0], mask=valid, want=1)
        engine.hh_track(inv, inv, b, thr[1], mask=valid, want=0)

    for _ in range(2):
        step(2, 3)
        engine.sync()
    v = valid.to_host(np.uint8, n).astype(bool)
    eager = []
    for k, sel in enumerate((v, ~v)):
        ref, rset = RefTable(*LDS_TABLE), RefSet(orc, 12)
        take = [items[i] for i in np.flatnonzero(sel)]
        for _ in range(2):
            ref.add(take)
            rset.track(ref, take, thr[k])
        check(engine, 2 + k, 2 + k, ref, rset, thr[k])
        assert 0 < len(rset.members) < len(set(take))
        eager.append((engine.hh_list(2 + k, 2 + k, thr[k]), engine.hh_info(2 + k)))

    g = engine.capture(lambda: step(0, 1))
    for i in (0, 1):  # recording ran nothing
        assert engine.hh_info(i)["used"] == 0
    g.launch()
    g.launch()
    engine.sync()
    for k in (0, 1):
        got = engine.hh_list(k, k, thr[k])
        assert got[0] == eager[k][0][0] and np.array_equal(got[1], eager[k][0][1]) and got[2] is True
        assert engine.hh_info(k) == eager[k][1]
    with pytest.raises(pkg.SketchLibError) as e:  # a recorded graph points to the set
        engine.hh_free(0)
    assert e.value.code == -13
    g.free()
    engine.hh_free(0)


def test_student_counts(pkg, client):
    members, ids, key_of = _c1_inputs()
    n = len(ids)
    keys = [f"hll:unique:CS10{k}:2025-10-03" for k in range(4)]
    mbuf, moffs = pkg.pack_ints(members)
    sbuf, _ = pkg.pack_ints(ids)
    id_mat = sbuf.reshape(n, 5)
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 1000)
    client.bf_madd_packed("bf:students", mbuf, moffs)
    slots = np.asarray([client.key_slot(k) for k in keys], np.uint32)[key_of]

    calls = []
    real = client.ctx.call
    client.ctx.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    plain = pkg.StudentCounts(client, "cms:a0", "cms:i0")
    calls.clear()
    want_valid = plain.update("bf:students", slots, id_mat)
    hot = [c for c in calls if c not in ("ske_device_alloc", "ske_memcpy")]
    assert hot == ["ske_swipes_fixed", "ske_cms_add_fixed_async", "ske_cms_add_fixed_async", "ske_sync"]
    assert 0.05 < 1 - want_valid.mean() < 0.2

    t_att, t_inv = 22, 8
    sc = pkg.StudentCounts(client, track_attended=t_att, track_invalid=t_inv, capacity_log2=12)
    half = n // 2
    got = np.concatenate([sc.update("bf:students", slots[:half], id_mat[:half]),
                          sc.update("bf:students", slots[half:], id_mat[half:])])
    assert np.array_equal(got, want_valid)
    for key, untracked in (("cms:attended", "cms:a0"), ("cms:invalid", "cms:i0")):  # tracking changes no counter
        assert np.array_equal(client.cms_table(key)[0], client.cms_table(untracked)[0])
    for sel, top, thr in ((want_valid, sc.top_attended, t_att), (~want_valid, sc.top_invalid, t_inv)):
        true = {}
        for i in np.flatnonzero(sel):
            s = bytes(id_mat[i])
            true[s] = true.get(s, 0) + 1
        heavy = {s for s, c in true.items() if c >= thr}
        assert 3 <= len(heavy) < len(true)
        ids_l, est, complete = top()
        assert complete and heavy <= set(ids_l)
        assert all(int(e) >= max(true.get(s, 0), thr) for s, e in zip(ids_l, est))
        assert [int(e) for e in est] == sorted((int(e) for e in est), reverse=True)
        assert top(k=3)[0] == ids_l[:3]
        higher = top(threshold=thr + 5)
        assert {s for s, c in true.items() if c >= thr + 5} <= set(higher[0]) <= set(ids_l)
    ins = sc.insights()
    assert [i["title"] for i in ins] == ["Most Consistent Attendees", "Invalid Attendance Attempts"]
    assert ins[1]["data"] == {s.decode(): int(e) for s, e in zip(*sc.top_invalid()[:2])}
    assert all(isinstance(k, str) and isinstance(v, int) for i in ins for k, v in i["data"].items())
    client.ctx.call = real
    # the packed form through the facade, into a set of its own over the same key: judged on the
    # final table it holds every listed student, with the same estimates; reset empties it
    ids_l, est, _ = sc.top_attended()
    client.hh_create("extra", "cms:attended", 10)
    client.hh_track_packed("extra", sbuf, np.arange(n + 1, dtype=np.uint32) * 5, t_att)
    more = dict(zip(*client.hh_list("extra", t_att)[:2]))
    assert set(ids_l) <= set(more) and all(more[s] == e for s, e in zip(ids_l, est))
    assert client.hh_info("extra")["used"] == len(more)
    client.hh_reset("extra")
    assert client.hh_info("extra") == {"capacity": 1024, "used": 0, "overflow": 0}
    # DEL of a tracked key frees its sets; FLUSHALL (the fixture's) the others
    assert client.execute_command("DEL", "cms:invalid") == 1
    with pytest.raises(pkg.ResponseError, match="heavy-hitter set does not exist"):
        sc.top_invalid()
    assert sc.top_attended()[2] is True
