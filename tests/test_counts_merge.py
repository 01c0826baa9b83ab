"""The per-student and per-lecture counts merged across contexts on the GPU
(ske_cms_sum_dev, ske_hh_export_dev / ske_hh_merge_dev, ske_tally_export_dev /
ske_tally_merge_dev, distributed.ShardedCounts): `world` contexts in one
process stand for the ranks.  Everything is exact equality against

  * one context that was fed everything in the same batch sequence, and
  * plain truths written here: a numpy restatement of the Count-Min cells (as
    test_cms.py / test_hh.py write one; copied, not imported), a Python set for
    membership, a collections.Counter for the tally.

Wherever a listing is compared the union stays within the destination's load
limit (capacity / 2) and the test asserts `complete`; only the refusal tests go
past it.  The source's stream is waited for (ske_sync, or a call that returns
when done) before the destination's stream reads its buffers."""
import ctypes as C
import threading
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U32 = 0xFFFFFFFF
U64 = 2 ** 64 - 1
BLOOM_SEED = 0xC6A4A7935BD1E995
SMALL, LARGE = (7, 3), (2000, 7)   # 21 cells (ncells & 3 == 1) and 14000


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
    out = np.zeros((depth, len(items)), np.int64)
    lens = np.fromiter(map(len, items), np.int64, count=len(items))
    for L in np.unique(lens):
        idx = np.flatnonzero(lens == L)
        mat = np.frombuffer(b"".join(items[i] for i in idx), np.uint8).reshape(len(idx), int(L))
        for r in range(depth):
            out[r, idx] = mm2(mat, r) % np.uint32(width)
    return out


def ref_table(items: list, width: int, depth: int, incr=None) -> np.ndarray:
    """[depth, width] u32: the table after adding every item (1 each, or incr)."""
    t = np.zeros((depth, width), np.uint64)
    if items:
        cs = cells_of(items, width, depth)
        inc = np.ones(len(items), np.uint64) if incr is None else np.asarray(incr, np.uint64)
        for r in range(depth):
            np.add.at(t[r], cs[r], inc)
    return np.minimum(t, np.uint64(U32)).astype(np.uint32)


def ref_query(table: np.ndarray, items: list) -> np.ndarray:
    depth, width = table.shape
    cs = cells_of(items, width, depth)
    return table[np.arange(depth)[:, None], cs].min(axis=0)


def ref_listing(table: np.ndarray, members, threshold: int):
    ids = sorted(members)
    if not ids:
        return [], []
    rows = [(int(e), i) for i, e in zip(ids, ref_query(table, ids)) if e >= threshold]
    rows.sort(key=lambda r: (-r[0], r[1]))
    return [r[1] for r in rows], [r[0] for r in rows]


def digest(orc, item: bytes) -> int:
    return orc.murmur64a(item, BLOOM_SEED) or 1


def assert_distinct_digests(orc, ids):
    ids = set(ids)
    assert len({digest(orc, i) for i in ids}) == len(ids), "no two test ids may share a digest"


# ---------------------------------------------------------------- plumbing
def dbuf(client, arr):
    from rtsas_amd.engine import DeviceBuffer
    a = np.ascontiguousarray(arr)
    d = DeviceBuffer(client.ctx, a.nbytes + 16)
    d.from_host(a)
    return d


def zbuf(client, nbytes):
    return dbuf(client, np.zeros(max(nbytes, 16), np.uint8))


@pytest.fixture
def clients(pkg):
    made = []

    def make(n):
        new = [pkg.SketchClient(decode_responses=True, device=0) for _ in range(n)]
        made.extend(new)
        return new
    yield make
    for c in made:
        c.flushall()


def rc_of(client, name, *args):
    """the raw return code of a C-ABI call"""
    return getattr(client.ctx.lib, name)(client.ctx.ptr, *args)


def vp(d):
    return None if d is None else C.c_void_p(d.ptr if hasattr(d, "ptr") else int(d))


# ================================================================ Count-Min
@pytest.mark.parametrize("dims", [SMALL, LARGE])
@pytest.mark.parametrize("ntables", [1, 2, 3, 64])
@pytest.mark.parametrize("slack", [0, 12])
def test_cms_sum_of_arrays(pkg, clients, dims, ntables, slack):
    """ntables tables laid `stride` cells apart: the padded size, or more."""
    (cl,) = clients(1)
    width, depth = dims
    ncells = width * depth
    stride = ((ncells + 3) & ~3) + slack
    rng = np.random.default_rng(ncells + ntables + slack)
    tabs = rng.integers(0, 1 << 20, (ntables, stride), dtype=np.uint64)
    tabs[:, ::5] = rng.integers(0, 1 << 32, tabs[:, ::5].shape, dtype=np.uint64)  # some sums saturate
    tabs[:, ncells - 1] = U32 // max(ntables - 1, 1)                               # the last cell, near the edge
    counts = rng.integers(0, 1 << 50, ntables, dtype=np.uint64)
    cl.cms_initbydim("dst", width, depth)
    cl.cms_incrby("dst", [b"stale"], [7])  # dst is overwritten, not added to
    d = dbuf(cl, tabs.astype(np.uint32))
    cl.cms_sum_dev("dst", d, stride, counts)
    cl.ctx.call("ske_sync")
    got, count = cl.cms_table("dst")
    want = np.minimum(tabs[:, :ncells].sum(axis=0), np.uint64(U32)).astype(np.uint32).reshape(depth, width)
    assert np.array_equal(got, want)
    assert (want == U32).any() or ntables == 1
    assert count == int(counts.astype(object).sum())
    d.free()


def gather_tables(dst, sources, key):
    """the sources' tables copied behind one another into a buffer of dst's
    context (the all-gather); returns (buffer, stride, counts)"""
    p0, ncells = sources[0].cms_table_dev(key)
    stride = (ncells + 3) & ~3
    buf = zbuf(dst, len(sources) * stride * 4)
    counts = []
    for k, s in enumerate(sources):
        p, n = s.cms_table_dev(key)
        assert n == ncells and p % 16 == 0
        s.ctx.call("ske_sync")
        dst.ctx.call("ske_memcpy", C.c_void_p(buf.ptr + k * stride * 4), C.c_void_p(p), stride * 4, 2)
        counts.append(s.cms_info(key)["count"])
    return buf, stride, counts


@pytest.mark.parametrize("dims", [SMALL, LARGE])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_cms_sum_of_contexts(pkg, clients, dims, world):
    width, depth = dims
    cs = clients(world + 2)
    srcs, dst, one = cs[:world], cs[world], cs[world + 1]
    rng = np.random.default_rng(world)
    items = [str(int(x)).encode() for x in rng.zipf(1.3, 6000) % 700]
    for c in cs:
        c.cms_initbydim("k", width, depth)
    for r, s in enumerate(srcs):
        s.cms_add_packed("k", *pkg.pack(items[r::world]))
    one.cms_add_packed("k", *pkg.pack(items))
    buf, stride, counts = gather_tables(dst, srcs, "k")
    dst.cms_sum_dev("k", buf, stride, counts)
    dst.ctx.call("ske_sync")
    got, count = dst.cms_table("k")
    assert np.array_equal(got, one.cms_table("k")[0])
    assert np.array_equal(got, ref_table(items, width, depth))
    assert count == len(items) == one.cms_info("k")["count"]
    buf.free()


def test_cms_sum_saturates(pkg, clients):
    a, b, dst, one = clients(4)
    for c in (a, b, dst, one):
        c.cms_initbydim("k", *LARGE)
    for c in (a, b):
        c.cms_incrby("k", [b"hot", b"cold"], [0xC0000000, 5])
    one.cms_incrby("k", [b"hot", b"cold", b"hot", b"cold"], [0xC0000000, 5, 0xC0000000, 5])
    buf, stride, counts = gather_tables(dst, [a, b], "k")
    dst.cms_sum_dev("k", buf, stride, counts)
    dst.ctx.call("ske_sync")
    got, count = dst.cms_table("k")
    want, want_count = one.cms_table("k")
    assert np.array_equal(got, want)
    assert dst.cms_query("k", b"hot", b"cold") == [U32, 10]
    assert count == want_count == 2 * (0xC0000000 + 5)
    buf.free()


def test_cms_sum_count_overflow_and_rejections(pkg, clients):
    from rtsas_amd import _lib
    a, b, dst = clients(3)
    width, depth = SMALL
    ncells = width * depth
    for c in (a, b, dst):
        c.cms_initbydim("k", width, depth)
    cells = np.arange(1, ncells + 1, dtype=np.uint32)
    for c in (a, b):
        c.ctx.call("ske_cms_import", c.cms_cid("k"), cells.ctypes.data_as(C.c_void_p), ncells, U64)
    dst.cms_incrby("k", [b"mine"], [3])
    before = dst.cms_table("k")
    buf, stride, counts = gather_tables(dst, [a, b], "k")
    assert counts == [U64, U64]
    cid = dst.cms_cid("k")
    cnt = np.asarray(counts, np.uint64)
    cp = cnt.ctypes.data_as(C.c_void_p)
    assert rc_of(dst, "ske_cms_sum_dev", cid, vp(buf), stride, 2, cp) == _lib.SKE_ECMSOVERFLOW
    with pytest.raises(pkg.ResponseError, match="overflow"):
        dst.cms_sum_dev("k", buf, stride, counts)
    one = np.asarray([1, 2], np.uint64)
    op = one.ctypes.data_as(C.c_void_p)
    assert stride == 24
    for args in ((cid, vp(buf), 22, 2, op),                # not a multiple of 4
                 (cid, vp(buf), 20, 2, op),                # below width * depth
                 (cid, vp(buf), stride, 0, op),
                 (cid, vp(buf), stride, _lib.SKE_CMS_MAX_MERGE + 1, op),
                 (cid, vp(buf.ptr + 4), stride, 1, op),    # the base is not 16-byte aligned
                 (cid, None, stride, 2, op), (cid, vp(buf), stride, 2, None)):
        assert rc_of(dst, "ske_cms_sum_dev", *args) == _lib.SKE_EINVAL, args
    assert rc_of(dst, "ske_cms_sum_dev", cid + 1, vp(buf), stride, 2, op) == _lib.SKE_ECMSNOKEY
    p, n = C.c_void_p(), C.c_uint64()
    assert rc_of(dst, "ske_cms_table_dev", cid + 1, C.byref(p), C.byref(n)) == _lib.SKE_ECMSNOKEY
    dst.ctx.call("ske_sync")
    after = dst.cms_table("k")
    assert np.array_equal(before[0], after[0]) and before[1] == after[1] == 3
    # and the accepted call: 2^64 - 1 + 0 is no overflow
    dst.cms_sum_dev("k", buf, stride, [U64, 0])
    dst.ctx.call("ske_sync")
    got, count = dst.cms_table("k")
    assert np.array_equal(got.reshape(-1), 2 * cells) and count == U64
    buf.free()


# ================================================================ heavy-hitter sets
def make_set(pkg, client, ids, log2=12, table=SMALL, name="s", key="k"):
    """a set that holds exactly `ids` (tracked at 1 behind their adds)"""
    if client.keys.type_of(pkg.encode(key)) is None:
        client.cms_initbydim(key, *table)
    client.hh_create(name, key, log2)
    ids = list(ids)
    if ids:
        buf, offs = pkg.pack(ids)
        client.cms_add_packed(key, buf, offs)
        client.hh_track_packed(name, buf, offs, 1)


def export_set(src, into, name="s", cap=None):
    """(ids buffer, lens buffer, n, overflow) in `into`'s context"""
    used = src.hh_info(name)["used"]
    cap = max(used, 1) if cap is None else cap
    ids, lens = zbuf(into, cap * 16), zbuf(into, cap * 4)
    n, ov = src.hh_export_dev(name, ids, lens, cap)  # returns when done
    return ids, lens, n, ov


def merge_sets(dst, sources, name="s", key="k"):
    """the union of the sources' sets and the sum of their tables into dst"""
    buf, stride, counts = gather_tables(dst, sources, key)
    dst.cms_sum_dev(key, buf, stride, counts)
    keep = [buf]
    for s in sources:
        ids, lens, n, ov = export_set(s, dst, name)
        dst.hh_merge_dev(name, ids, lens, n, ov)
        keep += [ids, lens]
    dst.ctx.call("ske_sync")
    for b in keep:
        b.free()


def wrapping_ids(orc, log2, count):
    """ids whose digest starts at the last slot of a 2^log2 set: the walk wraps"""
    out, i = [], 0
    while len(out) < count:
        cand = b"w%d" % i
        if digest(orc, cand) & ((1 << log2) - 1) == (1 << log2) - 1:
            out.append(cand)
        i += 1
    return out


def set_ids(n, seed):
    rng = np.random.default_rng(seed)
    ids = {b"", b"0123456789abcdef", bytes(16)}  # the empty id, full-length ids
    while len(ids) < n + 3:
        cand = bytes(rng.integers(0, 256, int(rng.integers(1, 17)), dtype=np.uint8))
        # b"\x01" shares the empty id's digest (the Bloom seed is MurmurHash64A's own
        # multiplier, so seed ^ 1 * m is 0 and the tail byte 1 brings m back): one entry
        if cand != b"\x01":
            ids.add(cand)
    return sorted(ids)[:n] if n < 3 else sorted(ids)[:n - 2] + [b"", b"0123456789abcdef"]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_set_union_equals_one_context(pkg, orc, clients, n):
    """three sources: every id in all three (the same id in every source), plus
    ids of their own, plus ids that wrap the walk"""
    log2 = 12
    common = set_ids(n, n)
    wrap = wrapping_ids(orc, log2, 6)
    own = [[b"own%d_%d" % (r, i) for i in range(n // 3)] + (wrap[2 * r:2 * r + 2] if n >= 63 else [])
           for r in range(3)]
    union = set(common) | {i for o in own for i in o}
    assert_distinct_digests(orc, union)
    assert len(union) <= (1 << log2) // 2
    cs = clients(5)
    srcs, dst, one = cs[:3], cs[3], cs[4]
    everything = []
    for r, s in enumerate(srcs):
        # a source counts some ids more than once: the estimates differ
        batch = common + own[r] + common[:n // 2]
        make_set(pkg, s, batch, log2)
        everything += batch
    make_set(pkg, dst, [], log2)
    make_set(pkg, one, everything, log2)
    merge_sets(dst, srcs)
    table = ref_table(everything, *SMALL)
    assert np.array_equal(dst.cms_table("k")[0], table)
    info = dst.hh_info("s")
    assert info["used"] == len(union) == one.hh_info("s")["used"] and info["overflow"] == 0
    for thr in (1, 2, 3, 4, 7, 10 ** 6):
        got = dst.hh_list("s", thr)
        want = one.hh_list("s", thr)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and got[2] and want[2]
        ids, est = ref_listing(table, union, thr)
        assert got[0] == ids and got[1].tolist() == est
    for thr in (0, 3):  # (assert_equal: an empty set's mean, median and std are nan on both sides)
        np.testing.assert_equal(dst.hh_stats("s", thr), one.hh_stats("s", thr))
        assert dst.hh_stats("s", thr)["n"] == len(ref_listing(table, union, thr)[0])
    m = len(union)
    if m:
        ranks = [0, (m - 1) // 2, m // 2, m - 1]
        got = dst.hh_select("s", ranks)
        assert np.array_equal(got, one.hh_select("s", ranks))
        assert got.tolist() == [int(x) for x in np.sort(ref_query(table, sorted(union)))[ranks]]
    # the view is rebuilt, never double counted: reset and merge again
    dst.hh_reset("s")
    assert dst.hh_info("s")["used"] == 0
    merge_sets(dst, srcs)
    again = dst.hh_list("s", 1)
    want = one.hh_list("s", 1)
    assert again[0] == want[0] and np.array_equal(again[1], want[1]) and again[2]
    assert dst.hh_info("s")["used"] == len(union)


@pytest.mark.parametrize("shape", ["disjoint", "identical", "half"])
def test_set_union_sizes(pkg, orc, clients, shape):
    a_ids = [b"id%04d" % i for i in range(200)]
    b_ids = {"disjoint": [b"id%04d" % i for i in range(200, 400)], "identical": a_ids,
             "half": [b"id%04d" % i for i in range(100, 300)]}[shape]
    union = set(a_ids) | set(b_ids)
    assert_distinct_digests(orc, union)
    a, b, dst = clients(3)
    make_set(pkg, a, a_ids, 10)
    make_set(pkg, b, b_ids, 10)
    make_set(pkg, dst, [], 10)
    merge_sets(dst, [a, b])
    assert dst.hh_info("s") == {"capacity": 1024, "used": len(union), "overflow": 0}
    ids, est, complete = dst.hh_list("s", 1)
    assert sorted(ids) == sorted(union) and complete


def hand_entries(client, entries):
    """device arrays of hand-made (16 raw bytes, length) entries"""
    ids = np.zeros((len(entries), 16), np.uint8)
    for i, (raw, _) in enumerate(entries):
        ids[i, :len(raw)] = np.frombuffer(raw, np.uint8)
    lens = np.asarray([ln for _, ln in entries], np.uint32)
    return dbuf(client, ids), dbuf(client, lens)


def test_set_merge_one_id_many_times(pkg, clients):
    (dst,) = clients(1)
    make_set(pkg, dst, [b"seed"], 8)
    ids, lens = hand_entries(dst, [(b"racer", 5)] * 4096)
    dst.hh_merge_dev("s", ids, lens, 4096, 0)
    dst.ctx.call("ske_sync")
    assert dst.hh_info("s") == {"capacity": 256, "used": 2, "overflow": 0}
    assert sorted(dst.hh_list("s", 0)[0]) == [b"racer", b"seed"]


def test_set_merge_masks_lengths_and_flags(pkg, clients):
    dst, other = clients(2)
    make_set(pkg, dst, [], 8)
    make_set(pkg, other, [], 8)
    # garbage behind len does not make a second member
    ids, lens = hand_entries(dst, [(b"abc", 3), (b"abc\xff\x01garbage!", 3), (b"abcdefgh\x07junk", 8),
                                   (b"abcdefgh", 8), (b"abcdefghij\x99\x98", 10), (b"abcdefghij", 10),
                                   (b"\xaa" * 16, 0), (b"", 0), (b"0123456789abcdef", 16)])
    dst.hh_merge_dev("s", ids, lens, 9, 0)
    dst.ctx.call("ske_sync")
    assert dst.hh_info("s") == {"capacity": 256, "used": 5, "overflow": 0}
    got, _, complete = dst.hh_list("s", 0)
    assert sorted(got) == sorted([b"abc", b"abcdefgh", b"abcdefghij", b"", b"0123456789abcdef"]) and complete
    # a length of 17 is skipped and flags
    ids2, lens2 = hand_entries(dst, [(b"fine", 4), (b"0123456789abcdef", 17)])
    dst.hh_merge_dev("s", ids2, lens2, 2, 0)
    dst.ctx.call("ske_sync")
    info = dst.hh_info("s")
    assert info["used"] == 6 and info["overflow"] != 0
    assert dst.hh_list("s", 0)[2] is False
    # foreign_overflow alone makes the union incomplete
    other.hh_merge_dev("s", None, None, 0, 1)
    other.ctx.call("ske_sync")
    assert other.hh_info("s") == {"capacity": 256, "used": 0, "overflow": 1}
    assert other.hh_stats("s", 0)["complete"] is False


def test_set_merge_refuses_at_the_load_limit(pkg, orc, clients):
    from rtsas_amd import _lib
    a, b, dst = clients(3)
    a_ids = [b"a%03d" % i for i in range(100)]
    b_ids = [b"b%03d" % i for i in range(100)]
    make_set(pkg, a, a_ids, 8)
    make_set(pkg, b, b_ids, 8)
    make_set(pkg, dst, [], 8)
    assert a.hh_info("s")["used"] == b.hh_info("s")["used"] == 100
    merge_sets(dst, [a, b])
    info = dst.hh_info("s")
    assert info["overflow"] != 0 and 128 <= info["used"] <= 256
    got, _, complete = dst.hh_list("s", 0)
    assert complete is False and set(got) <= set(a_ids) | set(b_ids) and len(got) == info["used"]
    # cap below used: SKE_EHHSPACE, n_out right
    ids, lens = zbuf(a, 99 * 16), zbuf(a, 99 * 4)
    n, ov = C.c_uint64(0), C.c_uint32(7)
    hid = a._hh_entry("s")[0]
    assert rc_of(a, "ske_hh_export_dev", hid, vp(ids), vp(lens), 99, C.byref(n), C.byref(ov)) == _lib.SKE_EHHSPACE
    assert n.value == 100 and ov.value == 0
    with pytest.raises(pkg.SketchLibError):
        a.hh_export_dev("s", ids, lens, 99)
    assert rc_of(a, "ske_hh_export_dev", hid + 1, vp(ids), vp(lens), 99, C.byref(n), C.byref(ov)) == _lib.SKE_EHHNOSET
    assert rc_of(a, "ske_hh_merge_dev", hid + 1, vp(ids), vp(lens), 1, 0) == _lib.SKE_EHHNOSET
    assert rc_of(a, "ske_hh_merge_dev", hid, None, vp(lens), 1, 0) == _lib.SKE_EINVAL


# ================================================================ tallies
def make_tally(client, keys, valid=None, log2=12, name="t"):
    client.tally_create(name, log2)
    if keys:
        client.tally_add(name, keys, valid)


def export_tally(src, into, name="t", cap=None):
    used = src.tally_info(name)["used"]
    cap = max(used, 1) if cap is None else cap
    bufs = [zbuf(into, cap * 32), zbuf(into, cap * 4), zbuf(into, cap * 8), zbuf(into, cap * 8)]
    n = src.tally_export_dev(name, *bufs, cap)  # returns when done
    return bufs, n


def merge_tallies(dst, sources, name="t"):
    keep = []
    for s in sources:
        bufs, n = export_tally(s, dst, name)
        info = s.tally_info(name)
        dst.tally_merge_dev(name, *bufs, n, info["dropped_events"], info["dropped_valid"], info["overflow"])
        keep += bufs
    dst.ctx.call("ske_sync")
    for b in keep:
        b.free()


def head_holds(client, name="t"):
    keys, ev, va, _ = client.tally_list(name)
    info = client.tally_info(name)
    assert int(ev.astype(object).sum()) + info["dropped_events"] == info["taken"]
    assert (va <= ev).all()
    return info, int(va.astype(object).sum()) + info["dropped_valid"]


def lecture_stream(n, seed, nkeys=300):
    rng = np.random.default_rng(seed)
    pool = [b"", b"A", b"A\0", b"L" * 32] + [b"lec%d" % i for i in range(nkeys)]
    keys = [pool[i] for i in np.minimum(rng.zipf(1.2, n) - 1, rng.integers(0, len(pool), n))]
    keys[:4] = pool[:4]
    return keys, (rng.random(n) < 0.8).astype(np.uint8)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_tally_sum_equals_one_context(pkg, clients, world):
    cs = clients(world + 2)
    srcs, dst, one = cs[:world], cs[world], cs[world + 1]
    keys, valid = lecture_stream(5000, world)
    for r, s in enumerate(srcs):
        # every source also sees the four edge keys: a key present in all sources
        make_tally(s, keys[r::world] + keys[:4], np.concatenate([valid[r::world], valid[:4]]))
    make_tally(dst, [])
    all_keys = keys + keys[:4] * world
    all_valid = np.concatenate([valid] + [valid[:4]] * world)
    make_tally(one, all_keys, all_valid)
    merge_tallies(dst, srcs)
    got, want = dst.tally_list("t"), one.tally_list("t")
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert got[3] and want[3]
    events = Counter(all_keys)
    valids = Counter(k for k, v in zip(all_keys, all_valid) if v)
    assert dict(zip(got[0], got[1].tolist())) == dict(events)
    assert dict(zip(got[0], got[2].tolist())) == {k: valids[k] for k in events}
    assert events[b"A"] and events[b"A\0"] and events[b""] and events[b"L" * 32]
    info, valid_total = head_holds(dst)
    assert info["taken"] == len(all_keys) and valid_total == int(all_valid.sum())
    assert dst.tally_info("t") == one.tally_info("t")
    ev, va = dst.tally_query("t", [b"A", b"A\0", b"absent"])
    assert ev.tolist() == [events[b"A"], events[b"A\0"], 0]


def test_tally_merge_carries_drops_and_refuses(pkg, clients):
    from rtsas_amd import _lib
    small, other, dst, tight = clients(4)
    many = [b"key%04d" % i for i in range(300)] * 2          # 300 keys into 2^8 slots: some are refused
    few = [b"key%04d" % i for i in range(50)] * 3
    make_tally(small, many, np.ones(len(many), np.uint8), log2=8)
    make_tally(other, few, np.zeros(len(few), np.uint8), log2=8)
    sinfo = small.tally_info("t")
    assert sinfo["overflow"] and sinfo["dropped_events"] > 0 and sinfo["taken"] == 600
    # into a roomy destination: the source's drops arrive in the head
    make_tally(dst, [])
    merge_tallies(dst, [small, other])
    info, valid_total = head_holds(dst)
    assert info["taken"] == 600 + 150 and valid_total == 600
    assert info["dropped_events"] == sinfo["dropped_events"] and info["dropped_valid"] == sinfo["dropped_valid"]
    assert info["overflow"] != 0 and dst.tally_list("t")[3] is False
    # a destination at its load limit: two disjoint 100-key sources into 2^8 slots
    a, b = clients(2)
    make_tally(a, [b"a%03d" % i for i in range(100)] * 2, None, log2=8)
    make_tally(b, [b"b%03d" % i for i in range(100)], np.ones(100, np.uint8), log2=8)
    make_tally(tight, [], log2=8)
    merge_tallies(tight, [a, b])
    info, valid_total = head_holds(tight)
    assert info["overflow"] != 0 and 128 <= info["used"] <= 256
    assert info["taken"] == 300 and info["dropped_events"] > 0 and valid_total == 100
    # cap below used: SKE_ETALLYSPACE, n_out right
    bufs = [zbuf(a, 99 * 32), zbuf(a, 99 * 4), zbuf(a, 99 * 8), zbuf(a, 99 * 8)]
    n = C.c_uint64(0)
    tid = a.tally_tid("t")
    assert rc_of(a, "ske_tally_export_dev", tid, *[vp(x) for x in bufs], 99, C.byref(n)) == _lib.SKE_ETALLYSPACE
    assert n.value == 100
    assert rc_of(a, "ske_tally_export_dev", tid + 1, *[vp(x) for x in bufs], 99, C.byref(n)) == _lib.SKE_ETALLYNOSET
    assert rc_of(a, "ske_tally_merge_dev", tid + 1, *[vp(x) for x in bufs], 1, 0, 0, 0) == _lib.SKE_ETALLYNOSET
    # a length over 32 goes the too-long way: dropped, overflow set
    (fresh,) = clients(1)
    make_tally(fresh, [])
    kb = np.zeros((2, 32), np.uint8)
    kb[0, :2] = (65, 66)
    d = [dbuf(fresh, kb), dbuf(fresh, np.asarray([2, 33], np.uint32)), dbuf(fresh, np.asarray([5, 9], np.uint64)),
         dbuf(fresh, np.asarray([1, 4], np.uint64))]
    fresh.tally_merge_dev("t", *d, 2)
    fresh.ctx.call("ske_sync")
    assert fresh.tally_info("t") == {"capacity": 4096, "used": 1, "overflow": 1, "taken": 14, "dropped_events": 9,
                                     "dropped_valid": 4}
    k, ev, va, complete = fresh.tally_list("t")
    assert (k, ev.tolist(), va.tolist(), complete) == ([b"AB"], [5], [1], False)


# ================================================================ ShardedCounts
class ThreadTransport:
    """The stub process group: `world` threads of this process, one per rank,
    exchange their tensors at a barrier.  Only the transport is faked; the ops
    are the real LibsketchCountsOps of every rank's context."""

    class Shared:
        def __init__(self, world):
            self.world = world
            self.barrier = threading.Barrier(world, timeout=120)
            self.slots = [None] * world

    def __init__(self, shared, rank):
        self.shared, self.rank, self.world = shared, rank, shared.world

    def _exchange(self, t):
        sh = self.shared
        sh.slots[self.rank] = t
        sh.barrier.wait()
        every = list(sh.slots)
        sh.barrier.wait()
        return every

    def all_gather(self, t):
        import torch
        if t.is_cuda:
            torch.cuda.synchronize()
        out = torch.stack(self._exchange(t))
        if t.is_cuda:
            torch.cuda.synchronize()
        return out

    def gather_ints(self, words, device):
        return np.stack(self._exchange(np.ascontiguousarray(words, dtype=np.int64)))

    def sum_ints(self, words, device):
        return np.stack(self._exchange(np.array(words, dtype=np.int64))).sum(axis=0)


def run_ranks(world, fn):
    """fn(rank) on `world` threads; the first exception is raised here"""
    errors = [None] * world
    shared = ThreadTransport.Shared(world)

    def body(r):
        try:
            fn(r, ThreadTransport(shared, r))
        except BaseException as e:  # noqa: BLE001
            errors[r] = e
            shared.barrier.abort()
    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    real = [e for e in errors if e is not None and not isinstance(e, threading.BrokenBarrierError)]
    if real or any(errors):
        raise (real or [e for e in errors if e is not None])[0]


OPTS = dict(track_attended=1, track_invalid=1, capacity_log2=12, late_key="cms:late", track_late=1,
            day_profile="week", lecture_counts="lectures", lecture_capacity_log2=10, error=0.002, probability=0.01)
N_SWIPES, N_BATCHES = 4000, 4


def swipe_stream(pkg, seed=5):
    rng = np.random.default_rng(seed)
    roster = rng.choice(np.arange(10 ** 7, 10 ** 8), 600, replace=False)
    sids = np.where(rng.random(N_SWIPES) < 0.85, roster[np.minimum(rng.zipf(1.3, N_SWIPES) - 1, 599)],
                    rng.integers(10 ** 7, 10 ** 8, N_SWIPES))
    ids = np.frombuffer("".join(str(int(s)) for s in sids).encode(), np.uint8).reshape(N_SWIPES, 8).copy()
    lectures = ["CS%03d" % l for l in np.minimum(rng.zipf(1.4, N_SWIPES) - 1, 59)]
    days = rng.integers(17, 24, N_SWIPES)
    times = (np.datetime64("2025-03-17T00:00:00").astype("datetime64[s]").astype(np.int64)
             + (days - 17) * 86400 + rng.integers(6 * 3600, 14 * 3600, N_SWIPES))
    keys = ["hll:unique:%s:2025-03-%02d" % (l, d) for l, d in zip(lectures, days)]
    return roster, ids, lectures, times, keys


def feed(pkg, client, counts, roster, ids, lectures, times, keys, rows):
    """the rows of one batch that this context processes, through update()"""
    if len(rows) == 0:
        return
    slots = np.asarray([client.key_slot(keys[i]) for i in rows], np.uint32)
    counts.update("bf:students", slots, ids[rows], times[rows], [lectures[i] for i in rows])


def new_rank(pkg, client, roster, **opts):
    client.execute_command("BF.RESERVE", "bf:students", 0.001, 5000)
    client.bf_madd_packed("bf:students", *pkg.pack_ints(roster))
    return pkg.StudentCounts(client, **dict(OPTS, **opts))


QUERIES = (dict(), dict(attended_threshold=3, invalid_threshold=2, late_threshold=2),
           dict(attended_threshold="reference", late_threshold="reference"),
           dict(attended_threshold="reference", invalid_threshold="reference", late_threshold="reference",
                lecture_k=5))


@pytest.mark.parametrize("split", ["round-robin", "route"])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_sharded_counts_equal_one_context(pkg, clients, world, split):
    from rtsas_amd.distributed import ShardedCounts, route
    roster, ids, lectures, times, keys = swipe_stream(pkg)
    cs = clients(world + 1)
    one_client, rank_clients = cs[0], cs[1:]
    one = new_rank(pkg, one_client, roster)
    locals_ = [new_rank(pkg, c, roster) for c in rank_clients]
    dest = route(keys, world) if split == "route" else np.arange(N_SWIPES) % world
    sharded = [None] * world

    def construct(r, transport):
        sharded[r] = ShardedCounts(locals_[r], r, world, transport=transport)
    run_ranks(world, construct)
    per = N_SWIPES // N_BATCHES
    results = [None] * world
    for half in range(2):          # several batches between two merges
        for b in range(2 * half, 2 * half + 2):
            rows = np.arange(b * per, (b + 1) * per)
            feed(pkg, one_client, one, roster, ids, lectures, times, keys, rows)
            for r in range(world):
                feed(pkg, rank_clients[r], locals_[r], roster, ids, lectures, times, keys, rows[dest[rows] == r])

        def query(r, transport):
            sc = sharded[r]
            res = [sc.insights(**q) for q in QUERIES]   # collective: merge, then the view's insights
            tables = [sc.ops.client.cms_table(k) for k in sc.ops.view_cms_keys()]
            results[r] = (res, sc.lecture_rankings(4), sc.lecture_rankings(3, by="valid"), sc.by_hour_of_week(),
                          tables, sc.population("attended"), sc.by_day())
        run_ranks(world, query)
        want_ins = [one.insights(**q) for q in QUERIES]
        want_tables = [one_client.cms_table(k) for k in (one.attended_key, one.invalid_key, one.late_key)]
        for r in range(world):
            res, ranks, ranks_valid, hours, tables, population, by_day = results[r]
            assert res == want_ins, (world, split, r)
            assert all(i.get("complete", True) for q in res for i in q)
            assert ranks == one.lecture_rankings(4) and ranks["complete"]
            assert ranks_valid == one.lecture_rankings(3, by="valid")
            assert np.array_equal(hours, one.by_hour_of_week()) and int(hours.sum()) == (half + 1) * 2 * per
            for (t, c), (wt, wc) in zip(tables, want_tables):
                assert np.array_equal(t, wt) and c == wc
            np.testing.assert_equal(population, one.population("attended"))
            assert by_day == one.by_day() and population["n"] > 10
    # the plain truths, independent of the code under test: valid by the one
    # context's BF.EXISTS answers, counted in Python
    valid = one_client.bf_mexists_packed("bf:students", *pkg.pack([bytes(r) for r in ids])).astype(bool)
    sc = sharded[0]
    id_bytes = [bytes(r) for r in ids]
    att = Counter(i for i, v in zip(id_bytes, valid) if v)
    inv = Counter(i for i, v in zip(id_bytes, valid) if not v)
    w, d = sc.ops.client.cms_info(sc.view.attended_key)["width"], sc.ops.client.cms_info(sc.view.attended_key)["depth"]
    assert np.array_equal(sc.ops.client.cms_table(sc.view.attended_key)[0],
                          ref_table(list(att), w, d, [att[i] for i in att]))
    assert np.array_equal(sc.ops.client.cms_table(sc.view.invalid_key)[0],
                          ref_table(list(inv), w, d, [inv[i] for i in inv]))
    got_ids, _, complete = sc.top_attended()
    assert set(got_ids) == set(att) and complete            # membership: a Python set
    assert set(sc.top_invalid()[0]) == set(inv)
    ev, va = sc.lecture_events(sorted(set(lectures)))
    lec_events = Counter(lectures)
    lec_valid = Counter(l for l, v in zip(lectures, valid) if v)
    assert ev.tolist() == [lec_events[l] for l in sorted(set(lectures))]
    assert va.tolist() == [lec_valid[l] for l in sorted(set(lectures))]
    # counting goes to the local object, which merge() never touches
    assert sc.timed and sc.counts_lectures
    if world > 1:
        assert int(sc.local.by_hour_of_week().sum()) < N_SWIPES


def test_sharded_counts_threshold_guarantee(pkg, clients):
    """t = 3 over 2 ranks: the view refuses a list threshold of 4 and at 5 lists
    every id whose true count is at least 5."""
    from rtsas_amd.distributed import ShardedCounts
    roster, ids, lectures, times, keys = swipe_stream(pkg, seed=9)
    world = 2
    rank_clients = clients(world)
    locals_ = [new_rank(pkg, c, roster, track_attended=3, track_invalid=3, track_late=3) for c in rank_clients]
    sharded = [None] * world

    def construct(r, transport):
        sharded[r] = ShardedCounts(locals_[r], r, world, transport=transport)
    run_ranks(world, construct)
    per = N_SWIPES // N_BATCHES
    for b in range(N_BATCHES):
        rows = np.arange(b * per, (b + 1) * per)
        for r in range(world):
            feed(pkg, rank_clients[r], locals_[r], roster, ids, lectures, times, keys, rows[rows % world == r])
    run_ranks(world, lambda r, transport: sharded[r].merge())
    valid = rank_clients[0].bf_mexists_packed("bf:students", *pkg.pack([bytes(r) for r in ids])).astype(bool)
    att = Counter(bytes(i) for i, v in zip(ids, valid) if v)
    for sc in sharded:
        assert sc.view._track_of(sc.view.attended_key)[1] == 5
        with pytest.raises(ValueError):
            sc.top_attended(threshold=4)
        got, est, complete = sc.top_attended(threshold=5)
        assert complete
        must = {i for i, c in att.items() if c >= 5}
        assert must and must <= set(got)
        assert all(int(e) >= att[i] for i, e in zip(got, est))


def test_processor_takes_sharded_counts(pkg, clients):
    """AttendanceProcessor(counts=ShardedCounts(...)) counts into the local
    object and its insights are the merged view's."""
    from rtsas_amd.distributed import ShardedCounts
    (client,) = clients(1)
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 1000)
    local = pkg.StudentCounts(client, track_attended=1, track_invalid=1, capacity_log2=10, lecture_counts="lectures")
    sc = ShardedCounts(local, 0, 1)
    proc = pkg.AttendanceProcessor(client, pkg.AttendanceConfig(cassandra_row_types=False), counts=sc)
    assert proc.counts.timed is False and proc.counts.counts_lectures is True
    buf, offs = pkg.pack([b"10000001", b"10000002", b"10000001"])
    proc.counts.count_packed(buf, offs, [1, 0, 1], None, ["CS1", "CS1", "CS2"])
    assert sc.view.insights()[1]["data"] == {}   # counted locally; the view is as of the last merge
    ins = proc.insights()                          # merge, then the view's insights
    assert ins == sc.view.insights()
    assert [i["title"] for i in ins] == ["Lecture Attendance Rankings", "Most Consistent Attendees",
                                         "Invalid Attendance Attempts"]
    assert ins[0]["data"]["most_attended"] == {"CS1": 2, "CS2": 1}
    assert ins[1]["data"] == {"10000001": 2} and ins[2]["data"] == {"10000002": 1}
