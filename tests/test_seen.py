"""Seen-row sets on the device (csrc/sketch_seen.hip) against a Python dict from
key to first index: the add's answer bytes, ``info`` and ``test`` over sizes,
populations and masks; several calls; a small grid; hand-placed keys (chains,
the wrap at the table's end, equal words); overflow, which fails open;
determinism; a recorded add replayed; and the device folds against the Python
restatement ``client_seen.seen_row_keys``."""
import ctypes as C
import os

import numpy as np
import pytest

import __graft_entry__ as ge

pytestmark = pytest.mark.gpu

FIRST, REPEAT, SKIPPED = 0, 1, 2
SIZES = (0, 1, 63, 64, 65, 1025, 100003)
POPULATIONS = ("distinct", "one", "adjacent", "apart64", "half", "zipf37")
MASKS = ("none", "zeros", "ones", "random85")


def make_client(grid=None):
    """a client on a context opened with SKE_SEEN_GRID (ske_open reads it)"""
    pkg = ge.load_package()
    if grid is not None:
        os.environ["SKE_SEEN_GRID"] = str(grid)
    try:
        return pkg.SketchClient(context=pkg.Context(0))
    finally:
        os.environ.pop("SKE_SEEN_GRID", None)


@pytest.fixture(scope="module")
def cl():
    c = make_client()
    yield c
    c.flushall()


@pytest.fixture(scope="module")
def small():
    """two workgroups: 512 threads walk 1025 items in three turns of the stride loop"""
    c = make_client(2)
    yield c
    c.flushall()


class Oracle:
    """the set as a dict from key to the (call, index) of its first sighting"""

    def __init__(self):
        self.members, self.calls, self.looked_at, self.first = {}, 0, 0, 0

    def add(self, keys, mask=None, want=0):
        out = np.empty(len(keys), np.uint8)
        for i, (k0, k1) in enumerate(keys.tolist()):
            if mask is not None and mask[i] != want:
                out[i] = SKIPPED
                continue
            self.looked_at += 1
            k = (k0 or 1, k1 or 1)
            if k in self.members:
                out[i] = REPEAT
            else:
                self.members[k] = (self.calls, i)
                self.first += 1
                out[i] = FIRST
        self.calls += len(keys) > 0
        return out

    def present(self, keys):
        return np.asarray([(k0 or 1, k1 or 1) in self.members for k0, k1 in keys.tolist()], bool)

    def check_info(self, info, log2):
        assert info == {"capacity": 1 << log2, "limit": 1 << (log2 - 1), "used": len(self.members),
                        "calls": self.calls, "looked_at": self.looked_at, "first": self.first, "unplaced": 0}


def pool(rng, m):
    return rng.integers(0, 2 ** 64, (m, 2), dtype=np.uint64)


def keys_of(pop, n, seed=0):
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(n)
    if pop == "distinct":
        idx = i
    elif pop == "one":
        idx = np.zeros(n, np.int64)
    elif pop == "adjacent":  # each key twice at neighbouring indices: the same wavefront
        idx = i // 2
    elif pop == "apart64":  # twice 64 apart: the neighbouring wavefront
        idx = (i // 128) * 64 + i % 64
    elif pop == "half":  # twice n / 2 apart
        idx = i % max((n + 1) // 2, 1)
    else:
        idx = np.minimum(rng.zipf(1.3, n), 37) - 1
    p = pool(rng, int(idx.max()) + 1 if n else 1)
    return np.ascontiguousarray(p[idx])


def mask_of(kind, n, seed=0):
    if kind == "none":
        return None
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "ones":
        return np.ones(n, np.uint8)
    return (np.random.default_rng(77 + seed).random(n) >= 0.85).astype(np.uint8)


@pytest.fixture(scope="module")
def table(cl):
    cl.seen_create("t", 18)
    return "t"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pop", POPULATIONS)
def test_sizes_and_populations(cl, table, pop, n):
    keys = keys_of(pop, n)
    fresh = pool(np.random.default_rng(5), 9)
    for kind in MASKS:
        cl.seen_reset(table)
        want, mask = Oracle(), mask_of(kind, n)
        got = cl.seen_add_keys(table, keys, mask, 0)
        exp = want.add(keys, mask, 0)
        assert np.array_equal(got, exp), (kind, np.nonzero(got != exp)[0][:8])
        want.check_info(cl.seen_info(table), 18)
        probe = np.concatenate([keys, fresh])
        assert np.array_equal(cl.seen_test_keys(table, probe), want.present(probe)), kind
        # the test inserted nothing
        want.check_info(cl.seen_info(table), 18)


def test_two_and_three_calls(cl, table):
    rng = np.random.default_rng(9)
    n = 1025
    cl.seen_reset(table)
    want = Oracle()
    a = keys_of("adjacent", n, seed=1)
    mask = mask_of("random85", n, seed=1)
    for _ in range(2):
        got = cl.seen_add_keys(table, a, mask, 0)
        assert np.array_equal(got, want.add(a, mask, 0))
    assert set(got.tolist()) == {REPEAT, SKIPPED}  # the same batch again: every let-through item repeats
    # half old, half new, shuffled: FIRST exactly at the new keys' lowest indices
    new = pool(rng, 300)
    b = np.concatenate([a[mask == 0][:400], new, new[:150]])
    b = np.ascontiguousarray(b[rng.permutation(len(b))])
    got = cl.seen_add_keys(table, b)
    assert np.array_equal(got, want.add(b))
    firsts = {}
    for i, k in enumerate(map(tuple, b.tolist())):
        firsts.setdefault(k, i)
    newset = set(map(tuple, new.tolist()))
    assert sorted(np.nonzero(got == FIRST)[0].tolist()) == sorted(i for k, i in firsts.items() if k in newset)
    want.check_info(cl.seen_info(table), 18)


def test_small_grid(cl, small, table):
    small.seen_create("s", 18)
    try:
        for pop in POPULATIONS:
            keys = keys_of(pop, 1025, seed=2)
            mask = mask_of("random85", 1025, seed=2)
            cl.seen_reset(table)
            small.seen_reset("s")
            want = Oracle()
            for _ in range(2):
                exp = want.add(keys, mask, 0)
                assert np.array_equal(small.seen_add_keys("s", keys, mask, 0), exp), pop
                assert np.array_equal(cl.seen_add_keys(table, keys, mask, 0), exp), pop
            assert small.seen_info("s") == cl.seen_info(table)
            want.check_info(small.seen_info("s"), 18)
    finally:
        small.seen_drop("s")


def placed(k0s, k1s):
    return np.ascontiguousarray(np.asarray([k0s, k1s], np.uint64).T)


def test_hand_placed_keys(cl):
    log2 = 10
    cl.seen_create("h", log2)
    try:
        want = Oracle()

        def both(keys):
            got = cl.seen_add_keys("h", keys)
            assert np.array_equal(got, want.add(keys)), keys
            assert cl.seen_test_keys("h", keys).all()
            return got

        # 40 keys whose k0 low bits are equal: one chain of 40 slots from slot 5
        chain = placed([(j + 1 << log2) | 5 for j in range(40)], [100 + j for j in range(40)])
        assert (both(chain) == FIRST).all() and (both(chain) == REPEAT).all()
        # not in the set, but on the chain's path: walks all 40 slots and the empty one behind
        assert not cl.seen_test_keys("h", placed([(99 << log2) | 5], [1])).any()
        # a chain that starts 3 slots before the table's end: it wraps
        wrap = placed([(j + 1 << log2) | 1021 for j in range(9)], [7] * 9)
        assert (both(wrap) == FIRST).all() and (both(wrap[::-1].copy()) == REPEAT).all()
        # equal k0, different k1: two rows
        same0 = placed([0xABC00 | 300, 0xABC00 | 300], [1, 2])
        assert both(same0).tolist() == [FIRST, FIRST]
        # equal k1, different k0
        same1 = placed([(1 << 40) | 400, (2 << 40) | 400], [0xFEED, 0xFEED])
        assert both(same1).tolist() == [FIRST, FIRST]
        # a word 0 behaves as 1
        zeros = placed([0, 1, 600, 600, 0], [5, 5, 0, 1, 0])
        assert both(zeros).tolist() == [FIRST, REPEAT, FIRST, REPEAT, FIRST]
        assert cl.seen_test_keys("h", placed([1, 0, 1], [5, 1, 1])).all()
        want.check_info(cl.seen_info("h"), log2)
        assert cl.seen_info("h")["used"] == 40 + 9 + 2 + 2 + 3
    finally:
        cl.seen_drop("h")


def test_overflow_fails_open(cl):
    """2^10 slots take 512 keys (SKE_SEEN_LOAD_DEN): 4000 distinct keys cannot all be held.
    Which of them find room is not fixed, so the invariants are checked."""
    log2 = 10
    cl.seen_create("o", log2)
    try:
        keys = pool(np.random.default_rng(21), 4000)
        out1 = cl.seen_add_keys("o", keys)
        info = cl.seen_info("o")
        assert info["used"] <= info["capacity"] and info["unplaced"] > 0
        assert not (out1 == REPEAT).any()  # every key is distinct: a REPEAT would be false
        assert info["looked_at"] == 4000 == info["first"]
        assert info["used"] + info["unplaced"] == 4000  # every key claimed one slot or found none
        present = cl.seen_test_keys("o", keys)
        assert present.sum() == info["used"]
        out2 = cl.seen_add_keys("o", keys)
        assert present[out2 == REPEAT].all()      # every REPEAT is a key the set holds
        assert (out2[~present] == FIRST).all()    # a key it does not hold counts again
        info2 = cl.seen_info("o")
        assert info2["looked_at"] == 8000 and info2["calls"] == 2
        assert info2["first"] == 4000 + int((out2 == FIRST).sum())
        assert info2["unplaced"] >= info["unplaced"] + int((~present).sum())
        assert info2["used"] <= info2["capacity"]
    finally:
        cl.seen_drop("o")


def test_determinism(cl):
    rng = np.random.default_rng(33)
    calls = [keys_of("zipf37", 100003, seed=3), keys_of("half", 100003, seed=4)]
    calls.append(np.ascontiguousarray(np.concatenate([calls[0][:500], pool(rng, 500), calls[1][:500]])))
    masks = [mask_of("random85", len(k), seed=j) for j, k in enumerate(calls)]
    outs = []
    for name in ("d1", "d2"):
        cl.seen_create(name, 18)
        try:
            outs.append([cl.seen_add_keys(name, k, m, 0) for k, m in zip(calls, masks)])
        finally:
            cl.seen_drop(name)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_errors(cl, pkg):
    from rtsas_amd import _lib
    with pytest.raises(pkg.ResponseError, match="does not exist"):
        cl.seen_add_keys("nope", np.zeros((1, 2), np.uint64))
    cl.seen_create("e", 8)
    try:
        keys = np.zeros((3, 2), np.uint64)
        with pytest.raises(ValueError):
            cl.seen_add_keys("e", keys, np.zeros(2, np.uint8))
        sid = cl.seen_sid("e")
        with pytest.raises(pkg.SketchLibError) as ei:
            cl.ctx.call("ske_seen_init", sid, 8)
        assert ei.value.code == _lib.SKE_ESEENEXISTS
        with pytest.raises(pkg.SketchLibError) as ei:
            cl.ctx.call("ske_seen_init", sid + 1, 31)
        assert ei.value.code == _lib.SKE_ESEENCAP
        with pytest.raises(pkg.SketchLibError) as ei:
            cl.ctx.call("ske_seen_info", sid + 1, C.byref(_lib.SeenInfo()))
        assert ei.value.code == _lib.SKE_ESEENNOSET
        out = np.zeros(3, np.uint8)
        for args in ((sid, C.c_void_p(8), 1, None, 0, out.ctypes.data_as(C.c_void_p)),   # keys not 16-byte aligned
                     (sid, None, 1, None, 0, out.ctypes.data_as(C.c_void_p)),
                     (sid, C.c_void_p(16), 2 ** 32 - 1, None, 0, out.ctypes.data_as(C.c_void_p))):
            with pytest.raises(pkg.SketchLibError) as ei:
                cl.ctx.call("ske_seen_add_async", *args)
            assert ei.value.code == _lib.SKE_EINVAL
        with pytest.raises(pkg.SketchLibError) as ei:  # a granularity below one second
            cl.ctx.call("ske_seen_fold_epoch_async", C.c_void_p(16), C.c_void_p(16), 0, 1, 1)
        assert ei.value.code == _lib.SKE_EINVAL
        assert cl.seen_info("e")["calls"] == 0
    finally:
        cl.seen_drop("e")


def test_graph_replays_see_new_calls(pkg, engine):
    """the fold and the add recorded once, replayed twice over the same buffers:
    the call counter lives on the device, so the second replay is a later call"""
    from rtsas_amd.engine import DeviceBuffer
    n, width = 1025, 5
    ids = np.frombuffer(b"".join(b"%05d" % (10000 + 7 * i) for i in range(n)), np.uint8)
    ep = np.arange(n, dtype=np.int64) - 500
    d_ids, d_ep = DeviceBuffer(engine.ctx, n * width + 64), DeviceBuffer(engine.ctx, n * 8 + 16)
    d_keys, d_out = DeviceBuffer(engine.ctx, n * 16), DeviceBuffer(engine.ctx, n + 16)
    d_ids.from_host(ids)
    d_ep.from_host(ep)
    engine.seen_init(1, 12)
    engine.seen_init(2, 12)
    g = None

    def step(sid):
        engine.ctx.call("ske_seen_fold_fixed_async", C.c_void_p(d_keys.ptr), C.c_void_p(d_ids.ptr), width, n, 1)
        engine.seen_fold_epoch(d_keys, d_ep, n, 1, False)
        engine.seen_add(sid, d_keys, n, d_out)

    try:
        step(2)  # a direct call first: it sizes the context scratch the recording pins
        engine.sync()
        assert (d_out.to_host(np.uint8, n) == FIRST).all()
        g = engine.capture(lambda: step(1))
        assert engine.seen_info(1)["calls"] == 0  # recording ran nothing
        g.launch()
        engine.sync()
        assert (d_out.to_host(np.uint8, n) == FIRST).all()
        g.launch()
        engine.sync()
        assert (d_out.to_host(np.uint8, n) == REPEAT).all()
        info = engine.seen_info(1)
        assert (info["calls"], info["used"], info["looked_at"], info["first"]) == (2, n, 2 * n, n)
    finally:
        if g is not None:
            g.free()
        engine.seen_free(1)
        engine.seen_free(2)
        for b in (d_ids, d_ep, d_keys, d_out):
            b.free()


# ---------------------------------------------------------------- the folds
def device_keys(ctx, d_keys, n):
    ctx.call("ske_sync")
    return d_keys.to_host(np.uint64, 2 * n).reshape(n, 2)


@pytest.mark.parametrize("granularity", [1, 86400])
def test_fold_parity_packed_and_spans(pkg, cl, granularity):
    """ids of 1 to 24 bytes and lectures of 0 to 40 bytes, every combination, the
    columns starting at every offset mod 8; negative epochs; against seen_row_keys"""
    from rtsas_amd.client_seen import seen_row_keys
    from rtsas_amd.engine import DeviceBuffer
    rng = np.random.default_rng(50 + granularity)
    ids = [bytes(rng.integers(1, 256, li, dtype=np.uint8)) for li in range(1, 25) for _ in range(41)]
    lecs = [bytes(rng.integers(1, 256, ll, dtype=np.uint8)) for _ in range(1, 25) for ll in range(41)]
    n = len(ids)
    ep = rng.integers(-5 * 86400, 5 * 86400, n).astype(np.int64)
    ep[:6] = (-1, 0, 86399, 86400, -86401, -86400)
    want = seen_row_keys(ids, ep, lecs, granularity)
    assert len({tuple(k) for k in want.tolist()}) == n
    ctx = cl.ctx
    bufs = {k: DeviceBuffer(ctx, 1 << 16) for k in ("ids", "lecs", "io", "lo", "il", "ll", "at", "ep")}
    d_keys = DeviceBuffer(ctx, n * 16)
    bufs["ep"].from_host(ep)
    try:
        for align in range(8):
            cols = {}
            for name, items in (("ids", ids), ("lecs", lecs)):
                blob = bytes(align) + b"".join(items)
                offs = np.zeros(n + 1, np.uint32)
                np.cumsum([len(x) for x in items], out=offs[1:])
                offs += align
                bufs[name].from_host(np.frombuffer(blob, np.uint8))
                cols[name] = offs
            bufs["io"].from_host(cols["ids"])
            bufs["lo"].from_host(cols["lecs"])
            bufs["il"].from_host(np.diff(cols["ids"]).astype(np.uint32))
            bufs["ll"].from_host(np.diff(cols["lecs"]).astype(np.uint32))
            p = {k: C.c_void_p(b.ptr) for k, b in bufs.items()}
            keys = C.c_void_p(d_keys.ptr)
            # lectures packed, ids as spans
            ctx.call("ske_seen_fold_packed_async", keys, p["lecs"], p["lo"], n, 1)
            ctx.call("ske_seen_fold_spans_async", keys, p["ids"], p["io"], p["il"], None, n, 0)
            ctx.call("ske_seen_fold_epoch_async", keys, p["ep"], granularity, n, 0)
            assert np.array_equal(device_keys(ctx, d_keys, n), want), align
            # lectures as spans, ids packed
            ctx.call("ske_seen_fold_spans_async", keys, p["lecs"], p["lo"], p["ll"], None, n, 1)
            ctx.call("ske_seen_fold_packed_async", keys, p["ids"], p["io"], n, 0)
            ctx.call("ske_seen_fold_epoch_async", keys, p["ep"], granularity, n, 0)
            assert np.array_equal(device_keys(ctx, d_keys, n), want), align
            # spans through `at`: item i is message at[i]
            at = rng.permutation(n).astype(np.uint32)
            bufs["at"].from_host(at)
            bufs["ep"].from_host(ep[at])
            ctx.call("ske_seen_fold_spans_async", keys, p["lecs"], p["lo"], p["ll"], p["at"], n, 1)
            ctx.call("ske_seen_fold_spans_async", keys, p["ids"], p["io"], p["il"], p["at"], n, 0)
            ctx.call("ske_seen_fold_epoch_async", keys, p["ep"], granularity, n, 0)
            assert np.array_equal(device_keys(ctx, d_keys, n), want[at]), align
            bufs["ep"].from_host(ep)
    finally:
        d_keys.free()
        for b in bufs.values():
            b.free()


def test_fold_parity_fixed(pkg, cl):
    """fixed-width columns of 1 to 24 bytes from a base at every offset mod 8"""
    from rtsas_amd.client_seen import SEEN_SEED0, SEEN_SEED1, seen_fold
    from rtsas_amd.engine import DeviceBuffer
    rng = np.random.default_rng(60)
    n = 67
    ctx = cl.ctx
    d_col, d_keys = DeviceBuffer(ctx, 8 + n * 24 + 64), DeviceBuffer(ctx, n * 16)
    try:
        for width in (1, 5, 7, 8, 9, 15, 16, 17, 24):
            rows = rng.integers(0, 256, (n, width), dtype=np.uint8)
            items = [r.tobytes() for r in rows]
            once = seen_fold([(SEEN_SEED0, SEEN_SEED1)] * n, items)
            twice = seen_fold(once, items[::-1])
            for align in range(8):
                d_col.from_host(np.frombuffer(bytes(align) + rows.tobytes(), np.uint8))
                base = C.c_void_p(d_col.ptr + align)
                ctx.call("ske_seen_fold_fixed_async", C.c_void_p(d_keys.ptr), base, width, n, 1)
                assert device_keys(ctx, d_keys, n).tolist() == [list(k) for k in once], (width, align)
                d_col.from_host(np.frombuffer(bytes(align) + rows[::-1].tobytes(), np.uint8))
                ctx.call("ske_seen_fold_fixed_async", C.c_void_p(d_keys.ptr), base, width, n, 0)
                assert device_keys(ctx, d_keys, n).tolist() == [list(k) for k in twice], (width, align)
    finally:
        d_col.free()
        d_keys.free()


def test_rows_facade(pkg, cl):
    """seen_add_rows / seen_test_rows build the keys on the device from the
    columns a caller has; the answers are those of the Python keys"""
    from rtsas_amd.client_seen import seen_row_keys
    ids = [12345, 12345, "12345", 99999, 12345, 12345]
    lectures = ["CS101", "CS101", "CS101", "CS101", "CS102", "CS101"]
    times = np.asarray([100, 100, 100, 100, 100, 86400 + 100], np.int64)
    cl.seen_create("r1", 10)
    cl.seen_create("r2", 10)
    cl.seen_create("rk", 10)
    try:
        assert cl.seen_add_rows("r1", ids, times, lectures).tolist() == [True, False, False, True, True, True]
        assert cl.seen_test_rows("r1", ids, times, lectures).all()
        assert not cl.seen_test_rows("r1", [12345], [101], ["CS101"]).any()
        # one row per lecture-day at granularity 86400
        assert cl.seen_add_rows("r2", ids, times + np.arange(6), lectures, 86400).tolist() == \
            [True, False, False, True, True, True]
        assert (cl.seen_add_keys("rk", seen_row_keys(ids, times, lectures)) == FIRST).tolist() == \
            [True, False, False, True, True, True]
        assert cl.seen_add_rows("r1", [], [], []).size == 0
    finally:
        for name in ("r1", "r2", "rk"):
            cl.seen_drop(name)
