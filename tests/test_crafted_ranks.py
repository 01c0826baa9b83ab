"""Every PFADD writer under crafted ranks: ids built by tests/crafted_ids.py to
hit a chosen register with a chosen rank, all 51 of them.

A PFADD rank is geometric, so random ids stop near rank 10 at a register of
one's choosing and ranks 29 .. 51 reach no writer at all.  The rank travels
through six byte-in-word CAS-max loops (k_pfadd, k_swipes / k_swipes_lds,
k_xr_finish, pass C, k_hll_apply, the window pass's LDS maximum), the
``register | rank << 16`` words of pass A and k_xr_hash, the segmented form's
``slot << 20 | register << 6 | rank`` records, its floor filter and its hint
estimate.  Here every arm gets, inside filler of its usual kind:

- the ladder: every rank 1 .. 51 on registers 0, 1, 2, 3 (one 32-bit word),
  127 | 128 (two 128-byte lines), 8191 and 16383 of two keys -- ascending,
  descending, shuffled, and wave-packed (every run of 64 consecutive items on
  the four bytes of one word of one key);
- one rank-51 id 64 times in a row;
- the same batch reversed as a second call, which must change nothing.

Answers and every register of every key equal ``oracle.process_swipes``; the
crafted ids are Bloom members through one BF.MADD on both sides (the replies
compared too).  The segmented form's floors get records one under, at and one
above a floor of 1, 31, 32, 50 and 51; the order-exact PFADD a strict 51-step
staircase, whose replies equal ``oracle.hll_madd``.  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import chain_shapes as cs
import crafted_ids as ci
import order_inputs as oi

pytestmark = pytest.mark.gpu

M = oi.M
N = 6144                        # chain_shapes.make_items' batch: a multiple of 64 at every tile size
KEYS = (0, 1)                   # the crafted keys of the chain rows (of cs.NKEYS)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _batches(keys):
    """(name, crafted batch, whole runs of 64?) -- built once per key pair."""
    out = [(order, ci.ladder(order=order, keys=keys), order == "wave-packed") for order in ci.ORDERS]
    return out + [("repeats", ci.repeats(key=keys[1]), True)]


def _union(batches):
    """Every crafted id of the batches as one packed batch (for BF.MADD)."""
    ids = [x for _, (buf, offs, _), _ in batches for x in ci.unpack(buf, offs)]
    return ci.pack(ids)


def _madd_both(engine, chain, buf, offs, want=None):
    """One BF.MADD of the ids into filter 0 and into the oracle's chain: equal replies, all members after."""
    if want is None:
        want = chain.madd_packed(buf, offs)
    n = len(offs) - 1
    got = np.full(n, 7, np.int8)
    engine.ctx.call("ske_bf_madd", 0, _ptr(buf), _ptr(offs), n, _ptr(got), 0)
    assert np.array_equal(got, want), "BF.MADD replies"
    assert chain.mexists_packed(buf, offs)[0].all()
    return want


def _swipes(engine, buf, offs, slots):
    n = len(offs) - 1
    got = np.full(n, 7, np.uint8)
    engine.ctx.call("ske_swipes", 0, _ptr(slots), _ptr(buf), _ptr(offs), n, _ptr(got), 0)
    return got


def _same_regs(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: registers differ at (key, register): got / want " + ", ".join(
        f"({k}, {r}): {got[k, r]} / {want[k, r]}" for k, r in bad[:8]) + f" ({len(bad)} in all)"


def _ends_at_51(name, regs, keys):
    """On the oracle's registers: the batch took every register it aims at to 51."""
    if name == "repeats":
        assert regs[keys[1], 3] == 51
    else:
        aimed = [r for r in ci.REGS if r < 4] if name == "wave-packed" else list(ci.REGS)
        for k in keys:
            assert (regs[k, aimed] == 51).all(), (name, k, regs[k, aimed])


# ---------------------------------------------------------------------------
# k_pfadd: PFADD without a filter
# ---------------------------------------------------------------------------
def test_pfadd_kernel(engine, orc):
    rng = np.random.default_rng(11)
    fbuf, foffs = cs.random_ids(rng, N, short=(np.arange(N) // 64) % 4 == 3)
    fslots = rng.integers(0, cs.NKEYS, N).astype(np.uint32)
    batches = _batches(KEYS)
    engine.hll_reserve(cs.NKEYS * len(batches))
    for j, (name, crafted, runs) in enumerate(batches):
        buf, offs, slots, _ = ci.spread(fbuf, foffs, fslots, crafted, rng, runs)
        regs = np.zeros((cs.NKEYS, M), np.uint8)
        orc.hll_madd(regs, slots, buf, offs)
        _ends_at_51(name, regs, KEYS)
        dev = slots + np.uint32(j * cs.NKEYS)
        engine.ctx.call("ske_hll_pfadd", _ptr(dev), _ptr(buf), _ptr(offs), N, None, 0)
        got = engine.registers_all(cs.NKEYS * len(batches))[j * cs.NKEYS:(j + 1) * cs.NKEYS]
        _same_regs(got, regs, name)
        rbuf, roffs, rslots = ci.reverse(buf, offs, dev)
        engine.ctx.call("ske_hll_pfadd", _ptr(rslots), _ptr(rbuf), _ptr(roffs), N, None, 0)
        got = engine.registers_all(cs.NKEYS * len(batches))[j * cs.NKEYS:(j + 1) * cs.NKEYS]
        _same_regs(got, regs, name + " reversed")


# ---------------------------------------------------------------------------
# the K1 arms of tests/chain_shapes.py
# ---------------------------------------------------------------------------
# (row, the arm of the writer)
ARMS = [("global-e", "k_swipes, 32-bit cursor"), ("global-cursor64", "k_swipes, 64-bit cursor"),
        ("legacy-pieces", "k_swipes<kLds>"), ("lds-f", "k_swipes_lds"),
        ("part-11", "pass C, km 11"), ("part-7-7-8", "pass C, km 22"),
        ("xr-k11", "k_xr_region_b + k_xr_finish"), ("xr-k17", "k_xr_region + k_xr_finish")]
ARM_OF = {"global-e": "global", "global-cursor64": "global", "legacy-pieces": "legacy", "lds-f": "lds P=9",
          "part-11": "part km=11", "part-7-7-8": "part km=22", "xr-k11": "xr KB=11", "xr-k17": "xr KB=0"}


@pytest.mark.parametrize("name", [a for a, _ in ARMS])
def test_k1_arm(engine, orc, name):
    row = cs.ROW[name]
    assert cs.csrc_constants() == {k: getattr(cs, k) for k in cs.csrc_constants()}
    assert cs.csrc_cut_constants() == {"XR_REGIONS": cs.XR_REGIONS, "XR_SLICE_ALIGN": cs.XR_SLICE_ALIGN}
    assert cs.plan(row.specs, row.variant)[1] == row.arm == ARM_OF[name]
    if name == "global-cursor64":
        assert row.specs[0][0] > 1 << 31     # the link's bit positions need the 64-bit cursor
    ch = cs.make_chain(orc, row.specs, row.seed)
    rng = np.random.default_rng(row.seed * 16 + 9)
    filler = cs.make_items(ch, rng, N)
    batches = _batches(KEYS)
    variants = sorted({row.variant, -1}, reverse=True)
    engine.hll_reserve(cs.NKEYS * len(batches) * len(variants) * len(row.tiles))
    cs.load_engine(engine, 0, ch)
    engine.set_option("hll_seg", 0)   # the partitioned rows: pass C writes the registers
    engine.set_option("pass_timing", 1)
    _madd_both(engine, ch.chain, *_union(batches))
    base = 0
    for bname, crafted, runs in batches:
        buf, offs, slots, at = ci.spread(filler.buf, filler.offs, filler.slots, crafted, rng, runs)
        regs = np.zeros((cs.NKEYS, M), np.uint8)
        valid, _, _ = orc.process_swipes(ch.chain, regs, slots, buf, offs)
        assert valid[at].all() and 0.2 <= valid.mean() <= 0.9
        _ends_at_51(bname, regs, KEYS)
        rbuf, roffs, rslots = ci.reverse(buf, offs, slots)
        again = regs.copy()
        rvalid, _, _ = orc.process_swipes(ch.chain, again, rslots, rbuf, roffs)
        assert np.array_equal(again, regs) and np.array_equal(rvalid, valid[::-1])
        for variant in variants:
            for tile in row.tiles:
                what = f"{bname}, variant {variant}, tile {tile}"
                engine.set_option("variant", variant)
                engine.set_option("tile", tile)
                assert engine.variant(0) == cs.plan(row.specs, variant)[0]
                engine.pass_times(reset=True)
                assert np.array_equal(_swipes(engine, buf, offs, slots + np.uint32(base)), valid), what
                pt = engine.pass_times(reset=True)
                if cs.plan(row.specs, variant)[1].startswith("part"):   # pass C wrote, not the segmented form
                    assert pt[3][1] > 0 and pt[4][1] == 0 and pt[5][1] == 0, (what, pt)
                else:
                    assert pt[0][1] > 0 and pt[3][1] == 0, (what, pt)
                got = np.stack([engine.registers(base + s) for s in range(cs.NKEYS)])
                _same_regs(got, regs, what)
                assert np.array_equal(_swipes(engine, rbuf, roffs, rslots + np.uint32(base)), rvalid), what
                got = np.stack([engine.registers(base + s) for s in range(cs.NKEYS)])
                _same_regs(got, regs, what + ", reversed")
                base += cs.NKEYS


# ---------------------------------------------------------------------------
# the segmented form on C3's one-link filter
# ---------------------------------------------------------------------------
SEG_MEMBERS = 100_000   # preloaded; a call's member ids are distinct
SEG_OTHERS = 2_000      # ids never added
SEG_N = 1 << 14         # swipes per call: hll_seg 1 engages the form at any size
SEG_NKEYS = 8
SEG_KEYS = (1, 6)       # one window at seg_klog 3, two below
FLOOR_KEY = 3
FLOORS = (1, 31, 32, 50, 51)

_seg = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_shared():
    yield
    _seg.clear()  # the oracle's chain is freed with the module, not at interpreter exit


def _seg_setup(engine, orc):
    """C3's filter preloaded with the generator's members and, by one BF.MADD on
    both sides, every crafted id of this section; the slab reserved.  The ids on
    the host, the crafted batches and the oracle's chain are shared."""
    from rtsas_amd import synthetic
    w = synthetic.WORKLOADS["c3"]
    w = synthetic.Workload(**{**w.__dict__, "n_members": SEG_MEMBERS + SEG_OTHERS, "n_keys": SEG_NKEYS,
                              "zipf_lectures": 0, "zipf_days": 0})
    engine.reserve(0, w.bf_error, w.bf_capacity)
    p = engine.gen_params(w)
    engine.preload(0, p, SEG_MEMBERS)
    engine.hll_reserve(SEG_NKEYS)
    assert engine.variant(0) == 3
    engine.set_option("hll_seg", 1)
    engine.set_option("pass_timing", 1)
    if not _seg:
        mb = engine.members_batch(p, 0, SEG_MEMBERS + SEG_OTHERS)
        buf, offs, _ = mb.to_host()
        mb.free()
        width = int(offs[1] - offs[0])
        ids = np.ascontiguousarray(buf[:(SEG_MEMBERS + SEG_OTHERS) * width].reshape(-1, width))
        chain = orc.Chain(w.bf_capacity, w.bf_error)
        chain.madd_packed(np.concatenate([ids[:SEG_MEMBERS].reshape(-1), np.zeros(16, np.uint8)]),
                          np.arange(0, width * SEG_MEMBERS + 1, width, dtype=np.uint32))
        batches = _batches(SEG_KEYS)
        edges = {f: ci.floor_edges(f, key=FLOOR_KEY) for f in FLOORS}
        union = _union(batches + [(f, b, False) for f, b in edges.items()])
        _seg.update(ids=ids, width=width, chain=chain, batches=batches, edges=edges, union=union,
                    replies=chain.madd_packed(*union))
    _madd_both(engine, _seg["chain"], *_seg["union"], want=_seg["replies"])
    return _seg


def _seg_filler(st, seed):
    """SEG_N swipes as test_seg_floor._batch builds them: distinct member ids, 1 % replaced by ids
    never added, the keys uniform."""
    rng = np.random.default_rng(seed)
    idx = rng.permutation(SEG_MEMBERS)[:SEG_N]
    bad = rng.random(SEG_N) < 0.01
    idx[bad] = SEG_MEMBERS + rng.integers(0, SEG_OTHERS, int(bad.sum()))
    w = st["width"]
    buf = np.concatenate([st["ids"][idx].reshape(-1), np.zeros(16, np.uint8)])
    return buf, np.arange(0, w * SEG_N + 1, w, dtype=np.uint32), rng.integers(0, SEG_NKEYS, SEG_N).astype(np.uint32)


def _seg_call(engine, orc, st, regs, buf, offs, slots, what):
    """One call through the segmented form (its window pass ran: the pass
    timing says so) and its comparison; ``regs`` (the oracle's) is advanced in
    place.  Returns (the oracle's answers, the floor statistics)."""
    engine.pass_times(reset=True)
    engine.seg_floor_stats()
    got = _swipes(engine, buf, offs, slots)
    pt = engine.pass_times(reset=True)
    stats = engine.seg_floor_stats()
    assert pt[1][1] > 0 and pt[3][1] > 0 and pt[4][1] > 0 and pt[5][1] > 0, (what, pt)
    valid, _, _ = orc.process_swipes(st["chain"], regs, slots, buf, offs)
    assert np.array_equal(got, valid), what
    _same_regs(engine.registers_all(SEG_NKEYS), regs, what)
    return valid, stats


@pytest.mark.parametrize("floor", [0, 1])
@pytest.mark.parametrize("dense_min", [0, 10 ** 6], ids=["staged", "in-place"])
@pytest.mark.parametrize("klog", [0, 1, 2, 3])
def test_segmented(engine, orc, klog, dense_min, floor):
    """seg_dense_min 0: every window with records staged (the LDS maximum);
    10^6: every record raised in place.  seg_hot_min 0 hints every visited
    window, so with seg_floor 1 the reversed call derives floors."""
    st = _seg_setup(engine, orc)
    engine.set_option("seg_klog", klog)
    engine.set_option("seg_dense_min", dense_min)
    engine.set_option("seg_floor", floor)
    engine.set_option("seg_hot_min", 0)
    rng = np.random.default_rng(21)
    for j, (name, crafted, runs) in enumerate(st["batches"]):
        for s in range(SEG_NKEYS):
            engine.ctx.call("ske_hll_clear", s)
        regs = np.zeros((SEG_NKEYS, M), np.uint8)
        buf, offs, slots, at = ci.spread(*_seg_filler(st, 30 + j), crafted, rng, runs)
        valid, stats = _seg_call(engine, orc, st, regs, buf, offs, slots, name)
        assert valid[at].all() and valid.mean() < 0.995
        assert stats[1] > 0 if floor else stats == (0, 0, 0)
        _ends_at_51(name, regs, SEG_KEYS)
        before = regs.copy()
        rvalid, stats = _seg_call(engine, orc, st, regs, *ci.reverse(buf, offs, slots), name + ", reversed")
        assert np.array_equal(before, regs) and np.array_equal(rvalid, valid[::-1])
        if floor:
            assert stats[0] > 0      # hinted windows had their floors derived


@pytest.mark.parametrize("f", FLOORS)
def test_floor_edges(engine, orc, f):
    """One key with every register at f (ske_hll_import_raw) before a call
    that holds records of rank f - 1, f, f + 1 and 51 for 64 of its registers:
    the floor is f, the records at or under it are dropped, the one above it
    raises.  The first call's filler visits every window, and seg_hot_min 0
    hints every visited window, so the second call derives the floor."""
    st = _seg_setup(engine, orc)
    engine.set_option("seg_floor", 1)
    engine.set_option("seg_hot_min", 0)
    regs = np.zeros((SEG_NKEYS, M), np.uint8)
    buf, offs, slots = _seg_filler(st, 40)
    assert set(slots.tolist()) == set(range(SEG_NKEYS))
    _seg_call(engine, orc, st, regs, buf, offs, slots, "first call")
    regs[FLOOR_KEY] = f
    engine.ctx.call("ske_hll_import_raw", FLOOR_KEY, _ptr(np.ascontiguousarray(regs[FLOOR_KEY])))
    before = regs[FLOOR_KEY].copy()
    crafted = st["edges"][f]
    buf, offs, slots, at = ci.spread(*_seg_filler(st, 41), crafted, np.random.default_rng(42))
    valid, (nfl, saw, dropped) = _seg_call(engine, orc, st, regs, buf, offs, slots, f"floor {f}")
    print(f"floor {f}: floored {nfl} saw {saw} dropped {dropped}")
    assert valid[at].all()
    # at least the crafted records at or under the floor, and no more than the call's records
    under = sum(1 for n in range(64) for q in ci.floor_edge_ranks(f, n) if q <= f)
    assert nfl > 0 and under <= dropped <= saw
    # (the oracle alone) the key ends where the batch's name says
    want = before.copy()
    for n, reg in enumerate(ci.FLOOR_REGS):
        want[reg] = max(ci.floor_edge_ranks(f, n) + [f])
    touched = np.zeros(M, bool)
    touched[list(ci.FLOOR_REGS)] = True
    assert np.array_equal(regs[FLOOR_KEY][touched], want[touched])
    assert (regs[FLOOR_KEY] >= f).all()
    if f == 51:
        assert np.array_equal(regs[FLOOR_KEY], before)


# ---------------------------------------------------------------------------
# order-exact replies (sketch_order.hip): the 51-step staircase
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("preset", [0, 25])
@pytest.mark.parametrize("registers", [(2,), (0, 1, 2, 3)], ids=["one", "word"])
@pytest.mark.parametrize("order", oi.ORDERS)
def test_staircase_replies(client, orc, order, registers, preset):
    """Ranks 1 .. 51 in strict order on one register, or on registers 0 .. 3
    interleaved rank by rank, onto an empty key or one preset to 25 in those
    registers: the per-element replies (ske_hll_pfadd with ``changed``, as
    test_pfadd_stairs calls it) and the slab equal oracle.hll_madd."""
    from rtsas_amd.engine import SketchEngine
    buf, offs = ci.staircase(registers, order)
    n = len(offs) - 1
    slots = np.full(n, 1, np.uint32)
    client.ctx.call("ske_hll_reserve", 2)
    cap = client.ctx.lib.ske_hll_capacity(client.ctx.ptr)
    regs = np.zeros((cap, M), np.uint8)
    regs[1, 5], regs[0, 2] = 7, 33              # a neighbour in the next word, the same register of another key
    if len(registers) == 1:
        regs[1, [0, 1, 3]] = 51, 1, 9           # the other bytes of the word
    regs[1, list(registers)] = preset
    for s in (0, 1):
        client.ctx.call("ske_hll_import_raw", s, _ptr(np.ascontiguousarray(regs[s])))
    want = orc.hll_madd(regs, slots, buf, offs)
    ranks = np.asarray([oi.patlen(x)[1] for x in ci.unpack(buf, offs)])
    if order == "ascending":                    # (the oracle alone) every step above the preset raises
        assert np.array_equal(want, ranks > preset)
    elif order == "descending":
        assert int(want.sum()) == len(registers)
    else:
        assert np.array_equal(want, (ranks > preset) & (np.arange(n) % 2 == 0))
    assert (regs[1, list(registers)] == 51).all()
    got = client.pfadd_packed(slots, buf, offs, changed=True)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {n} replies differ, first at {bad[:8].tolist()}"
    _same_regs(SketchEngine(ctx=client.ctx).registers_all(cap), regs, "slab")
