"""The preconditions of tests/crafted_ids.py, on the CPU: every id has the hash
it was built for (the oracle's MurmurHash64A and hllPatLen say so), and every
batch the shape its name promises."""
import numpy as np
import pytest

import chain_shapes as cs
import crafted_ids as ci
import order_inputs as oi


@pytest.mark.parametrize("seed", [ci.HLL_SEED, ci.BLOOM_SEED, None], ids=["hll", "bloom", "random"])
def test_round_trip(orc, seed):
    """Lengths 8 .. 40, 12 targets each, 0 and 2^64 - 1 among them."""
    rng = np.random.default_rng(1)
    for length in range(8, 41):
        for j in range(12):
            want = (0, ci.M64)[j] if j < 2 else int.from_bytes(rng.bytes(8), "little")
            s = int.from_bytes(rng.bytes(8), "little") if seed is None else seed
            x = ci.invert(want, s, length, rng)
            assert len(x) == length and orc.murmur64a(x, s) == want


def test_free_bytes_are_free(orc):
    """Two ids of one target differ (the leading blocks and the tail come from the generator)."""
    rng = np.random.default_rng(2)
    for length in (9, 16, 17, 40):
        a, b = ci.invert(12345, ci.HLL_SEED, length, rng), ci.invert(12345, ci.HLL_SEED, length, rng)
        assert a != b and orc.murmur64a(a, ci.HLL_SEED) == orc.murmur64a(b, ci.HLL_SEED) == 12345
    # eight bytes hold exactly one
    assert ci.invert(12345, ci.HLL_SEED, 8, rng) == ci.invert(12345, ci.HLL_SEED, 8, rng)


@pytest.mark.parametrize("length", range(8))
def test_invert_refuses_short_ids(length):
    with pytest.raises(ValueError):
        ci.invert(1, ci.HLL_SEED, length, np.random.default_rng(0))


@pytest.mark.parametrize("length", ci.LENGTHS)
def test_every_register_and_rank(length):
    rng = np.random.default_rng(3)
    for reg in ci.REGS:
        for rank in range(1, ci.MAX_RANK + 1):
            assert oi.patlen(ci.hll_id(reg, rank, length, rng)) == (reg, rank)


def _items(batch):
    buf, offs, slots = batch
    return [(int(s),) + oi.patlen(x) + (x,) for s, x in zip(slots, ci.unpack(buf, offs))]


@pytest.mark.parametrize("order", ci.ORDERS)
def test_ladder(order):
    items = _items(ci.ladder(order=order))
    regs = [r for r in ci.REGS if r < 4] if order == "wave-packed" else ci.REGS
    assert {x[:3] for x in items} == {(k, r, q) for k in (0, 1) for r in regs for q in range(1, 52)}
    assert {len(x[3]) for x in items} == set(ci.LENGTHS)
    ranks = [x[2] for x in items]
    if order == "ascending":
        assert ranks == sorted(ranks) and len(items) == 2 * 8 * 51
    elif order == "descending":
        assert ranks == sorted(ranks, reverse=True)
    elif order == "shuffled":
        assert ranks != sorted(ranks) and ranks != sorted(ranks, reverse=True)
        assert sorted(x[3] for x in items) == sorted(x[3] for x in _items(ci.ladder(order="ascending")))
    else:
        assert len(items) % 64 == 0
        short_runs = 0
        for r0 in range(0, len(items), 64):
            run = items[r0:r0 + 64]
            assert len({x[0] for x in run}) == 1 and {x[1] for x in run} == {0, 1, 2, 3}
            assert len({x[2] for x in run}) >= 16
            short_runs += all(len(x[3]) == 8 for x in run)
        assert 0 < short_runs < len(items) // 64
        assert {x[0] for x in items} == {0, 1}


def test_repeats():
    items = _items(ci.repeats(key=1))
    assert len(items) == 64 and len(set(items)) == 1 and items[0][:3] == (1, 3, 51)


@pytest.mark.parametrize("f", [1, 31, 32, 50, 51])
def test_floor_edges(f):
    items = _items(ci.floor_edges(f, key=2))
    assert {x[0] for x in items} == {2} and {x[1] for x in items} == set(ci.FLOOR_REGS) and len(ci.FLOOR_REGS) == 64
    assert len({x[3] for x in items}) == len(items)
    assert {x[2] for x in items} == {q for q in (f - 1, f, f + 1, 51) if 1 <= q <= 51}
    by_reg = {}
    for _, reg, rank, _ in items:
        by_reg.setdefault(reg, []).append(rank)
    # what the key ends at from a floor of f: f + 1 alone on some registers, 51 on others, both on a third kind
    ends = {max([f] + r) for r in by_reg.values()}
    assert ends == ({51} if f >= 50 else {f + 1, 51})
    # 32 registers end one above the floor through a record of rank f + 1 alone
    assert sum(max(r) == f + 1 and r.count(f + 1) == 1 for r in by_reg.values()) == {50: 64, 51: 0}.get(f, 32)


@pytest.mark.parametrize("order", oi.ORDERS)
@pytest.mark.parametrize("registers", [(2,), (0, 1, 2, 3)])
def test_staircase(order, registers):
    buf, offs = ci.staircase(registers, order)
    got = [oi.patlen(x) for x in ci.unpack(buf, offs)]
    steps = [(r, q) for q in range(1, 52) for r in registers]
    want = {"ascending": steps, "descending": steps[::-1],
            "ascending-repeated": [s for s in steps for _ in range(2)]}[order]
    assert got == want


def test_spread_and_reverse():
    rng = np.random.default_rng(4)
    fb, fo = cs.random_ids(rng, 1280, short=np.arange(1280) % 2 == 0)
    fs = rng.integers(0, 5, 1280).astype(np.uint32)
    for order, runs in (("shuffled", False), ("wave-packed", True)):
        crafted = ci.ladder(order=order)
        buf, offs, slots, at = ci.spread(fb, fo, fs, crafted, rng, runs=runs)
        got, filler, want = ci.unpack(buf, offs), ci.unpack(fb, fo), ci.unpack(*crafted[:2])
        assert len(got) == 1280 and [got[p] for p in at] == want and slots[at].tolist() == crafted[2].tolist()
        rest = np.setdiff1d(np.arange(1280), at)
        assert [got[p] for p in rest] == [filler[p] for p in rest] and np.array_equal(slots[rest], fs[rest])
        if runs:
            assert (at.reshape(-1, 64)[:, 0] % 64 == 0).all() and (np.diff(at.reshape(-1, 64), axis=1) == 1).all()
        rb, ro, rs = ci.reverse(buf, offs, slots)
        assert ci.unpack(rb, ro) == got[::-1] and rs.tolist() == slots[::-1].tolist()


def test_cut_restatements():
    assert cs.csrc_constants() == {k: getattr(cs, k) for k in cs.csrc_constants()}
    assert cs.csrc_cut_constants() == {"XR_REGIONS": cs.XR_REGIONS, "XR_SLICE_ALIGN": cs.XR_SLICE_ALIGN}
    assert cs.xr_cuts(1 << 19) == tuple(65536 * r for r in range(1, 8))
    assert cs.xr_cuts(8) == () and cs.xr_cuts(1024) == () and cs.xr_cuts(1032) == (1024,)
    # 8256 bits: ceil / 8 = 1032 -> 2048 a region; regions 5 .. 7 are empty
    assert cs.xr_cuts(8256) == (2048, 4096, 6144, 8192)
    assert ci.lds_cuts(8192) == () and ci.lds_cuts(8200) == (8192,)
    assert ci.part_cuts(1 << 19) == () and ci.part_cuts((1 << 19) + 64) == (1 << 19,)


@pytest.mark.parametrize("row,cuts", ci.PROBE_ROWS, ids=[r.name for r, _ in ci.PROBE_ROWS])
def test_probe_targets(orc, row, cuts):
    """The row is the arm its name says, a chain of one link; the first probe
    of the ids lands on 0, 1, bits - 1 and both sides of every cut, from the
    oracle's hash; the raw edge values of ``a`` are there."""
    assert cs.plan(row.specs, row.variant)[1] == row.arm and len(row.specs) == 1
    bits = row.specs[0][0]
    c = cuts(bits)
    if row.arm.startswith("lds"):
        assert len(c) + 1 == cs.lds_pieces(row.specs)
    elif row.arm.startswith("part"):
        assert len(c) + 1 == cs.part_slices(row.specs)[1]
    elif row.arm.startswith("xr"):
        assert len(c) == cs.XR_REGIONS - 1
    assert row.arm == "global" or c
    buf, offs, a_of = ci.probe_targets(bits, c)
    ids = ci.unpack(buf, offs)
    assert len(set(ids)) == len(ids) == len(a_of)
    got = [orc.murmur64a(x, ci.BLOOM_SEED) for x in ids]
    assert got == a_of
    first = {a % bits for a in got}
    assert first >= {0, 1, bits - 1} | {x for cut in c for x in (cut - 1, cut)}
    q = (1 << 64) // bits
    assert set(got) >= {0, bits - 1, bits, 2 ** 32 - 1, 2 ** 32, 2 ** 63, q * bits - 1, 2 ** 64 - 2, 2 ** 64 - 1}
    assert q * bits > ci.M64 or q * bits in got
    by_a = {}
    for a, x in zip(got, ids):
        by_a.setdefault(a, []).append(len(x))
    assert all(v == list(ci.PROBE_LENGTHS) for v in by_a.values())
    # every position comes with t = 0, the largest t and one between
    for x in (0, bits - 1) + tuple(c):
        ts = sorted(a // bits for a in by_a if a % bits == x)
        assert ts[0] == 0 and ts[-1] == (ci.M64 - x) // bits and len(ts) >= 3
