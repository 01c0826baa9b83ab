"""The preconditions of tests/order_inputs.py, on the oracle alone (CPU).

tests/test_order_replies.py compares the device's per-element PFADD and
BF.MADD replies with the oracle's.  A wrong kernel shows there only if the
batches really hold what their builders promise: long same-register segments,
false positives made inside the batch, replies of both kinds past the first
trip of the K4 grids.  Those promises are asserted here, where no GPU is
needed."""
import numpy as np
import pytest

import order_inputs as oi


@pytest.fixture(scope="module")
def pool():
    return oi.same_register_pool()


def _replies(orc, preset, reg, buf, offs):
    regs = np.zeros((1, oi.M), np.uint8)
    regs[0, reg] = preset
    return orc.hll_madd(regs, np.zeros(len(offs) - 1, np.uint32), buf, offs), regs


def test_pool_shares_a_word(pool):
    """113 or more elements in every target register; 0, 1 and 3 are bytes of one 32-bit word."""
    assert set(pool) == set(oi.TARGETS)
    assert len({r // 4 for r in oi.WORD}) == 1 and set(oi.WORD) <= set(pool)
    for reg, (ids, ranks) in pool.items():
        assert ids.size >= 100 and np.unique(ids).size == ids.size, reg


@pytest.mark.parametrize("reg", oi.WORD)
@pytest.mark.parametrize("preset", [0, 1, 3, 51])
def test_stairs_ascending_one_reply_per_new_rank(orc, pool, reg, preset):
    """Ascending (repeated or not): as many 1-replies as distinct ranks above the preset register."""
    for order in ("ascending", "ascending-repeated"):
        buf, offs, ranks = oi.stairs(pool, reg, order)
        got, regs = _replies(orc, preset, reg, buf, offs)
        above = np.unique(ranks[ranks > preset])
        assert int(got.sum()) == above.size, order
        assert regs[0, reg] == max(preset, int(ranks.max()))
        assert np.count_nonzero(regs) == 1
    assert preset == 51 or above.size >= 3


@pytest.mark.parametrize("reg", oi.WORD)
def test_stairs_descending_one_reply(orc, pool, reg):
    buf, offs, ranks = oi.stairs(pool, reg, "descending")
    got, _ = _replies(orc, 0, reg, buf, offs)
    assert got[0] == 1 and int(got.sum()) == 1
    got, _ = _replies(orc, int(ranks.max()), reg, buf, offs)
    assert int(got.sum()) == 0


def test_long_segment_lengths(orc, pool):
    """Every (slot, register) segment holds more than 1000 elements, one more
    than 8192; the oracle puts every element in the register its segment names."""
    buf, offs, slot, reg, rank = oi.long_segment(pool, seed=3)
    n = len(offs) - 1
    assert n == 20_000
    key, count = np.unique(slot.astype(np.int64) * oi.M + reg, return_counts=True)
    assert key.size == 2 * len(oi.TARGETS)
    assert count.min() > 1000 and count.max() > 8192
    regs = np.zeros((2, oi.M), np.uint8)
    got = orc.hll_madd(regs, slot, buf, offs)
    assert set(np.flatnonzero(regs.reshape(-1)).tolist()) == set(key.tolist())
    for k in key:
        assert regs.reshape(-1)[k] == rank[slot.astype(np.int64) * oi.M + reg == k].max()
    # the slots are interleaved: neither comes as one run
    assert np.count_nonzero(np.diff(slot.astype(np.int64))) > n // 4
    assert 0 < int(got.sum()) < 200


def test_mixed_lengths_repeats_reply_zero(orc):
    buf, offs, repeat = oi.mixed_lengths(seed=5)
    regs = np.zeros((1, oi.M), np.uint8)
    got = orc.hll_madd(regs, np.zeros(len(offs) - 1, np.uint32), buf, offs)
    assert not got[repeat].any() and got[~repeat].mean() > 0.5


@pytest.fixture(scope="module")
def tiny(orc):
    out = []
    for row in oi.tiny_chain_rows():
        ch = oi.tiny_chain(row)
        out.append((row, ch, ch.madd_packed(row["buf"], row["offs"])))
    return out


def test_tiny_rows_fit_the_chain(tiny):
    assert len(tiny) == 8
    for row, ch, _ in tiny:
        assert 1 <= ch.nlinks <= oi.MAX_LINKS, (row["name"], ch.nlinks)
        assert len(row["ids"]) == oi.TINY_DRAWS and row["ids"].max() < oi.TINY_IDS
    # the scaling rows grow: the call crosses a filled link 2 .. 45 times
    assert [ch.nlinks > 1 for row, ch, _ in tiny] == [not row["nonscaling"] for row, _, _ in tiny]


def test_tiny_rows_false_positives_inside_the_batch(tiny):
    """A first occurrence that replies 0 is present only through bits that
    earlier items of the same call set: at least four rows hold one."""
    rows_with = 0
    for row, _, rep in tiny:
        rows_with += bool(((rep == 0) & oi.first_occurrence(row["ids"])).any())
    assert rows_with >= 4, rows_with


def test_tiny_rows_nonscaling_full(tiny):
    """Both NONSCALING rows reply -2 (full), and 0 for present items after the first -2."""
    non = [(row, rep) for row, _, rep in tiny if row["nonscaling"]]
    assert len(non) == 2
    for row, rep in non:
        full = np.flatnonzero(rep == -2)
        assert full.size > 0, row["name"]
        assert (rep[full[0]:] == 0).any(), row["name"]
        assert not (rep[full[0]:] == 1).any()
    for row, _, rep in tiny:
        assert row["nonscaling"] or not (rep == -2).any()


def test_tiny_rows_duplicates_straddle_a_fill(tiny):
    """In every scaling row some id comes both before and after an item that fills a link."""
    for row, ch, rep in tiny:
        if row["nonscaling"]:
            continue
        ones = np.flatnonzero(rep == 1)
        fills = ones[np.cumsum([ch.link_info(l)["entries"] for l in range(ch.nlinks - 1)]) - 1]
        ids = row["ids"]
        assert any(np.intersect1d(ids[:f], ids[f + 1:]).size for f in fills), row["name"]


def test_past_the_grid_256(orc):
    """At 256 CUs: replies past the first trip of a 16 * CU grid hold both
    values, for BF.MADD and for PFADD; the chain grows in the call; the last
    link's first-setter table (4 bytes a bit) stays under 64 MiB."""
    buf, offs, ids, slot = oi.past_the_grid(256)
    n = len(ids)
    trip = oi.grid_items(256)
    assert n == trip + 333 == 1_048_909 and n > 4 * (4 * 256 * oi.BLOCK)
    err, cap, _, exp = oi.past_the_grid_reserve(n)
    ch = orc.Chain(cap, err, exp)
    rep = ch.madd_packed(buf, offs)
    assert set(rep[trip:].tolist()) == {0, 1}
    assert ch.nlinks >= 2
    assert max(ch.link_info(l)["bits"] for l in range(ch.nlinks)) * 4 < 64 << 20
    regs = oi.geometric_presets(3, 9)
    changed = orc.hll_madd(regs, slot, buf, offs)
    assert set(changed[trip:].tolist()) == {0, 1}
