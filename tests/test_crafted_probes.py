"""The first Bloom probe on every cut of the bit space.

Where a probe lands relative to a cut decides which 1 KiB LDS piece
(k1_lds_plan), which slice unit of 2^19 bits (part_plan) or which of the
eight regions (sketch_xr.hip: ``lo = region * slice``, ``(x - lo) < len``)
tests it; a boundary off by one bit leaves a probe untested, and an untested
probe turns a non-member valid.  tests/crafted_ids.py builds ids whose first
probe ``a mod bits`` is 0, 1, bits - 1, and c - 1 and c for every cut c of the
row -- each as several ``a = x + bits * t`` up to the largest below 2^64 --
and ids whose ``a`` sits on the edges of fastmod and of 32- and 64-bit
arithmetic.  ``b`` cannot be chosen, so the later probes land where they land.

Per row (one chain of one link per arm that cuts the bit space, and a plain
k_swipes one), inside chain_shapes.make_items' filler, two images:

- "members": the crafted ids added by one BF.MADD on both sides (equal
  replies); every one of them answers 1;
- "first bit cleared": the bit of every crafted id's first probe cleared, in
  the oracle's bits and through ske_bf_link_write on the device; every one of
  them answers 0 -- unless its first probe goes untested.

On both, test_chain_shapes._check under the forced variant and under -1 at
every tile of the row: BF.MEXISTS, swipes, the registers and ske_swipes_stats
equal the oracle's on the same image (the filler's members that the clearing
broke with them).  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import chain_shapes as cs
import crafted_ids as ci
from test_chain_shapes import _check, _ptr

pytestmark = pytest.mark.gpu

N = 6144


class _Ref:
    """A batch and the oracle's answers to it on the chain as it stands."""

    def __init__(self, orc, ch, items):
        self.items = items
        self.regs = np.zeros((cs.NKEYS, 16384), np.uint8)
        self.valid, self.nvalid, self.probes = orc.process_swipes(ch.chain, self.regs, items.slots, items.buf,
                                                                  items.offs)
        self.valid.setflags(write=False)
        self.regs.setflags(write=False)


@pytest.mark.parametrize("row,cuts", ci.PROBE_ROWS, ids=[r.name for r, _ in ci.PROBE_ROWS])
def test_first_probe_on_every_cut(engine, orc, row, cuts):
    assert cs.csrc_constants() == {k: getattr(cs, k) for k in cs.csrc_constants()}
    assert cs.csrc_cut_constants() == {"XR_REGIONS": cs.XR_REGIONS, "XR_SLICE_ALIGN": cs.XR_SLICE_ALIGN}
    assert cs.plan(row.specs, row.variant)[1] == row.arm and len(row.specs) == 1
    bits = row.specs[0][0]
    ch = cs.make_chain(orc, row.specs, row.seed)
    assert not ch.sparse
    rng = np.random.default_rng(row.seed * 16 + 5)
    filler = cs.make_items(ch, rng, N)
    cbuf, coffs, a_of = ci.probe_targets(bits, cuts(bits))
    m = len(a_of)
    crafted = (cbuf, coffs, rng.integers(0, cs.NKEYS, m).astype(np.uint32))
    buf, offs, slots, at = ci.spread(filler.buf, filler.offs, filler.slots, crafted, rng)
    link = filler.link.copy()
    link[at] = 0
    items = cs.Items(buf, offs, slots, link)
    variants = sorted({row.variant, -1}, reverse=True)
    engine.hll_reserve(cs.NKEYS * 2 * len(variants) * len(row.tiles))
    cs.load_engine(engine, 0, ch)
    base = 0

    def check(ref):
        nonlocal base
        for variant in variants:
            for tile in row.tiles:
                _check(engine, ref, variant, tile, cs.plan(row.specs, variant)[0], base)
                base += cs.NKEYS

    # image "members"
    want = ch.chain.madd_packed(cbuf, coffs)
    got = np.full(m, 7, np.int8)
    engine.ctx.call("ske_bf_madd", 0, _ptr(cbuf), _ptr(coffs), m, _ptr(got), 0)
    assert np.array_equal(got, want), "BF.MADD replies"
    assert want[::len(ci.PROBE_LENGTHS)].sum() > m // 8     # (most targets' first id was new to the link)
    ref = _Ref(orc, ch, items)
    assert ref.valid[at].all()
    check(ref)

    # image "first bit cleared"
    nbytes = bits // 8
    bf = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(orc.lib().orc_chain_link_bits(ch.chain.p, 0)))
    for x in sorted({a % bits for a in a_of}):
        bf[x >> 3] &= 0xff ^ (1 << (x & 7))
        w0 = (x >> 6) * 8
        word = bf[w0:min(w0 + 8, nbytes)].copy()
        engine.ctx.call("ske_bf_link_write", 0, 0, w0, word.tobytes(), word.size)
    assert not ch.chain.mexists_packed(cbuf, coffs)[0].any()
    ref = _Ref(orc, ch, items)
    assert not ref.valid[at].any()
    members = filler.link >= 0
    members[at] = False
    assert ref.valid[members].mean() > 0.5                  # (the image still holds most of the filler's members)
    check(ref)
