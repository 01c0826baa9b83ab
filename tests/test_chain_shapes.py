"""Every K1 dispatch arm on chains of edge geometry, bit-exact against the oracle.

The chain's geometry alone decides which K1 kernel answers and with which
template instance ("K1 dispatch"):

    image <= 152 KiB, k1_lds_plan accepts     k_swipes_lds<kHll, U, P>, P = ceil(pieces / 16)
    image <= 152 KiB, k1_lds_plan refuses     k_swipes<.., kLds = true, U> (stage_bloom)
    else, under 8 MB or nothing else fits     k_swipes<.., false, U>, 32- or 64-bit cursor per link
    >= 8 MB or variant 3, part_plan accepts   sketch_part.hip, km = 11 or 22
    >= 8 MB or variant 2/3, xr_supported      sketch_xr.hip, k_xr_region_b<2, KB> or the per-step kernel

tests/chain_shapes.py restates that table (``plan``) and holds the rows; its
constants and the arm of every row are asserted in tests/test_chain_shapes_host.py
(no GPU needed) and again here before a row runs.  ske_swipes_variant cannot
tell a template instance, so it is ``plan`` that says a row reaches its
instance, and the device that says the instance computes what RedisBloom
computes: the chains are loaded by BF.LOADCHUNK (any link of bytes >= 1,
1 <= hashes <= 64), a tenth full, half of the items members -- one probe on a
wrong bit and a member turns invalid -- and a tenth near members, all of whose
bits are set but one: an instance that drops a probe calls them valid.

Per row and batch size, under the row's forced variant and under -1, at every
tile size of the row: ske_swipes_variant, BF.MEXISTS answers, swipes answers,
the registers of every key and ske_swipes_stats == (probes, nvalid) equal the
oracle's.  No tolerance anywhere.
"""
import ctypes as C

import numpy as np
import pytest

import chain_shapes as cs

pytestmark = pytest.mark.gpu


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class _Ref:
    """A batch and the oracle's answers to it (computed once, read by every combination)."""

    def __init__(self, orc, ch, items, strict=True):
        self.items = items
        cs.check_inputs(orc, ch, items, strict)
        self.regs = np.zeros((cs.NKEYS, 16384), np.uint8)
        self.valid, self.nvalid, self.probes = orc.process_swipes(ch.chain, self.regs, items.slots, items.buf,
                                                                  items.offs)
        self.valid.setflags(write=False)
        self.regs.setflags(write=False)


def _regs(engine, base):
    return np.stack([engine.registers(base + s) for s in range(cs.NKEYS)])


def _check(engine, ref, variant, tile, expect_variant, base):
    """The chain is filter 0 of ``engine``; keys base .. base + NKEYS - 1 are untouched so far."""
    from rtsas_amd.engine import DeviceBatch
    it = ref.items
    engine.set_option("variant", variant)
    engine.set_option("tile", tile)
    assert engine.variant(0) == expect_variant
    got = np.full(it.n, 7, np.uint8)
    engine.ctx.call("ske_bf_mexists", 0, _ptr(it.buf), _ptr(it.offs), it.n, _ptr(got), 0)
    assert np.array_equal(got, ref.valid), "BF.MEXISTS"
    got = np.full(it.n, 7, np.uint8)
    slots = it.slots + np.uint32(base)
    engine.ctx.call("ske_swipes", 0, _ptr(slots), _ptr(it.buf), _ptr(it.offs), it.n, _ptr(got), 0)
    assert np.array_equal(got, ref.valid), "swipes"
    assert np.array_equal(_regs(engine, base), ref.regs), "registers"
    b = DeviceBatch.from_host(engine.ctx, it.buf, it.offs, slots)
    try:
        assert engine.swipes_stats(0, b) == (ref.probes, ref.nvalid)
    finally:
        b.free()


@pytest.mark.parametrize("row", cs.ROWS, ids=lambda r: r.name)
def test_row(engine, orc, row):
    assert cs.csrc_constants() == {k: getattr(cs, k) for k in cs.csrc_constants()}
    assert cs.plan(row.specs, row.variant)[1] == row.arm
    ch = cs.make_chain(orc, row.specs, row.seed)
    ns = [(_cus() + 1) * 512 + 3 if n == "cu" else n for n in row.ns]
    refs = [_Ref(orc, ch, cs.make_items(ch, np.random.default_rng(row.seed * 16 + j), n), strict=n >= 4000)
            for j, n in enumerate(ns)]
    variants = sorted({row.variant, -1}, reverse=True)
    engine.hll_reserve(cs.NKEYS * len(refs) * len(variants) * len(row.tiles))
    cs.load_engine(engine, 0, ch)
    base = 0
    for ref in refs:
        for variant in variants:
            for tile in row.tiles:
                _check(engine, ref, variant, tile, cs.plan(row.specs, variant)[0], base)
                base += cs.NKEYS


def test_lds_two_stage_pipeline_fixed_width(engine, orc):
    """Row h: lds-f (P = 9) at tile 1 over (2 CUs + 1) 1024 + 17 fixed-width ids: every block runs a
    first, a steady and a last tile of the two-stage pipeline, the last block a ragged one."""
    ch = cs.make_chain(orc, cs.ROW_F, 77, width=8)
    n = (2 * _cus() + 1) * 1024 + 17
    ref = _Ref(orc, ch, cs.make_items(ch, np.random.default_rng(78), n, width=8))
    it = ref.items
    engine.hll_reserve(cs.NKEYS)
    cs.load_engine(engine, 0, ch)
    engine.set_option("tile", 1)
    assert engine.variant(0) == 1 and cs.plan(cs.ROW_F, -1) == (1, "lds P=9")
    got = np.full(n, 7, np.uint8)
    engine.ctx.call("ske_swipes_fixed", 0, _ptr(it.slots), _ptr(it.buf), 8, n, _ptr(got), 0)
    assert np.array_equal(got, ref.valid)
    assert np.array_equal(_regs(engine, 0), ref.regs)


@pytest.mark.parametrize("name", ["lds-e", "lds-f"])
def test_lds_many_batches_persistent(engine, orc, name):
    """Row i: five batches of 1, 1023, 4096, 4097 and 9000 swipes in one persistent launch
    (k_swipes_lds_many) on two blocks, at tile 1 and 4."""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    row = cs.ROW[name]
    ch = cs.make_chain(orc, row.specs, row.seed)
    batches = [cs.make_items(ch, np.random.default_rng(80 + j), n) for j, n in enumerate((1, 1023, 4096, 4097, 9000))]
    want_regs = np.zeros((cs.NKEYS, 16384), np.uint8)
    want = [orc.process_swipes(ch.chain, want_regs, it.slots, it.buf, it.offs)[0] for it in batches]
    tiles = (1, 4)
    engine.hll_reserve(cs.NKEYS * len(tiles))
    cs.load_engine(engine, 0, ch)
    engine.set_option("k1_persistent", 1)
    engine.set_option("k1_grid", 2)
    assert engine.variant(0) == 1 and cs.plan(row.specs, -1)[1] == row.arm
    for t, tile in enumerate(tiles):
        engine.set_option("tile", tile)
        dev = [DeviceBatch.from_host(engine.ctx, it.buf, it.offs, it.slots + np.uint32(t * cs.NKEYS)) for it in batches]
        outs = [DeviceBuffer(engine.ctx, it.n) for it in batches]
        try:
            engine.swipes_many_async(0, dev, outs)
            engine.sync()
            for o, it, w in zip(outs, batches, want):
                assert np.array_equal(o.to_host(np.uint8, it.n), w), (tile, it.n)
            assert np.array_equal(_regs(engine, t * cs.NKEYS), want_regs), tile
        finally:
            for x in dev + outs:
                x.free()


# ---------------------------------------------------------------------------
# BF.MADD into loaded chains of odd geometry (sketch_order.hip, the epochs of ske_bf_madd)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("specs", [[(72, 5)], [(1 << 20, 17), (64, 1)], cs.ROW_E], ids=["72x5", "1Mi-64", "row-e"])
def test_madd_into_loaded_chain(client, orc, specs):
    """400 items -- 40 of them repeats of earlier ones, 40 members already in the chain -- in one call
    into a chain whose last link has room for 3: replies, the links the call grows and every link's
    bits equal the oracle's; the same items again answer all 0."""
    ch = cs.make_chain(orc, specs, 31, last_entries_over=3)
    rng = np.random.default_rng(32)
    fresh, fo = cs.random_ids(rng, 320, short=np.arange(320) % 2 == 0)
    ids = [fresh[fo[i]:fo[i + 1]].tobytes() for i in range(320)]
    ids += [ids[int(i)] for i in rng.integers(0, 320, 40)]
    for j in range(40):
        b, o = ch.members[j % len(specs)]
        m = int(rng.integers(0, len(o) - 1))
        ids.append(b[o[m]:o[m + 1]].tobytes())
    head, tail = ids[:100], ids[100:]
    ids = head + [tail[int(i)] for i in rng.permutation(len(tail))]
    buf, offs = orc.pack(ids)
    want = ch.chain.madd_packed(buf, offs)
    assert (want == 1).sum() > 200 and (want == 0).sum() >= 40 and ch.chain.nlinks > len(specs)
    cs.load_client(client, "k", ch)
    got = client.bf_madd_packed("k", buf, offs)
    assert np.array_equal(got, want)
    links = client.bf_links("k")
    assert len(links) == ch.chain.nlinks
    for l, L in enumerate(links):
        info = ch.chain.link_info(l)
        assert {k: L[k] for k in ("entries", "bytes", "bits", "hashes", "size")} == \
               {k: info[k] for k in ("entries", "bytes", "bits", "hashes", "size")}, l
        assert np.array_equal(client.bf_link_bits("k", l), ch.chain.link_bits(l)), l
    assert not client.bf_madd_packed("k", buf, offs).any()
    assert not ch.chain.madd_packed(buf, offs).any()


# ---------------------------------------------------------------------------
# BF.LOADCHUNK and the header's n2
# ---------------------------------------------------------------------------
def test_loadchunk_n2_power_of_two(client, orc):
    """One link of 8 KiB with n2 = 16 in its header: RedisBloom probes mod 2^16, which is mod bits
    (the power-of-two divisor, magic m = 1); answers == the oracle's.  A header whose n2 is not
    log2(bits) is refused and leaves no key."""
    from rtsas_amd.exceptions import ResponseError
    ch = cs.make_chain(orc, [(1 << 16, 7)], 41, n2=16)
    it = cs.make_items(ch, np.random.default_rng(42), 6144)
    want = cs.check_inputs(orc, ch, it)
    cs.load_client(client, "k", ch)
    assert np.array_equal(client.bf_mexists_packed("k", it.buf, it.offs), want)
    keys = np.asarray([client.key_slot(f"hll:{s}") for s in range(cs.NKEYS)], np.uint32)
    assert np.array_equal(client.swipes_slots("k", keys[it.slots], it.buf, it.offs), want.astype(bool))
    bad = cs.pack_header([cs.link_record(1 << 16, 7, n2=15)])
    with pytest.raises(ResponseError, match="ERR received bad data"):
        client.execute_command("BF.LOADCHUNK", "k2", 1, bad)
    assert client.exists("k2") == 0
