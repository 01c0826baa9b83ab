"""Per-element PFADD and BF.MADD replies where the order of the batch decides.

csrc/sketch_order.hip rebuilds Redis's sequential replies from order-free
primitives: PFADD's ``changed[i]`` from a radix sort by (slot, register) and a
segmented running maximum (rocprim's scan-by-key with MaxU8); BF.MADD's reply
from a first-setter table per bit, a prefix count of the absent items and one
epoch per link the call fills (ske_bf_madd, csrc/sketch_api_bloom.cpp).  Every
comparison here is bit-exact against the oracle's sequential loops
(``oracle.hll_madd``, ``oracle.Chain.madd_packed``) on batches built by
tests/order_inputs.py, whose preconditions tests/test_order_inputs_host.py
asserts on the CPU:

- hundreds to thousands of elements of one register (a running maximum carried
  along a segment and across rocprim's tiles), registers 0, 1 and 3 of one
  32-bit word preset and raised together (k_hll_apply's byte-lane CAS);
- slabs of 16, 17, 24 and 33 slots with the highest slot in use (the sort's end_bit);
- chains that fill after 1 .. 8 items, 200 items drawn from 60 ids: false
  positives made inside the call, duplicates on both sides of the item that
  fills a link, NONSCALING filters that answer -2 and then 0;
- 16 * CU * 256 + 333 items: the second trip of every K4 grid-stride loop;
- PFADD and BF.MADD alternating on one context (they share a scratch slot).
"""
import ctypes as C

import numpy as np
import pytest

import order_inputs as oi

pytestmark = pytest.mark.gpu

M = oi.M


def _cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def pool():
    return oi.same_register_pool()


# ---------------------------------------------------------------------------
# PFADD
# ---------------------------------------------------------------------------
def _slab(ctx, nslots, presets):
    """Reserve (``nslots`` a tuple: one ske_hll_reserve after the other),
    import the preset rows; the whole slab as the oracle's copy."""
    for want in (nslots if isinstance(nslots, tuple) else (nslots,)):
        ctx.call("ske_hll_reserve", want)
    cap = ctx.lib.ske_hll_capacity(ctx.ptr)
    assert cap >= want
    regs = np.zeros((cap, M), np.uint8)
    for s, row in presets.items():
        regs[s] = row
        ctx.call("ske_hll_import_raw", s, _ptr(np.ascontiguousarray(regs[s])))
    return regs


def _check_slab(ctx, orc, want_regs, what):
    """Every slot of the slab (untouched ones too) and its PFCOUNT == the oracle's."""
    from rtsas_amd.engine import SketchEngine
    eng = SketchEngine(ctx=ctx)
    got = eng.registers_all(len(want_regs))
    bad = np.argwhere(got != want_regs)
    assert bad.size == 0, (f"{what}: {len(bad)} wrong registers, first (slot, register) {bad[:6].tolist()}: got "
                           f"{[int(got[s, r]) for s, r in bad[:6]]}, want {[int(want_regs[s, r]) for s, r in bad[:6]]}")
    counts = eng.pfcount_each(np.arange(len(want_regs)))
    assert counts.tolist() == [orc.hll_count_regs(r) for r in want_regs], what


def _pfadd_case(pkg, client, orc, nslots, presets, calls, what=""):
    """``calls`` = [(slots, buf, offs)], one ske_hll_pfadd each, in order, on a
    slab of ``nslots`` with ``presets`` = {slot: registers}: every call's
    ``changed`` == the oracle's on the same registers, then the slab.  Then the
    same calls without replies (launch_pfadd) on a second client: the same slab."""
    want_regs = _slab(client.ctx, nslots, presets)
    for c, (slots, buf, offs) in enumerate(calls):
        want = orc.hll_madd(want_regs, slots, buf, offs)
        got = client.pfadd_packed(slots, buf, offs, changed=True)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (f"{what} call {c}: {bad.size} of {got.size} replies differ, first at {bad[:8].tolist()}: "
                               f"got {got[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")
    _check_slab(client.ctx, orc, want_regs, what)
    plain = pkg.SketchClient(device=0)
    _slab(plain.ctx, nslots, presets)
    for slots, buf, offs in calls:
        assert plain.pfadd_packed(slots, buf, offs) is None
    _check_slab(plain.ctx, orc, want_regs, what + " (no replies)")
    return want_regs


PRESETS = ("zero", "below", "equal", "max", "51")
NEIGHBOURS = {2: 33, 5: 7}  # registers no batch touches: one in the word of 0, 1 and 3, one in the next


def _preset_row(kind, ranks_of):
    """The registers of one slot before the batch.  ``ranks_of``: {register:
    the ranks the batch holds for it}.  ``zero``: nothing set.  Otherwise every
    register of the batch holds min rank - 1 (``below``), a rank of the batch
    between its extremes (``equal``), the maximum (``max``) or 51, and the
    untouched NEIGHBOURS hold values of their own."""
    row = np.zeros(M, np.uint8)
    if kind == "zero":
        return row
    for reg, ranks in ranks_of.items():
        u = np.unique(ranks)
        row[reg] = {"below": u[0] - 1, "equal": u[len(u) // 2], "max": u[-1], "51": 51}[kind]
    for reg, v in NEIGHBOURS.items():
        assert reg not in ranks_of
        row[reg] = v
    return row


@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("order", oi.ORDERS)
def test_pfadd_stairs(pkg, client, orc, pool, order, preset):
    """All 113 .. 133 pool elements of one register in rank order, for each of
    registers 0, 1 and 3 in turn; the other two and register 2 of the same word
    hold presets that must survive the byte-lane CAS."""
    for reg in oi.WORD:
        buf, offs, ranks = oi.stairs(pool, reg, order)
        ranks_of = {r: pool[r][1] for r in oi.WORD}  # the neighbours are preset relative to their own pool ranks
        row = _preset_row(preset, ranks_of)
        slots = np.full(len(ranks), 1, np.uint32)
        _pfadd_case(pkg, client, orc, 2, {1: row, 0: row[::-1].copy()}, [(slots, buf, offs)], f"register {reg}")


@pytest.mark.parametrize("preset", PRESETS)
def test_pfadd_long_segment(pkg, client, orc, pool, preset):
    """20 000 elements over 2 slots x 6 registers, one segment of 8 400: the
    running maximum crosses rocprim's tiles; registers 0, 1 and 3 of both slots
    are raised by concurrent CAS on one word."""
    buf, offs, slot, reg, rank = oi.long_segment(pool, seed=3)
    used = np.asarray([2, 0], np.uint32)
    presets = {int(used[s]): _preset_row(preset, {r: rank[(slot == s) & (reg == r)] for r in oi.TARGETS})
               for s in range(2)}
    _pfadd_case(pkg, client, orc, 3, presets, [(used[slot], buf, offs)])


def test_pfadd_two_calls(pkg, client, orc, pool):
    """The second call's replies depend on the registers the first call left."""
    buf, offs, slot, reg, rank = oi.long_segment(pool, seed=4)
    cut = 7001
    calls = [(slot[:cut],) + oi.take(buf, offs, 0, cut), (slot[cut:],) + oi.take(buf, offs, cut, len(slot))]
    row = _preset_row("equal", {r: rank[reg == r] for r in oi.TARGETS})
    _pfadd_case(pkg, client, orc, 2, {0: row, 1: row}, calls)


@pytest.mark.parametrize("equal_preset", [False, True])
def test_pfadd_one_element_10000_times(pkg, client, orc, pool, equal_preset):
    """One element repeated 10 000 times: exactly one 1, the first; none when the register already holds its rank."""
    ids, ranks = pool[1]
    buf, offs = oi.pack8(np.full(10_000, ids[-1]))
    slots = np.zeros(10_000, np.uint32)
    row = np.zeros(M, np.uint8)
    row[1] = ranks[-1] if equal_preset else 0
    row[0], row[2], row[3] = 51, 1, 9
    _pfadd_case(pkg, client, orc, 1, {0: row}, [(slots, buf, offs)])
    # (the reference alone) the oracle's replies are what the name says
    regs = row[None].copy()
    want = orc.hll_madd(regs, slots, buf, offs)
    assert want.sum() == (0 if equal_preset else 1) and want[0] == (not equal_preset)


# (slots reserved, slots used).  ske_hll_reserve never makes a slab of fewer than 16 slots, so the
# first four run on 16 (end_bit 18, slot 8 not the highest); 17, 33 and 16 -> 24 are slabs that
# are no power of two, the highest slot -- the sort's highest key -- in use.
SLABS = [(1, (0,)), (4, (0, 3)), (5, (1, 4)), (9, (0, 8)), (16, (0, 15)), (17, (0, 16)), (33, (7, 32)),
         ((16, 17), (5, 23))]


@pytest.mark.parametrize("reserve,used", SLABS, ids=[f"{r}-{'-'.join(map(str, u))}" for r, u in SLABS])
def test_pfadd_mixed_lengths(pkg, client, orc, reserve, used):
    """4 000 strings of 0 .. 40 bytes, a third of them repeats, over the used
    slots of slabs whose size is, or is not, a power of two."""
    buf, offs, _ = oi.mixed_lengths(seed=5)
    n = len(offs) - 1
    slots = np.asarray(used, np.uint32)[np.random.default_rng(6).integers(0, len(used), n)]
    presets = {s: oi.geometric_presets(1, 10 + s, density=0.3)[0] for s in used}
    regs = _pfadd_case(pkg, client, orc, reserve, presets, [(slots, buf, offs)])
    assert len(regs) == {1: 16, 4: 16, 5: 16, 9: 16, 16: 16, 17: 17, 33: 33}.get(reserve, 24)


_PAST = {}


def _past(orc, cus):
    """past_the_grid's oracle answers, computed once: (HLL presets, registers
    after, changed; the chain, its replies)."""
    if cus not in _PAST:
        buf, offs, ids, slot = oi.past_the_grid(cus)
        presets = oi.geometric_presets(3, 9)
        ch = orc.Chain(*_chain_args(oi.past_the_grid_reserve(len(ids))))
        _PAST[cus] = (presets, ch, ch.madd_packed(buf, offs))
    return _PAST[cus]


def _chain_args(reserve):
    err, cap = reserve[:2]
    return cap, err, (reserve[3] if len(reserve) > 3 else 2), oi.NONSCALING in reserve


def test_pfadd_past_the_grid(pkg, client, orc):
    """16 * CU * 256 + 333 elements over 3 preset slots: the tail of every
    PFADD kernel's grid-stride loop (k_hll_prep, k_gather_u8, k_hll_changed, k_hll_apply)."""
    cus = _cu()
    buf, offs, ids, slot = oi.past_the_grid(cus)
    assert len(ids) > oi.grid_items(cus)
    presets = _past(orc, cus)[0]
    _pfadd_case(pkg, client, orc, 3, {s: presets[s] for s in range(3)}, [(slot, buf, offs)])


# ---------------------------------------------------------------------------
# BF.MADD
# ---------------------------------------------------------------------------
FIELDS = ("entries", "bytes", "bits", "hashes", "size")
PROBE = None


def _probe(orc):
    global PROBE
    if PROBE is None:
        PROBE = orc.pack([str(i).encode() for i in range(100)])
    return PROBE


def _check_chain(client, orc, key, ch, what, probe=True):
    """Links, bits, the item count and BF.MEXISTS of ids 0 .. 99 == the oracle chain's."""
    links = client.bf_links(key)
    assert len(links) == ch.nlinks, (what, len(links), ch.nlinks)
    for l, L in enumerate(links):
        info = ch.link_info(l)
        assert {k: L[k] for k in FIELDS} == {k: info[k] for k in FIELDS}, (what, l)
        assert np.array_equal(client.bf_link_bits(key, l), ch.link_bits(l)), (what, "bits of link", l)
    assert client.bf_info(key)["Number of items inserted"] == ch.size, what
    if probe:
        pb, po = _probe(orc)
        assert np.array_equal(client.bf_mexists_packed(key, pb, po), ch.mexists_packed(pb, po)[0]), what


def _same(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {len(want)} replies differ, first at {bad[:8].tolist()}: got "
                           f"{np.asarray(got)[bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")


def _splits(cap):
    return sorted({s for s in (1, cap - 1, cap, cap + 1, 100) if 0 < s < oi.TINY_DRAWS})


ROWS = oi.tiny_chain_rows()


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_madd_tiny_chains(client, orc, row):
    """200 draws from 60 ids into a chain that fills after 1 .. 8 items (or
    never grows): as one call, as two calls split around the first link's
    capacity, and -- the two smallest chains -- one BF.ADD at a time; replies,
    links, bits, item count and BF.MEXISTS == the oracle's every time."""
    buf, offs, n = row["buf"], row["offs"], oi.TINY_DRAWS
    ch = oi.tiny_chain(row)
    want = ch.madd_packed(buf, offs)
    assert ch.nlinks <= oi.MAX_LINKS

    client.execute_command("BF.RESERVE", "one", *row["reserve"])
    _same(client.bf_madd_packed("one", buf, offs), want, "one call")
    _check_chain(client, orc, "one", ch, "one call")

    for s in _splits(row["capacity"]):
        key = f"split{s}"
        client.execute_command("BF.RESERVE", key, *row["reserve"])
        got = np.concatenate([client.bf_madd_packed(key, *oi.take(buf, offs, 0, s)),
                              client.bf_madd_packed(key, *oi.take(buf, offs, s, n))])
        _same(got, want, f"split at {s}")
        _check_chain(client, orc, key, ch, f"split at {s}")

    if row["capacity"] <= 2:
        assert not row["nonscaling"]
        client.execute_command("BF.RESERVE", "each", *row["reserve"])
        got = [client.execute_command("BF.ADD", "each", int(v)) for v in row["ids"]]
        _same(got, want, "one BF.ADD at a time")
        _check_chain(client, orc, "each", ch, "one BF.ADD at a time")


def _madd_device(client, key, buf, offs):
    """ske_bf_madd over device memory with a device reply buffer, as engine.preload(..., replies=True)."""
    from rtsas_amd._lib import SKE_MEM_DEVICE
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    n = len(offs) - 1
    b = DeviceBatch.from_host(client.ctx, buf, offs, np.zeros(1, np.uint32))
    out = DeviceBuffer(client.ctx, n)
    out.from_host(np.full(n, 7, np.int8))
    client.ctx.call("ske_bf_madd", client.keys.fid[key.encode()], C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), n,
                    C.c_void_p(out.ptr), SKE_MEM_DEVICE)
    got = out.to_host(np.int8, n)
    out.free()
    b.free()
    return got


@pytest.mark.parametrize("row", [ROWS[0], ROWS[3], ROWS[6]], ids=[ROWS[i]["name"] for i in (0, 3, 6)])
def test_madd_tiny_chains_device_memory(client, orc, row):
    """The same batch from device memory into a device reply buffer: identical replies and chain."""
    ch = oi.tiny_chain(row)
    want = ch.madd_packed(row["buf"], row["offs"])
    client.execute_command("BF.RESERVE", "dev", *row["reserve"])
    _same(_madd_device(client, "dev", row["buf"], row["offs"]), want, "device memory")
    _check_chain(client, orc, "dev", ch, "device memory")


def test_madd_past_the_grid(client, orc):
    """16 * CU * 256 + 333 ids, about half of them repeats, into a chain that
    grows in the call: the tail of every BF.MADD kernel's grid-stride loop,
    k_bf_count_cands' (4 * CU blocks) fifth trip."""
    cus = _cu()
    buf, offs, ids, _ = oi.past_the_grid(cus)
    _, ch, want = _past(orc, cus)
    assert ch.nlinks >= 2 and set(want[oi.grid_items(cus):].tolist()) == {0, 1}
    client.execute_command("BF.RESERVE", "past", *oi.past_the_grid_reserve(len(ids)))
    _same(client.bf_madd_packed("past", buf, offs), want, "past the grid")
    _check_chain(client, orc, "past", ch, "past the grid", probe=False)


# ---------------------------------------------------------------------------
# both on one context
# ---------------------------------------------------------------------------
def test_pfadd_and_madd_share_scratch(client, orc):
    """PFADD's sort keys and BF.MADD's first-setter table live in one scratch
    slot (kScrKeysOrFirst).  On one context: a PFADD of 50 000 (400 000 bytes of
    keys), a BF.MADD whose tables are larger, a PFADD of 200, a BF.MADD into a
    64-bit link (a 256-byte table), the first PFADD again -- each exact."""
    rng = np.random.default_rng(12)
    big_ids = 10_000_000 + rng.integers(0, 30_000, 50_000)
    big = oi.pack8(big_ids) + (rng.integers(0, 2, 50_000).astype(np.uint32),)
    small = oi.pack8(big_ids[:200] + 40_000) + (rng.integers(0, 2, 200).astype(np.uint32),)
    regs = _slab(client.ctx, 2, {0: oi.geometric_presets(1, 13, density=0.2)[0]})

    def pfadd(batch, what):
        buf, offs, slots = batch
        want = orc.hll_madd(regs, slots, buf, offs)
        _same(client.pfadd_packed(slots, buf, offs, changed=True), want, what)
        _check_slab(client.ctx, orc, regs, what)
        return want

    first = pfadd(big, "PFADD of 50 000")
    assert 0 < first.sum() < 50_000

    reserve = (0.01, 20_000, "EXPANSION", 2)
    ch = orc.Chain(*_chain_args(reserve))
    mbuf, moffs = oi.pack8(big_ids[:40_000])
    want = ch.madd_packed(mbuf, moffs)
    # (the slot holds keys * 5 / 4 + 256 bytes after the PFADD: both links' tables make it grow)
    assert ch.nlinks == 2 and ch.link_info(1)["bits"] > ch.link_info(0)["bits"] > 50_000 * 8 * 3 // 2 // 4
    client.execute_command("BF.RESERVE", "wide", *reserve)
    _same(client.bf_madd_packed("wide", mbuf, moffs), want, "BF.MADD, wide tables")
    _check_chain(client, orc, "wide", ch, "BF.MADD, wide tables")

    pfadd(small, "PFADD of 200")

    row = ROWS[6]
    assert row["nonscaling"]
    tiny = oi.tiny_chain(row)
    want = tiny.madd_packed(row["buf"], row["offs"])
    assert tiny.nlinks == 1 and tiny.link_info(0)["bits"] == 64
    client.execute_command("BF.RESERVE", "narrow", *row["reserve"])
    _same(client.bf_madd_packed("narrow", row["buf"], row["offs"]), want, "BF.MADD, 64-bit link")
    _check_chain(client, orc, "narrow", tiny, "BF.MADD, 64-bit link")

    again = pfadd(big, "the first PFADD again")
    assert not again.any()
