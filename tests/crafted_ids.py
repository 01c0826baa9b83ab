"""Ids with a chosen hash: plain builders, no tests, no fixtures.

MurmurHash64A is a bijection on each of its 8-byte blocks (the multiplier is
odd, ``x ^= x >> 47`` is its own inverse), so for any length >= 8, any seed and
any 64-bit target an id with that hash can be computed: the leading blocks and
the tail are free, one block is solved.  One id has one free target: its HLL
hash (seed 0xADC83B19: register and rank), or its Bloom ``a`` (seed
0xC6A4A7935BD1E995: the first probe ``a mod bits``).  ``b = Murmur(id, a)``
follows from the id and cannot be chosen, and neither can both hashes of one
id.

The arithmetic here only *chooses* inputs, as ``order_inputs.py`` does with
``_murmur_same_len``: every builder asserts on the oracle alone
(``orc_murmur64a``, ``orc_hll_patlen``) that each id it returns has the
register and rank, or the ``a``, it was asked for, and every expected value of
the tests is the oracle's.

tests/test_crafted_ids_host.py asserts the preconditions of every builder on
the CPU; tests/test_crafted_ranks.py and tests/test_crafted_probes.py run the
batches on the device.
"""
from __future__ import annotations

import numpy as np

import chain_shapes as cs
import order_inputs as oi

M64 = (1 << 64) - 1
MUL = 0xC6A4A7935BD1E995
MUL_INV = pow(MUL, -1, 1 << 64)
SHIFT = 47
HLL_SEED = oi.HLL_SEED
BLOOM_SEED = cs.BLOOM_SEED
MAX_RANK = 51                   # 64 - 14 + 1: all 50 bits above the register zero
REGS = (0, 1, 2, 3, 127, 128, 8191, 16383)  # 0..3 share a word, 127 | 128 straddle a 128-byte line
LENGTHS = (8, 9, 16, 17, 40)    # 8: murmur_short; the others: murmur_item's block and tail edges
ORDERS = ("ascending", "descending", "shuffled", "wave-packed")
WAVE = 64


def _orc():
    return oi._orc()


def _mix(k):
    k = k * MUL & M64
    k ^= k >> SHIFT
    return k * MUL & M64


def _unmix(k):
    k = k * MUL_INV & M64
    k ^= k >> SHIFT         # (2 * 47 >= 64: the shift-xor is its own inverse)
    return k * MUL_INV & M64


def invert(hash, seed, length, rng) -> bytes:
    """``length`` bytes whose MurmurHash64A under ``seed`` is ``hash``: the
    leading blocks and the tail from ``rng``, the last whole block solved."""
    if length < 8:
        raise ValueError("an id under 8 bytes carries fewer than 64 bits: not every hash has one")
    assert 0 <= hash <= M64 and 0 <= seed <= M64
    lead = rng.bytes(8 * (length // 8 - 1))
    tail = rng.bytes(length & 7)
    h = (seed ^ (length * MUL)) & M64
    for j in range(0, len(lead), 8):
        h = ((h ^ _mix(int.from_bytes(lead[j:j + 8], "little"))) * MUL) & M64
    g = hash ^ (hash >> SHIFT)
    g = g * MUL_INV & M64
    g ^= g >> SHIFT
    if tail:
        g = (g * MUL_INV & M64) ^ int.from_bytes(tail, "little")
    # g = (h ^ mix(block)) * MUL
    block = _unmix((g * MUL_INV & M64) ^ h)
    out = lead + block.to_bytes(8, "little") + tail
    assert len(out) == length and _orc().murmur64a(out, seed) == hash
    return out


def hll_id(register, rank, length, rng) -> bytes:
    """An id of HLL register ``register`` and rank ``rank`` (1 .. 51): the low
    14 bits of its hash are the register, the next rank - 1 bits zero, then a
    one (rank 51: all 50 bits zero), random bits above."""
    assert 0 <= register < oi.M and 1 <= rank <= MAX_RANK
    h = register
    if rank < MAX_RANK:
        top = 14 + rank                                  # the first free bit
        h |= 1 << (top - 1)
        h |= (int.from_bytes(rng.bytes(8), "little") << top) & M64
    out = invert(h, HLL_SEED, length, rng)
    assert oi.patlen(out) == (register, rank), (register, rank, oi.patlen(out))
    return out


def bloom_id(a, length, rng) -> bytes:
    """An id whose Bloom hash ``a`` (MurmurHash64A under the Bloom seed) is ``a``."""
    out = invert(a, BLOOM_SEED, length, rng)
    assert _orc().murmur64a(out, BLOOM_SEED) == a
    return out


def pack(ids, slots=None):
    """(buf with 16 bytes of slack, offs[, slots]) of a list of byte strings."""
    offs = np.zeros(len(ids) + 1, np.uint32)
    offs[1:] = np.cumsum([len(x) for x in ids])
    buf = np.frombuffer(b"".join(ids) + bytes(16), np.uint8).copy()
    return (buf, offs) if slots is None else (buf, offs, np.asarray(slots, np.uint32))


def unpack(buf, offs):
    return [bytes(buf[offs[i]:offs[i + 1]]) for i in range(len(offs) - 1)]


# ---------------------------------------------------------------------------
# PFADD batches: (buf, offs, slots)
# ---------------------------------------------------------------------------
_LADDER = {}


def _ladder_ids(registers, keys, seed):
    """{(key, register, rank): id}, every rank 1 .. 51, lengths in rotation."""
    at = (tuple(registers), tuple(keys), seed)
    if at not in _LADDER:
        rng = np.random.default_rng([seed, 1])
        ids, j = {}, 0
        for key in keys:
            for reg in registers:
                for rank in range(1, MAX_RANK + 1):
                    ids[key, reg, rank] = hll_id(reg, rank, LENGTHS[j % len(LENGTHS)], rng)
                    j += 1
        assert len(set(ids.values())) == len(ids)
        assert {len(x) for x in ids.values()} == set(LENGTHS)
        _LADDER[at] = ids
    return _LADDER[at]


def _wave_ids(registers, keys, seed):
    """The wave-packed ladder's own ids: per key, runs of 64 over registers
    0 .. 3 only, every (register, rank) once and the last run filled up with
    further ids of ranks of its own; the even runs hold 8-byte ids only (a wave
    of short ids), the odd ones every length of LENGTHS."""
    at = ("wave", tuple(registers), tuple(keys), seed)
    if at not in _LADDER:
        rng = np.random.default_rng([seed, 2])
        word = [r for r in registers if r < 4]
        assert len(word) >= 2
        out = []
        for key in keys:
            pairs = [(reg, rank) for reg in word for rank in range(1, MAX_RANK + 1)]
            pairs = [pairs[int(i)] for i in rng.permutation(len(pairs))]
            while len(pairs) % WAVE:
                # (ranks with free hash bits left: an 8-byte id of rank 51 is the only one of its register)
                pairs.append((word[int(rng.integers(0, len(word)))], int(rng.integers(1, 33))))
            for j, (reg, rank) in enumerate(pairs):
                run = j // WAVE
                length = 8 if run % 2 == 0 else LENGTHS[j % len(LENGTHS)]
                out.append((key, reg, rank, hll_id(reg, rank, length, rng)))
        # distinct within a key (the one 8-byte id of a register's rank 51 serves every key)
        assert len({(x[0], x[3]) for x in out}) == len(out)
        _LADDER[at] = out
    return _LADDER[at]


def ladder(registers=REGS, order="ascending", keys=(0, 1), seed=0):
    """Every rank 1 .. 51 on every register of ``registers`` for every key of
    ``keys``, distinct ids: ``ascending`` / ``descending`` by rank (registers
    and keys interleaved within a rank), ``shuffled``, or ``wave-packed``:
    every run of 64 consecutive items holds only registers 0 .. 3 of one key,
    ranks mixed (64 lanes of a wave on the four bytes of one word)."""
    assert order in ORDERS, order
    if order == "wave-packed":
        items = _wave_ids(registers, keys, seed)
        for r0 in range(0, len(items), WAVE):
            run = items[r0:r0 + WAVE]
            assert len(run) == WAVE and len({x[0] for x in run}) == 1 and {x[1] for x in run} <= {0, 1, 2, 3}
            assert len({x[2] for x in run}) >= 16
        want = {(k, r, q) for k in keys for r in registers if r < 4 for q in range(1, MAX_RANK + 1)}
    else:
        ids = _ladder_ids(registers, keys, seed)
        items = sorted(((k, r, q, x) for (k, r, q), x in ids.items()), key=lambda t: (t[2], t[1], t[0]))
        if order == "descending":
            items = items[::-1]
        elif order == "shuffled":
            by = np.random.default_rng([seed, 3]).permutation(len(items))
            items = [items[int(i)] for i in by]
        want = {(k, r, q) for k in keys for r in registers for q in range(1, MAX_RANK + 1)}
    assert {x[:3] for x in items} == want
    for k, r, q, x in items:
        assert oi.patlen(x) == (r, q)
    return pack([x[3] for x in items], [x[0] for x in items])


def repeats(key=0, register=3, length=16, seed=0):
    """One rank-51 id 64 times in a row."""
    x = hll_id(register, MAX_RANK, length, np.random.default_rng([seed, 4]))
    assert oi.patlen(x) == (register, MAX_RANK)
    return pack([x] * WAVE, [key] * WAVE)


FLOOR_REGS = tuple(range(32)) + tuple(range(oi.M - 32, oi.M))   # 64 registers: the key's first and last


def floor_edge_ranks(f, j):
    """The ranks floor_edges(f) sends to the j-th register of FLOOR_REGS: f - 1
    and f (at or under the floor) everywhere, f + 1 (one above it) on the even
    ones and on j = 3 mod 4, 51 on the odd ones; ranks outside 1 .. 51 left out."""
    ranks = [f - 1, f]
    if j % 2 == 0 or j % 4 == 3:
        ranks.append(f + 1)
    if j % 2 == 1:
        ranks.append(MAX_RANK)
    return sorted({q for q in ranks if 1 <= q <= MAX_RANK})


def floor_edges(f, key=0, seed=0):
    """Records of rank f - 1, f, f + 1 and 51 on the 64 registers FLOOR_REGS of
    one key (floor_edge_ranks), shuffled, distinct ids."""
    rng = np.random.default_rng([seed, 5, f])
    ids, j = [], 0
    for n, reg in enumerate(FLOOR_REGS):
        for rank in floor_edge_ranks(f, n):
            ids.append(hll_id(reg, rank, LENGTHS[j % len(LENGTHS)], rng))
            j += 1
    assert len(set(ids)) == len(ids)
    ids = [ids[int(i)] for i in rng.permutation(len(ids))]
    got = {}
    for x in ids:
        reg, rank = oi.patlen(x)
        got.setdefault(reg, set()).add(rank)
    assert got == {reg: set(floor_edge_ranks(f, n)) for n, reg in enumerate(FLOOR_REGS)}
    return pack(ids, [key] * len(ids))


def staircase(registers, order, seed=0):
    """The 51-step staircase of order-exact replies on ``registers`` (one, or
    several interleaved rank by rank): ``ascending``, ``descending`` or
    ``ascending-repeated`` (each element twice in a row).  (buf, offs)."""
    ids = _ladder_ids(tuple(registers), (0,), seed + 100)
    items = [ids[0, r, q] for q in range(1, MAX_RANK + 1) for r in registers]
    if order == "descending":
        items = items[::-1]
    elif order == "ascending-repeated":
        items = [x for x in items for _ in range(2)]
    else:
        assert order == "ascending", order
    return pack(items)


def spread(buf, offs, slots, crafted, rng, runs=False):
    """The filler batch (buf, offs, slots) with the crafted batch's items put in
    place of filler items, their order kept: at random places, or (``runs``) in
    whole runs of 64 that start on a multiple of 64.  Returns (buf, offs, slots,
    the crafted items' positions)."""
    cbuf, coffs, cslots = crafted
    n, m = len(offs) - 1, len(coffs) - 1
    if runs:
        assert m % WAVE == 0 and m <= n // WAVE * WAVE
        first = np.sort(rng.choice(n // WAVE, m // WAVE, replace=False)) * WAVE
        at = (first[:, None] + np.arange(WAVE)[None, :]).reshape(-1)
    else:
        assert m <= n
        at = np.sort(rng.choice(n, m, replace=False))
    ids = unpack(buf, offs)
    out_slots = np.array(slots, np.uint32)
    for p, x, s in zip(at.tolist(), unpack(cbuf, coffs), cslots.tolist()):
        ids[p] = x
        out_slots[p] = s
    return pack(ids, out_slots) + (at,)


def reverse(buf, offs, slots):
    """The same items in reverse order."""
    return pack(unpack(buf, offs)[::-1], slots[::-1].copy())


# ---------------------------------------------------------------------------
# Bloom: the first probe on every cut
# ---------------------------------------------------------------------------
PROBE_LENGTHS = (8, 13, 16, 24)


def lds_cuts(bits):
    """The bit positions where one 1 KiB LDS piece of a link ends and the next begins (k1_lds_plan)."""
    return tuple(range(8192, bits, 8192))


def part_cuts(bits):
    """Where one slice of 2^19 bits ends and the next begins (part_plan)."""
    return tuple(range(1 << cs.P_SLICE_LOG, bits, 1 << cs.P_SLICE_LOG))


def probe_positions(bits, cuts):
    pos = {0, 1, bits - 1}
    for c in cuts:
        assert 0 < c < bits
        pos |= {c - 1, c}
    return sorted(pos)


def probe_targets(bits, cuts, seed=0):
    """Ids whose first probe ``a mod bits`` is 0, 1, bits - 1, and c - 1 and c
    for every cut c -- each position x as a = x + bits * t for t = 0, a random
    t and the largest -- and the raw values of ``a`` at the edges of fastmod
    and of 32- and 64-bit arithmetic; four ids (8, 13, 16 and 24 bytes) per
    target.  Returns (buf, offs, a: one Python int per id)."""
    rng = np.random.default_rng([seed, 6, bits])
    q = (1 << 64) // bits
    targets = []
    for x in probe_positions(bits, cuts):
        tmax = (M64 - x) // bits
        ts = {0, tmax, 1 + int.from_bytes(rng.bytes(8), "little") % max(tmax - 1, 1)}
        targets += [x + bits * t for t in sorted(ts)]
    raw = [0, bits - 1, bits, (1 << 32) - 1, 1 << 32, 1 << 63, q * bits - 1, q * bits, M64 - 1, M64]
    targets += [a for a in raw if a <= M64]
    targets = list(dict.fromkeys(targets))
    ids, a_of = [], []
    for a in targets:
        assert 0 <= a <= M64
        for length in PROBE_LENGTHS:
            ids.append(bloom_id(a, length, rng))
            a_of.append(a)
    assert len(set(ids)) == len(ids)
    assert {a % bits for a in a_of} >= set(probe_positions(bits, cuts))
    return pack(ids) + (a_of,)


# The rows of tests/test_crafted_probes.py: one link each (BF.MADD adds to the
# last link alone, so only a one-link chain has every cut of the row within
# reach of a member), one per arm that cuts the bit space, and a plain one.
# part-11-cuts is this file's own: the km = 11 rows of chain_shapes.ROWS have
# one slice (part-11) or a last link of 64 bits (part-5-6); its fourth slice
# holds 64 bits.
PROBE_ROWS = (
    (cs.ROW["lds-b5"], lds_cuts),
    (cs.Row("part-11-cuts", [(8 * (192 * cs.KIB + 8), 11)], 3, "part km=11", seed=2001), part_cuts),
    (cs.ROW["part-12"], part_cuts),
    (cs.ROW["xr-k11"], cs.xr_cuts),
    (cs.ROW["xr-k17"], cs.xr_cuts),
    (cs.ROW["lds-d"], lambda bits: ()),
)
