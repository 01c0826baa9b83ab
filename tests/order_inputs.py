"""Inputs for the order-exact paths (csrc/sketch_order.hip and the epoch loop
of ske_bf_madd): plain builders, no tests, no fixtures.

PFADD's per-element ``changed`` and BF.MADD's per-item replies depend on the
order of the batch.  The builders here choose batches in which that order
matters a great deal -- hundreds of elements of one HLL register, chains that
fill after one or two items, ids that repeat across the item that fills a link
-- and assert, on the oracle alone, that the batch has the shape its name says.
``rtsas_amd.keyhash._murmur_same_len`` (numpy MurmurHash64A) only *chooses*
elements; no expected value comes from it: every expectation of the tests is
``oracle.hll_madd`` or ``oracle.Chain``.

tests/test_order_inputs_host.py asserts the preconditions of every builder on
the CPU; tests/test_order_replies.py runs the batches on the device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import __graft_entry__ as ge

M = 16384                       # registers per key
HLL_SEED = 0xADC83B19           # hllPatLen's MurmurHash64A seed; register = low 14 bits
TARGETS = (0, 1, 3, 4, 8191, 16383)   # 0, 1 and 3 share one 32-bit word of the slab
WORD = (0, 1, 3)                # the registers of TARGETS that share a word
POOL_FIRST, POOL_IDS = 10_000_000, 1 << 21
NONSCALING = "NONSCALING"
MAX_LINKS = 48                  # SKE_MAX_LINKS (include/sketch.h)
BLOCK = 256                     # threads of every K4 block
K4_GRID = 16                    # blocks per CU of the K4 grids (4 for k_bf_count_cands)


def _orc():
    return ge.load_oracle()


def pack8(ids) -> tuple[np.ndarray, np.ndarray]:
    """Eight-digit decimal ids as (buf, offs)."""
    v = np.ascontiguousarray(ids, dtype=np.int64)
    assert v.size == 0 or (v.min() >= 10_000_000 and v.max() < 100_000_000)
    digits = np.zeros((v.size, 8), np.uint8)
    x = v.copy()
    for d in range(7, -1, -1):
        digits[:, d] = x % 10 + 48
        x //= 10
    return digits.reshape(-1), (np.arange(v.size + 1, dtype=np.uint64) * 8).astype(np.uint32)


def patlen(elem: bytes) -> tuple[int, int]:
    """(register, rank) of one element, from the oracle's hllPatLen."""
    reg = C.c_long()
    rank = _orc().lib().orc_hll_patlen(elem, len(elem), C.byref(reg))
    return int(reg.value), int(rank)


# ---------------------------------------------------------------------------
# PFADD
# ---------------------------------------------------------------------------
_POOL = {}


def same_register_pool(targets=TARGETS) -> dict:
    """The 8-digit ids 10_000_000 .. +2^21 whose HLL register is one of
    ``targets``: {register: (ids int64, ranks int64)}, ids ascending.  numpy
    picks the candidates; register and rank of every one kept are the
    oracle's."""
    targets = tuple(targets)
    if targets in _POOL:
        return _POOL[targets]
    ge.load_package()
    from rtsas_amd.keyhash import _murmur_same_len
    ids = POOL_FIRST + np.arange(POOL_IDS, dtype=np.int64)
    buf, _ = pack8(ids)
    idx = (_murmur_same_len(buf.reshape(-1, 8), HLL_SEED) & np.uint64(M - 1)).astype(np.int64)
    pool = {}
    for t in targets:
        mine = ids[idx == t]
        ranks = np.zeros(mine.size, np.int64)
        for j, v in enumerate(mine.tolist()):
            reg, ranks[j] = patlen(str(v).encode())
            assert reg == t, (v, reg, t)
        assert mine.size >= 64 and np.unique(ranks).size >= 4, (t, mine.size)
        pool[t] = (mine, ranks)
    _POOL[targets] = pool
    return pool


ORDERS = ("ascending", "descending", "ascending-repeated")


def stairs(pool, reg, order):
    """Every pool element of register ``reg`` as one batch, by rank:
    ``ascending`` (every new rank raises the register), ``descending`` (only
    the first does), ``ascending-repeated`` (ascending, each element twice in a
    row: the repeat meets its own rank).  Returns (buf, offs, ranks)."""
    ids, ranks = pool[reg]
    by = np.argsort(ranks, kind="stable")
    if order == "descending":
        by = by[::-1]
    elif order == "ascending-repeated":
        by = np.repeat(by, 2)
    else:
        assert order == "ascending", order
    buf, offs = pack8(ids[by])
    return buf, offs, ranks[by]


HEAVY = 8400                    # elements of long_segment's longest segment (> 8192)


def long_segment(pool, n=20_000, nslots_used=2, seed=0):
    """n elements over ``nslots_used`` slots and the pool's registers, drawn
    with replacement from the pool, slots and registers interleaved at random.
    Segment (slot 0, register 1) holds HEAVY elements; the other
    (slot, register) segments share the rest evenly.  Returns
    (buf, offs, slot index 0 .. nslots_used - 1, register, rank)."""
    rng = np.random.default_rng(seed)
    regs = sorted(pool)
    segs = [(s, r) for s in range(nslots_used) for r in regs]
    heavy = (0, 1) if 1 in pool else segs[0]
    rest = [sg for sg in segs if sg != heavy]
    counts = {heavy: HEAVY}
    for j, sg in enumerate(rest):
        counts[sg] = (n - HEAVY) // len(rest) + (j < (n - HEAVY) % len(rest))
    assert sum(counts.values()) == n and min(counts.values()) > 1000
    slot, reg, ids, rank = [], [], [], []
    for (s, r), c in counts.items():
        pick = rng.integers(0, pool[r][0].size, c)
        slot.append(np.full(c, s))
        reg.append(np.full(c, r))
        ids.append(pool[r][0][pick])
        rank.append(pool[r][1][pick])
    order = rng.permutation(n)
    slot, reg, ids, rank = (np.concatenate(a)[order] for a in (slot, reg, ids, rank))
    buf, offs = pack8(ids)
    return buf, offs, slot.astype(np.uint32), reg, rank


MIXED_LENGTHS = (0, 7, 8, 9, 15, 16, 17)   # MurmurHash64A's block and tail edges


def mixed_lengths(n=4_000, seed=0):
    """n byte strings of 0..40 bytes, one in three a repeat of an earlier one
    (the empty string and the lengths around the hash's 8-byte blocks among the
    fresh ones).  Returns (buf, offs, repeat: bool per item)."""
    rng = np.random.default_rng(seed)
    items, repeat = [], np.zeros(n, bool)
    forced = list(MIXED_LENGTHS)
    for i in range(n):
        if i >= len(forced) and i % 3 == 2:
            items.append(items[int(rng.integers(0, i))])
            repeat[i] = True
        else:
            k = forced[i] if i < len(forced) else int(rng.integers(0, 41))
            items.append(rng.integers(0, 256, k, dtype=np.uint8).tobytes())
    lens = {len(x) for x in items}
    assert lens >= set(MIXED_LENGTHS) and max(lens) == 40, sorted(lens)
    assert abs(repeat.mean() - 1 / 3) < 0.01
    return _orc().pack(items) + (repeat,)


def geometric_presets(nslots, seed, density=0.5):
    """[nslots, 16384] registers as earlier PFADDs leave them: geometric
    ranks (clipped to 51) on ``density`` of the registers, 0 elsewhere."""
    rng = np.random.default_rng(seed)
    vals = rng.geometric(0.5, (nslots, M)).clip(1, 51)
    return np.where(rng.random((nslots, M)) < density, vals, 0).astype(np.uint8)


# ---------------------------------------------------------------------------
# BF.MADD
# ---------------------------------------------------------------------------
TINY_IDS, TINY_DRAWS, TINY_SEED = 60, 200, 1
TINY = ((1, .5, 1), (2, .3, 1), (3, .25, 2), (5, .1, 2), (7, .4, 1), (8, .01, 4),
        (4, .3, 2, NONSCALING), (50, .01, 2, NONSCALING))


def tiny_chain_rows():
    """The chains that fill after a few items: one dict per row of TINY with
    ``capacity``, ``error``, ``expansion``, ``nonscaling``, the BF.RESERVE
    arguments after the key (``reserve``), and 200 draws from the decimal ids
    0 .. 59 as ``ids`` / ``buf`` / ``offs``."""
    rng = np.random.default_rng(TINY_SEED)
    rows = []
    for spec in TINY:
        cap, err, exp = spec[:3]
        non = len(spec) > 3
        ids = rng.integers(0, TINY_IDS, TINY_DRAWS)
        buf, offs = _orc().pack([str(int(v)).encode() for v in ids])
        rows.append(dict(capacity=cap, error=err, expansion=exp, nonscaling=non, ids=ids, buf=buf, offs=offs,
                         reserve=(err, cap, NONSCALING) if non else (err, cap, "EXPANSION", exp),
                         name=f"{cap}-{err}-{exp}" + ("-nonscaling" if non else "")))
    return rows


def tiny_chain(row):
    """A new oracle chain with the row's options."""
    return _orc().Chain(row["capacity"], row["error"], row["expansion"], row["nonscaling"])


def take(buf, offs, lo, hi):
    """Items lo .. hi - 1 of a packed batch as a packed batch of their own."""
    o = offs[lo:hi + 1].astype(np.int64)
    return buf[o[0]:o[-1]].copy(), (o - o[0]).astype(np.uint32)


def first_occurrence(ids):
    """bool per item: no earlier item of the batch has the same id."""
    first = np.zeros(len(ids), bool)
    first[np.unique(ids, return_index=True)[1]] = True
    return first


def grid_items(cus):
    """Items one trip of a K4 grid covers: 16 * CU blocks of 256."""
    return K4_GRID * cus * BLOCK


_PAST = {}


def past_the_grid(cus):
    """grid_items(cus) + 333 eight-digit ids drawn from 0.65 n values (about
    half of the items repeat an earlier one): every K4 kernel takes a second
    trip of its grid-stride loop, k_bf_count_cands (4 * CU blocks) a fifth.
    Returns (buf, offs, ids, slot: 0 .. 2 per item at random)."""
    if cus not in _PAST:
        n = grid_items(cus) + 333
        rng = np.random.default_rng(cus)
        ids = 10_000_000 + rng.integers(0, int(0.65 * n), n)
        assert ids.max() < 100_000_000
        _PAST[cus] = pack8(ids) + (ids, rng.integers(0, 3, n).astype(np.uint32))
    return _PAST[cus]


def past_the_grid_reserve(n):
    """BF.RESERVE's arguments after the key for past_the_grid: the chain grows in the call."""
    return (0.01, n // 4, "EXPANSION", 2)
