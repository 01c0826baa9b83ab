"""Pass A of the fail-list path (k_part_a3, sketch_part.hip): the tile's
counting sort, placed by the counting atomic's rank, at two blocks per CU.

Every case runs the partitioned K1 (variant 3) on a one-link k = 11 chain
(RESERVE 0.001) and compares the answers and all registers bit-exactly with
the CPU oracle (oracle/sketch_oracle.c), as tests/test_k1_partitioned.py does.
The shapes are the smallest at which this sort can go wrong:

- tile edges: 1, 1023, 1024, 1025 and 2 * 1024 + 7 swipes (one thread of one
  tile, the full / not-full probe loops, the sink counter, both counter
  parities);
- 8 * 1024 + 1 swipes on a filter of 1e5 capacity (four slices: runs of
  thousands of records per tile), and 1600 tiles + 1 swipes on the same
  filter: tiles are dealt to 8 groups and a group's to a quarter of the
  resident blocks (64), so 200 tiles per group give blocks three or four
  tiles -- both counter parities and the record array reused
  while the copy-out of the tile before is in flight;
- one id repeated over whole tiles (11 slices take 1024 records each, the
  largest rank a counter hands out), an all-invalid and an all-valid batch;
- ids of 1..8 bytes mixed with longer ones (part_hash3's generic path), in
  the offsets layout and in the fixed layout (widths 5, 8 and 12);
- the 2048-counter instantiation: a chain of over 512 slice pairs (4e7
  capacity, over 1100 slices).
"""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ERROR = 0.001
NKEYS = 7


def _pack(items):
    offs = np.zeros(len(items) + 1, np.uint32)
    offs[1:] = np.cumsum([len(x) for x in items])
    buf = np.frombuffer(b"".join(items) + b"\0" * 16, np.uint8).copy()
    return buf, offs


def _pack_rows(rows):
    """Fixed-width ids (n x w bytes) in the offsets layout."""
    n, w = rows.shape
    buf = np.concatenate([rows.reshape(-1), np.zeros(16, np.uint8)])
    return buf, (np.arange(n + 1, dtype=np.uint64) * w).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _members():
    """20 000 ids of 8 bytes, 2 000 of 1..8 and 2 000 of 9..24 bytes."""
    rng = np.random.default_rng(1107)
    rows8 = rng.integers(0, 256, (20000, 8), dtype=np.uint8)
    items = [r.tobytes() for r in rows8]
    for lo, hi in ((1, 8), (9, 24)):
        items += [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(lo, hi + 1, 2000)]
    return rows8, items


@pytest.fixture(scope="module")
def chains(orc):
    """capacity -> the oracle's chain, built once per capacity and only read
    afterwards (released with the module)."""
    cache = {}

    def get(capacity):
        if capacity not in cache:
            buf, offs = _pack(_members()[1])
            chain = orc.Chain(capacity, ERROR)
            chain.madd_packed(buf, offs)
            assert chain.nlinks == 1 and chain.link_info(0)["hashes"] == 11
            cache[capacity] = chain
        return cache[capacity]

    yield get
    cache.clear()


def _filter(engine, chains, capacity):
    from rtsas_amd.engine import DeviceBatch
    items = _members()[1]
    buf, offs = _pack(items)
    engine.reserve(0, ERROR, capacity)
    dm = DeviceBatch.from_host(engine.ctx, buf, offs, np.zeros(len(items), np.uint32))
    engine.ctx.call("ske_bf_madd", 0, C.c_void_p(dm.bytes.ptr), C.c_void_p(dm.offs.ptr), len(items), None, 1)
    engine.set_option("variant", 3)
    assert engine.variant(0) == 3
    engine.hll_reserve(NKEYS)
    return chains(capacity)


def _check(engine, orc, chains, capacity, buf, offs, width=0):
    """Answers and registers of one batch == the oracle's; width > 0: the
    batch goes in the fixed layout (ids at i * width, no offsets)."""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    chain = _filter(engine, chains, capacity)
    n = len(offs) - 1
    keys = ((np.arange(n, dtype=np.uint64) * 2654435761) % NKEYS).astype(np.uint32)
    out = DeviceBuffer(engine.ctx, n)
    if width:
        assert np.array_equal(offs, (np.arange(n + 1, dtype=np.uint64) * width).astype(np.uint32))
        b = DeviceBatch(engine.ctx, n, width)
        b.bytes.from_host(buf[:n * width])
        b.slot.from_host(keys)
        engine.swipes_fixed(0, b, out)
    else:
        b = DeviceBatch.from_host(engine.ctx, buf, offs, keys)
        engine.swipes(0, b, out)
    regs = np.zeros((NKEYS, 16384), np.uint8)
    valid, nvalid, _ = orc.process_swipes(chain, regs, keys, buf, offs)
    assert np.array_equal(out.to_host(np.uint8, n), valid)
    assert np.array_equal(engine.registers_all(NKEYS), regs)
    return int(nvalid)


def _rows8(seed, n, member_frac=0.8):
    """n ids of 8 bytes: members with probability member_frac, else random."""
    rng = np.random.default_rng(seed)
    rows8 = _members()[0]
    rows = rng.integers(0, 256, (n, 8), dtype=np.uint8)
    pick = rng.random(n) < member_frac
    rows[pick] = rows8[rng.integers(0, len(rows8), int(pick.sum()))]
    return rows


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2 * 1024 + 7])
def test_tile_edges(engine, orc, chains, n):
    nvalid = _check(engine, orc, chains, 10_000_000, *_pack_rows(_rows8(n, n)))
    assert n < 1000 or 0.7 * n < nvalid < 0.9 * n


@pytest.mark.parametrize("ntiles", [8, 1600])
def test_small_filter_tiles_per_block(engine, orc, chains, ntiles):
    n = ntiles * 1024 + 1
    nvalid = _check(engine, orc, chains, 100_000, *_pack_rows(_rows8(ntiles, n)))
    assert 0.7 * n < nvalid < 0.9 * n


@pytest.mark.parametrize("member", [True, False])
def test_one_id_repeated_over_tiles(engine, orc, chains, member):
    """2 * 1024 + 5 copies of one id: its 11 probes' slices take every record."""
    rng = np.random.default_rng(3)
    row = _members()[0][17] if member else rng.integers(0, 256, 8, dtype=np.uint8)
    n = 2 * 1024 + 5
    nvalid = _check(engine, orc, chains, 10_000_000, *_pack_rows(np.tile(row, (n, 1))))
    assert nvalid == (n if member else 0)


@pytest.mark.parametrize("member_frac", [0.0, 1.0])
def test_all_invalid_and_all_valid(engine, orc, chains, member_frac):
    n = 3 * 1024 + 100
    nvalid = _check(engine, orc, chains, 10_000_000, *_pack_rows(_rows8(5, n, member_frac)))
    assert nvalid == n if member_frac else nvalid < n // 100


def test_mixed_id_lengths_offsets_layout(engine, orc, chains):
    """Members and strangers of 1..8 bytes, empty ids, and ids of 9..24 bytes
    (a wave holding one takes the generic MurmurHash64A), shuffled."""
    rng = np.random.default_rng(9)
    items = _members()[1]
    n = 4 * 1024 + 77
    batch = [items[int(i)] for i in rng.integers(0, len(items), n // 2)]
    batch += [rng.integers(0, 256, int(l), dtype=np.uint8).tobytes() for l in rng.integers(0, 13, n - len(batch))]
    batch = [batch[int(i)] for i in rng.permutation(n)]
    nvalid = _check(engine, orc, chains, 10_000_000, *_pack(batch))
    assert nvalid >= n // 2


@pytest.mark.parametrize("width", [5, 8, 12])
def test_fixed_layout_widths(engine, orc, chains, width):
    """The fixed layout (no offsets array); width 12 takes the generic hash.
    Members of exactly `width` bytes make up about half the batch."""
    rng = np.random.default_rng(width)
    own = np.asarray([np.frombuffer(x, np.uint8) for x in _members()[1] if len(x) == width])
    assert len(own) >= 50
    n = 2 * 1024 + 300
    rows = rng.integers(0, 256, (n, width), dtype=np.uint8)
    pick = rng.random(n) < 0.5
    rows[pick] = own[rng.integers(0, len(own), int(pick.sum()))]
    buf, offs = _pack_rows(rows)
    nvalid = _check(engine, orc, chains, 10_000_000, buf, offs, width=width)
    assert 0.4 * n < nvalid < 0.6 * n


@pytest.mark.parametrize("member_frac", [0.8, 0.0])
def test_2048_counters(engine, orc, chains, member_frac):
    """4e7 capacity: over 512 slice pairs, the 2048-counter instantiation."""
    chain = chains(40_000_000)
    assert chain.link_info(0)["bits"] >= 512 * 2 * (1 << 19)
    n = 3 * 1024 + 513
    _check(engine, orc, chains, 40_000_000, *_pack_rows(_rows8(11, n, member_frac)))
