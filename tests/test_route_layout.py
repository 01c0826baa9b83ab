"""Routing at its edges, in one process with no collective.

csrc/sketch_route.hip is otherwise reached through the gloo subprocess tests
(world 2 and 3) and tests/test_exchange_gpu.py::test_route_cap_layout (world
<= 5, at most 245 scan words).  Here the key tables are built by hand, so the
cases hold what a KeyMap never produces -- an entry whose owner is outside
the world, a route word of 0xffffffff, keys past the table -- and reach:

- the exact form (ske_route_swipes: k_route_count, k_route_scan,
  k_route_scatter) directly, at worlds 1, 2, 5 and 64, id widths 8 (the
  8-byte path), 7, 1 and 19, and batch sizes around the 4096-swipe tile;
- k_route_scan's LDS carry between its 1024-word chunks (world * blocks >
  1024), in the exact and the capacity form, also with every swipe on one
  owner and with a last owner that receives nothing;
- world 64, where the route word's 6-bit owner field is full and 0xffffffff
  has to be told apart from "owner 63, slot 2^26 - 1";
- the capacity form at the largest owner's count, one below it (a single
  overflowing swipe) and 1;
- ske_route_slots_async / ske_route_return_async in their 16-byte vector and
  scalar variants (chosen by pointer alignment) with every n & 3.

Everything is compared bit-exactly with a numpy restatement."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO = 0xFFFFFFFF
NKEYS = 40
TILE = 4096          # swipes per routing block (kRtTile)
SCAN = 1024          # words per chunk of k_route_scan
BIG_LOCAL = (1 << 26) - 2
CARRY_N = {64: 17 * TILE + 1, 5: 205 * TILE + 7}
CARRY3_N = 32 * TILE + 1  # world 64: 2112 scan words, the carry passes through a whole chunk


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _tables(world):
    """key_owner / key_local and the packed key_route of 40 keys.  Key 5 names
    an owner outside the world, key 7 has no owner (route word 0xffffffff),
    key 0 belongs to rank 0 and key 13 to the last rank; at world 64 key 11 is
    rank 63's with a local slot just below 2^26 - 1 (route word 0xfffffffe)."""
    g = np.arange(NKEYS, dtype=np.uint64)
    owner = ((g * 7 + 3) % world).astype(np.uint32)
    local = (100 + 3 * g).astype(np.uint32)
    owner[0], owner[13] = 0, world - 1
    if world == 64:
        owner[11], local[11] = 63, BIG_LOCAL
    route = (owner << np.uint32(26)) | local
    owner[5] = world
    route[5] = (world << 26 | local[5]) if world < 64 else NO  # (6 bits cannot name rank 64)
    owner[7], route[7] = NO, NO
    if world == 64:
        assert route[11] == 0xFFFFFFFE
    return owner, local, route.astype(np.uint32)


def _expect(gk, world, owner, local):
    """Owner and local slot of every swipe: a key past the table, or one whose
    entry names no rank of this world, goes to rank 0 with slot 0xffffffff."""
    gk = gk.astype(np.int64)
    inside = gk < NKEYS
    gc = np.where(inside, gk, 0)
    known = inside & (owner[gc] < world)
    return np.where(known, owner[gc], 0).astype(np.int64), np.where(known, local[gc], NO).astype(np.uint32)


def _skew_owner(world, n):
    """The owner whose histogram words hold word 1024 of the scan (its later
    blocks' bases come through the carry), the last owner in a shorter scan."""
    return min(world - 1, SCAN // max(1, -(-n // TILE)))


def _gkeys(rng, n, world, owner, kind):
    if kind == "mixed":  # keys of the table, past it (40..42) and 0xffffffff
        gk = rng.integers(0, NKEYS + 3, n).astype(np.uint32)
        gk[rng.random(n) < 0.02] = NO
        return gk
    if kind == "skew":  # every swipe to one owner
        keys = np.nonzero(owner == _skew_owner(world, n))[0]
    else:  # "nolast": the last owner receives nothing
        keys = np.nonzero(owner < world - 1)[0]
    assert keys.size
    return keys[rng.integers(0, keys.size, n)].astype(np.uint32)


EXACT = [(w, (8, 7, 1, 19)[(i + j) % 4], n, "mixed")
         for i, w in enumerate((1, 2, 5, 64)) for j, n in enumerate((0, 1, TILE - 1, TILE, TILE + 1))]
EXACT += [(64, 8, CARRY_N[64], "mixed"), (5, 7, CARRY_N[5], "mixed"), (64, 19, CARRY_N[64], "skew"),
          (5, 8, CARRY_N[5], "skew"), (64, 1, CARRY_N[64], "nolast"), (5, 8, TILE + 1, "nolast"),
          (2, 8, 3 * TILE + 5, "skew"), (64, 8, CARRY3_N, "mixed")]


@pytest.mark.parametrize("world,width,n,kind", EXACT)
def test_route_exact_layout(engine, world, width, n, kind):
    """ske_route_swipes: counts == the owners' histogram; pos is a permutation
    of [0, n) that keeps every swipe inside its owner's range; the send rows
    hold the swipes' id bytes and local slots (0xffffffff on rank 0 for an
    unknown or unowned key)."""
    import torch
    owner, local, _ = _tables(world)
    rng = np.random.default_rng(world * 1000003 + n)
    if n in CARRY_N.values():
        assert world * -(-n // TILE) > SCAN, "the scan's carry is not live"
    if n == CARRY3_N:
        assert world * -(-n // TILE) > 2 * SCAN, "the scan has no third chunk"
    gk = _gkeys(rng, n, world, owner, kind)
    ids = rng.integers(0, 256, (n, width), dtype=np.uint8)
    own, loc = _expect(gk, world, owner, local)
    if kind == "mixed" and n >= TILE - 1:
        assert (loc == NO).any() and (gk == NO).any() and (gk >= NKEYS).any() and (gk == 5).any() and (gk == 7).any()
    d_ids, d_gk = torch.from_numpy(ids).cuda(), torch.from_numpy(gk.view(np.int32)).cuda()
    d_own, d_loc = torch.from_numpy(owner.view(np.int32)).cuda(), torch.from_numpy(local.view(np.int32)).cuda()
    s_ids = torch.full((n * width,), 0xCC, dtype=torch.uint8, device="cuda")
    s_slots = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pos = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    counts = np.full(world, 99, np.uint64)
    torch.cuda.synchronize()
    engine.ctx.call("ske_route_swipes", _vp(d_ids), width, _vp(d_gk), n, world, _vp(d_own), _vp(d_loc), NKEYS,
                    _vp(s_ids), _vp(s_slots), _vp(pos), counts.ctypes.data_as(C.c_void_p))
    torch.cuda.synchronize()
    want_counts = np.bincount(own, minlength=world)
    assert counts.tolist() == want_counts.tolist()
    if kind == "skew":
        assert counts[_skew_owner(world, n)] == n
    if kind == "nolast":
        assert counts[world - 1] == 0 and n > 0
    ps = pos.cpu().numpy().view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(ps), np.arange(n)), "pos is not a permutation of [0, n)"
    base = np.concatenate([[0], np.cumsum(want_counts)])
    assert ((ps >= base[own]) & (ps < base[own + 1])).all(), "a swipe outside its owner's rows"
    sid = s_ids.cpu().numpy().reshape(n, width)
    ssl = s_slots.cpu().numpy().view(np.uint32)
    assert np.array_equal(sid[ps], ids), "send_ids[pos[i]] != ids[i]"
    assert np.array_equal(ssl[ps], loc), "send_slots[pos[i]] != the key's local slot"


def _row_hash(row, slot, idb):
    """One u64 per (row, slot, id bytes)."""
    n, w = idb.shape
    pad = np.zeros((n, -(-w // 8) * 8), np.uint8)
    pad[:, :w] = idb
    h = row.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) ^ (slot.astype(np.uint64) << np.uint64(40))
    for word in pad.view(np.uint64).T:
        h = (h ^ word) * np.uint64(0xFF51AFD7ED558CCD)
        h ^= h >> np.uint64(33)
    return h


def _check_cap(engine, world, width, n, gk, ids, cap, route, owner, local, sinks):
    """The assertions of test_exchange_gpu.py::test_route_cap_layout."""
    import torch
    own, loc = _expect(gk, world, owner, local)
    rows = world * cap
    s_ids = torch.full((rows * width + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    s_slots = torch.full((rows,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    pos = torch.full((max(1, n),), -2, dtype=torch.int32, device="cuda")
    counts = torch.full((world,), -3, dtype=torch.int32, device="cuda")
    d_ids, d_gk = torch.from_numpy(ids).cuda(), torch.from_numpy(gk.view(np.int32)).cuda()
    d_route, d_sink = torch.from_numpy(route.view(np.int32)).cuda(), torch.from_numpy(sinks.view(np.int32)).cuda()
    torch.cuda.synchronize()
    engine.ctx.call("ske_route_swipes_cap_async", _vp(d_ids), width, _vp(d_gk), n, world, _vp(d_route), NKEYS, cap,
                    _vp(d_sink), _vp(s_ids), _vp(s_slots), _vp(pos), _vp(counts))
    engine.sync()
    torch.cuda.synchronize()
    ct = counts.cpu().numpy().view(np.uint32).astype(np.int64)
    assert ct.tolist() == np.bincount(own, minlength=world).tolist()
    ps = pos.cpu().numpy().view(np.uint32)[:n].astype(np.int64)
    assert ((ps // cap) == own).all(), "a swipe (overflowed ones included) outside its owner's rows"
    sid = s_ids.cpu().numpy()[:rows * width].reshape(rows, width)
    ssl = s_slots.cpu().numpy().view(np.uint32)
    for o in range(world):
        k = min(int(ct[o]), cap)
        r = o * cap + np.arange(cap)
        hit = np.zeros(cap, bool)
        hit[ps[own == o] - o * cap] = True
        assert hit[:k].all() and not hit[k:].any(), f"owner {o}: rows named by pos"
        assert (ssl[r[k:]] == sinks[o]).all() and not sid[r[k:]].any(), f"owner {o}: padding rows"
    # every real row holds (the id, the local slot) of one of the swipes that name it
    want = _row_hash(ps, loc, ids)
    rr = np.unique(ps)
    assert np.isin(_row_hash(rr, ssl[rr], sid[rr]), want).all()
    if (ct <= cap).all():  # nothing overflowed: every swipe is in its row
        assert np.array_equal(sid[ps], ids) and np.array_equal(ssl[ps], loc)
    return ct


@pytest.mark.parametrize("world,width,n,kind", [(64, 8, CARRY_N[64], "mixed"), (64, 7, CARRY_N[64], "skew"),
                                                (5, 7, TILE + 1, "mixed"), (5, 8, CARRY_N[5], "nolast"),
                                                (64, 8, CARRY3_N, "mixed")])
def test_route_cap_layout_edges(engine, world, width, n, kind):
    """ske_route_swipes_cap_async with a capacity equal to the largest
    owner's count (nothing overflows, no padding on that owner), one below it
    (one swipe overflows: counts[o] == cap + 1) and 1."""
    owner, local, route = _tables(world)
    rng = np.random.default_rng(world * 7919 + n)
    if n in CARRY_N.values():
        assert world * -(-n // TILE) > SCAN, "the scan's carry is not live"
    if n == CARRY3_N:
        assert world * -(-n // TILE) > 2 * SCAN, "the scan has no third chunk"
    gk = _gkeys(rng, n, world, owner, kind)
    ids = rng.integers(0, 256, (n, width), dtype=np.uint8)
    sinks = (5000 + 11 * np.arange(world)).astype(np.uint32)
    own, _ = _expect(gk, world, owner, local)
    top = int(np.bincount(own, minlength=world).max())
    assert top >= 3
    ct = _check_cap(engine, world, width, n, gk, ids, top, route, owner, local, sinks)
    assert ct.max() == top
    ct = _check_cap(engine, world, width, n, gk, ids, top - 1, route, owner, local, sinks)
    assert ct.max() == (top - 1) + 1
    _check_cap(engine, world, width, n, gk, ids, 1, route, owner, local, sinks)


def test_route_tables_agree():
    """The packed route words decode to the owner / local tables the
    expected values are computed from, at every world of this module."""
    for world in (1, 2, 3, 5, 64):
        owner, local, route = _tables(world)
        owned = (route != NO) & ((route >> 26) < world)
        assert np.array_equal(owned, owner < world)
        assert np.array_equal((route >> 26)[owned], owner[owned])
        assert np.array_equal((route & 0x3FFFFFF)[owned], local[owned])
        assert not owned[5] and not owned[7] and route[7] == NO


# ----------------------------------------------- route_slots / route_return
def _offset(torch, arr, off, guard):
    """A device copy of arr that starts `off` elements past a 16-byte aligned
    address, between two guard elements."""
    a = np.ascontiguousarray(arr)
    buf = np.full(4 * 16 + a.size + 1, guard, a.dtype)
    start = 16 + off
    buf[start:start + a.size] = a
    t = torch.from_numpy(buf).cuda()
    view = t[start:start + a.size]
    assert t.data_ptr() % 16 == 0 and (not a.size or view.data_ptr() - t.data_ptr() == start * a.itemsize)
    return t, view, start


@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 1), (0, 1), (1, 0)])
@pytest.mark.parametrize("table", ["identity", "route"])
def test_route_slots_alignment_and_tails(engine, table, off_in, off_out):
    """ske_route_slots_async == the numpy gather, with n & 3 = 0..3, through
    k_route_slots (both arrays 16-byte aligned) and k_route_slots1 (either one
    offset by 4 bytes); nothing is written outside out[0:n]."""
    import torch
    rng = np.random.default_rng(17)
    if table == "identity":  # key_route NULL: slot = gkey below nkeys
        world, d_route = 1, None
    else:  # a world-5 table read by a world of 3: ranks 3 and 4 own nothing here
        world = 3
        owner, local, route = _tables(5)
        assert (owner[owner < 5] >= world).any()
        d_route = torch.from_numpy(route.view(np.int32)).cuda()
    for n in (0, 1, 2, 3, 4, 5, 1027):
        gk = rng.integers(0, NKEYS + 3, n).astype(np.uint32)
        gk[rng.random(n) < 0.1] = NO
        if n >= 5:
            gk[:4] = [NKEYS - 1, NKEYS, NO, 5]
        if table == "identity":
            want = np.where(gk < NKEYS, gk, NO).astype(np.uint32)
        else:
            want = _expect(gk, world, owner, local)[1]
        t_in, v_in, _ = _offset(torch, gk.view(np.int32), off_in, -7)
        t_out, v_out, s_out = _offset(torch, np.zeros(n, np.int32), off_out, 0x0BADBEEF)
        v_out.fill_(0x0BADBEEF)
        torch.cuda.synchronize()
        engine.ctx.call("ske_route_slots_async", _vp(v_in), n, _vp(d_route) if d_route is not None else None,
                        NKEYS, world, _vp(v_out))
        engine.sync()
        torch.cuda.synchronize()
        got = t_out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[s_out:s_out + n], want), f"n = {n}"
        assert (got[:s_out] == 0x0BADBEEF).all() and (got[s_out + n:] == 0x0BADBEEF).all(), f"n = {n}: guards"


@pytest.mark.parametrize("off_pos,off_out", [(0, 0), (1, 1), (0, 1), (1, 0), (0, 4)])
def test_route_return_alignment_and_tails(engine, off_pos, off_out):
    """ske_route_return_async: out[i] == answers[pos[i]] with n & 3 = 0..3,
    through k_route_return4 (pos 16-byte, out 4-byte aligned) and
    k_route_return (pos offset by 4 bytes or out by 1 byte)."""
    import torch
    rng = np.random.default_rng(19)
    for n in (0, 1, 2, 3, 4, 5, 1027):
        m = n + 13
        answers = rng.integers(0, 256, m, dtype=np.uint8)
        pos = rng.integers(0, m, n).astype(np.uint32)
        d_ans = torch.from_numpy(answers).cuda()
        _, v_pos, _ = _offset(torch, pos.view(np.int32), off_pos, -1)
        t_out, v_out, s_out = _offset(torch, np.zeros(n, np.uint8), off_out, 0xEE)
        v_out.fill_(0xEE)
        torch.cuda.synchronize()
        engine.ctx.call("ske_route_return_async", _vp(d_ans), _vp(v_pos), n, _vp(v_out))
        engine.sync()
        torch.cuda.synchronize()
        got = t_out.cpu().numpy()
        assert np.array_equal(got[s_out:s_out + n], answers[pos]), f"n = {n}"
        assert (got[:s_out] == 0xEE).all() and (got[s_out + n:] == 0xEE).all(), f"n = {n}: guards"
