"""HLL keys in bulk on the GPU (csrc/sketch_hll_fmt.hip through ske_hll_dump_sizes
/ ske_hll_dump / ske_hll_load, the engine, the facade's dump_hlls / load_hlls /
save_hlls / restore_hlls and MGET / MSET).  Expected bytes are
``formats.encode_hll`` of the registers read back with ``hll_registers``;
expected registers are ``formats.decode_hll`` and the oracle's
``hll_decode_string`` -- never the device against itself.  Every case is a few
keys."""
import ctypes as C

import numpy as np
import pytest

import hllfmt_cases as hc

pytestmark = pytest.mark.gpu
M = 16384
HOST, DEVICE = 0, 1
EINVAL, ERANGE, EBADHLL = -1, -7, -11


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _plant(client, rows, prefix="k"):
    names = [f"{prefix}{i}" for i in range(len(rows))]
    for n, r in zip(names, rows):
        client.hll_load_registers(n, r)
    return names


def _slots(client, names):
    return np.asarray([client.keys.slot[n.encode()] for n in names], np.uint32)


def _abi_dump(client, slots, smb=3000, flags=0):
    """sizes, then the strings into a buffer with a guard behind ``total``"""
    slots = np.ascontiguousarray(slots, np.uint32)
    n = slots.size
    offs, offs2 = np.zeros(n + 1, np.uint32), np.full(n + 1, 0xFFFFFFFF, np.uint32)
    client.ctx.call("ske_hll_dump_sizes", _ptr(slots), n, smb, _ptr(offs), HOST)
    total = int(offs[-1])
    out = np.full(total + 64, 0xA5, np.uint8)
    client.ctx.call("ske_hll_dump", _ptr(slots), n, smb, flags, _ptr(out), total, _ptr(offs2), HOST)
    assert np.array_equal(offs, offs2) and offs[0] == 0 and (np.diff(offs.astype(np.int64)) >= 16).all()
    assert (out[total:] == 0xA5).all()
    return [out[offs[i]:offs[i + 1]].tobytes() for i in range(n)], offs


def _abi_load(client, slots, strings, mem_status=True):
    slots = np.ascontiguousarray(slots, np.uint32)
    offs = np.zeros(len(strings) + 1, np.uint32)
    np.cumsum([len(s) for s in strings], out=offs[1:])
    blob = np.frombuffer(b"".join(strings) + b"\0", np.uint8)
    status = np.full(len(strings), 9, np.uint8)
    rc = client.ctx.lib.ske_hll_load(client.ctx.ptr, _ptr(slots), len(strings), _ptr(blob), _ptr(offs),
                                     _ptr(status) if mem_status else None, HOST)
    return rc, status.tolist()


# ---------------------------------------------------------------- encode
@pytest.mark.parametrize("smb", [3000, 0, 16384])
def test_encode_patterns(pkg, client, smb):
    f = pkg.formats
    cases = hc.encode_rows()
    names = _plant(client, [r for _, r in cases])
    got = client.dump_hlls(names, sparse_max_bytes=smb)
    for (what, _), n, s in zip(cases, names, got):
        assert s == f.encode_hll(client.hll_registers(n), None, smb), (what, smb)
    by = dict(zip([w for w, _ in cases], got))
    if smb == 3000:
        assert by["empty"] == f.encode_hll(np.zeros(M, np.uint8)) and by["empty"][16:] == b"\x7f\xff" \
            and len(by["empty"]) == 18
        assert by["VAL runs 1..9 of 33"][4] == 0 and by["VAL runs 1..9 of 32"][4] == 1
    if smb == 16384:
        assert len(by["alternating"]) == 16 + M and by["alternating"][4] == 1  # the longest sparse string
    if smb == 0:
        assert all(s[4] == 0 and len(s) == 16 + 12288 for s in got)
    # dump_hll is what it was
    assert client.dump_hll(names[1]) == f.encode_hll(client.hll_registers(names[1]))


def test_encode_promotion_edge(pkg, client):
    f = pkg.formats
    rows = hc.promotion_rows()
    assert [len(f.sparse_pack(r)) for r in rows.values()] == [2999, 3000, 3001]
    alt = np.zeros(M, np.uint8)
    alt[::2] = 5
    names = _plant(client, list(rows.values()) + [alt])
    for smb in (2998, 2999, 3000, 3001, 16383, 16384):
        got = client.dump_hlls(names, sparse_max_bytes=smb)
        for n, s, size in zip(names, got, [2999, 3000, 3001, 16384]):
            assert s == f.encode_hll(client.hll_registers(n), None, smb), (size, smb)
            assert s[4] == (1 if size <= smb else 0)


def test_encode_filled_keys_with_cardinality(pkg, client):
    f = pkg.formats
    names = []
    for n in (1, 10, 300, 3000, 20000):
        names.append(f"filled{n}")
        client.pfadd(names[-1], *range(5000000, 5000000 + n))
    counts = client.pfcount_each(names)
    plain = client.dump_hlls(names)
    carded = client.dump_hlls(names, with_card=True)
    encs = []
    for n, s, sc, cnt in zip(names, plain, carded, counts):
        regs = client.hll_registers(n)
        assert s == f.encode_hll(regs) == client.dump_hll(n)
        assert sc == f.encode_hll(regs, int(cnt)) and f.cached_card(sc) == int(cnt) and f.cached_card(s) is None
        encs.append(s[4])
    assert encs == [1, 1, 1, 0, 0]  # 3000 ids pass 3000 sparse bytes


def _many_keys(pkg, client, nkeys, seed):
    """nkeys keys, each with a few registers of its own, filled by one PFADD batch"""
    rng = np.random.default_rng(seed)
    names = [f"many{i}" for i in range(nkeys)]
    slots = np.asarray([client.key_slot(n) for n in names], np.uint32)
    ids = rng.integers(10**6, 10**7, nkeys * 6)
    buf, offs = pkg.pack_ints(ids)
    client.pfadd_packed(np.repeat(slots, 6), buf, offs)
    return names, slots


def test_key_lists(pkg, client):
    f = pkg.formats
    from rtsas_amd.engine import SketchEngine
    names, slots = _many_keys(pkg, client, 300, 3)
    rows = SketchEngine(ctx=client.ctx).registers_all(int(slots.max()) + 1)
    want = {int(s): f.encode_hll(rows[s]) for s in slots}
    rng = np.random.default_rng(4)
    for n in (1, 2, 255, 257):
        pick = rng.permutation(slots)[:n][::1].copy()  # shuffled, non-contiguous
        if n > 1:
            pick[-1] = pick[0]  # a repeat
        got, offs = _abi_dump(client, pick)
        assert got == [want[int(s)] for s in pick]
        assert offs[-1] == sum(len(want[int(s)]) for s in pick)
    # slots == NULL: keys 0 .. n - 1
    offs = np.zeros(6, np.uint32)
    client.ctx.call("ske_hll_dump_sizes", None, 5, 3000, _ptr(offs), HOST)
    assert np.diff(offs).tolist() == [len(f.encode_hll(rows[s])) for s in range(5)]
    out = np.zeros(int(offs[-1]), np.uint8)
    client.ctx.call("ske_hll_dump", None, 5, 3000, 0, _ptr(out), out.size, _ptr(offs), HOST)
    assert out.tobytes() == b"".join(f.encode_hll(rows[s]) for s in range(5))
    # no keys: the one offset
    offs = np.full(1, 7, np.uint32)
    client.ctx.call("ske_hll_dump_sizes", _ptr(slots), 0, 3000, _ptr(offs), HOST)
    assert offs[0] == 0
    # the facade in chunks of 3 over 10 keys, a missing one among them
    ten = names[:4] + ["nokey"] + names[290:296]
    assert client.dump_hlls(ten, chunk_keys=3) == [client.dump_hll(n) for n in ten]


def test_cardinality_flag(pkg, client):
    f = pkg.formats
    names, slots = _many_keys(pkg, client, 40, 5)
    client.pfadd(names[7], *range(100, 4100))  # a dense one among them
    got, _ = _abi_dump(client, slots, flags=1)
    counts = client.pfcount_each(names)
    assert [f.cached_card(s) for s in got] == [int(c) for c in counts] and counts[7] > 3000
    assert all(s[15] & 0x80 == 0 for s in got)
    assert got == [f.encode_hll(client.hll_registers(n), int(c)) for n, c in zip(names, counts)]
    with pytest.raises(pkg.SketchLibError) as e:  # an unknown flag
        offs = np.zeros(41, np.uint32)
        client.ctx.call("ske_hll_dump", _ptr(slots), 40, 3000, 2, _ptr(np.zeros(1 << 20, np.uint8)), 1 << 20,
                        _ptr(offs), HOST)
    assert e.value.code == EINVAL


def test_cap_one_byte_short(pkg, client):
    names, slots = _many_keys(pkg, client, 5, 6)
    _, offs = _abi_dump(client, slots)
    total = int(offs[-1])
    buf = np.full(total + 64, 0x5A, np.uint8)
    offs2 = np.full(6, 0xFFFFFFFF, np.uint32)
    rc = client.ctx.lib.ske_hll_dump(client.ctx.ptr, _ptr(slots), 5, 3000, 0, _ptr(buf[32:]), total - 1, _ptr(offs2),
                                     HOST)
    assert rc == EINVAL and (buf == 0x5A).all() and (offs2 == 0xFFFFFFFF).all()
    # the same on the device, where the kernel writes the caller's buffer itself
    from rtsas_amd.engine import DeviceBuffer
    dev = DeviceBuffer(client.ctx, total + 64)
    dslots, doffs = DeviceBuffer(client.ctx, 20), DeviceBuffer(client.ctx, 24)
    try:
        dev.from_host(buf)
        dslots.from_host(slots)
        rc = client.ctx.lib.ske_hll_dump(client.ctx.ptr, C.c_void_p(dslots.ptr), 5, 3000, 0, C.c_void_p(dev.ptr + 32),
                                         total - 1, C.c_void_p(doffs.ptr), DEVICE)
        assert rc == EINVAL and (dev.to_host(np.uint8, total + 64) == 0x5A).all()
    finally:
        for b in (dev, dslots, doffs):
            b.free()


def test_device_form_end_to_end_every_alignment(pkg, client):
    """SKE_MEM_DEVICE: dump into a device buffer at every address mod 16 (guards
    around it), load it back from there into other slots"""
    f = pkg.formats
    from rtsas_amd.engine import DeviceBuffer, SketchEngine
    eng = SketchEngine(ctx=client.ctx)
    rows = [np.zeros(M, np.uint8), hc.promotion_rows()[2999], hc.encode_rows()[-1][1],
            np.random.default_rng(8).integers(0, 52, M).astype(np.uint8), hc.promotion_rows()[3001]]
    src = _plant(client, rows, "src")
    dst = _plant(client, [np.full(M, 1, np.uint8)] * len(rows), "dst")
    want = [f.encode_hll(client.hll_registers(n)) for n in src]
    assert [s[4] for s in want] == [1, 1, 1, 0, 0] and len({len(s) % 16 for s in want}) >= 3
    total = sum(map(len, want))
    n = len(rows)
    dslots, dslots2 = DeviceBuffer(client.ctx, 4 * n), DeviceBuffer(client.ctx, 4 * n)
    doffs, dstat = DeviceBuffer(client.ctx, 4 * n + 4), DeviceBuffer(client.ctx, n)
    out = DeviceBuffer(client.ctx, total + 96)
    try:
        dslots.from_host(_slots(client, src))
        dslots2.from_host(_slots(client, dst))
        eng.hll_dump_sizes(dslots, n, doffs)
        assert doffs.to_host(np.uint32, n + 1).tolist() == np.concatenate(([0], np.cumsum([len(s) for s in want]))).tolist()
        for shift in range(16):
            out.from_host(np.full(total + 96, 0xC3, np.uint8))
            client.ctx.call("ske_hll_dump", C.c_void_p(dslots.ptr), n, 3000, 0, C.c_void_p(out.ptr + 32 + shift), total,
                            C.c_void_p(doffs.ptr), DEVICE)
            got = out.to_host(np.uint8, total + 96)
            assert got[32 + shift:32 + shift + total].tobytes() == b"".join(want), shift
            assert (got[:32 + shift] == 0xC3).all() and (got[32 + shift + total:] == 0xC3).all(), shift
            # back in from the same place: every string starts at another address mod 16
            for d in dst:
                client.hll_load_registers(d, np.full(M, 1, np.uint8))
            client.ctx.call("ske_hll_load", C.c_void_p(dslots2.ptr), n, C.c_void_p(out.ptr + 32 + shift),
                            C.c_void_p(doffs.ptr), C.c_void_p(dstat.ptr), DEVICE)
            assert dstat.to_host(np.uint8, n).tolist() == [0] * n
            for d, r in zip(dst, rows):
                assert np.array_equal(client.hll_registers(d), r), shift
        # the engine's calls
        out2 = DeviceBuffer(client.ctx, total)
        eng.hll_dump(dslots, n, out2, doffs, with_card=True)
        head = out2.to_host(np.uint8, total)[:16].tobytes()
        assert f.cached_card(head) == 0  # the empty key
        eng.hll_load(dslots2, n, out2, doffs, dstat)
        out2.free()
        # offsets that decrease, and a slot list past the slab, are refused on the device
        bad = doffs.to_host(np.uint32, n + 1)
        bad[2] = bad[1] - 1
        doffs.from_host(bad)
        rc = client.ctx.lib.ske_hll_load(client.ctx.ptr, C.c_void_p(dslots2.ptr), n, C.c_void_p(out.ptr),
                                         C.c_void_p(doffs.ptr), None, DEVICE)
        assert rc == EINVAL
        cap = client.ctx.lib.ske_hll_capacity(client.ctx.ptr)
        dslots.from_host(np.asarray([0, 1, cap, 2, 3], np.uint32))
        out.from_host(np.full(total + 96, 0xC3, np.uint8))
        doffs.from_host(np.full(n + 1, 0x77777777, np.uint32))
        lib, ctx = client.ctx.lib, client.ctx.ptr
        assert lib.ske_hll_dump_sizes(ctx, C.c_void_p(dslots.ptr), n, 3000, C.c_void_p(doffs.ptr), DEVICE) == ERANGE
        assert lib.ske_hll_dump(ctx, C.c_void_p(dslots.ptr), n, 3000, 0, C.c_void_p(out.ptr), total + 96,
                                C.c_void_p(doffs.ptr), DEVICE) == ERANGE
        assert (out.to_host(np.uint8, total + 96) == 0xC3).all()
        assert (doffs.to_host(np.uint32, n + 1) == 0x77777777).all()
    finally:
        for b in (dslots, dslots2, doffs, dstat, out):
            b.free()


def test_slot_at_capacity_and_too_many_keys(pkg, client):
    client.pfadd("a", 1)
    lib, ctx = client.ctx.lib, client.ctx.ptr
    cap = lib.ske_hll_capacity(ctx)
    slots = np.asarray([0, cap], np.uint32)
    offs = np.full(3, 5, np.uint32)
    out = np.full(64, 0x11, np.uint8)
    assert lib.ske_hll_dump_sizes(ctx, _ptr(slots), 2, 3000, _ptr(offs), HOST) == ERANGE
    assert lib.ske_hll_dump(ctx, _ptr(slots), 2, 3000, 0, _ptr(out), 64, _ptr(offs), HOST) == ERANGE
    s = pkg.formats.encode_hll(np.zeros(M, np.uint8))
    o = np.asarray([0, len(s), 2 * len(s)], np.uint32)
    blob = np.frombuffer(s + s, np.uint8)
    assert lib.ske_hll_load(ctx, _ptr(slots), 2, _ptr(blob), _ptr(o), None, HOST) == ERANGE
    assert (offs == 5).all() and (out == 0x11).all() and client.pfcount("a") == 1
    assert lib.ske_hll_dump_sizes(ctx, None, cap + 1, 3000, _ptr(offs), HOST) in (ERANGE, EINVAL)
    too_many = (1 << 18) + 1
    assert lib.ske_hll_dump_sizes(ctx, None, too_many, 3000, _ptr(offs), HOST) == EINVAL
    assert lib.ske_hll_dump(ctx, None, too_many, 3000, 0, _ptr(out), 64, _ptr(offs), HOST) == EINVAL
    assert lib.ske_hll_load(ctx, None, too_many, _ptr(blob), _ptr(o), None, HOST) == EINVAL
    o[1] = len(s) + 1  # offsets that decrease
    o[2] = len(s)
    assert lib.ske_hll_load(ctx, _ptr(np.asarray([0, 1], np.uint32)), 2, _ptr(blob), _ptr(o), None, HOST) == EINVAL


# ---------------------------------------------------------------- decode
def test_dump_flush_load_round_trip(pkg, client):
    rows = [r for _, r in hc.encode_rows()[:30]]
    names = _plant(client, rows)
    client.pfadd("filled", *range(700000, 704000))
    names.append("filled")
    rows.append(client.hll_registers("filled"))
    counts = client.pfcount_each(names)
    strings = client.dump_hlls(names)
    client.flushall()
    assert client.exists(*names) == 0
    client.hll_load_registers(names[3], np.full(M, 50, np.uint8))  # SET replaces: no merge with what is there
    client.load_hlls(zip(names, strings))
    assert client.exists(*names) == len(names)
    for n, r in zip(names, rows):
        assert np.array_equal(client.hll_registers(n), r), n
    assert np.array_equal(client.pfcount_each(names), counts)


def test_load_noncanonical_strings(pkg, orc, client):
    f = pkg.formats
    cases = hc.valid_noncanonical()
    client.load_hlls([(f"nc{i}", s) for i, (_, s) in enumerate(cases)])
    for i, (what, s) in enumerate(cases):
        got = client.hll_registers(f"nc{i}")
        assert np.array_equal(got, f.decode_hll(s)), what
        assert np.array_equal(got, orc.hll_decode_string(s)), what


def test_load_corrupt_strings_beside_good_ones(pkg, orc, client):
    f = pkg.formats
    bad = hc.corrupt_strings()
    good = [f.encode_hll(r) for _, r in hc.encode_rows()[5:9]] + [s for _, s in hc.valid_noncanonical()[:3]]
    strings, kinds = [], []
    for i, (_, s) in enumerate(bad):  # good ones between the bad ones
        strings += [s, good[i % len(good)]]
        kinds += [True, False]
    sentinel = np.full(M, 7, np.uint8)
    names = _plant(client, [sentinel] * len(strings), "t")
    rc, status = _abi_load(client, _slots(client, names), strings)
    assert rc == EBADHLL
    assert status == [hc.expect_decode(f, s)[0] for s in strings]
    want_bad = {"bad magic": 1, "15 bytes": 1, "empty string": 1}
    assert [st for st, k in zip(status, kinds) if k] == [want_bad.get(what, 2) for what, _ in bad]
    for n, s, is_bad in zip(names, strings, kinds):
        got = client.hll_registers(n)
        if is_bad:
            assert np.array_equal(got, sentinel), n  # untouched
        else:
            assert np.array_equal(got, f.decode_hll(s)) and np.array_equal(got, orc.hll_decode_string(s)), n
    # all good: SKE_OK, with and without a status array
    rc, status = _abi_load(client, _slots(client, names[:4]), good[:4])
    assert rc == 0 and status == [0] * 4
    rc, _ = _abi_load(client, _slots(client, names[:2]), [bad[0][1], good[0]], mem_status=False)
    assert rc == EBADHLL
    # the facade: the good pairs are in, load_hll's error for the first bad pair, no key made for a bad string
    client.flushall()
    pairs = [(f"p{i}", s) for i, s in enumerate(strings)]
    with pytest.raises(pkg.ResponseError) as e1:
        client.load_hlls(pairs)
    with pytest.raises(pkg.ResponseError) as e2:
        client.load_hll("x", strings[0])
    assert str(e1.value) == str(e2.value) and client.exists("x") == 0
    for (n, s), is_bad in zip(pairs, kinds):
        assert client.exists(n) == (0 if is_bad else 1)
        if not is_bad:
            assert np.array_equal(client.hll_registers(n), f.decode_hll(s))
    only52 = [s for what, s in bad if what == "dense register of 52"]
    with pytest.raises(pkg.SketchLibError) as e3:
        client.load_hlls([("y", only52[0])])
    assert client.exists("y") == 0
    with pytest.raises(pkg.SketchLibError) as e4:
        client.load_hll("y2", only52[0])
    assert e3.value.code == e4.value.code == EBADHLL and str(e3.value) == str(e4.value)


def test_load_strings_at_every_offset_mod_16(pkg, client):
    """host form: strings back to back in the blob, each behind a filler that
    moves the next to another alignment"""
    f = pkg.formats
    sparse = f.encode_hll(hc.encode_rows()[12][1])
    dense = f.encode_hll(np.random.default_rng(2).integers(0, 52, M).astype(np.uint8))
    strings, at = [], 0
    for k in range(16):
        j = (k - at - 18) % 16 + 16  # a valid filler string of 18 + j bytes: the next string starts at k mod 16
        strings += [hc.hyll(hc.ops(*[("z", 1)] * j)), sparse if k % 2 else dense]
        at += len(strings[-2]) + len(strings[-1])
    starts = np.concatenate(([0], np.cumsum([len(s) for s in strings])))[:-1] % 16
    assert starts[1::2].tolist() == list(range(16))
    names = _plant(client, [np.full(M, 3, np.uint8)] * len(strings), "al")
    rc, status = _abi_load(client, _slots(client, names), strings)
    assert rc == 0 and status == [0] * len(strings)
    for n, s in zip(names, strings):
        assert np.array_equal(client.hll_registers(n), f.decode_hll(s)), n


def test_load_hlls_repeated_name_last_wins(pkg, client):
    f = pkg.formats
    a, b, c = (f.encode_hll(np.full(M, v, np.uint8)) for v in (1, 2, 40))
    client.load_hlls([("r", a), ("other", b), ("r", c), ("r", b)])
    assert (client.hll_registers("r") == 2).all() and (client.hll_registers("other") == 2).all()
    with pytest.raises(pkg.ResponseError):  # the last string is bad: the last good one stays
        client.load_hlls([("r2", a), ("r2", c), ("r2", b"HYLL" + bytes(20))])
    assert (client.hll_registers("r2") == 40).all()
    client.execute_command("BF.RESERVE", "wasbloom", 0.01, 100)  # SET replaces a key of another type
    client.load_hlls([("wasbloom", a)])
    assert client.type("wasbloom") == "string" and (client.hll_registers("wasbloom") == 1).all()


def test_mset_then_mget(pkg, client):
    f = pkg.formats
    rows = [r for _, r in hc.encode_rows()[1:6]]
    strings = [f.encode_hll(r) for r in rows]
    args = [x for i, s in enumerate(strings) for x in (f"ms{i}", s)]
    assert client.execute_command("MSET", *args) == "OK"
    client.execute_command("BF.RESERVE", "bloom", 0.01, 100)
    got = client.execute_command("MGET", "ms0", "nokey", "ms4", "bloom", "ms2")
    assert got == [strings[0], None, strings[4], None, strings[2]]
    assert [client.execute_command("GET", f"ms{i}") for i in range(5)] == strings
    with pytest.raises(pkg.ResponseError, match="WRONGTYPE Key is not a valid"):
        client.execute_command("MSET", "ms0", strings[1], "junk", "junk")
    assert client.execute_command("GET", "ms0") == strings[1] and client.exists("junk") == 0


def test_save_and_restore_into_a_second_client(pkg, client, tmp_path):
    names, _ = _many_keys(pkg, client, 60, 9)
    client.pfadd("big", *range(3000000, 3006000))
    client.pfadd("skip:me", 1, 2, 3)
    client.execute_command("BF.RESERVE", "bloom", 0.01, 100)
    path = tmp_path / "hll.npz"
    assert client.save_hlls(path) == 62
    every = names + ["big", "skip:me"]
    want = client.pfcount_each(every)
    other = pkg.SketchClient(decode_responses=True, device=0)
    try:
        assert other.restore_hlls(path) == 62
        assert np.array_equal(other.pfcount_each(every), want)
        assert sorted(other.scan_iter()) == sorted(every)
        for n in ("big", names[0], names[59]):
            assert np.array_equal(other.hll_registers(n), client.hll_registers(n))
        other.flushall()
        assert client.save_hlls(path, match="many*") == 60
        assert other.restore_hlls(path) == 60 and other.exists("big", "skip:me") == 0
    finally:
        other.flushall()
    with np.load(path) as z:
        assert sorted(z.files) == ["blob", "name_offs", "names", "offs"]


# ---------------------------------------------------------------- fuzz
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz_strings(pkg, orc, client, seed):
    f = pkg.formats
    from rtsas_amd.engine import SketchEngine
    strings = hc.fuzz_strings(seed, 120)
    sentinel = np.full(M, 9, np.uint8)
    names = [f"fz{i}" for i in range(len(strings))]
    slots = np.asarray([client.key_slot(n) for n in names], np.uint32)
    client.hll_load_registers(names[0], sentinel)
    # every row the sentinel, in one call
    sent = f.encode_hll(sentinel)
    rc, _ = _abi_load(client, slots, [sent] * len(strings))
    assert rc == 0
    rc, status = _abi_load(client, slots, strings)
    want = [hc.expect_decode(f, s) for s in strings]
    assert status == [w[0] for w in want]
    assert rc == (EBADHLL if any(status) else 0) and 30 <= status.count(0) <= 100
    rows = SketchEngine(ctx=client.ctx).registers_all(int(slots.max()) + 1)
    for s, sl, (st, regs) in zip(strings, slots, want):
        if st:
            assert np.array_equal(rows[sl], sentinel)
        else:
            assert np.array_equal(rows[sl], regs) and np.array_equal(rows[sl], orc.hll_decode_string(s))
    # every valid one encoded again on the device is the canonical string of its registers
    valid = [i for i, w in enumerate(want) if w[0] == 0]
    got, _ = _abi_dump(client, slots[valid])
    assert got == [f.encode_hll(want[i][1]) for i in valid]
