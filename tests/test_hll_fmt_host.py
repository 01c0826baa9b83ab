"""The bulk "HYLL" encoder / decoder, the parts that need no GPU: the opcode
rules of csrc/sketch_hll_fmt.h run serially by tests/native/hllfmt_host.cpp (a
stand-alone program that can also be built by hand with ``-fsanitize=address,
undefined``) against ``formats.encode_hll`` / ``formats.decode_hll`` and the
oracle's ``hll_decode_string``; the argument checks that come before any device
call, the constants, the error texts that must not move, MGET / MSET arity, and
what ``dump_hlls`` / ``load_hlls`` make of the native calls (over a context
stub)."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import hllfmt_cases as hc
from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sketch.h")
M = 16384


def test_null_context_is_rejected(pkg):
    lib = pkg.load_library()
    offs = (C.c_uint32 * 2)()
    out = (C.c_uint8 * 64)()
    assert lib.ske_hll_dump_sizes(None, None, 1, 3000, offs, 0) == -1
    assert lib.ske_hll_dump(None, None, 1, 3000, 0, out, 64, offs, 0) == -1
    assert lib.ske_hll_load(None, None, 1, out, offs, None, 0) == -1


def test_constants_match_the_header(pkg):
    from rtsas_amd import _lib
    txt = open(HEADER).read()
    assert re.search(r"#define SKE_HLL_DUMP_MAX_KEYS \(1u << 18\)", txt) and _lib.SKE_HLL_DUMP_MAX_KEYS == 1 << 18
    assert re.search(r"#define SKE_HLL_DUMP_CARD 1\b", txt) and _lib.SKE_HLL_DUMP_CARD == 1
    assert _lib.SKE_HLL_DUMP_MAX_KEYS * (16 + 12288) < 1 << 32  # what lets the offsets be u32


def test_no_new_error_code(pkg):
    from rtsas_amd import _lib
    assert _lib.strerror(-28) == "ERR unknown" and _lib.strerror(-31) == "ERR unknown"
    assert not re.search(r"#define SKE_E\w+ -(28|31)\b", open(HEADER).read())


# ---------------------------------------------------------------- the rules on the host
@pytest.fixture(scope="module")
def fmt_exe(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "hllfmt_host.cpp")
    exe = str(tmp_path_factory.mktemp("hllfmt") / "hllfmt_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-Wall", "-o", exe, src], check=True)
    return exe


def _encode(exe, tmp_path, rows, smb, card=None):
    src, dst = tmp_path / "rows.bin", tmp_path / "strings.bin"
    src.write_bytes(b"".join(np.ascontiguousarray(r, np.uint8).tobytes() for r in rows))
    cmd = [exe, "enc", str(src), str(dst), str(smb)] + ([str(card)] if card is not None else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    data, out, at = dst.read_bytes(), [], 0
    for _ in rows:
        (n,) = struct.unpack_from("<I", data, at)
        out.append(data[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(data)
    return out


def _decode(exe, tmp_path, strings):
    src, dst = tmp_path / "strings.bin", tmp_path / "regs.bin"
    src.write_bytes(struct.pack("<I", len(strings)) + b"".join(struct.pack("<I", len(s)) + s for s in strings))
    p = subprocess.run([exe, "dec", str(src), str(dst)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    data = np.frombuffer(dst.read_bytes(), np.uint8).reshape(len(strings), 1 + M)
    return data[:, 0].tolist(), data[:, 1:]


def test_spans_are_the_headers(fmt_exe):
    out = subprocess.run([fmt_exe, "spans"], capture_output=True, text=True, check=True).stdout
    got = {ln.split()[0]: int(ln.split()[1]) for ln in out.splitlines()}
    assert got == hc.kernel_spans() == {"threads": 256, "span": 64, "wave": 4096}


@pytest.mark.parametrize("smb", [3000, 0, 16384, 40])
def test_encode_patterns(pkg, fmt_exe, tmp_path, smb):
    f = pkg.formats
    cases = hc.encode_rows()
    got = _encode(fmt_exe, tmp_path, [r for _, r in cases], smb)
    for (name, r), s in zip(cases, got):
        assert s == f.encode_hll(r, None, smb), (name, smb)
    if smb == 16384:
        alt = dict(cases)["alternating"]
        assert len(f.sparse_pack(alt)) == M and len(dict(zip([n for n, _ in cases], got))["alternating"]) == 16 + M
    if smb == 0:
        assert all(s[4] == 0 and len(s) == 16 + 12288 for s in got)


def test_encode_promotion_edge(pkg, fmt_exe, tmp_path):
    f = pkg.formats
    rows = hc.promotion_rows()
    assert {k: len(f.sparse_pack(r)) for k, r in rows.items()} == {2999: 2999, 3000: 3000, 3001: 3001}
    for smb in (2998, 2999, 3000, 3001):
        got = _encode(fmt_exe, tmp_path, list(rows.values()), smb)
        for (size, r), s in zip(rows.items(), got):
            assert s == f.encode_hll(r, None, smb), (size, smb)
            assert s[4] == (1 if size <= smb else 0)  # exactly sparse_max_bytes stays sparse, one more goes dense


def test_encode_filled_keys_and_cardinality(pkg, orc, fmt_exe, tmp_path):
    f = pkg.formats
    rows = []
    for n in (1, 10, 300, 3000, 20000):
        h = orc.HLL()
        for i in range(n):
            h.add(str(1000000 + i).encode())
        rows.append(np.asarray(h.regs, np.uint8).copy())
    for card in (None, 0, 12345, (1 << 63) - 1, (1 << 63) + 5):
        got = _encode(fmt_exe, tmp_path, rows, 3000, card)
        for r, s in zip(rows, got):
            assert s == f.encode_hll(r, card, 3000)
            assert f.cached_card(s) == (None if card is None else card & ((1 << 63) - 1))


def _check_decodes(pkg, orc, strings, status, regs):
    f = pkg.formats
    for i, s in enumerate(strings):
        want_st, want = hc.expect_decode(f, s)
        assert status[i] == want_st, (i, s[:24])
        if want_st == 0:
            assert np.array_equal(regs[i], want), i
            assert np.array_equal(regs[i], orc.hll_decode_string(s)), i
        else:
            assert not regs[i].any()


def test_decode_patterns(pkg, orc, fmt_exe, tmp_path):
    good, bad = hc.valid_noncanonical(), hc.corrupt_strings()
    strings = [s for _, s in good + bad]
    status, regs = _decode(fmt_exe, tmp_path, strings)
    assert status[:len(good)] == [0] * len(good)
    assert all(status[len(good):])
    _check_decodes(pkg, orc, strings, status, regs)
    # what the canonical encoder writes decodes back to the rows
    rows = [r for _, r in hc.encode_rows()]
    for smb in (3000, 16384):
        strings = _encode(fmt_exe, tmp_path, rows, smb)
        status, regs = _decode(fmt_exe, tmp_path, strings)
        assert status == [0] * len(rows) and np.array_equal(regs, np.stack(rows))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_decode_fuzz(pkg, orc, fmt_exe, tmp_path, seed):
    f = pkg.formats
    strings = hc.fuzz_strings(seed, 120)
    status, regs = _decode(fmt_exe, tmp_path, strings)
    _check_decodes(pkg, orc, strings, status, regs)
    valid = [i for i, st in enumerate(status) if st == 0]
    assert len(valid) >= 40 and len(valid) <= 100  # both kinds are in the set
    again = _encode(fmt_exe, tmp_path, [regs[i] for i in valid], 3000)
    for i, s in zip(valid, again):
        assert s == f.encode_hll(regs[i], None, 3000)


# ---------------------------------------------------------------- the facade over a stub
@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def _u32(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), (n,))


def _u8(p, n):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (n,))


def _dump_hooks(ctx, seen):
    """the device's side of a dump: slot s holds the string b"S<s>" * (s + 1)"""
    def string(s):
        return (b"S%d" % s) * (s + 1)

    def sizes(slots, n, smb, offs, mem):
        sl = _u32(slots, n)
        _u32(offs, n + 1)[1:] = np.cumsum([len(string(int(s))) for s in sl])

    def dump(slots, n, smb, flags, out, cap, offs, mem):
        sl = _u32(slots, n).tolist()
        seen.append((sl, smb, flags))
        data = b"".join(string(s) for s in sl)
        assert cap == len(data)
        _u8(out, cap)[:] = np.frombuffer(data, np.uint8)
        _u32(offs, n + 1)[1:] = np.cumsum([len(string(s)) for s in sl])
    ctx.hooks["ske_hll_dump_sizes"], ctx.hooks["ske_hll_dump"] = sizes, dump
    return string


def test_mget_mset_arity(pkg, stub_client):
    cl, ctx = stub_client
    for cmd in (("MGET",), ("MSET",), ("MSET", "k"), ("MSET", "k", "v", "k2")):
        with pytest.raises(pkg.ResponseError, match=f"wrong number of arguments for '{cmd[0].lower()}' command"):
            cl.execute_command(*cmd)
    assert ctx.calls == []


def test_dump_hlls_chunks_and_missing_keys(pkg, stub_client):
    cl, ctx = stub_client
    names = [f"k{i}" for i in range(7)]
    for n in names:
        cl.pfadd(n)
    cl.execute_command("BF.RESERVE", "bloom", 0.01, 100)
    seen = []
    string = _dump_hooks(ctx, seen)
    ctx.log.clear()
    want = [string(cl.keys.slot[n.encode()]) for n in names]
    got = cl.dump_hlls(["nokey"] + names + [names[2]], chunk_keys=3, with_card=True, sparse_max_bytes=77)
    assert got == [None] + want + [want[2]]
    assert [len(s[0]) for s in seen] == [3, 3, 2] and all(s[1:] == (77, 1) for s in seen)
    assert [c[0] for c in ctx.log] == ["ske_hll_dump_sizes", "ske_hll_dump"] * 3
    seen.clear()
    assert cl.dump_hlls(names) == want and [len(s[0]) for s in seen] == [7] and seen[0][1:] == (3000, 0)
    assert cl.dump_hlls([]) == [] and cl.dump_hlls(["nokey"]) == [None]
    with pytest.raises(pkg.ResponseError, match="WRONGTYPE"):
        cl.dump_hlls([names[0], "bloom"])
    # MGET: None for a missing key and for a key that is no string
    assert cl.execute_command("MGET", names[1], "nokey", "bloom", names[0]) == [want[1], None, None, want[0]]


def test_load_hlls_dedup_chunks_and_errors(pkg, stub_client):
    cl, ctx = stub_client
    f = pkg.formats
    good = [f.encode_hll(np.full(M, v, np.uint8)) for v in range(1, 6)]
    bad_magic, corrupt = b"not an hll string", hc.hyll(b"\x00")
    calls = []

    def load(slots, n, blob, offs, status, mem):
        sl, o = _u32(slots, n).tolist(), _u32(offs, n + 1).tolist()
        data = bytes(_u8(blob, o[-1])) if o[-1] else b""
        strings = [data[o[i]:o[i + 1]] for i in range(n)]
        calls.append(list(zip(sl, strings)))
        st = [hc.expect_decode(f, s)[0] for s in strings]
        _u8(status, n)[:] = st
        if any(st):
            raise pkg.SketchLibError(-11, "INVALIDOBJ Corrupted HLL object detected")
    ctx.hooks["ske_hll_load"] = load
    cl.pfadd("old")
    cl.execute_command("BF.RESERVE", "bloom", 0.01, 100)
    cl.execute_command("BF.RESERVE", "bloom2", 0.01, 100)
    old_slot = cl.keys.slot[b"old"]
    # a repeated name: one string goes to the device, the last
    cl.load_hlls([("a", good[0]), ("b", good[1]), ("a", good[2]), ("old", good[3]), ("bloom", good[4])], chunk_keys=2)
    assert [len(c) for c in calls] == [2, 2]
    sent = dict(x for c in calls for x in c)
    assert len(sent) == 4 and len(set(sent)) == 4  # distinct slots
    assert sent[cl.keys.slot[b"a"]] == good[2] and sent[cl.keys.slot[b"b"]] == good[1]
    assert sent[old_slot] == good[3] and cl.keys.kind[b"bloom"] == "hll" and sent[cl.keys.slot[b"bloom"]] == good[4]
    assert "ske_bf_free" in ctx.calls  # SET replaced the Bloom key
    # bad strings: the good pairs are in, the first bad pair's error is raised, its name is not created
    calls.clear()
    before = dict(cl.keys.kind)
    with pytest.raises(pkg.ResponseError, match="INVALIDOBJ"):
        cl.load_hlls([("c", good[0]), ("new1", corrupt), ("new2", bad_magic), ("a", bad_magic), ("d", good[1]),
                      ("bloom2", bad_magic), ("e", good[2]), ("e", corrupt)])
    assert set(cl.keys.kind) == set(before) | {"c".encode(), b"d", b"e"} and cl.keys.kind[b"bloom2"] == "bf"
    loaded = {s: v for c in calls for s, v in c if hc.expect_decode(f, v)[0] == 0}
    assert loaded == {cl.keys.slot[b"c"]: good[0], cl.keys.slot[b"d"]: good[1], cl.keys.slot[b"e"]: good[2]}
    assert len(calls) == 2 and len(calls[1]) == 1  # the second round: e's earlier, good string
    with pytest.raises(pkg.ResponseError, match="WRONGTYPE Key is not a valid HyperLogLog"):
        cl.load_hlls([("new3", bad_magic), ("new4", corrupt)])
    assert b"new3" not in cl.keys.kind and b"new4" not in cl.keys.kind
    # a freed name's slot is handed out again: nothing leaked
    free_before = len(cl.keys._free_slots)
    with pytest.raises(pkg.ResponseError):
        cl.load_hlls([("new5", corrupt)])
    assert len(cl.keys._free_slots) == free_before
    calls.clear()
    cl.load_hlls([])
    assert calls == []
    # MSET runs over the same method
    assert cl.execute_command("MSET", "m1", good[0], "m2", good[1]) == "OK"
    assert [len(c) for c in calls] == [2] and cl.keys.kind[b"m1"] == cl.keys.kind[b"m2"] == "hll"
