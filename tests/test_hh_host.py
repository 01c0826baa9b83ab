"""Heavy-hitter sets, the parts that need no GPU: the digest and start-slot
arithmetic of sketch_common.h (a stand-alone program, tests/native/hh_host.cpp,
which can also be built by hand with ``-Xarch_host
-fsanitize=address,undefined``), the argument checks that come before any
device call, the error texts, and the facade's registry of live sets (over a
context stub): DEL and FLUSHALL free the bound sets, and make no further native
call while there is none."""
import ctypes as C
import os
import subprocess

import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOOM_SEED = 0xC6A4A7935BD1E995


def test_hh_host_arith(tmp_path, orc):
    src = os.path.join(ROOT, "tests", "native", "hh_host.cpp")
    exe = str(tmp_path / "hh_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)
    ids = [b"", bytes(8), bytes(16), bytes(1), b"12345", b"20251003", b"\xff" * 16, b"abcdefghi"]
    ids += [bytes((7 * i + j) & 0xFF for j in range(n)) for n in range(1, 17) for i in (1, 29)]
    # digest 0 does occur: the seed is the multiplier, so one zero byte hashes to 0
    assert orc.murmur64a(bytes(1), BLOOM_SEED) == 0 and ids[3] == bytes(1)
    for log2 in (8, 18, 24):
        out = subprocess.run([exe, str(log2)] + [i.hex() or "-" for i in ids], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        lines = out.stdout.splitlines()
        assert len(lines) == len(ids)
        for i, line in zip(ids, lines):
            digest = orc.murmur64a(i, BLOOM_SEED) or 1
            assert line == f"{i.hex() or '-'} {digest} {digest & ((1 << log2) - 1)}", (i, line)
        assert lines[3] == "00 1 1"


def test_hh_error_texts(pkg):
    from rtsas_amd import _lib
    want = {_lib.SKE_EHHNOSET: "ERR heavy-hitter set does not exist",
            _lib.SKE_EHHEXISTS: "ERR heavy-hitter set already exists",
            _lib.SKE_EHHCAP: "ERR heavy-hitter capacity out of range",
            _lib.SKE_EHHSPACE: "ERR heavy-hitter list does not fit the output"}
    assert sorted(want) == [-27, -26, -25, -24]
    for code, text in want.items():
        assert _lib.strerror(code) == text
    assert _lib.strerror(-23) == "CMS: Cannot parse number" and _lib.strerror(-28) == "ERR unknown"


def test_null_context_is_rejected(pkg):
    lib = pkg.load_library()
    n, done = C.c_uint64(), C.c_int()
    assert lib.ske_hh_init(None, 0, 10) == -1
    assert lib.ske_hh_free(None, 0) == -1
    assert lib.ske_hh_reset(None, 0) == -1
    assert lib.ske_hh_info(None, 0, None) == -1
    assert lib.ske_hh_track_fixed_async(None, 0, 0, None, 8, 0, None, 1, 1) == -1
    assert lib.ske_hh_track(None, 0, 0, None, None, 0, 1, 0) == -1
    assert lib.ske_hh_list(None, 0, 0, 1, None, None, None, 0, C.byref(n), C.byref(done)) == -1


def test_constants_match_the_header(pkg):
    import re
    from rtsas_amd import _lib
    txt = open(_lib.HEADER_PATH).read()
    for name in ("SKE_MAX_HH", "SKE_HH_MIN_LOG2", "SKE_HH_MAX_LOG2", "SKE_HH_ID_BYTES", "SKE_HH_MAX_PROBES",
                 "SKE_HH_LOAD_DEN", "SKE_EHHNOSET", "SKE_EHHEXISTS", "SKE_EHHCAP", "SKE_EHHSPACE"):
        m = re.search(rf"#define {name} (-?\d+)", txt)
        assert m and int(m.group(1)) == getattr(_lib, name), name


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def test_del_and_flushall_without_sets(pkg, stub_client):
    cl, ctx = stub_client
    ex = cl.execute_command
    ex("CMS.INITBYDIM", "c", 100, 5)
    ex("CMS.INITBYDIM", "c2", 100, 5)
    ex("PFADD", "h", "a")
    ctx.calls.clear()
    assert ex("DEL", "c", "nokey") == 1
    assert ctx.calls == ["ske_cms_free"]
    ctx.calls.clear()
    assert ex("FLUSHALL") == "OK"
    assert sorted(ctx.calls) == ["ske_cms_free", "ske_hll_clear"]
    assert not any("hh" in c for c in ctx.calls)


def test_registry_frees_bound_sets(pkg, stub_client):
    cl, ctx = stub_client
    ex = cl.execute_command
    for key in ("c", "c2", "c3"):
        ex("CMS.INITBYDIM", key, 100, 5)
    ctx.calls.clear()
    ctx.log.clear()
    a = cl.hh_create("top:c", "c", 10)
    b = cl.hh_create("top:c:b", "c", 12)
    d = cl.hh_create("top:c2", "c2")
    assert len({a, b, d}) == 3 and ctx.calls == ["ske_hh_init"] * 3
    assert ctx.log[0] == ["ske_hh_init", a, 10] and ctx.log[2] == ["ske_hh_init", d, 16]
    # what the facade refuses on its own
    for args, text in ((("top:c", "c"), "ERR heavy-hitter set already exists"),
                       (("x", "nokey"), "CMS: key does not exist"),
                       (("x", "c", 7), "ERR heavy-hitter capacity out of range"),
                       (("x", "c", 25), "ERR heavy-hitter capacity out of range")):
        with pytest.raises(pkg.ResponseError) as e:
            cl.hh_create(*args)
        assert str(e.value) == text
    ex("PFADD", "h", "a")
    with pytest.raises(pkg.ResponseError, match="WRONGTYPE"):
        cl.hh_create("x", "h")
    with pytest.raises(pkg.ResponseError, match="ERR heavy-hitter set does not exist"):
        cl.hh_info("nosuch")
    assert ctx.calls.count("ske_hh_init") == 3
    # DEL of a key without sets: no hh call; of the bound key: its sets go first
    ctx.calls.clear()
    assert ex("DEL", "c3") == 1 and ctx.calls == ["ske_cms_free"]
    ctx.log.clear()
    assert ex("DEL", "c") == 1
    assert sorted(ctx.log[:2]) == sorted([["ske_hh_free", a], ["ske_hh_free", b]])
    assert [c[0] for c in ctx.log] == ["ske_hh_free", "ske_hh_free", "ske_cms_free"]
    with pytest.raises(pkg.ResponseError, match="ERR heavy-hitter set does not exist"):
        cl.hh_list("top:c", 1)
    # a freed id is handed out again; FLUSHALL frees what is left
    ex("CMS.INITBYDIM", "c", 100, 5)
    assert cl.hh_create("again", "c", 10) in (a, b)
    ctx.log.clear()
    assert ex("FLUSHALL") == "OK"
    assert sorted(c[0] for c in ctx.log if "hh" in c[0]) == ["ske_hh_free", "ske_hh_free"]
    assert cl._hh == {} and len(cl._hh_free_ids) == 256
    ctx.calls.clear()
    assert ex("FLUSHALL") == "OK" and ctx.calls == []
    assert cl.hh_free("again") is False


def test_student_counts_off_by_default(pkg, stub_client):
    """without track thresholds update() makes the native calls it made before"""
    import numpy as np
    cl, ctx = stub_client
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    ids = np.full((4, 5), 49, np.uint8)
    slots = np.zeros(4, np.uint32)
    plain = pkg.StudentCounts(cl)
    ctx.calls.clear()
    plain.update("bf", slots, ids)
    base = [c for c in ctx.calls if c not in ("ske_device_alloc", "ske_memcpy")]
    assert base == ["ske_swipes_fixed", "ske_cms_add_fixed_async", "ske_cms_add_fixed_async", "ske_sync"]
    with pytest.raises(ValueError):
        plain.top_invalid()
    assert plain.insights() == []
    tracked = pkg.StudentCounts(cl, "a2", "i2", track_attended=3, track_invalid=2, capacity_log2=12)
    ctx.calls.clear()
    ctx.log.clear()
    tracked.update("bf", slots, ids)
    got = [c for c in ctx.log if c[0] not in ("ske_device_alloc", "ske_memcpy")]
    assert [c[0] for c in got] == base[:3] + ["ske_hh_track_fixed_async"] * 2 + ["ske_sync"]
    assert got[3][5:] == [4, "*", 1, 3] and got[4][5:] == [4, "*", 0, 2]  # n, mask, want, threshold
    with pytest.raises(ValueError):
        tracked.top_invalid(threshold=1)  # below the track threshold
