"""Count-Min Sketch, the parts that need no GPU: the 32-bit MurmurHash2 and the
cell arithmetic of sketch_common.h (a stand-alone program, tests/native/
cms_host.cpp, which can also be built by hand with
``-Xarch_host -fsanitize=address,undefined``), CMS.INITBYPROB's dimensions,
the error texts, and the facade's argument errors (raised before any device
call: the client here runs over a context stub)."""
import ctypes as C
import os
import subprocess

import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cms_host_arith(tmp_path):
    src = os.path.join(ROOT, "tests", "native", "cms_host.cpp")
    exe = str(tmp_path / "cms_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bad=0" in out.stdout
    assert "smhasher verification 0x27864C1E" in out.stdout
    for r, c in enumerate((18, 136, 1146, 1175)):
        assert f"12345 row {r} cell {c}\n" in out.stdout


def _dims(lib, error, prob):
    w, d = C.c_uint32(0), C.c_uint32(0)
    rc = lib.ske_cms_dims_from_prob(error, prob, C.byref(w), C.byref(d))
    return rc, w.value, d.value


def test_dims_from_prob(pkg):
    from rtsas_amd import _lib
    lib = pkg.load_library()
    assert _dims(lib, 0.001, 0.01) == (0, 2000, 7)
    assert _dims(lib, 0.01, 0.001) == (0, 200, 10)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        assert _dims(lib, bad, 0.01)[0] == _lib.SKE_ECMSERROR
        assert _dims(lib, 0.01, bad)[0] == _lib.SKE_ECMSPROB
    assert lib.ske_cms_dims_from_prob(0.01, 0.01, None, None) == _lib.SKE_EINVAL


def test_cms_error_texts(pkg):
    from rtsas_amd import _lib
    want = {-14: "CMS: key does not exist", -15: "CMS: key already exists", -16: "CMS: invalid width",
            -17: "CMS: invalid depth", -18: "CMS: width/depth is not equal",
            -19: "CMS: Number cannot be negative", -20: "CMS: MERGE overflow"}
    for code, text in want.items():
        assert _lib.strerror(code) == text
    assert _lib.strerror(-13) == "ERR device buffers in use by a recorded graph"


def test_null_context_is_rejected(pkg):
    lib = pkg.load_library()
    assert lib.ske_cms_init(None, 0, 10, 2) == -1
    assert lib.ske_cms_free(None, 0) == -1
    assert lib.ske_cms_info(None, 0, None) == -1
    assert lib.ske_cms_incrby(None, 0, None, None, 0, None, None, 0) == -1
    assert lib.ske_cms_add_fixed_async(None, 0, None, 8, 0, None, None, 1) == -1
    assert lib.ske_cms_query(None, 0, None, None, 0, None, 0) == -1
    assert lib.ske_cms_merge(None, 0, None, None, 0) == -1
    assert lib.ske_cms_export(None, 0, None, 0) == -1
    assert lib.ske_cms_import(None, 0, None, 0, 0) == -1


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def _raises(pkg, text, fn, *args):
    with pytest.raises(pkg.ResponseError) as e:
        fn(*args)
    assert str(e.value) == text, str(e.value)


def test_facade_argument_errors(pkg, stub_client):
    cl, ctx = stub_client
    ex = cl.execute_command
    for w in (0, -1, "abc", 2 ** 32, 1.5):
        _raises(pkg, "CMS: invalid width", ex, "CMS.INITBYDIM", "k", w, 5)
    for d in (0, -3, "x", 2 ** 32):
        _raises(pkg, "CMS: invalid depth", ex, "CMS.INITBYDIM", "k", 100, d)
    for e in (0, 1, 1.5, "no"):
        _raises(pkg, "CMS: invalid overestimation value", ex, "CMS.INITBYPROB", "k", e, 0.01)
        _raises(pkg, "CMS: invalid prob value", ex, "CMS.INITBYPROB", "k", 0.01, e)
    for cmd in (("CMS.INCRBY", "k", "a", 1), ("CMS.QUERY", "k", "a"), ("CMS.INFO", "k"),
                ("CMS.MERGE", "k", 1, "k")):
        _raises(pkg, "CMS: key does not exist", ex, *cmd)
    for cmd in (("CMS.INITBYDIM", "k", 5), ("CMS.INITBYDIM", "k", 5, 5, 5), ("CMS.INITBYPROB", "k", 0.1),
                ("CMS.INCRBY", "k", "a"), ("CMS.INCRBY", "k", "a", 1, "b"), ("CMS.QUERY", "k"),
                ("CMS.INFO",), ("CMS.MERGE", "k", 1), ("CMS.MERGE", "k", 2, "a")):
        _raises(pkg, f"ERR wrong number of arguments for '{cmd[0].lower()}' command", ex, *cmd)
    assert ctx.calls == []  # none of the above reached the device

    assert ex("CMS.INITBYDIM", "k", 100, 5) == "OK"
    assert ctx.calls == ["ske_cms_init"]
    assert ex("TYPE", "k") == "CMSk-TYPE" and ex("EXISTS", "k") == 1
    assert list(cl.scan_iter(_type="CMSk-TYPE")) == ["k"]
    _raises(pkg, "CMS: key already exists", ex, "CMS.INITBYDIM", "k", 100, 5)
    _raises(pkg, "CMS: key already exists", ex, "CMS.INITBYPROB", "k", 0.01, 0.01)
    _raises(pkg, "CMS: Number cannot be negative", ex, "CMS.INCRBY", "k", "a", -1)
    _raises(pkg, "CMS: Cannot parse number", ex, "CMS.INCRBY", "k", "a", "one")
    _raises(pkg, "CMS: Cannot parse number", ex, "CMS.INCRBY", "k", "a", 2 ** 32)
    _raises(pkg, "CMS: key does not exist", ex, "CMS.MERGE", "k", 2, "k", "other")
    _raises(pkg, "ERR wrong number of arguments for 'cms.merge' command", ex, "CMS.MERGE", "k", 1, "k",
            "WEIGHTS", 1, 2)
    _raises(pkg, "CMS: Cannot parse number", ex, "CMS.MERGE", "k", 1, "k", "WEIGHTS", "w")
    assert ctx.calls == ["ske_cms_init"]
    # a key of another kind
    wrongtype = "WRONGTYPE Operation against a key holding the wrong kind of value"
    _raises(pkg, wrongtype, ex, "BF.EXISTS", "k", "a")
    _raises(pkg, wrongtype, ex, "PFCOUNT", "k")
    _raises(pkg, wrongtype, ex, "GET", "k")
    assert ex("DEL", "k") == 1 and ctx.calls[-1] == "ske_cms_free"
    assert ex("TYPE", "k") == "none"
