"""Seen-row sets, the parts that need no GPU: the fold, the bucket floor
division, the 0-to-1 remap and the limit arithmetic of sketch_common.h (a
stand-alone program, tests/native/seen_host.cpp, built with ``-Xarch_host
-fsanitize=address,undefined``) against ``keyhash.murmur64a``, the oracle's
MurmurHash64A and the Python restatement ``client_seen.seen_row_keys``; the
error texts and constants; and over a context stub: the facade's registry of
named sets, ``FLUSHALL``, and what ``StudentCounts(dedup=...)`` asks of its
callers."""
import os
import re
import subprocess

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (0, 1, 7, 8, 9, 15, 16)
EPOCHS = (-1, 0, 86399, 86400, -86401)
GRANULARITIES = (1, 86400)


@pytest.fixture(scope="module")
def seen_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "seen_host.cpp")
    exe = str(tmp_path_factory.mktemp("seen") / "seen_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "runtime error" not in out.stderr, out.stderr
        return out.stdout.splitlines()
    return run


def column(n: int, salt: int) -> bytes:
    return bytes((salt * 37 + 11 * j + 1) & 0xFF for j in range(n))


def test_fold_words(pkg, seen_host, orc):
    from rtsas_amd import client_seen as cs
    from rtsas_amd.keyhash import murmur64a
    cols = [column(n, s) for s in (1, 2) for n in LENGTHS] + [bytes(8), bytes(16), b"\xff" * 16]
    lines = seen_host("fold", *[c.hex() or "-" for c in cols])
    assert len(lines) == len(cols)
    k = (cs.SEEN_SEED0, cs.SEEN_SEED1)
    assert k[0] != k[1] and 0xC6A4A7935BD1E995 not in k  # two seeds, neither is kBloomSeed
    for c, line in zip(cols, lines):
        k = (murmur64a(c, k[0]), murmur64a(c, k[1]))
        assert line == f"{k[0]} {k[1]}", (c, line)
    # keyhash.murmur64a against the oracle's, over the same columns and both seeds
    for c in cols:
        for seed in (cs.SEEN_SEED0, cs.SEEN_SEED1):
            assert murmur64a(c, seed) == orc.murmur64a(c, seed)
    # the fold is one murmur per word and column, in order: not commutative
    a, b = column(7, 5), column(9, 6)
    assert seen_host("fold", a.hex(), b.hex())[-1] != seen_host("fold", b.hex(), a.hex())[-1]
    assert cs.seen_fold([(cs.SEEN_SEED0, cs.SEEN_SEED1)], [a]) == \
        [tuple(int(x) for x in seen_host("fold", a.hex())[0].split())]


def test_bucket_floor_and_epoch_fold(pkg, seen_host):
    from rtsas_amd import client_seen as cs
    from rtsas_amd.keyhash import murmur64a
    for g in GRANULARITIES:
        lines = seen_host("epoch", g, *EPOCHS)
        for e, line in zip(EPOCHS, lines):
            bucket = e // g  # Python's floor division
            col = bucket.to_bytes(8, "little", signed=True)
            assert line == f"{bucket} {murmur64a(col, cs.SEEN_SEED0)} {murmur64a(col, cs.SEEN_SEED1)}", (g, e, line)
    assert [int(x.split()[0]) for x in seen_host("epoch", 86400, *EPOCHS)] == [-1, 0, 0, 1, -2]
    # the extremes of int64 do not overflow the correction
    lo, hi = -2 ** 63, 2 ** 63 - 1
    assert [int(x.split()[0]) for x in seen_host("epoch", 86400, lo, hi)] == [lo // 86400, hi // 86400]
    assert [int(x.split()[0]) for x in seen_host("epoch", 1, lo, hi)] == [lo, hi]


def test_row_keys_restatement(pkg, seen_host):
    """``seen_row_keys`` is the three folds in order, then the remap: checked
    against the stand-alone program's fold over the same columns."""
    from rtsas_amd import client_seen as cs
    ids = [12345, "x", "abcdefghijklmnop", 7]
    lectures = ["CS101-L01", "", "L" * 16, 42]
    for g in GRANULARITIES:
        times = np.asarray([-1, 0, 86399, -86401], np.int64)
        got = cs.seen_row_keys(ids, times, lectures, g)
        assert got.shape == (4, 2) and got.dtype == np.uint64
        for i in range(4):
            cols = [str(lectures[i]).encode(), str(ids[i]).encode(),
                    (int(times[i]) // g).to_bytes(8, "little", signed=True)]
            last = seen_host("fold", *[c.hex() or "-" for c in cols])[-1]
            assert [int(x) for x in last.split()] == [int(got[i, 0]), int(got[i, 1])]
    with pytest.raises(ValueError):
        cs.seen_row_keys(ids, np.zeros(4, np.int64), lectures, 0)
    with pytest.raises(ValueError):
        cs.seen_row_keys(ids, np.zeros(3, np.int64), lectures, 1)


def test_word_remap_and_limit(seen_host):
    assert seen_host("word", 0, 1, 2, 2 ** 64 - 1) == ["1", "1", "2", str(2 ** 64 - 1)]
    assert seen_host("limit", 1, 10, 30) == ["2 1 1", "1024 512 1023", f"{2 ** 30} {2 ** 29} {2 ** 30 - 1}"]


def test_error_texts_and_constants(pkg):
    from rtsas_amd import _lib
    want = {-37: ("SKE_ESEENNOSET", "ERR seen set does not exist"),
            -38: ("SKE_ESEENEXISTS", "ERR seen set already exists"),
            -39: ("SKE_ESEENCAP", "ERR seen set capacity out of range"),
            -40: ("SKE_ESEENCALLS", "ERR seen set has run out of call numbers")}
    txt = open(_lib.HEADER_PATH).read()
    for code, (name, text) in want.items():
        assert getattr(_lib, name) == code and _lib.strerror(code) == text
        assert re.search(rf"#define {name} {code}\b", txt), name
    assert _lib.strerror(-36) == "ERR unknown" and _lib.strerror(-41) == "ERR unknown"
    consts = {"SKE_MAX_SEEN": 256, "SKE_SEEN_MIN_LOG2": 8, "SKE_SEEN_MAX_LOG2": 30, "SKE_SEEN_MAX_PROBES": 128,
              "SKE_SEEN_LOAD_DEN": 2, "SKE_SEEN_FIRST": 0, "SKE_SEEN_REPEAT": 1, "SKE_SEEN_SKIPPED": 2}
    for name, value in consts.items():
        m = re.search(rf"#define {name} (\d+)", txt)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    import ctypes as C
    assert C.sizeof(_lib.SeenInfo) == 56


def test_argument_checks_before_any_device_call(pkg):
    lib = pkg.load_library()
    assert lib.ske_seen_init(None, 0, 10) == -1
    assert lib.ske_seen_free(None, 0) == -1 and lib.ske_seen_reset(None, 0) == -1
    assert lib.ske_seen_info(None, 0, None) == -1
    assert lib.ske_seen_add_async(None, 0, None, 0, None, 0, None) == -1
    assert lib.ske_seen_test_async(None, 0, None, 0, None) == -1
    assert lib.ske_seen_fold_epoch_async(None, None, None, 1, 0, 1) == -1


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
    return cl, ctx


def test_registry_and_flushall(pkg, stub_client):
    cl, ctx = stub_client
    ctx.log.clear()
    sid = cl.seen_create("rows", 10)
    assert ctx.log == [["ske_seen_init", sid, 10]] and cl.seen_sid("rows") == sid
    with pytest.raises(pkg.ResponseError, match="already exists"):
        cl.seen_create("rows", 10)
    for bad in (7, 31):
        with pytest.raises(pkg.ResponseError, match="capacity out of range"):
            cl.seen_create("other", bad)
    with pytest.raises(pkg.ResponseError, match="does not exist"):
        cl.seen_info("nope")
    other = cl.seen_create(b"other")
    assert other != sid and ctx.log[-1] == ["ske_seen_init", other, 22]
    assert cl.exists("rows") == 0 and cl.type("rows") == "none"  # no Redis key
    assert cl.seen_drop("other") and not cl.seen_drop("other")
    assert cl.seen_create("again", 8) == other  # the id is free again
    ctx.log.clear()
    cl.flushall()
    assert sorted(c for c in ctx.log if c[0] == "ske_seen_free") == [["ske_seen_free", sid], ["ske_seen_free", other]]
    assert not cl._seen
    ctx.log.clear()
    cl.flushall()
    assert not [c for c in ctx.log if c[0].startswith("ske_seen")]


def test_student_counts_dedup_options(pkg, stub_client):
    cl, ctx = stub_client
    plain = pkg.StudentCounts(cl)
    assert not plain.dedup and not plain.needs_times and not plain.needs_lectures
    with pytest.raises(ValueError):
        plain.duplicate_rows()
    ctx.log.clear()
    sc = pkg.StudentCounts(cl, attended_key="a2", invalid_key="i2", dedup="seen:rows", dedup_capacity_log2=12,
                           dedup_granularity=86400)
    assert ["ske_seen_init", cl.seen_sid("seen:rows"), 12] in ctx.log
    assert sc.dedup and sc.needs_times and sc.needs_lectures
    assert not sc.timed and not sc.counts_lectures  # no profile, no tally: their meaning is kept
    # an existing set is taken as it is
    ctx.log.clear()
    pkg.StudentCounts(cl, attended_key="a3", invalid_key="i3", dedup="seen:rows")
    assert not [c for c in ctx.log if c[0] == "ske_seen_init"]
    with pytest.raises(ValueError):
        pkg.StudentCounts(cl, attended_key="a4", invalid_key="i4", dedup="s", dedup_granularity=0)
    ids = np.frombuffer(b"1234", np.uint8).reshape(1, 4)
    with pytest.raises(ValueError):  # the row key needs the time and the lecture
        sc.update("bf", np.zeros(1, np.uint32), ids)
    with pytest.raises(ValueError):
        sc.update("bf", np.zeros(1, np.uint32), ids, times=[0])
    with pytest.raises(ValueError):
        sc.count_packed(np.zeros(4, np.uint8), np.asarray([0, 4], np.uint32), [1], lectures=["L"])
    with pytest.raises(ValueError):  # and without dedup both stay refused
        plain.count_packed(np.zeros(4, np.uint8), np.asarray([0, 4], np.uint32), [1], times=[0])


def test_take_packed(pkg):
    buf = np.frombuffer(b"xxaabbbcdddd", np.uint8)
    offs = np.asarray([2, 4, 7, 7, 8, 12], np.uint32)  # "aa", "bbb", "", "c", "dddd"; offs[0] is not 0
    keep = np.asarray([True, False, True, False, True])
    got, goffs = pkg.StudentCounts._take_packed(buf, offs, keep)
    assert got.tobytes() == b"aadddd" and goffs.tolist() == [0, 2, 2, 6]
    got, goffs = pkg.StudentCounts._take_packed(buf, offs, np.zeros(5, bool))
    assert got.size == 0 and goffs.tolist() == [0]
