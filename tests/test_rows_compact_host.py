"""Row log compaction, the parts that need no GPU: ``rows_compact_oracle``
against a pandas expression written here; the counts and the head's update of
sketch_rows_compact.h (a stand-alone program, tests/native/rowscompact_host.cpp,
built with ``-Xarch_host -fsanitize=address,undefined``) against the rule in
Python; the struct; and over a context stub what ``rows_compact``,
``compact_records`` and ``StudentCounts(records_compact=True)`` call and when."""
import ctypes as C
import os
import re
import subprocess
from datetime import datetime

import numpy as np
import pytest

from facade_stub import StubContext
from rows_compact_cases import LECTURES, Rows, patterned, wild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def pandas_compact(log, keep_since):
    """drop epoch < keep_since, then keep each (lec, epoch, id)'s last row, the index order preserved"""
    import pandas as pd
    df = pd.DataFrame({"lec": log[0], "epoch": log[1], "id": log[2], "valid": log[3]})
    lo = I64_MIN if keep_since is None else keep_since
    live = df[df["epoch"] >= lo]
    out = live.drop_duplicates(["lec", "epoch", "id"], keep="last").sort_index()
    return out, len(df) - len(live), len(live) - len(out)


def check_oracle(pkg, log, keep_since):
    from rtsas_amd.client_rows import rows_compact_oracle
    got = rows_compact_oracle(log, keep_since)
    want, expired, superseded = pandas_compact(log, keep_since)
    assert (got["kept"], got["superseded"], got["expired"]) == (len(want), superseded, expired)
    assert got["kept"] + got["superseded"] + got["expired"] == len(log[0])
    for col, name, dtype in zip(got["log"], ("lec", "epoch", "id", "valid"), (np.uint64, np.int64, np.int64, np.uint8)):
        assert col.dtype == dtype and np.array_equal(col, want[name].to_numpy()), (name, keep_since)
    return got


def test_oracle_against_pandas_random(pkg):
    for seed, n in enumerate((0, 1, 2, 64, 257, 1500)):
        rng = np.random.default_rng(seed)
        ids, _ = wild(rng.integers(0, max(n // 64, 1), n))
        rows = Rows([LECTURES[j] for j in rng.integers(0, len(LECTURES), n)], ids, rng.integers(-4, 4, n),
                    rng.integers(0, 2, n))
        for keep_since in (None, I64_MIN, -4, -2, 0, 3, 4, I64_MAX):
            got = check_oracle(pkg, rows.log(), keep_since)
            if n == 1500 and keep_since == -2:
                assert got["superseded"] > 100 and got["expired"] > 100 and got["kept"] > 100


def test_oracle_against_pandas_edges(pkg):
    n = 2 * 256 + 17
    i = np.arange(n)
    keeps = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": i % 2 == 1,
             "one_per_wave": i % 64 == 37, "first": i == 0, "last": i == n - 1}
    for kind, keep in keeps.items():
        rows = patterned(keep, -70000, seed=3)
        got = check_oracle(pkg, rows.log(), -70000)
        assert got["kept"] == int(keep.sum()), kind
        assert check_oracle(pkg, rows.log(), int(rows.ep.max()) + 1)["kept"] == 0
    # one row written 600 times: the last write's byte stays
    rows = Rows([b"r"] * 600 + [b"o"], [77] * 600 + [78], [5] * 601, [j % 2 for j in range(600)] + [0])
    got = check_oracle(pkg, rows.log(), None)
    assert got["log"][3].tolist() == [1, 0] and got["superseded"] == 599
    # extreme ids and negative epochs; a superseded row below the cutoff is expired
    rows = Rows([b"a"] * 8, [I64_MIN, I64_MAX, 7, 7, 8, 7, 8, 9], [-9, -9, -1, -1, 0, 0, 0, -1], [1, 0, 0, 1, 0, 1, 1, 1])
    assert check_oracle(pkg, rows.log(), None)["kept"] == 6
    got = check_oracle(pkg, rows.log(), 0)
    assert (got["kept"], got["superseded"], got["expired"]) == (2, 1, 5) and got["log"][2].tolist() == [7, 8]
    got = check_oracle(pkg, rows.log(), -1)  # rows at keep_since stay, rows at keep_since - 1 go
    assert got["log"][1].tolist() == [-1, 0, 0, -1] and got["expired"] == 2


def test_struct_matches_the_header(pkg):
    from rtsas_amd import _lib
    assert C.sizeof(_lib.RowsCompact) == 32
    txt = open(_lib.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ske_rows_compact_t;", txt).group(1)
    fields = re.findall(r"uint64_t (\w+);", body)
    assert fields == [f for f, _ in _lib.RowsCompact._fields_] == ["before", "kept", "superseded", "expired"]
    assert all(t is C.c_uint64 for _, t in _lib.RowsCompact._fields_)
    assert re.search(r"int ske_rows_compact\(ske_ctx \*ctx, uint32_t rid, int64_t keep_since, ske_rows_compact_t \*out\);",
                     txt)
    assert "ske_rows_compact" not in txt.split("---- stream capture")[1]  # it waits for the stream: not capturable
    assert C.sizeof(_lib.RowsInfo) == 48 and _lib.strerror(-46) == "ERR unknown"  # no new field, no new code
    lib = pkg.load_library()
    assert lib.ske_rows_compact(None, 0, 0, None) == -1  # argument checks come before any device call


# ---- the SKE_HD arithmetic

@pytest.fixture(scope="module")
def compact_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "rowscompact_host.cpp")
    exe = str(tmp_path_factory.mktemp("rowscompact") / "rowscompact_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "runtime error" not in out.stderr, out.stderr
        return out.stdout.splitlines()
    return run


def test_counts_and_head_rule(compact_host):
    top = 1 << 28  # the largest log
    triples = [(0, 0, 0), (1, 0, 0), (1, 1, 1), (5, 5, 5), (10, 7, 3), (10, 10, 1), (top, top, top), (top, top - 1, 1),
               (top, 0, 0), (257, 256, 255)]
    lines = compact_host("counts", *[f"{b}:{m}:{r}" for b, m, r in triples])
    assert len(lines) == len(triples)
    for (before, m, runs), line in zip(triples, lines):
        got = [int(x) for x in line.split()]
        assert got == [before, runs, m - runs, before - m] and got[0] == sum(got[1:])
    # the head: used = kept, taken less the rows removed; used + refused + dropped == taken holds on
    heads = [(0, 0, 0), (10, 10, 10), (10, 14, 3), (256, 400, 200), (top, top + 77, 0), (top, 2 ** 40, top - 1),
             (1, 2 ** 64 - 1, 0)]
    lines = compact_host("head", *[f"{u}:{t}:{k}" for u, t, k in heads])
    for (used, taken, kept), line in zip(heads, lines):
        assert [int(x) for x in line.split()] == [kept, taken - (used - kept)]
        assert kept + (taken - used) == taken - (used - kept)  # the other counts (taken - used) are untouched


# ---- over a context stub

def rows_calls(ctx):
    return [c for c in ctx.log if c[0].startswith("ske_rows")]


@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    return cl, ctx


def test_rows_compact_is_one_call(pkg, stub_client):
    cl, ctx = stub_client
    rid = cl.rows_create("table", 10)

    def compact(r, keep_since, out):
        out._obj.before, out._obj.kept, out._obj.superseded, out._obj.expired = 9, 4, 3, 2
    ctx.hooks["ske_rows_compact"] = compact
    for keep_since, want in ((None, I64_MIN), (0, 0), (-5, -5), (1742374800, 1742374800),
                             (datetime(2025, 3, 19, 9, 0, 0), 1742374800), (np.datetime64("1969-12-31T23:59:59.5"), -1),
                             (np.int64(7), 7)):
        ctx.log.clear()
        got = cl.rows_compact("table", keep_since)
        assert ctx.log == [["ske_rows_compact", rid, want, "*"]], keep_since
        assert got == dict(before=9, kept=4, superseded=3, expired=2)
    with pytest.raises(pkg.ResponseError, match="ERR row log does not exist"):
        cl.rows_compact("nope")
    # StudentCounts and the processor pass it on; without records they refuse
    sc = pkg.StudentCounts(cl, records="table")
    proc = pkg.AttendanceProcessor(cl, counts=sc)
    ctx.log.clear()
    assert sc.compact_records(5)["kept"] == 4 and proc.compact_records()["expired"] == 2
    assert ctx.log == [["ske_rows_compact", rid, 5, "*"], ["ske_rows_compact", rid, I64_MIN, "*"]]
    plain = pkg.StudentCounts(cl, "a2", "i2")
    ctx.log.clear()
    for call in (plain.compact_records, pkg.AttendanceProcessor(cl, counts=plain).compact_records):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        pkg.StudentCounts(cl, "a3", "i3", records_compact=True)
    assert rows_calls(ctx) == []


def feed(pkg, sc, n):
    buf, offs = pkg.pack(list(range(n)))
    sc.count_packed(buf, offs, [1] * n, times=np.arange(n, dtype=np.int64), lectures=["L"] * n)


def test_auto_compact_bound(pkg, stub_client):
    """the bound compacts when, and only when, bound + n > capacity"""
    cl, ctx = stub_client
    kept = []

    def info(r, out):
        out._obj.capacity, out._obj.used = 256, 28

    def compact(r, keep_since, out):
        out._obj.kept = kept.pop(0)
    ctx.hooks.update({"ske_rows_info": info, "ske_rows_compact": compact})
    ctx.log.clear()
    sc = pkg.StudentCounts(cl, records="table", records_capacity_log2=8, records_compact=True,
                           records_keep_since=datetime(2025, 3, 19, 9, 0, 0))
    rid = cl.rows_rid("table")
    assert [c[0] for c in rows_calls(ctx)] == ["ske_rows_init", "ske_rows_info"]  # an existing log's `used` is the start
    ctx.log.clear()
    kept[:] = [56, 0, 255]
    #                 bound before -> after
    feed(pkg, sc, 100)  # 28 -> 128
    feed(pkg, sc, 128)  # 128 -> 256: exactly full is no reason
    feed(pkg, sc, 1)    # 256 + 1 > 256: compact (kept 56) -> 57
    feed(pkg, sc, 199)  # 57 -> 256
    feed(pkg, sc, 300)  # compact (kept 0); the batch still does not fit and goes ahead -> 300
    feed(pkg, sc, 1)    # compact (kept 255) -> 256
    calls = [(c[0], c[2] if c[0] == "ske_rows_compact" else c[-1]) for c in rows_calls(ctx)]
    A, K = "ske_rows_append_packed_async", "ske_rows_compact"
    assert calls == [(A, 100), (A, 128), (K, 1742374800), (A, 1), (A, 199), (K, 1742374800), (A, 300),
                     (K, 1742374800), (A, 1)]
    assert all(c[1] == rid for c in rows_calls(ctx)) and kept == []
    assert "ske_rows_info" not in ctx.calls[ctx.calls.index(A):]  # the append path never asks the device
    # a compaction the caller asks for resets the bound as well
    kept[:] = [10]
    ctx.log.clear()
    sc.compact_records()
    feed(pkg, sc, 246)  # 10 -> 256
    assert [c[0] for c in rows_calls(ctx)] == [K, A] and rows_calls(ctx)[0][2] == I64_MIN


def test_default_path_is_unchanged(pkg):
    """without records_compact no new call is made: the same feed gives the call list of the plain option"""
    logs = []
    for opts in (dict(), dict(records_compact=False), dict(records_compact=True)):
        ctx = StubContext(pkg.load_library())
        ctx.hooks["ske_rows_info"] = lambda r, out: setattr(out._obj, "capacity", 1 << 12)
        cl = pkg.SketchClient(decode_responses=True, context=ctx)
        cl.execute_command("BF.RESERVE", "bf", 0.01, 100)
        sc = pkg.StudentCounts(cl, records="table", records_capacity_log2=12, **opts)
        ids = np.zeros((3, 8), np.uint8)
        sc.update("bf", np.zeros(3, np.uint32), ids, times=[1, 2, 3], lectures=["a", "b", "c"])
        feed(pkg, sc, 5)
        logs.append([c for c in ctx.log if c[0] not in ("ske_device_alloc", "ske_device_free")])
    rid = 0
    assert logs[0] == logs[1]
    assert [c for c in logs[0] if c[0].startswith("ske_rows")] == [
        ["ske_rows_init", rid, 12],
        ["ske_rows_append_fixed_async", rid, "*", "*", "*", 8, "*", "*", None, 3],
        ["ske_rows_append_packed_async", rid, "*", "*", "*", "*", "*", "*", None, 5]]
    # with the option on and room left: one ske_rows_info when the object is made, nothing else
    assert [c for c in logs[2] if c[0] != "ske_rows_info"] == logs[0]
    assert [c[0] for c in logs[2]].count("ske_rows_info") == 1
