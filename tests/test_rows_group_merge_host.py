"""The group merge, the parts that need no GPU: ``rows_group_merge_oracle`` over
the ``rows_group_oracle`` of a by-lecture split against the one-context truth
(and that against pandas); the counter-case that pins the precondition -- a
lecture split over two parts with one row sent to both; the arithmetic of
csrc/sketch_rows_merge.h (a stand-alone program, tests/native/rowsmerge_host.cpp,
built with ``-Xarch_host -fsanitize=address,undefined``); the C ABI's surface;
and over a context stub the facade's two calls and its ``ValueError`` paths."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from facade_stub import StubContext
from rows_group_cases import DAY0, LATE, hand_batches
from rows_merge_cases import FILTERS, lecture_owner, merge_entries, random_batch, split_by_lecture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
STAT_KEYS = ("rows", "n", "sum", "sumsq", "min", "max", "med_lo", "med_hi", "median")
DATA = {"hand": hand_batches, "random": lambda: [random_batch(400, 11), random_batch(150, 12)]}


def same(got, want):
    assert got["keys"].dtype == want["keys"].dtype and got["counts"].dtype == np.uint64
    assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["counts"], want["counts"])
    assert {k: got["stats"][k] for k in STAT_KEYS} == {k: want["stats"][k] for k in STAT_KEYS}


def parts_of(batches, world):
    # five parts: the owners are drawn among four, so the last part is empty whatever the names hash to
    owner = (lambda lec, w: lecture_owner(lec, w - 1)) if world == 5 else lecture_owner
    return split_by_lecture(batches, world, owner)


@pytest.mark.parametrize("world", [1, 2, 3, 5])
@pytest.mark.parametrize("data", sorted(DATA))
def test_merge_of_a_lecture_split_is_the_one_context_answer(pkg, data, world):
    from rtsas_amd.client_rows import rows_group_merge_oracle, rows_group_oracle
    batches = DATA[data]()
    parts = parts_of(batches, world)
    assert sum(len(b[1]) for p in parts for b in p) == sum(len(b[1]) for b in batches)
    if world == 5:
        assert any(not p for p in parts)
    if world > 1:
        assert sum(1 for p in parts if p) >= 2  # the lectures do lie on more than one part
    for by in ("student", "lecture"):
        for which, kw in FILTERS.items():
            got = rows_group_merge_oracle([rows_group_oracle(p, by, **kw) for p in parts], by)
            want = rows_group_oracle(batches, by, **kw)
            same(got, want)
            assert got["multi"] == 0 if by == "lecture" else got["multi"] <= got["stats"]["n"], (by, which)
    if world > 1:  # a student attends lectures of several ranks: the by-student merge does sum entries
        got = rows_group_merge_oracle([rows_group_oracle(p, "student") for p in parts], "student")
        assert got["multi"] > 0


@pytest.mark.parametrize("data", sorted(DATA))
def test_merged_students_against_pandas(pkg, data):
    pd = pytest.importorskip("pandas")
    from rtsas_amd.client_rows import rows_group_merge_oracle, rows_group_oracle
    batches = DATA[data]()
    rows = [(lec, e, int(i), bool(v)) for lecs, ids, eps, valid, _ in batches
            for lec, i, e, v in zip(lecs, ids, eps, valid)]
    df = pd.DataFrame(rows, columns=["lecture_id", "epoch", "student_id", "is_valid"])
    df = df.drop_duplicates(subset=["lecture_id", "epoch", "student_id"], keep="last")
    masks = {"attended": np.ones(len(df), bool), "late": (df["epoch"] % 86400 >= LATE).to_numpy(),
             "invalid": (~df["is_valid"]).to_numpy()}
    parts = parts_of(batches, 3)
    for which, kw in FILTERS.items():
        sizes = df[masks[which]].groupby("student_id").size()
        got = rows_group_merge_oracle([rows_group_oracle(p, "student", **kw) for p in parts], "student")
        assert got["keys"].tolist() == [int(k) for k in sizes.index] and got["counts"].tolist() == sizes.tolist()
        assert got["stats"]["rows"] == len(df) and got["stats"]["n"] == len(sizes)
        if len(sizes):
            assert got["stats"]["median"] == sizes.median()
            assert (got["stats"]["min"], got["stats"]["max"]) == (sizes.min(), sizes.max())


def test_a_split_lecture_with_a_row_on_both_ranks_counts_it_twice(pkg):
    """the precondition, pinned: the upsert collapse is rank-local"""
    from rtsas_amd.client_rows import rows_group_merge_oracle, rows_group_oracle
    rows = [("L", str(i), DAY0 + i, 1) for i in range(6)] + [("M", "1", DAY0, 1)]
    redelivered = ("L", "2", DAY0 + 2, 0)

    def batch(rs):
        return [([r[0] for r in rs], [r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs], None)]
    everything = batch(rows + [redelivered])
    part0, part1 = batch(rows[:3] + [rows[6]] + [redelivered]), batch(rows[3:6] + [redelivered])
    for by in ("lecture", "student"):
        one = rows_group_oracle(everything, by)
        got = rows_group_merge_oracle([rows_group_oracle(part0, by), rows_group_oracle(part1, by)], by)
        assert got["stats"]["sum"] == one["stats"]["sum"] + 1 and got["stats"]["rows"] == one["stats"]["rows"] + 1
        assert np.array_equal(got["keys"], one["keys"])
        assert (got["counts"].astype(np.int64) - one["counts"].astype(np.int64)).tolist().count(1) == 1
        if by == "lecture":
            assert got["multi"] == 1  # L lies on both parts, M on one
    # the same split without the second copy: multi still says the lecture was split, the sums are right
    got = rows_group_merge_oracle([rows_group_oracle(part0, "lecture"), rows_group_oracle(batch(rows[3:6]), "lecture")],
                                  "lecture")
    assert got["multi"] == 1 and np.array_equal(got["counts"], rows_group_oracle(everything, "lecture")["counts"])


def test_oracle_rules(pkg):
    from rtsas_amd.client_rows import group_stats, rows_group_merge_oracle
    part = {"keys": np.asarray([I64_MIN, -1, 0, I64_MAX], np.int64), "counts": np.asarray([0, 3, 0, 2], np.uint64),
            "stats": {"rows": 9}}
    got = rows_group_merge_oracle([part], "student")
    assert got["keys"].tolist() == [-1, I64_MAX] and got["counts"].tolist() == [3, 2] and got["multi"] == 0
    assert got["stats"] == dict(group_stats([3, 2]), rows=9)
    # the same bits by lecture: unsigned order
    u = dict(part, keys=part["keys"].view(np.uint64))
    got = rows_group_merge_oracle([u, u], "lecture")
    assert got["keys"].tolist() == [I64_MAX, (1 << 64) - 1] and got["counts"].tolist() == [4, 6] and got["multi"] == 2
    assert got["stats"]["rows"] == 18
    # a zero entry beside a nonzero one feeds nothing: not multi
    z = {"keys": np.asarray([5, 5, 6, 6], np.int64), "counts": np.asarray([0, 7, 0, 0], np.uint64)}
    got = rows_group_merge_oracle([z], "student")
    assert (got["keys"].tolist(), got["counts"].tolist(), got["multi"]) == ([5], [7], 0)
    assert rows_group_merge_oracle([], "student")["stats"]["n"] == 0
    top = {"keys": np.asarray([1, 2], np.int64), "counts": np.asarray([(1 << 32) - 2, 1], np.uint64)}
    assert rows_group_merge_oracle([top], "student")["stats"]["sum"] == (1 << 32) - 1
    for bad in ({"keys": [1, 2], "counts": [(1 << 32) - 1, 1]}, {"keys": [1], "counts": [1 << 32]}):
        with pytest.raises(ValueError):
            rows_group_merge_oracle([bad], "student")
    with pytest.raises(ValueError):
        rows_group_merge_oracle([], "day")


# ---- the header's arithmetic, sanitized

def test_merge_arithmetic_sanitized():
    import tempfile
    src = os.path.join(ROOT, "tests", "native", "rowsmerge_host.cpp")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rowsmerge_host")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host",
                        "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe,
                        src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr, out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "bad=0", out.stdout
    verdict = {ln.split()[0]: ln.split()[1:] for ln in lines[:-1]}
    assert verdict["total_max"][0] == "accepted=1" and verdict["total_over"][0] == "accepted=0"
    assert verdict["wide_entry"][0] == "accepted=0" and verdict["one_entry_max"][0] == "accepted=1"
    assert verdict["all_zero_groups"][1:3] == ["listed=2", "multi=1"]
    assert verdict["ones"][1:3] == ["listed=4", "multi=0"]


# ---- the C ABI's surface

def test_symbol_and_null_arguments(pkg):
    from rtsas_amd import _lib
    assert "ske_rows_group_merge" in _lib.SIGNATURES
    assert "ske_rows_group_merge" in open(_lib.HEADER_PATH).read()
    lib = pkg.load_library()
    assert lib.ske_rows_group_merge(None, 0, None, None, 0, None, None, 0, None, None, None, 0) == -1


# ---- the facade over a context stub

@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def merge_hook(pkg, keys, counts, stats, multi):
    """ske_rows_group_merge as the device answers it: the statistics always, the groups when they fit"""
    def hook(by, k_in, c_in, n_in, o_key, o_count, cap, n_out, st, m_out, mem):
        n_out._obj.value, m_out._obj.value = len(keys), multi
        for k, v in stats.items():
            setattr(st._obj, k, v)
        if len(keys) > cap:
            raise pkg.SketchLibError(-45, "ERR row log selection does not fit the output")
        for ptr, col in ((o_key, keys), (o_count, counts)) if keys else ():
            arr = (C.c_uint64 * len(keys)).from_address(ptr.value)
            for j, v in enumerate(col):
                arr[j] = v % (1 << 64)
    return hook


def merge_calls(ctx):
    return [c for c in ctx.log if c[0] == "ske_rows_group_merge"]


def test_two_call_protocol(pkg, stub_client):
    cl, ctx = stub_client
    stats = dict(rows=0, n=3, sum=8, sumsq=26, min=1, max=4, med_lo=3, med_hi=3)
    ctx.hooks["ske_rows_group_merge"] = merge_hook(pkg, [-2, 5, I64_MAX], [1, 4, 3], stats, 2)
    keys, counts = np.asarray([5, -2, 5, I64_MAX, 9], np.int64), np.asarray([1, 1, 3, 3, 0], np.uint64)
    got = cl.rows_group_merge("student", keys, counts)
    # the count call, then the sized call; host memory, five entries
    assert merge_calls(ctx) == [["ske_rows_group_merge", 0, "*", "*", 5, None, None, 0, "*", "*", "*", 0],
                                ["ske_rows_group_merge", 0, "*", "*", 5, "*", "*", 3, "*", "*", "*", 0]]
    assert got["keys"].dtype == np.int64 and got["keys"].tolist() == [-2, 5, I64_MAX]
    assert got["counts"].dtype == np.uint64 and got["counts"].tolist() == [1, 4, 3]
    assert got["stats"] == dict(stats, median=3.0) and got["multi"] == 2
    ctx.log.clear()
    got = cl.rows_group_merge("lecture", keys.view(np.uint64), counts, groups=False)
    assert [c[1] for c in merge_calls(ctx)] == [1] and got["keys"].size == 0 and got["keys"].dtype == np.uint64
    assert got["stats"]["n"] == 3 and got["multi"] == 2
    # nothing listed: the count call succeeds and is the only one
    ctx.hooks["ske_rows_group_merge"] = merge_hook(pkg, [], [], dict(n=0), 0)
    ctx.log.clear()
    got = cl.rows_group_merge("student", np.zeros(0, np.int64), np.zeros(0, np.uint64))
    assert merge_calls(ctx) == [["ske_rows_group_merge", 0, None, None, 0, None, None, 0, "*", "*", "*", 0]]
    assert got["keys"].size == 0 and got["multi"] == 0 and got["stats"]["median"] == 0
    # any other error passes through
    ctx.hooks["ske_rows_group_merge"] = lambda *a: (_ for _ in ()).throw(pkg.SketchLibError(-1, "ERR invalid argument"))
    with pytest.raises(pkg.SketchLibError):
        cl.rows_group_merge("student", keys, counts)


def test_value_error_paths(pkg, stub_client):
    cl, ctx = stub_client
    k, c = np.asarray([1, 2], np.int64), np.asarray([1, 1], np.uint64)
    for bad in (lambda: cl.rows_group_merge("day", k, c), lambda: cl.rows_group_merge("student", k, c[:1]),
                lambda: cl.rows_group_merge("student", k.reshape(1, 2), c.reshape(1, 2)),
                lambda: cl.rows_group_merge("student", k.astype(float), c),
                lambda: cl.rows_group_merge("student", k, np.asarray([1, -1], np.int64)),
                lambda: cl.rows_group_merge("student", k, np.asarray([1 << 32, 0], np.uint64)),
                lambda: cl.rows_group_merge("student", k, np.asarray([(1 << 32) - 1, 1], np.uint64))):
        with pytest.raises(ValueError):
            bad()
    assert ctx.calls == []  # refused before any native call
