"""Heavy-hitter set statistics, the parts that need no GPU: the argument checks
that come before any device call, the constants and the struct layout, the
error texts that must not move, the radix select's arithmetic
(csrc/sketch_hh_select.h through tests/native/hhstats_host.cpp, a stand-alone
program that can also be built by hand with ``-Xarch_host
-fsanitize=address,undefined``), the reference's threshold rules in integers
(``analysis.reference_rule``) against ``fractions.Fraction`` and numpy, and what
the facade and ``StudentCounts`` make of the struct (over a context stub)."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from facade_stub import StubContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "sketch.h")
U32 = 0xFFFFFFFF


def test_null_context_is_rejected(pkg):
    from rtsas_amd import _lib
    lib = pkg.load_library()
    out, n = _lib.HhStats(), C.c_uint64()
    ranks, est = (C.c_uint64 * 1)(0), (C.c_uint32 * 1)(0)
    assert lib.ske_hh_stats(None, 0, 0, 0, C.byref(out)) == -1
    assert lib.ske_hh_select(None, 0, 0, 0, ranks, 1, est, C.byref(n)) == -1


def test_max_ranks_matches_the_header(pkg):
    from rtsas_amd import _lib
    m = re.search(r"#define SKE_HH_MAX_RANKS (\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == _lib.SKE_HH_MAX_RANKS == 16


def test_stats_struct_layout(pkg, tmp_path):
    """ctypes' HhStats mirrors ske_hh_stats_t field by field; 56 bytes"""
    from rtsas_amd._lib import HhStats
    fields = [f for f, _ in HhStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "sketch.h"\n'
                   'int main(void) { printf("%zu", sizeof(ske_hh_stats_t));\n'
                   + "".join(f'printf(" %zu", offsetof(ske_hh_stats_t, {f}));\n' for f in fields)
                   + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(HhStats)] + [getattr(HhStats, f).offset for f in fields]
    assert got[0] == 56 and fields == ["n", "sum", "sq_lo", "sq_hi", "min", "max", "med_lo", "med_hi", "complete",
                                       "reserved"]


def test_no_new_error_code(pkg):
    from rtsas_amd import _lib
    assert _lib.strerror(-28) == "ERR unknown" and _lib.strerror(-31) == "ERR unknown"
    assert not re.search(r"#define SKE_E\w+ -(28|31)\b", open(HEADER).read())


# ---------------------------------------------------------------- the select on the host
@pytest.fixture(scope="module")
def select_exe(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "hhstats_host.cpp")
    exe = str(tmp_path_factory.mktemp("hhstats") / "hhstats_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-o", exe, src], check=True)
    return exe


def _run(exe, args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()}
    return lines


SELECT_SIZES = [1, 2, 3, 255, 256, 257]


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_values_on_the_command_line(select_exe, n):
    rng = np.random.default_rng(n)
    cases = {
        "all equal": np.full(n, 0x01020304, np.uint64),
        "top byte only": (rng.integers(0, 256, n).astype(np.uint64) << np.uint64(24)) | np.uint64(0x345678),
        "low byte only": np.uint64(0x12345600) | rng.integers(0, 256, n).astype(np.uint64),
        "extremes": np.where(rng.random(n) < 0.5, 0, U32).astype(np.uint64),
        "both extremes": np.asarray(([0, U32] * n)[:n], np.uint64),
        "random": rng.integers(0, 1 << 32, n, dtype=np.uint64),
        "small counts": rng.zipf(1.3, n).clip(max=U32).astype(np.uint64),
    }
    for name, vals in cases.items():
        vals = [int(v) for v in vals]
        got = _run(select_exe, vals)
        assert got["n"] == [n], name
        assert got["select"] == sorted(vals), name  # every rank 0 .. n-1


@pytest.mark.parametrize("kind", range(5))
def test_select_values_from_a_seed(select_exe, kind):
    for n in SELECT_SIZES:
        got = _run(select_exe, ["-s", 17 + n, n, kind])
        assert got["n"] == [n] and len(got["values"]) == n
        assert got["select"] == sorted(got["values"]), (kind, n)
        if kind == 1:
            assert len(set(got["values"])) == 1
        if kind == 4:
            assert set(got["values"]) <= {0, U32}


# ---------------------------------------------------------------- the threshold rules
def _stats_of(vals):
    """what hh_stats returns for a population, from Python ints"""
    from rtsas_amd.client_hh import derive_stats
    v = sorted(int(x) for x in vals)
    n = len(v)
    sq = sum(x * x for x in v)
    raw = {"n": n, "sum": sum(v), "sq_lo": 0, "sq_hi": 0, "min": v[0] if n else 0, "max": v[-1] if n else 0,
           "med_lo": v[(n - 1) // 2] if n else 0, "med_hi": v[n // 2] if n else 0, "complete": 1}
    # any split with sq_hi * 2^32 + sq_lo == sq and both words below 2^56 is legal; the device's is this one
    raw["sq_lo"] = sum((x * x) & U32 for x in v)
    raw["sq_hi"] = sum((x * x) >> 32 for x in v)
    assert raw["sq_hi"] * 2 ** 32 + raw["sq_lo"] == sq and max(raw["sq_lo"], raw["sq_hi"]) < 1 << 56
    return derive_stats(raw)


def _passes_exactly(est, vals, rule):
    """est > median (+ std), decided with Fractions: est - median > std <=> positive and its square > variance"""
    v = sorted(vals)
    n = len(v)
    median = Fraction(v[(n - 1) // 2] + v[n // 2], 2)
    if rule == "median":
        return est > median
    var = Fraction(n * sum(x * x for x in v) - sum(v) ** 2, n * (n - 1))
    d = est - median
    return d > 0 and d * d > var


@pytest.mark.parametrize("rule", ["median", "median+std"])
def test_reference_rule_random_populations(pkg, rule):
    from rtsas_amd.analysis import reference_rule
    rng = np.random.default_rng(5)
    pops = [rng.zipf(1.5, n).clip(max=U32) for n in (2, 3, 4, 5, 10, 11, 100, 1001)]
    pops += [rng.integers(0, 1 << 32, n, dtype=np.uint64) for n in (2, 3, 50, 51)]
    pops += [rng.integers(0, 4, n) for n in (2, 7, 64)] + [np.full(9, 4), np.asarray([0, 0, 0, 1])]
    for vals in pops:
        vals = [int(x) for x in vals]
        thr = reference_rule(_stats_of(vals), rule)
        assert isinstance(thr, int)
        assert _passes_exactly(thr, vals, rule) and not _passes_exactly(thr - 1, vals, rule)
        # numpy's floats agree wherever no estimate sits within rounding of the bound
        a = np.asarray(vals, np.float64)
        bound = np.median(a) + (np.std(a, ddof=1) if rule == "median+std" else 0.0)
        want = {x for x in vals if x > bound}
        near = {x for x in vals if abs(x - bound) <= 1e-9 * max(1.0, abs(bound))}
        assert {x for x in vals if x >= thr} - near == want - near


def test_reference_rule_edges(pkg):
    from rtsas_amd.analysis import reference_rule
    # median 5, std exactly 2, strict >: 7 does not pass, the threshold is 8 and nobody passes
    s = _stats_of([3, 5, 7])
    assert s["median"] == 5.0 and s["std"] == 2.0 == np.std([3, 5, 7], ddof=1)
    assert reference_rule(s, "median+std") == 8 and reference_rule(s, "median") == 6
    for rule in ("median", "median+std"):
        assert reference_rule(_stats_of([]), rule) is None
    assert reference_rule(_stats_of([4]), "median+std") is None  # pandas' std of one value is NaN
    assert reference_rule(_stats_of([4]), "median") == 5
    assert math.isnan(_stats_of([4])["std"]) and math.isnan(_stats_of([])["std"])
    two = _stats_of([1, 4])  # median 2.5, std sqrt(4.5) = 2.12..: the bound is 4.62..
    assert reference_rule(two, "median") == 3 and reference_rule(two, "median+std") == 5
    assert two["std"] == pytest.approx(np.std([1, 4], ddof=1), rel=1e-15)
    with pytest.raises(ValueError):
        reference_rule(two, "mean")


def test_reference_rule_beyond_64_bits(pkg):
    """2^23 estimates of 2^32 - 1: n * sumsq and sum * sum pass 2^64"""
    from rtsas_amd.analysis import reference_rule
    from rtsas_amd.client_hh import derive_stats
    n = 1 << 23
    raw = {"n": n, "sum": n * U32, "sq_lo": n * ((U32 * U32) & U32), "sq_hi": n * ((U32 * U32) >> 32),
           "min": U32, "max": U32, "med_lo": U32, "med_hi": U32, "complete": 1}
    assert max(raw["sq_lo"], raw["sq_hi"]) < 1 << 56
    s = derive_stats(raw)
    assert s["sumsq"] == n * U32 * U32 and n * s["sumsq"] > 1 << 64
    assert s["std"] == 0.0 and s["mean"] == float(U32) and s["median"] == float(U32)
    assert reference_rule(s, "median+std") == 1 << 32 == reference_rule(s, "median")  # above every u32: nobody passes
    # one estimate lower: the variance numerator is n - 1 squares of the gap, still exact
    raw2 = dict(raw, sum=raw["sum"] - U32, min=0)
    sq = (n - 1) * U32 * U32
    raw2["sq_lo"], raw2["sq_hi"] = sq & U32, sq >> 32
    s2 = derive_stats(raw2)
    var = Fraction(n * sq - raw2["sum"] ** 2, n * (n - 1))
    assert s2["std"] == pytest.approx(math.sqrt(var), rel=1e-15)
    thr = reference_rule(s2, "median+std")
    d = thr - U32
    assert d > 0 and d * d > var and (d - 1) ** 2 <= var


# ---------------------------------------------------------------- the facade over a stub
@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    return pkg.SketchClient(decode_responses=True, context=ctx), ctx


def _fill_stats(vals, complete=1):
    """a ske_hh_stats hook: the struct as the device would fill it for these estimates"""
    v = sorted(int(x) for x in vals)
    n = len(v)

    def hook(hid, cid, threshold, ref):
        s = ref._obj
        s.n, s.sum = n, sum(v)
        s.sq_lo, s.sq_hi = sum((x * x) & U32 for x in v), sum((x * x) >> 32 for x in v)
        s.min, s.max = (v[0], v[-1]) if n else (0, 0)
        s.med_lo, s.med_hi = (v[(n - 1) // 2], v[n // 2]) if n else (0, 0)
        s.complete = complete
    return hook


def test_hh_stats_derived_fields(pkg, stub_client):
    cl, ctx = stub_client
    cl.execute_command("CMS.INITBYDIM", "c", 100, 5)
    cl.hh_create("s", "c", 10)
    vals = [7, 1, 4, 4, 4000000000, 9]
    ctx.hooks["ske_hh_stats"] = _fill_stats(vals, complete=0)
    ctx.log.clear()
    s = cl.hh_stats("s", 3)
    assert [c[:4] for c in ctx.log] == [["ske_hh_stats", cl._hh[b"s"][0], cl.cms_cid("c"), 3]]
    a = np.asarray(vals, np.float64)
    assert s["n"] == 6 and s["sum"] == sum(vals) and s["sumsq"] == sum(x * x for x in vals)
    assert isinstance(s["sumsq"], int) and s["sumsq"] > 1 << 63
    assert (s["min"], s["max"], s["median"], s["complete"]) == (1, 4000000000, 5.5, False)
    assert s["mean"] == pytest.approx(a.mean(), rel=1e-15) and s["std"] == pytest.approx(a.std(ddof=1), rel=1e-14)
    ctx.hooks["ske_hh_stats"] = _fill_stats([])
    e = cl.hh_stats("s")
    assert ctx.log[-1][3] == 0  # the default threshold: every member
    assert (e["n"], e["sum"], e["sumsq"], e["min"], e["max"], e["complete"]) == (0, 0, 0, 0, 0, True)
    assert all(math.isnan(e[k]) for k in ("median", "mean", "std"))
    ctx.hooks["ske_hh_stats"] = _fill_stats([5])
    one = cl.hh_stats("s")
    assert one["median"] == 5.0 == one["mean"] and math.isnan(one["std"])
    with pytest.raises(pkg.ResponseError, match="heavy-hitter set does not exist"):
        cl.hh_stats("nosuch")


def test_hh_select_splits_the_ranks(pkg, stub_client):
    cl, ctx = stub_client
    cl.execute_command("CMS.INITBYDIM", "c", 100, 5)
    cl.hh_create("s", "c", 10)
    seen = []

    def hook(hid, cid, threshold, ranks, nranks, out, n_out):
        r = np.ctypeslib.as_array(C.cast(ranks, C.POINTER(C.c_uint64)), (nranks,))
        seen.append(r.tolist())
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), (nranks,))[:] = r * 3 + 1
    ctx.hooks["ske_hh_select"] = hook
    ranks = list(range(39, -1, -1))
    ctx.log.clear()
    got = cl.hh_select("s", ranks, threshold=2)
    assert got.dtype == np.uint32 and got.tolist() == [3 * r + 1 for r in ranks]
    assert [len(s) for s in seen] == [16, 16, 8] and sum(seen, []) == ranks
    assert [(c[0], c[3], c[5]) for c in ctx.log] == [("ske_hh_select", 2, 16), ("ske_hh_select", 2, 16),
                                                     ("ske_hh_select", 2, 8)]
    ctx.log.clear()
    assert cl.hh_select("s", []).size == 0 and ctx.log == []
    # the quantile: numpy's linear interpolation between the two order statistics around q * (n - 1)
    vals = sorted([3, 9, 4, 100, 7, 7, 2])
    ctx.hooks["ske_hh_stats"] = _fill_stats(vals)

    def pick(hid, cid, threshold, ranks, nranks, out, n_out):
        r = np.ctypeslib.as_array(C.cast(ranks, C.POINTER(C.c_uint64)), (nranks,))
        np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint32)), (nranks,))[:] = [vals[int(i)] for i in r]
    ctx.hooks["ske_hh_select"] = pick
    for q in (0.0, 0.1, 0.25, 0.5, 0.9, 1.0):
        assert cl.hh_quantile("s", q) == pytest.approx(np.quantile(vals, q), rel=1e-12)
    ctx.hooks["ske_hh_stats"] = _fill_stats([])
    assert math.isnan(cl.hh_quantile("s", 0.5))
    with pytest.raises(ValueError):
        cl.hh_quantile("s", 1.5)


def _no_memory(calls):
    return [c for c in calls if c[0] not in ("ske_device_alloc", "ske_memcpy", "ske_device_free")]


def test_insights_reference_call_sequence(pkg, stub_client):
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, "a", "i", track_attended=1, track_invalid=2, capacity_log2=12, late_key="l",
                           track_late=1)
    vals = [3, 5, 7, 9, 40]
    ctx.hooks["ske_hh_stats"] = _fill_stats(vals)
    want = sc.reference_threshold("attended", "median+std")
    a = np.asarray(vals, np.float64)
    assert want == math.floor(np.median(a) + a.std(ddof=1)) + 1 == 23
    assert sc.population("attended")["n"] == 5 and sc.reference_threshold("late", "median") == 8
    with pytest.raises(ValueError):
        sc.population("lectures")
    hid, cid = cl._hh_entry(b"hh:a")
    ctx.log.clear()
    ins = sc.insights(attended_threshold="reference", invalid_threshold=7, late_threshold=9)
    got = _no_memory(ctx.log)
    # late (an integer: as before), attended (stats, then the list at the derived threshold), invalid
    assert [c[0] for c in got] == ["ske_hh_info", "ske_hh_list", "ske_hh_stats", "ske_hh_list", "ske_hh_info",
                                   "ske_hh_list"]
    assert got[2][1:4] == [hid, cid, 1] and got[3][1:4] == [hid, cid, want]
    assert got[1][3] == 9 and got[5][3] == 7
    assert [i["title"] for i in ins] == ["Habitual Latecomers", "Most Consistent Attendees",
                                         "Invalid Attendance Attempts"]
    # the other two: the late key by the median rule; the invalid key lists all, its track threshold
    ctx.log.clear()
    sc.insights(invalid_threshold="reference", late_threshold="reference")
    got = _no_memory(ctx.log)
    assert [c[0] for c in got] == ["ske_hh_stats", "ske_hh_list", "ske_hh_info", "ske_hh_list", "ske_hh_info",
                                   "ske_hh_list"]
    assert got[0][3] == 1 and got[1][3] == 8 and got[3][3] == 1 and got[5][3] == 2
    # nothing can pass: no list call, data is {}
    for vals in ([], [6]):
        ctx.hooks["ske_hh_stats"] = _fill_stats(vals, complete=0)
        ctx.log.clear()
        ins = sc.insights(attended_threshold="reference")
        got = _no_memory(ctx.log)
        assert [c[0] for c in got][2:3] == ["ske_hh_stats"] and [c[0] for c in got].count("ske_hh_list") == 2
        assert ins[1]["data"] == {} and ins[1]["complete"] is False


def test_insights_defaults_make_todays_calls(pkg, stub_client):
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, "a", "i", track_attended=3, track_invalid=2, capacity_log2=12, late_key="l",
                           track_late=1)
    ctx.log.clear()
    sc.insights()
    got = _no_memory(ctx.log)
    assert [c[0] for c in got] == ["ske_hh_info", "ske_hh_list"] * 3
    assert [c[3] for c in got if c[0] == "ske_hh_list"] == [1, 3, 2]  # late, attended, invalid: the track thresholds
    assert not any("stats" in c[0] or "select" in c[0] for c in ctx.log)
    untracked = pkg.StudentCounts(cl, "a2", "i2")
    with pytest.raises(ValueError):
        untracked.population("attended")
    with pytest.raises(ValueError):
        untracked.reference_threshold("late", "median")
