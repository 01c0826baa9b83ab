"""The row log's group-by, the parts that need no GPU: ``rows_group_oracle`` and
``rows_profile_oracle`` against pandas over a hand-built batch, with
``reference_rule`` picking the students pandas picks; the arithmetic of
csrc/sketch_rows_group.h (a stand-alone program, tests/native/rowsgroup_host.cpp,
built with ``-Xarch_host -fsanitize=address,undefined``) against Python; the
constants and the struct; and over a context stub the facade's native calls,
the capacity protocol and the ``ValueError`` paths."""
import ctypes as C
import os
import re
import subprocess
from datetime import datetime, timezone

import numpy as np
import pytest

from facade_stub import StubContext
from rows_group_cases import COUNT_SETS, DAY0, LATE, hand_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
WINDOWS = [dict(), dict(lecture="CS101"), dict(lecture="solo"), dict(lecture="pair"), dict(lecture="nobody"),
           dict(since=DAY0 + 86400, until=DAY0 + 3 * 86400), dict(lecture="MA201", until=DAY0 + LATE)]


def test_day0_is_the_monday_it_says():
    d = datetime.fromtimestamp(DAY0, timezone.utc)
    assert (d.year, d.month, d.day, d.hour, d.weekday()) == (2025, 3, 17, 0, 0)


# ---- the oracles against pandas

def table(pd, batches, lecture=None, since=None, until=None):
    """the batches as the reference's de-duplicated frame: arrival order, the
    last write per (lecture, timestamp, student) kept, the window applied"""
    rows = [(lec, e, int(i), bool(v)) for lecs, ids, eps, valid, _ in batches
            for lec, i, e, v in zip(lecs, ids, eps, valid)]
    df = pd.DataFrame(rows, columns=["lecture_id", "epoch", "student_id", "is_valid"])
    df = df.drop_duplicates(subset=["lecture_id", "epoch", "student_id"], keep="last")
    if lecture is not None:
        df = df[df["lecture_id"] == lecture]
    if since is not None:
        df = df[df["epoch"] >= since]
    if until is not None:
        df = df[df["epoch"] < until]
    df = df.copy()
    df["timestamp"] = pd.to_datetime(df["epoch"], unit="s")
    return df


def same_groups(got, sizes):
    assert got["keys"].tolist() == sizes.index.tolist() and got["counts"].tolist() == sizes.tolist()
    assert got["stats"]["n"] == len(sizes) and got["stats"]["sum"] == int(sizes.sum())


def test_hand_batch_shape(pkg):
    from rtsas_amd.client_rows import rows_oracle
    batches = hand_batches()
    n = sum(len(b[1]) for b in batches)
    assert 200 <= n <= 300
    o = rows_oracle(batches)
    log_valid = dict()
    flips = 0
    for d, e, i, v in zip(*[c.tolist() for c in o["log"]]):
        flips += (d, e, i) in log_valid and log_valid[(d, e, i)] != v
        log_valid[(d, e, i)] = v
    assert flips >= 5 and o["select"][0].size < n  # redelivered rows whose last write flips is_valid
    sods = {e % 86400 for e in o["log"][1].tolist()}
    assert {LATE - 1, LATE} <= sods and min(o["log"][1]) < 0 and min(o["log"][2]) < 0


@pytest.mark.parametrize("window", WINDOWS, ids=[str(sorted(w)) + str(w.get("lecture", "")) for w in WINDOWS])
def test_oracles_against_pandas(pkg, window):
    pd = pytest.importorskip("pandas")
    from rtsas_amd.analysis import DAY_NAMES, reference_rule
    from rtsas_amd.client_rows import lecture_digest, rows_group_oracle, rows_profile_oracle
    batches = hand_batches()
    df = table(pd, batches, **window)

    # every row per student, and the reference's consistency rule
    att = rows_group_oracle(batches, "student", **window)
    sizes = df.groupby("student_id").size()
    same_groups(att, sizes)
    assert att["stats"]["rows"] == len(df)
    if len(sizes):
        assert att["stats"]["median"] == sizes.median()
        assert (att["stats"]["min"], att["stats"]["max"]) == (sizes.min(), sizes.max())
    picked = sizes[sizes > sizes.median() + sizes.std()]
    thr = reference_rule(att["stats"], "median+std")
    assert [k for k, c in zip(att["keys"].tolist(), att["counts"].tolist()) if thr is not None and c >= thr] \
        == picked.index.tolist()

    # the late rows per student, and the median rule
    late = rows_group_oracle(batches, "student", late_from=LATE, **window)
    sizes = df[df["timestamp"].dt.hour >= 9].groupby("student_id").size()
    same_groups(late, sizes)
    picked = sizes[sizes > sizes.median()]
    thr = reference_rule(late["stats"], "median")
    assert [k for k, c in zip(late["keys"].tolist(), late["counts"].tolist()) if thr is not None and c >= thr] \
        == picked.index.tolist()
    twice = late["stats"]["med_lo"] + late["stats"]["med_hi"]
    assert [k for k, c in zip(late["keys"].tolist(), late["counts"].tolist()) if 2 * c > twice] \
        == picked.index.tolist()

    # the invalid and the valid rows per student
    same_groups(rows_group_oracle(batches, "student", valid=False, **window),
                df[~df["is_valid"]].groupby("student_id").size())
    same_groups(rows_group_oracle(batches, "student", valid=True, **window),
                df[df["is_valid"]].groupby("student_id").size())

    # per lecture: the digests name the lectures
    lec = rows_group_oracle(batches, "lecture", **window)
    sizes = df.groupby("lecture_id").size()
    assert dict(zip(lec["keys"].tolist(), lec["counts"].tolist())) == {lecture_digest(k): c for k, c in sizes.items()}
    assert lec["keys"].tolist() == sorted(lec["keys"].tolist()) and lec["keys"].dtype == np.uint64

    # per weekday and hour
    prof = rows_profile_oracle(batches, **window)
    by_day = df.groupby(df["timestamp"].dt.day_name()).size().to_dict()
    assert {DAY_NAMES[d]: int(c) for d, c in enumerate(prof.sum(axis=1)) if c} == by_day
    by_hour = df.groupby(df["timestamp"].dt.hour).size().to_dict()
    assert {h: int(c) for h, c in enumerate(prof.sum(axis=0)) if c} == by_hour
    late_prof = rows_profile_oracle(batches, late_from=LATE, valid=False, **window)
    assert int(late_prof.sum()) == int(((df["timestamp"].dt.hour >= 9) & ~df["is_valid"]).sum())
    assert int(late_prof[:, :9].sum()) == 0


def test_windows_cover_n1_and_even_n(pkg):
    from rtsas_amd.client_rows import rows_group_oracle
    ns = [rows_group_oracle(hand_batches(), "student", **w)["stats"]["n"] for w in WINDOWS]
    assert 1 in ns and 0 in ns and any(n % 2 == 0 and n > 1 for n in ns) and any(n % 2 == 1 and n > 1 for n in ns)


def test_group_stats_and_rule_on_count_sets(pkg):
    """the count sets' statistics as numpy states them; the rule against floats where they are exact"""
    from rtsas_amd.analysis import reference_rule
    from rtsas_amd.client_rows import group_stats
    for name, counts in COUNT_SETS.items():
        st = group_stats(counts)
        a = np.asarray(counts, np.int64)
        assert st["median"] == float(np.median(a)) and st["sum"] == a.sum() and st["sumsq"] == (a * a).sum(), name
        assert (st["n"], st["min"], st["max"]) == (a.size, a.min(), a.max())
        thr = reference_rule(st, "median")
        assert [c for c in counts if c >= thr] == [c for c in counts if c > np.median(a)]
    assert reference_rule(group_stats([5]), "median+std") is None
    assert group_stats([]) == {"n": 0, "sum": 0, "sumsq": 0, "min": 0, "max": 0, "med_lo": 0, "med_hi": 0,
                               "median": 0.0}


# ---- the header's arithmetic, sanitized, against Python

@pytest.fixture(scope="module")
def group_host(tmp_path_factory):
    src = os.path.join(ROOT, "tests", "native", "rowsgroup_host.cpp")
    exe = str(tmp_path_factory.mktemp("rowsgroup") / "rowsgroup_host")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-o", exe, src], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "runtime error" not in out.stderr, out.stderr
        return out.stdout.splitlines()
    return run


def test_median_select(pkg, group_host):
    from rtsas_amd.client_rows import group_stats
    rng = np.random.default_rng(5)
    sets = list(COUNT_SETS.values()) + [[0xFFFFFFFF, 0, 0x80000000], [1 << 28] * 2 + [1]]
    sets += [rng.integers(0, 1 << int(b), int(n)).tolist() for b, n in ((3, 50), (9, 51), (17, 64), (32, 33))]
    for counts in sets:
        st = group_stats(counts)
        assert group_host("median", *counts) == ["%d %d" % (st["med_lo"], st["med_hi"])], counts
    assert group_host("median") == ["0 0"]


def test_difference_and_drop_rule(group_host):
    # the counted prefix at each group's end: a group whose rows were all filtered out repeats it
    ends = [0, 0, 3, 3, 4, 260, 260, 65796, 65796]
    counts = np.diff([0] + ends).tolist()
    assert group_host("groups", *ends) == ["%d %d" % (c, c != 0) for c in counts]
    assert group_host("groups", 5) == ["5 1"] and group_host("groups") == []


def test_counted_rule(group_host):
    epochs = [0, LATE - 1, LATE, 86399, 86400, -1, -86400, -86401, DAY0 + LATE - 1, DAY0 + LATE, I64_MIN, I64_MAX]
    rows = [(v, e) for e in epochs for v in (0, 1)]
    for vf in (0, 1, 2):
        for sod in (0, 1, LATE, 86399):
            want = [int((vf == 0 or (vf == 1) == bool(v)) and e % 86400 >= sod) for v, e in rows]
            assert group_host("counted", vf, sod, *["%d:%d" % r for r in rows]) == [str(w) for w in want], (vf, sod)


# ---- the C ABI's surface

def test_constants_and_struct(pkg):
    from rtsas_amd import _lib
    txt = open(_lib.HEADER_PATH).read()
    for name, value in (("SKE_ROWS_BY_STUDENT", 0), ("SKE_ROWS_BY_LECTURE", 1), ("SKE_ROWS_VALID_ANY", 0),
                        ("SKE_ROWS_VALID_ONLY", 1), ("SKE_ROWS_INVALID_ONLY", 2)):
        m = re.search(rf"#define {name} (\d+)", txt)
        assert m and int(m.group(1)) == value == getattr(_lib, name), name
    assert C.sizeof(_lib.RowsGroupStats) == 64
    assert [f for f, _ in _lib.RowsGroupStats._fields_] == ["rows", "n", "sum", "sumsq", "min", "max", "med_lo",
                                                          "med_hi"]
    assert "ske_rows_group" in _lib.SIGNATURES and "ske_rows_profile" in _lib.SIGNATURES
    lib = pkg.load_library()
    assert lib.ske_rows_group(None, 0, 0, None, 0, 0, 0, 0, 0, None, None, 0, None, None, None, 0) == -1
    assert lib.ske_rows_profile(None, 0, None, 0, 0, 0, 0, 0, None, None, None) == -1


# ---- the facade over a context stub

@pytest.fixture
def stub_client(pkg):
    ctx = StubContext(pkg.load_library())
    cl = pkg.SketchClient(decode_responses=True, context=ctx)
    return cl, ctx


def group_calls(ctx):
    return [c for c in ctx.log if c[0] in ("ske_rows_group", "ske_rows_profile")]


def test_rows_group_calls(pkg, stub_client):
    cl, ctx = stub_client
    rid = cl.rows_create("table", 10)
    ctx.log.clear()
    got = cl.rows_group("table")
    assert group_calls(ctx) == [["ske_rows_group", rid, 0, None, 0, I64_MIN, I64_MAX, 0, 0, None, None, 0, "*", "*",
                                 "*", 0]]  # nothing listed: the count call is the only one
    assert got["keys"].dtype == np.int64 and got["counts"].dtype == np.uint64 and got["keys"].size == 0
    assert got["stats"]["n"] == 0 and got["stats"]["median"] == 0 and not got["complete"]
    ctx.log.clear()
    got = cl.rows_group("table", by="lecture", lecture="CS101", since=-5, until=77, valid=False, late_from=LATE)
    assert group_calls(ctx) == [["ske_rows_group", rid, 1, "*", 5, -5, 77, 2, LATE, None, None, 0, "*", "*", "*", 0]]
    assert got["keys"].dtype == np.uint64
    ctx.log.clear()
    cl.rows_group("table", valid=True, late_from=86399)
    assert group_calls(ctx)[0][7:9] == [1, 86399]
    ctx.log.clear()
    prof = cl.rows_profile("table", lecture=b"L", valid=True, late_from=1)
    assert group_calls(ctx) == [["ske_rows_profile", rid, "*", 1, I64_MIN, I64_MAX, 1, 1, "*", "*", "*"]]
    assert prof.shape == (7, 24) and prof.dtype == np.uint64
    ctx.calls.clear()
    for bad in (lambda: cl.rows_group("table", by="day"), lambda: cl.rows_group("table", late_from=86400),
                lambda: cl.rows_group("table", late_from=-1), lambda: cl.rows_profile("table", late_from=86400)):
        with pytest.raises(ValueError):
            bad()
    assert ctx.calls == []  # refused before any native call
    for call in (cl.rows_group, cl.rows_profile):
        with pytest.raises(pkg.ResponseError, match="ERR row log does not exist"):
            call("nope")


def group_hook(pkg, keys, counts, stats):
    """ske_rows_group as the device answers it: the statistics always, the groups when they fit"""
    def hook(rid, by, lec, llen, since, until, vf, sod, o_key, o_count, cap, n_out, st, complete, mem):
        n_out._obj.value, complete._obj.value = len(keys), 1
        for k, v in stats.items():
            setattr(st._obj, k, v)
        if len(keys) > cap:
            raise pkg.SketchLibError(-45, "ERR row log selection does not fit the output")
        for ptr, col in ((o_key, keys), (o_count, counts)):
            arr = (C.c_uint64 * len(keys)).from_address(ptr.value)
            for j, v in enumerate(col):
                arr[j] = v % (1 << 64)
    return hook


def test_capacity_protocol(pkg, stub_client):
    from rtsas_amd.analysis import reference_rule
    cl, ctx = stub_client
    cl.rows_create("table", 10)
    stats = dict(rows=9, n=3, sum=8, sumsq=26, min=1, max=4, med_lo=3, med_hi=3)
    ctx.hooks["ske_rows_group"] = group_hook(pkg, [-2, 5, I64_MAX], [1, 4, 3], stats)
    ctx.log.clear()
    got = cl.rows_group("table")
    calls = group_calls(ctx)
    assert [c[9:12] for c in calls] == [[None, None, 0], ["*", "*", 3]]  # the count call, then the sized call
    assert got["keys"].tolist() == [-2, 5, I64_MAX] and got["counts"].tolist() == [1, 4, 3] and got["complete"]
    assert got["stats"] == dict(stats, median=3.0)
    assert reference_rule(got["stats"], "median") == 4 and reference_rule(got["stats"], "median+std") == 5
    ctx.log.clear()
    got = cl.rows_group("table", groups=False)
    assert len(group_calls(ctx)) == 1 and got["keys"].size == 0 and got["stats"]["n"] == 3
    ctx.hooks["ske_rows_group"] = lambda *a: (_ for _ in ()).throw(pkg.SketchLibError(-1, "ERR invalid argument"))
    with pytest.raises(pkg.SketchLibError):
        cl.rows_group("table")


def test_student_counts_exact(pkg, stub_client):
    from rtsas_amd.client_rows import group_stats, lecture_digest
    cl, ctx = stub_client
    sc = pkg.StudentCounts(cl, records="table", lecture_counts="lectures", late_from=LATE + 1800)
    rid = cl.rows_rid("table")
    for which, vf, sod in (("attended", 0, 0), ("late", 0, LATE + 1800), ("invalid", 2, 0)):
        ctx.log.clear()
        sc.exact_counts(which)
        assert [c[:9] for c in group_calls(ctx)] == [["ske_rows_group", rid, 0, None, 0, I64_MIN, I64_MAX, vf, sod]]
    ctx.log.clear()
    assert sc.exact_by_day() == {}
    assert group_calls(ctx) == [["ske_rows_profile", rid, None, 0, I64_MIN, I64_MAX, 0, 0, "*", "*", "*"]]
    with pytest.raises(ValueError):
        sc.exact_counts("present")

    # the five entries, from one answer per call
    names = [b"B", b"A", b"C", b"D"]
    by = {0: dict(keys=[-3, 4, 9, 11], counts=[1, 2, 2, 7]), 1: dict(keys=[lecture_digest(x) for x in names],
                                                                     counts=[5, 5, 1, 9])}

    def group(rid, by_, *rest):
        st = group_stats(by[by_]["counts"])
        st.pop("median")
        order = sorted(range(4), key=lambda j: by[by_]["keys"][j])
        return group_hook(pkg, [by[by_]["keys"][j] for j in order], [by[by_]["counts"][j] for j in order],
                          dict(st, rows=12))(rid, by_, *rest)

    def tally_list(tid, min_events, keys, lens, events, valid, room, n, complete):
        n._obj.value, complete._obj.value = len(names), 1
        kb = (C.c_uint8 * (room * 32)).from_address(keys.value)
        ln = (C.c_uint32 * room).from_address(lens.value)
        for j, x in enumerate(names):
            kb[j * 32], ln[j] = x[0], 1

    def tally_info(tid, info):
        info._obj.used = len(names)

    def profile(rid, lec, llen, since, until, vf, sod, bins, rows, complete):
        arr = (C.c_uint64 * 168).from_address(bins.value)
        arr[0], arr[25], arr[26], complete._obj.value = 3, 1, 1, 1  # Monday 00h, Tuesday 01h and 02h

    ctx.hooks.update({"ske_rows_group": group, "ske_tally_list": tally_list, "ske_tally_info": tally_info,
                      "ske_rows_profile": profile})
    assert sc.exact_lecture_rankings(2) == {"most_attended": {"D": 9, "A": 5}, "least_attended": {"B": 5, "C": 1},
                                            "complete": True}
    ins = sc.exact_insights(lecture_k=1)
    assert [i["title"] for i in ins] == ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings",
                                         "Most Consistent Attendees", "Invalid Attendance Attempts"]
    assert all(i["complete"] is True for i in ins)
    assert ins[0]["data"] == {11: 7} and ins[0]["description"] == "Found 1 students who frequently arrive after 9:00 AM"
    assert ins[1]["data"] == {"Monday": 3, "Tuesday": 2}
    assert ins[2]["data"] == {"most_attended": {"D": 9}, "least_attended": {"C": 1}}
    assert ins[3]["data"] == {11: 7}  # median 2, std 2.71: above 4.71
    assert ins[4]["data"] == {-3: 1, 4: 2, 9: 2, 11: 7}
    assert len(sc.exact_insights(lecture_k=None)) == 4
    proc = pkg.AttendanceProcessor(cl, counts=sc)
    assert proc.insights(exact=True, k=1) == ins


def test_value_error_paths(pkg, stub_client):
    cl, ctx = stub_client
    plain = pkg.StudentCounts(cl, "a1", "i1")
    for call in (lambda: plain.exact_counts("attended"), plain.exact_by_day, plain.exact_lecture_rankings,
                 plain.exact_insights):
        with pytest.raises(ValueError, match="no records"):
            call()
    with pytest.raises(ValueError, match="records"):
        pkg.AttendanceProcessor(cl, counts=plain).insights(exact=True)
    nameless = pkg.StudentCounts(cl, "a2", "i2", records="table")
    with pytest.raises(ValueError, match="lecture_counts"):
        nameless.exact_lecture_rankings()
    with pytest.raises(ValueError, match="lecture_counts"):
        nameless.exact_insights()
    ctx.log.clear()
    before = pkg.AttendanceProcessor(cl, counts=nameless).insights()  # the default path is untouched
    assert before == [] and not group_calls(ctx)
