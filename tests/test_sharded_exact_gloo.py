"""distributed.ShardedCounts' exact insights under gloo on CPU tensors, worlds 2
and 3.  The device ops are a numpy double (test infrastructure): a rank's
group-by is ``rows_group_oracle`` over its share of the rows, the merge is
``rows_group_merge_oracle``; the gather, padding, layout and formatting logic of
ShardedCounts and the real Collectives are the product code under test.  The
rows are split by lecture and one rank holds none.  Every rank's answers must be
those of one context fed every row; ranks that disagree on ``records`` raise on
every rank rather than hang."""
import os
import pickle
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from rows_group_cases import LATE, hand_batches
from rows_merge_cases import FILTERS, random_batch, split_by_lecture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATE_FROM = LATE + 1800


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def all_batches():
    return hand_batches() + [random_batch(300, 21)]


def owner_skipping_rank1(lecture, world):
    """rank 1 owns no lecture; the others share them by the name's bytes"""
    ranks = [r for r in range(world) if r != 1]
    return ranks[sum(str(lecture).encode()) % len(ranks)]


def share(rank, world):
    return split_by_lecture(all_batches(), world, owner_skipping_rank1)[rank]


def u8(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy())


class ExactOps:
    """what LibsketchCountsOps gives ShardedCounts, over plain values: no
    Count-Min key, no set, no profile; a tally (the lecture names) and a log"""
    device = torch.device("cpu")

    def __init__(self, batches, records=True):
        self.batches = batches
        self.cms_keys, self.sets, self.profile, self.tally = [], [], None, "lectures"
        self.keeps_records, self.late_from = records, LATE_FROM
        self.view_tally, self.log = None, []

    def config(self):
        return [0, self.late_from, 1, int(self.keeps_records), 10]

    def make_view(self, suffix, world, capacity_log2=None, lecture_capacity_log2=None):
        self.world, self.view_tally = world, {}
        return self.view_tally

    def sync(self):
        pass

    # -- the tally, as far as the names need it
    def tally_export(self):
        names = sorted({str(x).encode() for b in self.batches for x in b[0]})
        a = np.zeros((len(names), 32), np.uint8)
        for j, k in enumerate(names):
            a[j, :len(k)] = np.frombuffer(k, np.uint8)
        lens = np.asarray([len(k) for k in names], np.uint32)
        ev = np.ones(len(names), np.uint64)
        return (u8(a), u8(lens), u8(ev), u8(ev), len(names), 0, 0, 0)

    def tally_reset(self):
        self.view_tally.clear()

    def tally_merge(self, keys, lens, events, valid, n, dropped_events, dropped_valid, overflow):
        if n:
            a, ln = keys.contiguous().numpy().reshape(-1, 32), lens.contiguous().numpy().view(np.uint32)
            for j in range(n):
                self.view_tally[a[j, :ln[j]].tobytes()] = 1

    def view_lecture_names(self):
        return sorted(self.view_tally)

    # -- the log's group-bys
    def rows_group_export(self, which):
        from rtsas_amd.client_rows import rows_group_oracle
        kw = dict(by="lecture") if which == "lectures" else dict(
            by="student", **{k: (LATE_FROM if k == "late_from" else v) for k, v in FILTERS[which].items()})
        g = rows_group_oracle(self.batches, **kw)
        self.log.append(("export", which, int(g["keys"].size)))
        return u8(g["keys"]), u8(g["counts"]), int(g["keys"].size), g["stats"]["rows"], 1

    def rows_profile_read(self):
        from rtsas_amd.client_rows import rows_profile_oracle
        return rows_profile_oracle(self.batches).reshape(-1)

    def rows_group_merge(self, by, keys_u8, counts_u8, n_in, groups=True):
        from rtsas_amd.client_rows import rows_group_merge_oracle
        assert keys_u8.dtype == torch.uint8 and keys_u8.is_contiguous() and counts_u8.is_contiguous()
        assert keys_u8.numel() == counts_u8.numel() == 8 * n_in and n_in % (4 * self.world) == 0
        k, c = keys_u8.numpy().view(np.uint64), counts_u8.numpy().view(np.uint64)
        assert not k[c == 0].any()  # a pad is (key 0, count 0)
        self.log.append(("merge", by, n_in, groups))
        part = {"keys": k.view(np.int64) if by == "student" else k, "counts": c}
        m = rows_group_merge_oracle([part], by)
        m["stats"].pop("median")
        none = np.zeros(0, np.uint64)
        return (m["keys"].view(np.uint64) if groups else none, m["counts"] if groups else none, m["stats"],
                m["multi"])


def one_context(k):
    """what a StudentCounts fed every row answers, from the oracles alone"""
    from rtsas_amd.analysis import DAY_NAMES, reference_rule
    from rtsas_amd.client_rows import lecture_digest, rows_group_oracle, rows_profile_oracle
    batches = all_batches()
    counts = {w: rows_group_oracle(batches, "student", **{a: (LATE_FROM if a == "late_from" else v)
                                                          for a, v in FILTERS[w].items()}) for w in FILTERS}
    late, att, inv = counts["late"], counts["attended"], counts["invalid"]
    twice = late["stats"]["med_lo"] + late["stats"]["med_hi"]
    per_day = rows_profile_oracle(batches).sum(axis=1)
    by_day = {d: int(per_day[i]) for d, i in sorted((d, i) for i, d in enumerate(DAY_NAMES)) if per_day[i]}
    names = sorted({str(x) for b in batches for x in b[0]})
    lec = rows_group_oracle(batches, "lecture")
    by_digest = {lecture_digest(x): x for x in names}
    ranked = sorted((-c, by_digest[d]) for d, c in zip(lec["keys"].tolist(), lec["counts"].tolist()))
    ranks = {"most_attended": {x: -c for c, x in ranked[:k]}, "least_attended": {x: -c for c, x in ranked[-k:]}}
    thr = reference_rule(att["stats"], "median+std")
    data = [{i: c for i, c in zip(late["keys"].tolist(), late["counts"].tolist()) if 2 * c > twice}, by_day, ranks,
            {i: c for i, c in zip(att["keys"].tolist(), att["counts"].tolist()) if thr is not None and c >= thr},
            dict(zip(inv["keys"].tolist(), inv["counts"].tolist()))]
    return {"counts": counts, "by_day": by_day, "ranks": ranks, "data": data}


def _worker(rank, world, port, out_dir, mismatch):
    import sys
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    ge.load_package()
    from rtsas_amd.distributed import ShardedCounts
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    res = {}
    if mismatch:
        try:
            ShardedCounts(None, rank, world, ops=ExactOps(share(rank, world), records=rank != world - 1))
            res["raised"] = None
        except ValueError as e:
            res["raised"] = str(e)
    else:
        ops = ExactOps(share(rank, world))
        sc = ShardedCounts(None, rank, world, ops=ops)
        res["keeps_records"] = sc.keeps_records
        res["counts"] = {w: sc.exact_counts(w) for w in FILTERS}
        res["stats_only"] = sc.exact_counts("attended", groups=False)
        res["by_day"] = sc.exact_by_day()
        res["names_before_merge"] = ops.view_lecture_names()
        sc.merge()
        res["ranks"] = sc.exact_lecture_rankings(2)
        ops.log.clear()
        res["insights"] = sc.exact_insights(2)
        res["log"] = list(ops.log)
        res["rows_here"] = sum(len(b[1]) for b in ops.batches)
    dist.barrier()
    with open(os.path.join(out_dir, f"rank{rank}.pkl"), "wb") as f:
        pickle.dump(res, f)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_answers_as_one_context(pkg, tmp_path, world):
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), False), nprocs=world, join=True)
    want = one_context(2)
    assert all(len(d) > 0 for d in want["data"])
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.pkl", "rb") as f:
            res = pickle.load(f)
        assert res["keeps_records"] is True
        assert (res["rows_here"] == 0) == (rank == 1)  # one rank holds no rows
        for which, w in want["counts"].items():
            got = res["counts"][which]
            assert got["keys"].dtype == np.int64 and got["counts"].dtype == np.uint64
            assert np.array_equal(got["keys"], w["keys"]) and np.array_equal(got["counts"], w["counts"]), (rank, which)
            assert got["stats"] == w["stats"], (rank, which)
            assert got["complete"] is True and got["split_lectures"] == 0
        so = res["stats_only"]
        assert so["keys"].size == 0 and so["stats"] == want["counts"]["attended"]["stats"]
        assert res["by_day"] == want["by_day"]
        assert res["names_before_merge"] == []  # the names are the view's, as of the last merge()
        assert res["ranks"] == dict(want["ranks"], complete=True, split_lectures=0)
        ins = res["insights"]
        assert [i["title"] for i in ins] == ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings",
                                             "Most Consistent Attendees", "Invalid Attendance Attempts"]
        assert [i["data"] for i in ins] == want["data"], rank
        assert all(i["complete"] is True and i["split_lectures"] == 0 for i in ins)
        assert ins[0]["description"] == f"Found {len(want['data'][0])} students who frequently arrive after 9:00 AM"
        # one export and one merge per group-by; the by-lecture merge runs once for all five entries
        assert [e[1] for e in res["log"] if e[0] == "export"] == ["lectures", "late", "attended", "invalid"]
        merges = [e for e in res["log"] if e[0] == "merge"]
        assert [m[1] for m in merges] == ["lecture", "student", "student", "student"]
        assert all(m[2] % (4 * world) == 0 and m[3] for m in merges)


def test_mismatched_records_raise_on_every_rank(pkg, tmp_path):
    world = 3
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), True), nprocs=world, join=True)
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.pkl", "rb") as f:
            res = pickle.load(f)
        assert res["raised"] is not None and "differ" in res["raised"], rank


def test_one_rank_and_no_records(pkg):
    """world == 1 needs no process group; without records every exact call is a ValueError"""
    from rtsas_amd.distributed import ShardedCounts
    assert not dist.is_initialized()
    ops = ExactOps(all_batches())
    sc = ShardedCounts(None, 0, 1, ops=ops)
    want = one_context(3)
    assert [i["data"] for i in sc.exact_insights()] == want["data"]
    assert len(sc.exact_insights(lecture_k=None)) == 4
    got = sc.exact_counts("late")
    assert np.array_equal(got["counts"], want["counts"]["late"]["counts"]) and got["split_lectures"] == 0
    with pytest.raises(ValueError):
        sc.exact_counts("present")
    plain = ShardedCounts(None, 0, 1, ops=ExactOps(all_batches(), records=False))
    assert plain.keeps_records is False
    for call in (lambda: plain.exact_counts("attended"), plain.exact_by_day, plain.exact_lecture_rankings,
                 plain.exact_insights):
        with pytest.raises(ValueError, match="no records"):
            call()


def test_config_carries_keeps_records(pkg):
    """the real LibsketchCountsOps.config() over a context stub: counts with and without a row log
    differ in exactly the keeps_records word, so ranks that disagree meet the constructor's ValueError"""
    from facade_stub import StubContext
    from rtsas_amd.distributed import LibsketchCountsOps
    words = []
    for records in (None, "table"):
        ctx = StubContext(pkg.load_library())
        ctx.device = 0
        cl = pkg.SketchClient(decode_responses=True, context=ctx)
        ops = LibsketchCountsOps(pkg.StudentCounts(cl, "a", "i", records=records, lecture_counts="lectures"))
        assert ops.keeps_records is (records is not None)
        words.append([int(x) for x in ops.config()])
    without, with_log = words
    assert len(without) == len(with_log)
    differ = [j for j, (a, b) in enumerate(zip(without, with_log)) if a != b]
    assert differ == [len(without) - 3] and (without[-3], with_log[-3]) == (0, 1)
