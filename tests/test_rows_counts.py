"""The row log end to end: ``StudentCounts(records=...)`` and
``AttendanceProcessor`` over a few thousand messages with batches redelivered
whole and in part, against a plain-Python dict over the distinct (lecture,
second, id) rows with the last write kept -- what a read of the reference's
Cassandra table returns (attendance_processor.py:64-72, :154-165;
attendance_analysis.py:19-52)."""
import json
from datetime import datetime, timedelta

import numpy as np
import pytest

from test_seen_counts import options, row_of, setup_bloom, stream

pytestmark = pytest.mark.gpu


class Table:
    """the upsert: (lecture, second, integer id) -> the last is_valid written; a
    row whose id is no integer is refused"""

    def __init__(self):
        self.rows, self.delivered, self.refused = {}, 0, 0

    def deliver(self, row, valid):
        from rtsas_amd.client_rows import parse_id
        lec, e, sid = row
        self.delivered += 1
        v = parse_id(sid)
        if v is None:
            self.refused += 1
        else:
            self.rows[(lec, e, v)] = bool(valid)

    def of(self, lec):
        return sorted((e, i, v) for (x, e, i), v in self.rows.items() if x == lec)

    def lectures(self):
        return sorted({x for x, _, _ in self.rows})


def rows_of(rec):
    return list(zip(rec["epoch"].tolist(), rec["student_id"].tolist(), [bool(v) for v in rec["is_valid"]]))


def mixed(pkg, msgs, seed):
    """the stream with host-decoded and undecodable messages in it"""
    base = json.loads(msgs[0])
    digits = "".join("\\u003%s" % c for c in str(base["student_id"]))
    host = [b'{"student_id": "%s", "lecture_id": "%s", "timestamp": "%s"}'
            % (digits.encode(), base["lecture_id"].encode(), base["timestamp"][:19].encode()),  # msgs[0]'s row
            b'{"student_id": 123.5, "lecture_id": "R00-20250318", "timestamp": "2025-03-18T08:15:00"}',
            b'{"student_id": "\\u0031\\u0032345", "lecture_id": "R01-20250318", "timestamp": "2025-03-18T10:00:00.500"}']
    junk = [b"not json", b'{"student_id": 1}', b'{"student_id": 12345, "lecture_id": "L", "timestamp": "yesterday"}']
    rng = np.random.default_rng(seed)
    mix = list(msgs)
    for m in host + junk:
        mix.insert(int(rng.integers(1, len(mix))), m)
    return mix


@pytest.mark.parametrize("dedup", [True, False])
def test_update_messages_redelivered(pkg, client, dedup):
    roster, msgs = stream(seed=31, n_students=96)
    setup_bloom(pkg, client, roster)
    mix = mixed(pkg, msgs, 31)
    assert 200 < len(mix) < 2000
    more = dict(dedup="seen:a", dedup_capacity_log2=12) if dedup else {}
    sc = pkg.StudentCounts(client, records="table", records_capacity_log2=13, **options("a", **more))
    if dedup:
        more["dedup"] = "seen:b"
    plain = pkg.StudentCounts(client, **options("b", **more))
    want = Table()
    cut = len(mix) // 2 + 3
    for batch in (mix, mix[cut:], mix[1::3]):  # redelivered in part, twice
        valid, status = sc.update_messages("bf:students", batch)
        v2, s2 = plain.update_messages("bf:students", batch)
        assert np.array_equal(valid, v2) and np.array_equal(status, s2)  # the swipe half is untouched
        if batch is mix:
            assert (status == 1).sum() == 3 and (status == -1).sum() == 3
        for m, ok, st in zip(batch, valid, status):
            row = row_of(pkg, m)
            assert (row is None) == (st == -1)
            if row is not None:
                want.deliver(row, ok)
    info = sc.records_info()
    assert info["used"] + info["refused_ids"] + info["dropped"] == info["taken"] == want.delivered
    assert info["refused_ids"] == want.refused >= 1 and info["dropped"] == 0  # 123.5, once per delivery
    assert info["used"] > len(want.rows)  # the log keeps every delivery; the read collapses them
    lectures = want.lectures()
    assert len(lectures) > 24 and b"R01-20250318" in lectures
    for lec in lectures:
        rec = sc.records(lec)
        assert rows_of(rec) == want.of(lec) and rec["complete"], lec
    whole = sc.records()
    assert whole["epoch"].size == len(want.rows)
    assert 0 < whole["is_valid"].sum() < whole["is_valid"].size
    # the counters answer the same with and without the log
    ids = sorted({pkg.encode(i) for _, _, i in want.rows} | {b"123.5"})
    names = sorted(set(lectures) | {b"R00-20250318"})
    for q in (sc.attended, sc.invalid, sc.late):
        assert q(ids).tolist() == getattr(plain, q.__name__)(ids).tolist()
    assert sc.by_day() == plain.by_day()
    ev, va = sc.lecture_events(names)
    ev2, va2 = plain.lecture_events(names)
    assert ev.tolist() == ev2.tolist() and va.tolist() == va2.tolist()
    if dedup:  # the tally counts distinct rows: the lecture's records, but for the refused id's row
        assert plain.duplicate_rows() == sc.duplicate_rows()
        refused_lecture = b"R00-20250318"
        for lec, n_rows in zip(names, ev.tolist()):
            assert len(want.of(lec)) == n_rows - (1 if lec == refused_lecture else 0), lec
    else:
        assert int(ev.sum()) == want.delivered


def test_processor_records(pkg, client):
    from rtsas_amd.client_rows import lecture_digest
    roster, msgs = stream(seed=33)
    setup_bloom(pkg, client, roster)
    cfg = pkg.AttendanceConfig(cassandra_row_types=False)
    sc = pkg.StudentCounts(client, "p:att", "p:inv", lecture_counts="p:lectures", lecture_capacity_log2=10,
                           dedup="seen:proc", dedup_capacity_log2=12, records="p:table", records_capacity_log2=12)
    proc = pkg.AttendanceProcessor(client, cfg, counts=sc)
    third = len(msgs) // 3
    batches = [msgs[:third], msgs[third:2 * third], msgs[third:2 * third], msgs[2 * third:], msgs[5::7]]
    table = {}
    for batch in batches:
        rows = proc.process_batch(batch)
        assert len(rows) == len(batch)
        for r in rows:
            e = int(pkg.epoch_seconds([r["timestamp"]])[0])
            table[(r["lecture_id"], e, r["student_id"])] = r["is_valid"]  # the last write is kept

    def utc(e):
        return datetime(1970, 1, 1) + timedelta(seconds=e)

    lectures = sorted({k[0] for k in table})
    for lec in lectures[:8]:
        stats = proc.get_attendance_stats(lec)
        want = sorted((e, i) for (x, e, i) in table if x == lec)
        assert stats["attendance_records"] == [{"student_id": i, "timestamp": utc(e)} for e, i in want]
        assert stats["attendance_record_count"] == len(want)  # dedup: the tally counts the same distinct rows
    want = sorted((lecture_digest(x), e, i, x, v) for (x, e, i), v in table.items())
    assert proc.fetch_attendance_data() == [{"student_id": i, "lecture_id": x, "timestamp": utc(e), "is_valid": v}
                                            for _, e, i, x, v in want]
    assert proc.get_attendance_stats("no-such-lecture")["attendance_records"] == []


@pytest.mark.parametrize("width", [8, 4])
def test_update_fixed_ids(pkg, client, width):
    rng = np.random.default_rng(width)
    n = 3000
    lim = 1 << (8 * width - 1)
    vals = rng.integers(-lim, lim, n, dtype=np.int64)
    vals[:4] = (-lim, lim - 1, 0, -1)
    vals[n // 2:] = vals[:n - n // 2]  # every row twice
    ids = vals.astype("<i%d" % width).view(np.uint8).reshape(n, width)
    lectures = ["L%d" % (v % 7) for v in range(n // 2)] * 2
    times = np.concatenate([rng.integers(-50, 50, n // 2)] * 2).astype(np.int64)
    client.execute_command("BF.RESERVE", "bf:raw", 0.001, 10000)
    client.execute_command("BF.MADD", "bf:raw", *[ids[i].tobytes() for i in range(0, n // 2, 2)])
    slots = np.full(n, client.key_slot("hll:unique:x"), np.uint32)
    sc = pkg.StudentCounts(client, records="fixed", records_capacity_log2=12)
    with pytest.raises(ValueError):
        sc.update("bf:raw", slots, np.zeros((n, 5), np.uint8), times=times, lectures=lectures)
    assert sc.records_info()["taken"] == 0
    valid = sc.update("bf:raw", slots, ids, times=times, lectures=lectures)
    assert 0 < valid.sum() < n
    info = sc.records_info()
    assert (info["used"], info["taken"], info["refused_ids"], info["dropped"]) == (n, n, 0, 0)
    table = {(lec, int(e), int(i)): bool(v) for lec, e, i, v in zip(lectures, times, vals, valid)}
    assert len(table) == n // 2
    for lec in sorted(set(lectures)):
        assert rows_of(sc.records(lec)) == sorted((e, i, v) for (x, e, i), v in table.items() if x == lec)
    rec = sc.records("L3", since=-10, until=10)
    assert rows_of(rec) == sorted((e, i, v) for (x, e, i), v in table.items() if x == "L3" and -10 <= e < 10)
    # count_packed: the ids as text
    sc.count_packed(*pkg.pack([int(v) for v in vals[:100]]), valid[:100], times=times[:100], lectures=lectures[:100])
    assert sc.records_info()["used"] == n + 100 and sc.records()["epoch"].size == n // 2  # the same rows again
