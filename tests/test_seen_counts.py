"""Counts that ignore repeats: ``StudentCounts(dedup=...)`` and
``AttendanceProcessor`` over streams with redelivered rows, against a
plain-Python group-by over the distinct (lecture, second, id) rows -- what the
reference's pandas group-bys see in its Cassandra table, where a redelivered
row overwrites itself (attendance_processor.py:64-72)."""
import collections
import json
from datetime import datetime

import numpy as np
import pytest

from test_processor import reference_messages

pytestmark = pytest.mark.gpu

DAY_NAMES = ("Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday", "Sunday")
LATE_FROM = 9 * 3600


def stream(seed=11, n_students=64):
    """A few hundred reference-style payloads over a few dozen students and
    lectures (three days, twelve rooms), in some other fast-path timestamp forms
    too; the generator's standalone invalid attempts repeat a row now and then."""
    roster, msgs = reference_messages(seed=seed, n_students=n_students, days=3)
    rng = np.random.default_rng(seed)
    out = []
    for k, m in enumerate(msgs):
        d = json.loads(m)
        d["lecture_id"] = "R%02d-%s" % (d["student_id"] % 12, d["lecture_id"][-8:])
        if d["student_id"] >= 100000:
            d["student_id"] = 10000 + d["student_id"] % 89  # five digits, off the roster or on it
        if rng.random() < 0.2:
            d["timestamp"] = d["timestamp"].replace("T", " ") + (".250", "+00:00")[k % 2]
        out.append(json.dumps(d).encode())
    return roster, out


def row_of(pkg, m):
    """(lecture bytes, epoch second, id bytes) of a message the reference's loop
    acknowledges, else None"""
    try:
        d = json.loads(m.decode())
        ts = datetime.fromisoformat(d["timestamp"])
        return str(d["lecture_id"]).encode(), int(pkg.epoch_seconds([ts])[0]), pkg.encode(d["student_id"])
    except Exception:
        return None


class GroupBy:
    """the reference's group-bys over distinct rows (``granularity`` 1), or over
    distinct (lecture, day, id) sessions"""

    def __init__(self, granularity=1):
        self.g, self.rows = granularity, {}

    def deliver(self, row, valid):
        lec, e, sid = row
        self.rows.setdefault((lec, e // self.g, sid), (e, bool(valid)))

    def tables(self):
        t = {k: collections.Counter() for k in ("att", "inv", "late", "day", "lec_ev", "lec_va")}
        for (lec, _, sid), (e, v) in self.rows.items():
            t["att" if v else "inv"][sid] += 1
            t["late"][sid] += e % 86400 >= LATE_FROM
            t["day"][DAY_NAMES[(e // 86400 + 3) % 7]] += 1
            t["lec_ev"][lec] += 1
            t["lec_va"][lec] += v
        t["late"] = +t["late"]
        return t


def options(prefix, **more):
    return dict(attended_key=prefix + ":att", invalid_key=prefix + ":inv", late_key=prefix + ":late",
                late_from=LATE_FROM, track_attended=1, track_invalid=1, track_late=1, capacity_log2=10,
                day_profile=prefix + ":week", lecture_counts=prefix + ":lectures", lecture_capacity_log2=10, **more)


def check_counts(sc, t, ids, lectures):
    assert sc.attended(ids).tolist() == [t["att"][s] for s in ids]
    assert sc.invalid(ids).tolist() == [t["inv"][s] for s in ids]
    assert sc.late(ids).tolist() == [t["late"][s] for s in ids]
    assert sc.by_day() == {d: c for d, c in sorted(t["day"].items())}
    ev, va = sc.lecture_events(lectures)
    assert ev.tolist() == [t["lec_ev"][x] for x in lectures] and va.tolist() == [t["lec_va"][x] for x in lectures]


def setup_bloom(pkg, client, roster):
    mbuf, moffs = pkg.pack_ints(roster)
    client.execute_command("BF.RESERVE", "bf:students", 0.001, 10000)
    client.bf_madd_packed("bf:students", mbuf, moffs)


def packed_rows(pkg, msgs, valid):
    """the decodable messages as ``count_packed`` takes them"""
    rows = [(i, row_of(pkg, m), m) for i, m in enumerate(msgs)]
    rows = [(i, r, m) for i, r, m in rows if r is not None]
    buf, offs = pkg.pack([r[2] for _, r, _ in rows])
    times = np.asarray([r[1] for _, r, _ in rows], np.int64)
    lectures = [r[0] for _, r, _ in rows]
    return buf, offs, valid[[i for i, _, _ in rows]], times, lectures


def test_redelivery(pkg, client):
    roster, msgs = stream()
    assert 200 < len(msgs) < 900
    setup_bloom(pkg, client, roster)
    once = pkg.StudentCounts(client, dedup="seen:once", dedup_capacity_log2=12, **options("once"))
    again = pkg.StudentCounts(client, dedup="seen:again", dedup_capacity_log2=12, **options("again"))
    naive = pkg.StudentCounts(client, **options("naive"))
    cut = len(msgs) // 2 + 3
    want = GroupBy()
    valid = np.zeros(len(msgs), bool)
    for lo, hi in ((0, cut), (cut, len(msgs))):
        v, status = once.update_messages("bf:students", msgs[lo:hi])
        assert (status == 0).all()
        valid[lo:hi] = v
        for m, ok in zip(msgs[lo:hi], v):
            want.deliver(row_of(pkg, m), ok)
    assert 0 < valid.sum() < len(msgs)
    third = msgs[1::3]
    for sc in (again, naive):
        for batch in (msgs[:cut], msgs[cut:], third):
            sc.update_messages("bf:students", batch)
        sc.count_packed(*packed_rows(pkg, msgs, valid))
    t = want.tables()
    n_distinct = len(want.rows)
    assert n_distinct < len(msgs)  # the stream itself repeats a row now and then
    ids = sorted(set(t["att"]) | set(t["inv"]))
    lectures = sorted(t["lec_ev"])
    assert len(ids) > 24 and len(lectures) > 24
    for sc in (once, again):
        check_counts(sc, t, ids, lectures)
    assert once.insights() == again.insights()
    titles = [i["title"] for i in once.insights()]
    assert titles == ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings",
                      "Most Consistent Attendees", "Invalid Attendance Attempts"]
    ins = {i["title"]: i for i in once.insights()}
    assert ins["Most Consistent Attendees"]["data"] == {s.decode(): c for s, c in t["att"].items()}
    assert ins["Invalid Attendance Attempts"]["data"] == {s.decode(): c for s, c in t["inv"].items()}
    assert ins["Attendance by Day"]["data"] == dict(sorted(t["day"].items()))
    assert once.duplicate_rows() == len(msgs) - n_distinct
    assert again.duplicate_rows() == 2 * len(msgs) + len(third) - n_distinct
    info = client.seen_info("seen:again")
    assert info["used"] == n_distinct and info["unplaced"] == 0
    # without the set the same deliveries count every time: the feature does something
    assert sum(naive.by_day().values()) == 2 * len(msgs) + len(third) != n_distinct
    assert naive.insights() != once.insights()
    ev, _ = naive.lecture_events(lectures)
    assert (ev > np.asarray([t["lec_ev"][x] for x in lectures])).all()


def test_sessions(pkg, client):
    """granularity 86400: a student counts once per lecture and UTC day"""
    roster, msgs = stream(seed=12)
    setup_bloom(pkg, client, roster)
    sc = pkg.StudentCounts(client, "s:att", "s:inv", dedup="seen:sessions", dedup_capacity_log2=12,
                           dedup_granularity=86400)
    assert sc.needs_times and sc.needs_lectures and not sc.timed and not sc.counts_lectures
    want, rows_seen = GroupBy(86400), GroupBy(1)
    for batch in (msgs, msgs[::2]):
        valid, _ = sc.update_messages("bf:students", batch)
        for m, ok in zip(batch, valid):
            want.deliver(row_of(pkg, m), ok)
            rows_seen.deliver(row_of(pkg, m), ok)
    t = want.tables()
    ids = sorted(set(t["att"]) | set(t["inv"]))
    sessions = collections.Counter()
    for (lec, day, sid), (_, v) in want.rows.items():
        sessions[sid] += v
    assert sc.attended(ids).tolist() == [sessions[s] for s in ids] == [t["att"][s] for s in ids]
    assert sc.invalid(ids).tolist() == [t["inv"][s] for s in ids]
    assert len(want.rows) < len(rows_seen.rows)  # entry and exit of a day are one session
    assert sc.duplicate_rows() == len(msgs) + len(msgs[::2]) - len(want.rows)


def test_processor(pkg, client):
    roster, msgs = stream(seed=13)
    setup_bloom(pkg, client, roster)
    cfg = pkg.AttendanceConfig(cassandra_row_types=False)
    sc = pkg.StudentCounts(client, "p:att", "p:inv", lecture_counts="p:lectures", lecture_capacity_log2=10,
                           dedup="seen:proc", dedup_capacity_log2=12)
    plain = pkg.StudentCounts(client, "q:att", "q:inv", lecture_counts="q:lectures", lecture_capacity_log2=10)
    proc = pkg.AttendanceProcessor(client, cfg, counts=sc)
    ref = pkg.AttendanceProcessor(client, cfg, counts=plain)
    third = len(msgs) // 3
    batches = [msgs[:third], msgs[third:2 * third], msgs[third:2 * third], msgs[2 * third:]]  # one batch repeated
    want = GroupBy()
    delivered = 0
    for batch in batches:
        rows, rows_ref = proc.process_batch(batch), ref.process_batch(batch)
        assert rows == rows_ref and len(rows) == len(batch)  # the rows and is_valid are unchanged by dedup
        delivered += len(rows)
        for m, r in zip(batch, rows):
            want.deliver(row_of(pkg, m), r["is_valid"])
    t = want.tables()
    for lec in sorted(t["lec_ev"])[:6]:
        stats = proc.get_attendance_stats(lec.decode())
        assert stats["attendance_record_count"] == t["lec_ev"][lec]
        assert stats["invalid_record_count"] == t["lec_ev"][lec] - t["lec_va"][lec]
        assert stats["duplicate_record_count"] == delivered - len(want.rows) > third - 10
        other = ref.get_attendance_stats(lec.decode())
        assert "duplicate_record_count" not in other
        assert other["attendance_record_count"] >= stats["attendance_record_count"]
    total = sum(ref.get_attendance_stats(lec.decode())["attendance_record_count"] for lec in t["lec_ev"])
    assert total == delivered


def test_host_decoded_messages(pkg, client):
    """Messages Python decodes (status 1) and undecodable ones (status -1) in the
    mix: the host-decoded rows take the count_packed route, and a row seen on
    one route is a repeat on the other."""
    roster, msgs = stream(seed=14)
    setup_bloom(pkg, client, roster)
    base = json.loads(msgs[0])
    lec, ts = base["lecture_id"], base["timestamp"][:19]
    digits = "".join("\\u003%s" % c for c in str(base["student_id"]))
    host = [b'{"student_id": "%s", "lecture_id": "%s", "timestamp": "%s"}' % (digits.encode(), lec.encode(),
                                                                               ts.encode()),  # msgs[0]'s row
            b'{"student_id": 123.5, "lecture_id": "R00-20250318", "timestamp": "2025-03-18T08:15:00"}',
            b'{"student_id": "\\u0031\\u0032345", "lecture_id": "R01-20250318", "timestamp": "2025-03-18T10:00:00.500"}']
    device_twin = b'{"student_id": 12345, "lecture_id": "R01-20250318", "timestamp": "2025-03-18 10:00:00"}'
    junk = [b"not json", b'{"student_id": 1}', b'{"student_id": 12345, "lecture_id": "L", "timestamp": "yesterday"}']
    rng = np.random.default_rng(14)
    mix = list(msgs[:300])
    for m in (host + junk) * 2:
        mix.insert(int(rng.integers(1, len(mix))), m)
    mix.append(device_twin)  # after its host-decoded twin
    sc = pkg.StudentCounts(client, dedup="seen:mix", dedup_capacity_log2=12, **options("mix"))
    want = GroupBy()
    delivered = 0
    for batch in (mix, mix[::-1]):
        valid, status = sc.update_messages("bf:students", batch)
        assert (status == 1).sum() == 6 and (status == -1).sum() == 6
        for m, ok, st in zip(batch, valid, status):
            row = row_of(pkg, m)
            assert (row is None) == (st == -1)
            if row is not None:
                want.deliver(row, ok)
                delivered += 1
    t = want.tables()
    assert b"123.5" in t["inv"] and t["inv"][b"123.5"] == 1
    ids = sorted(set(t["att"]) | set(t["inv"]))
    check_counts(sc, t, ids, sorted(t["lec_ev"]))
    # msgs[0] and its host-decoded form, the twin pair, each host message twice, and the second delivery
    assert sc.duplicate_rows() == delivered - len(want.rows)
    assert len(want.rows) <= 300 + 2
