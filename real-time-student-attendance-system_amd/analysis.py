"""Per-student counters beside the swipe path.

The reference's analysis answers "Most Consistent Attendees"
(attendance_analysis.py:99-109) and "Invalid Attendance Attempts" (:111-118)
with pandas group-bys over the Cassandra rows its processor wrote.  Here the
processor keeps no per-event store; ``StudentCounts`` keeps two Count-Min
Sketch keys instead, updated on the device from the very ids and answers the
fused swipe kernel just produced, so the per-swipe valid bytes never cross to
the host to be grouped.

A Count-Min estimate never undercounts; it overcounts by at most
``error * count`` with probability ``1 - probability`` (CMS.INITBYPROB).

The reference's two insights are lists, and the invalid ids are on no roster a
caller could enumerate.  With ``track_attended`` / ``track_invalid`` set, each
key gets a heavy-hitter set (client_hh.py, DESIGN.md "Heavy hitters"): every
batch's ids whose estimate reached the threshold are kept on the device, and
``top_attended`` / ``top_invalid`` / ``insights`` list them.

"Habitual Latecomers" (:65-75) and "Attendance by Day" (:77-85) need each
swipe's time.  With ``late_key`` / ``day_profile`` set, ``update`` takes the
times too: a time profile (client_tp.py, DESIGN.md "Time profile") counts the
swipes per weekday and hour and marks the late ones on the device, and that
mark is the mask of a third Count-Min key, the late swipes per student.

The reference has none of this as arrays; it has JSON messages.
``update_messages`` takes those: the device decodes them (client_ingest.py),
timestamps included, and the decoded ids, answers and times feed the same
counters in place (DESIGN.md "Insights from the message stream");
``count_packed`` is the counting alone, for swipes already answered.

Every counter adds one per row it is given, and an at-least-once transport
gives some rows twice.  With ``dedup`` set, a seen-row set (client_seen.py,
DESIGN.md "Seen rows") answers per row whether it was counted before, and only
first sightings reach the counters -- the reference's analytics read a
Cassandra table in which a redelivered row overwrites itself.

That table's rows have a counterpart too.  With ``records`` set, a row log
(client_rows.py, DESIGN.md "Row log") keeps every row the counting calls are
given -- (lecture, time, student id, is_valid), in arrival order, on the
device -- and ``records`` reads a lecture's rows back in the table's order,
each row once with its last write.  Over those rows ``exact_insights`` runs the
reference's five group-bys themselves on the device (DESIGN.md "Row log
group-by"): no estimate, no track threshold, repeats collapsed by the log.
"""
from __future__ import annotations

import ctypes as C
import math
from datetime import datetime, timedelta, timezone

import numpy as np

from ._lib import IngestCols, IngestDense, SKE_MEM_DEVICE, SKE_SEEN_FIRST
from .client_ingest import join_messages
from .encoding import encode, pack
from .engine import DeviceBuffer, hh_list, tally_query


DAY_NAMES = ("Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday", "Sunday")
_EPOCH = datetime(1970, 1, 1)
_EPOCH_UTC = datetime(1970, 1, 1, tzinfo=timezone.utc)
_SECOND = timedelta(seconds=1)


def epoch_seconds(times) -> np.ndarray:
    """Swipe times as int64 seconds since 1970-01-01T00:00:00 UTC, floored.

    An integer array is taken as it is; a ``datetime64`` array of any unit is
    floored to seconds; a sequence of ``datetime`` objects: a naive one is UTC
    as written, an aware one is converted to UTC, fractions are floored (also
    before 1970).  This is what Cassandra keeps of the timestamps the
    reference's processor inserts (attendance_processor.py:106, :116-124), and
    the convention of the ingest kernel's UTC day."""
    a = times if isinstance(times, np.ndarray) else np.asarray(times)
    if a.size == 0:
        return np.zeros(0, np.int64)
    if a.dtype.kind in "iu":
        return np.ascontiguousarray(a, dtype=np.int64).reshape(-1)
    if a.dtype.kind == "M":
        return np.ascontiguousarray(a.astype("datetime64[s]").astype(np.int64)).reshape(-1)
    if a.dtype.kind != "O":
        raise TypeError("times are int64 seconds, datetime64 values or datetime objects")
    out = np.empty(a.size, np.int64)
    for i, t in enumerate(a.reshape(-1)):
        if not isinstance(t, datetime):
            raise TypeError("times are int64 seconds, datetime64 values or datetime objects")
        out[i] = (t - (_EPOCH if t.tzinfo is None else _EPOCH_UTC)) // _SECOND
    return out


def reference_rule(stats: dict, rule: str):
    """The smallest integer estimate that passes one of the reference's two
    population rules, from ``hh_stats``' exact integers (``n``, ``sum``,
    ``sumsq``, ``median``); None when nothing can pass.

    ``"median"``: ``est > median`` (attendance_analysis.py:69).  Twice the
    median is the integer M = med_lo + med_hi, so the rule is ``2 * est > M``.

    ``"median+std"``: ``est > median + std`` (:101-103), std the sample
    standard deviation sqrt(V / k) with V = n * sumsq - sum * sum and
    k = n * (n - 1).  With x = 2 * est - M the rule reads x > 2 * sqrt(V / k):
    x is positive and x * x * k > 4 * V.  x * x is an integer, so that is
    x * x > floor(4 * V / k), i.e. x >= isqrt(floor(4 * V / k)) + 1 -- Python
    ints throughout, no float is compared.  ``n == 1``: pandas' std is NaN and
    nothing compares greater."""
    n = int(stats["n"])
    if rule not in ("median", "median+std"):
        raise ValueError('rule is "median" or "median+std"')
    if n == 0:
        return None
    twice_median = int(round(2 * stats["median"]))  # med_lo + med_hi: exact, both below 2^32
    if rule == "median":
        return twice_median // 2 + 1
    if n == 1:
        return None
    s = int(stats["sum"])
    x = math.isqrt(4 * (n * int(stats["sumsq"]) - s * s) // (n * (n - 1))) + 1
    return (x + twice_median + 1) // 2


def exact_by_day_format(bins) -> dict:
    """``{day name: rows}`` of the weekdays that have any, in the order of the
    names, from the ``[7, 24]`` (or 168) weekday-by-hour bins of the log's rows."""
    per_day = np.asarray(bins).reshape(7, 24).sum(axis=1)
    return {d: int(per_day[i]) for d, i in sorted((d, i) for i, d in enumerate(DAY_NAMES)) if per_day[i]}


def exact_rankings_format(g: dict, names, k: int = 3) -> dict:
    """The by-lecture group-by ``g`` as ``lecture_rankings`` writes it: the
    digests joined to the tally listing's ``names`` (a digest none of them has
    shows as ``"#<hex digest>"``), count descending, name ascending; carries
    ``g``'s ``complete``."""
    from .client_rows import lecture_digest
    by_digest = {lecture_digest(key): key.decode("utf-8", "replace") for key in names}
    ranked = sorted((-int(c), by_digest.get(int(d), "#%016x" % int(d))) for d, c in zip(g["keys"], g["counts"]))
    k = int(k)
    return {"most_attended": {name: -c for c, name in ranked[:k]},
            "least_attended": {name: -c for c, name in ranked[max(len(ranked) - k, 0):]} if k > 0 else {},
            "complete": g["complete"]}


def exact_insight_entries(late: dict, by_day: dict, ranks, att: dict, inv: dict, late_from: int) -> list:
    """The five exact entries from their answers: the per-student group-bys of
    the late, of all and of the invalid rows (``rows_group``'s dicts), the
    ``{day name: rows}`` dict and the rankings (None: no lecture entry).  One
    context (``StudentCounts.exact_insights``) and the ranks' merge
    (``distributed.ShardedCounts.exact_insights``) both end here.  An entry
    carries its answer's ``complete`` and, where the answer has one, its
    ``split_lectures``."""
    def marks(src):
        return {key: src[key] for key in ("complete", "split_lectures") if key in src}

    twice = late["stats"]["med_lo"] + late["stats"]["med_hi"]
    data = {int(i): int(c) for i, c in zip(late["keys"], late["counts"]) if 2 * int(c) > twice}
    out = [{"title": "Habitual Latecomers",
            "description": f"Found {len(data)} students who frequently arrive after {late_from // 3600}:00 AM",
            "data": data, **marks(late)},
           {"title": "Attendance by Day", "description": "Distribution of attendance across different days",
            "data": by_day, **marks(late)}]
    if ranks is not None:
        out.append({"title": "Lecture Attendance Rankings", "description": "Most and least attended lectures",
                    "data": {"most_attended": ranks["most_attended"], "least_attended": ranks["least_attended"]},
                    **marks(ranks)})
    thr = reference_rule(att["stats"], "median+std")
    out.append({"title": "Most Consistent Attendees",
                "description": "Students whose estimated attendance reaches the threshold",
                "data": {int(i): int(c) for i, c in zip(att["keys"], att["counts"])
                         if thr is not None and int(c) >= thr},
                **marks(att)})
    out.append({"title": "Invalid Attendance Attempts",
                "description": "Estimated invalid attendance attempts by student id",
                "data": {int(i): int(c) for i, c in zip(inv["keys"], inv["counts"])}, **marks(inv)})
    return out


class StudentCounts:
    """Attended / invalid swipe counts per student id, as two CMS keys of a
    ``SketchClient``.

    ``track_attended`` / ``track_invalid`` (default None: off, ``update``
    enqueues exactly the swipes and the two adds): a count from which a
    student is kept in the key's heavy-hitter set of ``2 ** capacity_log2``
    slots.  Guarantee, while the listing says ``complete``: every id whose true
    count reaches ``threshold`` is listed by ``top_*(threshold=threshold)`` for
    any ``threshold`` at or above the track threshold -- at the batch of its
    last swipe its estimate was at least its true count, so it joined the set
    then at the latest, and estimates never fall.  Ids are at most 16 bytes;
    ids with equal 64-bit digests share one entry.

    ``late_key`` (default None: off): a third CMS key that counts, per
    student, the swipes -- valid or not, as the reference counts them -- whose
    UTC second of the day is at least ``late_from``; ``track_late`` keeps its
    heavy-hitter set.  ``day_profile``: the name of a time profile
    (``client.tp_create``; made here when it does not exist) that counts every
    swipe by weekday and hour.  With either set ``update`` needs the swipes'
    times; with only ``late_key`` the profile is named ``b"tp:" + late_key``.

    ``lecture_counts`` (default None: off): the name of a tally
    (``client.tally_create``; made here with ``2 ** lecture_capacity_log2``
    slots when it does not exist) that counts every swipe, valid or not, by
    lecture -- the reference's ``groupby('lecture_id').size()``
    (attendance_analysis.py:87-97) -- and the valid ones beside.  The group key
    is the text ``keyspace.day_key`` puts into the key name,
    ``str(lecture_id).encode()``, at most 32 bytes.  With it set ``update`` and
    ``count_packed`` need the swipes' ``lectures``; ``update_messages`` reads
    them from the messages.

    ``dedup`` (default None: off): the name of a seen-row set
    (``client.seen_create``; made here with ``2 ** dedup_capacity_log2`` slots
    when it does not exist).  The counting half of ``update``, ``count_packed``
    and ``update_messages`` then counts a row -- (lecture, id,
    ``floor(epoch / dedup_granularity)``) -- only at its first sighting, so a
    redelivered row counts once, as it does in the reference's Cassandra table
    (``PRIMARY KEY ((lecture_id), timestamp, student_id)``,
    attendance_processor.py:64-72).  ``dedup_granularity=86400`` counts a
    student once per lecture and UTC day.  The swipe half (BF.EXISTS, PFADD)
    still runs on every row and the returned validity is unchanged.  With it
    set the counting calls need the swipes' times and lectures whether or not
    the time and lecture options are on (``needs_times`` / ``needs_lectures``).
    A set that is full answers "first": a count is never lost.

    ``records`` (default None: off): the name of a row log
    (``client.rows_create``; made here with ``2 ** records_capacity_log2`` rows
    when it does not exist), the counterpart of the reference's Cassandra
    table.  ``update``, ``count_packed`` and ``update_messages`` then append
    every row they are given -- every acknowledged row, valid or not, before any
    ``dedup`` compaction; the log collapses repeats itself when it is read
    (``records``).  The id must be an integer: ``update`` takes 4- or 8-byte
    little-endian ids only, the other calls the id's canonical decimal text;
    anything else is refused and counted (``records_info()["refused_ids"]``).
    With it set the counting calls need the swipes' times and lectures.

    ``records_compact`` (default False): make room in the log instead of
    dropping rows.  ``StudentCounts`` then keeps a host-side upper bound of the
    log's ``used`` -- the log's own count when this object is made, plus the
    ``n`` of every append it enqueues -- and never waits for the device on the
    append path to learn it.  When the bound plus the next batch would pass the
    capacity it first calls ``compact_records(records_keep_since)`` (superseded
    rows leave, and those older than ``records_keep_since``: seconds, or
    anything ``epoch_seconds`` takes; None expires nothing) and continues from
    the exact ``kept``.  A batch that still does not fit is appended all the
    same and fails open as without the option.  Replays of an append graph the
    caller recorded bypass the bound: call ``compact_records`` after them."""

    def __init__(self, client, attended_key="cms:attended", invalid_key="cms:invalid",
                 error: float = 0.001, probability: float = 0.01, track_attended: int | None = None,
                 track_invalid: int | None = None, capacity_log2: int = 16, late_key=None,
                 late_from: int = 9 * 3600, track_late: int | None = None, day_profile=None,
                 lecture_counts=None, lecture_capacity_log2: int = 16, dedup=None,
                 dedup_capacity_log2: int = 22, dedup_granularity: int = 1, records=None,
                 records_capacity_log2: int = 22, records_compact: bool = False, records_keep_since=None):
        self.client = client
        self._records = encode(records) if records is not None else None
        if records_compact and records is None:
            raise ValueError("records_compact needs records")
        self._rec_compact, self._rec_keep = bool(records_compact), records_keep_since
        self._dedup = encode(dedup) if dedup is not None else None
        self._dedup_gran = int(dedup_granularity)
        if self._dedup_gran < 1:
            raise ValueError("dedup_granularity is at least 1 second")
        self._lectures = encode(lecture_counts) if lecture_counts is not None else None
        self._lec_bufs = None
        self.attended_key, self.invalid_key = attended_key, invalid_key
        self.late_key, self.late_from = late_key, int(late_from)
        if not 0 <= self.late_from <= 86400:
            raise ValueError("late_from is a second of the day, 0 to 86400")
        if track_late is not None and late_key is None:
            raise ValueError("track_late needs a late_key")
        for key in (attended_key, invalid_key) + ((late_key,) if late_key is not None else ()):
            if client.keys.type_of(encode(key)) is None:
                client.cms_initbyprob(key, error, probability)
            client.keys.expect(encode(key), "cms")  # WRONGTYPE for a key of another kind
        self._bufs = None
        self._pk_bufs: dict[str, dict] = {}  # _packed_buffers
        # per key: (set name, track threshold, the mask value its swipes carry)
        self._tracks = []
        for key, thr, want in ((attended_key, track_attended, 1), (invalid_key, track_invalid, 0)):
            if thr is None:
                continue
            if int(thr) < 1:
                raise ValueError("a track threshold is at least 1")
            name = b"hh:" + encode(key)
            client.hh_create(name, key, capacity_log2)
            self._tracks.append((name, int(thr), want))
        # the late key's set reads the late bytes, not K1's answers
        self._late_track = None
        if track_late is not None:
            if int(track_late) < 1:
                raise ValueError("a track threshold is at least 1")
            name = b"hh:" + encode(late_key)
            client.hh_create(name, late_key, capacity_log2)
            self._late_track = (name, int(track_late), 1)
        self._day_insight = day_profile is not None
        self._profile = None
        if day_profile is not None or late_key is not None:
            self._profile = encode(day_profile) if day_profile is not None else b"tp:" + encode(late_key)
            if self._profile not in client._tp:
                client.tp_create(self._profile)
        if self._lectures is not None and self._lectures not in client._tally:
            client.tally_create(self._lectures, lecture_capacity_log2)
        if self._dedup is not None and self._dedup not in client._seen:
            client.seen_create(self._dedup, dedup_capacity_log2)
        if self._records is not None and self._records not in client._rows:
            client.rows_create(self._records, records_capacity_log2)
        if self._rec_compact:  # the one wait: an existing log says where it stands
            info = client.rows_info(self._records)
            self._rec_cap, self._rec_bound = info["capacity"], info["used"]

    def _buffers(self, n: int, width: int):
        b = self._bufs
        if b is None or b[0] < n or b[1] < width:
            if b is not None:
                for x in b[2:]:
                    x.free()
            cn, cw = max(n, 1024), max(width, 8)
            ctx = self.client.ctx
            b = (cn, cw, DeviceBuffer(ctx, cn * cw + 64), DeviceBuffer(ctx, cn * 4 + 16),
                 DeviceBuffer(ctx, cn + 16))
            if self._profile is not None:  # the times and the late bytes
                b += (DeviceBuffer(ctx, cn * 8 + 16), DeviceBuffer(ctx, cn + 16))
            self._bufs = b
        return b[2:]

    def _check_lectures(self, lectures, n: int):
        """The swipes' lectures as a packed batch ``(buf, offs)`` (None when
        the option is off): a packed pair is taken as it is, a sequence is
        encoded as ``keyspace.day_key`` names the lecture, ``str(x).encode()``."""
        if (lectures is None) != (not self.needs_lectures):
            raise ValueError("lectures go with lecture_counts (or dedup): required with it, refused without")
        if lectures is None:
            return None
        if isinstance(lectures, tuple) and len(lectures) == 2 and isinstance(lectures[1], np.ndarray):
            buf = np.ascontiguousarray(lectures[0], dtype=np.uint8).reshape(-1)
            offs = np.ascontiguousarray(lectures[1], dtype=np.uint32).reshape(-1)
        else:
            buf, offs = pack([x if isinstance(x, bytes) else str(x) for x in lectures])
        if offs.size != n + 1:
            raise ValueError("one lecture per id")
        return buf, offs

    def _enqueue_lectures(self, lec, n: int, d_valid) -> None:
        """Upload the packed lectures and enqueue their tally add, masked by
        the swipes' valid bytes (on the device already)."""
        buf, offs = lec
        nbytes = int(offs[-1])
        b = self._lec_bufs
        if b is None or b[0] < n or b[1] < nbytes:
            if b is not None:
                for x in b[2:]:
                    x.free()
            cn, cb = max(n, 1024), max(nbytes, 1 << 14)
            ctx = self.client.ctx
            b = (cn, cb, DeviceBuffer(ctx, cb + 64), DeviceBuffer(ctx, (cn + 1) * 4))
            self._lec_bufs = b
        b[2].from_host(buf[:nbytes])
        b[3].from_host(offs)
        cl = self.client
        cl.ctx.call("ske_tally_add_packed_async", cl.tally_tid(self._lectures), C.c_void_p(b[2].ptr),
                    C.c_void_p(b[3].ptr), n, C.c_void_p(d_valid.ptr))

    def update(self, bf_key, slots: np.ndarray, ids: np.ndarray, times=None, lectures=None) -> np.ndarray:
        """One batch of swipes: ``client.swipes_fixed`` semantics (BF.EXISTS
        of every id, PFADD of the valid ones into their HLL slot), then every
        valid swipe's id counts in the attended key and every invalid one's
        in the invalid key.  ``ids``: [n, width] uint8, ``slots``: one HLL
        slot per swipe (``client.key_slot``).  ``times`` (one per swipe, any
        form ``epoch_seconds`` takes; required with ``late_key`` or
        ``day_profile``, refused without): every swipe counts in the profile,
        every late one's id in the late key.  ``lectures`` (one per swipe, a
        sequence or a packed ``(buf, offs)``; required with ``lecture_counts``,
        refused without): every swipe counts under its lecture.  Returns the
        validity (bool)."""
        cl = self.client
        ids = np.ascontiguousarray(ids, dtype=np.uint8)
        if ids.ndim != 2:
            raise ValueError("ids must be a [n, width] uint8 array")
        n, width = ids.shape
        if self._records is not None and width not in (4, 8):
            raise ValueError("with records an id is a 4- or 8-byte little-endian integer")
        ep = self._check_times(times, n)
        lec = self._check_lectures(lectures, n)
        if n == 0 or width == 0:
            return np.zeros(n, bool)
        if self._dedup is not None:
            return self._update_dedup(bf_key, slots, ids, ep, lec)
        rows = (ep, lec)  # the log's columns; the counters take theirs only where their option is on
        ep, lec = ep if self.timed else None, lec if self.counts_lectures else None
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        if s.shape != (n,):
            raise ValueError("one slot per id")
        d_ids, d_slots, d_valid, *d_time = self._buffers(n, width)
        d_ids.from_host(ids)
        d_slots.from_host(s)
        if ep is not None:
            d_time[0].from_host(ep)
        bkey = encode(bf_key)
        if cl.keys.expect(bkey, "bf"):
            cl.ctx.call("ske_swipes_fixed", cl.keys.fid[bkey], C.c_void_p(d_slots.ptr), C.c_void_p(d_ids.ptr),
                        width, n, C.c_void_p(d_valid.ptr), SKE_MEM_DEVICE)
        else:
            d_valid.from_host(np.zeros(n, np.uint8))  # BF.EXISTS of a missing key answers 0
        if self._records is not None:  # every row, with K1's answers where they are
            self._records_room(n)
            cl.rows_enqueue(cl.rows_rid(self._records), rows[1], rows[0], fixed_ids=ids, d_valid=d_valid)
        for key, want in ((self.attended_key, 1), (self.invalid_key, 0)):
            cl.ctx.call("ske_cms_add_fixed_async", cl.cms_cid(key), C.c_void_p(d_ids.ptr), width, n,
                        None, C.c_void_p(d_valid.ptr), want)
        if ep is not None:  # every swipe into the profile; the late bytes mask the late key's add
            d_epoch, d_late = d_time
            late = self.late_key is not None
            cl.ctx.call("ske_tp_add_async", cl.tp_tid(self._profile), C.c_void_p(d_epoch.ptr), n, None, 1,
                        self.late_from, C.c_void_p(d_late.ptr) if late else None)
            if late:
                cl.ctx.call("ske_cms_add_fixed_async", cl.cms_cid(self.late_key), C.c_void_p(d_ids.ptr), width, n,
                            None, C.c_void_p(d_late.ptr), 1)
        for name, thr, want in self._tracks:  # behind the adds: the estimates include this batch
            hid, cid = cl._hh_entry(name)
            cl.ctx.call("ske_hh_track_fixed_async", hid, cid, C.c_void_p(d_ids.ptr), width, n,
                        C.c_void_p(d_valid.ptr), want, thr)
        if self._late_track is not None:
            name, thr, want = self._late_track
            hid, cid = cl._hh_entry(name)
            cl.ctx.call("ske_hh_track_fixed_async", hid, cid, C.c_void_p(d_ids.ptr), width, n,
                        C.c_void_p(d_time[1].ptr), want, thr)
        if lec is not None:  # every swipe by its lecture, the valid ones beside
            self._enqueue_lectures(lec, n, d_valid)
        cl.ctx.call("ske_sync")
        return d_valid.to_host(np.uint8, n).astype(bool)

    @property
    def timed(self) -> bool:
        """Whether the counting calls take the swipes' times (``late_key`` /
        ``day_profile``)."""
        return self._profile is not None

    @property
    def counts_lectures(self) -> bool:
        """Whether the counting calls take the swipes' lectures (``lecture_counts``)."""
        return self._lectures is not None

    @property
    def dedup(self) -> bool:
        """Whether a seen-row set keeps repeats out of the counts (``dedup``)."""
        return self._dedup is not None

    @property
    def needs_times(self) -> bool:
        """Whether the counting calls need the swipes' times: for a profile
        (``timed``), for the row keys of ``dedup`` or for the rows of ``records``."""
        return self._profile is not None or self._dedup is not None or self._records is not None

    @property
    def needs_lectures(self) -> bool:
        """Whether the counting calls need the swipes' lectures: for the tally
        (``counts_lectures``), for the row keys of ``dedup`` or for the rows of ``records``."""
        return self._lectures is not None or self._dedup is not None or self._records is not None

    @property
    def keeps_records(self) -> bool:
        """Whether a row log keeps every row (``records``)."""
        return self._records is not None

    def records(self, lecture=None, since=None, until=None) -> dict:
        """``client.rows_select`` over the log: the rows of ``lecture`` (None:
        every lecture's, digest-major) with ``since <= time < until`` (seconds,
        or anything ``epoch_seconds`` takes; None: open), each (lecture, time,
        id) once with its last write, in (time, id) order."""
        if self._records is None:
            raise ValueError("no records")
        lo = None if since is None else int(epoch_seconds([since])[0])
        hi = None if until is None else int(epoch_seconds([until])[0])
        return self.client.rows_select(self._records, lecture, lo, hi)

    _EXACT = {"attended": dict(), "late": dict(late=True), "invalid": dict(valid=False)}

    def exact_counts(self, which: str, groups: bool = True) -> dict:
        """``client.rows_group`` by student over the whole log -- the
        reference's per-student ``groupby('student_id').size()``, exact, each
        row once with its last write: ``which`` "attended" counts every row,
        valid or not, as the reference's consistency insight does
        (attendance_analysis.py:100); "late" the rows whose UTC second of the
        day is at least ``late_from`` (:68); "invalid" the rows with
        ``is_valid`` false (:112).  ``{"keys", "counts", "stats", "complete"}``."""
        if self._records is None:
            raise ValueError("no records")
        if which not in self._EXACT:
            raise ValueError('which is "attended", "invalid" or "late"')
        opt = self._EXACT[which]
        return self.client.rows_group(self._records, "student", valid=opt.get("valid"),
                                      late_from=self.late_from if opt.get("late") else None, groups=groups)

    def exact_by_day(self) -> dict:
        """``by_day`` from the log's rows (``client.rows_profile``): ``{day
        name: rows}`` of the weekdays that have any, in the order of the names."""
        if self._records is None:
            raise ValueError("no records")
        return exact_by_day_format(self.client.rows_profile(self._records))

    def exact_lecture_rankings(self, k: int = 3) -> dict:
        """``lecture_rankings`` from the log's rows: ``client.rows_group`` by
        lecture, the digests joined to names through the tally's listing (as
        ``AttendanceProcessor.fetch_attendance_data`` does; a digest the listing
        does not name shows as ``"#<hex digest>"``), in ``lecture_rankings``'
        total order -- count descending, name ascending."""
        if self._records is None:
            raise ValueError("no records")
        if self._lectures is None:
            raise ValueError("exact_lecture_rankings needs lecture_counts (the lecture names)")
        names, *_ = self.client.tally_list(self._lectures)
        return exact_rankings_format(self.client.rows_group(self._records, "lecture"), names, k)

    def exact_insights(self, lecture_k: int | None = 3) -> list:
        """The reference's five insights (attendance_analysis.py:65-118) in its
        order, exact: each a group-by over the log's rows after the upsert,
        computed on the device; only the groups come to the host.  Titles and
        descriptions as ``insights`` writes them; ``data`` is ``{int
        student_id: count}``, ``{day name: count}`` by day.  Latecomers pass
        ``count > median`` (``2 * count > med_lo + med_hi``), consistent
        attendees ``count > median + std`` (``reference_rule``, in integers);
        every entry carries the log's ``complete``.  ``lecture_k=None`` leaves
        the lecture entry out (it needs ``lecture_counts``)."""
        late = self.exact_counts("late")
        by_day = self.exact_by_day()
        ranks = self.exact_lecture_rankings(lecture_k) if lecture_k is not None else None
        return exact_insight_entries(late, by_day, ranks, self.exact_counts("attended"),
                                     self.exact_counts("invalid"), self.late_from)

    def records_info(self) -> dict:
        """``client.rows_info`` of the log: capacity, used, taken, refused_ids,
        dropped, overflow."""
        if self._records is None:
            raise ValueError("no records")
        return self.client.rows_info(self._records)

    def compact_records(self, keep_since=None) -> dict:
        """``client.rows_compact`` of the log: the superseded rows and those
        older than ``keep_since`` (seconds, or anything ``epoch_seconds`` takes;
        None: none) leave it; ``before``, ``kept``, ``superseded``, ``expired``.
        No read of a window at or after ``keep_since`` changes its answer."""
        if self._records is None:
            raise ValueError("no records")
        out = self.client.rows_compact(self._records, keep_since)
        if self._rec_compact:
            self._rec_bound = out["kept"]
        return out

    def _records_room(self, n: int) -> None:
        """``records_compact``: before an append of ``n`` rows is enqueued, the
        compaction when the bound says the batch may not fit; then the bound's step."""
        if not self._rec_compact:
            return
        if self._rec_bound + n > self._rec_cap:
            self.compact_records(self._rec_keep)
        self._rec_bound += n

    def duplicate_rows(self) -> int:
        """Rows the seen set kept out of the counts so far: ``looked_at - first``."""
        if self._dedup is None:
            raise ValueError("no dedup")
        info = self.client.seen_info(self._dedup)
        return info["looked_at"] - info["first"]

    def _first_sightings(self, buf, offs, ep, lec) -> np.ndarray:
        """The rows' keys folded on the device, added to the seen set: bool per
        row, True where it is to be counted."""
        cl = self.client
        n = ep.size
        b = cl.seen_fold_rows_packed((buf, offs), ep, lec, self._dedup_gran)
        cl.ctx.call("ske_seen_add_async", cl.seen_sid(self._dedup), C.c_void_p(b["keys"].ptr), n, None, 0,
                    C.c_void_p(b["out"].ptr))
        cl.ctx.call("ske_sync")
        return b["out"].to_host(np.uint8, n) == SKE_SEEN_FIRST

    @staticmethod
    def _take_packed(buf, offs, keep):
        """The kept items of a packed batch, packed again."""
        lens = np.diff(offs.astype(np.int64))
        body = buf[int(offs[0]):int(offs[-1])]
        out = np.zeros(int(keep.sum()) + 1, np.uint32)
        np.cumsum(lens[keep], out=out[1:])
        return np.ascontiguousarray(body[np.repeat(keep, lens)]), out

    def _count_first(self, buf, offs, v, ep, lec) -> None:
        """``dedup``: the rows seen before leave, the others take the counting
        path.  The time and lecture columns go on only where their option is on."""
        keep = self._first_sightings(buf, offs, ep, lec)
        if not keep.any():
            return
        if not keep.all():
            buf, offs = self._take_packed(buf, offs, keep)
            v, ep, lec = v[keep], ep[keep], self._take_packed(lec[0], lec[1], keep)
        self._count_kept(buf, offs, v, ep if self.timed else None, lec if self.counts_lectures else None)

    def _update_dedup(self, bf_key, slots, ids, ep, lec) -> np.ndarray:
        """``update`` with ``dedup``: the swipe call over every row, then the
        counting over the first sightings (host-fed, as ``count_packed``)."""
        cl = self.client
        n, width = ids.shape
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        if s.shape != (n,):
            raise ValueError("one slot per id")
        d_ids, d_slots, d_valid, *_ = self._buffers(n, width)
        bkey = encode(bf_key)
        valid = np.zeros(n, np.uint8)  # BF.EXISTS of a missing key answers 0
        if cl.keys.expect(bkey, "bf"):
            d_ids.from_host(ids)
            d_slots.from_host(s)
            cl.ctx.call("ske_swipes_fixed", cl.keys.fid[bkey], C.c_void_p(d_slots.ptr), C.c_void_p(d_ids.ptr),
                        width, n, C.c_void_p(d_valid.ptr), SKE_MEM_DEVICE)
            valid = d_valid.to_host(np.uint8, n)
        if self._records is not None:  # every row, before the repeats leave
            self._records_room(n)
            cl.rows_enqueue(cl.rows_rid(self._records), lec, ep, fixed_ids=ids, valid=valid)
        offs = (np.arange(n + 1, dtype=np.uint64) * width).astype(np.uint32)
        self._count_first(ids.reshape(-1), offs, valid, ep, lec)
        return valid.astype(bool)

    def _enqueue_packed(self, d_ids, d_offs, n: int, d_valid, d_epoch, d_late) -> None:
        """The counting half of ``update`` over a packed batch on the device
        (id i = ``ids[offs[i]:offs[i + 1]]``), enqueued in ``update``'s order:
        the attended and invalid adds masked by the valid bytes; with the time
        options the profile add, which writes the late bytes, and the late
        key's add masked by them; then the tracks."""
        cl = self.client
        ids, offs, valid = C.c_void_p(d_ids.ptr), C.c_void_p(d_offs.ptr), C.c_void_p(d_valid.ptr)
        for key, want in ((self.attended_key, 1), (self.invalid_key, 0)):
            cl.ctx.call("ske_cms_add_packed_async", cl.cms_cid(key), ids, offs, n, None, valid, want)
        if d_epoch is not None:
            late = self.late_key is not None
            cl.ctx.call("ske_tp_add_async", cl.tp_tid(self._profile), C.c_void_p(d_epoch.ptr), n, None, 1,
                        self.late_from, C.c_void_p(d_late.ptr) if late else None)
            if late:
                cl.ctx.call("ske_cms_add_packed_async", cl.cms_cid(self.late_key), ids, offs, n, None,
                            C.c_void_p(d_late.ptr), 1)
        for name, thr, want in self._tracks:
            hid, cid = cl._hh_entry(name)
            cl.ctx.call("ske_hh_track_packed_async", hid, cid, ids, offs, n, valid, want, thr)
        if self._late_track is not None:
            name, thr, want = self._late_track
            hid, cid = cl._hh_entry(name)
            cl.ctx.call("ske_hh_track_packed_async", hid, cid, ids, offs, n, C.c_void_p(d_late.ptr), want, thr)

    def _packed_buffers(self, which: str, n: int, nbytes: int) -> dict:
        """Device buffers of a packed batch of up to ``n`` ids in ``nbytes``
        bytes, kept between calls (``which``: "host", ``count_packed``'s
        upload, or "dense", ``update_messages``' batch)."""
        b = self._pk_bufs.get(which)
        if b is None or b["n"] < n or b["nbytes"] < nbytes:
            if b is not None:
                for x in b.values():
                    if isinstance(x, DeviceBuffer):
                        x.free()
            cn, cb = max(n, 1024), max(nbytes, 1 << 14)
            ctx = self.client.ctx
            b = {"n": cn, "nbytes": cb, "ids": DeviceBuffer(ctx, cb + 64), "offs": DeviceBuffer(ctx, (cn + 1) * 4),
                 "valid": DeviceBuffer(ctx, cn + 16)}
            if self.timed or which == "dense":
                b["epoch"] = DeviceBuffer(ctx, cn * 8 + 16)
                b["late"] = DeviceBuffer(ctx, cn + 16)
            if which == "dense":  # every message's epoch before compaction; the entries' message indices
                b["epoch_all"] = DeviceBuffer(ctx, cn * 8 + 16)
                b["at"] = DeviceBuffer(ctx, cn * 4 + 16)
                if self._dedup is not None:  # every message's row key and the set's answer
                    b["seen_keys"] = DeviceBuffer(ctx, cn * 16 + 16)
                    b["seen_out"] = DeviceBuffer(ctx, cn + 16)
            self._pk_bufs[which] = b
        return b

    def _check_times(self, times, n: int):
        if (times is None) != (not self.needs_times):
            raise ValueError("times go with late_key / day_profile (or dedup): required with either, refused without")
        if times is None:
            return None
        ep = epoch_seconds(times)
        if ep.size != n:
            raise ValueError("one time per id")
        return ep

    def count_packed(self, buf, offs, valid, times=None, lectures=None) -> None:
        """The counting half of ``update`` for swipes whose BF.EXISTS answers
        the caller already has: id i is ``buf[offs[i]:offs[i + 1]]`` (the ids
        as redis-py encodes them, ``encoding.pack``), ``valid`` one answer per
        id.  Every valid swipe's id counts in the attended key and every
        invalid one's in the invalid key; ``times`` and ``lectures`` as in
        ``update``.  No swipe call is made.  Uploads, enqueues, returns when done."""
        buf = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
        offs = np.ascontiguousarray(offs, dtype=np.uint32).reshape(-1)
        n = offs.size - 1
        v = np.ascontiguousarray(np.asarray(valid).astype(bool), dtype=np.uint8).reshape(-1)
        if n < 0 or v.size != n:
            raise ValueError("one valid answer per id, offs one entry more")
        ep = self._check_times(times, n)
        lec = self._check_lectures(lectures, n)
        if n == 0:
            return
        if self._records is not None:  # every row, before the repeats leave
            self._records_room(n)
            self.client.rows_enqueue(self.client.rows_rid(self._records), lec, ep, ids=(buf, offs), valid=v)
        if self._dedup is not None:
            self._count_first(buf, offs, v, ep, lec)
        else:
            self._count_kept(buf, offs, v, ep if self.timed else None, lec if self.counts_lectures else None)

    def _count_kept(self, buf, offs, v, ep, lec) -> None:
        """``count_packed``'s work over checked arrays."""
        n = offs.size - 1
        b = self._packed_buffers("host", n, int(offs[-1]))
        b["ids"].from_host(buf[:int(offs[-1])])
        b["offs"].from_host(offs)
        b["valid"].from_host(v)
        if ep is not None:
            b["epoch"].from_host(ep)
        self._enqueue_packed(b["ids"], b["offs"], n, b["valid"], b["epoch"] if ep is not None else None,
                             b.get("late"))
        if lec is not None:
            self._enqueue_lectures(lec, n, b["valid"])
        self.client.ctx.call("ske_sync")

    def update_messages(self, bf_key, messages, hll_key_prefix: str = "hll:unique:", key_form: str = "readme"):
        """``client.ingest`` over raw message payloads, and every decodable
        message's swipe counted as ``update`` counts it: its student id in the
        attended or the invalid key by its BF.EXISTS answer and, with the time
        options, its ``timestamp`` -- as ``epoch_seconds(fromisoformat(...))``
        -- in the profile and, when late, its id in the late key.  Messages
        decoded on the device are counted there: their ids, answers and times
        never come to the host.  The others are decoded by Python, as
        ``ingest`` does, and counted through ``count_packed``; a message that
        cannot be decoded (status -1) counts nowhere.  With ``lecture_counts``
        every counted message also counts under its ``lecture_id``: the
        device-decoded ones from the lecture spans the parse left beside the
        message bytes.  Returns ``(valid, status)`` as ``ingest``."""
        blob, moffs = join_messages(messages)
        return self.update_messages_packed(bf_key, blob, moffs, hll_key_prefix, key_form)

    def update_messages_packed(self, bf_key, blob, moffs, hll_key_prefix: str = "hll:unique:",
                               key_form: str = "readme"):
        """``update_messages`` over payloads already laid end to end
        (``client.ingest_packed``'s layout)."""
        cl = self.client
        valid, status, run = cl._ingest_batch(bf_key, blob, moffs, hll_key_prefix, key_form)
        if run is None:
            return valid, status
        B, n = run.B, run.n
        d = self._packed_buffers("dense", n, B["msgs"].nbytes)  # an id is a piece of its message
        msgs = C.c_void_p(B["msgs"].ptr)
        if self.needs_times:
            cl.ctx.call("ske_ingest_times", msgs, C.byref(run.cols), n, C.c_void_p(d["epoch_all"].ptr))
        cols = run.cols
        if self._records is not None:
            # every decoded message's row from the parse columns in place: the parse's own status
            # (not the seen set's answers), the message times and K1's valid bytes
            self._records_room(n)
            cl.ctx.call("ske_rows_append_spans_async", cl.rows_rid(self._records), msgs, cols.lec_start,
                        cols.lec_len, cols.id_start, cols.id_len, cols.status, C.c_void_p(d["epoch_all"].ptr),
                        C.c_void_p(B["valid"].ptr) if run.has_bf else None, None, n)
        if self._dedup is not None:
            # The row keys from the parse columns in place, per message; the
            # set's answer bytes then stand in for the status column: 0 is a
            # decoded message whose row is new, so the repeats leave with the
            # undecoded ones and nothing is compacted.
            keys, seen_out = C.c_void_p(d["seen_keys"].ptr), C.c_void_p(d["seen_out"].ptr)
            cl.ctx.call("ske_seen_fold_spans_async", keys, msgs, cols.lec_start, cols.lec_len, None, n, 1)
            cl.ctx.call("ske_seen_fold_spans_async", keys, msgs, cols.id_start, cols.id_len, None, n, 0)
            cl.ctx.call("ske_seen_fold_epoch_async", keys, C.c_void_p(d["epoch_all"].ptr), self._dedup_gran, n, 0)
            cl.ctx.call("ske_seen_add_async", cl.seen_sid(self._dedup), keys, n, cols.status, 0, seen_out)
            cols = IngestCols.from_buffer_copy(run.cols)
            cols.status = d["seen_out"].ptr
        out = IngestDense(*[C.c_void_p(d[k].ptr) for k in ("ids", "offs", "epoch", "valid", "at")])
        ndense, nbytes = C.c_uint64(), C.c_uint64()
        cl.ctx.call("ske_ingest_dense", msgs, C.byref(cols), n,
                    C.c_void_p(B["valid"].ptr) if run.has_bf else None,  # a missing key answers 0
                    C.c_void_p(d["epoch_all"].ptr) if self.timed else None, C.byref(out), d["nbytes"],
                    C.byref(ndense), C.byref(nbytes))
        if ndense.value:
            self._enqueue_packed(d["ids"], d["offs"], int(ndense.value), d["valid"],
                                 d["epoch"] if self.timed else None, d["late"])
            if self._lectures is not None:  # the lecture spans of the parse columns, in place
                cl.ctx.call("ske_tally_add_spans_async", cl.tally_tid(self._lectures), msgs, cols.lec_start,
                            cols.lec_len, n, cols.status,
                            C.c_void_p(B["valid"].ptr) if run.has_bf else None)
            cl.ctx.call("ske_sync")
        if run.host_at:
            hbuf, hoffs = pack(run.host_ids)
            self.count_packed(hbuf, hoffs, valid[np.asarray(run.host_at)],
                              run.host_ts if self.needs_times else None,
                              run.host_lectures if self.needs_lectures else None)
        return valid, status

    def _query(self, key, ids) -> np.ndarray:
        if isinstance(ids, np.ndarray) and ids.dtype == np.uint8 and ids.ndim == 2:
            n, width = ids.shape
            buf = np.ascontiguousarray(ids).reshape(-1)
            offs = (np.arange(n + 1, dtype=np.uint64) * width).astype(np.uint32)
        else:
            buf, offs = pack(ids)
        return self.client.cms_query_packed(key, buf, offs)

    def attended(self, ids) -> np.ndarray:
        """Estimated valid swipes of each id (ids as redis-py encodes them, or
        a [n, width] uint8 array)."""
        return self._query(self.attended_key, ids)

    def invalid(self, ids) -> np.ndarray:
        """Estimated invalid attempts of each id."""
        return self._query(self.invalid_key, ids)

    def _track_of(self, key):
        """(set name, track threshold) of a tracked key."""
        name = b"hh:" + encode(key)
        track = [t for t in self._tracks + [self._late_track] if t is not None and t[0] == name]
        if not track:
            raise ValueError(f"{key} is not tracked (track_attended / track_invalid / track_late)")
        return name, track[0][1]

    def _which_key(self, which: str):
        keys = {"attended": self.attended_key, "invalid": self.invalid_key, "late": self.late_key}
        if which not in keys:
            raise ValueError('which is "attended", "invalid" or "late"')
        if keys[which] is None:
            raise ValueError("no late_key is tracked (track_late)")
        return keys[which]

    def population(self, which: str) -> dict:
        """``client.hh_stats`` of the key's set at its track threshold: the
        statistics of every tracked student's estimate -- with a track
        threshold of 1 the reference's whole population -- computed on the
        device.  ``which``: "attended", "invalid" or "late"."""
        name, thr = self._track_of(self._which_key(which))
        return self.client.hh_stats(name, thr)

    def reference_threshold(self, which: str, rule: str):
        """The smallest integer estimate that passes the reference's rule over
        ``population(which)``: ``rule="median+std"`` is ``est > median + std``
        (attendance_analysis.py:101-103), ``"median"`` is ``est > median``
        (:69); decided in integers (``reference_rule``).  None when nothing can
        pass: no student, or one student under ``"median+std"``."""
        return reference_rule(self.population(which), rule)

    def _top_reference(self, key, rule: str):
        """``_top`` at the threshold the reference's rule derives on the
        device: ske_hh_stats, then ske_hh_list at that threshold, so only the
        passing students cross to the host."""
        name, thr = self._track_of(key)
        stats = self.client.hh_stats(name, thr)
        derived = reference_rule(stats, rule)
        if derived is None or derived > 0xFFFFFFFF:  # nobody can pass
            return [], np.zeros(0, np.uint32), stats["complete"]
        hid, cid = self.client._hh_entry(name)
        return hh_list(self.client.ctx, hid, cid, derived, room=stats["n"])

    def _top(self, key, k, threshold):
        name, track_thr = self._track_of(key)
        thr = track_thr if threshold is None else int(threshold)
        if thr < track_thr:
            raise ValueError("a list threshold below the track threshold promises nothing")
        ids, est, complete = self.client.hh_list(name, thr)
        if k is not None:
            ids, est = ids[:k], est[:k]
        return ids, est, complete

    def top_attended(self, k: int | None = None, threshold: int | None = None):
        """``(ids, estimates, complete)``: the students whose estimated valid
        swipes reach ``threshold`` (default: the track threshold), largest
        first, ties in id order; the first ``k`` of them when ``k`` is given.
        ``complete`` is False once the set refused an id (it was full): the
        list may then miss students."""
        return self._top(self.attended_key, k, threshold)

    def top_invalid(self, k: int | None = None, threshold: int | None = None):
        """The same over the invalid attempts."""
        return self._top(self.invalid_key, k, threshold)

    def late(self, ids) -> np.ndarray:
        """Estimated late swipes (valid or not) of each id."""
        if self.late_key is None:
            raise ValueError("no late_key")
        return self._query(self.late_key, ids)

    def top_late(self, k: int | None = None, threshold: int | None = None):
        """The same over the late swipes (``track_late``)."""
        if self.late_key is None:
            raise ValueError("no late_key is tracked (track_late)")
        return self._top(self.late_key, k, threshold)

    def lecture_events(self, lectures):
        """``(events, valid)``, u64 per lecture: the swipes counted under it,
        valid or not, and the valid ones; 0, 0 for a lecture never seen.
        ``lectures`` as ``update`` takes them."""
        if self._lectures is None:
            raise ValueError("no lecture_counts")
        lectures = list(lectures)
        buf, offs = self._check_lectures(lectures, len(lectures))
        return tally_query(self.client.ctx, self.client.tally_tid(self._lectures), buf, offs)

    def lecture_rankings(self, k: int = 3, by: str = "events") -> dict:
        """The reference's ``groupby('lecture_id').size().sort_values(
        ascending=False)``, ``.head(k)`` and ``.tail(k)`` (attendance_analysis.py
        :87-97): ``{"most_attended": {lecture: count}, "least_attended": {...},
        "complete": bool}`` in the listing's total order (count descending,
        lecture ascending; pandas leaves ties in quicksort order), the tail as
        ``.tail(k)`` lists it.  ``by="valid"`` ranks and reports the valid
        swipes instead.  ``complete`` False: the tally refused a swipe and the
        counts are lower bounds."""
        if self._lectures is None:
            raise ValueError("no lecture_counts")
        head, tail, complete = self.client.tally_top(self._lectures, k, by)
        col = 2 if by == "valid" else 1
        return {"most_attended": {key.decode("utf-8", "replace"): int(c) for key, c in zip(head[0], head[col])},
                "least_attended": {key.decode("utf-8", "replace"): int(c) for key, c in zip(tail[0], tail[col])},
                "complete": complete}

    def by_hour_of_week(self) -> np.ndarray:
        """Swipes, valid or not, per weekday (Monday first) and UTC hour:
        [7, 24] uint64."""
        if self._profile is None:
            raise ValueError("no time profile (late_key / day_profile)")
        return self.client.tp_counts(self._profile)

    def by_day(self) -> dict:
        """``{day name: swipes}`` of the weekdays that have any, in the order of
        the names, as pandas' ``groupby('day_of_week').size().to_dict()``
        (attendance_analysis.py:78-84)."""
        per_day = self.by_hour_of_week().sum(axis=1)
        return {d: int(per_day[i]) for d, i in sorted((d, i) for i, d in enumerate(DAY_NAMES)) if per_day[i]}

    def insights(self, attended_threshold: int | str | None = None, invalid_threshold: int | str | None = None,
                 late_threshold: int | str | None = None, lecture_k: int | None = 3) -> list:
        """The reference's insights (attendance_analysis.py:65-118) in its
        order, each only when its option is on: "Habitual Latecomers"
        (``track_late``), "Attendance by Day" (``day_profile``), "Lecture
        Attendance Rankings" (``lecture_counts``: ``lecture_rankings(lecture_k)``,
        its two lists as ``data``; ``lecture_k=None`` leaves the entry out), then
        the two below.  ``data`` is ``{student_id:
        estimate}`` of the tracked keys, ``{day name: swipes}`` by day.
        The reference picks its consistent attendees by the median plus the
        standard deviation of every student's count, its latecomers by the
        median.  A set tracked at threshold 1 is that population -- every id
        that ever counted, each with its current estimate -- so the string
        ``"reference"`` as a threshold applies the reference's own rule:
        ``attended_threshold="reference"`` lists ``est > median + std``,
        ``late_threshold="reference"`` lists ``est > median``, both over the
        key's set at its track threshold; the statistics are computed on the
        device and the rule is decided in integers (``reference_threshold``),
        then only the passing students are listed.  The reference lists every
        invalid attempt, so ``invalid_threshold="reference"`` is the track
        threshold.  An integer is a threshold of the caller's; the default is
        the track threshold.  ``complete`` is added to each per-student entry.

        Latecomers with ``late_threshold=None`` follow the reference's rule on
        the host: listed at the track threshold, a student stays whose
        estimate is above the median of the listed estimates -- the same
        students as ``"reference"``, the reference's result when ``track_late``
        is 1, the list is complete and the estimates are exact."""
        out = []
        if invalid_threshold == "reference":
            invalid_threshold = None
        if self._late_track is not None:
            if late_threshold == "reference":
                ids, est, complete = self._top_reference(self.late_key, "median")
            else:
                ids, est, complete = self._top(self.late_key, None, late_threshold)
            if late_threshold is None and len(ids):
                keep = est > np.median(est)
                ids, est = [i for i, k in zip(ids, keep) if k], est[keep]
            out.append({"title": "Habitual Latecomers",
                        "description": f"Found {len(ids)} students who frequently arrive after "
                                       f"{self.late_from // 3600}:00 AM",
                        "data": {i.decode("utf-8", "replace"): int(e) for i, e in zip(ids, est)},
                        "complete": complete})
        if self._day_insight:
            out.append({"title": "Attendance by Day",
                        "description": "Distribution of attendance across different days",
                        "data": self.by_day()})
        if self._lectures is not None and lecture_k is not None:
            ranks = self.lecture_rankings(lecture_k)
            out.append({"title": "Lecture Attendance Rankings",
                        "description": "Most and least attended lectures",
                        "data": {"most_attended": ranks["most_attended"],
                                 "least_attended": ranks["least_attended"]},
                        "complete": ranks["complete"]})
        for title, text, key, thr in (
                ("Most Consistent Attendees", "Students whose estimated attendance reaches the threshold",
                 self.attended_key, attended_threshold),
                ("Invalid Attendance Attempts", "Estimated invalid attendance attempts by student id",
                 self.invalid_key, invalid_threshold)):
            if not any(t[0] == b"hh:" + encode(key) for t in self._tracks):
                continue
            if thr == "reference":  # the attended key: the invalid one's was resolved above
                ids, est, complete = self._top_reference(key, "median+std")
            else:
                ids, est, complete = self._top(key, None, thr)
            out.append({"title": title, "description": text,
                        "data": {i.decode("utf-8", "replace"): int(e) for i, e in zip(ids, est)},
                        "complete": complete})
        return out
