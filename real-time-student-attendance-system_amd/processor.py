"""Batched counterpart of the reference's processor and analytics callers.

``AttendanceProcessor`` mirrors attendance_processor.py:26-165 with the
transport (Pulsar) and persistence (Cassandra) removed: messages arrive as an
iterable of JSON payloads, and the per-event loop at :100-137 (decode ->
``BF.EXISTS`` -> valid-gated ``PFADD``) runs as one fused device call per
batch.  The rows it returns are what the reference inserts into Cassandra
(:116-124), including invalid events.

``lecture_rankings`` is attendance_analysis.py:87-97 in the PFCOUNT form the
README describes (README.md:179: "rank by unique daily counts (from HLL)").
"""
from __future__ import annotations

import json
import logging
from datetime import datetime, timedelta
from typing import Iterable, Sequence

import numpy as np

from .client import SketchClient
from .config import AttendanceConfig
from .encoding import encode, pack
from .exceptions import ResponseError
from .keyspace import day_key

logger = logging.getLogger(__name__)


class AttendanceProcessor:
    def __init__(self, client: SketchClient | None = None, config: AttendanceConfig | None = None,
                 counts=None):
        """``counts``: a ``StudentCounts`` of the same client (default None:
        nothing is counted); every acknowledged row's swipe then counts in it
        (``count_packed``), which is what ``insights`` reads."""
        self.config = config or AttendanceConfig()
        self.counts = counts
        # attendance_processor.py:37-41
        self.redis_client = client or SketchClient(decode_responses=True, device=self.config.device)
        self.acked = 0
        self.nacked = 0

    # attendance_processor.py:74-92
    def _setup_bloom_filter(self):
        cfg = self.config
        try:
            self.redis_client.execute_command("BF.EXISTS", cfg.bloom_filter_key, "test")
            logger.info("Bloom Filter already exists")
            if cfg.faithful_setup:
                return
            if self.redis_client.exists(cfg.bloom_filter_key):
                return
            raise ResponseError("ERR not found")
        except ResponseError:
            try:
                self.redis_client.execute_command("BF.RESERVE", cfg.bloom_filter_key,
                                                  cfg.bloom_filter_error_rate,
                                                  cfg.bloom_filter_capacity)
                logger.info("Created new Bloom Filter")
            except ResponseError as e:
                if "already exists" not in str(e):
                    raise

    def hll_key(self, lecture_id: str, timestamp: datetime) -> str:
        """attendance_processor.py:128 (code form) or README.md:105-106 form."""
        return day_key(self.config.hll_key_prefix, lecture_id,
                       None if self.config.hll_key_form == "code" else timestamp)

    def process_batch(self, messages: Sequence) -> list[dict]:
        """One batch of the loop at attendance_processor.py:100-137.

        Returns one row per acknowledged message: student_id, lecture_id,
        timestamp, is_valid (what :121-124 inserts).  A message is negatively
        acknowledged (:134-136), produces no row and no PFADD when any step of
        the reference's loop would raise for it, in the loop's order:
          - json.loads / a missing field / datetime.fromisoformat (:103-106);
          - BF.EXISTS: redis-py refuses to encode the id (bool, None, list,
            dict: DataError, :109-113);
          - the Cassandra INSERT (:116-124, before PFADD): the table's
            ``student_id int`` / ``lecture_id text`` columns refuse an id that
            is not an int in the 32-bit range or a lecture_id that is not a
            string (``config.cassandra_row_types``; off: any id redis-py can
            encode is counted).
        The surviving messages go through one fused device call."""
        cfg = self.config
        ids, keys, rows = [], [], []
        for m in messages:
            try:
                data = json.loads(m.decode() if isinstance(m, (bytes, bytearray)) else m) \
                    if not isinstance(m, dict) else m
                student_id = data["student_id"]
                lecture_id = data["lecture_id"]
                ts = datetime.fromisoformat(data["timestamp"])
                sid = encode(student_id)  # redis-py's Encoder: DataError as BF.EXISTS raises it
                if cfg.cassandra_row_types:
                    if type(student_id) is not int or not -2**31 <= student_id < 2**31:
                        raise TypeError(f"Received an argument of invalid type for column "
                                        f"\"student_id\": {student_id!r}")
                    if not isinstance(lecture_id, str):
                        raise TypeError(f"Received an argument of invalid type for column "
                                        f"\"lecture_id\": {lecture_id!r}")
                key = self.hll_key(lecture_id, ts)
            except Exception as e:  # :134-136
                logger.error(f"Error processing message: {e}")
                self.nacked += 1
                continue
            ids.append(sid)
            keys.append(key)
            rows.append({"student_id": student_id, "lecture_id": lecture_id, "timestamp": ts})
        if rows:
            valid = self.redis_client.swipes(cfg.bloom_filter_key, keys, ids)
            for r, v in zip(rows, valid):
                r["is_valid"] = bool(v)
            self.acked += len(rows)
            if self.counts is not None:  # the rows the reference inserts, invalid ones included
                buf, offs = pack(ids)
                # what the counting call asks for: a profile / tally that exists, or the row keys of dedup
                timed = getattr(self.counts, "needs_times", self.counts.timed)
                lectured = getattr(self.counts, "needs_lectures", getattr(self.counts, "counts_lectures", False))
                self.counts.count_packed(buf, offs, valid,
                                         [r["timestamp"] for r in rows] if timed else None,
                                         **({"lectures": [r["lecture_id"] for r in rows]} if lectured else {}))
        return rows

    def insights(self, keys: Sequence[str] | None = None, k: int = 3, rank_by: str | None = None,
                 exact: bool = False, **thresholds) -> list:
        """attendance_analysis.py:65-118 in its order: ``counts.insights(
        **thresholds)`` with "Lecture Attendance Rankings" (:87-97) at its
        place, after the per-day entries and before the per-student lists of
        :99-118, in one of the two forms README.md:179 allows, never both:
          - ``rank_by="events"``, or no ``keys`` and ``counts`` has a lecture
            tally (``lecture_counts``): the reference's own form, rows per
            lecture (``counts.lecture_rankings(k)``), no key list needed;
          - ``keys`` (lecture-day HLL keys) with ``rank_by`` None or
            ``"unique"``: the unique counts by PFCOUNT (``lecture_rankings(keys,
            k)``);
          - neither: no such entry.
        ``exact=True``: ``counts.exact_insights(k)`` instead -- the five
        group-bys over the row log, exact (``counts`` needs ``records``)."""
        if self.counts is None:
            raise ValueError("insights need a StudentCounts (counts=)")
        if exact:
            if not getattr(self.counts, "keeps_records", False):
                raise ValueError("exact insights need a StudentCounts with records")
            return self.counts.exact_insights(k)
        if rank_by not in (None, "unique", "events"):
            raise ValueError('rank_by is None, "unique" or "events"')
        lectured = getattr(self.counts, "counts_lectures", False)
        if rank_by == "events" and not lectured:
            raise ValueError('rank_by="events" needs a StudentCounts with lecture_counts')
        if rank_by == "unique" and keys is None:
            raise ValueError('rank_by="unique" needs the lecture-day keys')
        by_events = rank_by == "events" or (keys is None and lectured)
        if by_events:
            return self.counts.insights(lecture_k=k, **thresholds)
        # the PFCOUNT entry takes the place of the tally's
        out = self.counts.insights(**(dict(thresholds, lecture_k=None) if lectured else thresholds))
        if keys is not None:
            at = sum(1 for i in out if i["title"] in ("Habitual Latecomers", "Attendance by Day"))
            out.insert(at, {"title": "Lecture Attendance Rankings",
                            "description": "Most and least attended lectures",
                            "data": lecture_rankings(self.redis_client, keys, k)})
        return out

    def process_attendance(self, source: Iterable, batch_size: int | None = None):
        """attendance_processor.py:94-141 over an in-memory message source;
        yields the rows of each processed batch."""
        logger.info("Starting attendance processing...")
        self._setup_bloom_filter()
        bs = batch_size or self.config.batch_size
        batch = []
        for m in source:
            batch.append(m)
            if len(batch) >= bs:
                yield self.process_batch(batch)
                batch = []
        if batch:
            yield self.process_batch(batch)

    # attendance_processor.py:149-165 (the Cassandra half: counts' row log, when it keeps one)
    def get_attendance_stats(self, lecture_id: str, day: str | None = None) -> dict:
        """PFCOUNT of the lecture's key (:151-152).  In the README key form a
        lecture is counted per day: with a day, that day's key; without one
        (the reference's signature), the union of every day key
        prefix+lecture:YYYY-MM-DD in the store -- PFCOUNT k1 k2 ...  The day
        keys come from the key table's stem index (KeySpace.day_keys, kept
        by every key creation / DEL, so a fresh processor on the same store
        answers the same without scanning every key; a lecture id that is a
        prefix of another, e.g. 'A' and 'A:B', keeps its own keys).  When
        ``counts`` has a lecture tally the dict also carries
        ``attendance_record_count`` and ``invalid_record_count``, the lecture's
        rows valid or not and the invalid ones, over every day.  When ``counts``
        keeps a seen-row set (``dedup``) those are distinct rows, and
        ``duplicate_record_count`` is how many redelivered rows, of any
        lecture, the set kept out of the counts.  When ``counts`` keeps a row
        log (``records``) the dict carries ``attendance_records`` too, the
        reference's ``SELECT student_id, timestamp`` (:154-165): the lecture's
        rows as ``{"student_id", "timestamp"}`` in (timestamp, student_id)
        order, each row once, timestamps as naive UTC datetimes of whole seconds."""
        out = {"unique_attendees": self._unique_attendees(lecture_id, day)}
        if getattr(self.counts, "keeps_records", False):
            rec = self.counts.records(lecture_id)
            out["attendance_records"] = [{"student_id": int(i), "timestamp": _utc(int(e))}
                                         for i, e in zip(rec["student_id"], rec["epoch"])]
        if getattr(self.counts, "counts_lectures", False):
            # the reference's attendance_records (:154-165), rows per lecture over
            # every day: the tally is keyed by lecture alone
            ev, va = self.counts.lecture_events([lecture_id])
            out["attendance_record_count"] = int(ev[0])
            out["invalid_record_count"] = int(ev[0]) - int(va[0])
        if getattr(self.counts, "dedup", False):
            out["duplicate_record_count"] = self.counts.duplicate_rows()
        return out

    def fetch_attendance_data(self) -> list[dict]:
        """attendance_analysis.py:19-52, the whole table as its ``all_records``
        dicts (``student_id``, ``lecture_id``, ``timestamp``, ``is_valid``), each
        row once with its last write, partitions in digest order and rows in
        (timestamp, student_id) order inside one.  The log holds lecture
        digests; the names come from the lecture tally's listing, so ``counts``
        needs both ``records`` and ``lecture_counts`` (ValueError otherwise)."""
        if not getattr(self.counts, "keeps_records", False):
            raise ValueError("fetch_attendance_data needs a StudentCounts with records")
        if not getattr(self.counts, "counts_lectures", False):
            raise ValueError("fetch_attendance_data needs a StudentCounts with lecture_counts (the lecture names)")
        from .client_rows import lecture_digest
        names, *_ = self.redis_client.tally_list(self.counts._lectures)
        by_digest = {lecture_digest(k): k.decode("utf-8", "replace") for k in names}
        rec = self.counts.records()
        return [{"student_id": int(i), "lecture_id": by_digest.get(int(d)), "timestamp": _utc(int(e)),
                 "is_valid": bool(v)}
                for d, e, i, v in zip(rec["lecture_digest"], rec["epoch"], rec["student_id"], rec["is_valid"])]

    def compact_records(self, keep_since=None) -> dict:
        """The table's overwrite and TTL over the row log
        (``StudentCounts.compact_records``): redelivered rows' earlier copies and
        the rows older than ``keep_since`` leave it; ``before``, ``kept``,
        ``superseded``, ``expired``.  ValueError without ``records``."""
        if not getattr(self.counts, "keeps_records", False):
            raise ValueError("compact_records needs a StudentCounts with records")
        return self.counts.compact_records(keep_since)

    def _unique_attendees(self, lecture_id: str, day: str | None) -> int:
        prefix = self.config.hll_key_prefix
        if self.config.hll_key_form == "code":
            key = f"{prefix}{lecture_id}" + (f":{day}" if day else "")
            return self.redis_client.pfcount(key)
        if day is not None:
            return self.redis_client.pfcount(f"{prefix}{lecture_id}:{day}")
        stem = f"{prefix}{lecture_id}"
        index = getattr(self.redis_client, "day_keys", None)
        if callable(index):  # SketchClient: the key table's stem index
            keys = index(stem)
        else:  # any redis-py-like client: SCAN for exactly <stem>:YYYY-MM-DD
            pat = glob_escape(stem)
            keys = list(self.redis_client.scan_iter(match=pat + ":" + "[0-9]" * 4 + "-" + "[0-9]" * 2 + "-" +
                                                     "[0-9]" * 2, _type="string"))
        return self.redis_client.pfcount(*keys) if keys else 0


_EPOCH = datetime(1970, 1, 1)


def _utc(seconds: int) -> datetime:
    """Seconds since 1970-01-01T00:00:00 UTC as a naive UTC datetime."""
    return _EPOCH + timedelta(seconds=seconds)


def glob_escape(text: str) -> str:
    """`text` as a Redis MATCH pattern that matches exactly it: every glob
    special byte backslash-escaped (redis src/util.c stringmatchlen reads
    ``\\x`` as a literal x outside a class; a bracket class would not do:
    ``[^]`` is an empty negated class, ``[]]`` and ``[\\]`` misparse)."""
    return "".join("\\" + ch if ch in "*?[]\\^" else ch for ch in text)


def rank_top_bottom(counts: np.ndarray, keys: Sequence[str], k: int) -> tuple[list, list]:
    """Indices of the first k and the last k keys of the order (count
    descending, key ascending), without sorting every key: only the keys tied
    with or beyond the k-th count (np.partition) are ordered (np.lexsort).
    Returns (head, tail), tail in that order as ``.tail(k)`` lists it."""
    n = len(keys)
    k = min(max(int(k), 0), n)
    if k == 0:
        return [], []
    # counts compare as unsigned: PFCOUNT replies are u64, and a saturated
    # key's (2^63, Redis' llroundl(inf)) is the largest even when the caller
    # holds it in an int64 array
    c = np.ascontiguousarray(np.asarray(counts).astype(np.int64)).view(np.uint64)
    karr = np.asarray(keys)

    def ordered(idx):
        return idx[np.lexsort((karr[idx], ~c[idx]))]

    hi = np.partition(c, n - k)[n - k]      # k-th largest count
    head = ordered(np.nonzero(c >= hi)[0])[:k]
    lo = np.partition(c, k - 1)[k - 1]      # k-th smallest count
    tail = ordered(np.nonzero(c <= lo)[0])[-k:]
    return head.tolist(), tail.tolist()


def rank_top_bottom_dev(counts, k: int, key_rank=None) -> tuple[list, list]:
    """rank_top_bottom over a torch tensor of PFCOUNTs (int64 holding the u64
    replies; device or CPU) without moving the counts: the k-th largest and
    k-th smallest counts come from ``torch.topk`` on the tensor, and only the
    keys tied with or beyond them (normally k each) are copied to the host
    and ordered there.  Order: count descending, then key ascending, where a
    key's place in the key order is ``key_rank[i]`` (a tensor, or None when
    the keys are already in ascending order by index, as C5's
    ``LECT%05d`` / day-key universes are).  Counts compare as unsigned, so a
    saturated key's PFCOUNT (2^63, Redis' llroundl(inf)) stays the largest.
    Returns (head, tail) as rank_top_bottom does."""
    import torch
    n = int(counts.numel())
    k = min(max(int(k), 0), n)
    if k == 0:
        return [], []
    u = counts.view(torch.int64) ^ torch.iinfo(torch.int64).min  # unsigned order as signed order
    hi = torch.topk(u, k, largest=True, sorted=True).values[-1]
    lo = torch.topk(u, k, largest=False, sorted=True).values[-1]

    def ordered(mask):
        idx = torch.nonzero(mask).flatten()
        c = counts.view(torch.int64)[idx].cpu().numpy().view(np.uint64)
        key = (key_rank[idx] if key_rank is not None else idx).cpu().numpy()
        return idx.cpu().numpy()[np.lexsort((key, ~c))]  # ~c: descending unsigned counts

    head = ordered(u >= hi)[:k]
    tail = ordered(u <= lo)[-k:]
    return head.tolist(), tail.tolist()


def lecture_rankings(client: SketchClient, keys: Sequence[str], k: int = 3) -> dict:
    """Most / least attended lecture-day keys by PFCOUNT (one K2 launch).

    Order: count descending, then key ascending (the reference's pandas
    ``sort_values(ascending=False)`` leaves ties in quicksort order; a total
    order is used here so results are reproducible).  ``least_attended`` is
    the tail of the same order, as ``.tail(3)`` (attendance_analysis.py:95).
    At C5 scale (1.8M lecture-day keys) only the tie sets at the two ends are
    ordered (``rank_top_bottom``)."""
    keys = list(keys)
    counts = client.pfcount_each(keys).astype(np.int64)
    head, tail = rank_top_bottom(counts, keys, k)
    return {"most_attended": {keys[i]: int(counts[i]) for i in head},
            "least_attended": {keys[i]: int(counts[i]) for i in tail}}


def campus_rollup(client: SketchClient, groups: dict, dest: str | None = None) -> dict:
    """Per-lecture unions over their day keys (PFCOUNT k1..kn per lecture, one
    launch) and, when ``dest`` is given, a campus-wide PFMERGE of every key."""
    names = list(groups)
    counts = client.pfcount_groups([groups[n] for n in names])
    out = {"per_lecture": {n: int(c) for n, c in zip(names, counts)}}
    if dest is not None:
        client.pfmerge(dest, *[k for n in names for k in groups[n]])
        out["campus_unique"] = client.pfcount(dest)
    return out
