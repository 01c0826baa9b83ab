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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SKE_MEM_DEVICE
from .encoding import encode, pack
from .engine import DeviceBuffer


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
    ids with equal 64-bit digests share one entry."""

    def __init__(self, client, attended_key="cms:attended", invalid_key="cms:invalid",
                 error: float = 0.001, probability: float = 0.01, track_attended: int | None = None,
                 track_invalid: int | None = None, capacity_log2: int = 16):
        self.client = client
        self.attended_key, self.invalid_key = attended_key, invalid_key
        for key in (attended_key, invalid_key):
            if client.keys.type_of(encode(key)) is None:
                client.cms_initbyprob(key, error, probability)
            client.keys.expect(encode(key), "cms")  # WRONGTYPE for a key of another kind
        self._bufs = None
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
            self._bufs = b
        return b[2:]

    def update(self, bf_key, slots: np.ndarray, ids: np.ndarray) -> np.ndarray:
        """One batch of swipes: ``client.swipes_fixed`` semantics (BF.EXISTS
        of every id, PFADD of the valid ones into their HLL slot), then every
        valid swipe's id counts in the attended key and every invalid one's
        in the invalid key.  ``ids``: [n, width] uint8, ``slots``: one HLL
        slot per swipe (``client.key_slot``).  Returns the validity (bool)."""
        cl = self.client
        ids = np.ascontiguousarray(ids, dtype=np.uint8)
        if ids.ndim != 2:
            raise ValueError("ids must be a [n, width] uint8 array")
        n, width = ids.shape
        if n == 0 or width == 0:
            return np.zeros(n, bool)
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        if s.shape != (n,):
            raise ValueError("one slot per id")
        d_ids, d_slots, d_valid = self._buffers(n, width)
        d_ids.from_host(ids)
        d_slots.from_host(s)
        bkey = encode(bf_key)
        if cl.keys.expect(bkey, "bf"):
            cl.ctx.call("ske_swipes_fixed", cl.keys.fid[bkey], C.c_void_p(d_slots.ptr), C.c_void_p(d_ids.ptr),
                        width, n, C.c_void_p(d_valid.ptr), SKE_MEM_DEVICE)
        else:
            d_valid.from_host(np.zeros(n, np.uint8))  # BF.EXISTS of a missing key answers 0
        for key, want in ((self.attended_key, 1), (self.invalid_key, 0)):
            cl.ctx.call("ske_cms_add_fixed_async", cl.cms_cid(key), C.c_void_p(d_ids.ptr), width, n,
                        None, C.c_void_p(d_valid.ptr), want)
        for name, thr, want in self._tracks:  # behind the adds: the estimates include this batch
            hid, cid = cl._hh_entry(name)
            cl.ctx.call("ske_hh_track_fixed_async", hid, cid, C.c_void_p(d_ids.ptr), width, n,
                        C.c_void_p(d_valid.ptr), want, thr)
        cl.ctx.call("ske_sync")
        return d_valid.to_host(np.uint8, n).astype(bool)

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

    def _top(self, key, k, threshold):
        name = b"hh:" + encode(key)
        track = [t for t in self._tracks if t[0] == name]
        if not track:
            raise ValueError(f"{key} is not tracked (track_attended / track_invalid)")
        thr = track[0][1] if threshold is None else int(threshold)
        if thr < track[0][1]:
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

    def insights(self, attended_threshold: int | None = None, invalid_threshold: int | None = None) -> list:
        """The reference's two per-student insights (attendance_analysis.py:
        105-118), ``data`` as ``{student_id: estimate}`` of the tracked keys.
        The reference picks its consistent attendees by the median plus the
        standard deviation of every student's count; a sketch holds no such
        population, so the caller passes the thresholds (default: the track
        thresholds).  ``complete`` is added to each entry."""
        out = []
        for title, text, key, thr in (
                ("Most Consistent Attendees", "Students whose estimated attendance reaches the threshold",
                 self.attended_key, attended_threshold),
                ("Invalid Attendance Attempts", "Estimated invalid attendance attempts by student id",
                 self.invalid_key, invalid_threshold)):
            if not any(t[0] == b"hh:" + encode(key) for t in self._tracks):
                continue
            ids, est, complete = self._top(key, None, thr)
            out.append({"title": title, "description": text,
                        "data": {i.decode("utf-8", "replace"): int(e) for i, e in zip(ids, est)},
                        "complete": complete})
        return out
