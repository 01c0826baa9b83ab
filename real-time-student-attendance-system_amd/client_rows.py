"""The row-log part of ``SketchClient`` (csrc/sketch_api_rows.cpp): named
device-resident, append-only logs of attendance rows -- (lecture, timestamp,
student_id, is_valid), the reference's Cassandra table -- read back per lecture
in the table's clustering order, a redelivered row overwriting itself.

A log is no Redis key -- no kind, no TYPE reply, no command; ``DEL``, ``EXISTS``
and ``scan_iter`` do not see it -- so the client keeps its own registry of live
logs, by name, as it does for the seen sets.  ``FLUSHALL`` frees them; while no
log exists it makes no further native call.

A row's partition is its lecture's digest (``lecture_digest``), its id an
integer: the id column of an append is canonical decimal text (``parse_id``),
anything else is refused and counted.  ``rows_oracle`` restates the whole
pipeline in Python and is the oracle of the device's answers.

``rows_group`` and ``rows_profile`` count the log's rows after the upsert by
student, by lecture or by weekday and hour, on the device -- the reference's
``groupby(...).size()`` calls (attendance_analysis.py:65-118), exact;
``rows_group_oracle`` and ``rows_profile_oracle`` are their oracles.
``rows_group_merge`` sums several such group lists -- the ranks' of a run
sharded by lecture -- into the list of all their rows, on the device
(``ske_rows_group_merge``); ``rows_group_merge_oracle`` is its oracle.

``rows_compact`` is the table's overwrite and TTL: the superseded rows and
those older than a cutoff leave the log on the device, the survivors move to
the front in arrival order; ``rows_compact_oracle`` is its oracle."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from . import _lib
from .encoding import encode, pack
from .engine import (DeviceBuffer, rows_compact, rows_group, rows_group_merge, rows_info, rows_profile, rows_read,
                     rows_select)
from .exceptions import ResponseError
from .keyhash import murmur64a

BLOOM_SEED = 0xC6A4A7935BD1E995  # kBloomSeed (csrc/sketch_common.h)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _lecture_bytes(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


@functools.lru_cache(maxsize=1 << 16)
def _digest(b: bytes) -> int:
    return murmur64a(b, BLOOM_SEED) or 1


def lecture_digest(x) -> int:
    """A lecture's partition word: MurmurHash64A of ``str(x).encode()`` (bytes
    as they are) with the Bloom seed, 0 mapped to 1 -- the tally's identity."""
    return _digest(_lecture_bytes(x))


def parse_id(text: bytes):
    """The id rule: canonical decimal text -- ``-?`` then digits, no leading
    zero except ``0`` itself, no ``-0``, no ``+``, no blanks -- that fits int64.
    Returns the integer, or None (not a Cassandra int: the row is refused)."""
    neg = text[:1] == b"-"
    digits = text[1:] if neg else text
    if not digits or any(not 0x30 <= b <= 0x39 for b in digits):
        return None
    if digits[:1] == b"0" and (len(digits) > 1 or neg):
        return None
    v = int(text)
    return v if INT64_MIN <= v <= INT64_MAX else None


def rows_oracle(batches, lecture=None, since=None, until=None, capacity=None) -> dict:
    """The log and a select over it in pure Python.  ``batches``: an iterable
    of ``(lectures, ids, epochs, valid, take)`` in arrival order -- per row the
    lecture (bytes or anything ``str()`` names), the id text (as redis-py
    encodes it), int seconds, a truth value, and whether the status and mask
    let the row through (``valid`` / ``take`` None: all 0 / all taken).

    Returns ``{"log": (digest, epoch, id, valid) arrays in arrival order,
    "taken", "refused_ids", "dropped", "select": the four columns after the
    upsert, in order}``: the last write per (digest, epoch, id) wins, rows sort
    by (epoch, id), signed, behind the digest (unsigned) when no ``lecture`` is
    given; ``since <= epoch < until``; ``capacity`` keeps the first rows only."""
    log, taken, refused = [], 0, 0
    for lectures, ids, epochs, valid, take in batches:
        n = len(ids)
        valid = [0] * n if valid is None else valid
        take = [1] * n if take is None else take
        for lec, i, e, v, t in zip(lectures, ids, epochs, valid, take):
            if not t:
                continue
            taken += 1
            val = parse_id(encode(i))
            if val is None:
                refused += 1
                continue
            log.append((lecture_digest(lec), int(e), val, 1 if v else 0))
    dropped = 0
    if capacity is not None and len(log) > capacity:
        dropped = len(log) - capacity
        log = log[:capacity]
    want = None if lecture is None else lecture_digest(lecture)
    lo = INT64_MIN if since is None else int(since)
    hi = INT64_MAX if until is None else int(until)
    last = {}
    for d, e, i, v in log:
        if (want is None or d == want) and lo <= e and (hi == INT64_MAX or e < hi):
            last[(d, e, i)] = v  # the upsert: the last write wins
    sel = sorted((d, e, i, v) for (d, e, i), v in last.items())

    def cols(rows):
        return (np.asarray([r[0] for r in rows], np.uint64), np.asarray([r[1] for r in rows], np.int64),
                np.asarray([r[2] for r in rows], np.int64), np.asarray([r[3] for r in rows], np.uint8))

    return {"log": cols(log), "taken": taken, "refused_ids": refused, "dropped": dropped, "select": cols(sel)}


def rows_compact_oracle(log, keep_since=None) -> dict:
    """``RowsMixin.rows_compact`` in pure Python over the four arrival-order
    columns ``rows_oracle`` returns in ``"log"``: a row survives when ``epoch >=
    keep_since`` (None: every epoch) and no later row has its (digest, epoch,
    id); the survivors in arrival order.  Returns ``{"log": the compacted
    columns, "kept", "superseded", "expired"}`` -- a row below the cutoff is
    expired whether or not it was superseded."""
    lec, ep, ids, valid = (np.asarray(c).tolist() for c in log)
    lo = INT64_MIN if keep_since is None else int(keep_since)
    last = {}
    for pos, key in enumerate(zip(lec, ep, ids)):
        if key[1] >= lo:
            last[key] = pos  # the upsert: the last write wins
    keep = sorted(last.values())
    expired = sum(1 for e in ep if e < lo)
    cols = (np.asarray([lec[p] for p in keep], np.uint64), np.asarray([ep[p] for p in keep], np.int64),
            np.asarray([ids[p] for p in keep], np.int64), np.asarray([valid[p] for p in keep], np.uint8))
    return {"log": cols, "kept": len(keep), "superseded": len(ep) - expired - len(keep), "expired": expired}


def _counted(rows, valid, late_from):
    """The selected rows that count: ``valid`` None / True / False keeps either
    validity / the valid / the invalid rows, ``late_from`` (None: 0) those whose
    floored UTC second of the day is at least it."""
    lec, ep, ids, ok = rows
    keep = np.ones(ep.size, bool)
    if valid is not None:
        keep &= (ok != 0) == bool(valid)
    if late_from:
        keep &= np.asarray([int(e) % 86400 >= int(late_from) for e in ep.tolist()], bool)
    return lec[keep], ep[keep], ids[keep]


def group_stats(counts) -> dict:
    """``n``, ``sum``, ``sumsq``, ``min``, ``max``, ``med_lo``, ``med_hi`` and
    ``median`` of a list of counts, in Python ints (``median`` exact: a half is
    a float's to hold)."""
    c = sorted(int(x) for x in counts)
    n = len(c)
    lo, hi = (c[(n - 1) // 2], c[n // 2]) if n else (0, 0)
    return {"n": n, "sum": sum(c), "sumsq": sum(x * x for x in c), "min": c[0] if n else 0, "max": c[-1] if n else 0,
            "med_lo": lo, "med_hi": hi, "median": (lo + hi) / 2}


def rows_group_oracle(batches, by="student", lecture=None, since=None, until=None, valid=None, late_from=None,
                      capacity=None) -> dict:
    """``RowsMixin.rows_group`` in pure Python on top of ``rows_oracle``: the
    rows after the upsert, those that count (``_counted``), grouped by student
    id (int64, ascending signed) or lecture digest (uint64, ascending)."""
    if by not in ("student", "lecture"):
        raise ValueError('by is "student" or "lecture"')
    sel = rows_oracle(batches, lecture, since, until, capacity)["select"]
    lec, ep, ids = _counted(sel, valid, late_from)
    col = ids.tolist() if by == "student" else lec.tolist()
    groups: dict[int, int] = {}
    for k in col:
        groups[k] = groups.get(k, 0) + 1
    keys = sorted(groups)
    stats = group_stats(groups.values())
    stats["rows"] = int(sel[1].size)
    return {"keys": np.asarray(keys, np.int64 if by == "student" else np.uint64),
            "counts": np.asarray([groups[k] for k in keys], np.uint64), "stats": stats}


def rows_group_merge_oracle(parts, by="student") -> dict:
    """``RowsMixin.rows_group_merge`` in pure Python.  ``parts``: a list of
    ``rows_group`` / ``rows_group_oracle`` results (``keys``, ``counts`` and,
    where present, ``stats["rows"]``).  A key's merged count is the sum of its
    entries' counts; the keys with a nonzero sum come out ascending, int64 by
    student, uint64 by lecture.  ``stats`` is ``group_stats`` of the sums with
    ``rows`` the sum of the parts' ``rows``; ``multi`` the listed keys that
    more than one entry with a nonzero count fed.  Refuses what the device
    call refuses: a count above 2^32 - 1, or a total above it."""
    if by not in ("student", "lecture"):
        raise ValueError('by is "student" or "lecture"')
    sums: dict[int, int] = {}
    fed: dict[int, int] = {}
    total = rows = 0
    for p in parts:
        rows += int(p.get("stats", {}).get("rows", 0))
        for k, c in zip(np.asarray(p["keys"]).tolist(), np.asarray(p["counts"]).tolist()):
            k, c = int(k), int(c)
            if c > 0xFFFFFFFF:
                raise ValueError("a count above 2^32 - 1")
            total += c
            sums[k] = sums.get(k, 0) + c
            fed[k] = fed.get(k, 0) + (c != 0)
    if total > 0xFFFFFFFF:
        raise ValueError("the counts' total is above 2^32 - 1")
    keys = sorted(k for k, c in sums.items() if c)
    stats = group_stats(sums[k] for k in keys)
    stats["rows"] = rows
    return {"keys": np.asarray(keys, np.int64 if by == "student" else np.uint64),
            "counts": np.asarray([sums[k] for k in keys], np.uint64), "stats": stats,
            "multi": sum(1 for k in keys if fed[k] > 1)}


def rows_profile_oracle(batches, lecture=None, since=None, until=None, valid=None, late_from=None,
                        capacity=None) -> np.ndarray:
    """``RowsMixin.rows_profile`` in pure Python: the counted rows per weekday
    (Monday first; 1970-01-01 was a Thursday) and UTC hour, by floor division."""
    sel = rows_oracle(batches, lecture, since, until, capacity)["select"]
    out = np.zeros((7, 24), np.uint64)
    for e in _counted(sel, valid, late_from)[1].tolist():
        out[(e // 86400 + 3) % 7, e % 86400 // 3600] += 1
    return out


class RowsMixin:
    def _rows_init_registry(self) -> None:
        self._rows: dict[bytes, int] = {}  # log name -> rid
        self._rows_free_ids = list(range(_lib.SKE_MAX_ROWS - 1, -1, -1))
        self._rows_bufs = None  # _rows_buffers
        self._rows_out = None   # rows_select's host arrays, grown as needed

    def rows_create(self, name, capacity_log2: int = 22) -> int:
        """A new, empty log of 2^capacity_log2 rows of 25 bytes; returns its native id."""
        name = encode(name)
        if name in self._rows:
            raise ResponseError(_lib.strerror(_lib.SKE_EROWSEXISTS))
        if not self._rows_free_ids:
            raise ResponseError("ERR too many row logs on this device")
        if not _lib.SKE_ROWS_MIN_LOG2 <= int(capacity_log2) <= _lib.SKE_ROWS_MAX_LOG2:
            raise ResponseError(_lib.strerror(_lib.SKE_EROWSCAP))
        rid = self._rows_free_ids[-1]
        self.ctx.call("ske_rows_init", rid, int(capacity_log2))
        self._rows_free_ids.pop()
        self._rows[name] = rid
        return rid

    def rows_rid(self, name) -> int:
        rid = self._rows.get(encode(name))
        if rid is None:
            raise ResponseError(_lib.strerror(_lib.SKE_EROWSNOLOG))
        return rid

    def rows_drop(self, name) -> bool:
        rid = self._rows.pop(encode(name), None)
        if rid is None:
            return False
        self.ctx.call("ske_rows_free", rid)
        self._rows_free_ids.append(rid)
        return True

    def _rows_release(self) -> None:
        for name in list(self._rows):
            self.rows_drop(name)

    def rows_reset(self, name) -> None:
        self.ctx.call("ske_rows_reset", self.rows_rid(name))

    def rows_info(self, name) -> dict:
        return rows_info(self.ctx, self.rows_rid(name))

    def _rows_buffers(self, n: int, nbytes: int) -> dict:
        """Device buffers of a batch of up to ``n`` rows whose longer packed
        column has ``nbytes`` bytes, kept between calls."""
        b = self._rows_bufs
        if b is None or b["n"] < n or b["nbytes"] < nbytes:
            if b is not None:
                for x in b.values():
                    if isinstance(x, DeviceBuffer):
                        x.free()
            cn, cb = max(n, 1024), max(nbytes, 1 << 14)
            b = {"n": cn, "nbytes": cb, "lec": DeviceBuffer(self.ctx, cb + 64),
                 "lec_offs": DeviceBuffer(self.ctx, (cn + 1) * 4), "ids": DeviceBuffer(self.ctx, cb + 64),
                 "id_offs": DeviceBuffer(self.ctx, (cn + 1) * 4), "epoch": DeviceBuffer(self.ctx, cn * 8 + 16),
                 "valid": DeviceBuffer(self.ctx, cn + 16)}
            self._rows_bufs = b
        return b

    def rows_enqueue(self, rid: int, lectures, ep: np.ndarray, ids=None, fixed_ids: np.ndarray | None = None,
                     valid=None, d_valid=None) -> None:
        """Upload one batch's columns and enqueue its append (not waited for):
        ``lectures`` a packed ``(buf, offs)``, ``ids`` a packed pair or
        ``fixed_ids`` a ``[n, 4 or 8]`` uint8 array, ``valid`` host bytes or
        ``d_valid`` a device buffer that holds them already (neither: all 0)."""
        n = int(ep.size)
        if n == 0:
            return
        lbuf, loffs = lectures
        if fixed_ids is not None:
            ibytes, width = np.ascontiguousarray(fixed_ids).reshape(-1), int(fixed_ids.shape[1])
            nid = ibytes.size
        else:
            ibytes, ioffs = ids
            nid = int(ioffs[-1])
        b = self._rows_buffers(n, max(int(loffs[-1]), nid))
        b["lec"].from_host(lbuf[:int(loffs[-1])])
        b["lec_offs"].from_host(loffs)
        b["ids"].from_host(ibytes[:nid])
        b["epoch"].from_host(ep)
        vp = None
        if d_valid is not None:
            vp = C.c_void_p(d_valid.ptr)
        elif valid is not None:
            b["valid"].from_host(np.ascontiguousarray(valid, dtype=np.uint8))
            vp = C.c_void_p(b["valid"].ptr)
        lec, lof = C.c_void_p(b["lec"].ptr), C.c_void_p(b["lec_offs"].ptr)
        if fixed_ids is not None:
            self.ctx.call("ske_rows_append_fixed_async", rid, lec, lof, C.c_void_p(b["ids"].ptr), width,
                          C.c_void_p(b["epoch"].ptr), vp, None, n)
        else:
            b["id_offs"].from_host(ioffs)
            self.ctx.call("ske_rows_append_packed_async", rid, lec, lof, C.c_void_p(b["ids"].ptr),
                          C.c_void_p(b["id_offs"].ptr), C.c_void_p(b["epoch"].ptr), vp, None, n)

    def rows_append(self, name, lectures, ids, times, valid=None) -> None:
        """One batch of rows through the host form (``ske_rows_append``; returns
        when done): ``lectures`` as ``str(x).encode()``, ``ids`` as redis-py
        encodes them, ``times`` in any form ``analysis.epoch_seconds`` takes,
        ``valid`` one truth value per row (None: all 0)."""
        from .analysis import epoch_seconds
        rid = self.rows_rid(name)
        ep = epoch_seconds(times)
        ibuf, ioffs = pack(list(ids))
        lbuf, loffs = pack([_lecture_bytes(x) for x in lectures])
        n = ep.size
        if not ioffs.size == loffs.size == n + 1:
            raise ValueError("one time and one lecture per id")
        v = None
        if valid is not None:
            v = np.ascontiguousarray(np.asarray(valid).astype(bool), dtype=np.uint8).reshape(-1)
            if v.size != n:
                raise ValueError("one valid answer per id")
        if n:
            self.ctx.call("ske_rows_append", rid, _lib.ptr(lbuf), _lib.ptr(loffs), _lib.ptr(ibuf), _lib.ptr(ioffs),
                          _lib.ptr(ep), _lib.ptr(v), None, n, _lib.SKE_MEM_HOST)

    def rows_select(self, name, lecture=None, since=None, until=None) -> dict:
        """The rows of ``lecture`` (None: of every lecture, digest-major) with
        ``since <= epoch < until`` (None: open), after the upsert, in (epoch,
        id) order: ``{"lecture_digest", "epoch", "student_id", "is_valid",
        "complete"}``, numpy columns.  ``complete`` False: the log dropped rows."""
        lec = None if lecture is None else _lecture_bytes(lecture)
        lo = INT64_MIN if since is None else int(since)
        hi = INT64_MAX if until is None else int(until)
        cols, n, complete = rows_select(self.ctx, self.rows_rid(name), lec, lo, hi, self._rows_out)
        self._rows_out = cols
        return {"lecture_digest": cols[0][:n].copy(), "epoch": cols[1][:n].copy(), "student_id": cols[2][:n].copy(),
                "is_valid": cols[3][:n].copy(), "complete": complete}

    def rows_compact(self, name, keep_since=None) -> dict:
        """Drop the log's dead rows on the device (``ske_rows_compact``): those
        a later row with the same (lecture, time, id) superseded and those with
        ``time < keep_since`` (seconds, or anything ``analysis.epoch_seconds``
        takes; None expires nothing).  The survivors keep their arrival order
        at positions ``0 .. kept - 1``; ``used`` and ``taken`` follow, the
        sticky ``overflow`` stays.  Returns ``{"before", "kept", "superseded",
        "expired"}``.  No ``rows_select``, ``rows_group`` or ``rows_profile``
        over a window with ``since >= keep_since`` changes its answer."""
        from .analysis import epoch_seconds
        lo = INT64_MIN if keep_since is None else int(epoch_seconds([keep_since])[0])
        return rows_compact(self.ctx, self.rows_rid(name), lo)

    def rows_read(self, name) -> dict:
        """The raw log in arrival order (a checkpoint): the four columns."""
        rid = self.rows_rid(name)
        used = rows_info(self.ctx, rid)["used"]
        lec, ep, ids, valid = rows_read(self.ctx, rid, 0, used)
        return {"lecture_digest": lec, "epoch": ep, "student_id": ids, "is_valid": valid}

    @staticmethod
    def _rows_window(lecture, since, until, valid, late_from):
        lec = None if lecture is None else _lecture_bytes(lecture)
        lo = INT64_MIN if since is None else int(since)
        hi = INT64_MAX if until is None else int(until)
        vf = _lib.SKE_ROWS_VALID_ANY if valid is None else (_lib.SKE_ROWS_VALID_ONLY if valid
                                                            else _lib.SKE_ROWS_INVALID_ONLY)
        sod = 0 if late_from is None else int(late_from)
        if not 0 <= sod <= 86399:
            raise ValueError("late_from is a second of the day, 0 to 86399")
        return lec, lo, hi, vf, sod

    def rows_group(self, name, by="student", lecture=None, since=None, until=None, valid=None, late_from=None,
                   groups: bool = True) -> dict:
        """The log's rows after the upsert, counted per student or per lecture
        on the device (``ske_rows_group``): ``{"keys", "counts", "stats",
        "complete"}``.  The window is ``rows_select``'s; ``valid`` None / True /
        False counts rows of either validity / the valid / the invalid ones,
        ``late_from`` (None: no filter) those whose UTC second of the day is at
        least it.  ``keys`` -- int64 student ids, ascending, or uint64 lecture
        digests, ascending -- and ``counts`` (uint64) list the groups with at
        least one counted row, as ``df[mask].groupby(col).size()`` does.
        ``stats``: ``rows`` (the window's rows after the upsert), ``n``, ``sum``,
        ``sumsq``, ``min``, ``max``, ``med_lo``, ``med_hi`` and ``median`` of the
        counts, in the form ``analysis.reference_rule`` takes.  ``groups``
        False: the statistics alone, ``keys`` and ``counts`` empty."""
        if by not in ("student", "lecture"):
            raise ValueError('by is "student" or "lecture"')
        lec, lo, hi, vf, sod = self._rows_window(lecture, since, until, valid, late_from)
        student = by == "student"
        keys, counts, stats, complete = rows_group(
            self.ctx, self.rows_rid(name), _lib.SKE_ROWS_BY_STUDENT if student else _lib.SKE_ROWS_BY_LECTURE, lec, lo,
            hi, vf, sod, groups)
        stats["median"] = (stats["med_lo"] + stats["med_hi"]) / 2
        return {"keys": keys.view(np.int64).copy() if student else keys.copy(), "counts": counts.copy(),
                "stats": stats, "complete": complete}

    def rows_profile(self, name, lecture=None, since=None, until=None, valid=None, late_from=None) -> np.ndarray:
        """The same counted rows per weekday (Monday first) and UTC hour
        (``ske_rows_profile``): a ``[7, 24]`` uint64 array."""
        lec, lo, hi, vf, sod = self._rows_window(lecture, since, until, valid, late_from)
        return rows_profile(self.ctx, self.rows_rid(name), lec, lo, hi, vf, sod)[0]

    def rows_group_merge(self, by, keys, counts, groups: bool = True) -> dict:
        """Several group lists summed into one on the device
        (``ske_rows_group_merge``): ``keys`` and ``counts`` are host numpy
        arrays of (key, count) entries in any order -- ``rows_group`` results
        end to end, say -- the same key any number of times.  Returns
        ``{"keys", "counts", "stats", "multi"}``: the keys whose counts sum to
        more than zero, ascending and typed as ``rows_group`` types them (int64
        student ids, uint64 lecture digests), their sums (uint64), ``stats`` as
        ``rows_group`` gives them with ``median`` added and ``rows`` 0 (the
        caller sums the parts' rows), and ``multi``, the listed keys that more
        than one entry with a nonzero count fed.  No count and no total may
        pass 2^32 - 1 (``ValueError``).  ``groups`` False: the statistics alone."""
        if by not in ("student", "lecture"):
            raise ValueError('by is "student" or "lecture"')
        student = by == "student"
        k, c = np.asarray(keys), np.asarray(counts)
        if k.ndim != 1 or k.shape != c.shape:
            raise ValueError("one count per key")
        if k.size and (k.dtype.kind not in "iu" or c.dtype.kind not in "iu"):
            raise ValueError("keys and counts are integers")
        if c.size and c.dtype.kind == "i" and int(c.min()) < 0:
            raise ValueError("a count is not negative")
        if k.size > 1 << 28:
            raise ValueError("at most 2^28 entries")
        k = np.ascontiguousarray(k.astype(np.int64 if k.dtype.kind == "i" else np.uint64, copy=False)).view(np.uint64)
        c = np.ascontiguousarray(c.astype(np.uint64, copy=False))
        # below 2^28 entries of at most 2^32 - 1 each: the uint64 sum cannot wrap
        if c.size and (int(c.max()) > 0xFFFFFFFF or int(c.sum(dtype=np.uint64)) > 0xFFFFFFFF):
            raise ValueError("no count and no total above 2^32 - 1")
        out_k, out_c, stats, multi = rows_group_merge(
            self.ctx, _lib.SKE_ROWS_BY_STUDENT if student else _lib.SKE_ROWS_BY_LECTURE, k, c, k.size,
            _lib.SKE_MEM_HOST, groups)
        stats["median"] = (stats["med_lo"] + stats["med_hi"]) / 2
        return {"keys": out_k.view(np.int64).copy() if student else out_k.copy(), "counts": out_c.copy(),
                "stats": stats, "multi": multi}
