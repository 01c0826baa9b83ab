"""The seen-row part of ``SketchClient`` (csrc/sketch_api_seen.cpp): named exact
sets of 128-bit row keys whose add answers, per row, first sighting or repeat
-- what lets the counters count a redelivered attendance row once.

A seen set is no Redis key -- no kind, no TYPE reply, no command; ``DEL``,
``EXISTS`` and ``scan_iter`` do not see it -- so the client keeps its own
registry of live sets, by name, as it does for the tallies.  ``FLUSHALL`` frees
them; while no set exists it makes no further native call.

The attendance row is (lecture, id, floor(epoch / granularity)), folded in that
order (include/sketch.h, "seen-row sets"); ``seen_row_keys`` restates the fold
in Python and is the oracle of the device's."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoding import encode, pack
from .engine import DeviceBuffer, seen_add_keys, seen_info, seen_test_keys
from .exceptions import ResponseError
from .keyhash import murmur64a

SEEN_SEED0 = 0x9E3779B97F4A7C15  # kSeenSeed0 / kSeenSeed1 (csrc/sketch_common.h)
SEEN_SEED1 = 0xD1B54A32D192ED03


def seen_fold(keys, column) -> list:
    """One fold: every key word k becomes ``murmur64a(column item, seed=k)``.
    ``keys``: a list of ``(k0, k1)``; ``column``: one ``bytes`` per key."""
    return [(murmur64a(c, k0), murmur64a(c, k1)) for (k0, k1), c in zip(keys, column)]


def _lecture_bytes(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


def seen_row_keys(ids, times, lectures, granularity: int = 1) -> np.ndarray:
    """The attendance rows' keys, ``[n, 2]`` uint64, in pure Python: from the
    two seeds, fold the lecture bytes (``str(lecture).encode()``), the id bytes
    (as redis-py encodes them) and the 8 little-endian bytes of int64
    ``floor(epoch / granularity)``; a word 0 becomes 1."""
    from .analysis import epoch_seconds
    granularity = int(granularity)
    if granularity < 1:
        raise ValueError("granularity is at least 1 second")
    ids = [encode(i) for i in ids]
    lectures = [_lecture_bytes(x) for x in lectures]
    ep = epoch_seconds(times)
    if not len(ids) == len(lectures) == ep.size:
        raise ValueError("one time and one lecture per id")
    keys = [(SEEN_SEED0, SEEN_SEED1)] * len(ids)
    keys = seen_fold(keys, lectures)
    keys = seen_fold(keys, ids)
    keys = seen_fold(keys, [(int(e) // granularity).to_bytes(8, "little", signed=True) for e in ep])
    return np.asarray([(a or 1, b or 1) for a, b in keys], np.uint64).reshape(-1, 2)


class SeenMixin:
    def _seen_init_registry(self) -> None:
        self._seen: dict[bytes, int] = {}  # set name -> sid
        self._seen_free_ids = list(range(_lib.SKE_MAX_SEEN - 1, -1, -1))
        self._seen_bufs = None  # _seen_buffers

    def seen_create(self, name, capacity_log2: int = 22) -> int:
        """A new, empty set of 2^capacity_log2 slots of 24 bytes (half of them
        can hold rows); returns its native id."""
        name = encode(name)
        if name in self._seen:
            raise ResponseError(_lib.strerror(_lib.SKE_ESEENEXISTS))
        if not self._seen_free_ids:
            raise ResponseError("ERR too many seen sets on this device")
        if not _lib.SKE_SEEN_MIN_LOG2 <= int(capacity_log2) <= _lib.SKE_SEEN_MAX_LOG2:
            raise ResponseError(_lib.strerror(_lib.SKE_ESEENCAP))
        sid = self._seen_free_ids[-1]
        self.ctx.call("ske_seen_init", sid, int(capacity_log2))
        self._seen_free_ids.pop()
        self._seen[name] = sid
        return sid

    def seen_sid(self, name) -> int:
        sid = self._seen.get(encode(name))
        if sid is None:
            raise ResponseError(_lib.strerror(_lib.SKE_ESEENNOSET))
        return sid

    def seen_drop(self, name) -> bool:
        sid = self._seen.pop(encode(name), None)
        if sid is None:
            return False
        self.ctx.call("ske_seen_free", sid)
        self._seen_free_ids.append(sid)
        return True

    def _seen_release(self) -> None:
        for name in list(self._seen):
            self.seen_drop(name)

    def seen_reset(self, name) -> None:
        self.ctx.call("ske_seen_reset", self.seen_sid(name))

    def seen_info(self, name) -> dict:
        return seen_info(self.ctx, self.seen_sid(name))

    def seen_add_keys(self, name, keys, mask=None, want: int = 0) -> np.ndarray:
        """Raw keys, ``[n, 2]`` uint64: one answer byte per key
        (``SKE_SEEN_FIRST`` 0, ``SKE_SEEN_REPEAT`` 1, ``SKE_SEEN_SKIPPED`` 2
        where ``mask[i] != want``).  A word 0 behaves as 1."""
        return seen_add_keys(self.ctx, self.seen_sid(name), keys, mask, want)

    def seen_test_keys(self, name, keys) -> np.ndarray:
        """Whether each raw key is in the set (bool); nothing is inserted."""
        return seen_test_keys(self.ctx, self.seen_sid(name), keys)

    def _seen_buffers(self, n: int, nbytes: int) -> dict:
        """Device buffers of a batch of up to ``n`` rows whose longest column
        has ``nbytes`` bytes, kept between calls."""
        b = self._seen_bufs
        if b is None or b["n"] < n or b["nbytes"] < nbytes:
            if b is not None:
                for x in b.values():
                    if isinstance(x, DeviceBuffer):
                        x.free()
            cn, cb = max(n, 1024), max(nbytes, 1 << 14)
            b = {"n": cn, "nbytes": cb, "keys": DeviceBuffer(self.ctx, cn * 16 + 16),
                 "bytes": DeviceBuffer(self.ctx, cb + 64), "offs": DeviceBuffer(self.ctx, (cn + 1) * 4),
                 "epoch": DeviceBuffer(self.ctx, cn * 8 + 16), "out": DeviceBuffer(self.ctx, cn + 16)}
            self._seen_bufs = b
        return b

    def seen_fold_rows_packed(self, ids, ep: np.ndarray, lectures, granularity: int = 1) -> dict:
        """Upload the rows' three columns (``ids``, ``lectures``: packed
        ``(buf, offs)`` pairs; ``ep``: int64 seconds) and enqueue their folds;
        returns the buffers, the rows' keys in ``["keys"]``."""
        if int(granularity) < 1:
            raise ValueError("granularity is at least 1 second")
        n = ep.size
        (ibuf, ioffs), (lbuf, loffs) = ids, lectures
        if not ioffs.size == loffs.size == n + 1:
            raise ValueError("one time and one lecture per id")
        b = self._seen_buffers(n, max(int(ioffs[-1]), int(loffs[-1])))
        keys = C.c_void_p(b["keys"].ptr)
        for begin, (buf, offs) in ((1, (lbuf, loffs)), (0, (ibuf, ioffs))):
            # the copies run on the context stream, behind the fold that read the buffers before
            b["bytes"].from_host(buf[:int(offs[-1])])
            b["offs"].from_host(offs)
            self.ctx.call("ske_seen_fold_packed_async", keys, C.c_void_p(b["bytes"].ptr), C.c_void_p(b["offs"].ptr),
                          n, begin)
        b["epoch"].from_host(ep)
        self.ctx.call("ske_seen_fold_epoch_async", keys, C.c_void_p(b["epoch"].ptr), int(granularity), n, 0)
        return b

    def _seen_rows(self, ids, times, lectures, granularity):
        from .analysis import epoch_seconds
        ep = epoch_seconds(times)
        ids = pack(list(ids))
        lectures = pack([_lecture_bytes(x) for x in lectures])
        return self.seen_fold_rows_packed(ids, ep, lectures, granularity), ep.size

    def seen_add_rows(self, name, ids, times, lectures, granularity: int = 1) -> np.ndarray:
        """One batch of attendance rows: True where the row (lecture, id,
        ``floor(epoch / granularity)``) is seen for the first time -- by this
        set, and in this batch at its lowest index.  ``ids`` as redis-py
        encodes them, ``times`` in any form ``analysis.epoch_seconds`` takes,
        ``lectures`` as ``str(x).encode()``.  The keys are built on the device."""
        sid = self.seen_sid(name)
        b, n = self._seen_rows(ids, times, lectures, granularity)
        if n == 0:
            return np.zeros(0, bool)
        self.ctx.call("ske_seen_add_async", sid, C.c_void_p(b["keys"].ptr), n, None, 0, C.c_void_p(b["out"].ptr))
        self.ctx.call("ske_sync")
        return b["out"].to_host(np.uint8, n) == _lib.SKE_SEEN_FIRST

    def seen_test_rows(self, name, ids, times, lectures, granularity: int = 1) -> np.ndarray:
        """Whether each row is in the set (bool); nothing is inserted."""
        sid = self.seen_sid(name)
        b, n = self._seen_rows(ids, times, lectures, granularity)
        if n == 0:
            return np.zeros(0, bool)
        self.ctx.call("ske_seen_test_async", sid, C.c_void_p(b["keys"].ptr), n, C.c_void_p(b["out"].ptr))
        self.ctx.call("ske_sync")
        return b["out"].to_host(np.uint8, n).astype(bool)
