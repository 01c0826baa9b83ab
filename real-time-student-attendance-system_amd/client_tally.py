"""The tally part of ``SketchClient`` (csrc/sketch_api_tally.cpp): named exact
event counts per key -- the group-by-count of a string column.

A tally is no Redis key -- it has no kind, no TYPE reply and no command in
``execute_command``; ``DEL``, ``EXISTS`` and ``scan_iter`` do not see it -- so
the client keeps its own registry of live tallies, by name.  ``FLUSHALL``
frees them; while no tally exists it makes no further native call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import SKE_MEM_HOST, ptr as _ptr
from .encoding import encode, pack
from .engine import tally_import, tally_info, tally_list, tally_query, tally_top
from .exceptions import ResponseError

TALLY_BY = {"events": 0, "valid": 1}


class TallyMixin:
    def _tally_init_registry(self) -> None:
        self._tally: dict[bytes, int] = {}  # tally name -> tid
        self._tally_free_ids = list(range(_lib.SKE_MAX_TALLY - 1, -1, -1))

    def tally_create(self, name, capacity_log2: int = 16) -> int:
        """A new, empty tally of 2^capacity_log2 slots (half of them can hold
        keys); returns its native id."""
        name = encode(name)
        if name in self._tally:
            raise ResponseError(_lib.strerror(_lib.SKE_ETALLYEXISTS))
        if not self._tally_free_ids:
            raise ResponseError("ERR too many tallies on this device")
        if not _lib.SKE_TALLY_MIN_LOG2 <= int(capacity_log2) <= _lib.SKE_TALLY_MAX_LOG2:
            raise ResponseError(_lib.strerror(_lib.SKE_ETALLYCAP))
        tid = self._tally_free_ids[-1]
        self.ctx.call("ske_tally_init", tid, int(capacity_log2))
        self._tally_free_ids.pop()
        self._tally[name] = tid
        return tid

    def tally_tid(self, name) -> int:
        tid = self._tally.get(encode(name))
        if tid is None:
            raise ResponseError(_lib.strerror(_lib.SKE_ETALLYNOSET))
        return tid

    def tally_free(self, name) -> bool:
        tid = self._tally.pop(encode(name), None)
        if tid is None:
            return False
        self.ctx.call("ske_tally_free", tid)
        self._tally_free_ids.append(tid)
        return True

    def _tally_release(self) -> None:
        for name in list(self._tally):
            self.tally_free(name)

    def tally_reset(self, name) -> None:
        self.ctx.call("ske_tally_reset", self.tally_tid(name))

    def tally_info(self, name) -> dict:
        return tally_info(self.ctx, self.tally_tid(name))

    def tally_add_packed(self, name, buf: np.ndarray, offs: np.ndarray, valid=None) -> None:
        """One packed host batch of keys (``encoding.pack``'s layout): every key
        counts one event, and one valid where its ``valid`` byte is 1.  Uploads,
        adds, returns when done."""
        tid = self.tally_tid(name)
        n = len(offs) - 1
        m = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
        if m is not None and m.size != n:
            raise ValueError("one valid byte per key")
        if n > 0:
            self.ctx.call("ske_tally_add", tid, _ptr(np.ascontiguousarray(buf, np.uint8)),
                          _ptr(np.ascontiguousarray(offs, np.uint32)), n, _ptr(m), SKE_MEM_HOST)

    def tally_add(self, name, keys, valid=None) -> None:
        """A host sequence of keys, encoded as redis-py would."""
        buf, offs = pack(keys)
        self.tally_add_packed(name, buf, offs, valid)

    def tally_query(self, name, keys):
        """``(events, valid)``, u64 per key; 0, 0 for a key never counted."""
        buf, offs = pack(keys)
        return tally_query(self.ctx, self.tally_tid(name), buf, offs)

    def tally_list(self, name, min_events: int = 0):
        """``(keys, events, valid, complete)``: the entries with at least
        ``min_events`` events, largest first (engine.tally_list)."""
        return tally_list(self.ctx, self.tally_tid(name), min_events)

    def tally_top(self, name, k: int = 3, by: str = "events"):
        """``(head, tail, complete)``: the first and last ``k`` entries of the
        listing's order by ``events`` or by ``valid``, each end as ``(keys,
        events, valid)``, the tail in list order (engine.tally_top)."""
        if by not in TALLY_BY:
            raise ValueError('by is "events" or "valid"')
        if not 1 <= int(k) <= _lib.SKE_TALLY_MAX_TOP:
            raise ValueError(f"k is between 1 and {_lib.SKE_TALLY_MAX_TOP}")
        return tally_top(self.ctx, self.tally_tid(name), k, TALLY_BY[by])

    def tally_export_dev(self, name, keys, lens, events, valid, cap: int) -> int:
        """Every entry, unordered, into device arrays of ``cap`` entries
        (``keys``: 32 zero-padded bytes each, 8-byte aligned; ``lens`` u32;
        ``events`` / ``valid`` u64); returns how many.  More entries than
        ``cap`` raises (SKE_ETALLYSPACE)."""
        n = C.c_uint64(0)
        self.ctx.call("ske_tally_export_dev", self.tally_tid(name), _lib.devptr(keys), _lib.devptr(lens),
                      _lib.devptr(events), _lib.devptr(valid), int(cap), C.byref(n))
        return int(n.value)

    def tally_merge_dev(self, name, keys, lens, events, valid, n: int, dropped_events: int = 0,
                        dropped_valid: int = 0, foreign_overflow: int = 0) -> None:
        """Insert-or-add of the ``n`` entries of another tally's export; the
        head takes the source's ``dropped_*`` and overflow (its
        ``tally_info``).  Enqueue only: the arrays stay as they are until the
        context's stream has run."""
        self.ctx.call("ske_tally_merge_dev", self.tally_tid(name), _lib.devptr(keys), _lib.devptr(lens),
                      _lib.devptr(events), _lib.devptr(valid), int(n), int(dropped_events), int(dropped_valid),
                      1 if foreign_overflow else 0)

    def tally_import(self, name, keys, events, valid) -> None:
        """Insert-or-add of a listing (another tally's, another rank's)."""
        tally_import(self.ctx, self.tally_tid(name), [encode(k) for k in keys], events, valid)
