"""The time-profile part of ``SketchClient`` (csrc/sketch_api_tp.cpp): named
weekday x hour counters of the swipes' times.

A profile is no Redis key -- it has no kind, no TYPE reply and no command in
``execute_command``; ``DEL``, ``EXISTS`` and ``scan_iter`` do not see it -- so
the client keeps its own registry of live profiles, by name.  ``FLUSHALL``
frees them; while no profile exists it makes no further native call."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoding import encode
from .engine import DeviceBuffer, tp_counts
from .exceptions import ResponseError


class TimeProfileMixin:
    def _tp_init_registry(self) -> None:
        self._tp: dict[bytes, int] = {}  # profile name -> tid
        self._tp_free_ids = list(range(_lib.SKE_MAX_TP - 1, -1, -1))

    def tp_create(self, name) -> int:
        """A new profile, every counter zero; returns its native id."""
        name = encode(name)
        if name in self._tp:
            raise ResponseError(_lib.strerror(_lib.SKE_ETPEXISTS))
        if not self._tp_free_ids:
            raise ResponseError("ERR too many time profiles on this device")
        tid = self._tp_free_ids[-1]
        self.ctx.call("ske_tp_init", tid)
        self._tp_free_ids.pop()
        self._tp[name] = tid
        return tid

    def tp_tid(self, name) -> int:
        tid = self._tp.get(encode(name))
        if tid is None:
            raise ResponseError(_lib.strerror(_lib.SKE_ETPNOSET))
        return tid

    def tp_free(self, name) -> bool:
        tid = self._tp.pop(encode(name), None)
        if tid is None:
            return False
        self.ctx.call("ske_tp_free", tid)
        self._tp_free_ids.append(tid)
        return True

    def _tp_release(self) -> None:
        for name in list(self._tp):
            self.tp_free(name)

    def tp_reset(self, name) -> None:
        self.ctx.call("ske_tp_reset", self.tp_tid(name))

    def tp_counts(self, name) -> np.ndarray:
        """The counters, [7, 24] uint64: weekday (Monday first) by hour, UTC."""
        return tp_counts(self.ctx, self.tp_tid(name))

    def tp_add(self, name, times, mask=None, want: int = 1) -> None:
        """Host arrays: ``times`` in any form ``analysis.epoch_seconds`` takes,
        ``mask`` one byte per swipe (only those equal to ``want`` count).
        Uploads, adds, returns when done."""
        from .analysis import epoch_seconds
        tid = self.tp_tid(name)
        ep = epoch_seconds(times)
        n = ep.size
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
        if m is not None and m.size != n:
            raise ValueError("one mask byte per time")
        if n == 0:
            return
        d_ep = DeviceBuffer(self.ctx, n * 8)
        d_m = DeviceBuffer(self.ctx, n + 16) if m is not None else None
        try:
            d_ep.from_host(ep)
            if d_m:
                d_m.from_host(m)
            self.ctx.call("ske_tp_add_async", tid, C.c_void_p(d_ep.ptr), n, C.c_void_p(d_m.ptr) if d_m else None,
                          int(want), 86400, None)
            self.ctx.call("ske_sync")
        finally:
            d_ep.free()
            if d_m:
                d_m.free()
