"""The heavy-hitter half of ``SketchClient`` (csrc/sketch_api_hh.cpp): sets of
ids whose Count-Min estimate reached a threshold, each bound to a CMS key.

A set is no Redis key -- it has no kind, no TYPE reply and no command in
``execute_command`` (RedisBloom's own TOPK cannot be matched bit for bit,
DESIGN.md "Heavy hitters") -- so the client keeps its own registry of live
sets, by name.  ``DEL`` of the bound CMS key and ``FLUSHALL`` free them; while
no set exists neither makes any further native call."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import SKE_MEM_HOST, ptr as _ptr
from .encoding import encode
from .engine import hh_info, hh_list, hh_select, hh_stats
from .exceptions import ResponseError


class HhMixin:
    def _hh_init_registry(self) -> None:
        self._hh: dict[bytes, tuple[int, bytes]] = {}  # set name -> (hid, the CMS key it reads)
        self._hh_free_ids = list(range(_lib.SKE_MAX_HH - 1, -1, -1))

    def hh_create(self, name, cms_key, capacity_log2: int = 16) -> int:
        """A new, empty set of 2^capacity_log2 slots bound to an existing CMS
        key; returns its native id."""
        name, key = encode(name), encode(cms_key)
        if name in self._hh:
            raise ResponseError(_lib.strerror(_lib.SKE_EHHEXISTS))
        self.cms_cid(key)  # the key must exist and be a CMS key
        if not self._hh_free_ids:
            raise ResponseError("ERR too many heavy-hitter sets on this device")
        if not _lib.SKE_HH_MIN_LOG2 <= int(capacity_log2) <= _lib.SKE_HH_MAX_LOG2:
            raise ResponseError(_lib.strerror(_lib.SKE_EHHCAP))
        hid = self._hh_free_ids[-1]
        self.ctx.call("ske_hh_init", hid, int(capacity_log2))
        self._hh_free_ids.pop()
        self._hh[name] = (hid, key)
        return hid

    def _hh_entry(self, name) -> tuple[int, int]:
        """(hid, cid) of a live set; the bound key is looked up now."""
        e = self._hh.get(encode(name))
        if e is None:
            raise ResponseError(_lib.strerror(_lib.SKE_EHHNOSET))
        return e[0], self.cms_cid(e[1])

    def hh_free(self, name) -> bool:
        e = self._hh.pop(encode(name), None)
        if e is None:
            return False
        self.ctx.call("ske_hh_free", e[0])
        self._hh_free_ids.append(e[0])
        return True

    def _hh_release(self, cms_key: bytes | None) -> None:
        """Free the sets bound to a key that is going away (None: all)."""
        for name in [n for n, (_, k) in self._hh.items() if cms_key is None or k == cms_key]:
            self.hh_free(name)

    def hh_reset(self, name) -> None:
        self.ctx.call("ske_hh_reset", self._hh_entry(name)[0])

    def hh_info(self, name) -> dict:
        return hh_info(self.ctx, self._hh_entry(name)[0])

    def hh_track_packed(self, name, buf: np.ndarray, offs: np.ndarray, threshold: int) -> None:
        """Every id of the packed batch whose estimate in the bound key is at
        least ``threshold`` joins the set (after the batch's own adds)."""
        hid, cid = self._hh_entry(name)
        n = len(offs) - 1
        if n > 0:
            self.ctx.call("ske_hh_track", hid, cid, _ptr(np.ascontiguousarray(buf, np.uint8)),
                          _ptr(np.ascontiguousarray(offs, np.uint32)), n, int(threshold), SKE_MEM_HOST)

    def hh_list(self, name, threshold: int):
        """``(ids, estimates, complete)``: the members whose current estimate
        is at least ``threshold``, largest first (engine.hh_list)."""
        hid, cid = self._hh_entry(name)
        return hh_list(self.ctx, hid, cid, threshold)

    def hh_stats(self, name, threshold: int = 0) -> dict:
        """The statistics of the members whose current estimate is at least
        ``threshold`` (0: every member), computed on the device
        (``derive_stats`` of engine.hh_stats): ``n``, ``sum``, ``sumsq``,
        ``min``, ``max``, ``median``, ``mean``, ``std``, ``complete``."""
        hid, cid = self._hh_entry(name)
        return derive_stats(hh_stats(self.ctx, hid, cid, threshold))

    def hh_select(self, name, ranks, threshold: int = 0) -> np.ndarray:
        """The ``ranks[j]``-th smallest of those estimates (0-based, any order,
        repeats allowed) as uint32; more than SKE_HH_MAX_RANKS ranks go in
        several calls."""
        hid, cid = self._hh_entry(name)
        r = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
        step = _lib.SKE_HH_MAX_RANKS
        parts = [hh_select(self.ctx, hid, cid, threshold, r[i:i + step]) for i in range(0, r.size, step)]
        return np.concatenate(parts) if parts else np.zeros(0, np.uint32)

    def hh_export_dev(self, name, ids, lens, cap: int) -> tuple[int, int]:
        """Every member, unordered, into device arrays of ``cap`` entries
        (``ids``: 16 zero-padded bytes each, 8-byte aligned; ``lens``: u32);
        returns ``(members, the set's overflow word)``.  More members than
        ``cap`` raises (SKE_EHHSPACE)."""
        n, ov = C.c_uint64(0), C.c_uint32(0)
        self.ctx.call("ske_hh_export_dev", self._hh_entry(name)[0], _lib.devptr(ids), _lib.devptr(lens), int(cap),
                      C.byref(n), C.byref(ov))
        return int(n.value), int(ov.value)

    def hh_merge_dev(self, name, ids, lens, n: int, foreign_overflow: int = 0) -> None:
        """The ``n`` entries of another set's export join this one (no
        threshold); ``foreign_overflow``: the source's overflow word.  Enqueue
        only: the arrays stay as they are until the context's stream has run."""
        self.ctx.call("ske_hh_merge_dev", self._hh_entry(name)[0], _lib.devptr(ids), _lib.devptr(lens), int(n),
                      1 if foreign_overflow else 0)

    def hh_quantile(self, name, q: float, threshold: int = 0) -> float:
        """The ``q``-quantile of those estimates as ``np.quantile`` computes it
        by default: linear interpolation at position ``q * (n - 1)`` between
        the two order statistics around it; ``nan`` over no member."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError("a quantile is between 0 and 1")
        hid, cid = self._hh_entry(name)
        n = hh_stats(self.ctx, hid, cid, threshold)["n"]
        if n == 0:
            return float("nan")
        pos = q * (n - 1)
        lo = min(int(math.floor(pos)), n - 1)
        hi = min(lo + 1, n - 1)
        a, b = (float(v) for v in hh_select(self.ctx, hid, cid, threshold, [lo, hi]))
        return a + (b - a) * (pos - lo)


def derive_stats(raw: dict) -> dict:
    """engine.hh_stats' integers as the dict ``hh_stats`` returns.  ``sumsq``
    is a Python int; ``median`` is the mean of the two middle order statistics
    (exact in float64); ``std`` is the sample standard deviation (``ddof=1``, as
    pandas; ``nan`` when ``n < 2``) from the exact integer variance numerator
    ``n * sumsq - sum * sum``: one correctly rounded division and one square
    root, no float sum."""
    n, s = raw["n"], raw["sum"]
    sumsq = raw["sq_hi"] * 2 ** 32 + raw["sq_lo"]
    nan = float("nan")
    return {"n": n, "sum": s, "sumsq": sumsq, "min": raw["min"], "max": raw["max"],
            "median": (raw["med_lo"] + raw["med_hi"]) / 2 if n else nan,
            "mean": s / n if n else nan,
            "std": math.sqrt((n * sumsq - s * s) / (n * (n - 1))) if n >= 2 else nan,
            "complete": bool(raw["complete"])}
