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
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import SKE_MEM_DEVICE
from .encoding import encode, pack
from .engine import DeviceBuffer


class StudentCounts:
    """Attended / invalid swipe counts per student id, as two CMS keys of a
    ``SketchClient``."""

    def __init__(self, client, attended_key="cms:attended", invalid_key="cms:invalid",
                 error: float = 0.001, probability: float = 0.01):
        self.client = client
        self.attended_key, self.invalid_key = attended_key, invalid_key
        for key in (attended_key, invalid_key):
            if client.keys.type_of(encode(key)) is None:
                client.cms_initbyprob(key, error, probability)
            client.keys.expect(encode(key), "cms")  # WRONGTYPE for a key of another kind
        self._bufs = None

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
