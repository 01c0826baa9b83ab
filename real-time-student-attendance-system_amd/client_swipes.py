"""The fused hot path of ``SketchClient`` (csrc/sketch_api_swipes.cpp):
BF.EXISTS then valid-gated PFADD for a whole batch of events."""
from __future__ import annotations

import numpy as np

from ._lib import SKE_MEM_HOST, ptr as _ptr
from .encoding import encode, pack
from .exceptions import DataError


class SwipesMixin:
    def swipes(self, bf_key, hll_keys, items=None, *, packed=None) -> np.ndarray:
        """Batched attendance_processor.py:109-129: for every event
        ``valid = BF.EXISTS bf_key id``; if valid ``PFADD hll_key id``.

        ``hll_keys``: one key for the whole batch or one key per item.
        ``items``: ids (encoded as redis-py does) or ``packed=(buf, offs)``.
        Returns the per-event validity (bool array).  HLL keys that receive
        no valid event are not created, exactly as in the per-event loop."""
        if packed is None:
            buf, offs = pack(items)
        else:
            buf, offs = packed
            buf = np.ascontiguousarray(buf, np.uint8)
            offs = np.ascontiguousarray(offs, np.uint32)
        n = len(offs) - 1
        bkey = encode(bf_key)
        has_bf = self.keys.expect(bkey, "bf")
        if n == 0:
            return np.zeros(0, bool)
        if isinstance(hll_keys, (str, bytes, int, float)):
            key_list = [encode(hll_keys)]
            slot_idx = np.zeros(n, np.int64)
        else:
            hk = [encode(k) for k in hll_keys]
            if len(hk) != n:
                raise DataError("hll_keys must be one key or one key per item")
            uniq = {}
            slot_idx = np.fromiter((uniq.setdefault(k, len(uniq)) for k in hk), np.int64, count=n)
            key_list = list(uniq)
        for k in key_list:
            self.keys.expect(k, "hll")
        tentative = [k for k in key_list if k not in self.keys.slot]
        key_slots = np.asarray([self.keys.slot[k] if k in self.keys.slot else self.keys.new_slot(k)
                                for k in key_list], dtype=np.uint32)
        slots = key_slots[slot_idx]
        valid = np.zeros(n, np.uint8)
        if has_bf:
            self.ctx.call("ske_swipes", self.keys.fid[bkey], _ptr(slots), _ptr(buf), _ptr(offs), n,
                          _ptr(valid), SKE_MEM_HOST)
        if tentative:
            hit = np.zeros(len(key_list), bool)
            hit[np.unique(slot_idx[valid.astype(bool)])] = True
            for k in tentative:
                if not hit[key_list.index(k)]:
                    self.keys.release_unused_slot(k)
        return valid.astype(bool)

    def swipes_slots(self, bf_key, slots: np.ndarray, buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
        """``swipes`` with keys already resolved to slots (see ``key_slot``)."""
        n = len(offs) - 1
        valid = np.zeros(n, np.uint8)
        bkey = encode(bf_key)
        if n and self.keys.expect(bkey, "bf"):
            s = np.ascontiguousarray(slots, dtype=np.uint32)
            self.ctx.call("ske_swipes", self.keys.fid[bkey], _ptr(s), _ptr(buf), _ptr(offs), n,
                          _ptr(valid), SKE_MEM_HOST)
        return valid.astype(bool)

    def swipes_fixed(self, bf_key, slots: np.ndarray, ids: np.ndarray) -> np.ndarray:
        """``swipes_slots`` for ids of one fixed width: ``ids`` is a [n, width]
        uint8 array of the ids' bytes (e.g. 8-digit student ids as redis-py
        encodes them).  Through ske_swipes_fixed_bits: no offsets cross the
        host link and the answers come back 1 bit per swipe, in chunks that
        overlap the copies with the kernels."""
        ids = np.ascontiguousarray(ids, dtype=np.uint8)
        if ids.ndim != 2:
            raise ValueError("ids must be a [n, width] uint8 array")
        n, width = ids.shape
        bits = np.zeros((n + 7) // 8, np.uint8)
        bkey = encode(bf_key)
        if n and width and self.keys.expect(bkey, "bf"):
            s = np.ascontiguousarray(slots, dtype=np.uint32)
            if s.shape != (n,):
                raise ValueError("one slot per id")
            self.ctx.call("ske_swipes_fixed_bits", self.keys.fid[bkey], _ptr(s), _ptr(ids), width, n,
                          _ptr(bits), SKE_MEM_HOST)
        return np.unpackbits(bits, count=n, bitorder="little").astype(bool)
