"""The HyperLogLog half of ``SketchClient`` (csrc/sketch_api_hll.cpp): PFADD /
PFCOUNT / PFMERGE over the register slab, and the keys as Redis strings."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import formats
from ._lib import SKE_MEM_HOST, HLL_DENSE_BYTES, HLL_REGISTERS, ptr as _ptr
from .commands import arity_error
from .encoding import encode, pack
from .exceptions import DataError, ResponseError


class HllMixin:
    def pfadd_calls(self, calls: Sequence[tuple]) -> list[int]:
        """Several PFADD calls executed as one device batch with Redis's
        sequential replies: call c replies 1 if it created its key or any of
        its elements raised a register given all elements before it."""
        keys = [encode(c[0]) for c in calls]
        for k in keys:  # type check before any side effect
            self.keys.expect(k, "hll")
        created = []
        slots = []
        seen_new = set()
        for k in keys:
            if k in self.keys.slot:
                slots.append(self.keys.slot[k])
                created.append(False)
            else:
                slots.append(self.keys.new_slot(k))
                created.append(k not in seen_new)
                seen_new.add(k)
        elems, owner = [], []
        for ci, c in enumerate(calls):
            for v in c[1:]:
                elems.append(v)
                owner.append(ci)
        replies = [1 if cr else 0 for cr in created]
        if elems:
            buf, offs = pack(elems)
            slot_arr = np.asarray([slots[o] for o in owner], dtype=np.uint32)
            changed = np.zeros(len(elems), np.uint8)
            self.ctx.call("ske_hll_pfadd", _ptr(slot_arr), _ptr(buf), _ptr(offs), len(elems),
                          _ptr(changed), SKE_MEM_HOST)
            any_changed = np.zeros(len(calls), np.uint8)
            np.maximum.at(any_changed, np.asarray(owner, dtype=np.int64), changed)
            replies = [1 if (replies[i] or any_changed[i]) else 0 for i in range(len(calls))]
        return replies

    def pfadd(self, name, *values) -> int:
        return self.pfadd_calls([(name, *values)])[0]

    def pfadd_packed(self, slots: np.ndarray, buf: np.ndarray, offs: np.ndarray,
                     changed: bool = False) -> np.ndarray | None:
        """PFADD of (slot, element) pairs already resolved to slots."""
        n = len(offs) - 1
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(n, np.uint8) if changed else None
        if n:
            self.ctx.call("ske_hll_pfadd", _ptr(slots), _ptr(buf), _ptr(offs), n, _ptr(out),
                          SKE_MEM_HOST)
        return out

    def _count_slots(self, names) -> list[int]:
        slots = []
        for n in names:
            k = encode(n)
            if self.keys.expect(k, "hll"):
                slots.append(self.keys.slot[k])
        return slots

    def pfcount(self, *sources) -> int:
        if not sources:
            raise arity_error("pfcount")
        slots = self._count_slots(sources)
        if not slots:
            return 0
        arr = np.asarray(slots, dtype=np.uint32)
        out = np.zeros(1, np.uint64)
        self.ctx.call("ske_hll_pfcount", _ptr(arr), len(slots), _ptr(out))
        return int(out[0])

    def pfcount_each(self, keys: Sequence) -> np.ndarray:
        """PFCOUNT of every key separately, one device launch (K2)."""
        slots = []
        present = []
        for n in keys:
            k = encode(n)
            ok = self.keys.expect(k, "hll")
            present.append(ok)
            slots.append(self.keys.slot[k] if ok else 0)
        out = np.zeros(len(slots), np.uint64)
        idx = np.flatnonzero(present)
        if idx.size:
            arr = np.asarray([slots[i] for i in idx], dtype=np.uint32)
            sub = np.zeros(idx.size, np.uint64)
            self.ctx.call("ske_hll_pfcount_each", _ptr(arr), arr.size, _ptr(sub), SKE_MEM_HOST)
            out[idx] = sub
        return out

    def pfcount_groups(self, groups: Sequence[Sequence]) -> np.ndarray:
        """PFCOUNT(k1 k2 ...) for many key groups in one launch (unions)."""
        slots, goffs = [], [0]
        for g in groups:
            slots.extend(self._count_slots(g))
            goffs.append(len(slots))
        out = np.zeros(len(groups), np.uint64)
        if groups:
            s = np.asarray(slots if slots else [0], dtype=np.uint32)
            go = np.asarray(goffs, dtype=np.uint32)
            self.ctx.call("ske_hll_pfcount_groups", _ptr(s), _ptr(go), len(groups), _ptr(out),
                          SKE_MEM_HOST)
        return out

    def pfmerge(self, dest, *sources) -> bool:
        d = encode(dest)
        src = [encode(s) for s in sources]
        for k in src:
            self.keys.expect(k, "hll")
        if not self.keys.expect(d, "hll"):
            self.keys.new_slot(d)
        slots = np.asarray([self.keys.slot[k] for k in src if k in self.keys.slot], dtype=np.uint32)
        self.ctx.call("ske_hll_pfmerge", self.keys.slot[d], _ptr(slots), slots.size)
        return True

    def hll_registers(self, name) -> np.ndarray:
        """Raw registers (Redis HLL_RAW view, one byte per register)."""
        k = encode(name)
        out = np.zeros(HLL_REGISTERS, np.uint8)
        if self.keys.expect(k, "hll"):
            self.ctx.call("ske_hll_export_raw", self.keys.slot[k], _ptr(out))
        return out

    def hll_dense(self, name) -> bytes:
        """The 12288-byte HLL_DENSE register payload of the key."""
        k = encode(name)
        if not self.keys.expect(k, "hll"):
            raise ResponseError("ERR no such key")
        out = np.zeros(HLL_DENSE_BYTES, np.uint8)
        self.ctx.call("ske_hll_export_dense", self.keys.slot[k], _ptr(out))
        return out.tobytes()

    def hll_load_registers(self, name, regs: np.ndarray) -> None:
        k = encode(name)
        if not self.keys.expect(k, "hll"):
            self.keys.new_slot(k)
        r = np.ascontiguousarray(regs, dtype=np.uint8)
        if r.shape != (HLL_REGISTERS,):
            raise DataError("expected 16384 registers")
        self.ctx.call("ske_hll_import_raw", self.keys.slot[k], _ptr(r))

    def dump_hll(self, name) -> bytes | None:
        """The key as Redis stores it (GET of an HLL key): "HYLL" header +
        canonical sparse or dense payload (formats.encode_hll)."""
        k = encode(name)
        if not self.keys.expect(k, "hll"):
            return None
        return formats.encode_hll(self.hll_registers(k))

    def load_hll(self, name, value: bytes) -> None:
        """SET of a Redis HLL string (dense or sparse) into a key."""
        regs = formats.decode_hll(bytes(value))
        k = encode(name)
        if k in self.keys.kind and self.keys.kind[k] != "hll":
            self.keys.drop(k)  # SET replaces a key of any type
        self.hll_load_registers(k, regs)

    def key_slot(self, name, create: bool = True) -> int:
        """Slot of an HLL key (creating it when asked) for batched calls."""
        k = encode(name)
        if self.keys.expect(k, "hll"):
            return self.keys.slot[k]
        if not create:
            raise ResponseError("ERR no such key")
        return self.keys.new_slot(k)
