"""The HyperLogLog half of ``SketchClient`` (csrc/sketch_api_hll.cpp): PFADD /
PFCOUNT / PFMERGE over the register slab, and the keys as Redis strings: one
key a call on the host (``dump_hll`` / ``load_hll``), many keys a call encoded
and decoded on the device (``dump_hlls`` / ``load_hlls``, csrc/sketch_hll_fmt.hip),
and a file of them (``save_hlls`` / ``restore_hlls``)."""
from __future__ import annotations

from typing import Sequence

import numpy as np

from . import formats
from ._lib import (SKE_EBADHLL, SKE_HLL_DUMP_CARD, SKE_HLL_DUMP_MAX_KEYS, SKE_MEM_HOST, HLL_DENSE_BYTES,
                   HLL_REGISTERS, SketchLibError, ptr as _ptr)
from .commands import arity_error
from .encoding import encode, pack
from .exceptions import DataError, ResponseError
from .keyspace import redis_glob

# a string longer than the header and the longest valid sparse payload (16384
# XZERO opcodes of run 1) cannot be valid: load_hlls refuses it without a copy
_HLL_STRING_MAX = formats.HLL_HDR + 2 * HLL_REGISTERS
_LOAD_CALL_BYTES = 1 << 31  # blob bytes per ske_hll_load call (u32 offsets)


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

    # ------------------------------------------------------------ many keys a call
    def dump_hlls(self, names: Sequence, with_card: bool = False, sparse_max_bytes: int = 3000,
                  chunk_keys: int | None = None) -> list:
        """``dump_hll`` of every name, encoded on the device: entry i is the
        key as Redis stores it, None for a missing key; a key of another type
        raises before anything runs.  ``with_card``: the header caches the
        key's PFCOUNT (``formats.cached_card``) instead of the invalid mark.
        ``chunk_keys``: keys per ske_hll_dump call (default the ABI's most)."""
        keys = [encode(n) for n in names]
        have = [i for i, k in enumerate(keys) if self.keys.expect(k, "hll")]
        out: list = [None] * len(keys)
        chunk = int(chunk_keys) if chunk_keys else SKE_HLL_DUMP_MAX_KEYS
        if chunk < 1:
            raise ValueError("chunk_keys must be positive")
        for c0 in range(0, len(have), chunk):
            part = have[c0:c0 + chunk]
            slots = np.asarray([self.keys.slot[keys[i]] for i in part], dtype=np.uint32)
            blob, offs = self.dump_slots(slots, with_card, sparse_max_bytes)
            for j, i in enumerate(part):
                out[i] = blob[int(offs[j]):int(offs[j + 1])].tobytes()
        return out

    def dump_slots(self, slots: np.ndarray, with_card: bool = False,
                   sparse_max_bytes: int = 3000) -> tuple[np.ndarray, np.ndarray]:
        """The strings of up to SKE_HLL_DUMP_MAX_KEYS slab slots as one blob
        (u8) and their offsets (u32, one more than slots): the sizes first,
        then the strings into a buffer of exactly that size."""
        slots = np.ascontiguousarray(slots, dtype=np.uint32)
        offs = np.zeros(slots.size + 1, np.uint32)
        self.ctx.call("ske_hll_dump_sizes", _ptr(slots), slots.size, int(sparse_max_bytes), _ptr(offs),
                      SKE_MEM_HOST)
        blob = np.zeros(int(offs[-1]), np.uint8)
        self.ctx.call("ske_hll_dump", _ptr(slots), slots.size, int(sparse_max_bytes),
                      SKE_HLL_DUMP_CARD if with_card else 0, _ptr(blob), blob.size, _ptr(offs), SKE_MEM_HOST)
        return blob, offs

    @staticmethod
    def _raise_bad_hll(value: bytes):
        """load_hll's error for a string the device refused."""
        formats.decode_hll(value)  # WRONGTYPE / INVALIDOBJ as load_hll raises them
        # a dense register above 51: decode_hll lets it pass, ske_hll_import_raw does not
        raise SketchLibError(SKE_EBADHLL, formats.INVALIDOBJ)

    @staticmethod
    def _host_refuses(value: bytes) -> bool:
        try:
            return int(formats.decode_hll(value).max(initial=0)) > 51
        except ResponseError:
            return True

    def load_hlls(self, pairs, chunk_keys: int | None = None) -> None:
        """``load_hll`` of every (name, string) pair in order, decoded on the
        device: new keys get slots, a key of another type is replaced, a name
        that repeats ends up with its last good string.  A string that is not a
        valid HLL string raises ``load_hll``'s error for the first such pair --
        after every good pair is in; a name with no good string is not created
        (and a key it names stays as it was)."""
        items = [(encode(n), bytes(v)) for n, v in pairs]
        chunk = int(chunk_keys) if chunk_keys else SKE_HLL_DUMP_MAX_KEYS
        if chunk < 1:
            raise ValueError("chunk_keys must be positive")
        first_bad = None
        pending: dict[bytes, list[int]] = {}  # name -> its pairs, in order
        for i, (k, _) in enumerate(items):
            pending.setdefault(k, []).append(i)
        while pending:
            # every name's last pair not yet refused
            batch = []
            for k, idxs in pending.items():
                v = items[idxs[-1]][1]
                kind = self.keys.kind.get(k)
                if len(v) > _HLL_STRING_MAX or (kind not in (None, "hll") and self._host_refuses(v)):
                    batch.append((k, None))  # refused here: too long, or it must not replace the other key
                    continue
                if kind not in (None, "hll"):
                    self.keys.drop(k)  # SET replaces a key of any type
                batch.append((k, v))
            bad = [k for k, v in batch if v is None]
            send = [(k, v) for k, v in batch if v is not None]
            c0 = 0
            while c0 < len(send):
                c1, nbytes = c0, 0
                while c1 < len(send) and c1 - c0 < chunk and nbytes + len(send[c1][1]) <= _LOAD_CALL_BYTES:
                    nbytes += len(send[c1][1])
                    c1 += 1
                bad += self._load_batch(send[c0:c1])
                c0 = c1
            nxt = {}
            for k in bad:
                idxs = pending[k]
                i = idxs.pop()
                first_bad = i if first_bad is None else min(first_bad, i)
                if idxs:
                    nxt[k] = idxs
            pending = nxt
        if first_bad is not None:
            self._raise_bad_hll(items[first_bad][1])

    def _load_batch(self, batch: list) -> list:
        """One ske_hll_load of (name, string) pairs with distinct names; the
        names whose string the device refused (a name it created for them is
        taken back)."""
        created = []
        slots = np.zeros(len(batch), np.uint32)
        for j, (k, _) in enumerate(batch):
            if k in self.keys.slot:
                slots[j] = self.keys.slot[k]
            else:
                slots[j] = self.keys.new_slot(k)
                created.append(k)
        offs = np.zeros(len(batch) + 1, np.uint32)
        np.cumsum([len(v) for _, v in batch], out=offs[1:])
        blob = np.frombuffer(b"".join(v for _, v in batch), dtype=np.uint8)
        status = np.zeros(len(batch), np.uint8)
        try:
            self.ctx.call("ske_hll_load", _ptr(slots), len(batch), _ptr(blob) if blob.size else None, _ptr(offs),
                          _ptr(status), SKE_MEM_HOST)
        except SketchLibError as e:
            if e.code != SKE_EBADHLL:
                for k in created:
                    self.keys.release_unused_slot(k)
                raise
        bad = [batch[j][0] for j in np.flatnonzero(status)]
        made = set(created)
        for k in bad:
            if k in made:
                self.keys.release_unused_slot(k)  # its row was never written
        return bad

    def save_hlls(self, path, match="*") -> int:
        """Every HLL key whose name matches (Redis' glob) into one ``.npz``
        file at ``path``: the packed key names and their offsets, the keys'
        Redis strings as one blob and their offsets.  The container is this
        project's own; the strings are Redis'.  Returns the number of keys."""
        pat = encode(match)
        keys = sorted(k for k, kind in self.keys.kind.items()
                      if kind == "hll" and (pat == b"*" or redis_glob(pat, k)))
        blobs, offs, total = [], [np.zeros(1, np.uint64)], 0
        for c0 in range(0, len(keys), SKE_HLL_DUMP_MAX_KEYS):
            slots = np.asarray([self.keys.slot[k] for k in keys[c0:c0 + SKE_HLL_DUMP_MAX_KEYS]], dtype=np.uint32)
            blob, o = self.dump_slots(slots)
            blobs.append(blob)
            offs.append(o[1:].astype(np.uint64) + np.uint64(total))
            total += int(o[-1])
        name_offs = np.zeros(len(keys) + 1, np.uint64)
        np.cumsum([len(k) for k in keys], out=name_offs[1:])
        with open(path, "wb") as f:
            np.savez(f, names=np.frombuffer(b"".join(keys), dtype=np.uint8), name_offs=name_offs,
                     offs=np.concatenate(offs), blob=np.concatenate(blobs) if blobs else np.zeros(0, np.uint8))
        return len(keys)

    def restore_hlls(self, path) -> int:
        """``load_hlls`` of every key of a ``save_hlls`` file; the number of keys."""
        with np.load(path) as z:
            names, name_offs, offs, blob = z["names"].tobytes(), z["name_offs"], z["offs"], z["blob"].tobytes()
        n = len(name_offs) - 1
        self.load_hlls((names[int(name_offs[i]):int(name_offs[i + 1])], blob[int(offs[i]):int(offs[i + 1])])
                       for i in range(n))
        return n

    def key_slot(self, name, create: bool = True) -> int:
        """Slot of an HLL key (creating it when asked) for batched calls."""
        k = encode(name)
        if self.keys.expect(k, "hll"):
            return self.keys.slot[k]
        if not create:
            raise ResponseError("ERR no such key")
        return self.keys.new_slot(k)
