"""The facade's key table: key name -> device object, the kinds a key can have
and their TYPE replies, Redis' MATCH glob, and the README's day-key form."""
from __future__ import annotations

from datetime import datetime, timezone

from . import _lib
from ._lib import Context
from .exceptions import ResponseError, WRONGTYPE

BF_TYPE_NAME = "MBbloom--"  # RedisBloom's module type name (TYPE reply)
CMS_TYPE_NAME = "CMSk-TYPE"  # RedisBloom's Count-Min Sketch type name (TYPE reply)
# kind of a key in the table -> its TYPE reply (an HLL key is a Redis string)
KIND_TYPE_NAMES = {"hll": "string", "bf": BF_TYPE_NAME, "cms": CMS_TYPE_NAME}
TYPE_NAME_KINDS = {name: kind for kind, name in KIND_TYPE_NAMES.items()}


def day_key(prefix: str, lecture_id, timestamp: datetime | None = None) -> str:
    """An HLL key of a lecture: ``<prefix><lecture_id>:<YYYY-MM-DD>`` with the
    timestamp's UTC day (README.md:105-106), or without a timestamp the code's
    form ``<prefix><lecture_id>`` (attendance_processor.py:128)."""
    if timestamp is None:
        return f"{prefix}{lecture_id}"
    if timestamp.tzinfo is not None:
        timestamp = timestamp.astimezone(timezone.utc)
    return f"{prefix}{lecture_id}:{timestamp.date().isoformat()}"


class KeySpace:
    """Key name -> device object (Bloom fid, HLL register-slab slot or
    Count-Min Sketch cid)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self.kind: dict[bytes, str] = {}
        self.fid: dict[bytes, int] = {}
        self.slot: dict[bytes, int] = {}
        self.cid: dict[bytes, int] = {}
        self._free_fids = list(range(_lib.SKE_MAX_FILTERS - 1, -1, -1))
        self._free_cids = list(range(_lib.SKE_MAX_CMS - 1, -1, -1))
        self._free_slots: list[int] = []
        self._next_slot = 0
        self._slot_key: dict[int, bytes] = {}
        self.slots_released = 0  # bumps whenever an HLL slot is freed (ingest key table)
        # README day keys <stem>:YYYY-MM-DD by stem (the key minus its day),
        # kept with the table: a lecture's day keys without a scan
        self.day_keys: dict[bytes, set] = {}

    @staticmethod
    def _day_stem(key: bytes):
        """The stem of a README-form day key <stem>:YYYY-MM-DD, else None."""
        if len(key) > 11 and key[-11] == 0x3A and key[-3] == key[-6] == 0x2D and \
                key[-10:-6].isdigit() and key[-5:-3].isdigit() and key[-2:].isdigit():
            return key[:-11]
        return None

    def _index(self, key: bytes, add: bool) -> None:
        stem = self._day_stem(key)
        if stem is None:
            return
        if add:
            self.day_keys.setdefault(stem, set()).add(key)
        else:
            ks = self.day_keys.get(stem)
            if ks is not None:
                ks.discard(key)
                if not ks:
                    del self.day_keys[stem]

    def type_of(self, key: bytes) -> str | None:
        return self.kind.get(key)

    def expect(self, key: bytes, kind: str) -> bool:
        """True if the key exists with this kind, False if missing; raises
        WRONGTYPE if it holds another kind."""
        k = self.kind.get(key)
        if k is None:
            return False
        if k != kind:
            raise ResponseError(WRONGTYPE)
        return True

    def new_fid(self, key: bytes) -> int:
        if not self._free_fids:
            raise ResponseError("ERR too many Bloom filters on this device")
        f = self._free_fids.pop()
        self.kind[key] = "bf"
        self.fid[key] = f
        return f

    def new_cid(self, key: bytes) -> int:
        if not self._free_cids:
            raise ResponseError("ERR too many Count-Min Sketch keys on this device")
        t = self._free_cids.pop()
        self.kind[key] = "cms"
        self.cid[key] = t
        return t

    def new_slot(self, key: bytes) -> int:
        if self._free_slots:
            s = self._free_slots.pop()
        else:
            s = self._next_slot
            self._next_slot += 1
            if s >= self.ctx.lib.ske_hll_capacity(self.ctx.ptr):
                self.ctx.call("ske_hll_reserve", s + 1)
        self.kind[key] = "hll"
        self.slot[key] = s
        self._slot_key[s] = key
        self._index(key, True)
        return s

    def bind(self, key: bytes, slot: int) -> None:
        """Name an HLL key at a given slab slot without touching its registers:
        a multi-GPU job's key map (distributed.KeyMap.bind) fixes the local
        slot of every key its rank owns, and K1 writes those slots directly."""
        slot = int(slot)
        if self.kind.get(key, "hll") != "hll":
            raise ResponseError(WRONGTYPE)
        have = self.slot.get(key)
        if have is not None:
            if have != slot:
                raise ResponseError(f"ERR key already bound to slot {have}")
            return
        if slot in self._slot_key:
            raise ResponseError(f"ERR slot {slot} already holds another key")
        if slot >= self.ctx.lib.ske_hll_capacity(self.ctx.ptr):
            self.ctx.call("ske_hll_reserve", slot + 1)
        if slot >= self._next_slot:
            self._free_slots.extend(range(slot - 1, self._next_slot - 1, -1))
            self._next_slot = slot + 1
        else:
            self._free_slots.remove(slot)
        self.kind[key] = "hll"
        self.slot[key] = slot
        self._slot_key[slot] = key
        self._index(key, True)

    def drop(self, key: bytes) -> bool:
        k = self.kind.pop(key, None)
        if k == "bf":
            f = self.fid.pop(key)
            self.ctx.call("ske_bf_free", f)
            self._free_fids.append(f)
        elif k == "cms":
            t = self.cid.pop(key)
            self.ctx.call("ske_cms_free", t)
            self._free_cids.append(t)
        elif k == "hll":
            s = self.slot.pop(key)
            self._slot_key.pop(s, None)
            self._index(key, False)
            self.ctx.call("ske_hll_clear", s)  # a reused slot starts empty
            self._free_slots.append(s)
            self.slots_released += 1
        return k is not None

    def undo_new(self, key: bytes) -> None:
        """Undo the new_fid / new_cid / new_slot that named this key, for a key
        that no command ended up creating: nothing was written on the device
        for it, so there is no device call."""
        k = self.kind.pop(key)
        if k == "bf":
            self._free_fids.append(self.fid.pop(key))
        elif k == "cms":
            self._free_cids.append(self.cid.pop(key))
        else:
            s = self.slot.pop(key)
            self._slot_key.pop(s, None)
            self._index(key, False)
            self._free_slots.append(s)
            self.slots_released += 1

    release_unused_slot = undo_new  # the name the HLL paths use


def _sc(b: int) -> int:
    """a byte as C's (signed) char, as Redis compares range bounds"""
    return b - 256 if b >= 128 else b


def redis_glob(pattern: bytes, string: bytes, _nest: int = 0) -> bool:
    """Redis' SCAN / KEYS MATCH rule, restated from redis ``src/util.c``
    ``stringmatchlen`` (case-sensitive; no Redis in this image, so parity is
    unpinned -- tests/test_encoding.py holds the cases): ``*`` any run, ``?``
    one byte, ``[...]`` a class with ``^`` negation, ``a-z`` ranges (bounds
    swapped when reversed) and ``\\`` escapes, ``\\`` escaping the next
    pattern byte outside a class.  Python's fnmatch differs (``[!...]``, no
    escapes)."""
    p, s = pattern, string
    pi, si = 0, 0
    if _nest > 1000:
        return False
    while pi < len(p) and si < len(s):
        c = p[pi]
        if c == 0x2A:  # '*'
            while pi + 1 < len(p) and p[pi + 1] == 0x2A:
                pi += 1
            if pi + 1 == len(p):
                return True
            while si < len(s):
                if redis_glob(p[pi + 1:], s[si:], _nest + 1):
                    return True
                si += 1
            return False
        elif c == 0x3F:  # '?'
            si += 1
        elif c == 0x5B:  # '['
            pi += 1
            neg = pi < len(p) and p[pi] == 0x5E  # '^'
            if neg:
                pi += 1
            match = False
            while True:
                if pi < len(p) and p[pi] == 0x5C and len(p) - pi >= 2:  # '\\'
                    pi += 1
                    if p[pi] == s[si]:
                        match = True
                elif pi < len(p) and p[pi] == 0x5D:  # ']'
                    break
                elif pi >= len(p):
                    pi -= 1
                    break
                elif len(p) - pi >= 3 and p[pi + 1] == 0x2D:  # 'a-z'
                    lo, hi, ch = _sc(p[pi]), _sc(p[pi + 2]), _sc(s[si])
                    if lo > hi:
                        lo, hi = hi, lo
                    pi += 2
                    if lo <= ch <= hi:
                        match = True
                elif p[pi] == s[si]:
                    match = True
                pi += 1
            if neg:
                match = not match
            if not match:
                return False
            si += 1
        else:
            if c == 0x5C and len(p) - pi >= 2:  # an escaped byte
                pi += 1
            if p[pi] != s[si]:
                return False
            si += 1
        pi += 1
        if si == len(s):
            while pi < len(p) and p[pi] == 0x2A:
                pi += 1
            break
    return pi == len(p) and si == len(s)
