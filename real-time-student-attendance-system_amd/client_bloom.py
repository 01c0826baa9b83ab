"""The Bloom half of ``SketchClient`` (csrc/sketch_api_bloom.cpp): BF.* over
RedisBloom's scalable chains, with BF.SCANDUMP / BF.LOADCHUNK."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import formats
from ._lib import BfInfo, BfLink, SketchLibError, SKE_MEM_HOST, ptr as _ptr
from .commands import token
from .encoding import encode, pack
from .exceptions import ResponseError, WRONGTYPE

_DEFAULT_ERROR = 0.01       # rebloom.c BFDefaultErrorRate
_DEFAULT_CAPACITY = 100     # rebloom.c BFDefaultInitCapacity
_DEFAULT_EXPANSION = 2      # rebloom.c BFDefaultExpansion


class BloomMixin:
    def _bf_reserve(self, key: bytes, error_rate, capacity, expansion=None, nonscaling=False):
        try:
            err = float(error_rate)
        except (TypeError, ValueError):
            raise ResponseError("ERR bad error rate")
        try:
            cap = int(capacity)
        except (TypeError, ValueError):
            raise ResponseError("ERR bad capacity")
        if not (0 < err < 1):
            raise ResponseError("ERR (0 < error rate range < 1)")
        if cap <= 0:
            raise ResponseError("ERR (capacity should be larger than 0)")
        exp = _DEFAULT_EXPANSION if expansion is None else int(expansion)
        if exp < 1 and not nonscaling:
            raise ResponseError("ERR expansion should be greater or equal to 1")
        if key in self.keys.kind:
            if self.keys.kind[key] != "bf":
                raise ResponseError(WRONGTYPE)
            raise ResponseError("ERR item exists")
        f = self.keys.new_fid(key)
        try:
            self.ctx.call("ske_bf_reserve", f, err, cap, exp, 1 if nonscaling else 0)
        except SketchLibError as e:
            self.keys.undo_new(key)
            raise ResponseError(str(e))
        return self._ok()

    def _bf_fid(self, key) -> int:
        """The filter of an existing Bloom key (``ERR not found`` otherwise)."""
        key = encode(key)
        if not self.keys.expect(key, "bf"):
            raise ResponseError("ERR not found")
        return self.keys.fid[key]

    def _bf_fid_for_add(self, key: bytes) -> int:
        if self.keys.expect(key, "bf"):
            return self.keys.fid[key]
        f = self.keys.new_fid(key)
        # rebloom.c: BF.ADD / BF.MADD on a missing key create a default chain
        self.ctx.call("ske_bf_reserve", f, _DEFAULT_ERROR, _DEFAULT_CAPACITY, _DEFAULT_EXPANSION, 0)
        return f

    def bf_madd_packed(self, key, buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
        """BF.MADD over a packed batch; returns int8 replies (1 / 0 / -2 full)."""
        key = encode(key)
        f = self._bf_fid_for_add(key)
        n = len(offs) - 1
        out = np.zeros(n, np.int8)
        if n:
            self.ctx.call("ske_bf_madd", f, _ptr(buf), _ptr(offs), n, _ptr(out), SKE_MEM_HOST)
        return out

    def bf_mexists_packed(self, key, buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
        """BF.MEXISTS over a packed batch; missing key -> zeros."""
        key = encode(key)
        n = len(offs) - 1
        out = np.zeros(n, np.uint8)
        if not self.keys.expect(key, "bf") or n == 0:
            return out
        self.ctx.call("ske_bf_mexists", self.keys.fid[key], _ptr(buf), _ptr(offs), n, _ptr(out),
                      SKE_MEM_HOST)
        return out

    def _bf_madd_reply(self, key: bytes, items: Sequence) -> list:
        buf, offs = pack(items)
        res = self.bf_madd_packed(key, buf, offs)
        return [ResponseError("ERR non scaling filter is full") if r == -2 else int(r) for r in res]

    def bf_info(self, key) -> dict:
        info = BfInfo()
        self.ctx.call("ske_bf_info", self._bf_fid(key), C.byref(info))
        return {"Capacity": info.capacity, "Size": info.size_bytes,
                "Number of filters": info.nfilters, "Number of items inserted": info.inserted,
                "Expansion rate": None if info.nonscaling else info.expansion}

    def bf_links(self, key) -> list[dict]:
        """BF.DEBUG-like view: one dict per link (bloom_init geometry)."""
        f = self._bf_fid(key)
        info = BfInfo()
        self.ctx.call("ske_bf_info", f, C.byref(info))
        out = []
        for i in range(info.nfilters):
            L = BfLink()
            self.ctx.call("ske_bf_link_info", f, i, C.byref(L))
            out.append(dict(entries=L.entries, bytes=L.bytes, bits=L.bits, size=L.size,
                            error=L.error, bpe=L.bpe, hashes=L.hashes))
        return out

    def bf_link_bits(self, key, link: int) -> np.ndarray:
        """Raw bit array of one link (BF.SCANDUMP data chunk layout)."""
        f = self._bf_fid(key)
        links = self.bf_links(key)
        out = np.zeros(links[link]["bytes"], np.uint8)
        self.ctx.call("ske_bf_export_link", f, link, _ptr(out), out.size)
        return out

    # ---- BF.SCANDUMP / BF.LOADCHUNK (RedisBloom rebloom.c BFScanDump /
    # BFLoadChunk, src/sb.c SBChain_GetEncodedHeader / GetEncodedChunk /
    # LoadEncodedChunk; [recall], unconfirmed on a Redis box).  Iterator 0
    # returns the header chunk with iterator 1; iterator i > 0 returns the bytes
    # at offset i - 1 of the links' bit arrays laid end to end, at most one link
    # and MAX_SCANDUMP_SIZE bytes per chunk, with the next iterator i + len;
    # past the end it returns (0, empty).  LOADCHUNK takes the iterator that
    # SCANDUMP returned with the chunk (offset = iter - 1 - len).
    MAX_SCANDUMP_SIZE = 10 * 1024 * 1024

    def bf_scandump(self, key, it: int) -> tuple[int, bytes]:
        f = self._bf_fid(key)
        it = int(it)
        links = self.bf_links(key)
        if it == 0:
            info = BfInfo()
            self.ctx.call("ske_bf_info", f, C.byref(info))
            hdr = formats.bf_dump_header(info.inserted, links, info.expansion, bool(info.nonscaling))
            return 1, hdr
        off = it - 1
        for i, L in enumerate(links):
            if off < L["bytes"]:
                n = min(L["bytes"] - off, self.MAX_SCANDUMP_SIZE)
                bits = self.bf_link_bits(key, i)
                return it + n, bits[off:off + n].tobytes()
            off -= L["bytes"]
        return 0, b""

    def bf_loadchunk(self, key, it: int, data: bytes) -> bool:
        key = encode(key)
        it, data = int(it), bytes(encode(data))
        if it == 1:
            try:
                h = formats.bf_parse_header(data)
            except Exception:
                raise ResponseError("ERR received bad data")
            if self.keys.type_of(key) is not None:
                raise ResponseError("ERR item exists")
            if h["options"] & formats.BLOOM_OPT_FORCE64 == 0 or not h["links"]:
                raise ResponseError("ERR received bad data")
            # bloom_check_add64 probes mod 2^n2 when n2 != 0; the device always
            # probes mod bits, so only a link whose bits are that power of two loads
            if any(L["n2"] and (L["n2"] > 63 or L["bits"] != 1 << L["n2"]) for L in h["links"]):
                raise ResponseError("ERR received bad data")
            arr = (BfLink * len(h["links"]))()
            for i, L in enumerate(h["links"]):
                arr[i].entries, arr[i].bytes, arr[i].bits = L["entries"], L["bytes"], L["bits"]
                arr[i].size, arr[i].error, arr[i].bpe, arr[i].hashes = (
                    L["size"], L["error"], L["bpe"], L["hashes"])
            fid = self.keys.new_fid(key)
            try:
                self.ctx.call("ske_bf_load_header", fid, arr, len(h["links"]), h["size"],
                              h["growth"], 1 if h["nonscaling"] else 0)
            except SketchLibError as e:
                self.keys.drop(key)
                raise ResponseError("ERR received bad data") from e
            return True
        f = self._bf_fid(key)
        off = it - 1 - len(data)
        if off < 0:
            raise ResponseError("ERR invalid offset - no link found")
        for i, L in enumerate(self.bf_links(key)):
            if off < L["bytes"]:
                if off + len(data) > L["bytes"]:
                    raise ResponseError("ERR invalid chunk - Too big for current filter")
                buf = np.frombuffer(data, np.uint8)
                self.ctx.call("ske_bf_link_write", f, i, off, _ptr(buf), buf.size)
                return True
            off -= L["bytes"]
        raise ResponseError("ERR invalid offset - no link found")

    # ---- command handlers (commands.COMMANDS)
    def _cmd_bf_reserve(self, a):
        exp, nonscaling = None, False
        rest = list(a[3:])
        while rest:
            opt = token(rest.pop(0))
            if opt == "EXPANSION" and rest:
                exp = rest.pop(0)
            elif opt == "NONSCALING":
                nonscaling = True
            else:
                raise ResponseError("ERR syntax error")
        return self._bf_reserve(encode(a[0]), a[1], a[2], exp, nonscaling)

    def _cmd_bf_add(self, a):
        r = self._bf_madd_reply(encode(a[0]), [a[1]])[0]
        if isinstance(r, ResponseError):
            raise r
        return r

    def _cmd_bf_mexists(self, a):
        buf, offs = pack(a[1:])
        return [int(x) for x in self.bf_mexists_packed(a[0], buf, offs)]

    def _cmd_bf_card(self, a):
        k = encode(a[0])
        return self.bf_info(k)["Number of items inserted"] if self.keys.expect(k, "bf") else 0
