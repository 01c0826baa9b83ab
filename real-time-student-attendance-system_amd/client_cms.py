"""The Count-Min Sketch half of ``SketchClient`` (csrc/sketch_api_cms.cpp).

RedisBloom src/rm_cms.c / src/cms.c, restated from memory (parity with a live
RedisBloom is unpinned, DESIGN.md "Count-Min Sketch").  The error texts come
from ske_strerror."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import CmsInfo, SketchLibError, SKE_MEM_HOST, ptr as _ptr
from .commands import arity_error, token
from .encoding import encode, pack
from .exceptions import ResponseError


class CmsMixin:
    @staticmethod
    def _cms_err(code: int) -> ResponseError:
        return ResponseError(_lib.strerror(code))

    @staticmethod
    def _cms_int(v, code: int) -> int:
        """A command argument as RedisModule_StringToLongLong reads it."""
        try:
            if isinstance(v, (bytes, bytearray, memoryview)):
                v = bytes(v).decode()
            if isinstance(v, float) and v != int(v):
                raise ValueError
            return int(v)
        except (TypeError, ValueError, UnicodeDecodeError):
            raise ResponseError(_lib.strerror(code))

    def cms_cid(self, key) -> int:
        """The table of an existing Count-Min Sketch key."""
        key = encode(key)
        if not self.keys.expect(key, "cms"):
            raise self._cms_err(_lib.SKE_ECMSNOKEY)
        return self.keys.cid[key]

    def cms_initbydim(self, key, width, depth):
        key = encode(key)
        w = self._cms_int(width, _lib.SKE_ECMSWIDTH)
        if not 1 <= w <= 0xFFFFFFFF:
            raise self._cms_err(_lib.SKE_ECMSWIDTH)
        d = self._cms_int(depth, _lib.SKE_ECMSDEPTH)
        if not 1 <= d <= 0xFFFFFFFF:
            raise self._cms_err(_lib.SKE_ECMSDEPTH)
        if key in self.keys.kind:  # CMS.INITBY* refuse a key of any type
            raise self._cms_err(_lib.SKE_ECMSEXISTS)
        t = self.keys.new_cid(key)
        try:
            self.ctx.call("ske_cms_init", t, w, d)
        except SketchLibError as e:
            self.keys.undo_new(key)
            raise ResponseError(str(e))
        return self._ok()

    def cms_initbyprob(self, key, error, probability):
        try:
            err = float(error)
        except (TypeError, ValueError):
            raise self._cms_err(_lib.SKE_ECMSERROR)
        try:
            prob = float(probability)
        except (TypeError, ValueError):
            raise self._cms_err(_lib.SKE_ECMSPROB)
        w, d = C.c_uint32(), C.c_uint32()
        rc = _lib.load().ske_cms_dims_from_prob(err, prob, C.byref(w), C.byref(d))
        if rc:
            raise self._cms_err(rc)
        return self.cms_initbydim(key, w.value, d.value)

    def cms_add_packed(self, key, buf: np.ndarray, offs: np.ndarray, incr=None, mask=None,
                       want: int = 1) -> None:
        """The bulk, order-free CMS.INCRBY over a packed batch (no replies):
        item i counts ``incr[i]`` (1 when ``incr`` is None); with ``mask`` only
        the items with ``mask[i] == want``."""
        t = self.cms_cid(key)
        n = len(offs) - 1
        if n <= 0:
            return
        inc = None if incr is None else np.ascontiguousarray(incr, dtype=np.uint32)
        if inc is not None and inc.shape != (n,):
            raise ValueError("one increment per item")
        if mask is not None:
            m = np.asarray(mask)
            if m.shape != (n,):
                raise ValueError("one mask byte per item")
            if want not in (0, 1):
                raise ValueError("want is 0 or 1")
            inc = np.where(m == want, np.uint32(1) if inc is None else inc, np.uint32(0)).astype(np.uint32)
        self.ctx.call("ske_cms_incrby", t, _ptr(np.ascontiguousarray(buf, np.uint8)),
                      _ptr(np.ascontiguousarray(offs, np.uint32)), n, _ptr(inc), None, SKE_MEM_HOST)

    def cms_incrby(self, key, items: Sequence, increments: Sequence) -> list[int]:
        """CMS.INCRBY's reply list: per item the minimum of its cells right
        after its own update, items taken in order."""
        key = encode(key)
        if len(items) != len(increments) or not items:
            raise arity_error("cms.incrby")
        t = self.cms_cid(key)
        inc = []
        for v in increments:
            x = self._cms_int(v, _lib.SKE_ECMSPARSE)
            if x < 0:
                raise self._cms_err(_lib.SKE_ECMSNEG)
            if x > 0xFFFFFFFF:  # a counter is 32 bits wide (deviation)
                raise self._cms_err(_lib.SKE_ECMSPARSE)
            inc.append(x)
        buf, offs = pack(items)
        inc = np.asarray(inc, dtype=np.uint32)
        out = np.zeros(len(items), np.uint32)
        self.ctx.call("ske_cms_incrby", t, _ptr(buf), _ptr(offs), len(items), _ptr(inc), _ptr(out),
                      SKE_MEM_HOST)
        return [int(x) for x in out]

    def cms_query_packed(self, key, buf: np.ndarray, offs: np.ndarray) -> np.ndarray:
        t = self.cms_cid(key)
        n = len(offs) - 1
        out = np.zeros(max(n, 0), np.uint32)
        if n > 0:
            self.ctx.call("ske_cms_query", t, _ptr(np.ascontiguousarray(buf, np.uint8)),
                          _ptr(np.ascontiguousarray(offs, np.uint32)), n, _ptr(out), SKE_MEM_HOST)
        return out

    def cms_query(self, key, *items) -> list[int]:
        buf, offs = pack(items)
        return [int(x) for x in self.cms_query_packed(key, buf, offs)]

    def cms_merge(self, dest, num_keys, src_keys: Sequence, weights: Sequence = ()):
        d = self.cms_cid(dest)
        nk = self._cms_int(num_keys, _lib.SKE_ECMSPARSE)
        if nk < 1 or nk != len(src_keys) or (len(weights) and len(weights) != nk):
            raise arity_error("cms.merge")
        if nk > _lib.SKE_CMS_MAX_MERGE:
            raise ResponseError(f"ERR at most {_lib.SKE_CMS_MAX_MERGE} source keys")
        srcs = np.asarray([self.cms_cid(k) for k in src_keys], dtype=np.uint32)
        w = None
        if len(weights):
            ws = [self._cms_int(x, _lib.SKE_ECMSPARSE) for x in weights]
            if any(not -2 ** 63 <= x < 2 ** 63 for x in ws):
                raise self._cms_err(_lib.SKE_ECMSPARSE)
            w = np.asarray(ws, dtype=np.int64)
        try:
            self.ctx.call("ske_cms_merge", d, _ptr(srcs), _ptr(w), nk)
        except SketchLibError as e:
            raise ResponseError(str(e))
        return self._ok()

    def cms_info(self, key) -> dict:
        t = self.cms_cid(key)
        info = CmsInfo()
        self.ctx.call("ske_cms_info", t, C.byref(info))
        return {"width": info.width, "depth": info.depth, "count": info.count}

    def cms_table(self, key) -> tuple[np.ndarray, int]:
        """The whole table, [depth, width] u32, and its count."""
        t = self.cms_cid(key)
        i = self.cms_info(key)
        out = np.zeros((i["depth"], i["width"]), np.uint32)
        self.ctx.call("ske_cms_export", t, _ptr(out), out.size)
        return out, i["count"]

    def cms_table_dev(self, key) -> tuple[int, int]:
        """``(address, ncells)`` of the table on the device (row-major u32
        cells; ``(ncells + 3) & ~3`` of them are readable): the source of an
        all-gather across contexts.  The count is ``cms_info``'s."""
        p, n = C.c_void_p(), C.c_uint64()
        self.ctx.call("ske_cms_table_dev", self.cms_cid(key), C.byref(p), C.byref(n))
        return int(p.value), int(n.value)

    def cms_sum_dev(self, dest, tables, stride_cells: int, counts) -> None:
        """``dest`` = the saturating sum of ``len(counts)`` tables on the device
        (a torch tensor, a DeviceBuffer or an address, 16-byte aligned; table k
        ``stride_cells`` cells behind table k - 1) and of their counts.
        Enqueue only: the tables stay as they are until the context's stream
        has run (``ske_sync``)."""
        cnt = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        try:
            self.ctx.call("ske_cms_sum_dev", self.cms_cid(dest), _lib.devptr(tables), int(stride_cells),
                          int(cnt.size), _ptr(cnt))
        except SketchLibError as e:
            raise ResponseError(str(e))

    # ---- command handlers (commands.COMMANDS)
    def _cmd_cms_incrby(self, a):
        if len(a) % 2 == 0:
            raise arity_error("cms.incrby")
        return self.cms_incrby(a[0], a[1::2], a[2::2])

    def _cmd_cms_merge(self, a):
        nk = self._cms_int(a[1], _lib.SKE_ECMSPARSE)
        rest = list(a[2:])
        if nk < 1 or len(rest) < nk:
            raise arity_error("cms.merge")
        srcs, rest = rest[:nk], rest[nk:]
        weights = []
        if rest:
            if token(rest[0]) != "WEIGHTS" or len(rest) != nk + 1:
                raise arity_error("cms.merge")
            weights = rest[1:]
        return self.cms_merge(a[0], nk, srcs, weights)
