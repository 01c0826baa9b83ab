"""The device ingest of ``SketchClient`` (csrc/sketch_api_ingest.cpp, SURVEY.md
§8f row 3): raw message payloads -> BF.EXISTS answers and PFADDs."""
from __future__ import annotations

import ctypes as C
import json
from datetime import datetime
from typing import Sequence

import numpy as np

from ._lib import IngestCols, ptr as _ptr
from .encoding import encode
from .engine import DeviceBuffer
from .keyspace import day_key

_COLS = ("status", "id_start", "id_len", "lec_start", "lec_len", "ts_start", "ts_len", "day", "kh")


class IngestState:
    """What ``ingest_packed`` keeps on the device between calls: its buffers
    with their capacities, and what the device key table was built under."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.n = self.nbytes = 0  # messages / payload bytes the buffers hold
        self.bufs: dict[str, DeviceBuffer] = {}
        self.keytab = None  # (slots released, key form, prefix)

    def reserve(self, n: int, nbytes: int) -> dict:
        if self.n < n or self.nbytes < nbytes:
            for b in self.bufs.values():
                b.free()
            cn, cb = max(n, 1024), max(nbytes, 1 << 16)
            B = {"msgs": DeviceBuffer(self.ctx, cb + 64), "moffs": DeviceBuffer(self.ctx, (cn + 1) * 4),
                 "status": DeviceBuffer(self.ctx, cn), "day": DeviceBuffer(self.ctx, cn * 4),
                 "kh": DeviceBuffer(self.ctx, cn * 16), "slot": DeviceBuffer(self.ctx, cn * 4),
                 "valid": DeviceBuffer(self.ctx, cn)}
            for k in ("id_start", "id_len", "lec_start", "lec_len", "ts_start", "ts_len"):
                B[k] = DeviceBuffer(self.ctx, cn * 4)
            self.n, self.nbytes, self.bufs = cn, cb, B
        return self.bufs


class IngestRun:
    """What one ``_ingest_batch`` leaves for a caller that goes on with the
    batch on the device (``StudentCounts.update_messages``): the device
    buffers and parse columns, whether BF.EXISTS ran (``B["valid"]`` holds the
    answers), and the host-decoded messages -- their indices, encoded ids,
    timestamps and lectures (the text ``keyspace.day_key`` puts into the key
    name, encoded)."""

    def __init__(self, B, cols, n, has_bf, host_at, host_ids, host_ts, host_lectures):
        self.B, self.cols, self.n, self.has_bf = B, cols, n, has_bf
        self.host_at, self.host_ids, self.host_ts = host_at, host_ids, host_ts
        self.host_lectures = host_lectures


def _message(blob: memoryview, moffs: np.ndarray, i) -> bytes:
    return blob[moffs[i]:moffs[i + 1]].tobytes()


def join_messages(messages: Sequence) -> tuple[np.ndarray, np.ndarray]:
    """Message payloads laid end to end: ``(blob, moffs)``, message i is
    ``blob[moffs[i]:moffs[i+1]]``."""
    n = len(messages)
    try:
        joined = b"".join(messages)
        raw = messages
    except TypeError:  # str payloads: as .decode() would see them
        raw = [m if isinstance(m, (bytes, bytearray, memoryview)) else str(m).encode()
               for m in messages]
        joined = b"".join(raw)
    lens = np.fromiter(map(len, raw), np.uint32, count=n)
    moffs = np.zeros(n + 1, np.uint32)
    np.cumsum(lens, out=moffs[1:])
    return np.frombuffer(joined, np.uint8), moffs


class IngestMixin:
    def ingest(self, bf_key, messages: Sequence, hll_key_prefix: str = "hll:unique:",
               key_form: str = "readme") -> tuple[np.ndarray, np.ndarray]:
        """The processor loop of attendance_processor.py:100-137 over raw
        message payloads: decode (json.loads, :103-106), BF.EXISTS of the
        student id (:109-113) and, if valid, PFADD into the lecture key (:128;
        README.md:105-106 form ``<prefix><lecture_id>:<YYYY-MM-DD>`` with the
        UTC day, or ``key_form="code"``: ``<prefix><lecture_id>``).

        Messages are decoded on the device (sketch_ingest.hip); those outside
        its fast JSON / ISO-8601 path go through Python's json / datetime here,
        so every message gets exactly the reference's treatment.  Returns
        ``(valid, status)``: per message the BF.EXISTS answer and 0 decoded on
        the device, 1 decoded on the host, -1 not decodable (the reference's
        negative_acknowledge, :134-136)."""
        blob, moffs = join_messages(messages)
        return self.ingest_packed(bf_key, blob, moffs, hll_key_prefix, key_form)

    def ingest_packed(self, bf_key, blob: np.ndarray, moffs: np.ndarray,
                      hll_key_prefix: str = "hll:unique:", key_form: str = "readme"):
        """``ingest`` over payloads already laid end to end: message i is
        ``blob[moffs[i]:moffs[i+1]]`` (the layout a network consumer fills)."""
        return self._ingest_batch(bf_key, blob, moffs, hll_key_prefix, key_form)[:2]

    def _ingest_batch(self, bf_key, blob, moffs, hll_key_prefix, key_form):
        """``ingest_packed``'s work; returns ``(valid, status, run)`` with
        ``run`` an ``IngestRun`` (None for an empty batch)."""
        blob = np.ascontiguousarray(blob, np.uint8)
        moffs = np.ascontiguousarray(moffs, np.uint32)
        n = len(moffs) - 1
        valid = np.zeros(n, bool)
        status = np.zeros(n, np.int8)
        if n <= 0:
            return valid, status, None
        day_form = 1 if key_form == "readme" else 0
        prefix = str(hll_key_prefix)
        mv = memoryview(blob)

        def key_name(i) -> tuple[dict, bytes, datetime]:
            """Message i decoded as Python does, its HLL key and its time."""
            data = json.loads(_message(mv, moffs, i).decode())
            lecture_id = data["lecture_id"]
            ts = datetime.fromisoformat(data["timestamp"])
            return data, encode(day_key(prefix, lecture_id, None if key_form == "code" else ts)), ts

        if self._ingest is None:
            self._ingest = IngestState(self.ctx)
        B = self._ingest.reserve(n, blob.size)
        cols = self._ingest_parse(B, blob, moffs, n, day_form)
        dev_status, tentative = self._ingest_resolve_keys(B, cols, n, (day_form, prefix), key_name)
        bkey = encode(bf_key)
        has_bf = self.keys.expect(bkey, "bf")
        if has_bf:
            taken = C.c_uint64()
            self.ctx.call("ske_ingest_swipes", self.keys.fid[bkey], C.c_void_p(B["msgs"].ptr),
                          C.byref(cols), n, C.c_void_p(B["valid"].ptr), C.byref(taken))
            valid[:] = B["valid"].to_host(np.uint8, n).astype(bool)
        keys, at, ids, tss, lecs = self._ingest_host_path(bkey, np.nonzero(dev_status != 0)[0], key_name, valid,
                                                          status)
        if tentative:
            self._ingest_release_unused(B, cols, n, tentative, has_bf, valid, dev_status, keys, at)
        return valid, status, IngestRun(B, cols, n, has_bf, at, ids, tss, lecs)

    def _ingest_parse(self, B, blob, moffs, n, day_form) -> IngestCols:
        """Upload the payloads and decode them on the device."""
        if blob.size:
            self.ctx.call("ske_memcpy", C.c_void_p(B["msgs"].ptr), _ptr(blob), blob.size, 0)
        self.ctx.call("ske_memcpy", C.c_void_p(B["moffs"].ptr), _ptr(moffs), moffs.nbytes, 0)
        cols = IngestCols(*[C.c_void_p(B[k].ptr) for k in _COLS])
        self.ctx.call("ske_ingest_parse", C.c_void_p(B["msgs"].ptr), C.c_void_p(B["moffs"].ptr), n,
                      day_form, C.byref(cols))
        return cols

    def _ingest_resolve_keys(self, B, cols, n, form, key_name):
        """Look every decoded message's key up in the device key table; name the
        keys seen for the first time (one Python decode per new key).  Returns
        the device's per-message status and the keys created tentatively."""
        st = self._ingest
        if st.keytab != (self.keys.slots_released, *form):
            self.ctx.call("ske_keytab_clear")  # a freed slot may be reused: start over
            st.keytab = (self.keys.slots_released, *form)
        nmiss = C.c_uint64()
        self.ctx.call("ske_keytab_lookup", C.byref(cols), n, C.c_void_p(B["slot"].ptr), C.byref(nmiss))
        dev_status = B["status"].to_host(np.uint8, n)
        tentative = []
        if nmiss.value:
            slot = B["slot"].to_host(np.uint32, n)
            kh = B["kh"].to_host(np.uint64, 2 * n).reshape(n, 2)
            miss = np.nonzero((dev_status == 0) & (slot == 0xFFFFFFFF))[0]
            uk, first = np.unique(kh[miss], axis=0, return_index=True)
            new_slots = np.zeros(len(uk), np.uint32)
            for j, m in enumerate(miss[first]):
                name = key_name(m)[1]
                self.keys.expect(name, "hll")
                if name not in self.keys.slot:
                    tentative.append(name)
                    new_slots[j] = self.keys.new_slot(name)
                else:
                    new_slots[j] = self.keys.slot[name]
            ukc = np.ascontiguousarray(uk, np.uint64)
            self.ctx.call("ske_keytab_insert", ukc.ctypes.data_as(C.c_void_p), _ptr(new_slots), len(uk))
        return dev_status, tentative

    def _ingest_host_path(self, bkey, host, key_name, valid, status):
        """The messages the device did not decode: Python's json / datetime
        semantics, then ``swipes``.  Fills their ``valid`` / ``status``; returns
        their keys, message indices, encoded ids, times and lectures."""
        ids, keys, at, tss, lecs = [], [], [], [], []
        for m in host:
            try:
                data, name, ts = key_name(m)
                sid = encode(data["student_id"])
            except Exception:
                status[m] = -1
                continue
            status[m] = 1
            ids.append(sid)
            keys.append(name)
            at.append(m)
            tss.append(ts)
            lecs.append(str(data["lecture_id"]).encode())
        if at:
            valid[np.asarray(at)] = self.swipes(bkey, keys, ids)
        return keys, at, ids, tss, lecs

    def _ingest_release_unused(self, B, cols, n, tentative, has_bf, valid, dev_status, keys, at):
        """Keys created for this batch that no valid swipe reached are not
        created (as in the per-event loop)."""
        hit = set()
        if has_bf:
            self.ctx.call("ske_keytab_lookup", C.byref(cols), n, C.c_void_p(B["slot"].ptr), None)
            slot = B["slot"].to_host(np.uint32, n)
            hit = set(np.unique(slot[valid & (dev_status == 0)]).tolist())
            hit |= {self.keys.slot[k] for k, m in zip(keys, at) if valid[m] and k in self.keys.slot}
        for name in tentative:
            if name in self.keys.slot and self.keys.slot[name] not in hit:
                self.keys.release_unused_slot(name)
