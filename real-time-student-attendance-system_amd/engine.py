"""Device-resident batches and the device-side driver used by the benchmark,
the GPU parity tests and the sharded runner.

Inputs of the hot path are kept resident in HBM (``DeviceBatch``: packed id
bytes + u32 offsets + u32 key slots), generated on the GPU by the
counter-based generator, so a timed step is one K1 launch over a batch that
is already on the device.
"""
from __future__ import annotations

import ctypes as C
import gc

import numpy as np

from ._lib import (CmsInfo, Context, GenParams, HhInfo, HhStats, IngestDense, SKE_HH_ID_BYTES, SKE_HLL_DUMP_CARD,
                   SKE_MEM_DEVICE, SKE_MEM_HOST, SKE_TALLY_KEY_BYTES, SKE_TP_BINS, RowsCompact, RowsGroupStats,
                   RowsInfo, SeenInfo, SKE_EROWSSPACE, SketchLibError, TallyInfo)
from . import synthetic

PASS_KINDS = 9  # SKE_PASS_KINDS (include/sketch.h)


class _no_gc:
    """Collect cyclic garbage now, then keep the collector off until exit
    (around a stream capture: see SketchEngine.capture)."""

    def __enter__(self):
        gc.collect()
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        if self.was:
            gc.enable()
        return False


class DeviceBuffer:
    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        p = C.c_void_p()
        ctx.call("ske_device_alloc", int(max(nbytes, 16)), C.byref(p))
        self.ptr = p.value
        self.nbytes = int(nbytes)

    def free(self):
        if self.ptr:
            self.ctx.call("ske_device_free", C.c_void_p(self.ptr))
            self.ptr = None

    def to_host(self, dtype, count) -> np.ndarray:
        out = np.zeros(count, dtype)
        if out.nbytes:
            self.ctx.call("ske_memcpy", out.ctypes.data_as(C.c_void_p), C.c_void_p(self.ptr),
                          out.nbytes, 1)
        return out

    def from_host(self, arr: np.ndarray):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        if a.nbytes:
            self.ctx.call("ske_memcpy", C.c_void_p(self.ptr), a.ctypes.data_as(C.c_void_p),
                          a.nbytes, 0)


def hh_info(ctx: Context, hid: int) -> dict:
    """ske_hh_info: capacity, used and the sticky overflow word."""
    info = HhInfo()
    ctx.call("ske_hh_info", int(hid), C.byref(info))
    return {"capacity": int(info.capacity), "used": int(info.used), "overflow": int(info.overflow)}


def hh_list(ctx: Context, hid: int, cid: int, threshold: int, room: int | None = None):
    """ske_hh_list: ``(ids, estimates, complete)`` -- the members of set
    ``hid`` whose current estimate in table ``cid`` is at least ``threshold``,
    as bytes, sorted by estimate descending, then id bytes ascending, their
    estimates (u32), and whether the set ever refused an insert.  ``room``:
    entries the output holds (default: the set's ``used``, always enough)."""
    if room is None:
        room = hh_info(ctx, hid)["used"]
    room = max(int(room), 1)
    ids = np.zeros((room, SKE_HH_ID_BYTES), np.uint8)
    lens = np.zeros(room, np.uint32)
    est = np.zeros(room, np.uint32)
    n, complete = C.c_uint64(0), C.c_int(1)
    ctx.call("ske_hh_list", int(hid), int(cid), int(threshold), ids.ctypes.data_as(C.c_void_p),
             lens.ctypes.data_as(C.c_void_p), est.ctypes.data_as(C.c_void_p), room, C.byref(n), C.byref(complete))
    k = int(n.value)
    return [ids[i, :lens[i]].tobytes() for i in range(k)], est[:k].copy(), bool(complete.value)


def hh_stats(ctx: Context, hid: int, cid: int, threshold: int = 0) -> dict:
    """ske_hh_stats: the fields of ske_hh_stats_t as Python ints (``reserved``
    left out) -- over the members of set ``hid`` whose current estimate in table
    ``cid`` is at least ``threshold``."""
    s = HhStats()
    ctx.call("ske_hh_stats", int(hid), int(cid), int(threshold), C.byref(s))
    return {k: int(getattr(s, k)) for k in ("n", "sum", "sq_lo", "sq_hi", "min", "max", "med_lo", "med_hi",
                                            "complete")}


def hh_select(ctx: Context, hid: int, cid: int, threshold: int, ranks) -> np.ndarray:
    """ske_hh_select: the ``ranks[j]``-th smallest passing estimates (0-based),
    at most SKE_HH_MAX_RANKS ranks a call; a rank at or above the number that
    pass raises (SKE_EINVAL)."""
    r = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
    out = np.zeros(r.size, np.uint32)
    n = C.c_uint64(0)
    ctx.call("ske_hh_select", int(hid), int(cid), int(threshold), r.ctypes.data_as(C.c_void_p), int(r.size),
             out.ctypes.data_as(C.c_void_p), C.byref(n))
    return out


def tp_counts(ctx: Context, tid: int) -> np.ndarray:
    """ske_tp_read: the profile's counters as [7, 24] uint64 (weekday, Monday
    first, by hour)."""
    out = np.zeros(SKE_TP_BINS, np.uint64)
    ctx.call("ske_tp_read", int(tid), out.ctypes.data_as(C.c_void_p))
    return out.reshape(7, 24)


def tp_import(ctx: Context, tid: int, counts) -> None:
    """ske_tp_import: overwrite the profile's counters (168 values, any shape)."""
    a = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    if a.size != SKE_TP_BINS:
        raise ValueError(f"a time profile has {SKE_TP_BINS} counters")
    ctx.call("ske_tp_import", int(tid), a.ctypes.data_as(C.c_void_p))


def tally_info(ctx: Context, tid: int) -> dict:
    """ske_tally_info: capacity, used, the sticky overflow word, the items
    looked at and the counts of those that were not grouped."""
    info = TallyInfo()
    ctx.call("ske_tally_info", int(tid), C.byref(info))
    return {k: int(getattr(info, k)) for k in ("capacity", "used", "overflow", "taken", "dropped_events",
                                               "dropped_valid")}


def _tally_rows(keys, lens, events, valid, k):
    return ([keys[i, :lens[i]].tobytes() for i in range(k)], events[:k].copy(), valid[:k].copy())


def tally_list(ctx: Context, tid: int, min_events: int = 0, room: int | None = None):
    """ske_tally_list: ``(keys, events, valid, complete)`` -- the entries of
    tally ``tid`` with at least ``min_events`` events, the keys as bytes, sorted
    by events descending, then key bytes ascending; their counters (u64), and
    whether every count is exact.  ``room``: entries the output holds (default:
    the tally's ``used``, always enough)."""
    if room is None:
        room = tally_info(ctx, tid)["used"]
    room = max(int(room), 1)
    keys = np.zeros((room, SKE_TALLY_KEY_BYTES), np.uint8)
    lens = np.zeros(room, np.uint32)
    events, valid = np.zeros(room, np.uint64), np.zeros(room, np.uint64)
    n, complete = C.c_uint64(0), C.c_int(1)
    ctx.call("ske_tally_list", int(tid), int(min_events), keys.ctypes.data_as(C.c_void_p),
             lens.ctypes.data_as(C.c_void_p), events.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p),
             room, C.byref(n), C.byref(complete))
    return _tally_rows(keys, lens, events, valid, int(n.value)) + (bool(complete.value),)


def tally_top(ctx: Context, tid: int, k: int = 3, by: int = 0):
    """ske_tally_top: ``(head, tail, complete)`` -- the first and the last
    ``k`` entries of the listing's order (``by`` 0: by events, 1: by valid), each
    end as ``(keys, events, valid)``; the tail in list order."""
    k = int(k)
    ends = []
    for _ in range(2):
        ends.append((np.zeros((max(k, 1), SKE_TALLY_KEY_BYTES), np.uint8), np.zeros(max(k, 1), np.uint32),
                     np.zeros(max(k, 1), np.uint64), np.zeros(max(k, 1), np.uint64)))
    n, complete = C.c_uint64(0), C.c_int(1)
    ctx.call("ske_tally_top", int(tid), k, int(by), *[a.ctypes.data_as(C.c_void_p) for e in ends for a in e],
             C.byref(n), C.byref(complete))
    m = int(n.value)
    return _tally_rows(*ends[0], m), _tally_rows(*ends[1], m), bool(complete.value)


def tally_query(ctx: Context, tid: int, buf: np.ndarray, offs: np.ndarray):
    """ske_tally_query over a packed host batch: ``(events, valid)``, u64 per
    key; 0, 0 for a key the tally does not hold."""
    n = len(offs) - 1
    events, valid = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    if n > 0:
        b = np.ascontiguousarray(buf, np.uint8)
        o = np.ascontiguousarray(offs, np.uint32)
        ctx.call("ske_tally_query", int(tid), b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n,
                 events.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p), SKE_MEM_HOST)
    return events, valid


def tally_import(ctx: Context, tid: int, keys, events, valid) -> None:
    """ske_tally_import: insert-or-add of a listing (keys as bytes)."""
    n = len(keys)
    if not (len(events) == n and len(valid) == n):
        raise ValueError("one events and one valid count per key")
    if n == 0:
        return
    if max(len(k) for k in keys) > SKE_TALLY_KEY_BYTES:
        raise ValueError(f"a tally key has at most {SKE_TALLY_KEY_BYTES} bytes")
    kb = np.zeros((n, SKE_TALLY_KEY_BYTES), np.uint8)
    for i, k in enumerate(keys):
        kb[i, :len(k)] = np.frombuffer(k, np.uint8)
    lens = np.asarray([len(k) for k in keys], np.uint32)
    ev = np.ascontiguousarray(events, dtype=np.uint64)
    va = np.ascontiguousarray(valid, dtype=np.uint64)
    ctx.call("ske_tally_import", int(tid), kb.ctypes.data_as(C.c_void_p), lens.ctypes.data_as(C.c_void_p),
             ev.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), n)


def seen_info(ctx: Context, sid: int) -> dict:
    """ske_seen_info: capacity, limit, used, the adds run so far, the items
    the masks let through, the first sightings among them and the items that
    found no slot (answered first: the set fails open)."""
    info = SeenInfo()
    ctx.call("ske_seen_info", int(sid), C.byref(info))
    return {k: int(getattr(info, k)) for k, _ in SeenInfo._fields_}


def seen_add_keys(ctx: Context, sid: int, keys: np.ndarray, mask=None, want: int = 0) -> np.ndarray:
    """ske_seen_add over a host ``[n, 2]`` uint64 array of row keys: one answer
    byte per key (SKE_SEEN_FIRST / REPEAT / SKIPPED)."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 2)
    n = k.shape[0]
    out = np.zeros(n, np.uint8)
    m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8).reshape(-1)
    if m is not None and m.size != n:
        raise ValueError("one mask byte per key")
    if n:
        ctx.call("ske_seen_add", int(sid), k.ctypes.data_as(C.c_void_p), n,
                 None if m is None else m.ctypes.data_as(C.c_void_p), int(want), out.ctypes.data_as(C.c_void_p),
                 SKE_MEM_HOST)
    return out


def seen_test_keys(ctx: Context, sid: int, keys: np.ndarray) -> np.ndarray:
    """ske_seen_test over a host ``[n, 2]`` uint64 array: bool per key."""
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, 2)
    n = k.shape[0]
    out = np.zeros(n, np.uint8)
    if n:
        ctx.call("ske_seen_test", int(sid), k.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p),
                 SKE_MEM_HOST)
    return out.astype(bool)


def rows_info(ctx: Context, rid: int) -> dict:
    """ske_rows_info: capacity, used, the rows taken, the refused ids among
    them, the rows dropped at a full log and the sticky overflow word."""
    info = RowsInfo()
    ctx.call("ske_rows_info", int(rid), C.byref(info))
    return {k: int(getattr(info, k)) for k, _ in RowsInfo._fields_}


def rows_compact(ctx: Context, rid: int, keep_since: int) -> dict:
    """ske_rows_compact: the superseded rows and those with ``epoch <
    keep_since`` leave the log, the survivors move to the front in arrival
    order; ``before``, ``kept``, ``superseded`` and ``expired`` as Python ints."""
    out = RowsCompact()
    ctx.call("ske_rows_compact", int(rid), int(keep_since), C.byref(out))
    return {k: int(getattr(out, k)) for k, _ in RowsCompact._fields_}


def rows_read(ctx: Context, rid: int, first: int, n: int):
    """ske_rows_read: the raw log columns of positions ``[first, first + n)``:
    ``(lecture digests u64, epochs i64, ids i64, valid u8)``."""
    n = int(n)
    lec, ep, ids, valid = np.zeros(n, np.uint64), np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint8)
    if n:
        ctx.call("ske_rows_read", int(rid), int(first), n, lec.ctypes.data_as(C.c_void_p),
                 ep.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), valid.ctypes.data_as(C.c_void_p))
    return lec, ep, ids, valid


def rows_select(ctx: Context, rid: int, lecture: bytes | None, since: int, until: int, cols=None):
    """ske_rows_select to host arrays: ``(cols, n, complete)``, ``cols`` the
    four columns of which the first ``n`` entries are the answer.  ``cols``
    given: a previous call's arrays, reused while they are large enough;
    otherwise (or when they are too small) the count is asked for first
    (``cap = 0``) and arrays of that size are made."""
    n_out, complete = C.c_uint64(), C.c_int()
    lec = None if lecture is None else C.c_char_p(lecture)
    llen = 0 if lecture is None else len(lecture)

    def call(cols, cap) -> bool:
        """False: the rows do not fit ``cap`` (n_out says how many there are)."""
        ptrs = [None] * 4 if cap == 0 else [c.ctypes.data_as(C.c_void_p) for c in cols]
        try:
            ctx.call("ske_rows_select", int(rid), lec, llen, int(since), int(until), *ptrs, cap, C.byref(n_out),
                     C.byref(complete), SKE_MEM_HOST)
        except SketchLibError as e:
            if e.code != SKE_EROWSSPACE:
                raise
            return False
        return int(n_out.value) <= cap

    cap = 0 if cols is None else int(cols[0].size)
    if not call(cols, cap):
        cap = int(n_out.value)
        cols = (np.zeros(cap, np.uint64), np.zeros(cap, np.int64), np.zeros(cap, np.int64), np.zeros(cap, np.uint8))
        if not call(cols, cap):
            raise SketchLibError(SKE_EROWSSPACE, "ERR row log selection does not fit the output")
    if cols is None:
        cols = (np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8))
    return cols, int(n_out.value), bool(complete.value)


def rows_group(ctx: Context, rid: int, by: int, lecture: bytes | None, since: int, until: int, valid_filter: int,
               sod_from: int, want_groups: bool = True):
    """ske_rows_group to host arrays: ``(keys u64, counts u64, stats, complete)``
    -- the groups with at least one counted row in ascending key order (the keys
    as the call writes them: a student id's two's-complement bits, a lecture's
    digest) and the fields of ske_rows_group_stats_t as Python ints.  The
    statistics are asked for first (``cap = 0``), then arrays of ``n`` entries
    are filled by a second call; ``want_groups`` False stops after the first."""
    n_out, complete, st = C.c_uint64(), C.c_int(), RowsGroupStats()
    lec = None if lecture is None else C.c_char_p(lecture)
    llen = 0 if lecture is None else len(lecture)
    head = (int(rid), int(by), lec, llen, int(since), int(until), int(valid_filter), int(sod_from))

    def call(keys, counts, cap) -> bool:
        ptrs = [None, None] if cap == 0 else [keys.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p)]
        try:
            ctx.call("ske_rows_group", *head, *ptrs, cap, C.byref(n_out), C.byref(st), C.byref(complete),
                     SKE_MEM_HOST)
        except SketchLibError as e:
            if e.code != SKE_EROWSSPACE:
                raise
            return False
        return int(n_out.value) <= cap

    keys, counts = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    if not call(keys, counts, 0) and want_groups:
        cap = int(n_out.value)
        keys, counts = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        if not call(keys, counts, cap):
            raise SketchLibError(SKE_EROWSSPACE, "ERR row log selection does not fit the output")
    n = int(n_out.value)
    stats = {k: int(getattr(st, k)) for k, _ in RowsGroupStats._fields_}
    return keys[:n], counts[:n], stats, bool(complete.value)


def _two_calls(call, n_out, want_groups: bool, alloc):
    """``cap = 0`` first (the statistics, and how many groups there are), then
    ``alloc(n)`` -- ``(what to return, the two pointers)`` -- and the call
    that fills them; returns what ``alloc`` made, or None when nothing is
    listed or ``want_groups`` is false."""
    def once(ptrs, cap) -> bool:
        try:
            call(ptrs, cap)
        except SketchLibError as e:
            if e.code != SKE_EROWSSPACE:
                raise
            return False
        return int(n_out.value) <= cap

    if once((None, None), 0) or not want_groups:
        return None
    cap = int(n_out.value)
    made, ptrs = alloc(cap)
    if not once(tuple(C.c_void_p(int(p)) for p in ptrs), cap):
        raise SketchLibError(SKE_EROWSSPACE, "ERR row log selection does not fit the output")
    return made


def _host_groups(cap: int):
    keys, counts = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    return (keys, counts), (keys.ctypes.data, counts.ctypes.data)


def rows_group_dev(ctx: Context, rid: int, by: int, lecture: bytes | None, since: int, until: int, valid_filter: int,
                   sod_from: int, alloc, want_groups: bool = True):
    """ske_rows_group with ``SKE_MEM_DEVICE`` outputs: ``(made, n, stats,
    complete)``.  The statistics are asked for first (``cap = 0``); with ``n``
    groups listed, ``alloc(n)`` returns ``(made, (keys pointer, counts
    pointer))`` -- device arrays of ``n`` u64 words each, the caller's (torch
    tensors, say) -- which a second call fills; ``made`` is handed back (None
    when nothing is listed or ``want_groups`` is false)."""
    n_out, complete, st = C.c_uint64(), C.c_int(), RowsGroupStats()
    lec = None if lecture is None else C.c_char_p(lecture)
    llen = 0 if lecture is None else len(lecture)
    head = (int(rid), int(by), lec, llen, int(since), int(until), int(valid_filter), int(sod_from))

    def call(ptrs, cap):
        ctx.call("ske_rows_group", *head, *ptrs, cap, C.byref(n_out), C.byref(st), C.byref(complete), SKE_MEM_DEVICE)

    made = _two_calls(call, n_out, want_groups, alloc)
    stats = {k: int(getattr(st, k)) for k, _ in RowsGroupStats._fields_}
    return made, int(n_out.value), stats, bool(complete.value)


def rows_group_merge(ctx: Context, by: int, keys, counts, n_in: int, mem: int = SKE_MEM_HOST,
                     want_groups: bool = True, alloc=None):
    """ske_rows_group_merge: ``(keys, counts, stats, multi)`` -- the ``n_in``
    (key, count) entries summed per key, the keys with a nonzero sum ascending
    (signed by student, unsigned by lecture).  ``SKE_MEM_HOST``: ``keys`` and
    ``counts`` are contiguous numpy arrays of 8-byte words and the answer comes
    as uint64 arrays.  ``SKE_MEM_DEVICE``: they are device pointers, and
    ``alloc(n)`` returns ``((keys, counts), (keys pointer, counts pointer))``
    for the ``n`` listed groups, as for ``rows_group_dev``; the pair it made is
    returned (``(None, None)`` when nothing is listed).  Two calls: ``cap = 0``
    first, then the fill; ``want_groups`` False stops after the first.
    ``stats`` holds ske_rows_group_stats_t's fields as Python ints, ``rows`` 0."""
    n_in = int(n_in)
    if n_in < 0:
        raise ValueError("n_in is a count")
    if mem == SKE_MEM_HOST:
        if n_in:
            for a in (keys, counts):
                if not (isinstance(a, np.ndarray) and a.dtype.itemsize == 8 and a.flags.c_contiguous
                        and a.size >= n_in):
                    raise ValueError("keys and counts are contiguous numpy arrays of n_in 8-byte words")
        kp = C.c_void_p(keys.ctypes.data) if n_in else None
        cp = C.c_void_p(counts.ctypes.data) if n_in else None
        alloc = _host_groups
    else:
        if alloc is None and want_groups:
            raise ValueError("device outputs need alloc")
        kp, cp = (C.c_void_p(int(keys)), C.c_void_p(int(counts))) if n_in else (None, None)
    n_out, multi, st = C.c_uint64(), C.c_uint64(), RowsGroupStats()

    def call(ptrs, cap):
        ctx.call("ske_rows_group_merge", int(by), kp, cp, n_in, *ptrs, cap, C.byref(n_out), C.byref(st),
                 C.byref(multi), int(mem))

    made = _two_calls(call, n_out, want_groups, alloc)
    stats = {k: int(getattr(st, k)) for k, _ in RowsGroupStats._fields_}
    if made is None:
        made = (np.zeros(0, np.uint64), np.zeros(0, np.uint64)) if mem == SKE_MEM_HOST else (None, None)
    return made[0], made[1], stats, int(multi.value)


def rows_profile(ctx: Context, rid: int, lecture: bytes | None, since: int, until: int, valid_filter: int,
                 sod_from: int):
    """ske_rows_profile: ``(bins, rows, complete)`` -- the counted rows per
    weekday (Monday first) and UTC hour as [7, 24] uint64, and the rows of the
    window after the upsert."""
    out = np.zeros(SKE_TP_BINS, np.uint64)
    rows, complete = C.c_uint64(), C.c_int()
    lec = None if lecture is None else C.c_char_p(lecture)
    ctx.call("ske_rows_profile", int(rid), lec, 0 if lecture is None else len(lecture), int(since), int(until),
             int(valid_filter), int(sod_from), out.ctypes.data_as(C.c_void_p), C.byref(rows), C.byref(complete))
    return out.reshape(7, 24), int(rows.value), bool(complete.value)


class SweBatch(C.Structure):
    """ske_swipe_batch (include/sketch.h)."""
    _fields_ = [("slot", C.c_void_p), ("bytes", C.c_void_p), ("offs", C.c_void_p),
                ("width", C.c_uint32), ("n", C.c_uint64), ("out_valid", C.c_void_p)]


class DeviceBatch:
    """Packed swipes resident on the device."""

    def __init__(self, ctx: Context, n: int, width: int):
        self.ctx, self.n, self.width = ctx, int(n), int(width)
        self.bytes = DeviceBuffer(ctx, self.n * width + 64)
        self.offs = DeviceBuffer(ctx, (self.n + 1) * 4)
        self.slot = DeviceBuffer(ctx, self.n * 4 + 16)

    @classmethod
    def from_host(cls, ctx: Context, buf: np.ndarray, offs: np.ndarray, slot: np.ndarray):
        b = cls.__new__(cls)
        b.ctx, b.n, b.width = ctx, len(offs) - 1, 0
        b.bytes = DeviceBuffer(ctx, buf.nbytes + 64)
        b.offs = DeviceBuffer(ctx, offs.nbytes)
        b.slot = DeviceBuffer(ctx, max(slot.nbytes, 16))
        b.bytes.from_host(np.ascontiguousarray(buf, np.uint8))
        b.offs.from_host(np.ascontiguousarray(offs, np.uint32))
        b.slot.from_host(np.ascontiguousarray(slot, np.uint32))
        return b

    def to_host(self):
        offs = self.offs.to_host(np.uint32, self.n + 1)
        buf = self.bytes.to_host(np.uint8, int(offs[-1]))
        slot = self.slot.to_host(np.uint32, self.n)
        return buf, offs, slot

    def free(self):
        for b in (self.bytes, self.offs, self.slot):
            b.free()


class Graph:
    """An executable HIP graph of recorded sketch calls (ske_capture_end)."""

    def __init__(self, ctx: Context, ptr: int):
        self.ctx, self.ptr = ctx, ptr

    def launch(self):
        self.ctx.call("ske_graph_launch", C.c_void_p(self.ptr))

    def free(self):
        if self.ptr:
            self.ctx.call("ske_graph_free", C.c_void_p(self.ptr))
            self.ptr = None


class SketchEngine:
    """Device-pointer driver over one libsketch context."""

    def __init__(self, device: int = 0, ctx: Context | None = None):
        self.ctx = ctx if ctx is not None else Context(device)
        self._cdf_bufs = []

    # ---- Bloom
    def reserve(self, fid: int, error: float, capacity: int, expansion: int = 2,
                nonscaling: bool = False):
        self.ctx.call("ske_bf_reserve", fid, float(error), int(capacity), int(expansion),
                      1 if nonscaling else 0)

    def gen_params(self, w: synthetic.Workload, seed=None, slot_base=0,
                   cdf: np.ndarray | None = None) -> GenParams:
        """Generator parameters; `cdf` (u32, n_keys entries) overrides the
        workload's own key distribution (e.g. a rank's share of the keys)."""
        if cdf is None:
            cdf = synthetic.key_cdf(w)
        dev = None
        if cdf is not None:
            buf = DeviceBuffer(self.ctx, cdf.nbytes)
            buf.from_host(cdf)
            self._cdf_bufs.append(buf)
            dev = buf.ptr
        return synthetic.gen_params(w, seed=seed, slot_base=slot_base, key_cdf_dev=dev)

    def members_batch(self, p: GenParams, start: int, n: int) -> DeviceBatch:
        width = self.ctx.lib.ske_gen_id_width(C.byref(p))
        b = DeviceBatch(self.ctx, n, width)
        self.ctx.call("ske_gen_members", C.byref(p), int(start), int(n), C.c_void_p(b.bytes.ptr),
                      C.c_void_p(b.offs.ptr))
        return b

    def preload(self, fid: int, p: GenParams, n: int, chunk: int = 1 << 24,
                replies: bool = False) -> np.ndarray | None:
        """BF.MADD of the first n members (data_generator.py:57-63 scaled)."""
        outs = []
        for s in range(0, n, chunk):
            m = min(chunk, n - s)
            b = self.members_batch(p, s, m)
            out = DeviceBuffer(self.ctx, m) if replies else None
            self.ctx.call("ske_bf_madd", fid, C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), m,
                          C.c_void_p(out.ptr) if out else None, SKE_MEM_DEVICE)
            if out:
                outs.append(out.to_host(np.int8, m))
                out.free()
            b.free()
        return np.concatenate(outs) if replies else None

    def swipe_batch(self, p: GenParams, start: int, n: int) -> DeviceBatch:
        width = self.ctx.lib.ske_gen_id_width(C.byref(p))
        b = DeviceBatch(self.ctx, n, width)
        self.ctx.call("ske_gen_swipes", C.byref(p), int(start), int(n), C.c_void_p(b.bytes.ptr),
                      C.c_void_p(b.offs.ptr), C.c_void_p(b.slot.ptr))
        return b

    # ---- hot path
    def hll_reserve(self, nslots: int):
        self.ctx.call("ske_hll_reserve", int(nslots))

    def swipes(self, fid: int, b: DeviceBatch, out: DeviceBuffer | None = None):
        self.ctx.call("ske_swipes", fid, C.c_void_p(b.slot.ptr), C.c_void_p(b.bytes.ptr),
                      C.c_void_p(b.offs.ptr), b.n, C.c_void_p(out.ptr) if out else None,
                      SKE_MEM_DEVICE)

    def swipes_async(self, fid: int, b: DeviceBatch, out: DeviceBuffer | None = None):
        self.ctx.call("ske_swipes_async", fid, C.c_void_p(b.slot.ptr), C.c_void_p(b.bytes.ptr),
                      C.c_void_p(b.offs.ptr), b.n, C.c_void_p(out.ptr) if out else None)

    def swipes_fixed(self, fid: int, b: DeviceBatch, out: DeviceBuffer | None = None):
        """K1 over a fixed-width batch (ids at bytes + i*width, no offsets)."""
        assert b.width > 0
        self.ctx.call("ske_swipes_fixed", fid, C.c_void_p(b.slot.ptr), C.c_void_p(b.bytes.ptr),
                      b.width, b.n, C.c_void_p(out.ptr) if out else None, SKE_MEM_DEVICE)

    def swipes_fixed_async(self, fid: int, b: DeviceBatch, out: DeviceBuffer | None = None):
        self.ctx.call("ske_swipes_fixed_async", fid, C.c_void_p(b.slot.ptr),
                      C.c_void_p(b.bytes.ptr), b.width, b.n, C.c_void_p(out.ptr) if out else None)

    @staticmethod
    def many_args(batches, outs=None, fixed: bool = False):
        """The ske_swipe_batch array of a many-batch call, built once: a
        caller that replays the same batches (a serving loop over resident
        buffers, the benchmark) passes it as `prepared` and skips the
        per-call Python marshalling."""
        outs = outs if outs is not None else [None] * len(batches)
        arr = (SweBatch * len(batches))()
        for a, b, o in zip(arr, batches, outs):
            a.slot, a.bytes = b.slot.ptr, b.bytes.ptr
            a.offs = None if fixed else b.offs.ptr
            a.width = b.width if fixed else 0
            a.n = b.n
            a.out_valid = o.ptr if o is not None else None
        return arr

    def swipes_many_async(self, fid: int, batches, outs=None, branches: int = 0,
                          fixed: bool = False, prepared=None):
        """Enqueue K1 over several resident batches in one native call
        (ske_swipes_many_async): batch j on branch j mod `branches` (0: 16),
        forked from and joined back into the context stream; with several
        branches two launches share the chip, half the CUs each.  `fixed`:
        read the ids as fixed-width (as swipes_fixed_async).  `prepared`: the
        many_args() array of these batches."""
        arr = prepared if prepared is not None else self.many_args(batches, outs, fixed)
        self.ctx.call("ske_swipes_many_async", fid, C.cast(arr, C.c_void_p), len(arr), branches)

    def swipes_stats(self, fid: int, b: DeviceBatch) -> tuple[int, int]:
        probes, nvalid = C.c_uint64(), C.c_uint64()
        self.ctx.call("ske_swipes_stats", fid, C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr),
                      b.n, C.byref(probes), C.byref(nvalid))
        return probes.value, nvalid.value

    def variant(self, fid: int) -> int:
        return self.ctx.lib.ske_swipes_variant(self.ctx.ptr, fid)

    def set_option(self, name: str, value: int):
        self.ctx.call("ske_set_option", name.encode(), int(value))

    def pass_times(self, reset: bool = True) -> list[tuple[float, int]]:
        """(summed ms, kernel count) per K1 pass kind, from the HIP event
        pairs the library records around each kernel while the option
        "pass_timing" is on: [single-kernel K1, partitioned A, B, C (or the
        segmented C1), segmented level-2 sort, segmented window apply, and a
        host-fed call's H2D copies, D2H copies, whole call]."""
        ms = (C.c_double * PASS_KINDS)()
        cnt = (C.c_uint64 * PASS_KINDS)()
        self.ctx.call("ske_pass_times", ms, cnt, 1 if reset else 0)
        return [(ms[i], cnt[i]) for i in range(PASS_KINDS)]

    def seg_floor_stats(self) -> tuple[int, int, int]:
        """(windows floored, records the level-2 sort saw, records it dropped)
        of the segmented PFADD since the last read; waits for the stream."""
        out = (C.c_uint64 * 3)()
        self.ctx.call("ske_seg_floor_stats", out)
        return int(out[0]), int(out[1]), int(out[2])

    def set_stream(self, stream_ptr: int | None):
        self.ctx.call("ske_set_stream", C.c_void_p(stream_ptr) if stream_ptr else None)

    def get_stream(self) -> int | None:
        """The stream calls enqueue on now (None: the context's own stream)."""
        p = C.c_void_p()
        self.ctx.call("ske_get_stream", C.byref(p))
        return p.value

    def sync(self):
        """Wait for the context stream; raises SKE_ERANGE (SketchLibError)
        when an enqueued K1 met a valid swipe whose slot is outside the slab."""
        self.ctx.call("ske_sync")

    def check_errors(self):
        self.ctx.call("ske_check_errors")

    # ---- Count-Min Sketch (per-student counters beside the swipe path)
    def cms_init(self, cid: int, width: int, depth: int):
        self.ctx.call("ske_cms_init", int(cid), int(width), int(depth))

    def cms_add(self, cid: int, b: DeviceBatch, mask: DeviceBuffer | None = None, want: int = 1,
                incr: DeviceBuffer | None = None):
        """The bulk, order-free add of a resident batch: item i counts
        ``incr[i]`` (u32; 1 each without ``incr``), with ``mask`` only the
        items whose mask byte equals ``want`` -- K1's answers read in place.
        A fixed-width batch is only enqueued (ske_cms_add_fixed_async, after
        swipes_fixed_async on the same stream, capturable; ``sync()`` waits);
        so is a masked batch of bytes + offsets (ske_cms_add_packed_async);
        an unmasked one goes through ske_cms_incrby, which returns when done."""
        if b.width > 0:
            self.ctx.call("ske_cms_add_fixed_async", int(cid), C.c_void_p(b.bytes.ptr), b.width, b.n,
                          C.c_void_p(incr.ptr) if incr else None, C.c_void_p(mask.ptr) if mask else None,
                          int(want))
            return
        if mask is not None:
            self.ctx.call("ske_cms_add_packed_async", int(cid), C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr),
                          b.n, C.c_void_p(incr.ptr) if incr else None, C.c_void_p(mask.ptr), int(want))
            return
        self.ctx.call("ske_cms_incrby", int(cid), C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), b.n,
                      C.c_void_p(incr.ptr) if incr else None, None, SKE_MEM_DEVICE)

    def cms_query(self, cid: int, b: DeviceBatch) -> np.ndarray:
        """The estimate (minimum over the rows) of every item of the batch."""
        out = DeviceBuffer(self.ctx, b.n * 4)
        try:
            self.ctx.call("ske_cms_query", int(cid), C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), b.n,
                          C.c_void_p(out.ptr), SKE_MEM_DEVICE)
            return out.to_host(np.uint32, b.n)
        finally:
            out.free()

    def cms_table(self, cid: int) -> tuple[np.ndarray, int]:
        """The whole table, [depth, width] u32, and its count."""
        info = CmsInfo()
        self.ctx.call("ske_cms_info", int(cid), C.byref(info))
        out = np.zeros((info.depth, info.width), np.uint32)
        self.ctx.call("ske_cms_export", int(cid), out.ctypes.data_as(C.c_void_p), out.size)
        return out, int(info.count)

    # ---- heavy hitters beside a Count-Min Sketch table
    def hh_init(self, hid: int, capacity_log2: int):
        self.ctx.call("ske_hh_init", int(hid), int(capacity_log2))

    def hh_free(self, hid: int):
        self.ctx.call("ske_hh_free", int(hid))

    def hh_reset(self, hid: int):
        self.ctx.call("ske_hh_reset", int(hid))

    def hh_info(self, hid: int) -> dict:
        return hh_info(self.ctx, hid)

    def hh_track(self, hid: int, cid: int, b: DeviceBatch, threshold: int, mask: DeviceBuffer | None = None,
                 want: int = 1):
        """Every id of the resident batch (with ``mask``: those whose mask
        byte equals ``want``) whose estimate in table ``cid`` is at least
        ``threshold`` joins set ``hid``.  A fixed-width batch is only enqueued
        (ske_hh_track_fixed_async, behind the batch's cms_add on the same
        stream, capturable; ``sync()`` waits); so is a masked batch of bytes +
        offsets (ske_hh_track_packed_async: an id over 16 bytes is skipped and
        turns ``complete`` false); an unmasked one goes through ske_hh_track,
        which returns when done."""
        if b.width > 0:
            self.ctx.call("ske_hh_track_fixed_async", int(hid), int(cid), C.c_void_p(b.bytes.ptr), b.width, b.n,
                          C.c_void_p(mask.ptr) if mask else None, int(want), int(threshold))
            return
        if mask is not None:
            self.ctx.call("ske_hh_track_packed_async", int(hid), int(cid), C.c_void_p(b.bytes.ptr),
                          C.c_void_p(b.offs.ptr), b.n, C.c_void_p(mask.ptr), int(want), int(threshold))
            return
        self.ctx.call("ske_hh_track", int(hid), int(cid), C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), b.n,
                      int(threshold), SKE_MEM_DEVICE)

    def hh_list(self, hid: int, cid: int, threshold: int):
        return hh_list(self.ctx, hid, cid, threshold)

    def hh_stats(self, hid: int, cid: int, threshold: int = 0) -> dict:
        return hh_stats(self.ctx, hid, cid, threshold)

    def hh_select(self, hid: int, cid: int, threshold: int, ranks) -> np.ndarray:
        return hh_select(self.ctx, hid, cid, threshold, ranks)

    # ---- time profile: weekday x hour counters of the swipes' times
    def tp_init(self, tid: int):
        self.ctx.call("ske_tp_init", int(tid))

    def tp_free(self, tid: int):
        self.ctx.call("ske_tp_free", int(tid))

    def tp_reset(self, tid: int):
        self.ctx.call("ske_tp_reset", int(tid))

    def tp_counts(self, tid: int) -> np.ndarray:
        return tp_counts(self.ctx, tid)

    def tp_import(self, tid: int, counts):
        tp_import(self.ctx, tid, counts)

    def tp_add(self, tid: int, epoch: DeviceBuffer, n: int, mask: DeviceBuffer | None = None, want: int = 1,
               late_from: int = 32400, late: DeviceBuffer | None = None):
        """One resident batch of ``n`` swipe times (int64 seconds since
        1970-01-01 UTC) into profile ``tid``: with ``mask`` only the swipes
        whose mask byte equals ``want`` count.  ``late`` (n bytes) receives 1
        for every swipe, masked or not, whose second of the day is at least
        ``late_from``.  Only enqueued (ske_tp_add_async, capturable; ``sync()``
        waits)."""
        self.ctx.call("ske_tp_add_async", int(tid), C.c_void_p(epoch.ptr), int(n),
                      C.c_void_p(mask.ptr) if mask else None, int(want), int(late_from),
                      C.c_void_p(late.ptr) if late else None)

    # ---- tallies: exact event counts per key
    def tally_init(self, tid: int, capacity_log2: int):
        self.ctx.call("ske_tally_init", int(tid), int(capacity_log2))

    def tally_free(self, tid: int):
        self.ctx.call("ske_tally_free", int(tid))

    def tally_reset(self, tid: int):
        self.ctx.call("ske_tally_reset", int(tid))

    def tally_info(self, tid: int) -> dict:
        return tally_info(self.ctx, tid)

    def tally_add(self, tid: int, b: DeviceBatch, mask: DeviceBuffer | None = None):
        """One resident batch of keys into tally ``tid``: every key counts one
        event, and one valid where its ``mask`` byte is 1.  Only enqueued
        (ske_tally_add_fixed_async for a fixed-width batch, else
        ske_tally_add_packed_async; capturable; ``sync()`` waits)."""
        m = C.c_void_p(mask.ptr) if mask else None
        if b.width > 0:
            self.ctx.call("ske_tally_add_fixed_async", int(tid), C.c_void_p(b.bytes.ptr), b.width, b.n, m)
        else:
            self.ctx.call("ske_tally_add_packed_async", int(tid), C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr),
                          b.n, m)

    def tally_add_spans(self, tid: int, msgs: DeviceBuffer, start: DeviceBuffer, length: DeviceBuffer, n: int,
                        status: DeviceBuffer | None = None, mask: DeviceBuffer | None = None):
        """ske_tally_add_spans_async: key i = ``msgs[start[i] .. start[i] +
        length[i])``, taken where ``status`` (if any) is 0.  Only enqueued."""
        self.ctx.call("ske_tally_add_spans_async", int(tid), C.c_void_p(msgs.ptr), C.c_void_p(start.ptr),
                      C.c_void_p(length.ptr), int(n), C.c_void_p(status.ptr) if status else None,
                      C.c_void_p(mask.ptr) if mask else None)

    def tally_list(self, tid: int, min_events: int = 0):
        return tally_list(self.ctx, tid, min_events)

    def tally_top(self, tid: int, k: int = 3, by: int = 0):
        return tally_top(self.ctx, tid, k, by)

    def tally_query(self, tid: int, buf: np.ndarray, offs: np.ndarray):
        return tally_query(self.ctx, tid, buf, offs)

    def tally_import(self, tid: int, keys, events, valid):
        tally_import(self.ctx, tid, keys, events, valid)

    # ---- seen-row sets (count each row once under redelivery)
    def seen_init(self, sid: int, capacity_log2: int):
        self.ctx.call("ske_seen_init", int(sid), int(capacity_log2))

    def seen_free(self, sid: int):
        self.ctx.call("ske_seen_free", int(sid))

    def seen_reset(self, sid: int):
        self.ctx.call("ske_seen_reset", int(sid))

    def seen_info(self, sid: int) -> dict:
        return seen_info(self.ctx, sid)

    def seen_fold(self, keys: DeviceBuffer, b: DeviceBatch, begin: bool):
        """One resident column folded into the ``2 * b.n`` key words of
        ``keys`` (ske_seen_fold_fixed_async for a fixed-width batch, else
        ske_seen_fold_packed_async; capturable)."""
        if b.width:
            self.ctx.call("ske_seen_fold_fixed_async", C.c_void_p(keys.ptr), C.c_void_p(b.bytes.ptr), b.width, b.n,
                          1 if begin else 0)
        else:
            self.ctx.call("ske_seen_fold_packed_async", C.c_void_p(keys.ptr), C.c_void_p(b.bytes.ptr),
                          C.c_void_p(b.offs.ptr), b.n, 1 if begin else 0)

    def seen_fold_epoch(self, keys: DeviceBuffer, epoch: DeviceBuffer, n: int, granularity: int, begin: bool):
        self.ctx.call("ske_seen_fold_epoch_async", C.c_void_p(keys.ptr), C.c_void_p(epoch.ptr), int(granularity),
                      int(n), 1 if begin else 0)

    def seen_add(self, sid: int, keys: DeviceBuffer, n: int, out: DeviceBuffer, mask: DeviceBuffer | None = None,
                 want: int = 0):
        """ske_seen_add_async: one answer byte per key into ``out`` (only
        enqueued, capturable; ``sync()`` waits)."""
        self.ctx.call("ske_seen_add_async", int(sid), C.c_void_p(keys.ptr), int(n),
                      C.c_void_p(mask.ptr) if mask is not None else None, int(want), C.c_void_p(out.ptr))

    def seen_test(self, sid: int, keys: DeviceBuffer, n: int, out: DeviceBuffer):
        self.ctx.call("ske_seen_test_async", int(sid), C.c_void_p(keys.ptr), int(n), C.c_void_p(out.ptr))

    # ---- row logs (the attendance rows in arrival order)
    def rows_init(self, rid: int, capacity_log2: int):
        self.ctx.call("ske_rows_init", int(rid), int(capacity_log2))

    def rows_free(self, rid: int):
        self.ctx.call("ske_rows_free", int(rid))

    def rows_reset(self, rid: int):
        self.ctx.call("ske_rows_reset", int(rid))

    def rows_info(self, rid: int) -> dict:
        return rows_info(self.ctx, rid)

    def rows_append_packed(self, rid: int, lec: DeviceBatch, ids: DeviceBatch, epoch: DeviceBuffer,
                           valid: DeviceBuffer | None = None, mask: DeviceBuffer | None = None):
        """ske_rows_append_fixed_async for fixed-width ids, else
        ske_rows_append_packed_async, over resident columns (only enqueued, capturable)."""
        vp = C.c_void_p(valid.ptr) if valid is not None else None
        mp = C.c_void_p(mask.ptr) if mask is not None else None
        if ids.width:
            self.ctx.call("ske_rows_append_fixed_async", int(rid), C.c_void_p(lec.bytes.ptr), C.c_void_p(lec.offs.ptr),
                          C.c_void_p(ids.bytes.ptr), ids.width, C.c_void_p(epoch.ptr), vp, mp, ids.n)
        else:
            self.ctx.call("ske_rows_append_packed_async", int(rid), C.c_void_p(lec.bytes.ptr),
                          C.c_void_p(lec.offs.ptr), C.c_void_p(ids.bytes.ptr), C.c_void_p(ids.offs.ptr),
                          C.c_void_p(epoch.ptr), vp, mp, ids.n)

    def rows_select(self, rid: int, lecture: bytes | None = None, since: int = -(1 << 63),
                    until: int = (1 << 63) - 1):
        return rows_select(self.ctx, rid, lecture, since, until)

    def rows_read(self, rid: int, first: int, n: int):
        return rows_read(self.ctx, rid, first, n)

    # ---- ingest: the decoded messages' times, and the decoded messages as one packed batch
    def ingest_times(self, msgs: DeviceBuffer, cols, n: int, epoch: DeviceBuffer):
        """ske_ingest_times: ``epoch[i]`` = message i's timestamp as seconds
        since 1970-01-01 UTC where ``ske_ingest_parse`` (``cols``, an
        ``IngestCols``) decoded it, else 0.  Only enqueued."""
        self.ctx.call("ske_ingest_times", C.c_void_p(msgs.ptr), C.byref(cols), int(n), C.c_void_p(epoch.ptr))

    def ingest_dense(self, msgs: DeviceBuffer, cols, n: int, out: IngestDense, cap_bytes: int,
                     valid: DeviceBuffer | None = None, epoch: DeviceBuffer | None = None) -> tuple[int, int]:
        """ske_ingest_dense: the decoded messages, in order, packed into
        ``out``'s device arrays; returns ``(ndense, nbytes)``."""
        nd, nb = C.c_uint64(), C.c_uint64()
        self.ctx.call("ske_ingest_dense", C.c_void_p(msgs.ptr), C.byref(cols), int(n),
                      C.c_void_p(valid.ptr) if valid else None, C.c_void_p(epoch.ptr) if epoch else None,
                      C.byref(out), int(cap_bytes), C.byref(nd), C.byref(nb))
        return int(nd.value), int(nb.value)

    # ---- HIP graphs: record enqueue-only calls once, replay many times
    def capture(self, fn) -> "Graph":
        """Record the device work `fn()` enqueues on the context stream (only
        *_async calls) into an uploaded executable graph.

        Python's cyclic garbage collector is run before and held off during
        the recording: a collection inside it could finalise an unreachable
        Context or device buffer (ske_close / hipFree / hipStreamSynchronize),
        which a thread-local stream capture forbids -- the capture would be
        invalidated and this recording fail."""
        with _no_gc():
            self.ctx.call("ske_capture_begin")
            try:
                fn()
            except BaseException:
                # end the capture (the stream must leave capture mode) and drop
                # the partial graph; the recording call's error is the one raised
                g = C.c_void_p()
                if self.ctx.lib.ske_capture_end(self.ctx.ptr, C.byref(g)) == 0 and g.value:
                    self.ctx.lib.ske_graph_free(self.ctx.ptr, g)
                raise
            g = C.c_void_p()
            self.ctx.call("ske_capture_end", C.byref(g))
        return Graph(self.ctx, g.value)

    def capture_branched(self, steps, main, side) -> "Graph":
        """Record `steps` (callables, each enqueuing one *_async call) into one
        graph of 1 + len(side) independent branches: step j on branch
        j mod (1 + len(side)), forked from and joined back into `main` (torch
        streams).  On replay, launches of different branches overlap; with the
        "k1_grid" option at half the CUs two K1 launches share the chip.  The
        context stream is `main` afterwards."""
        import torch
        streams = [main] + list(side)
        fork = torch.cuda.Event()
        joins = [torch.cuda.Event() for _ in side]

        def record():
            fork.record(main)
            for s_ in side:
                s_.wait_event(fork)
            for j, fn in enumerate(steps):
                self.set_stream(streams[j % len(streams)].cuda_stream)
                fn()
            for s_, ev in zip(side, joins):
                ev.record(s_)
                main.wait_event(ev)
            self.set_stream(main.cuda_stream)

        self.set_stream(main.cuda_stream)
        return self.capture(record)

    # ---- HLL reads
    def registers(self, slot: int) -> np.ndarray:
        out = np.zeros(16384, np.uint8)
        self.ctx.call("ske_hll_export_raw", int(slot), out.ctypes.data_as(C.c_void_p))
        return out

    def registers_all(self, nslots: int) -> np.ndarray:
        p, nb = C.c_void_p(), C.c_uint64()
        self.ctx.call("ske_hll_slab", C.byref(p), C.byref(nb))
        out = np.zeros((nslots, 16384), np.uint8)
        assert nslots * 16384 <= nb.value
        self.ctx.call("ske_memcpy", out.ctypes.data_as(C.c_void_p), p, out.nbytes, 1)
        return out

    def pfcount_each(self, slots) -> np.ndarray:
        s = np.ascontiguousarray(slots, dtype=np.uint32)
        out = np.zeros(s.size, np.uint64)
        if s.size:
            self.ctx.call("ske_hll_pfcount_each", s.ctypes.data_as(C.c_void_p), s.size,
                          out.ctypes.data_as(C.c_void_p), 0)
        return out

    # ---- HLL keys as Redis strings, many a call, every array on the device
    def hll_dump_sizes(self, slots: DeviceBuffer | None, nkeys: int, offs: DeviceBuffer,
                       sparse_max_bytes: int = 3000):
        """ske_hll_dump_sizes: ``offs`` (nkeys + 1 u32) receives the byte offset
        of every listed key's "HYLL" string, the last entry the total.
        ``slots`` None: keys 0 .. nkeys - 1."""
        self.ctx.call("ske_hll_dump_sizes", C.c_void_p(slots.ptr) if slots else None, int(nkeys),
                      int(sparse_max_bytes), C.c_void_p(offs.ptr), SKE_MEM_DEVICE)

    def hll_dump(self, slots: DeviceBuffer | None, nkeys: int, out: DeviceBuffer, offs: DeviceBuffer,
                 sparse_max_bytes: int = 3000, with_card: bool = False):
        """ske_hll_dump: the strings back to back into ``out`` (its size is
        the capacity), their offsets into ``offs``."""
        self.ctx.call("ske_hll_dump", C.c_void_p(slots.ptr) if slots else None, int(nkeys), int(sparse_max_bytes),
                      SKE_HLL_DUMP_CARD if with_card else 0, C.c_void_p(out.ptr), int(out.nbytes),
                      C.c_void_p(offs.ptr), SKE_MEM_DEVICE)

    def hll_load(self, slots: DeviceBuffer | None, nkeys: int, blob: DeviceBuffer, offs: DeviceBuffer,
                 status: DeviceBuffer | None = None):
        """ske_hll_load: SET of the nkeys strings ``blob[offs[i] .. offs[i + 1])``
        into the (distinct) slots; raises SKE_EBADHLL after loading the good
        ones when a string is refused (``status``: a byte per key)."""
        self.ctx.call("ske_hll_load", C.c_void_p(slots.ptr) if slots else None, int(nkeys), C.c_void_p(blob.ptr),
                      C.c_void_p(offs.ptr), C.c_void_p(status.ptr) if status else None, SKE_MEM_DEVICE)

    def bloom_bits(self, fid: int, link: int, nbytes: int) -> np.ndarray:
        out = np.zeros(nbytes, np.uint8)
        self.ctx.call("ske_bf_export_link", fid, link, out.ctypes.data_as(C.c_void_p), nbytes)
        return out
