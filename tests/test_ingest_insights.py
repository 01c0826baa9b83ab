"""Insights from the message stream on the device: ske_ingest_times against
``epoch_seconds(fromisoformat(...))``, ske_ingest_dense against a numpy
restatement built from the parse columns, the packed masked adds and tracks
against their fixed-width siblings, and ``StudentCounts.update_messages`` /
``AttendanceProcessor(counts=...)`` end to end against a Counter / datetime
restatement of the reference's group-bys (attendance_analysis.py:65-118)."""
import collections
import ctypes as C
import json
import os
from datetime import datetime

import numpy as np
import pytest

import __graft_entry__ as ge
from test_processor import reference_messages
from test_tp import cms_estimates

pytestmark = pytest.mark.gpu

DAY_NAMES = ("Monday", "Tuesday", "Wednesday", "Thursday", "Friday", "Saturday", "Sunday")
GUARD = 0xA5
COLS = ("status", "id_start", "id_len", "lec_start", "lec_len", "ts_start", "ts_len", "day", "kh")


def make_context(grid=None):
    """a context opened with SKE_INGEST_GRID (ske_open reads it)"""
    pkg = ge.load_package()
    if grid is not None:
        os.environ["SKE_INGEST_GRID"] = str(grid)
    try:
        return pkg.Context(0)
    finally:
        os.environ.pop("SKE_INGEST_GRID", None)


@pytest.fixture(scope="module")
def contexts():
    """the default launch shape, and 1 and 3 workgroups (the stride loop over a few hundred messages)"""
    return {g: make_context(g) for g in (None, 1, 3)}


class Parsed:
    """A batch of messages uploaded and decoded by ske_ingest_parse.  The
    payload buffer ends at the first 8-byte boundary behind the last message."""

    def __init__(self, ctx, msgs, day_form=1):
        from rtsas_amd._lib import IngestCols
        from rtsas_amd.engine import DeviceBuffer
        self.ctx, self.n = ctx, len(msgs)
        n = self.n
        self.blob = np.frombuffer(b"".join(msgs), np.uint8)
        moffs = np.zeros(n + 1, np.uint32)
        np.cumsum([len(m) for m in msgs], out=moffs[1:])
        self.bufs = {"msgs": DeviceBuffer(ctx, (self.blob.size + 7) & ~7), "moffs": DeviceBuffer(ctx, (n + 1) * 4),
                     "status": DeviceBuffer(ctx, n), "day": DeviceBuffer(ctx, n * 4), "kh": DeviceBuffer(ctx, n * 16)}
        for k in COLS[1:7]:
            self.bufs[k] = DeviceBuffer(ctx, n * 4)
        self.bufs["msgs"].from_host(self.blob)
        self.bufs["moffs"].from_host(moffs)
        self.cols = IngestCols(*[C.c_void_p(self.bufs[k].ptr) for k in COLS])
        self.msgs = C.c_void_p(self.bufs["msgs"].ptr)
        ctx.call("ske_ingest_parse", self.msgs, C.c_void_p(self.bufs["moffs"].ptr), n, day_form, C.byref(self.cols))

    def col(self, name, dtype=np.uint32):
        return self.bufs[name].to_host(dtype, self.n)

    def times(self):
        from rtsas_amd.engine import DeviceBuffer
        ep = DeviceBuffer(self.ctx, self.n * 8 + 16)
        self.bufs["epoch"] = ep
        ep.from_host(np.full(self.n + 2, -7, np.int64))
        self.ctx.call("ske_ingest_times", self.msgs, C.byref(self.cols), self.n, C.c_void_p(ep.ptr))
        out = ep.to_host(np.int64, self.n + 2)
        assert out[self.n:].tolist() == [-7, -7]  # nothing behind the n entries
        return out[:self.n]

    def free(self):
        for b in self.bufs.values():
            b.free()


# ---------------------------------------------------------------- times
# every fast-path form: date only, T / space / other separators, no fraction,
# .fff, .ffffff, naive, +HH:MM, -HH:MM; the year-2 and year-9998 edges, pre-1970
FAST = [
    "2025-03-19", "2025-03-19T08:59:59", "2025-03-19 09:00:00", "2025-03-19_09:00:00", "2025-03-19x23:59:59",
    "2025-03-19T09:00:00.123", "2025-03-19T09:00:00.123456", "2025-03-19 08:59:59.999", "2025-03-19T08:59:59.999999",
    "2025-03-19T02:10:00+05:30", "2025-03-19T23:30:00-02:00", "2025-03-19T23:30:00.250-02:00",
    "2025-03-19T00:00:00.250000+23:59", "2025-12-31T23:59:59.999-23:59", "2025-01-01 00:00:00.000001+00:01",
    "0002-01-01", "0002-01-01T00:00:00+23:59", "0002-01-01T00:00:01.500", "9998-12-31T23:59:59-23:59",
    "9998-12-31T23:59:59.999999", "0001-01-01", "0001-01-01T00:00:00", "9999-12-31T23:59:59",
    "1969-12-31T23:59:58.250", "1969-12-31T23:59:59+00:00", "1970-01-01T00:00:00-00:01", "1960-02-29T12:00:00+01:00",
    "2000-02-29T23:59:59.000", "2024-02-29", "1900-03-01T00:00:00",
]
# left to the host (status 1) or not decodable at all: their epoch is 0
SLOW = [
    b'{"student_id": 1, "lecture_id": "L", "timestamp": "2025-13-01"}',
    b'{"student_id": 1, "lecture_id": "L", "timestamp": "2025-03-19T09:00"}',
    b'{"student_id": 1, "lecture_id": "L", "timestamp": "0001-01-01T00:00:00+01:00"}',
    b'{"student_id": 1.5, "lecture_id": "L", "timestamp": "2025-03-19T09:00:00"}',
    b'{"student_id": "a\\u0041", "lecture_id": "L", "timestamp": "2025-03-19T09:00:00"}',
    b'not json', b'{}', b'',
]


def ts_message(ts, k=0):
    """a message with the timestamp first, in the middle or last"""
    fields = [('"student_id"', str(10000 + k)), ('"lecture_id"', '"L%d"' % (k % 5)), ('"timestamp"', '"%s"' % ts)]
    order = ([2, 0, 1], [0, 2, 1], [0, 1, 2])[(k // 7) % 3]
    return ("{" + ", ".join(fields[i][0] + ": " + fields[i][1] for i in order) + "}").encode()


def expected_epoch(pkg, ts):
    return int(pkg.epoch_seconds([datetime.fromisoformat(ts)])[0])


@pytest.mark.parametrize("grid", [None, 1, 3])
def test_times_every_alignment(pkg, contexts, grid):
    """Every form behind a filler of 0..7 bytes, so every message -- and with it
    every timestamp span -- starts at every offset mod 8; 900 messages, so that
    1 and 3 workgroups walk the stride loop."""
    ctx = contexts[grid]
    assert len({len(t) for t in FAST}) == 7
    msgs, want = [], []
    for k in range(900):
        if k % 11 == 10:
            msgs.append(SLOW[(k // 11) % len(SLOW)])
            want.append(None)
        else:
            ts = FAST[k % len(FAST)]
            msgs.append(ts_message(ts, k))
            want.append(expected_epoch(pkg, ts))
    exp = np.asarray([w or 0 for w in want], np.int64)
    exp_status = np.asarray([w is None for w in want], np.uint8)
    span_starts = set()
    for pad in range(8):
        p = Parsed(ctx, [b"x" * pad] + msgs)
        try:
            status = p.col("status", np.uint8)
            assert status[0] == 1 and np.array_equal(status[1:], exp_status), pad
            span_starts |= set((p.col("ts_start")[1:][exp_status == 0] % 8).tolist())
            got = p.times()
            assert got[0] == 0 and np.array_equal(got[1:], exp), pad
        finally:
            p.free()
    assert span_starts == set(range(8))


def test_times_span_ends_at_the_last_boundary(pkg, contexts):
    """The timestamp last in the last message, ending on the last byte before
    the buffer's final 8-byte boundary (the closing quote and brace lie in the
    final word): every form.  With the end pinned, a span starts where its
    length puts it -- six of the eight bytes of a word over the seven lengths;
    test_times_every_alignment starts the spans at all eight."""
    ctx = contexts[None]
    starts = set()
    for ts in FAST:
        msg = ('{"student_id": 1, "lecture_id": "L", "timestamp": "%s"}' % ts).encode()
        pad = -(len(msg) - 2) % 8
        p = Parsed(ctx, [b"x" * pad, msg])
        try:
            assert p.blob.size % 8 == 2 and p.bufs["msgs"].nbytes == p.blob.size + 6
            assert p.col("status", np.uint8).tolist() == [1, 0]
            s, ln = int(p.col("ts_start")[1]), int(p.col("ts_len")[1])
            assert (s + ln) % 8 == 0 and s + ln == p.blob.size - 2 and ln == len(ts)
            starts.add(s % 8)
            assert p.times().tolist() == [0, expected_epoch(pkg, ts)], ts
        finally:
            p.free()
    assert starts == {-n % 8 for n in (10, 19, 23, 26, 25, 29, 32)} == {0, 1, 3, 5, 6, 7}


# ---------------------------------------------------------------- dense
ID_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 40)


def dense_messages(rng, n, kinds=("str", "int", "host", "junk")):
    out = []
    for k in range(n):
        kind = kinds[int(rng.integers(0, len(kinds)))]
        ln = ID_LENGTHS[int(rng.integers(0, len(ID_LENGTHS)))]
        ts = FAST[int(rng.integers(0, len(FAST)))]
        if kind == "str":
            sid = '"%s"' % "".join(chr(int(c)) for c in rng.integers(97, 123, ln))
        elif kind == "int":
            ln = max(ln, 1)
            sid = str(int(rng.integers(1, 10))) + "".join(str(int(c)) for c in rng.integers(0, 10, ln - 1))
        elif kind == "host":
            sid = ('"\\u0041%d"' % k, "12.5", "-0")[k % 3]
        else:
            out.append((b"not json", b'{"student_id": 1}', b'{"student_id": 1, "lecture_id": "L", "timestamp": "x"}')[k % 3])
            continue
        out.append(('{"student_id": %s, "timestamp": "%s", "lecture_id": "LECT%d"}' % (sid, ts, k % 3)).encode())
    return out


def run_dense(ctx, p, valid=None, epoch=None, cap=None):
    """ske_ingest_dense into guarded buffers; returns rc, the totals and the buffers read back"""
    from rtsas_amd._lib import IngestDense
    from rtsas_amd.engine import DeviceBuffer
    n = p.n
    room = int(p.blob.size) + 64
    sizes = {"ids": room, "offs": (n + 3) * 4, "epoch": (n + 2) * 8, "valid": n + 16, "at": (n + 2) * 4}
    bufs = {k: DeviceBuffer(ctx, v) for k, v in sizes.items()}
    d_valid = d_epoch = None
    try:
        for k, v in sizes.items():
            bufs[k].from_host(np.full(v, GUARD, np.uint8))
        if valid is not None:
            d_valid = DeviceBuffer(ctx, n + 16)
            d_valid.from_host(valid)
        if epoch is not None:
            d_epoch = DeviceBuffer(ctx, n * 8 + 16)
            d_epoch.from_host(epoch)
        out = IngestDense(*[C.c_void_p(bufs[k].ptr) for k in ("ids", "offs", "epoch", "valid", "at")])
        nd, nb = C.c_uint64(99), C.c_uint64(99)
        rc = ctx.lib.ske_ingest_dense(ctx.ptr, p.msgs, C.byref(p.cols), n, C.c_void_p(d_valid.ptr) if d_valid else None,
                                      C.c_void_p(d_epoch.ptr) if d_epoch else None, C.byref(out),
                                      room - 64 if cap is None else cap, C.byref(nd), C.byref(nb))
        return rc, int(nd.value), int(nb.value), {k: bufs[k].to_host(np.uint8, sizes[k]) for k in sizes}
    finally:
        for b in list(bufs.values()) + [d_valid, d_epoch]:
            if b is not None:
                b.free()


def check_dense(ctx, rng, msgs, with_inputs=True):
    p = Parsed(ctx, msgs)
    try:
        n = p.n
        status, start, ln = p.col("status", np.uint8), p.col("id_start"), p.col("id_len")
        take = np.nonzero(status == 0)[0]
        valid = rng.integers(0, 2, n).astype(np.uint8) if with_inputs else None
        epoch = p.times() if with_inputs else None
        # the restatement, from the parse columns read back
        want_ids = b"".join(p.blob[start[m]:start[m] + ln[m]].tobytes() for m in take)
        want_offs = np.zeros(len(take) + 1, np.uint32)
        np.cumsum(ln[take], out=want_offs[1:])
        assert (ln[status != 0] == 0).all()
        rc, nd, nb, got = run_dense(ctx, p, valid, epoch)
        assert (rc, nd, nb) == (0, len(take), len(want_ids))
        assert got["ids"][:nb].tobytes() == want_ids and (got["ids"][nb:] == GUARD).all()
        offs = got["offs"].view(np.uint32)
        assert np.array_equal(offs[:nd + 1], want_offs) and (got["offs"][(nd + 1) * 4:] == GUARD).all()
        ep = got["epoch"].view(np.int64)
        assert np.array_equal(ep[:nd], epoch[take] if with_inputs else np.zeros(nd, np.int64))
        assert (got["epoch"][nd * 8:] == GUARD).all()
        assert np.array_equal(got["valid"][:nd], valid[take] if with_inputs else np.zeros(nd, np.uint8))
        assert (got["valid"][nd:] == GUARD).all()
        assert np.array_equal(got["at"].view(np.uint32)[:nd], take) and (got["at"][nd * 4:] == GUARD).all()
        if nb:  # one byte short: refused with the need reported and nothing written
            rc, nd2, nb2, got = run_dense(ctx, p, valid, epoch, cap=nb - 1)
            assert (rc, nd2, nb2) == (-1, nd, nb)
            assert all((v == GUARD).all() for v in got.values())
            assert run_dense(ctx, p, valid, epoch, cap=nb)[0] == 0  # exactly enough
        return nd, set(ln[take].tolist())
    finally:
        p.free()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3 * 256 * 2 + 5])
@pytest.mark.parametrize("grid", [None, 1, 3])
def test_dense_parity(contexts, grid, n):
    rng = np.random.default_rng(1000 * n + (grid or 0))
    nd, lens = check_dense(contexts[grid], rng, dense_messages(rng, n))
    if n > 200:
        assert 0 < nd < n and lens == set(ID_LENGTHS)


@pytest.mark.parametrize("grid", [None, 3])
def test_dense_all_host_all_device_and_no_inputs(contexts, grid):
    ctx = contexts[grid]
    rng = np.random.default_rng(5)
    n = 3 * 256 * 2 + 5
    assert check_dense(ctx, rng, dense_messages(rng, n, kinds=("host", "junk")))[0] == 0
    assert check_dense(ctx, rng, dense_messages(rng, n, kinds=("str", "int")))[0] == n
    assert check_dense(ctx, rng, dense_messages(rng, 300), with_inputs=False)[0] > 0  # NULL valid / epoch: zeros
    assert check_dense(ctx, rng, [b'{"student_id": "", "lecture_id": "L", "timestamp": "2025-03-19"}']) == (1, {0})


# ---------------------------------------------------------------- packed forms
def packed_twins(pkg, engine, ids, mask, want, dims, threshold, base):
    """the same ids fixed-width into keys (base, base) and packed into (base + 1, base + 1)"""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    n, width = len(ids), len(ids[0])
    fixed = DeviceBatch(engine.ctx, n, width)
    fixed.bytes.from_host(np.frombuffer(b"".join(ids), np.uint8))
    buf, offs = pkg.pack(ids)
    packed = DeviceBatch.from_host(engine.ctx, buf, offs, np.zeros(n, np.uint32))
    d_mask = None
    if mask is not None:
        d_mask = DeviceBuffer(engine.ctx, n + 16)
        d_mask.from_host(mask)
    out = []
    try:
        for cid, hid, b in ((base, base, fixed), (base + 1, base + 1, packed)):
            engine.cms_init(cid, *dims)
            engine.hh_init(hid, 12)
            if b is packed:  # also without a mask the enqueue-only form
                engine.ctx.call("ske_cms_add_packed_async", cid, C.c_void_p(b.bytes.ptr), C.c_void_p(b.offs.ptr), n,
                                None, C.c_void_p(d_mask.ptr) if d_mask else None, want)
                engine.ctx.call("ske_hh_track_packed_async", hid, cid, C.c_void_p(b.bytes.ptr),
                                C.c_void_p(b.offs.ptr), n, C.c_void_p(d_mask.ptr) if d_mask else None, want, threshold)
            else:
                engine.cms_add(cid, b, d_mask, want)
                engine.hh_track(hid, cid, b, threshold, d_mask, want)
            engine.sync()
            table, count = engine.cms_table(cid)
            ids_l, est, complete = engine.hh_list(hid, cid, threshold)
            out.append((table, count, ids_l, est.tolist(), complete, engine.hh_info(hid)))
    finally:
        for cid in (base, base + 1):
            engine.hh_free(cid)
            engine.ctx.call("ske_cms_free", cid)
        fixed.free()
        packed.free()
        if d_mask:
            d_mask.free()
    return out


@pytest.mark.parametrize("dims", [(2000, 7), (20011, 3)])  # the LDS form and the memory form of add and track
@pytest.mark.parametrize("masked,want", [(True, 0), (True, 1), (False, 1)])
def test_packed_forms_equal_fixed(pkg, engine, dims, masked, want):
    rng = np.random.default_rng(77)
    pool = [b"%05d" % v for v in rng.choice(np.arange(10000, 100000), 300, replace=False)]
    n = 5003
    ids = [pool[int(i)] for i in np.minimum(rng.geometric(0.02, n) - 1, 299)]
    mask = (rng.random(n) < 0.7).astype(np.uint8) if masked else None
    a, b = packed_twins(pkg, engine, ids, mask, want, dims, 12, 10)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] == (n if mask is None else int((mask == want).sum()))
    assert a[2:] == b[2:] and len(a[2]) > 3 and a[4] is True
    counted = [s for s, m in zip(ids, mask if masked else np.full(n, want)) if m == want]
    true = collections.Counter(counted)
    assert set(a[2]) >= {s for s, c in true.items() if c >= 12}


def test_packed_long_and_empty_ids(pkg, engine):
    """A 17-byte id is skipped by the packed track and turns ``complete`` false;
    it still counts in the table.  An empty id is the empty string in both, as
    in the synchronous packed forms."""
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    ids = [b"a" * 17, b"12345", b"", b"", b"12345", b"b" * 16]
    buf, offs = pkg.pack(ids)
    batch = DeviceBatch.from_host(engine.ctx, buf, offs, np.zeros(len(ids), np.uint32))
    ones = DeviceBuffer(engine.ctx, 32)
    ones.from_host(np.ones(len(ids), np.uint8))
    short = DeviceBatch.from_host(engine.ctx, *pkg.pack(ids[1:]), np.zeros(5, np.uint32))
    try:
        for cid in (20, 21):
            engine.cms_init(cid, 2000, 7)
        engine.hh_init(20, 8)
        engine.hh_init(21, 8)
        engine.cms_add(20, batch, ones, 1)   # ske_cms_add_packed_async
        engine.cms_add(21, batch)            # ske_cms_incrby, the precedent
        engine.sync()
        assert np.array_equal(engine.cms_table(20)[0], engine.cms_table(21)[0])
        assert engine.cms_table(20)[1] == engine.cms_table(21)[1] == 6
        q = engine.cms_query(20, batch)
        assert q.tolist() == [1, 2, 2, 2, 2, 1]
        # without the long id: complete, the empty id listed like any other
        engine.hh_track(21, 20, short, 1, ones, 1)
        engine.sync()
        got = engine.hh_list(21, 20, 1)
        assert (got[0], got[1].tolist(), got[2]) == ([b"", b"12345", b"b" * 16], [2, 2, 1], True)
        assert engine.hh_info(21)["overflow"] == 0
        # with it: skipped, the sticky overflow word set, no error from the call
        engine.hh_track(20, 20, batch, 1, ones, 1)
        engine.sync()
        got = engine.hh_list(20, 20, 1)
        assert (got[0], got[1].tolist(), got[2]) == ([b"", b"12345", b"b" * 16], [2, 2, 1], False)
        assert engine.hh_info(20)["overflow"] != 0 and engine.hh_info(20)["used"] == 3
        engine.hh_reset(20)
        assert engine.hh_list(20, 20, 1)[2] is True
    finally:
        for cid in (20, 21):
            engine.hh_free(cid)
            engine.ctx.call("ske_cms_free", cid)
        for b in (batch, short):
            b.free()
        ones.free()


# ---------------------------------------------------------------- end to end
def stream(seed=5):
    """Two batches of reference-style payloads over a Monday and a Tuesday
    around 09:00, every id five bytes wide (the six-digit invalid pool mapped to
    five-digit ids off the roster), plus host-path and undecodable payloads."""
    roster, msgs = reference_messages(seed=seed, n_students=900, days=2)
    rng = np.random.default_rng(seed)
    off = [int(x) for x in np.setdiff1d(np.arange(10000, 100000), roster)[:4000:80]]
    out = []
    for m in msgs:
        d = json.loads(m)
        if d["student_id"] >= 100000:
            d["student_id"] = off[d["student_id"] % len(off)]
        if rng.random() < 0.2:  # other fast-path forms of the same instant, and a few late / early offsets
            d["timestamp"] = d["timestamp"].replace("T", " ") + (".250", ".000001", "+00:00", "-01:00")[len(out) % 4]
        out.append(json.dumps(d).encode())
    host = [b'{"student_id": "\\u0031\\u0032345", "lecture_id": "LECTURE_20250317", "timestamp": "2025-03-17T09:30:00"}',
            b'{"student_id": 123.5, "lecture_id": "LECTURE_20250318", "timestamp": "2025-03-18T08:15:00"}',
            b'{"student_id": "\\u0031\\u0032345", "lecture_id": "LECTURE_20250318", "timestamp": "2025-03-18T10:00:00.5"}',
            b'{"student_id": %d, "lecture_id": "LECTURE_20250317", "timestamp": "2025-03-17T10:00:00Z"}' % roster[0],
            b'{"lecture_id": "LECTURE_20250317", "timestamp": "2025-03-17T10:00:00", "student_id": 123.5, "x": [1]}']
    junk = [b"not json", b'{"student_id": 1}', b'{"student_id": true, "lecture_id": "L", "timestamp": "2025-03-17"}',
            b'{"student_id": 12345, "lecture_id": "L", "timestamp": "yesterday"}']
    for k, m in enumerate((host + junk) * 3):
        out.insert(int(rng.integers(0, len(out))), m)
    cut = len(out) // 2 + 7
    return roster, [out[:cut], out[cut:]]


def decodable_rows(pkg, batch):
    """(index, id bytes, HLL key, datetime) of the messages the reference's loop
    acknowledges (cassandra_row_types off): json, the three fields, fromisoformat, encode"""
    rows = []
    for i, m in enumerate(batch):
        try:
            d = json.loads(m.decode())
            ts = datetime.fromisoformat(d["timestamp"])
            rows.append((i, pkg.encode(d["student_id"]), "hll:unique:%s:%s" % (d["lecture_id"], ts.date().isoformat())
                         if ts.tzinfo is None else None, ts))
        except Exception:
            pass
    return rows


OPTS = dict(track_attended=3, track_invalid=2, capacity_log2=12, late_key="cms:late", track_late=1, day_profile="week")


def tables_of(client, sc):
    out = {k: client.cms_table(k) for k in (sc.attended_key, sc.invalid_key, sc.late_key)}
    out = {k: (t.copy(), c) for k, (t, c) in out.items()}
    out["profile"] = sc.by_hour_of_week().copy()
    for name, top in (("att", sc.top_attended), ("inv", sc.top_invalid), ("late", sc.top_late)):
        ids, est, complete = top()
        out[name] = (ids, est.tolist(), complete)
    return out


def same_tables(a, b, keys_a, keys_b):
    for ka, kb in zip(keys_a, keys_b):
        assert np.array_equal(a[ka][0], b[kb][0]) and a[ka][1] == b[kb][1], ka
    assert np.array_equal(a["profile"], b["profile"])
    for name in ("att", "inv", "late"):
        assert a[name] == b[name], name


def test_update_messages_end_to_end(pkg, client):
    roster, batches = stream()
    assert sum(len(b) for b in batches) > 2500
    mbuf, moffs = pkg.pack_ints(roster)
    second = pkg.SketchClient(decode_responses=True, device=0)
    try:
        for cl in (client, second):
            cl.execute_command("BF.RESERVE", "bf:students", 0.01, 10000)
            cl.bf_madd_packed("bf:students", mbuf, moffs)
        sc = pkg.StudentCounts(client, **OPTS)
        sc2 = pkg.StudentCounts(second, **OPTS)
        att, inv, late, hist = (collections.Counter() for _ in range(4))
        n_rows = 0
        for batch in batches:
            valid, status = sc.update_messages("bf:students", batch)
            rows = decodable_rows(pkg, batch)
            at = np.asarray([r[0] for r in rows])
            n_rows += len(rows)
            # statuses: -1 exactly the undecodable ones; both other kinds occur
            assert np.array_equal(np.nonzero(status != -1)[0], at)
            assert (status == 0).sum() > 1000 and 1 <= (status == 1).sum() <= 20 and (status == -1).sum() >= 3
            # the same swipes through update(): ids as redis-py encodes them, all five bytes
            ids = np.frombuffer(b"".join(r[1] for r in rows), np.uint8).reshape(len(rows), 5)
            epochs = pkg.epoch_seconds([r[3] for r in rows])
            keys = [r[2] or "hll:unique:aware" for r in rows]
            uniq = {k: second.key_slot(k) for k in sorted(set(keys))}
            v2 = sc2.update("bf:students", np.asarray([uniq[k] for k in keys], np.uint32), ids, epochs)
            assert np.array_equal(valid[at], v2) and not valid[status == -1].any()
            assert 0 < v2.sum() < len(rows)
            for r, v, e in zip(rows, v2, epochs):
                (att if v else inv)[r[1]] += 1
                sod, dow = int(e) % 86400, (int(e) // 86400 + 3) % 7
                late[r[1]] += sod >= 9 * 3600
                hist[dow * 24 + sod // 3600] += 1
        late = +late
        t1, t2 = tables_of(client, sc), tables_of(second, sc2)
        names = (sc.attended_key, sc.invalid_key, sc.late_key)
        same_tables(t1, t2, names, names)
        # the exact histogram, by weekday and hour; nothing from the undecodable messages
        want_hist = np.zeros(168, np.uint64)
        for b, c in hist.items():
            want_hist[b] = c
        assert np.array_equal(t1["profile"].reshape(-1), want_hist)
        assert int(want_hist.sum()) == n_rows == t1[sc.attended_key][1] + t1[sc.invalid_key][1]
        assert set(np.nonzero(t1["profile"].sum(axis=1))[0].tolist()) == {0, 1}  # Monday, Tuesday
        assert t1[sc.late_key][1] == sum(late.values()) and 0 < sum(late.values()) < n_rows
        # every estimate is at least the true count
        for true, query in ((att, sc.attended), (inv, sc.invalid), (late, sc.late)):
            everyone = sorted(true)
            assert (query(everyone) >= np.asarray([true[s] for s in everyone])).all()
        assert b"12345" in inv and b"123.5" in inv  # the host-decoded ids counted
        # where the restatement says the estimates are exact, the lists are the group-bys'
        ins = sc.insights()
        assert ins == sc2.insights()
        assert [i["title"] for i in ins] == ["Habitual Latecomers", "Attendance by Day", "Most Consistent Attendees",
                                             "Invalid Attendance Attempts"]
        by_day = collections.Counter()
        for b, c in hist.items():
            by_day[DAY_NAMES[b // 24]] += c
        assert ins[1]["data"] == dict(by_day)
        for true, entry, thr in ((att, ins[2], 3), (inv, ins[3], 2)):
            assert entry["complete"] and set(entry["data"]) >= {s.decode() for s, c in true.items() if c >= thr}
            rows_of = [s for s, c in true.items() for _ in range(c)]
            if cms_estimates(rows_of) == dict(true):
                assert entry["data"] == {s.decode(): c for s, c in true.items() if c >= thr} and entry["complete"]
                assert len(entry["data"]) > 0
        rows_of = [s for s, c in late.items() for _ in range(c)]
        if cms_estimates(rows_of) == dict(late):
            med = float(np.median(list(late.values())))
            assert ins[0]["data"] == {s.decode(): c for s, c in late.items() if c > med}

        # the same messages through the drop-in processor give the same tables
        keys3 = ("p:att", "p:inv", "p:late")
        sc3 = pkg.StudentCounts(client, keys3[0], keys3[1], late_key=keys3[2], day_profile="p:week",
                                **{k: v for k, v in OPTS.items() if k not in ("late_key", "day_profile")})
        proc = pkg.AttendanceProcessor(client, pkg.AttendanceConfig(cassandra_row_types=False), counts=sc3)
        for batch in batches:
            proc.process_batch(batch)
        assert proc.acked == n_rows
        same_tables(tables_of(client, sc3), t1, keys3, names)
        pins = proc.insights(keys=["hll:unique:LECTURE_20250317:2025-03-17", "hll:unique:LECTURE_20250318:2025-03-18"])
        assert [i["title"] for i in pins] == ["Habitual Latecomers", "Attendance by Day", "Lecture Attendance Rankings",
                                              "Most Consistent Attendees", "Invalid Attendance Attempts"]
        assert [i for i in pins if i["title"] != "Lecture Attendance Rankings"] == ins
        assert all(v > 0 for v in pins[2]["data"]["most_attended"].values())
    finally:
        second.flushall()
