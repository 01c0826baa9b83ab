"""Ingest: batched JSON decode + key-slot resolution on
the device, checked against the reference's per-event loop
(attendance_processor.py:100-137) run in Python over the CPU oracle on the
same payloads -- BF.EXISTS answers, nacks and every HLL register array."""
import ctypes as C
import json
from datetime import datetime, timezone

import numpy as np
import pytest

from test_processor import reference_messages

pytestmark = pytest.mark.gpu

PREFIX = "hll:unique:"


def oracle_loop(orc, chain, messages, key_form="readme"):
    """attendance_processor.py:100-137 with redis-py's argument encoding."""
    from rtsas_amd.encoding import encode
    hlls, valid, nack = {}, [], []
    for m in messages:
        try:
            data = json.loads(bytes(m).decode())
            sid = encode(data["student_id"])
            lecture_id = data["lecture_id"]
            ts = datetime.fromisoformat(data["timestamp"])
            if key_form == "code":
                key = f"{PREFIX}{lecture_id}"
            else:
                if ts.tzinfo is not None:
                    ts = ts.astimezone(timezone.utc)
                key = f"{PREFIX}{lecture_id}:{ts.date().isoformat()}"
        except Exception:
            valid.append(False)
            nack.append(True)
            continue
        v = bool(chain.exists(sid))
        if v:
            hlls.setdefault(key.encode(), orc.HLL()).add(sid)
        valid.append(v)
        nack.append(False)
    return np.array(valid), np.array(nack), hlls


def check_against_oracle(client, orc, chain, msgs, key_form="readme"):
    valid, status = client.ingest("bf:students", msgs, key_form=key_form)
    want_valid, want_nack, hlls = oracle_loop(orc, chain, msgs, key_form)
    assert np.array_equal(valid, want_valid)
    assert np.array_equal(status == -1, want_nack)
    for k, h in hlls.items():
        assert np.array_equal(client.hll_registers(k), h.regs), k
    hll_keys = {k for k, kind in client.keys.kind.items() if kind == "hll"}
    assert hll_keys == set(hlls)
    return status


def preload(client, orc, ids):
    client.execute_command("BF.RESERVE", "bf:students", 0.01, 100000)
    client.execute_command("BF.MADD", "bf:students", *ids)
    chain = orc.Chain(100000, 0.01)
    for i in ids:
        chain.add(str(i).encode())
    return chain


@pytest.mark.parametrize("key_form", ["readme", "code"])
def test_ingest_reference_stream(client, orc, key_form):
    """The reference generator's message stream (data_generator.py:84-185):
    every message decoded on the device, answers and registers exact."""
    valid_ids, msgs = reference_messages(seed=5, n_students=800, days=5)
    chain = preload(client, orc, valid_ids)
    status = check_against_oracle(client, orc, chain, msgs, key_form)
    assert (status == 0).all()


def adversarial_messages(rng, valid_ids):
    good = lambda sid, lec="CS101-L1", ts="2025-03-19T09:15:00": json.dumps(  # noqa: E731
        {"student_id": sid, "timestamp": ts, "lecture_id": lec, "is_valid": True})
    v = lambda: int(rng.choice(valid_ids))  # noqa: E731
    msgs = [
        good(v()), good(v(), ts="2025-03-19"), good(v(), ts="2025-03-19 09:15:00"),
        good(v(), ts="2025-03-19x09:15:00.123"), good(v(), ts="2025-03-19T09:15:00.123456"),
        good(v(), ts="2025-03-19T23:30:00-05:00"), good(v(), ts="2025-03-20T01:30:00+05:30"),
        good(v(), ts="2024-02-29T23:59:59-23:59"), good(v(), ts="2025-01-01T00:00:00+00:00"),
        good(v(), ts="2025-03-19T09:15:00+05:30:00"),      # host (offset seconds)
        good(v(), ts="2025-03-19T09:15"),                   # host (no seconds)
        good(v(), ts="2025-03-19T09:15:00.1234"),           # rejected by fromisoformat: nack
        good(v(), ts="2025-02-29"), good(v(), ts="2025-13-01"), good(v(), ts="2025-03-19T24:00:00"),
        good(v(), ts="2025-03-19T09:15:00Z"), good(v(), ts="0001-01-01T00:10:00+05:30"),
        good(v(), ts="9999-12-31T23:00:00-05:00"),
        good(str(v())), good(v(), lec=7), good(v(), lec="Ünïcode"), good(v(), lec='a"b'),
        good(v(), lec="tab\there"), good(v(), lec=""), good(v(), lec="L:2025"),
        good(float(v())), good(True), good(None), good(-0), good(-5), good([1, 2]),
        good({"x": 1}), good(12345678901234567890), good(v(), lec=["x"]),
        '{"student_id": -0, "lecture_id": "L", "timestamp": "2025-03-19"}',
        '{"student_id": %d, "lecture_id": "L", "timestamp": "2025-03-19T09:15:00", "x": {"y": 1}}' % v(),
        '{"student_id": 1e5, "lecture_id": "L", "timestamp": "2025-03-19"}',
        '{"student_id": NaN, "lecture_id": "L", "timestamp": "2025-03-19"}',
        '{"student_id": %d, "student_id": %d, "lecture_id": "L", "timestamp": "2025-03-19"}' % (999999, v()),
        '  {"student_id" :%d ,"lecture_id":"L","timestamp":"2025-03-19T09:15:00"}\n\t ' % v(),
        '{"student_id": 0123, "lecture_id": "L", "timestamp": "2025-03-19"}',
        '{"student_id": %d, "lecture_id": "L", "timestamp": "2025-03-19",}' % v(),
        '{"lecture_id": "L", "timestamp": "2025-03-19"}',
        '{"student_id": %d, "timestamp": "2025-03-19"}' % v(),
        '{"student_id": %d, "lecture_id": "L"}' % v(),
        '{"student_id": %d, "lecture_id": "L", "timestamp": 20250319}' % v(),
        '[1, 2, 3]', '{}', '', 'not json', '{"student_id": 1', '{"student_id": 1} extra',
        '{"student_id": %d, "lecture_id": "L", "timestamp": "2025-03-19", "ok": true, "no": null,'
        ' "f": false, "n": -12}' % v(),
    ]
    return [m.encode() if isinstance(m, str) else m for m in msgs] + [b"\xff\xfe{}"]


def test_ingest_adversarial_json(client, orc):
    """Escapes, unicode, nested values, floats / bools / null / huge ints as
    ids, duplicate keys, whitespace, missing fields, malformed JSON and every
    timestamp form: decoded on the device when its fast path applies, by
    Python otherwise -- the same answers, nacks and registers either way."""
    rng = np.random.default_rng(6)
    valid_ids = [int(x) for x in rng.choice(np.arange(10000, 100000), 500, replace=False)]
    chain = preload(client, orc, valid_ids)
    msgs = adversarial_messages(rng, valid_ids)
    status = check_against_oracle(client, orc, chain, msgs * 3)
    assert (status == 0).any() and (status == 1).any() and (status == -1).any()


def test_ingest_key_table_lifecycle(client, orc):
    """Keys resolved through the device key table across batches; a key
    deleted between batches is recreated empty (the table is rebuilt)."""
    valid_ids, msgs = reference_messages(seed=7, n_students=300, days=3)
    chain = preload(client, orc, valid_ids)
    half = len(msgs) // 2
    client.ingest("bf:students", msgs[:half])
    client.ingest("bf:students", msgs[half:])
    _, _, hlls = oracle_loop(orc, chain, msgs)
    for k, h in hlls.items():
        assert np.array_equal(client.hll_registers(k), h.regs)
    gone = sorted(hlls)[0]
    client.delete(gone)
    client.ingest("bf:students", msgs[:half])
    _, _, again = oracle_loop(orc, chain, msgs[:half])
    if gone in again:
        assert np.array_equal(client.hll_registers(gone), again[gone].regs)
    for k in set(hlls) - {gone}:
        assert np.array_equal(client.hll_registers(k), hlls[k].regs)


def test_ingest_invalid_only_key_not_created(client, orc):
    """A lecture-day key whose every swipe is invalid is not created (the
    reference only PFADDs valid events)."""
    chain = preload(client, orc, [11111, 22222])
    msgs = [json.dumps({"student_id": 99999, "lecture_id": "EMPTY", "timestamp": "2025-03-19"}).encode(),
            json.dumps({"student_id": 11111, "lecture_id": "FULL", "timestamp": "2025-03-19"}).encode()]
    valid, status = client.ingest("bf:students", msgs)
    assert valid.tolist() == [False, True] and status.tolist() == [0, 0]
    assert client.exists(f"{PREFIX}EMPTY:2025-03-19") == 0
    assert client.exists(f"{PREFIX}FULL:2025-03-19") == 1


# ---------------------------------------------------- key table growth (rehash)
def _lecture_day_messages(rng, keys, valid_ids, per_key=(1, 3)):
    """One or two valid swipes for every (lecture, day) key, shuffled."""
    msgs = []
    for lec, day in keys:
        for _ in range(int(rng.integers(*per_key))):
            ts = f"{day}T{int(rng.integers(8, 18)):02d}:{int(rng.integers(0, 60)):02d}:00"
            msgs.append(json.dumps({"student_id": int(rng.choice(valid_ids)), "timestamp": ts,
                                    "lecture_id": lec, "is_valid": True}).encode())
    return [msgs[i] for i in rng.permutation(len(msgs))]


def test_ingest_key_table_grows_across_batches(client, orc):
    """The device key table starts at 1024 cells and is rehashed into a larger
    one when an insert would fill more than half of it (keytab_grow): batches
    of 400, 300 more and 1500 more distinct lecture-day keys rehash it at the
    second batch (700 keys: 2048 cells) and, two sizes up, at the third (2200:
    8192).  Every batch swipes each of its new keys once or twice, re-swipes
    earlier keys with other valid ids and adds invalid swipes on earlier keys.
    After each batch the answers and nacks, every key's registers and the set
    of HLL keys equal the per-event loop's over the whole stream so far: an
    entry that a rehash lost or misplaced would show as a missing or duplicate
    key, or as registers split over two slots."""
    rng = np.random.default_rng(23)
    valid_ids = [int(x) for x in rng.choice(np.arange(10000, 100000), 3000, replace=False)]
    chain = preload(client, orc, valid_ids)
    days = [f"2025-{m:02d}-{d:02d}" for m in (3, 4, 5) for d in range(1, 29)]
    keys = [(f"LEC{k % 40:02d}-R{k // 3360}", days[(k // 40) % len(days)]) for k in range(2200)]
    assert len(set(keys)) == 2200
    sizes = (400, 300, 1500)
    done, stream = 0, []
    assert sizes[0] <= 512 < sizes[0] + sizes[1] and 2 * sum(sizes[:2]) <= 2048 and 2 * sum(sizes) > 4096
    for b, k in enumerate(sizes):
        batch = _lecture_day_messages(rng, keys[done:done + k], valid_ids)
        if done:
            old = [keys[i] for i in rng.choice(done, min(done, 350), replace=False)]
            batch += _lecture_day_messages(rng, old, valid_ids, per_key=(1, 2))
            batch += _lecture_day_messages(rng, old[:40], [123456, 654321], per_key=(1, 2))  # not members
            batch = [batch[i] for i in rng.permutation(len(batch))]
        done += k
        stream += batch
        valid, status = client.ingest("bf:students", batch)
        want_valid, want_nack, hlls = oracle_loop(orc, chain, stream)
        assert np.array_equal(valid, want_valid[-len(batch):]), f"batch {b}: answers"
        assert not want_nack.any() and (status == 0).all(), f"batch {b}: every message decodes on the device"
        assert len(hlls) == done
        hll_keys = {name for name, kind in client.keys.kind.items() if kind == "hll"}
        assert hll_keys == set(hlls), f"batch {b}: {len(hll_keys)} keys, the oracle has {len(hlls)}"
        slots = [client.keys.slot[name] for name in hlls]
        assert len(set(slots)) == done
        for name, h in hlls.items():
            assert np.array_equal(client.hll_registers(name), h.regs), f"batch {b}: {name}"


def _keytab_hashes(rng):
    """(k0, k1) pairs for the table's hard cases; k0 is odd (0 marks an empty
    cell).  The table indexes by k0 & (cells - 1), cells <= 8192 here."""
    k0, k1 = [], []

    def add(a, b=None):
        k0.append(int(a) | 1)
        k1.append(int(rng.integers(0, 1 << 63)) if b is None else b)

    for low in (0x0A55, 0x1001, 0x0FFD):      # long probe chains at every table size:
        for j in range(1, 41):                # 40 hashes that share their low 13 bits
            add(j << 13 | low)
    for j in range(1, 31):                    # the chain at the table's last cell, which
        add(j << 13 | 0x1FFF)                 # wraps to cell 0 (k0 & mask == cells - 1)
    for j in range(25):                       # equal k0, different k1: a slot each
        a = int(rng.integers(1 << 20, 1 << 62))
        add(a, 1)
        add(a, 2)
    while len(k0) < 2200:                     # and hashes as the parser makes them
        add(rng.integers(0, 1 << 63))
    kh = np.stack([np.array(k0, np.uint64), np.array(k1, np.uint64)], axis=1)
    assert len(np.unique(kh, axis=0)) == len(kh)
    return kh[rng.permutation(len(kh))]


def test_keytab_probe_chains_wrap_and_growth_at_the_abi(engine, pkg):
    """ske_keytab_insert / ske_keytab_lookup over hand-built hash columns:
    clusters of k0 that share their low 13 bits (probe chains of 40 at every
    size of the table), a cluster at the table's last cell (the probe wraps to
    cell 0), pairs with equal k0 and different k1; inserted in three calls of
    400, 300 and 1500 that rehash the table twice.  After every call each
    hash inserted so far resolves to its own slot and every other one --
    never-inserted hashes that run through the same chains, or share a present
    k0 -- misses, with nmiss == their number.  An even k0 is SKE_EINVAL and
    changes nothing; after ske_keytab_clear everything misses."""
    from rtsas_amd._lib import IngestCols, SKE_EINVAL, SketchLibError
    from rtsas_amd.engine import DeviceBuffer
    rng = np.random.default_rng(29)
    ctx = engine.ctx
    kh = _keytab_hashes(rng)
    slots = (7 + 3 * np.arange(len(kh))).astype(np.uint32)
    absent0, absent1 = [], []
    for low in (0x0A55, 0x1001, 0x0FFD, 0x1FFF):  # through the clusters' chains
        for j in range(41, 141):
            absent0.append(j << 13 | low)
            absent1.append(int(rng.integers(0, 1 << 63)))
    for a, b in kh[rng.choice(len(kh), 300, replace=False)]:  # a present k0 with another k1
        absent0.append(int(a))
        absent1.append(int(b) ^ 0x10)
    while len(absent0) < 1000:
        absent0.append(int(rng.integers(0, 1 << 63)) | 1)
        absent1.append(int(rng.integers(0, 1 << 63)))
    absent = np.stack([np.array(absent0, np.uint64), np.array(absent1, np.uint64)], axis=1)
    assert len(np.unique(np.concatenate([kh, absent]), axis=0)) == len(kh) + len(absent)
    probe = np.concatenate([kh, absent])
    order = rng.permutation(len(probe))
    probe = np.ascontiguousarray(probe[order])
    n = len(probe)
    bufs = {"status": DeviceBuffer(ctx, n), "kh": DeviceBuffer(ctx, n * 16), "id_len": DeviceBuffer(ctx, n * 4),
            "slot": DeviceBuffer(ctx, n * 4)}
    bufs["status"].from_host(np.zeros(n, np.uint8))
    bufs["kh"].from_host(probe)
    bufs["id_len"].from_host(np.full(n, 5, np.uint32))
    cols = IngestCols()
    cols.status, cols.kh, cols.id_len = bufs["status"].ptr, bufs["kh"].ptr, bufs["id_len"].ptr

    def lookup():
        nmiss = C.c_uint64(12345)
        ctx.call("ske_keytab_lookup", C.byref(cols), n, C.c_void_p(bufs["slot"].ptr), C.byref(nmiss))
        return bufs["slot"].to_host(np.uint32, n), int(nmiss.value)

    def check(inserted, what):
        want = np.full(len(probe), 0xFFFFFFFF, np.uint32)
        want[:inserted] = slots[:inserted]
        got, nmiss = lookup()
        bad = np.nonzero(got != want[order])[0]
        assert bad.size == 0, f"{what}: {bad.size} wrong slots, e.g. hashes {probe[bad[:4]].tolist()}"
        assert nmiss == len(probe) - inserted, what

    check(0, "empty table")
    done = 0
    for k in (400, 300, 1500):
        part = np.ascontiguousarray(kh[done:done + k])
        ctx.call("ske_keytab_insert", part.ctypes.data_as(C.c_void_p),
                 np.ascontiguousarray(slots[done:done + k]).ctypes.data_as(C.c_void_p), k)
        done += k
        check(done, f"after {done} inserts")
    assert done == len(kh)
    even = np.array([[0x1234567890, 5], [0x77, 6]], np.uint64)
    with pytest.raises(SketchLibError) as e:
        ctx.call("ske_keytab_insert", even.ctypes.data_as(C.c_void_p),
                 np.array([1, 2], np.uint32).ctypes.data_as(C.c_void_p), 2)
    assert e.value.code == SKE_EINVAL
    check(done, "after the refused insert")
    ctx.call("ske_keytab_clear")
    check(0, "after clear")
    ctx.call("ske_keytab_insert", np.ascontiguousarray(kh[:400]).ctypes.data_as(C.c_void_p),
             np.ascontiguousarray(slots[:400]).ctypes.data_as(C.c_void_p), 400)
    check(400, "re-inserted after clear")
    for b in bufs.values():
        b.free()


# -------------------------------------------------------- message alignment
@pytest.mark.parametrize("last", ["corpus", "shortest"])
def test_ingest_every_message_alignment(client, orc, last):
    """The parser reads messages through aligned 8-byte loads that straddle
    message boundaries (Reader::at).  The adversarial corpus and the head of
    the reference stream go through ingest_packed eight times behind a
    nack-able filler of 0..7 bytes, so every message starts at every offset
    mod 8 -- `shortest`: with a two-byte message last in the blob.  Answers,
    statuses, nacks and registers are the same in all eight runs and equal the
    per-event loop's."""
    rng = np.random.default_rng(37)
    valid_ids, ref = reference_messages(seed=9, n_students=150, days=3)
    msgs = adversarial_messages(rng, valid_ids) + ref[:300]
    msgs = [msgs[i] for i in rng.permutation(len(msgs))]
    if last == "shortest":
        msgs.remove(b"{}")
        msgs.append(b"{}")
        assert len(msgs[-1]) == min(len(m) for m in msgs if m)
    chain = orc.Chain(100000, 0.01)
    for i in valid_ids:
        chain.add(str(i).encode())
    want_valid, want_nack, hlls = oracle_loop(orc, chain, msgs)
    assert want_valid.any() and want_nack.any() and len(hlls) > 5
    starts = np.cumsum([0] + [len(m) for m in msgs[:-1]])
    assert len(set((starts % 8).tolist())) == 8
    first = None
    for k in range(8):
        client.flushall()
        preload(client, orc, valid_ids)
        batch = [b"x" * k] + msgs
        blob = np.frombuffer(b"".join(batch), np.uint8)
        moffs = np.zeros(len(batch) + 1, np.uint32)
        np.cumsum([len(m) for m in batch], out=moffs[1:])
        valid, status = client.ingest_packed("bf:students", blob, moffs)
        assert not valid[0] and status[0] == -1, f"filler of {k} bytes"
        assert np.array_equal(valid[1:], want_valid), f"offset {k}: answers"
        assert np.array_equal(status[1:] == -1, want_nack), f"offset {k}: nacks"
        if first is None:
            first = status[1:].copy()
            assert (first == 0).any() and (first == 1).any()
        assert np.array_equal(status[1:], first), f"offset {k}: device / host statuses"
        hll_keys = {name for name, kind in client.keys.kind.items() if kind == "hll"}
        assert hll_keys == set(hlls), f"offset {k}"
        for name, h in hlls.items():
            assert np.array_equal(client.hll_registers(name), h.regs), f"offset {k}: {name}"
