"""The segmented PFADD's arena at its capacity limits (sketch_seg_plan.h sizes
it; tests/native/seg_capacity.cpp proves the sizing on the host): slot
patterns built so that C1's 4-record pads push a sub-batch's chunks past
ceil(sub / 8192) + nb1 rows -- the rows r2 / o2 had per sub-batch before the
pads were counted -- at 512, 256 and 64 level-1 buckets, in every sub-batch
and in the last one of the buffers; a bucket of ~64 chunks against 4 fixed
slots whose reservations straddle chunk boundaries (the owner and waiter
paths of seg_arena_slot); and the seg_b1 option over its range.  Same
harness as test_seg_pfadd.py: C3's one-link filter, 100 000 members, ids
from the device generator, the slot array replaced by hand; every answer
byte and every register of every key bit-exact against the oracle.

The cases marked "pre" first check, with a numpy copy of the host model (C1
reserves roundup4 of every (run, bucket) count; D gives a bucket
ceil(fill / 8192) rows) and the oracle's answers as validity, that the
pattern does need more rows than ceil(sub / 8192) + nb1.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RUN = 8192


def _setup(engine, nkeys, invalid_frac=None):
    from rtsas_amd import synthetic
    w = synthetic.WORKLOADS["c3"]
    over = {"n_members": 100_000, "n_keys": nkeys, "zipf_lectures": 0, "zipf_days": 0}
    if invalid_frac is not None:
        over["invalid_frac"] = invalid_frac
    w = synthetic.Workload(**{**w.__dict__, **over})
    engine.reserve(0, w.bf_error, w.bf_capacity)   # the 19.8 MB C3 geometry (one link, k = 11)
    p = engine.gen_params(w)
    engine.preload(0, p, w.n_members)
    engine.hll_reserve(w.n_keys)
    assert engine.variant(0) == 3
    return w, p


def _model_rows(valid, slot, klog, nb1, nslots):
    """Rows of r2 / o2 D writes for one sub-batch: run r = swipes
    [8192 r, 8192 (r + 1)), bucket h = (slot >> klog) & (nb1 - 1),
    fill_h = sum_r roundup4(c[r][h]), rows = sum_h ceil(fill_h / 8192)."""
    m = len(slot)
    runs = -(-m // RUN)
    ok = valid.astype(bool) & (slot < nslots)
    idx = (np.arange(m, dtype=np.int64) // RUN) * nb1 + ((slot.astype(np.int64) >> klog) & (nb1 - 1))
    c = np.bincount(idx[ok], minlength=runs * nb1).reshape(runs, nb1)
    fill = ((c + 3) & ~3).sum(axis=0)
    return int(((fill + RUN - 1) // RUN).sum())


def _rot_slots(nkeys, klog, b1, n, seed=3):
    """Per full run a quarter of the buckets get 8192 / nb1 - 3 swipes, the
    rest 8192 / nb1 + 1 (counts = 1 mod 4: every reservation pads 3), the
    quarter rotated by run; a bucket's swipes go round robin over its keys;
    the swipes of a run in a fixed shuffled order."""
    nb1 = 1 << b1
    s = np.arange(nkeys, dtype=np.uint32)
    keys_of = s[np.argsort((s >> klog) & (nb1 - 1), kind="stable")].reshape(nb1, nkeys // nb1)
    rng = np.random.default_rng(seed)
    templates = []
    for r in range(4):
        counts = np.where((np.arange(nb1) + r) % 4 == 0, RUN // nb1 - 3, RUN // nb1 + 1)
        assert counts.sum() == RUN
        bucket = np.repeat(np.arange(nb1), counts)
        j = np.arange(RUN) - np.repeat(np.cumsum(counts) - counts, counts)
        templates.append(keys_of[bucket, j % keys_of.shape[1]][rng.permutation(RUN)])
    runs = -(-n // RUN)
    return np.stack(templates)[np.arange(runs) % 4].reshape(-1)[:n].astype(np.uint32)


def _straddle_slots(n):
    """Run 0: 4096 swipes to key 0 and 8 to each of the 512 keys; later runs:
    8188 to key 0 and one each to keys 1-4."""
    assert n % RUN == 0
    run0 = np.concatenate([np.zeros(4096, np.uint32), np.repeat(np.arange(512, dtype=np.uint32), 8)])
    later = np.concatenate([np.zeros(8188, np.uint32), np.arange(1, 5, dtype=np.uint32)])
    rng = np.random.default_rng(11)
    out = np.tile(later[rng.permutation(RUN)], n // RUN)
    out[:RUN] = run0[rng.permutation(RUN)]
    return out


def _run(engine, orc, w, p, n, slots, klog, b1, sub, pre, all_valid):
    from rtsas_amd.engine import DeviceBatch, DeviceBuffer
    assert slots.size == n and int(slots.max()) < w.n_keys
    g = engine.swipe_batch(p, 0, n)
    buf, offs, _ = g.to_host()
    g.free()
    chain = orc.Chain(w.bf_capacity, w.bf_error)
    mb = engine.members_batch(p, 0, w.n_members)
    mbuf, moffs, _ = mb.to_host()
    mb.free()
    chain.madd_packed(mbuf, moffs)
    regs = np.zeros((w.n_keys, 16384), np.uint8)
    answers, _, _ = orc.process_swipes(chain, regs, slots, buf, offs, threads=8)
    assert answers.any() and regs.any(axis=1).all()  # every key got a record
    if all_valid:
        assert answers.all()
    if pre:  # the pattern is adversarial: every sub-batch needs more rows than the unpadded count gives
        assert n % sub == 0 and sub % RUN == 0
        for s0 in range(0, n, sub):
            rows = _model_rows(answers[s0:s0 + sub], slots[s0:s0 + sub], klog, 1 << b1, w.n_keys)
            assert rows > sub // RUN + (1 << b1), (rows, sub // RUN + (1 << b1))
    engine.set_option("hll_seg", 1)
    engine.set_option("seg_klog", klog)
    engine.set_option("seg_b1", b1)
    engine.set_option("part_sub", sub)
    engine.set_option("pass_timing", 1)
    engine.pass_times(reset=True)
    b = DeviceBatch.from_host(engine.ctx, buf, offs, slots)
    out = DeviceBuffer(engine.ctx, n)
    engine.swipes(0, b, out)
    assert engine.pass_times(reset=True)[5][1] > 0  # the window pass ran: the segmented form
    engine.set_option("pass_timing", 0)
    assert np.array_equal(out.to_host(np.uint8, n), answers)
    assert np.array_equal(engine.registers_all(w.n_keys), regs)


SUB512 = 432 * RUN  # 3 538 944


@pytest.mark.parametrize("case", ["rot512", "rot256", "rot64", "uniform512", "ragged", "mixed", "straddle"])
def test_seg_capacity(engine, orc, case):
    """rot512 / rot256 / rot64 (pre): the rotated pattern at 512, 256 and 64
    buckets, 2 or 3 sub-batches, each needing 1024 / 512 / 192 rows against
    944 / 491 / 190 unpadded.  uniform512 (pre): uniform random keys, every
    swipe valid, one sub-batch (its rows are the last of the buffers), ~1020
    rows against 992.  ragged: rot512 repeated over 2 x sub + 5000 swipes,
    which the library re-splits into three even sub-batches.  mixed: rot512's
    slots under the default 10 % invalid ids, so padded and unpadded runs
    alternate.  straddle: bucket 0 holds ~64 chunks against kstat = 4, nearly
    every reservation straddles a chunk boundary, window 0 is cut into ~16
    slices."""
    if case == "rot512":
        nkeys, klog, b1, sub, n, inv, pre = 512, 0, 9, SUB512, 2 * SUB512, 0.0, True
    elif case == "rot256":
        nkeys, klog, b1, sub, n, inv, pre = 1024, 1, 8, 235 * RUN, 2 * 235 * RUN, 0.0, True
    elif case == "rot64":
        nkeys, klog, b1, sub, n, inv, pre = 2048, 3, 6, 126 * RUN, 3 * 126 * RUN, 0.0, True
    elif case == "uniform512":
        nkeys, klog, b1, sub, n, inv, pre = 512, 0, 9, 480 * RUN, 480 * RUN, 0.0, True
    elif case == "ragged":
        nkeys, klog, b1, sub, n, inv, pre = 512, 0, 9, SUB512, 2 * SUB512 + 5000, 0.0, False
    elif case == "mixed":
        nkeys, klog, b1, sub, n, inv, pre = 512, 0, 9, SUB512, 2 * SUB512, None, False
    else:
        nkeys, klog, b1, sub, n, inv, pre = 512, 0, 9, 64 * RUN, 64 * RUN, 0.0, False
    if case == "uniform512":
        slots = np.random.default_rng(1).integers(0, 512, n).astype(np.uint32)
    elif case == "straddle":
        slots = _straddle_slots(n)
    else:
        slots = _rot_slots(nkeys, klog, b1, n)
    w, p = _setup(engine, nkeys, inv)
    _run(engine, orc, w, p, n, slots, klog, b1, sub, pre, all_valid=inv == 0.0)


@pytest.fixture(scope="module")
def b1_ref():
    return {}


@pytest.mark.parametrize("klog,b1,seg", [(0, 9, True), (0, 4, True), (3, 1, True), (3, 9, True), (0, 3, False)])
def test_seg_b1_option(engine, orc, b1_ref, klog, b1, seg):
    """seg_b1 over its range on 5000 uniform keys: 512 buckets of 16 windows,
    16 of 512, 2 of 512 (625 windows of 8 keys), 512 of 2; and 8 buckets, which
    would need 2^10 windows per bucket: the plan refuses and pass C must give
    the same answers and registers."""
    from rtsas_amd.engine import DeviceBuffer
    w, p = _setup(engine, 5000)
    n = 700_001
    b = engine.swipe_batch(p, 0, n)
    if not b1_ref:  # one reference for the five cases (same workload, same batch)
        buf, offs, slot = b.to_host()
        chain = orc.Chain(w.bf_capacity, w.bf_error)
        mb = engine.members_batch(p, 0, w.n_members)
        mbuf, moffs, _ = mb.to_host()
        mb.free()
        chain.madd_packed(mbuf, moffs)
        regs = np.zeros((w.n_keys, 16384), np.uint8)
        answers, _, _ = orc.process_swipes(chain, regs, slot.astype(np.uint32), buf, offs)
        regs.setflags(write=False)
        answers.setflags(write=False)
        b1_ref.update(regs=regs, answers=answers)
    engine.set_option("hll_seg", 1)
    engine.set_option("seg_klog", klog)
    engine.set_option("seg_b1", b1)
    engine.set_option("pass_timing", 1)
    engine.pass_times(reset=True)
    out = DeviceBuffer(engine.ctx, n)
    engine.swipes(0, b, out)
    pt = engine.pass_times(reset=True)
    engine.set_option("pass_timing", 0)
    assert (pt[5][1] > 0) == seg
    assert np.array_equal(out.to_host(np.uint8, n), b1_ref["answers"])
    assert np.array_equal(engine.registers_all(w.n_keys), b1_ref["regs"])
