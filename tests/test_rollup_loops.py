"""K2 / K3 past their grids, at small shapes.

The rollup kernels (csrc/sketch_kernels.hip) cap their grids by the device's
compute-unit count CU, so a wave's second batch of keys, a block's second
group and a PFMERGE partition of more than 16 sources otherwise run only at
C5 / bench scale (tests/test_c5_rollup.py's 30 GB slab).  Slot and source
lists may repeat slots and PFCOUNT / max-merge are well defined on repeats, so
a long *list* over a 64-row slab reaches the same paths:

- k_pfcount_wave (2*CU blocks x 4 waves, 8 keys per batch): lists of 64*CU,
  64*CU + 1, 72*CU + 5 and 128*CU + 3 keys -- a full batch that ends with the
  input, a ninth key, a full batch + tail, two full batches + tail;
- k_pfcount (min(ngroups, 8*CU) blocks): 16*CU + 3 groups;
- k_merge_groups (min(ngroups, 4*CU) groups per pass): 4*CU + 3 groups;
  group sizes cycle through 0, 1, 7, 8, 9, 16, 17 (both sides of max_keys'
  8-way unrolled body, empty groups in every pass);
- k_pfmerge_part / k_pfmerge_rows: 257 sources (per = 16, a last partition of
  one) and the first n above 64*CU with per > 16 and a short last partition.

Every comparison is bit-exact: counts against the oracle's hllCount on the
same registers, merged rows against numpy / torch maxima.  The preconditions
that make a misplaced count or a dropped source visible are asserted on the
reference alone (distinct counts of the 64 rows; every source the strict
unique maximum of some register)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 16384          # registers per key
R = 64             # rows of the small slab
SIZES = (0, 1, 7, 8, 9, 16, 17)  # group sizes: max_keys' unrolled body is 8 wide
N_SPECIAL = 3      # rows 0..2: all zero, all 51, half 51 / half 1
N_FILL = 11        # rows 3..13: the estimator's fills, empty to saturated


def _cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _make_rows(orc):
    """64 register rows with pairwise distinct PFCOUNTs: a count written to
    the wrong output index is then a wrong count.  Rows N_SPECIAL + N_FILL..63
    are the `mergeable` ones: geometric values at varied densities, where no
    row dominates another in a max."""
    rng = np.random.default_rng(31)
    rows, counts = [], set()

    def take(make):
        for _ in range(100):
            r = make().astype(np.uint8)
            c = orc.hll_count_regs(r)
            if c not in counts:
                counts.add(c)
                rows.append(r)
                return
        raise AssertionError("no row with a new count")

    take(lambda: np.zeros(M))
    take(lambda: np.full(M, 51))
    take(lambda: np.where(rng.random(M) < 0.5, 51, 1))

    def fill_row(fill):  # as test_pfcount_estimator_exact
        n_per = fill / float(M)
        u = rng.random(M)
        r = np.ceil(-np.log2(1 - u ** (1.0 / max(n_per, 1e-12)))).clip(0, 51)
        if fill < M:
            r[rng.random(M) > fill / float(M)] = 0
        return r

    fills = [30, 300, 3000, 30000, 10**5, 3 * 10**5, 3 * 10**6, 3 * 10**7, 3 * 10**8, 10**10, 10**12]
    assert len(fills) == N_FILL
    for fill in fills:
        take(lambda: fill_row(fill))

    def dens_row():  # as test_pfcount_each_many_keys_vs_oracle
        dens = rng.choice([0.02, 0.1, 0.3, 0.5, 0.9, 1.0])
        vals = rng.geometric(0.5, M).clip(1, 51)
        return np.where(rng.random(M) < dens, vals, 0)

    while len(rows) < R:
        take(dens_row)
    rows = np.stack(rows)
    want = np.array([orc.hll_count_regs(r) for r in rows], np.uint64)
    assert len(set(want.tolist())) == R, "the 64 rows need pairwise distinct counts"
    return rows, want


@pytest.fixture(scope="module")
def slab64(orc):
    return _make_rows(orc)


def _load(engine, rows):
    engine.hll_reserve(len(rows))
    for s, r in enumerate(rows):
        engine.ctx.call("ske_hll_import_raw", s, _ptr(r))


# ------------------------------------------------------------ K2, wave per key
def _k2_sizes(cu):
    return {"full": 64 * cu, "ninth": 64 * cu + 1, "full+tail": 72 * cu + 5, "two-full+tail": 128 * cu + 3}


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
@pytest.mark.parametrize("shape", ["full", "ninth", "full+tail", "two-full+tail"])
def test_pfcount_wave_full_batches(engine, slab64, shape, mem):
    """k_pfcount_wave: its 2*CU x 4 waves see 8 keys each from 64*CU keys on.
    `full`: every wave bins exactly 8, the flush and the end of the input
    coincide; `ninth`: one wave gets a ninth key; `full+tail`: a full batch,
    then a batch of one or two; `two-full+tail`: two full batches on one wave
    (the running-total columns and `prev` carry across them), then a tail.
    Every count of the list == the oracle's for that slot's row."""
    import torch
    rows, want = slab64
    cu = _cu()
    n = _k2_sizes(cu)[shape]
    waves = 2 * cu * 4
    assert n >= 8 * waves and (shape != "two-full+tail" or n > 16 * waves)
    _load(engine, rows)
    slots = np.random.default_rng(n).integers(0, R, n).astype(np.uint32)
    if mem == 0:
        out = np.zeros(n, np.uint64)
        engine.ctx.call("ske_hll_pfcount_each", _ptr(slots), n, _ptr(out), 0)
    else:
        ds = torch.from_numpy(slots.view(np.int32)).cuda()
        do = torch.zeros(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engine.ctx.call("ske_hll_pfcount_each", C.c_void_p(ds.data_ptr()), n, C.c_void_p(do.data_ptr()), 1)
        out = do.cpu().numpy().view(np.uint64)
    bad = np.nonzero(out != want[slots])[0]
    assert bad.size == 0, f"{bad.size} wrong counts, first at list index {bad[:8].tolist()}"


def test_pfcount_wave_raw_rows_full_batch(engine, slab64):
    """The same batching with the null slot list (ske_hll_count_raw_dev): a
    device buffer of 72*CU + 5 raw rows gathered from the 64."""
    import torch
    rows, want = slab64
    cu = _cu()
    n = 72 * cu + 5
    pick = np.random.default_rng(5).integers(0, R, n)
    regs = torch.from_numpy(rows).cuda()[torch.from_numpy(pick).cuda()].contiguous()
    assert regs.shape == (n, M)
    torch.cuda.synchronize()
    out = np.zeros(n, np.uint64)
    engine.ctx.call("ske_hll_count_raw_dev", C.c_void_p(regs.data_ptr()), n, _ptr(out))
    bad = np.nonzero(out != want[pick])[0]
    assert bad.size == 0, f"{bad.size} wrong counts, first at row {bad[:8].tolist()}"


# ------------------------------------------------- K2 / K3 over groups of slots
_GROUPS = {}  # (ngroups, seed) -> the lists and their reference, built once


def _groups(rows, ngroups, seed, shift=0):
    if (ngroups, seed, shift) not in _GROUPS:
        _GROUPS[ngroups, seed, shift] = _build_groups(rows, ngroups, seed, shift)
    return _GROUPS[ngroups, seed, shift]


def _build_groups(rows, ngroups, seed, shift):
    """Group g has SIZES[(g + shift) % 7] slots.  Two groups in three draw distinct
    mergeable rows and must be sensitive to every member: each member is the
    strict unique maximum of some register of its group, so a source that
    max_keys drops changes the group's row.  Every third group draws from all
    64 rows with repeats (dominating and empty rows, repeated slots).
    Returns (slots, goffs, the per-group maxima)."""
    rng = np.random.default_rng(seed)
    first = N_SPECIAL + N_FILL
    lists, maxima = [], np.zeros((ngroups, M), np.uint8)
    cols = np.arange(M)
    for g in range(ngroups):
        k = SIZES[(g + shift) % len(SIZES)]
        if g % 3 == 0:
            idx = rng.integers(0, R, k)
        else:
            idx = first + rng.choice(R - first, k, replace=False)
        lists.append(idx)
        if k == 0:
            continue
        G = rows[idx]
        m1 = G.max(axis=0)
        maxima[g] = m1
        if g % 3 != 0:
            am = G.argmax(axis=0)
            G[am, cols] = 0
            strict = m1 > G.max(axis=0)
            assert (np.bincount(am[strict], minlength=k) > 0).all(), f"group {g} hides a source"
    sizes = np.array([len(i) for i in lists])
    goffs = np.zeros(ngroups + 1, np.uint32)
    np.cumsum(sizes, out=goffs[1:])
    slots = np.concatenate(lists).astype(np.uint32)
    return slots, goffs, maxima


@pytest.mark.parametrize("mem", [0, 1], ids=["host", "device"])
def test_pfcount_groups_grid_stride(engine, orc, slab64, mem):
    """k_pfcount over 16*CU + 3 groups on a grid of 8*CU blocks: every block
    runs a second group (some a third) over the LDS histogram it re-zeroes,
    with empty groups in every pass.  Count == the oracle's on the numpy max
    of the group's rows, 0 for an empty group."""
    import torch
    rows, _ = slab64
    cu = _cu()
    ngroups = 16 * cu + 3
    assert ngroups > 2 * 8 * cu
    slots, goffs, maxima = _groups(rows, ngroups, 41)
    sizes = np.diff(goffs.astype(np.int64))
    assert (sizes[:8 * cu] == 0).any() and (sizes[8 * cu:] == 0).any()
    want = np.array([orc.hll_count_regs(m) if k else 0 for m, k in zip(maxima, sizes)], np.uint64)
    _load(engine, rows)
    if mem == 0:
        out = np.full(ngroups, 7, np.uint64)
        engine.ctx.call("ske_hll_pfcount_groups", _ptr(slots), _ptr(goffs), ngroups, _ptr(out), 0)
    else:
        ds = torch.from_numpy(slots.view(np.int32)).cuda()
        dg = torch.from_numpy(goffs.view(np.int32)).cuda()
        do = torch.full((ngroups,), 7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        engine.ctx.call("ske_hll_pfcount_groups", C.c_void_p(ds.data_ptr()), C.c_void_p(dg.data_ptr()), ngroups,
                        C.c_void_p(do.data_ptr()), 1)
        out = do.cpu().numpy().view(np.uint64)
    bad = np.nonzero(out != want)[0]
    assert bad.size == 0, f"{bad.size} wrong counts, first at groups {bad[:8].tolist()} (sizes {sizes[bad[:8]].tolist()})"


def test_merge_groups_grid_stride(engine, slab64):
    """k_merge_groups over 4*CU + 3 groups (4*CU per pass): the last three are
    a block's second iteration; rows == the numpy maxima, zeros for an empty
    group (the buffer starts non-zero)."""
    import torch
    rows, _ = slab64
    cu = _cu()
    ngroups = 4 * cu + 3
    # the cycle starts so that the second pass (groups 4*CU..) holds sizes 17, 0, 1
    slots, goffs, maxima = _groups(rows, ngroups, 43, shift=-(4 * cu + 1) % len(SIZES))
    sizes = np.diff(goffs.astype(np.int64))
    assert (sizes[:4 * cu] == 0).any() and sizes[4 * cu:].tolist() == [17, 0, 1]
    _load(engine, rows)
    dst = torch.full((ngroups, M), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.ctx.call("ske_hll_merge_groups_dev", _ptr(slots), _ptr(goffs), ngroups, C.c_void_p(dst.data_ptr()))
    got = dst.cpu().numpy()
    bad = np.nonzero((got != maxima).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} wrong rows, first at groups {bad[:8].tolist()} (sizes {sizes[bad[:8]].tolist()})"


# ------------------------------------------------------------- wide PFMERGE
def _partitions(n, cu):
    """pfmerge_partitions (csrc/sketch_kernels.hip): sources per partition, partitions."""
    per = max(16, -(-n // (4 * cu)))
    return per, -(-n // per)


def _slab_view(engine, nrows):
    import torch
    ptr, nbytes = C.c_void_p(), C.c_uint64()
    engine.ctx.call("ske_hll_slab", C.byref(ptr), C.byref(nbytes))
    assert nbytes.value >= nrows * M

    class _Slab:  # zero-copy device view of the slab's first nrows keys
        __cuda_array_interface__ = {"shape": (nrows, M), "typestr": "|u1", "data": (ptr.value, False),
                                    "version": 3, "strides": None}
    return torch.as_tensor(_Slab(), device="cuda")


BG_MAX, MARK, MARK_HI, DST_HI = 20, 40, 50, 51


def _wide_merge(engine, n):
    """PFMERGE of n distinct sparse rows (slots 0..n-1, listed in a shuffled
    order) into slot n, which holds registers of its own.

    A max over thousands of sources hides a dropped one unless it alone holds
    some register's maximum.  Row i < 16384 carries marker MARK (above every
    background value) at register i; rows past 16384 cannot have a register
    of their own, so they carry MARK_HI at a borrowed register -- which hides
    that register's own row -- and the destination holds DST_HI at another.
    Two arrangements borrow different registers: every list position must be
    the strict unique maximum of some register in at least one of them
    (asserted on the reference alone)."""
    import torch
    engine.hll_reserve(n + 1)
    slab = _slab_view(engine, n + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    for r0 in range(0, n, 4096):  # background: ~10 % of the registers, values 1..BG_MAX
        r1 = min(n, r0 + 4096)
        bg = torch.randint(0, 256, (r1 - r0, M), dtype=torch.uint8, device="cuda", generator=g)
        slab[r0:r1] = torch.where(bg < 26, 1 + bg % BG_MAX, torch.zeros_like(bg))
    base = min(n, M)
    own = torch.arange(base, device="cuda")
    slab[own, own] = MARK
    extra = n - base  # rows without a register of their own
    rng = np.random.default_rng(n)
    borrowed = rng.choice(base, 2 * (extra + 1), replace=False).reshape(2, extra + 1)
    dst_own = rng.integers(0, 3, M).astype(np.uint8)
    cols = torch.arange(M, device="cuda")
    covered = torch.zeros(n, dtype=torch.bool, device="cuda")  # by list position
    srcs = rng.permutation(n).astype(np.uint32)
    dsrcs = torch.from_numpy(srcs.view(np.int32)).cuda()
    for arr in range(2):
        if extra:
            slab[base:n] = torch.where(slab[base:n] >= MARK, torch.zeros_like(slab[base:n]), slab[base:n])
            slab[torch.arange(base, n, device="cuda"), torch.from_numpy(borrowed[arr, :extra]).cuda()] = MARK_HI
        prior = dst_own.copy()
        prior[borrowed[arr, extra]] = DST_HI
        dprior = torch.from_numpy(prior).cuda()
        # the reference: torch.amax over the listed rows and the destination's own registers
        listed = torch.cat([slab[:n][dsrcs.long()], dprior[None]])
        m1, am = listed.max(dim=0)
        want = torch.maximum(torch.amax(slab[:n], dim=0), dprior)
        assert torch.equal(m1, want)
        listed[am, cols] = 0
        strict = m1 > listed.amax(dim=0)
        winners = am[strict]
        covered[winners[winners < n]] = True  # (index n is the destination's own row)
        del listed
        for form in ("ske_hll_pfmerge", "ske_hll_pfmerge_dev"):
            slab[n] = dprior
            torch.cuda.synchronize()
            if form == "ske_hll_pfmerge":
                engine.ctx.call(form, n, _ptr(srcs), n)
            else:
                engine.ctx.call(form, n, C.c_void_p(dsrcs.data_ptr()), n)
            bad = torch.nonzero(slab[n] != want).flatten()
            assert bad.numel() == 0, (f"{form}, arrangement {arr}: {bad.numel()} wrong registers, first "
                                      f"{bad[:8].tolist()}: got {slab[n][bad[:8]].tolist()}, want {want[bad[:8]].tolist()}")
    assert bool(covered.all()), f"{int((~covered).sum())} sources are never a strict unique maximum"


def test_pfmerge_257_sources(engine):
    """The smallest two-level merge: per = 16, 17 partitions, the last of one source."""
    cu = _cu()
    per, P = _partitions(257, cu)
    assert (per, P) == (16, 17) and 257 - (P - 1) * per == 1
    _wide_merge(engine, 257)


def test_pfmerge_partitions_above_16(engine):
    """The first n above 64*CU whose partitions hold more than 16 sources with
    a short last one (otherwise only C5's 1.8M-key campus merge has per > 16)."""
    cu = _cu()
    n = next(n for n in range(64 * cu + 1, 68 * cu) if n % _partitions(n, cu)[0])
    per, P = _partitions(n, cu)
    last = n - (P - 1) * per
    assert per > 16 and P <= 4 * cu and 0 < last < per
    _wide_merge(engine, n)
