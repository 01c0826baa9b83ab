"""tests/chain_shapes.py on the CPU: the inputs of every row of
tests/test_chain_shapes.py meet their three conditions on the oracle (every
member valid, 20..80 % of the items valid, every link alone passes at most half
of the non-members); an assembled chain answers as the OR of its links; its
probe count is SBChain_Check's, restated here in Python; and the K1 dispatch
restated in chain_shapes.py rests on the constants csrc/ holds and puts every
row on the arm its name says."""
import numpy as np
import pytest

import chain_shapes as cs


def _ids(it):
    return [it.buf[it.offs[i]:it.offs[i + 1]].tobytes() for i in range(it.n)]


def test_constants_are_those_of_csrc():
    """A retune of any of these moves rows off their arms: restate chain_shapes.plan and the rows with it."""
    want = {k: getattr(cs, k) for k in cs.csrc_constants()}
    assert cs.csrc_constants() == want
    assert len(want) == 13


@pytest.mark.parametrize("row", cs.ROWS, ids=lambda r: r.name)
def test_row_lands_on_its_arm(row):
    assert cs.plan(row.specs, row.variant)[1] == row.arm


def test_plan_boundaries():
    """The arithmetic next to the rows: pieces and P, slices and km, KB."""
    by = cs._by
    assert [cs.lds_pieces(cs.ROW[f"lds-a{P}"].specs) for P in range(1, 11)] == [16 * (P - 1) + 1 for P in range(1, 11)]
    assert [cs.lds_pieces(cs.ROW[f"lds-b{P}"].specs) for P in (1, 5, 9)] == [16, 80, 144]
    assert cs.lds_pieces(by([160 * 1024], [7])) is None  # 10 full rounds do not fit the image
    assert cs.lds_pieces(cs.ROW["lds-c"].specs) == 152
    assert cs.lds_pieces(cs.ROW_E) == 1 + 2 + 3 + 1 + 5 + 1 + 1 + 30
    assert cs.lds_pieces(cs.ROW_F) == 69 + 61 and cs.lds_pieces(by([70000, 60000], [9, 8])) == 128
    assert cs.lds_pieces(cs.ROW["lds-g"].specs) == 120
    assert cs.lds_pieces(by([18440] * 8, range(7, 15))) == 152  # still accepted: P = 10
    sp = cs.ROW["legacy-pieces"].specs
    assert sum(cs._pad16(b) for b, _ in sp) == 148608 <= cs.LDS_MAX and cs.lds_pieces(sp) is None
    assert cs.plan(cs.ROW["lds-d"].specs, -1) == (0, "global")
    assert cs.plan(cs.ROW["global-48links"].specs, -1) == (0, "global")
    assert cs.plan(cs.ROW["global-cursor64"].specs, -1) == (0, "global")
    assert cs.plan(cs.ROW["xr-grown"].specs, -1) == (2, "xr KB=10") and cs.part_slices(cs.ROW["xr-grown"].specs) is None
    assert cs.part_slices(by([1 << 28], [11])) is None and cs.part_slices(by([(1 << 28) - 64 * 1024 * 2049], [11]))
    assert cs.part_slices(cs.ROW["part-11"].specs) == (11, 1)
    assert cs.part_slices(cs.ROW["part-5-6"].specs) == (11, 3)
    assert cs.part_slices(cs.ROW["part-12"].specs) == (22, 2)
    assert cs.part_slices(cs.ROW["part-4-4-4"].specs) == (22, 3 + 1 + 1)
    assert cs.part_slices(cs.ROW["part-7-7-8"].specs) == (22, 1 + 2 + 3)
    assert cs.part_slices(cs.ROW["part-8links"].specs) == (22, 1 + 1 + 1 + 2 + 1 + 3 + 1 + 1)
    assert cs.part_slices(cs.ROW["part-23"].specs) is None
    for r in cs.ROWS:  # every small row under no forced variant: the LDS image, fast where the plan takes it
        small = sum(cs._pad16(b) for b, _ in r.specs) <= cs.LDS_MAX
        assert (cs.plan(r.specs, -1)[0] == 1) == small
        assert (cs.plan(r.specs, -1)[1] == "legacy") == (small and cs.lds_pieces(r.specs) is None)


def _n_host(n):
    return (2 + 1) * 512 + 3 if n == "cu" else n  # (the GPU test takes the device's CU count)


@pytest.mark.parametrize("row", cs.ROWS, ids=lambda r: r.name)
def test_row_inputs(orc, row):
    ch = cs.make_chain(orc, row.specs, row.seed)
    for j, n in enumerate(row.ns):
        n = _n_host(n)
        it = cs.make_items(ch, np.random.default_rng(row.seed * 16 + j), n)
        cs.check_inputs(orc, ch, it, strict=n >= 4000)
        if n >= 6144:
            assert min(np.bincount(it.link[it.link >= 0], minlength=len(row.specs))) >= 64
            lens = np.diff(it.offs.astype(np.int64)).reshape(-1, 64)
            short = (lens <= 8).all(axis=1)
            assert short[3::4].all() and not short.reshape(-1, 4)[:, :3].any()
            assert {0, 1, 8, 9, 40} <= set(lens.ravel().tolist())


def test_fixed_width_and_many_batches_inputs(orc):
    """Rows h and i of the LDS fast path: lds-f with 8-byte ids at a tile-ragged n, and the five batches."""
    ch = cs.make_chain(orc, cs.ROW_F, 77, width=8)
    it = cs.make_items(ch, np.random.default_rng(78), (2 * 4 + 1) * 1024 + 17, width=8)
    assert (np.diff(it.offs.astype(np.int64)) == 8).all()
    cs.check_inputs(orc, ch, it)
    for specs in (cs.ROW_E, cs.ROW_F):
        ch = cs.make_chain(orc, specs, 79)
        for j, n in enumerate((1, 1023, 4096, 4097, 9000)):
            cs.check_inputs(orc, ch, cs.make_items(ch, np.random.default_rng(80 + j), n), strict=n >= 4000)


@pytest.mark.parametrize("specs", [cs.ROW_E, [(72, 5), (64, 1), (1024, 31), (1 << 20, 17), (8, 3), (1245184, 64)]],
                         ids=["row-e", "six-links"])
def test_assembled_chain_is_the_or_of_its_links(orc, specs):
    ch = cs.make_chain(orc, specs, 5)
    it = cs.make_items(ch, np.random.default_rng(6), 6144)
    got, _ = ch.chain.mexists_packed(it.buf, it.offs)
    each = [one.mexists_packed(it.buf, it.offs)[0] for one in ch.singles]
    assert np.array_equal(got, np.bitwise_or.reduce(each))
    assert ch.chain.nlinks == len(specs)
    for l, (bits, k) in enumerate(specs):
        info = ch.chain.link_info(l)
        assert (info["bits"], info["hashes"], info["bytes"]) == (bits, k, bits // 8)
        assert np.array_equal(ch.chain.link_bits(l), ch.singles[l].link_bits(0))


@pytest.mark.parametrize("specs", [[(72, 5), (64, 1), (8, 3)], [(1024, 31), (4096, 2)]], ids=["tiny", "small"])
def test_probe_count_is_sbchain_check(orc, specs):
    """SBChain_Check restated: links newest first, each link's probes
    (a + i b) mod 2^64 mod bits for i < hashes, stopping at the first unset bit;
    the first link that has every bit set answers."""
    ch = cs.make_chain(orc, specs, 9)
    it = cs.make_items(ch, np.random.default_rng(10), 512)
    bits = [np.unpackbits(ch.chain.link_bits(l), bitorder="little") for l in range(len(specs))]
    probes, answers = 0, []
    for x in _ids(it):
        a = orc.murmur64a(x, 0xC6A4A7935BD1E995)
        b = orc.murmur64a(x, a)
        hit = False
        for l in reversed(range(len(specs))):
            d, k = specs[l]
            ok = True
            for i in range(k):
                probes += 1
                if not bits[l][((a + i * b) & (2 ** 64 - 1)) % d]:
                    ok = False
                    break
            if ok:
                hit = True
                break
        answers.append(hit)
    got, n = ch.chain.mexists_packed(it.buf, it.offs)
    assert got.astype(bool).tolist() == answers and n == probes


@pytest.mark.parametrize("name", ["lds-e", "xr-k8", "xr-k17", "part-7-7-8", "global-48links"])
def test_near_members_miss_by_one_probe(orc, name):
    """On its own link, a near member whose missing bit is its last probe's is
    walked through every probe, and that probe alone decides: a kernel that
    drops it answers valid where the oracle (nearly always) does not.  With the
    bit set, it is a member."""
    ch = cs.make_chain(orc, cs.ROW[name].specs, 13)
    seen = valid = 0
    for l, (bits, k) in enumerate(ch.specs):
        if ch.near[l] is None:
            assert k == 1
            continue
        buf, offs, drop = ch.near[l]
        last = np.flatnonzero(drop == k - 1)
        ids = [buf[offs[i]:offs[i + 1]].tobytes() for i in last]
        b, o = orc.pack(ids)
        got, probes = ch.singles[l].mexists_packed(b, o)
        assert probes == k * len(ids)
        if bits >= 4096:
            seen += len(ids)
            valid += int(got.sum())
        one = orc.Chain.loadchunks([(1, cs.pack_header([ch.links[l]])), (1 + bits // 8, ch.singles[l].link_bits(0).tobytes())])
        for x in ids:
            a = orc.murmur64a(x, cs.BLOOM_SEED)
            at = ((a + (k - 1) * orc.murmur64a(x, a)) & (2 ** 64 - 1)) % bits
            bf = one.link_bits(0)
            bf[at >> 3] |= 1 << (at & 7)
            two = orc.Chain.loadchunks([(1, cs.pack_header([ch.links[l]])), (1 + bits // 8, bf.tobytes())])
            assert two.exists(x)
    assert seen >= 8 and valid <= 0.3 * seen  # (the other bit is set by chance in about a tenth)


def test_sparse_link(orc):
    """A link of 2^28 + 8 bytes: no chunk, the nonzero words listed instead."""
    ch = cs.make_chain(orc, cs.ROW["global-cursor64"].specs, 3)
    at, words = ch.sparse[0]
    most = (cs.SPARSE_MEMBERS + 256) * 11  # members and near members
    assert len(ch.chunks) == 1 and cs.SPARSE_MEMBERS < at.size <= most and (at % 8 == 0).all()
    assert sum(bin(int(w)).count("1") for w in words) <= most
    assert at.max() < (1 << 28) + 8 and (words != 0).all()
