"""Bloom chains of arbitrary link geometry for the tests, and the K1 dispatch
restated (plain helpers, no fixtures).

``make_chain`` builds a chain link by link on the oracle (each link a one-link
chain of its own, filled by ``add`` with its own members), assembles the
BF.SCANDUMP header plus one chunk per link, and loads that into a new oracle
chain; the same ``(iterator, data)`` list loads on the device by BF.LOADCHUNK.
Members carry the detection of a wrong position: at a tenth of the bits set, a
member whose probe lands on a wrong bit turns invalid almost surely.  Near
members carry the detection of a dropped probe (a walk cut short, a template
instance that holds fewer probes than the link has): every bit of theirs is set
but one, so a kernel that skips that probe calls them valid.

``plan`` restates, from csrc/, which K1 kernel and which template instance a
chain's geometry selects ("K1 dispatch"); ``ROWS`` are the
chains tests/test_chain_shapes.py runs, each with the arm its name says.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import struct
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "real-time-student-attendance-system_amd", "csrc")

_CHAIN = struct.Struct("<QIII")      # size, nfilters, options, growth
_LINK = struct.Struct("<QQQddIQB")   # bytes, bits, size, error, bpe, hashes, entries, n2
OPTIONS = 1 | 4                      # NOROUND | FORCE64
NEVER_GROWS = 1 << 40                # entries of a link that add must never grow past
SPARSE_FROM = 1 << 27                # link bytes from which no chunk is built (see make_chain)
SPARSE_MEMBERS = 1500                # members of such a link
FILL = 0.1                           # share of a link's bits its members set (about)


# ---------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------
def link_record(bits, hashes, size=0, entries=NEVER_GROWS, error=0.01, n2=0) -> dict:
    assert bits % 8 == 0 and bits >= 8
    return dict(bytes=bits // 8, bits=bits, size=size, error=error, bpe=hashes / 0.693147180559945,
                hashes=hashes, entries=entries, n2=n2)


def pack_header(links, size=None, growth=2) -> bytes:
    """dumpedChainHeader + dumpedChainLink[], as formats.bf_dump_header packs them (n2 kept)."""
    out = _CHAIN.pack(sum(L["size"] for L in links) if size is None else size, len(links), OPTIONS, growth)
    for L in links:
        out += _LINK.pack(L["bytes"], L["bits"], L["size"], L["error"], L["bpe"], L["hashes"], L["entries"],
                          L["n2"])
    return out


def random_ids(rng, n, short=None, width=None):
    """n packed ids (buf, offs): ``width`` bytes each, or 3..8 bytes where
    ``short[i]`` and 9..40 where not (exactly 8 is the most frequent short one)."""
    if width:
        lens = np.full(n, width, np.int64)
    else:
        short = np.asarray(short, bool)
        lens = np.where(short, np.minimum(rng.integers(3, 11, n), 8), rng.integers(9, 41, n))
    offs = np.zeros(n + 1, np.uint32)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, 256, int(offs[-1]), dtype=np.uint8), offs


@dataclass
class Chain:
    specs: list                 # [(bits, hashes)], oldest link first
    links: list                 # the header's link records
    chunks: list                # [(iterator, data)]: the header, then a chunk per link that is not sparse
    chain: object               # the loaded oracle chain
    singles: list               # the one-link oracle chain of every link
    members: list               # per link: (buf, offs)
    near: list                  # per link: (buf, offs, dropped probe) of its near members, None where hashes = 1
    sparse: dict = field(default_factory=dict)  # link -> (byte offsets, 8-byte words) of its nonzero words


def make_chain(orc, specs, seed, width=None, last_entries_over=None, n2=None) -> Chain:
    """The chain of ``specs`` = [(bits, hashes), ...], oldest link first.

    Every link is filled on a one-link oracle chain of its own (header options
    NOROUND | FORCE64, n2 = 0 unless given, entries 2^40 so add never grows it)
    with its own members until about a tenth of its bits are set, at least one
    member.  Then an eighth as many near members (1..256; none where hashes = 1)
    get the bits of all their probes but one set, straight in the bit array: the
    last probe for every other one, any probe for the rest.  ``width``: every id
    that many bytes (else ids alternate short, 3..8 bytes, and long).
    ``last_entries_over``: the last link's
    entries = its size + that (the chain then grows under BF.MADD).

    A link of SPARSE_FROM bytes or more (one-link chains only) gets
    SPARSE_MEMBERS members, no chunk is built for it, the one-link chain is the
    loaded chain, and ``sparse`` lists its nonzero 8-byte words for the device."""
    rng = np.random.default_rng(seed)
    singles, members, near, links = [], [], [], []
    for l, (bits, k) in enumerate(specs):
        rec = link_record(bits, k, n2=n2 or 0)
        one = orc.Chain.loadchunks([(1, pack_header([rec]))])
        nmem = max(1, int(bits * FILL / k))
        if bits // 8 >= SPARSE_FROM:
            assert len(specs) == 1
            nmem = SPARSE_MEMBERS
        buf, offs = random_ids(rng, nmem, short=np.arange(nmem) % 2 == 0, width=width)
        one.madd_packed(buf, offs)
        rec["size"] = one.link_info(0)["size"]
        singles.append(one)
        members.append((buf, offs))
        near.append(_near_members(orc, one, bits, k, rng, min(256, max(1, nmem // 8)), width) if k > 1 else None)
        links.append(rec)
    if last_entries_over is not None:
        links[-1]["entries"] = links[-1]["size"] + last_entries_over
    chunks, sparse, it = [(1, pack_header(links))], {}, 1
    if specs[0][0] // 8 >= SPARSE_FROM:
        words = np.ctypeslib.as_array(
            (C.c_uint64 * (specs[0][0] // 64)).from_address(orc.lib().orc_chain_link_bits(singles[0].p, 0)))
        at = np.flatnonzero(words)
        sparse[0] = (at * 8, words[at].copy())
        return Chain(list(specs), links, chunks, singles[0], singles, members, near, sparse)
    for one in singles:
        data = one.link_bits(0).tobytes()
        it += len(data)
        chunks.append((it, data))
    return Chain(list(specs), links, chunks, orc.Chain.loadchunks(chunks), singles, members, near, sparse)


BLOOM_SEED = 0xC6A4A7935BD1E995  # bloom_hash64: a = MurmurHash64A(id, this), b = MurmurHash64A(id, a)


def _near_members(orc, one, bits, k, rng, n, width):
    buf, offs = random_ids(rng, n, short=np.arange(n) % 2 == 0, width=width)
    bf = np.ctypeslib.as_array((C.c_uint8 * (bits // 8)).from_address(orc.lib().orc_chain_link_bits(one.p, 0)))
    drop = np.where(np.arange(n) % 2 == 0, k - 1, rng.integers(0, k, n))
    for i in range(n):
        x = buf[offs[i]:offs[i + 1]].tobytes()
        a = orc.murmur64a(x, BLOOM_SEED)
        b = orc.murmur64a(x, a)
        for j in range(k):
            if j != drop[i]:
                at = ((a + j * b) & (2 ** 64 - 1)) % bits
                bf[at >> 3] |= 1 << (at & 7)
    return buf, offs, drop


def load_engine(engine, fid, ch: Chain):
    """BF.LOADCHUNK of ``ch`` into filter ``fid`` through the C-ABI
    (ske_bf_load_header, ske_bf_link_write)."""
    from rtsas_amd._lib import BfLink
    arr = (BfLink * len(ch.links))()
    for a, L in zip(arr, ch.links):
        a.entries, a.bytes, a.bits, a.size = L["entries"], L["bytes"], L["bits"], L["size"]
        a.error, a.bpe, a.hashes = L["error"], L["bpe"], L["hashes"]
    engine.ctx.call("ske_bf_load_header", fid, arr, len(arr), sum(L["size"] for L in ch.links), 2, 0)
    for l, (_, data) in enumerate(ch.chunks[1:]):
        buf = np.frombuffer(data, np.uint8)
        engine.ctx.call("ske_bf_link_write", fid, l, 0, buf.ctypes.data_as(C.c_void_p), buf.size)
    for l, (at, words) in ch.sparse.items():
        for o, w in zip(at.tolist(), words):
            engine.ctx.call("ske_bf_link_write", fid, l, o, w.tobytes(), 8)


def load_client(client, key, ch: Chain):
    assert not ch.sparse
    for it, data in ch.chunks:
        assert client.execute_command("BF.LOADCHUNK", key, it, data) in ("OK", b"OK")


# ---------------------------------------------------------------------------
# items
# ---------------------------------------------------------------------------
@dataclass
class Items:
    buf: np.ndarray
    offs: np.ndarray
    slots: np.ndarray
    link: np.ndarray            # per item: the link it is a member of, -1 non-member, -2 near member
    width: int = 0              # fixed width (0: ragged)

    @property
    def n(self):
        return len(self.offs) - 1


NKEYS = 5


def make_items(ch: Chain, rng, n, width=None) -> Items:
    """n packed ids over NKEYS keys: 55 % members, every link's in equal shares
    (links in rotation), a tenth near members likewise, the rest random
    non-members.  ``link``: the member's link, -1 for a non-member, -2 for a near
    member.  Ragged ids come in runs of 64 (a wave of the kernels when a block's
    chunk starts on a multiple of 64, as with n = 6144 at every tile size): three
    runs of mixed lengths (members short or long; non-members of 0..8 or 9..40
    bytes), then one of short ids only (0..8 bytes, exactly 8 among them) -- k1's
    and k_swipes' wave-uniform short-id branch is taken by some waves and not
    by others."""
    i = np.arange(n)
    short_run = np.zeros(n, bool) if width else (i // 64) % 4 == 3
    u = rng.random(n)
    has_near = [l for l, x in enumerate(ch.near) if x is not None]
    cls = np.where(u < 0.55, 0, np.where((u < 0.65) & bool(has_near), 1, 2))  # member, near member, non-member
    owner = np.full(n, -1)
    owner[cls == 0] = np.arange((cls == 0).sum()) % len(ch.members)
    if has_near:
        owner[cls == 1] = np.asarray(has_near)[np.arange((cls == 1).sum()) % len(has_near)]
    non = cls == 2
    nn = int(non.sum())
    if width:
        nb, no = random_ids(rng, nn, width=width)
    else:
        nlen = np.where(short_run[non] | (rng.random(nn) < 0.5), rng.integers(0, 9, nn), rng.integers(9, 41, nn))
        no = np.zeros(nn + 1, np.uint32)
        no[1:] = np.cumsum(nlen)
        nb = rng.integers(0, 256, int(no[-1]), dtype=np.uint8)
    # the pool: every link's members, every link's near members, then this call's non-members
    pools = [(0, l, b, o) for l, (b, o) in enumerate(ch.members)]
    pools += [(1, l, x[0], x[1]) for l, x in enumerate(ch.near) if x is not None]
    pool = np.concatenate([b for _, _, b, _ in pools] + [nb])
    start = np.zeros(n, np.int64)
    lens = np.zeros(n, np.int64)
    base = 0
    for c, l, b, o in pools:
        o = o.astype(np.int64)
        mlen = np.diff(o)
        for want_short in (False, True):
            sel = np.flatnonzero((cls == c) & (owner == l) & (short_run == want_short))
            if sel.size == 0:
                continue
            cand = np.flatnonzero(mlen <= 8) if want_short else np.arange(mlen.size)
            j = cand[rng.integers(0, cand.size, sel.size)]
            start[sel], lens[sel] = base + o[j], mlen[j]
        base += b.size
    o = no.astype(np.int64)
    start[non], lens[non] = base + o[:-1], np.diff(o)
    offs = np.zeros(n + 1, np.uint32)
    offs[1:] = np.cumsum(lens)
    src = np.repeat(start - offs[:-1].astype(np.int64), lens) + np.arange(int(offs[-1]))
    buf = np.concatenate([pool[src], np.zeros(16, np.uint8)])  # (slack for 16-byte loads of a host copy)
    link = np.where(cls == 0, owner, np.where(cls == 1, -2, -1))
    return Items(buf, offs, rng.integers(0, NKEYS, n).astype(np.uint32), link, width or 0)


def check_inputs(orc, ch: Chain, it: Items, strict=True):
    """The conditions a case must meet on the oracle's answers alone: every
    member valid; 20..80 % of the items valid; every link's one-link chain passes
    at most half of the non-members.  Returns the oracle's answers.  (``strict``
    False: batches too small for the shares to mean anything skip the last two.)"""
    for l, (b, o) in enumerate(ch.members):
        got, _ = ch.chain.mexists_packed(b, o)
        assert got.all(), f"link {l}: a member is not in the assembled chain"
    valid, _ = ch.chain.mexists_packed(it.buf, it.offs)
    assert valid[it.link >= 0].all()
    if strict:
        assert 0.2 <= valid.mean() <= 0.8, valid.mean()
        non = it.link == -1
        for l, one in enumerate(ch.singles):
            got, _ = one.mexists_packed(it.buf, it.offs)
            assert got[non].mean() <= 0.5, (l, got[non].mean())
    return valid


# ---------------------------------------------------------------------------
# the K1 dispatch, restated from csrc/ (sketch_api_swipes.cpp k1_variant / use_lds,
# sketch_k1.hip k1_lds_plan, sketch_part.hip part_plan / part_km, sketch_xr.hip
# xr_supported and the KB ladder of launch_swipes_xr)
# ---------------------------------------------------------------------------
K1_MAX_PIECES, K1_MAX_LINKS, K1_WAVES = 10, 8, 16
LDS_MAX = 152 * 1024
XR_BATCH_K, XR_MAX_LINKS, XR_MAX_K, XR_KB = 16, 8, 31, (7, 8, 10, 11, 13, 16)
P_MAX_LINKS, P_MAX_SLICES, P_SLICE_LOG, P_KM = 8, 2047, 19, (11, 22)
XR_MIN_BYTES = 8 << 20
XR_REGIONS, XR_SLICE_ALIGN = 8, 1024    # sketch_xr.hip: one slice of every link per XCD, a multiple of 1024 bits


def csrc_constants() -> dict:
    """The constants above as csrc/ holds them now."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    def const(text, name):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
        assert m, name
        return int(eval(re.sub(r"(?<=\d)(ull|u)\b", "", m.group(1)), {"__builtins__": {}}))

    k1, xr, part, inl, api = (src(n) for n in ("sketch_k1.hip", "sketch_xr.hip", "sketch_part.hip",
                                               "sketch_internal.h", "sketch_api_swipes.cpp"))
    ladder = [int(a) for a, b in re.findall(r"kmax <= (\d+)\) \{ SKE_XR_B\((\d+)\)", xr) if a == b]
    ladder += [int(x) for x in re.findall(r"else \{ SKE_XR_B\((\d+)\) \}", xr)]
    return dict(
        K1_MAX_PIECES=const(k1, "kK1MaxPieces"), K1_MAX_LINKS=const(inl, "kK1MaxLinks"),
        K1_WAVES=const(k1, "kK1Block") // 64, LDS_MAX=const(inl, "kLdsBloomMaxBytes"),
        XR_BATCH_K=const(xr, "kXrBatchK"), XR_MAX_LINKS=const(xr, "kXrMaxLinks"),
        XR_MAX_K=int(re.search(r"\.k > (\d+)\) return false", xr).group(1)), XR_KB=tuple(ladder),
        P_MAX_LINKS=const(inl, "kPMaxLinks"), P_MAX_SLICES=const(inl, "kPMaxSlices"),
        P_SLICE_LOG=const(inl, "kPSliceLog"),
        P_KM=tuple(int(b) for a, b in re.findall(r"if \(ksum <= (\d+)\) return (\d+);", part) if a == b),
        XR_MIN_BYTES=const(api, "kXrMinBytes"))


def csrc_cut_constants() -> dict:
    """The constants of xr_cuts as csrc/ holds them now: kRegions, and the
    alignment A of both region kernels' ``slice = ((d + kRegions - 1) / kRegions + A - 1) & ~(A - 1)``."""
    def src(name):
        with open(os.path.join(CSRC, name)) as f:
            return f.read()

    m = re.search(r"constexpr\s+\w+\s+kRegions\s*=\s*(\d+);", src("sketch_common.h"))
    found = re.findall(r"slice = \(\(d \+ kRegions - 1\) / kRegions \+ (\d+)\) & ~(\d+)u;", src("sketch_xr.hip"))
    assert m and len(found) == 2 and len(set(found)) == 1 and found[0][0] == found[0][1], (m, found)
    return dict(XR_REGIONS=int(m.group(1)), XR_SLICE_ALIGN=int(found[0][0]) + 1)


def _pad16(bits):
    return (bits // 8 + 15) // 16 * 16


def lds_pieces(specs):
    """k1_lds_plan: the 1 KiB pieces of the LDS image, None where it refuses."""
    if not 1 <= len(specs) <= K1_MAX_LINKS:
        return None
    pieces = 0
    for bits, _ in specs:
        if bits > 1 << 31 or bits < 64:
            return None
        pieces += (_pad16(bits) + 1023) // 1024
    if pieces * 1024 > LDS_MAX or pieces > K1_WAVES * K1_MAX_PIECES:
        return None
    return pieces


def part_slices(specs):
    """part_plan: (km, slices), None where it refuses."""
    if not 1 <= len(specs) <= P_MAX_LINKS:
        return None
    slices = ksum = 0
    for bits, k in specs:
        if bits > 1 << 31 or bits < 64 or not 1 <= k <= 64:
            return None
        slices += (bits + (1 << P_SLICE_LOG) - 1) >> P_SLICE_LOG
        ksum += k
    km = next((m for m in P_KM if ksum <= m), None)
    return None if slices > P_MAX_SLICES or km is None else (km, slices)


def xr_kb(specs):
    """xr_supported and launch_swipes_xr: the KB of k_xr_region_b, 0 for the
    per-step k_xr_region, None where xr refuses."""
    if not 1 <= len(specs) <= XR_MAX_LINKS or any(bits > 1 << 31 or k > XR_MAX_K for bits, k in specs):
        return None
    kmax = max(k for _, k in specs)
    return next(kb for kb in XR_KB if kmax <= kb) if kmax <= XR_BATCH_K else 0


def xr_cuts(bits):
    """k_xr_region / k_xr_region_b: region r = 1 .. 7 of a link tests the bits
    from ``r * slice``, slice = ceil(bits / 8) rounded up to 1024 bits; the bit
    positions where one region ends and the next begins."""
    per = ((bits + XR_REGIONS - 1) // XR_REGIONS + XR_SLICE_ALIGN - 1) & ~(XR_SLICE_ALIGN - 1)
    return tuple(r * per for r in range(1, XR_REGIONS) if r * per < bits)


def plan(specs, variant):
    """(what ske_swipes_variant answers, the arm ske_swipes runs on) under the
    option "variant": the arm is "lds P=<P>" (k_swipes_lds<.., P>), "legacy"
    (k_swipes with the staged image), "global", "part km=<km>" or "xr KB=<KB>"
    (KB 0: the per-step kernel)."""
    image = sum(_pad16(bits) for bits, _ in specs)
    if variant in (-1, 1) and image <= LDS_MAX:
        pieces = lds_pieces(specs)
        return 1, "legacy" if pieces is None else f"lds P={(pieces + K1_WAVES - 1) // K1_WAVES}"
    big = sum(bits // 8 for bits, _ in specs) >= XR_MIN_BYTES or variant in (2, 3)
    if variant == 0 or not big:
        return 0, "global"
    if variant != 2 and part_slices(specs) is not None:
        return 3, f"part km={part_slices(specs)[0]}"
    if xr_kb(specs) is not None:
        return 2, f"xr KB={xr_kb(specs)}"
    return 0, "global"


# ---------------------------------------------------------------------------
# the rows: (name, specs, forced variant, the arm the name says, batch sizes)
# ---------------------------------------------------------------------------
@dataclass
class Row:
    name: str
    specs: list
    variant: int                # the variant the row forces (-1: none)
    arm: str                    # plan(specs, variant)[1]
    ns: tuple = (6144,)         # batch sizes ("cu": see test_chain_shapes._n)
    tiles: tuple = (1,)
    seed: int = 0


def _by(sizes, ks):
    return [(8 * b, k) for b, k in zip(sizes, ks)]


KIB = 1024
E_BYTES, E_K = [8, 1032, 2056, 40, 5000, 1024, 16, 30000], [1, 31, 8, 3, 17, 12, 64, 7]
ROW_E = _by(E_BYTES, E_K)
ROW_F = _by([70000, 62000], [9, 8])
T124 = (1, 2, 4)

ROWS = (
    # LDS fast path; the forced variant is 1, and -1 runs as for every row
    [Row(f"lds-a{P}", _by([16 * (P - 1) * KIB + 8], [7]), 1, f"lds P={P}", tiles=T124) for P in range(1, 11)]
    # full rounds: 16 P pieces.  P = 10 would be 160 KiB, past the 152 KiB image, so 9 is the largest
    + [Row(f"lds-b{P}", _by([16 * P * KIB], [7]), 1, f"lds P={P}", tiles=T124) for P in (1, 5, 9)]
    + [Row("lds-c", _by([152 * KIB], [7]), 1, "lds P=10", tiles=T124),
       Row("lds-d", _by([152 * KIB + 8], [7]), 1, "global", tiles=T124),
       Row("lds-e", ROW_E, 1, "lds P=3", tiles=T124),
       # 69 + 61 pieces (70 000 + 60 000 bytes would be 69 + 59 = 128: P = 8, which lds-g has)
       Row("lds-f", ROW_F, 1, "lds P=9", tiles=T124),
       Row("lds-g", _by([24 * KIB] * 5, range(7, 12)), 1, "lds P=8", tiles=T124),
       # d = 64 is the smallest link the plan takes
       Row("lds-8", _by([8], [1]), 1, "lds P=1", tiles=T124)]
    # the legacy LDS kernel: the image fits and k1_lds_plan refuses
    + [Row("legacy-9links", _by([KIB] * 9, range(7, 16)), -1, "legacy", tiles=T124),
       Row("legacy-7", _by([7], [5]), -1, "legacy"),
       Row("legacy-1-7", _by([1, 7], [3, 5]), -1, "legacy", tiles=T124),
       # 7 x 19 + 20 = 153 pieces of 1 KiB, while the 16-B padded sum is 148 608 bytes
       Row("legacy-pieces", _by([18440] * 7 + [19464], range(7, 15)), -1, "legacy")]
    # global
    + [Row("global-48links", _by([4 * KIB] * 48, [1 + i % 31 for i in range(48)]), 0, "global", tiles=T124),
       Row("global-e", ROW_E, 0, "global"),
       Row("global-cursor64", _by([(1 << 28) + 8], [11]), 0, "global")]
    # xr
    + [Row(f"xr-k{k}", _by([64 * KIB], [k]), 2, f"xr KB={kb}")
       for k, kb in ((1, 7), (7, 7), (8, 8), (9, 10), (10, 10), (11, 11), (12, 13), (13, 13), (14, 16), (16, 16),
                     (17, 0), (31, 0))]
    + [Row("xr-k32", _by([64 * KIB], [32]), 2, "global"),
       Row("xr-1byte", _by([1], [7]), 2, "xr KB=7"),
       Row("xr-8bytes", _by([8], [7]), 2, "xr KB=7"),
       Row("xr-128bytes", _by([128], [7]), 2, "xr KB=7"),
       Row("xr-1032bytes", _by([1032], [7]), 2, "xr KB=7"),
       Row("xr-8links", _by([4 * KIB + 8 * i for i in range(8)], range(7, 15)), 2, "xr KB=16"),
       Row("xr-9links", _by([4 * KIB] * 9, range(7, 16)), 2, "global"),
       # the grown chain of the product: sum k = 24, 9 MB
       Row("xr-grown", _by([3 << 20] * 3, [7, 8, 9]), -1, "xr KB=10"),
       # d = 2^31: 4096 slices, past the partitioned kernel's 2047
       Row("xr-2p31", _by([1 << 28], [11]), -1, "xr KB=11"),
       Row("xr-ragged", _by([64 * KIB], [11]), 2, "xr KB=11", ns=(64 * 11 + 1, 4095, 4097, "cu"))]
    # partitioned
    + [Row("part-11", _by([64 * KIB], [11]), 3, "part km=11", ns=(6144, 1, 1023, 1025, 3 * 1024 + 5)),
       Row("part-5-6", _by([64 * KIB + 8, 8], [5, 6]), 3, "part km=11"),
       Row("part-9links", _by([KIB] * 9, [1] * 8 + [3]), 3, "global"),
       Row("part-12", _by([64 * KIB + 8], [12]), 3, "part km=22"),
       Row("part-4-4-4", _by([128 * KIB + 16, 8, 64 * KIB], [4, 4, 4]), 3, "part km=22"),
       Row("part-22", _by([8], [22]), 3, "part km=22"),
       Row("part-7-7-8", _by([64 * KIB, 64 * KIB + 8, 128 * KIB + 16], [7, 7, 8]), 3, "part km=22",
           ns=(6144, 1, 1023, 1025, 3 * 1024 + 5)),
       Row("part-8links", _by([8, 64 * KIB, KIB, 64 * KIB + 8, 40, 128 * KIB + 16, 8, 4 * KIB],
                              [1, 1, 2, 2, 3, 3, 4, 6]), 3, "part km=22"),
       Row("part-23", _by([64 * KIB], [23]), 3, "xr KB=0")]
)
for _i, _r in enumerate(ROWS):
    _r.seed = 1000 + _i
ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)
