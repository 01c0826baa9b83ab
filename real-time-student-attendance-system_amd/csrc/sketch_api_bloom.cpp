// sketch_api_bloom.cpp -- libsketch C-ABI (include/sketch.h): Bloom chains.
//
// Host arithmetic here is the RedisBloom bookkeeping that is not
// data-parallel: link geometry (deps/bloom/bloom.c bloom_init + calc_bpe) and
// chain growth (src/sb.c SBChain_Add), with the same libm calls as
// RedisBloom.  Compiled with -ffp-contract=off.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "sketch_ctx.h"

using namespace ske;

// deps/bloom/bloom.c calc_bpe() + bloom_init() with BLOOM_OPT_NOROUND |
// BLOOM_OPT_FORCE64, the options rebloom.c's bfCreateChain() passes.
static int link_geometry(uint64_t entries, double error, Link *L) {
    if (entries < 1 || !(error > 0) || error >= 1.0) return SKE_EINVAL;
    const double denom = 0.480453013918201;  // ln(2)^2
    double bpe = -(log(error) / denom);
    if (bpe < 0) bpe = -bpe;
    uint64_t bits = (uint64_t)((double)entries * bpe);
    if (bits == 0) bits = 1;
    uint64_t bytes = (bits % 64) ? ((bits / 64) + 1) * 8 : bits / 8;
    L->entries = entries;
    L->error = error;
    L->bpe = bpe;
    L->bytes = bytes;
    L->bits = bytes * 8;
    L->hashes = (int)ceil(0.693147180559945 * bpe);
    L->size = 0;
    if (L->bits >= (uint64_t(1) << 62)) return SKE_ENOMEM;
    L->div = make_divisor(L->bits);
    return SKE_OK;
}

// a link's device bytes, padded to 16 so 4-byte atomics and 16-byte staging never leave it
static uint64_t link_padded(const Link &L) { return (L.bytes + 15) & ~uint64_t(15); }

// L.bf: the link's device bits, zeroed on st (*allocated: the failure, if any, was the zeroing's)
static hipError_t link_alloc(Link &L, hipStream_t st, bool *allocated) {
    hipError_t e = hipMalloc(&L.bf, link_padded(L));
    *allocated = e == hipSuccess;
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(L.bf, 0, link_padded(L), st);
    if (e != hipSuccess) {
        (void)hipFree(L.bf);
        L.bf = nullptr;
    }
    return e;
}

static int add_link(ske_ctx *c, Filter &F, uint64_t entries, double error) {
    if ((int)F.links.size() >= SKE_MAX_LINKS) return SKE_ENOMEM;
    Link L;
    int rc = link_geometry(entries, error, &L);
    if (rc) return rc;
    bool allocated;
    const hipError_t e = link_alloc(L, c->st, &allocated);
    if (e != hipSuccess) {
        c->last_hip = std::string(allocated ? "hipMemset" : "hipMalloc") + "(bloom link): " + hipGetErrorString(e);
        return allocated ? SKE_EHIP : SKE_ENOMEM;
    }
    F.links.push_back(L);
    F.dev_ok = false;
    return SKE_OK;
}

namespace ske {
void free_filter(Filter &F) {
    for (auto &L : F.links)
        if (L.bf) (void)hipFree(L.bf);
    F = Filter();
}
}  // namespace ske

static LinkDev link_dev(const Link &L) {
    LinkDev D{};
    D.bf = L.bf;
    D.div = L.div;
    D.k = uint32_t(L.hashes);
    D.lds_off = 0;
    D.rmul = uint32_t((uint64_t(kRegions) << 32) / L.bits);
    return D;
}

static ChainDev chain_dev(const Filter &F) {
    ChainDev ch{};
    uint32_t lds = 0;  // each link's offset in the LDS image
    for (const Link &L : F.links) {
        LinkDev &D = ch.link[ch.nlinks++];
        D = link_dev(L);
        D.lds_off = lds;
        lds = (lds + link_padded(L) > 0xffffffffu) ? 0xffffffffu : uint32_t(lds + link_padded(L));
    }
    ch.lds_bytes = lds;
    return ch;
}

namespace ske {
const ChainDev &chain_of(Filter *F) {
    static const ChainDev empty{};
    if (!F->exists) return empty;
    if (!F->dev_ok) {
        F->dev = chain_dev(*F);
        F->dev_ok = true;
    }
    return F->dev;
}
}  // namespace ske

extern "C" {

int ske_bf_reserve(ske_ctx *c, uint32_t fid, double error_rate, uint64_t capacity,
                   uint32_t expansion, int nonscaling) {
    if (!c) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (!(error_rate > 0) || error_rate >= 1) return SKE_EBADRATE;
    if (capacity == 0) return SKE_EBADCAP;
    if (expansion < 1 && !nonscaling) return SKE_EBADEXP;
    if (F->exists) return SKE_EEXISTS;
    Filter nf;
    nf.growth = expansion;
    nf.nonscaling = nonscaling != 0;
    // SB_NewChain(): first link error * ERROR_TIGHTENING_RATIO unless NONSCALING
    const double tightening = nf.nonscaling ? 1.0 : 0.5;
    int rc = add_link(c, nf, capacity, error_rate * tightening);
    if (rc) {
        free_filter(nf);
        return rc;
    }
    nf.exists = true;
    *F = nf;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_bf_exists_key(ske_ctx *c, uint32_t fid) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    return (F && F->exists) ? 1 : 0;
}

int ske_bf_free(ske_ctx *c, uint32_t fid) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F) return SKE_EINVAL;
    (void)hipStreamSynchronize(c->st);
    free_filter(*F);
    return SKE_OK;
}

int ske_bf_info(ske_ctx *c, uint32_t fid, ske_bf_info_t *out) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || !out) return SKE_EINVAL;
    if (!F->exists) return SKE_ENOFILTER;
    memset(out, 0, sizeof(*out));
    // SBChain_MemUsage(): sizeof(SBChain) + nfilters*sizeof(SBLink) + bytes
    uint64_t mem = 32 + 64 * F->links.size();
    for (auto &L : F->links) {
        out->capacity += L.entries;
        mem += L.bytes;
    }
    out->size_bytes = mem;
    out->nfilters = uint32_t(F->links.size());
    out->expansion = F->growth;
    out->inserted = F->size;
    out->nonscaling = F->nonscaling;
    return SKE_OK;
}

int ske_bf_link_info(ske_ctx *c, uint32_t fid, uint32_t link, ske_bf_link_t *out) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || !out) return SKE_EINVAL;
    if (!F->exists) return SKE_ENOFILTER;
    if (link >= F->links.size()) return SKE_EINVAL;
    const Link &L = F->links[link];
    memset(out, 0, sizeof(*out));
    out->entries = L.entries;
    out->bytes = L.bytes;
    out->bits = L.bits;
    out->size = L.size;
    out->error = L.error;
    out->bpe = L.bpe;
    out->hashes = L.hashes;
    return SKE_OK;
}

int ske_bf_export_link(ske_ctx *c, uint32_t fid, uint32_t link, uint8_t *out, uint64_t cap) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || !out) return SKE_EINVAL;
    if (!F->exists) return SKE_ENOFILTER;
    if (link >= F->links.size()) return SKE_EINVAL;
    const Link &L = F->links[link];
    if (cap < L.bytes) return SKE_EINVAL;
    HIPCHK(c, hipMemcpyAsync(out, L.bf, L.bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_bf_import_link(ske_ctx *c, uint32_t fid, uint32_t link, const uint8_t *in,
                       uint64_t nbytes) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || !in) return SKE_EINVAL;
    if (!F->exists) return SKE_ENOFILTER;
    if (link >= F->links.size() || nbytes != F->links[link].bytes) return SKE_EINVAL;
    HIPCHK(c, hipMemcpyAsync(F->links[link].bf, in, nbytes, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_bf_link_write(ske_ctx *c, uint32_t fid, uint32_t link, uint64_t offset, const uint8_t *in,
                      uint64_t nbytes) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || (!in && nbytes)) return SKE_EINVAL;
    if (!F->exists) return SKE_ENOFILTER;
    if (link >= F->links.size()) return SKE_EINVAL;
    const Link &L = F->links[link];
    if (offset > L.bytes || nbytes > L.bytes - offset) return SKE_EINVAL;
    if (nbytes) {
        HIPCHK(c, hipMemcpyAsync(L.bf + offset, in, nbytes, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    return SKE_OK;
}

int ske_bf_load_header(ske_ctx *c, uint32_t fid, const ske_bf_link_t *links, uint32_t nlinks,
                       uint64_t inserted, uint32_t expansion, int nonscaling) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F || (!links && nlinks)) return SKE_EINVAL;
    if (F->exists) return SKE_EEXISTS;
    if (nlinks == 0 || nlinks > SKE_MAX_LINKS) return SKE_EINVAL;
    Filter nf;
    nf.growth = expansion;
    nf.nonscaling = nonscaling != 0;
    for (uint32_t i = 0; i < nlinks; i++) {
        const ske_bf_link_t &H = links[i];
        if (H.bytes == 0 || H.bits != H.bytes * 8 || H.bits >= (uint64_t(1) << 62) || H.hashes < 1 ||
            H.hashes > 64) {
            free_filter(nf);
            return SKE_EINVAL;
        }
        Link L;
        L.entries = H.entries;
        L.bytes = H.bytes;
        L.bits = H.bits;
        L.size = H.size;
        L.error = H.error;
        L.bpe = H.bpe;
        L.hashes = H.hashes;
        L.div = make_divisor(L.bits);
        bool allocated;
        const hipError_t e = link_alloc(L, c->st, &allocated);
        if (e != hipSuccess) {
            free_filter(nf);
            c->last_hip = std::string("load header: ") + hipGetErrorString(e);
            return SKE_ENOMEM;
        }
        nf.links.push_back(L);
    }
    nf.size = inserted;
    nf.exists = true;
    *F = nf;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_bf_mexists(ske_ctx *c, uint32_t fid, const uint8_t *bytes, const uint32_t *offs,
                   uint64_t n, uint8_t *out, int mem) {
    if (!c || !out) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!F->exists) {  // BFCheck on a missing key answers 0
        if (mem == SKE_MEM_DEVICE) {
            HIPCHK(c, hipMemsetAsync(out, 0, n, c->st));
            HIPCHK(c, hipStreamSynchronize(c->st));
        } else {
            memset(out, 0, n);
        }
        return SKE_OK;
    }
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    uint8_t *dout = out;
    if (mem != SKE_MEM_DEVICE) {
        dout = (uint8_t *)stage_buf(c, kStgOut, n, &rc);
        if (rc) return rc;
    }
    const ChainDev &ch = chain_of(F);
    K1Args A;
    if (k1_fast_args(c, ch, PartBatch{s.bytes, s.offs, 0, nullptr, n, dout}, &A))
        HIPCHK(c, launch_swipes_lds(A, false, c->pb, c->cus, c->st));
    else
        HIPCHK(c, launch_swipes(1, ch, use_lds(c, ch), c->pb, s.bytes, s.offs, 0, nullptr, n, nullptr,
                                0, dout, nullptr, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(out, dout, n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

// BF.MADD with SBChain_Add's sequential semantics, in epochs: an epoch fills
// the current link up to its remaining capacity with the candidates in
// order ("first setter" per bit decides who is still absent when its turn
// comes), then the chain grows and the rest continue in the new link.
int ske_bf_madd(ske_ctx *c, uint32_t fid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                int8_t *out, int mem) {
    if (!c) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (!F->exists) {  // rebloom.c BF.ADD / BF.MADD auto-create: 0.01, 100, expansion 2
        int rc = ske_bf_reserve(c, fid, 0.01, 100, 2, 0);
        if (rc) return rc;
    }
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    uint64_t *ha = (uint64_t *)scratch_get(c->scratch, kScrBfHa, n * 8, &e);
    uint64_t *hb = (uint64_t *)scratch_get(c->scratch, kScrBfHb, n * 8, &e);
    uint8_t *state = (uint8_t *)scratch_get(c->scratch, kScrBfState, n, &e);
    int8_t *res = (int8_t *)scratch_get(c->scratch, kScrBfRes, n, &e);
    uint32_t *absent = (uint32_t *)scratch_get(c->scratch, kScrBfAbsent, n * 4, &e);
    uint32_t *pos = (uint32_t *)scratch_get(c->scratch, kScrBfPos, n * 4, &e);
    if (e != hipSuccess) {
        c->last_hip = hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    HIPCHK(c, hipMemsetAsync(state, 0, n, c->st));
    HIPCHK(c, launch_bf_hash(s.bytes, s.offs, n, ha, hb, c->cus, c->st));
    HIPCHK(c, launch_bf_settle_present(chain_of(F), n, ha, hb, state, res, c->cus, c->st));
    for (int epoch = 0; epoch < 4 * SKE_MAX_LINKS + 4; epoch++) {
        Link *L = &F->links.back();
        uint64_t cap = L->size >= L->entries ? 0 : L->entries - L->size;
        if (cap == 0) {
            HIPCHK(c, hipMemsetAsync(c->stats, 0, 8, c->st));
            HIPCHK(c, launch_bf_count_cands(n, state, c->stats, c->cus, c->st));
            unsigned long long remaining = 0;
            HIPCHK(c, hipMemcpyAsync(&remaining, c->stats, 8, hipMemcpyDeviceToHost, c->st));
            HIPCHK(c, hipStreamSynchronize(c->st));
            if (remaining == 0) break;
            if (F->nonscaling) {
                HIPCHK(c, launch_bf_fill_rest(n, state, res, -2, c->cus, c->st));
                break;
            }
            // SBChain_Add(): next link entries * growth, error * 0.5
            rc = add_link(c, *F, L->entries * (uint64_t)F->growth, L->error * 0.5);
            if (rc) return rc;
            L = &F->links.back();
            cap = L->entries;
        }
        if (L->bits > 0xffffffffull * 4ull) return SKE_ENOMEM;
        uint32_t *first = (uint32_t *)scratch_get(c->scratch, kScrKeysOrFirst, L->bits * 4, &e);
        if (e != hipSuccess) {
            c->last_hip = hipGetErrorString(e);
            return SKE_ENOMEM;
        }
        HIPCHK(c, hipMemsetAsync(first, 0xff, L->bits * 4, c->st));
        const LinkDev D = link_dev(*L);
        HIPCHK(c, launch_bf_first_setter(D, n, ha, hb, state, first, c->cus, c->st));
        HIPCHK(c, launch_bf_absent(D, n, ha, hb, state, first, absent, c->cus, c->st));
        HIPCHK(c, scan_inclusive_u32(c->scratch, absent, pos, n, c->st));
        uint32_t total_absent = 0;
        HIPCHK(c, hipMemcpyAsync(&total_absent, pos + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        const uint32_t cap32 = cap > 0xffffffffull ? 0xffffffffu : uint32_t(cap);
        HIPCHK(c, launch_bf_resolve(D, n, ha, hb, state, absent, pos, cap32, res, L->bf, c->cus,
                                    c->st));
        const uint64_t added = std::min<uint64_t>(cap, total_absent);
        L->size += added;
        F->size += added;
        if (total_absent < cap) break;  // every candidate resolved
        // the rest see this link as left by the resolved adds
        ChainDev one{};
        one.nlinks = 1;
        one.link[0] = D;
        HIPCHK(c, launch_bf_settle_present(one, n, ha, hb, state, res, c->cus, c->st));
    }
    if (out) {
        if (mem == SKE_MEM_DEVICE)
            HIPCHK(c, hipMemcpyAsync(out, res, n, hipMemcpyDeviceToDevice, c->st));
        else
            HIPCHK(c, hipMemcpyAsync(out, res, n, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

}  // extern "C"
