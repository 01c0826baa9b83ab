// sketch_api_swipes.cpp -- libsketch C-ABI (include/sketch.h): K1 (BF.EXISTS +
// PFADD per swipe) -- the variant a chain selects, launch_k1, the ske_swipes*
// entry points -- and the routing of unpartitioned swipes (ske_route_*).
#include "sketch_ctx.h"

using namespace ske;

namespace ske {

bool use_lds(const ske_ctx *c, const ChainDev &ch) {
    if (!c->lds_ok || ch.nlinks == 0) return false;
    if (c->variant == 0 || c->variant == 2 || c->variant == 3) return false;
    return ch.lds_bytes <= lds_bloom_max();
}

}  // namespace ske

// K1 variant for a chain: 1 LDS image (fits 152 KiB); for larger chains
// (>= 8 MB, or when asked for) 3 partitioned (probes routed to LDS-resident
// slices; sketch_part.hip) or 2 XCD-partitioned (L2-resident slices;
// sketch_xr.hip) when the chain's shape does not fit the partitioned
// kernel; else 0 global.
constexpr uint64_t kXrMinBytes = 8ull << 20;
static int k1_variant(const ske_ctx *c, const ChainDev &ch) {
    if (ch.nlinks == 0) return 0;
    if (use_lds(c, ch)) return 1;
    if (c->variant == 0) return 0;
    uint64_t total = 0;
    for (int l = 0; l < ch.nlinks; l++) total += ch.link[l].div.d >> 3;
    const bool big = total >= kXrMinBytes || c->variant == 2 || c->variant == 3;
    if (!big) return 0;
    if (c->variant != 2 && part_supported(ch)) return 3;
    if (xr_supported(ch)) return 2;
    return 0;
}

namespace ske {

bool k1_fast_args(ske_ctx *c, const ChainDev &ch, const PartBatch &b, K1Args *A) {
    if (!c->k1_ok || !use_lds(c, ch)) return false;
    if (b.n >= (uint64_t(1) << 31)) return false;
    if (!b.offs && uint64_t(b.fixed_w) * b.n >= (uint64_t(1) << 32)) return false;
    if (!k1_lds_plan(ch, A)) return false;
    A->bytes = b.bytes;
    A->offs = b.offs;
    A->slot = b.slot;
    A->regs = c->regs;
    A->out = b.out;
    A->err = c->err;
    A->zero16 = c->zero16;
    A->n = uint32_t(b.n);
    A->nslots = c->nslots;
    A->fixed_w = b.fixed_w;
    return true;
}

}  // namespace ske

// The partitioned K1 over nb batches, every pass on st.
static int launch_part(ske_ctx *c, const ChainDev &ch, const PartBatch *bt, uint32_t nb, hipStream_t st) {
    uint64_t nmax = 0;
    for (uint32_t j = 0; j < nb; j++) nmax = bt[j].n > nmax ? bt[j].n : nmax;
    if (nmax == 0) return SKE_OK;
    hipError_t e = part_reserve(ch, nmax, c->part_sub, c->nslots, c->seg, c->scratch);
    if (e != hipSuccess) return scratch_error(c, e);
    ScratchUser use(c, c->xr, st);
    if (use.rc) return use.rc;
    // one event pair per kernel and unit, bracketed on the kernel's stream;
    // back-to-back kernels on one stream share the event between them
    struct Hook {
        ske_ctx *c;
        PassMark pm[5];
        hipEvent_t last = nullptr;  // the end event recorded last, if nothing came after it,
        hipStream_t last_st = nullptr;  // and its stream
    } hs{c};
    auto hook = [](void *u, int pass, int end, hipStream_t kst) {
        Hook *h = static_cast<Hook *>(u);
        if (end) {
            h->pm[pass].end();
            h->last = h->pm[pass].end_event();
            h->last_st = kst;
        } else {
            const bool share = h->last && h->last_st == kst;
            h->pm[pass].begin(h->c, 1 + pass, kst, share ? h->last : nullptr);
            h->last = nullptr;
        }
    };
    e = launch_swipes_part(ch, bt, nb, c->regs, c->nslots, c->scratch, c->err, c->cus, c->part_sub, c->seg, st,
                           c->timing && !c->capturing ? +hook : nullptr, &hs);
    if (e != hipSuccess) {
        c->last_hip = std::string("launch_swipes_part: ") + hipGetErrorString(e);
        return SKE_EHIP;
    }
    return SKE_OK;
}

namespace ske {

int launch_k1(ske_ctx *c, const ChainDev &ch, const PartBatch &b, hipStream_t st, int grid) {
    if (b.n == 0) return SKE_OK;
    K1Args A;
    if (k1_fast_args(c, ch, b, &A)) {
        PassMark m(c, 0, st);
        HIPCHK(c, launch_swipes_lds(A, true, c->pb, grid, st));
        m.end();
        return SKE_OK;
    }
    const int var = k1_variant(c, ch);
    if (var == 3) return launch_part(c, ch, &b, 1, st);
    if (var == 2) {
        hipError_t e = hipSuccess;
        void *scr = scratch_get(c->scratch, kScrXr, xr_scratch_bytes(b.n, ch.nlinks), &e);
        if (e != hipSuccess) return scratch_error(c, e);
        ScratchUser use(c, c->xr, st);
        if (use.rc) return use.rc;
        PassMark m(c, 0, st);
        HIPCHK(c, launch_swipes_xr(ch, b.bytes, b.offs, b.fixed_w, b.slot, b.n, c->regs, c->nslots, b.out,
                                   scr, c->err, c->cus, 2, 1, st));
        m.end();
        return SKE_OK;
    }
    PassMark m(c, 0, st);
    HIPCHK(c, launch_swipes(0, ch, use_lds(c, ch), c->pb, b.bytes, b.offs, b.fixed_w, b.slot, b.n, c->regs,
                            c->nslots, b.out, (unsigned long long *)c->err, c->cus, st));
    m.end();
    return SKE_OK;
}

}  // namespace ske

// a batch of ske_swipes_many_async as K1's (width != 0: fixed-width ids, no offsets)
static PartBatch part_batch(const ske_swipe_batch &b) {
    return PartBatch{b.bytes, b.width ? nullptr : b.offs, b.width, b.slot, b.n, b.out_valid};
}

// Several resident batches in one call: batch j on branch j mod B, each branch
// a side stream forked from and joined back into the context stream (so the
// call also records into a graph).  With B > 1 the short-id K1 runs on one
// block per two CUs unless "k1_grid" is set, so two launches share the chip
// and one launch's fixed cost overlaps the other's steady state.
static int swipes_many_body(ske_ctx *c, const ChainDev &ch, const ske_swipe_batch *b, uint32_t nb, uint32_t br,
                            int grid) {
    const hipStream_t home = c->st;
    HIPCHK(c, hipEventRecord(c->many_fork, home));
    uint32_t forked = 0;
    int rc = SKE_OK;
    for (; forked + 1 < br; forked++) {
        hipError_t e = hipStreamWaitEvent(c->many_st[forked], c->many_fork, 0);
        if (e != hipSuccess) {
            c->last_hip = std::string("hipStreamWaitEvent(fork): ") + hipGetErrorString(e);
            rc = SKE_EHIP;
            break;
        }
    }
    for (uint32_t j = 0; j < nb && rc == SKE_OK; j++) {
        const uint32_t k = j % br;
        rc = launch_k1(c, ch, part_batch(b[j]), k ? c->many_st[k - 1] : home, grid);
    }
    // join every forked branch on every path (an unjoined side stream would
    // invalidate a capture, and outside one leave work the home stream does
    // not wait for); the first error is returned
    for (uint32_t i = 0; i < forked; i++) {
        hipError_t e = hipEventRecord(c->many_join[i], c->many_st[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(home, c->many_join[i], 0);
        if (e != hipSuccess && rc == SKE_OK) {
            c->last_hip = std::string("join: ") + hipGetErrorString(e);
            rc = SKE_EHIP;
        }
    }
    return rc;
}

static int swipes_many_persistent(ske_ctx *c, const K1Args &A, const ske_swipe_batch *b, uint32_t nb) {
    const uint32_t T = k1_many_tile(c->pb);
    for (uint32_t j0 = 0; j0 < nb; j0 += kK1ManyMax) {
        K1Many M{};
        M.nb = nb - j0 < kK1ManyMax ? nb - j0 : kK1ManyMax;
        M.tpre[0] = 0;
        for (uint32_t j = 0; j < M.nb; j++) {
            const PartBatch B = part_batch(b[j0 + j]);
            M.b[j] = K1Batch{B.bytes, B.offs, B.slot, B.out, uint32_t(B.n), B.fixed_w};
            const uint64_t tp = M.tpre[j] + (B.n + T - 1) / T;
            if (tp >= (uint64_t(1) << 31)) return SKE_EINVAL;
            M.tpre[j + 1] = uint32_t(tp);
        }
        PassMark m(c, 0, c->st);
        HIPCHK(c, launch_swipes_lds_many(A, M, c->pb, k1_grid(c), c->st));
        m.end();
    }
    return SKE_OK;
}

extern "C" {

int ske_swipes(ske_ctx *c, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
               const uint32_t *offs, uint64_t n, uint8_t *out_valid, int mem) {
    if (!c || !slot) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (const int erc = err_begin(c)) return erc;  // earlier enqueue-only calls' slot errors
    const bool fed = mem != SKE_MEM_DEVICE;  // pass kinds 6-8: the host-fed call's stages
    PassMark mcall, mh2d;
    if (fed) {
        mcall.begin(c, 8, c->st);
        mh2d.begin(c, 6, c->st);
    }
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    const uint32_t *dslot;
    rc = stage_u32(c, slot, n, mem, kStgSlots, &dslot);
    if (rc) return rc;
    mh2d.end();
    uint8_t *dout = out_valid;
    if (out_valid && fed) {
        dout = (uint8_t *)stage_buf(c, kStgOut, n, &rc);
        if (rc) return rc;
    }
    rc = launch_k1(c, chain_of(F), PartBatch{s.bytes, s.offs, 0, dslot, n, dout}, c->st, k1_grid(c));
    if (rc) return rc;
    if (out_valid && fed) {
        PassMark md2h(c, 7, c->st);
        HIPCHK(c, hipMemcpyAsync(out_valid, dout, n, hipMemcpyDeviceToHost, c->st));
        md2h.end();
    }
    mcall.end();
    return check_call_err(c);
}

int ske_swipes_async(ske_ctx *c, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                     const uint32_t *offs, uint64_t n, uint8_t *out_valid) {
    if (!c || !slot) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    return launch_k1(c, chain_of(F), PartBatch{bytes, offs, 0, slot, n, out_valid}, c->st, k1_grid(c));
}

int ske_swipes_many_async(ske_ctx *c, uint32_t fid, const ske_swipe_batch *b, uint32_t nb,
                          uint32_t branches) {
    if (!c || (nb && !b) || branches > SKE_MANY_MAX_BRANCHES) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    for (uint32_t j = 0; j < nb; j++)
        if (!b[j].slot || (b[j].width == 0 && !b[j].offs) || b[j].width > 4096) return SKE_EINVAL;
    const ChainDev &ch = chain_of(F);
    // the short-id LDS K1: one persistent launch per kK1ManyMax batches, the
    // branches unused
    if (nb && c->k1_persistent) {
        K1Args A;
        bool ok = true;
        for (uint32_t j = 0; j < nb && ok; j++) ok = k1_fast_args(c, ch, part_batch(b[j]), &A);
        if (ok) return swipes_many_persistent(c, A, b, nb);
    }
    // the partitioned K1: one call over every batch, before any branch
    // streams are made (it uses none; creating them lazily here cost ms of
    // host time per new count)
    const int var = nb ? k1_variant(c, ch) : 0;
    if (var == 3) {
        std::vector<PartBatch> pb(nb);
        for (uint32_t j = 0; j < nb; j++) pb[j] = part_batch(b[j]);
        return launch_part(c, ch, pb.data(), nb, c->st);
    }
    uint32_t br = branches ? branches : SKE_MANY_DEFAULT_BRANCHES;
    if (nb && br > nb) br = nb;
    if (br > 1) {  // with nb == 0: only prepares the side streams (e.g. before capture)
        if (!c->many_fork) HIPCHK(c, hipEventCreateWithFlags(&c->many_fork, hipEventDisableTiming));
        while (c->many_n < int(br) - 1) {
            HIPCHK(c, hipStreamCreateWithFlags(&c->many_st[c->many_n], hipStreamNonBlocking));
            HIPCHK(c, hipEventCreateWithFlags(&c->many_join[c->many_n], hipEventDisableTiming));
            c->many_n++;
        }
    }
    if (nb == 0) return SKE_OK;
    // the scratch of the largest batch before the first launch: batches of
    // different sizes never reallocate it between recorded launches
    uint64_t nmax = 0;
    for (uint32_t j = 0; j < nb; j++) nmax = b[j].n > nmax ? b[j].n : nmax;
    if (var == 2 && nmax) {
        hipError_t e = hipSuccess;
        (void)scratch_get(c->scratch, kScrXr, xr_scratch_bytes(nmax, ch.nlinks), &e);
        if (e != hipSuccess) return scratch_error(c, e);
    }
    if (br == 1) {
        for (uint32_t j = 0; j < nb; j++) {
            int rc = launch_k1(c, ch, part_batch(b[j]), c->st, k1_grid(c));
            if (rc) return rc;
        }
        return SKE_OK;
    }
    // (the branches' short-id K1: one block per two CUs unless "k1_grid" is set)
    return swipes_many_body(c, ch, b, nb, br, c->k1_grid ? c->k1_grid : c->cus / 2 > 0 ? c->cus / 2 : 1);
}

int ske_route_swipes(ske_ctx *c, const uint8_t *ids, uint32_t width, const uint32_t *gkey, uint64_t n,
                     uint32_t world, const uint32_t *key_owner, const uint32_t *key_local, uint32_t nkeys,
                     uint8_t *send_ids, uint32_t *send_slots, uint32_t *pos, uint64_t *counts) {
    if (!c || !counts || world == 0 || world > 64 || width == 0 || width > 4096 || n >= (uint64_t(1) << 32))
        return SKE_EINVAL;
    if (n && (!ids || !gkey || !send_ids || !send_slots || !pos)) return SKE_EINVAL;
    if (nkeys && (!key_owner || !key_local)) return SKE_EINVAL;
    hipError_t e = hipSuccess;
    uint32_t *hist = (uint32_t *)scratch_get(c->scratch, kScrRouteHist, route_hist_words(n, world) * 4 + 4, &e);
    uint32_t *tot = e == hipSuccess ? (uint32_t *)scratch_get(c->scratch, kScrRouteTot, size_t(world) * 4, &e) : nullptr;
    if (e != hipSuccess) return scratch_error(c, e);
    ScratchUser use(c, c->rt, c->st);  // an async routing call on another stream finishes first
    if (use.rc) return use.rc;
    HIPCHK(c, launch_route(ids, width, gkey, n, world, key_owner, key_local, nkeys, send_ids, send_slots, pos,
                           hist, tot, c->st));
    uint32_t h[64];
    HIPCHK(c, hipMemcpyAsync(h, tot, size_t(world) * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (uint32_t o = 0; o < world; o++) counts[o] = h[o];
    return SKE_OK;
}

int ske_route_swipes_cap_async(ske_ctx *c, const uint8_t *ids, uint32_t width, const uint32_t *gkey, uint64_t n,
                               uint32_t world, const uint32_t *key_route, uint32_t nkeys, uint32_t cap,
                               const uint32_t *sink_slots, uint8_t *send_ids, uint32_t *send_slots, uint32_t *pos,
                               uint32_t *counts) {
    if (!c || !counts || !sink_slots || world == 0 || world > 64 || width == 0 || width > 4096 ||
        n >= (uint64_t(1) << 32) || cap == 0 || uint64_t(cap) * world >= (uint64_t(1) << 32))
        return SKE_EINVAL;
    if (!send_ids || !send_slots || (n && (!ids || !gkey || !pos))) return SKE_EINVAL;
    if (nkeys && !key_route) return SKE_EINVAL;
    hipError_t e = hipSuccess;
    uint32_t *hist = (uint32_t *)scratch_get(c->scratch, kScrRouteHist, route_hist_words(n, world) * 4 + 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    // the histogram is context scratch of routing's own (kScrRouteHist; K1's
    // slots are another group): a routing call on another stream waits for
    // this one's kernels, a K1 does not -- the next batch's routing runs
    // beside this batch's K1 (distributed.SwipeExchange's pipelined form)
    ScratchUser use(c, c->rt, c->st);
    if (use.rc) return use.rc;
    const hipError_t le = launch_route_cap(ids, width, gkey, n, world, key_route, nkeys, cap, sink_slots, send_ids,
                                           send_slots, pos, hist, counts, c->cus, c->st);
    if (le != hipSuccess) {
        c->last_hip = std::string("launch_route_cap: ") + hipGetErrorString(le);
        return SKE_EHIP;
    }
    return SKE_OK;
}

int ske_route_slots_async(ske_ctx *c, const uint32_t *gkey, uint64_t n, const uint32_t *key_route, uint32_t nkeys,
                          uint32_t world, uint32_t *out_slots) {
    if (!c || world == 0 || world > 64 || (n && (!gkey || !out_slots)) || (!key_route && world != 1) ||
        (!key_route && nkeys > 0x3ffffffu))
        return SKE_EINVAL;
    HIPCHK(c, launch_route_slots(gkey, n, key_route, nkeys, world, out_slots, c->cus, c->st));
    return SKE_OK;
}

int ske_route_return_async(ske_ctx *c, const uint8_t *answers, const uint32_t *pos, uint64_t n, uint8_t *out) {
    if (!c || (n && (!answers || !pos || !out))) return SKE_EINVAL;
    HIPCHK(c, launch_route_return(answers, pos, n, out, c->cus, c->st));
    return SKE_OK;
}

int ske_swipes_fixed_async(ske_ctx *c, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                           uint32_t width, uint64_t n, uint8_t *out_valid) {
    if (!c || !slot || width == 0 || width > 4096) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    return launch_k1(c, chain_of(F), PartBatch{bytes, nullptr, width, slot, n, out_valid}, c->st, k1_grid(c));
}

int ske_swipes_fixed(ske_ctx *c, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                     uint32_t width, uint64_t n, uint8_t *out_valid, int mem) {
    if (!c || !slot || width == 0 || width > 4096) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (const int erc = err_begin(c)) return erc;  // earlier enqueue-only calls' slot errors
    int rc = SKE_OK;
    const uint8_t *db = bytes;
    const uint32_t *dslot = slot;
    uint8_t *dout = out_valid;
    if (mem != SKE_MEM_DEVICE) {
        uint8_t *b = (uint8_t *)stage_buf(c, kStgBytes, n * width + 16, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(b, bytes, n * width, hipMemcpyHostToDevice, c->st));
        db = b;
        rc = stage_u32(c, slot, n, mem, kStgSlots, &dslot);
        if (rc) return rc;
        if (out_valid) {
            dout = (uint8_t *)stage_buf(c, kStgOut, n, &rc);
            if (rc) return rc;
        }
    }
    rc = ske_swipes_fixed_async(c, fid, dslot, db, width, n, dout);
    if (rc) return rc;
    if (out_valid && mem != SKE_MEM_DEVICE)
        HIPCHK(c, hipMemcpyAsync(out_valid, dout, n, hipMemcpyDeviceToHost, c->st));
    return check_call_err(c);
}

// Fixed-width swipes with bit-packed answers.  Host inputs are cut into
// chunks of kFeedChunk swipes: the chunk's ids and slots go host -> device on
// a copy stream (sketch_host.cpp's pinned double buffer for pageable memory)
// while K1 runs on the previous chunk on the context stream; each chunk's
// answers are packed to bits on the device and copied back (1 bit per swipe).
// Per swipe the host link carries width + 4 bytes in and 1/8 byte out.
constexpr uint64_t kFeedChunk = uint64_t(4) << 20;

int ske_swipes_fixed_bits(ske_ctx *c, uint32_t fid, const uint32_t *slot, const uint8_t *bytes, uint32_t width,
                          uint64_t n, uint8_t *out_bits, int mem) {
    if (!c || !slot || !bytes || width == 0 || width > 4096) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (const int erc = err_begin(c)) return erc;  // earlier enqueue-only calls' slot errors
    int rc = SKE_OK;
    // the answers (bytes, 8-B aligned for the packer) always on the device
    uint8_t *dans = (uint8_t *)stage_buf(c, kStgAnswers, n + 16, &rc);
    if (rc) return rc;
    if (mem == SKE_MEM_DEVICE) {
        rc = ske_swipes_fixed_async(c, fid, slot, bytes, width, n, dans);
        if (rc) return rc;
        if (out_bits) HIPCHK(c, launch_pack_bits(dans, n, out_bits, c->cus, c->st));
        return check_call_err(c);
    }
    uint8_t *db = (uint8_t *)stage_buf(c, kStgBytes, n * width + 16, &rc);
    uint32_t *ds = rc ? nullptr : (uint32_t *)stage_buf(c, kStgSlots, n * 4 + 16, &rc);
    uint8_t *dbits = rc ? nullptr : (uint8_t *)stage_buf(c, kStgOut, (n + 7) / 8 + 16, &rc);
    if (rc) return rc;
    if (!c->copy_st) HIPCHK(c, hipStreamCreateWithFlags(&c->copy_st, hipStreamNonBlocking));
    if (!c->hs) c->hs = stager_new();
    const uint64_t nchunks = (n + kFeedChunk - 1) / kFeedChunk;
    while (c->chunk_ev.size() < nchunks) {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->chunk_ev.push_back(e);
    }
    // the copy stream starts behind everything already on the context stream
    // (earlier users of the staging buffers)
    PassMark mcall(c, 8, c->st);  // pass kinds 6-8: this host-fed call's stages
    HIPCHK(c, hipEventRecord(c->chunk_ev[0], c->st));
    HIPCHK(c, hipStreamWaitEvent(c->copy_st, c->chunk_ev[0], 0));
    // once a copy is queued, every exit waits for the copy stream first: the
    // DMA may still read the caller's (pinned) buffers
    auto chunks = [&]() -> int {
        for (uint64_t j = 0; j < nchunks; j++) {
            const uint64_t s0 = j * kFeedChunk, m = n - s0 < kFeedChunk ? n - s0 : kFeedChunk;
            PassMark mh2d(c, 6, c->copy_st);
            HIPCHK(c, stage_h2d(c->hs, db + s0 * width, bytes + s0 * width, m * width, c->copy_st, false, nullptr));
            HIPCHK(c, stage_h2d(c->hs, ds + s0, slot + s0, m * 4, c->copy_st, false, nullptr));
            mh2d.end();
            HIPCHK(c, hipEventRecord(c->chunk_ev[j], c->copy_st));
            HIPCHK(c, hipStreamWaitEvent(c->st, c->chunk_ev[j], 0));
            const int r = ske_swipes_fixed_async(c, fid, ds + s0, db + s0 * width, width, m, dans + s0);
            if (r) return r;
            if (out_bits) {
                HIPCHK(c, launch_pack_bits(dans + s0, m, dbits + s0 / 8, c->cus, c->st));
                PassMark md2h(c, 7, c->st);
                HIPCHK(c, hipMemcpyAsync(out_bits + s0 / 8, dbits + s0 / 8, (m + 7) / 8, hipMemcpyDeviceToHost, c->st));
                md2h.end();
            }
        }
        return SKE_OK;
    };
    rc = chunks();
    if (rc == SKE_OK) mcall.end();
    const hipError_t se = hipStreamSynchronize(c->copy_st);
    if (rc) return rc;
    HIPCHK(c, se);
    return check_call_err(c);
}

#ifdef SKE_STAMPS
// diagnostic build only: point the phase-stamp side buffer at dev_ptr
int ske_diag_set_stamp_buffer(ske_ctx *c, void *dev_ptr) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, ske::set_stamp_buffer(dev_ptr));
    return SKE_OK;
}
int ske_diag_set_pb_stamp_buffer(ske_ctx *c, void *dev_ptr) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, ske::set_pb_stamp_buffer(dev_ptr));
    return SKE_OK;
}
int ske_diag_set_k1_stamp_buffer(ske_ctx *c, void *dev_ptr) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, ske::set_k1_stamp_buffer(dev_ptr));
    return SKE_OK;
}
#endif
#ifdef SKE_SEG_STAMPS
int ske_diag_set_seg_stamp_buffer(ske_ctx *c, void *dev_ptr) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, ske::set_seg_stamp_buffer(dev_ptr));
    return SKE_OK;
}
#endif

int ske_swipes_stats(ske_ctx *c, uint32_t fid, const uint8_t *bytes, const uint32_t *offs,
                     uint64_t n, uint64_t *probes, uint64_t *nvalid) {
    if (!c || !probes || !nvalid) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    const ChainDev &ch = chain_of(F);
    HIPCHK(c, hipMemsetAsync(c->stats, 0, 16, c->st));
    // every tile size follows RedisBloom's per-swipe probe order, so the
    // count is the sequential one
    HIPCHK(c, launch_swipes(2, ch, use_lds(c, ch), c->pb, bytes, offs, 0, nullptr, n, nullptr, 0, nullptr,
                            c->stats, c->cus, c->st));
    unsigned long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, c->stats, 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *probes = h[0];
    *nvalid = h[1];
    return SKE_OK;
}

int ske_swipes_variant(ske_ctx *c, uint32_t fid) {
    Filter *F = c ? get_filter(c, fid) : nullptr;
    if (!F) return SKE_EINVAL;
    return k1_variant(c, chain_of(F));
}

}  // extern "C"
