// sketch_api_hh.cpp -- libsketch C-ABI (include/sketch.h): heavy-hitter sets
// beside a Count-Min Sketch table (init, reset, info, track, list: kernels in
// sketch_hh.hip; stats, select: sketch_hh_stats.hip).  A set holds no pointer to
// a table: every track, list, stats and select looks the table up by cid, so a
// freed table is an error, never a stale pointer.
#include <string.h>

#include <algorithm>
#include <new>

#include "sketch_ctx.h"

using namespace ske;

static_assert(kHhMaxProbes == SKE_HH_MAX_PROBES && kHhLoadDen == SKE_HH_LOAD_DEN, "sketch.h states the kernels' bounds");
static_assert((1u << SKE_HH_MIN_LOG2) % 256 == 0, "k_hh_list and k_hhs_est cover the slots with whole blocks");
static_assert(kHhStatRanks == SKE_HH_MAX_RANKS && sizeof(ske_hh_stats_t) == 56, "sketch.h states the select's ranks");

// the set of a hid in use, else nullptr (SKE_EHHNOSET: a hid is not range-checked, kHhFamily)
static Hh *get_hh(ske_ctx *c, uint32_t hid) {
    int rc = SKE_OK;
    return obj_get(kHhFamily, c->hh, hid, &rc);
}

static HhSet set_of(const Hh &H) {
    const uint64_t cap = uint64_t(1) << H.log2;
    HhSet S{};
    S.used = reinterpret_cast<unsigned int *>(H.base);
    S.overflow = S.used + 1;
    S.claim = reinterpret_cast<unsigned long long *>(H.base + 16);
    S.ids = reinterpret_cast<uint64_t *>(H.base + 16 + cap * 8);
    S.len = reinterpret_cast<uint32_t *>(H.base + 16 + cap * 24);
    S.mask = uint32_t(cap - 1);
    S.limit = uint32_t(cap / kHhLoadDen);
    return S;
}

static bool hh_use_lds(const ske_ctx *c, const Cms &T) { return uint64_t(T.width) * T.depth <= c->hh_lds_cells; }

extern "C" {

int ske_hh_init(ske_ctx *c, uint32_t hid, uint32_t capacity_log2) {
    Hh H;
    H.log2 = capacity_log2;
    return obj_alloc(c, kHhFamily, c->hh, hid, H, [c](const Hh &N) { return obj_zero(N, N.bytes, c->st); });
}

int ske_hh_free(ske_ctx *c, uint32_t hid) { return obj_release(c, kHhFamily, c->hh, hid); }

int ske_hh_reset(ske_ctx *c, uint32_t hid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Hh *H = obj_for_sync_call(c, kHhFamily, c->hh, hid, "ske_hh_reset", &rc);
    if (!H) return rc;
    HIPCHK(c, obj_zero(*H, H->bytes, c->st));
    return SKE_OK;
}

int ske_hh_info(ske_ctx *c, uint32_t hid, ske_hh_info_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Hh *H = obj_for_sync_call(c, kHhFamily, c->hh, hid, "ske_hh_info", &rc, kHhFamily.info_refuses);
    if (!H) return rc;
    unsigned int head[2] = {0, 0};
    rc = obj_read_head(c, *H, head, 8);
    if (rc) return rc;
    out->capacity = uint64_t(1) << H->log2;
    out->used = head[0];
    out->overflow = head[1];
    return SKE_OK;
}

int ske_hh_track_fixed_async(ske_ctx *c, uint32_t hid, uint32_t cid, const uint8_t *ids, uint32_t width, uint64_t n,
                             const uint8_t *mask, int want, uint32_t threshold) {
    if (!c) return SKE_EINVAL;
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (width > SKE_HH_ID_BYTES) return SKE_ETOOLONG;
    if (threshold == 0 || width == 0 || (want != 0 && want != 1) || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!ids) return SKE_EINVAL;
    CmsItems I{};
    I.bytes = ids;
    I.fixed_w = width;
    I.n = uint32_t(n);
    I.mask = mask;
    I.want = uint32_t(want);
    HIPCHK(c, launch_hh_track(table_of(*T), I, set_of(*H), threshold, hh_use_lds(c, *T), nullptr, c->cus, c->st));
    return SKE_OK;
}

int ske_hh_track_packed_async(ske_ctx *c, uint32_t hid, uint32_t cid, const uint8_t *bytes, const uint32_t *offs,
                              uint64_t n, const uint8_t *mask, int want, uint32_t threshold) {
    if (!c) return SKE_EINVAL;
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (threshold == 0 || (want != 0 && want != 1) || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!bytes || !offs) return SKE_EINVAL;
    CmsItems I{};
    I.bytes = bytes;
    I.offs = offs;
    I.n = uint32_t(n);
    I.mask = mask;
    I.want = uint32_t(want);
    // an id longer than SKE_HH_ID_BYTES is skipped and is a refused insert: the
    // kernel's too-long word is the set's sticky overflow word
    const HhSet S = set_of(*H);
    HIPCHK(c, launch_hh_track(table_of(*T), I, S, threshold, hh_use_lds(c, *T), S.overflow, c->cus, c->st));
    return SKE_OK;
}

int ske_hh_track(ske_ctx *c, uint32_t hid, uint32_t cid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                 uint32_t threshold, int mem) {
    if (!c) return SKE_EINVAL;
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (threshold == 0 || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!offs) return SKE_EINVAL;
    if (mem != SKE_MEM_DEVICE)
        for (uint64_t i = 0; i < n; i++)
            if (offs[i + 1] - offs[i] > SKE_HH_ID_BYTES) return SKE_ETOOLONG;
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    unsigned int *flag = (unsigned int *)stage_buf(c, kStgHhFlag, 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(flag, 0, 16, c->st));
    CmsItems I{};
    I.bytes = s.bytes;
    I.offs = s.offs;
    I.n = uint32_t(n);
    HIPCHK(c, launch_hh_track(table_of(*T), I, set_of(*H), threshold, hh_use_lds(c, *T), flag, c->cus, c->st));
    unsigned int toolong = 0;
    HIPCHK(c, hipMemcpyAsync(&toolong, flag, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return toolong ? SKE_ETOOLONG : SKE_OK;
}

int ske_hh_list(ske_ctx *c, uint32_t hid, uint32_t cid, uint32_t threshold, uint8_t *out_ids, uint32_t *out_lens,
                uint32_t *out_est, uint64_t cap, uint64_t *n_out, int *complete) {
    if (!c || !n_out || !complete) return SKE_EINVAL;
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (cap && (!out_ids || !out_lens || !out_est)) return SKE_EINVAL;
    // the device side holds min(cap, capacity) entries: no more can pass
    const uint64_t slots = uint64_t(1) << H->log2;
    const uint32_t dcap = uint32_t(cap < slots ? cap : slots);
    int rc = SKE_OK;
    unsigned int *cnt = (unsigned int *)stage_buf(c, kStgHhFlag, 16, &rc);
    if (rc) return rc;
    uint64_t *d_ids = (uint64_t *)stage_buf(c, kStgHhIds, size_t(dcap) * 16 + 16, &rc);
    if (rc) return rc;
    uint32_t *d_len = (uint32_t *)stage_buf(c, kStgHhLen, size_t(dcap) * 4 + 16, &rc);
    if (rc) return rc;
    uint32_t *d_est = (uint32_t *)stage_buf(c, kStgHhEst, size_t(dcap) * 4 + 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(cnt, 0, 16, c->st));
    HIPCHK(c, launch_hh_list(table_of(*T), set_of(*H), threshold, dcap, d_ids, d_len, d_est, cnt, c->st));
    unsigned int n = 0, head[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(head, H->base, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *n_out = n;
    *complete = head[1] == 0;
    if (n > cap) return SKE_EHHSPACE;
    if (n == 0) return SKE_OK;
    struct Entry {
        uint8_t id[SKE_HH_ID_BYTES];
        uint32_t len, est;
    };
    std::vector<Entry> v;
    std::vector<uint64_t> ids;
    std::vector<uint32_t> lens, est;
    try {
        v.resize(n);
        ids.resize(size_t(n) * 2);
        lens.resize(n);
        est.resize(n);
    } catch (const std::bad_alloc &) {
        return SKE_ENOMEM;
    }
    HIPCHK(c, hipMemcpyAsync(ids.data(), d_ids, size_t(n) * 16, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(lens.data(), d_len, size_t(n) * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(est.data(), d_est, size_t(n) * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (uint32_t i = 0; i < n; i++) {
        memcpy(v[i].id, &ids[2 * size_t(i)], 16);  // little-endian words: the id bytes in order, zero padded
        v[i].len = lens[i];
        v[i].est = est[i];
    }
    // estimate descending, then id bytes ascending (a prefix before its
    // extensions: the padding is zero, so the padded bytes decide all but that)
    std::sort(v.begin(), v.end(), [](const Entry &a, const Entry &b) {
        if (a.est != b.est) return a.est > b.est;
        const int k = memcmp(a.id, b.id, SKE_HH_ID_BYTES);
        return k ? k < 0 : a.len < b.len;
    });
    for (uint32_t i = 0; i < n; i++) {
        memcpy(out_ids + size_t(i) * SKE_HH_ID_BYTES, v[i].id, SKE_HH_ID_BYTES);
        out_lens[i] = v[i].len;
        out_est[i] = v[i].est;
    }
    return SKE_OK;
}

int ske_hh_export_dev(ske_ctx *c, uint32_t hid, uint8_t *ids_dev, uint32_t *lens_dev, uint64_t cap, uint64_t *n_out,
                      uint32_t *overflow_out) {
    if (!c || !n_out || !overflow_out) return SKE_EINVAL;
    int rc = SKE_OK;
    Hh *H = obj_for_sync_call(c, kHhFamily, c->hh, hid, "ske_hh_export_dev", &rc);
    if (!H) return rc;
    if (cap && (!ids_dev || !lens_dev || (reinterpret_cast<uintptr_t>(ids_dev) & 7))) return SKE_EINVAL;
    // no more than the capacity can pass
    const uint64_t slots = uint64_t(1) << H->log2;
    const uint32_t dcap = uint32_t(cap < slots ? cap : slots);
    unsigned int *cnt = (unsigned int *)stage_buf(c, kStgHhFlag, 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(cnt, 0, 16, c->st));
    HIPCHK(c, launch_hh_export(set_of(*H), dcap, reinterpret_cast<uint64_t *>(ids_dev), lens_dev, cnt, c->st));
    unsigned int n = 0, head[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(head, H->base, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *n_out = n;
    *overflow_out = head[1];
    return n > cap ? SKE_EHHSPACE : SKE_OK;
}

int ske_hh_merge_dev(ske_ctx *c, uint32_t hid, const uint8_t *ids_dev, const uint32_t *lens_dev, uint64_t n,
                     uint32_t foreign_overflow) {
    if (!c) return SKE_EINVAL;
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n && (!ids_dev || !lens_dev || (reinterpret_cast<uintptr_t>(ids_dev) & 7))) return SKE_EINVAL;
    HIPCHK(c, launch_hh_merge(set_of(*H), reinterpret_cast<const uint64_t *>(ids_dev), lens_dev, uint32_t(n),
                              foreign_overflow, c->cus, c->st));
    return SKE_OK;
}

}  // extern "C"

// ske_hh_stats and ske_hh_select: the record zeroed, the whole chain of
// kernels, one copy of the record's head, one wait.  R.n == 0: the medians.
static int hh_stats_run(ske_ctx *c, uint32_t hid, uint32_t cid, uint32_t threshold, const HhRanks &R,
                        HhStatDev *reply) {
    Hh *H = get_hh(c, hid);
    if (!H) return SKE_EHHNOSET;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (c->capturing) {
        c->last_hip = "ske_hh_stats / ske_hh_select wait for the stream and cannot be recorded";
        return SKE_EBUSY;
    }
    int rc = SKE_OK;
    HhStatDev *D = (HhStatDev *)stage_buf(c, kStgHhStat, sizeof(HhStatDev), &rc);
    if (rc) return rc;
    uint32_t *est = (uint32_t *)stage_buf(c, kStgHhSelEst, (size_t(1) << H->log2) * 4 + 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(D, 0, sizeof(HhStatDev), c->st));
    HIPCHK(c, launch_hh_stats(table_of(*T), set_of(*H), threshold, R, D, est, c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(reply, D, kHhStatReplyBytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

extern "C" {

int ske_hh_stats(ske_ctx *c, uint32_t hid, uint32_t cid, uint32_t threshold, ske_hh_stats_t *out) {
    if (!c || !out) return SKE_EINVAL;
    HhRanks R{};
    HhStatDev r{};
    const int rc = hh_stats_run(c, hid, cid, threshold, R, &r);
    if (rc) return rc;
    out->n = r.n;
    out->sum = r.sum;
    out->sq_lo = r.sq_lo;
    out->sq_hi = r.sq_hi;
    out->min = r.min;
    out->max = r.max;
    out->med_lo = r.prefix[0];
    out->med_hi = r.prefix[1];
    out->complete = r.complete;
    out->reserved = 0;
    return SKE_OK;
}

int ske_hh_select(ske_ctx *c, uint32_t hid, uint32_t cid, uint32_t threshold, const uint64_t *ranks, uint32_t nranks,
                  uint32_t *out_est, uint64_t *n_out) {
    if (!c || !ranks || !out_est || !n_out || nranks == 0 || nranks > SKE_HH_MAX_RANKS) return SKE_EINVAL;
    HhRanks R{};
    R.n = nranks;
    for (uint32_t j = 0; j < nranks; j++) R.r[j] = ranks[j];
    HhStatDev r{};
    const int rc = hh_stats_run(c, hid, cid, threshold, R, &r);
    if (rc) return rc;
    *n_out = r.n;
    if (r.bad) return SKE_EINVAL;
    for (uint32_t j = 0; j < nranks; j++) out_est[j] = r.prefix[j];
    return SKE_OK;
}

}  // extern "C"
