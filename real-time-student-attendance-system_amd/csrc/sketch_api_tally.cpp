// sketch_api_tally.cpp -- libsketch C-ABI (include/sketch.h): tallies, the exact
// event counts per key (init, reset, info, the adds, query, list, top, import),
// kernels in sketch_tally.hip.  A tally is one device allocation owned by the
// context and addressed by tid.
#include <string.h>

#include <algorithm>
#include <new>

#include "sketch_ctx.h"

using namespace ske;

static_assert(kTallyKeyBytes == SKE_TALLY_KEY_BYTES && kTallyMaxProbes == SKE_TALLY_MAX_PROBES &&
                  kTallyLoadDen == SKE_TALLY_LOAD_DEN,
              "sketch.h states the kernels' bounds");
static_assert((1u << SKE_TALLY_MIN_LOG2) % 256 == 0, "k_tally_list covers the slots with whole blocks");
static_assert(SKE_MAX_TALLY == 256 && SKE_TALLY_MIN_LOG2 == 8 && SKE_TALLY_MAX_LOG2 == 24 && SKE_TALLY_MAX_TOP == 16,
              "the limits sketch.h states");
static_assert(sizeof(ske_tally_info_t) == 48, "six u64 words");
static_assert(SKE_ETALLYNOSET == -32 && SKE_ETALLYEXISTS == -33 && SKE_ETALLYCAP == -34 && SKE_ETALLYSPACE == -35,
              "the tally error codes");

namespace {

constexpr size_t kTallyHead = 64;       // used, overflow, taken, dropped_events, dropped_valid
constexpr size_t kTallySlotBytes = 60;  // claim 8, key 32, events 8, valid 8, length 4

struct TallyHeadHost {
    unsigned int used, overflow;
    unsigned long long taken, dropped_events, dropped_valid;
};

}  // namespace

static_assert(kTallyFamily.head_bytes == kTallyHead && kTallyFamily.slot_bytes == kTallySlotBytes, "the allocation");

static TallyTab tab_of(const Tally &Y) {
    const uint64_t cap = uint64_t(1) << Y.log2;
    TallyTab T{};
    T.used = reinterpret_cast<unsigned int *>(Y.base);
    T.overflow = T.used + 1;
    T.taken = reinterpret_cast<unsigned long long *>(Y.base + 8);
    T.dropped_events = T.taken + 1;
    T.dropped_valid = T.taken + 2;
    uint8_t *p = Y.base + kTallyHead;
    T.claim = reinterpret_cast<unsigned long long *>(p);
    T.keys = reinterpret_cast<uint64_t *>(p + cap * 8);
    T.events = reinterpret_cast<unsigned long long *>(p + cap * 40);
    T.valid = reinterpret_cast<unsigned long long *>(p + cap * 48);
    T.len = reinterpret_cast<uint32_t *>(p + cap * 56);
    T.mask = uint32_t(cap - 1);
    T.limit = uint32_t(cap / kTallyLoadDen);
    return T;
}

static int tally_launch(ske_ctx *c, const Tally &Y, const TallyItems &I) {
    HIPCHK(c, launch_tally_add(tab_of(Y), I, c->tally_form, unsigned(c->tally_grid), c->tally_lds_log2, c->cus, c->st));
    return SKE_OK;
}

namespace {

struct TallyEntry {
    uint8_t key[SKE_TALLY_KEY_BYTES];
    uint32_t len;
    uint64_t events, valid;
};

}  // namespace

// every entry with events >= min_events, unordered, on the host; *n_pass = how
// many pass (more than cap: v stays empty)
static int tally_fetch(ske_ctx *c, const Tally &Y, uint64_t min_events, uint64_t cap, std::vector<TallyEntry> *v,
                       uint64_t *n_pass, int *complete) {
    // the device side holds min(cap, capacity) entries: no more can pass
    const uint64_t slots = uint64_t(1) << Y.log2;
    const uint32_t dcap = uint32_t(cap < slots ? cap : slots);
    int rc = SKE_OK;
    unsigned int *cnt = (unsigned int *)stage_buf(c, kStgTallyFlag, 16, &rc);
    if (rc) return rc;
    uint64_t *d_keys = (uint64_t *)stage_buf(c, kStgTallyKeys, size_t(dcap) * 32 + 16, &rc);
    if (rc) return rc;
    uint32_t *d_len = (uint32_t *)stage_buf(c, kStgTallyLen, size_t(dcap) * 4 + 16, &rc);
    if (rc) return rc;
    uint64_t *d_ev = (uint64_t *)stage_buf(c, kStgTallyEv, size_t(dcap) * 8 + 16, &rc);
    if (rc) return rc;
    uint64_t *d_va = (uint64_t *)stage_buf(c, kStgTallyVa, size_t(dcap) * 8 + 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(cnt, 0, 16, c->st));
    HIPCHK(c, launch_tally_list(tab_of(Y), min_events, dcap, d_keys, d_len, d_ev, d_va, cnt, c->st));
    unsigned int n = 0;
    TallyHeadHost h{};
    HIPCHK(c, hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, c->st));
    rc = obj_read_head(c, Y, &h, sizeof h);
    if (rc) return rc;
    *n_pass = n;
    *complete = h.overflow == 0;
    v->clear();
    if (n > cap || n == 0) return SKE_OK;
    std::vector<uint64_t> ev, va;
    std::vector<uint32_t> lens;
    std::vector<uint8_t> keys;
    try {
        v->resize(n);
        keys.resize(size_t(n) * SKE_TALLY_KEY_BYTES);
        lens.resize(n);
        ev.resize(n);
        va.resize(n);
    } catch (const std::bad_alloc &) {
        return SKE_ENOMEM;
    }
    HIPCHK(c, hipMemcpyAsync(keys.data(), d_keys, keys.size(), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(lens.data(), d_len, size_t(n) * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(ev.data(), d_ev, size_t(n) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(va.data(), d_va, size_t(n) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    for (uint32_t i = 0; i < n; i++) {
        TallyEntry &e = (*v)[i];
        // little-endian words: the key bytes in order, zero padded
        memcpy(e.key, &keys[size_t(i) * SKE_TALLY_KEY_BYTES], SKE_TALLY_KEY_BYTES);
        e.len = lens[i];
        e.events = ev[i];
        e.valid = va[i];
    }
    return SKE_OK;
}

static bool entry_before(const TallyEntry &a, const TallyEntry &b, int by) {
    return tally_before(by ? a.valid : a.events, a.key, a.len, by ? b.valid : b.events, b.key, b.len);
}

static void entry_out(const TallyEntry &e, uint64_t at, uint8_t *keys, uint32_t *lens, uint64_t *events,
                      uint64_t *valid) {
    memcpy(keys + at * SKE_TALLY_KEY_BYTES, e.key, SKE_TALLY_KEY_BYTES);
    lens[at] = e.len;
    events[at] = e.events;
    valid[at] = e.valid;
}

extern "C" {

int ske_tally_init(ske_ctx *c, uint32_t tid, uint32_t capacity_log2) {
    Tally Y;
    Y.log2 = capacity_log2;
    return obj_alloc(c, kTallyFamily, c->tally, tid, Y, [c](const Tally &N) { return obj_zero(N, N.bytes, c->st); });
}

int ske_tally_free(ske_ctx *c, uint32_t tid) { return obj_release(c, kTallyFamily, c->tally, tid); }

int ske_tally_reset(ske_ctx *c, uint32_t tid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_reset", &rc);
    if (!Y) return rc;
    HIPCHK(c, obj_zero(*Y, Y->bytes, c->st));
    return SKE_OK;
}

int ske_tally_info(ske_ctx *c, uint32_t tid, ske_tally_info_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_info", &rc, kTallyFamily.info_refuses);
    if (!Y) return rc;
    TallyHeadHost h{};
    rc = obj_read_head(c, *Y, &h, sizeof h);
    if (rc) return rc;
    out->capacity = uint64_t(1) << Y->log2;
    out->used = h.used;
    out->overflow = h.overflow;
    out->taken = h.taken;
    out->dropped_events = h.dropped_events;
    out->dropped_valid = h.dropped_valid;
    return SKE_OK;
}

int ske_tally_add_packed_async(ske_ctx *c, uint32_t tid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                               const uint8_t *mask) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_get(kTallyFamily, c->tally, tid, &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!bytes || !offs) return SKE_EINVAL;
    TallyItems I{};
    I.kind = 0;
    I.bytes = bytes;
    I.offs = offs;
    I.n = uint32_t(n);
    I.mask = mask;
    return tally_launch(c, *Y, I);
}

int ske_tally_add_fixed_async(ske_ctx *c, uint32_t tid, const uint8_t *keys, uint32_t width, uint64_t n,
                              const uint8_t *mask) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_get(kTallyFamily, c->tally, tid, &rc);
    if (!Y) return rc;
    if (width == 0 || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys) return SKE_EINVAL;
    TallyItems I{};
    I.kind = 1;
    I.bytes = keys;
    I.fixed_w = width;
    I.n = uint32_t(n);
    I.mask = mask;
    return tally_launch(c, *Y, I);
}

int ske_tally_add_spans_async(ske_ctx *c, uint32_t tid, const uint8_t *bytes, const uint32_t *start,
                              const uint32_t *len, uint64_t n, const uint8_t *status, const uint8_t *mask) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_get(kTallyFamily, c->tally, tid, &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!bytes || !start || !len) return SKE_EINVAL;
    TallyItems I{};
    I.kind = 2;
    I.bytes = bytes;
    I.offs = start;
    I.len = len;
    I.status = status;
    I.n = uint32_t(n);
    I.mask = mask;
    return tally_launch(c, *Y, I);
}

int ske_tally_add(ske_ctx *c, uint32_t tid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                  const uint8_t *mask, int mem) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_add", &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!offs) return SKE_EINVAL;
    if (mem != SKE_MEM_DEVICE)
        for (uint64_t i = 0; i < n; i++)
            if (offs[i + 1] - offs[i] > SKE_TALLY_KEY_BYTES) return SKE_ETOOLONG;
    Staged s;
    rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    const uint8_t *d_mask = mask;
    if (mask && mem != SKE_MEM_DEVICE) {
        uint8_t *m = (uint8_t *)stage_buf(c, kStgTallyMask, n + 16, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(m, mask, n, hipMemcpyHostToDevice, c->st));
        d_mask = m;
    }
    unsigned int *flag = (unsigned int *)stage_buf(c, kStgTallyFlag, 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(flag, 0, 16, c->st));
    TallyItems I{};
    I.kind = 0;
    I.bytes = s.bytes;
    I.offs = s.offs;
    I.n = uint32_t(n);
    I.mask = d_mask;
    I.toolong = flag;
    rc = tally_launch(c, *Y, I);
    if (rc) return rc;
    unsigned int toolong = 0;
    HIPCHK(c, hipMemcpyAsync(&toolong, flag, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return toolong ? SKE_ETOOLONG : SKE_OK;
}

int ske_tally_query(ske_ctx *c, uint32_t tid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                    uint64_t *events_out, uint64_t *valid_out, int mem) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_query", &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!offs || !events_out || !valid_out) return SKE_EINVAL;
    Staged s;
    rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    uint64_t *d_ev = events_out, *d_va = valid_out;
    if (mem != SKE_MEM_DEVICE) {
        d_ev = (uint64_t *)stage_buf(c, kStgTallyEv, n * 8, &rc);
        if (rc) return rc;
        d_va = (uint64_t *)stage_buf(c, kStgTallyVa, n * 8, &rc);
        if (rc) return rc;
    }
    TallyItems I{};
    I.kind = 0;
    I.bytes = s.bytes;
    I.offs = s.offs;
    I.n = uint32_t(n);
    HIPCHK(c, launch_tally_query(tab_of(*Y), I, d_ev, d_va, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(events_out, d_ev, n * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(valid_out, d_va, n * 8, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tally_list(ske_ctx *c, uint32_t tid, uint64_t min_events, uint8_t *out_keys, uint32_t *out_lens,
                   uint64_t *out_events, uint64_t *out_valid, uint64_t cap, uint64_t *n_out, int *complete) {
    if (!c || !n_out || !complete) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_list", &rc);
    if (!Y) return rc;
    if (cap && (!out_keys || !out_lens || !out_events || !out_valid)) return SKE_EINVAL;
    std::vector<TallyEntry> v;
    rc = tally_fetch(c, *Y, min_events, cap, &v, n_out, complete);
    if (rc) return rc;
    if (*n_out > cap) return SKE_ETALLYSPACE;
    std::sort(v.begin(), v.end(), [](const TallyEntry &a, const TallyEntry &b) { return entry_before(a, b, 0); });
    for (size_t i = 0; i < v.size(); i++) entry_out(v[i], i, out_keys, out_lens, out_events, out_valid);
    return SKE_OK;
}

// The two ends of the listing's order.  The entries come from the device
// unordered; the 2k that are returned are selected here (two partial sorts),
// the rest is never ordered.
int ske_tally_top(ske_ctx *c, uint32_t tid, uint32_t k, int by, uint8_t *head_keys, uint32_t *head_lens,
                  uint64_t *head_events, uint64_t *head_valid, uint8_t *tail_keys, uint32_t *tail_lens,
                  uint64_t *tail_events, uint64_t *tail_valid, uint64_t *n_out, int *complete) {
    if (!c || !n_out || !complete) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_top", &rc);
    if (!Y) return rc;
    if (k == 0 || k > SKE_TALLY_MAX_TOP || (by != 0 && by != 1)) return SKE_EINVAL;
    if (!head_keys || !head_lens || !head_events || !head_valid || !tail_keys || !tail_lens || !tail_events ||
        !tail_valid)
        return SKE_EINVAL;
    std::vector<TallyEntry> v;
    uint64_t n = 0;
    rc = tally_fetch(c, *Y, 0, uint64_t(1) << Y->log2, &v, &n, complete);
    if (rc) return rc;
    const size_t m = v.size() < k ? v.size() : k;
    *n_out = m;
    if (m == 0) return SKE_OK;
    const auto first = [by](const TallyEntry &a, const TallyEntry &b) { return entry_before(a, b, by); };
    const auto last = [by](const TallyEntry &a, const TallyEntry &b) { return entry_before(b, a, by); };
    std::partial_sort(v.begin(), v.begin() + m, v.end(), first);
    for (size_t i = 0; i < m; i++) entry_out(v[i], i, head_keys, head_lens, head_events, head_valid);
    std::partial_sort(v.begin(), v.begin() + m, v.end(), last);
    for (size_t i = 0; i < m; i++) entry_out(v[m - 1 - i], i, tail_keys, tail_lens, tail_events, tail_valid);
    return SKE_OK;
}

int ske_tally_import(ske_ctx *c, uint32_t tid, const uint8_t *keys, const uint32_t *lens, const uint64_t *events,
                     const uint64_t *valid, uint64_t n) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_import", &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys || !lens || !events || !valid) return SKE_EINVAL;
    for (uint64_t i = 0; i < n; i++) {
        if (lens[i] > SKE_TALLY_KEY_BYTES) return SKE_ETOOLONG;
        if (valid[i] > events[i]) return SKE_EINVAL;
        for (uint32_t j = lens[i]; j < SKE_TALLY_KEY_BYTES; j++)  // the padding takes part in the digest
            if (keys[i * SKE_TALLY_KEY_BYTES + j]) return SKE_EINVAL;
    }
    uint8_t *d_keys = (uint8_t *)stage_buf(c, kStgTallyKeys, n * 32 + 16, &rc);
    if (rc) return rc;
    uint32_t *d_len = (uint32_t *)stage_buf(c, kStgTallyLen, n * 4 + 16, &rc);
    if (rc) return rc;
    uint64_t *d_ev = (uint64_t *)stage_buf(c, kStgTallyEv, n * 8 + 16, &rc);
    if (rc) return rc;
    uint64_t *d_va = (uint64_t *)stage_buf(c, kStgTallyVa, n * 8 + 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_keys, keys, n * 32, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(d_len, lens, n * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(d_ev, events, n * 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(d_va, valid, n * 8, hipMemcpyHostToDevice, c->st));
    TallyItems I{};
    I.kind = 3;
    I.bytes = d_keys;
    I.len = d_len;
    I.ev = d_ev;
    I.va = d_va;
    I.n = uint32_t(n);
    rc = tally_launch(c, *Y, I);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tally_export_dev(ske_ctx *c, uint32_t tid, uint8_t *keys_dev, uint32_t *lens_dev, uint64_t *events_dev,
                         uint64_t *valid_dev, uint64_t cap, uint64_t *n_out) {
    if (!c || !n_out) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_for_sync_call(c, kTallyFamily, c->tally, tid, "ske_tally_export_dev", &rc);
    if (!Y) return rc;
    if (cap && (!keys_dev || !lens_dev || !events_dev || !valid_dev || (reinterpret_cast<uintptr_t>(keys_dev) & 7)))
        return SKE_EINVAL;
    // no more than the capacity can pass
    const uint64_t slots = uint64_t(1) << Y->log2;
    const uint32_t dcap = uint32_t(cap < slots ? cap : slots);
    unsigned int *cnt = (unsigned int *)stage_buf(c, kStgTallyFlag, 16, &rc);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(cnt, 0, 16, c->st));
    HIPCHK(c, launch_tally_list(tab_of(*Y), 0, dcap, reinterpret_cast<uint64_t *>(keys_dev), lens_dev, events_dev,
                                valid_dev, cnt, c->st));
    unsigned int n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, cnt, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *n_out = n;
    return n > cap ? SKE_ETALLYSPACE : SKE_OK;
}

int ske_tally_merge_dev(ske_ctx *c, uint32_t tid, const uint8_t *keys_dev, const uint32_t *lens_dev,
                        const uint64_t *events_dev, const uint64_t *valid_dev, uint64_t n, uint64_t dropped_events,
                        uint64_t dropped_valid, uint32_t foreign_overflow) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tally *Y = obj_get(kTallyFamily, c->tally, tid, &rc);
    if (!Y) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n && (!keys_dev || !lens_dev || !events_dev || !valid_dev || (reinterpret_cast<uintptr_t>(keys_dev) & 7)))
        return SKE_EINVAL;
    if (n) {
        TallyItems I{};
        I.kind = 3;
        I.bytes = keys_dev;
        I.len = lens_dev;
        I.ev = events_dev;
        I.va = valid_dev;
        I.n = uint32_t(n);
        const int rc = tally_launch(c, *Y, I);
        if (rc) return rc;
    }
    HIPCHK(c, launch_tally_head_add(tab_of(*Y), dropped_events, dropped_valid, foreign_overflow, c->st));
    return SKE_OK;
}

}  // extern "C"
