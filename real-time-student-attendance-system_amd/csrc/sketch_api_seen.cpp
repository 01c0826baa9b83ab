// sketch_api_seen.cpp -- libsketch C-ABI (include/sketch.h): seen-row sets, the
// exact insert-only sets of 128-bit row keys (init, reset, info, the folds that
// build the keys, add, test), kernels in sketch_seen.hip.  A set is one device
// allocation owned by the context and addressed by sid.
#include <string.h>

#include "sketch_ctx.h"

using namespace ske;

static_assert(kSeenMaxProbes == SKE_SEEN_MAX_PROBES && kSeenLoadDen == SKE_SEEN_LOAD_DEN,
              "sketch.h states the kernels' bounds");
static_assert(kSeenFirst == SKE_SEEN_FIRST && kSeenRepeat == SKE_SEEN_REPEAT && kSeenSkipped == SKE_SEEN_SKIPPED,
              "sketch.h states the answer bytes");
static_assert(SKE_MAX_SEEN == 256 && SKE_SEEN_MIN_LOG2 == 8 && SKE_SEEN_MAX_LOG2 == 30, "the limits sketch.h states");
static_assert(sizeof(ske_seen_info_t) == 56, "seven u64 words");
static_assert(SKE_ESEENNOSET == -37 && SKE_ESEENEXISTS == -38 && SKE_ESEENCAP == -39 && SKE_ESEENCALLS == -40,
              "the seen-set error codes");

namespace {

constexpr size_t kSeenHeadBytes = 64;
constexpr size_t kSeenSlotBytes = 24;  // w0, w1, stamp
static_assert(sizeof(SeenHead) <= kSeenHeadBytes, "the head fits its 64 bytes");

}  // namespace

static_assert(kSeenFamily.head_bytes == kSeenHeadBytes && kSeenFamily.slot_bytes == kSeenSlotBytes, "the allocation");

static SeenTab tab_of(const Seen &S) {
    const uint64_t cap = uint64_t(1) << S.log2;
    SeenTab T{};
    T.head = reinterpret_cast<SeenHead *>(S.base);
    uint8_t *p = S.base + kSeenHeadBytes;
    T.w0 = reinterpret_cast<unsigned long long *>(p);
    T.w1 = reinterpret_cast<unsigned long long *>(p + cap * 8);
    T.stamp = reinterpret_cast<unsigned long long *>(p + cap * 16);
    T.mask = uint32_t(cap - 1);
    T.limit = uint32_t(seen_limit(S.log2));
    return T;
}

// an empty set: the head and the key words zero, every stamp all ones
static hipError_t seen_clear(const Seen &S, hipStream_t st) {
    const size_t cap = size_t(1) << S.log2;
    hipError_t e = hipMemsetAsync(S.base, 0, kSeenHeadBytes + cap * 16, st);
    if (e == hipSuccess) e = hipMemsetAsync(S.base + kSeenHeadBytes + cap * 16, 0xff, cap * 8, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the walk, the answers and the bump on the context stream; the per-item slots
// are context scratch, ordered behind the previous add's on another stream
static int seen_enqueue_add(ske_ctx *c, Seen &S, const uint64_t *keys, uint64_t n, const uint8_t *mask, int want,
                            uint8_t *out) {
    if (S.calls_host >= kSeenLastCall) return SKE_ESEENCALLS;
    ScratchUser use(c, c->sn, c->st);
    if (use.rc) return use.rc;
    hipError_t e = hipSuccess;
    uint32_t *slot = (uint32_t *)scratch_get(c->scratch, kScrSeenSlot, n * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    HIPCHK(c, launch_seen_add(tab_of(S), keys, uint32_t(n), mask, uint32_t(want), slot, out, unsigned(c->seen_grid),
                              c->cus, c->st));
    S.calls_host++;
    return SKE_OK;
}

static int fold_args(ske_ctx *c, const uint64_t *keys, uint64_t n) {
    if (!c || n >= 0xffffffffull) return SKE_EINVAL;
    if (n && (!keys || !aligned16(keys))) return SKE_EINVAL;
    return SKE_OK;
}

static int fold_launch(ske_ctx *c, uint64_t *keys, const SeenCol &C, int begin) {
    HIPCHK(c, launch_seen_fold(keys, C, begin != 0, unsigned(c->seen_grid), c->cus, c->st));
    return SKE_OK;
}

extern "C" {

int ske_seen_init(ske_ctx *c, uint32_t sid, uint32_t capacity_log2) {
    Seen S;
    S.log2 = capacity_log2;
    return obj_alloc(c, kSeenFamily, c->seen, sid, S, [c](const Seen &N) { return seen_clear(N, c->st); });
}

int ske_seen_free(ske_ctx *c, uint32_t sid) { return obj_release(c, kSeenFamily, c->seen, sid); }

int ske_seen_reset(ske_ctx *c, uint32_t sid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_for_sync_call(c, kSeenFamily, c->seen, sid, "ske_seen_reset", &rc);
    if (!S) return rc;
    HIPCHK(c, seen_clear(*S, c->st));
    S->calls_host = 0;
    return SKE_OK;
}

int ske_seen_info(ske_ctx *c, uint32_t sid, ske_seen_info_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_for_sync_call(c, kSeenFamily, c->seen, sid, "ske_seen_info", &rc, kSeenFamily.info_refuses);
    if (!S) return rc;
    SeenHead h{};
    rc = obj_read_head(c, *S, &h, sizeof h);
    if (rc) return rc;
    S->calls_host = h.calls;  // recorded graphs' replays included
    out->capacity = uint64_t(1) << S->log2;
    out->limit = seen_limit(S->log2);
    out->used = h.used;
    out->calls = h.calls;
    out->looked_at = h.looked_at;
    out->first = h.first;
    out->unplaced = h.unplaced;
    return SKE_OK;
}

int ske_seen_fold_packed_async(ske_ctx *c, uint64_t *keys, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                               int begin) {
    const int rc = fold_args(c, keys, n);
    if (rc || n == 0) return rc;
    if (!bytes || !offs) return SKE_EINVAL;
    SeenCol C{};
    C.kind = 0;
    C.bytes = bytes;
    C.offs = offs;
    C.n = uint32_t(n);
    return fold_launch(c, keys, C, begin);
}

int ske_seen_fold_fixed_async(ske_ctx *c, uint64_t *keys, const uint8_t *bytes, uint32_t width, uint64_t n,
                              int begin) {
    const int rc = fold_args(c, keys, n);
    if (rc || n == 0) return rc;
    if (!bytes && width) return SKE_EINVAL;
    SeenCol C{};
    C.kind = 1;
    C.bytes = bytes ? bytes : c->zero16;  // width 0: the empty column, no byte is read
    C.fixed_w = width;
    C.n = uint32_t(n);
    return fold_launch(c, keys, C, begin);
}

int ske_seen_fold_spans_async(ske_ctx *c, uint64_t *keys, const uint8_t *bytes, const uint32_t *start,
                              const uint32_t *len, const uint32_t *at, uint64_t n, int begin) {
    const int rc = fold_args(c, keys, n);
    if (rc || n == 0) return rc;
    if (!bytes || !start || !len) return SKE_EINVAL;
    SeenCol C{};
    C.kind = 2;
    C.bytes = bytes;
    C.offs = start;
    C.len = len;
    C.at = at;
    C.n = uint32_t(n);
    return fold_launch(c, keys, C, begin);
}

int ske_seen_fold_epoch_async(ske_ctx *c, uint64_t *keys, const int64_t *epoch, int64_t granularity, uint64_t n,
                              int begin) {
    const int rc = fold_args(c, keys, n);
    if (rc) return rc;
    if (granularity < 1) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!epoch || (reinterpret_cast<uintptr_t>(epoch) & 7)) return SKE_EINVAL;
    SeenCol C{};
    C.kind = 3;
    C.epoch = epoch;
    C.granularity = granularity;
    C.n = uint32_t(n);
    return fold_launch(c, keys, C, begin);
}

int ske_seen_add_async(ske_ctx *c, uint32_t sid, const uint64_t *keys, uint64_t n, const uint8_t *mask, int want,
                       uint8_t *out) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_get(kSeenFamily, c->seen, sid, &rc);
    if (!S) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys || !out || !aligned16(keys)) return SKE_EINVAL;
    return seen_enqueue_add(c, *S, keys, n, mask, want, out);
}

int ske_seen_test_async(ske_ctx *c, uint32_t sid, const uint64_t *keys, uint64_t n, uint8_t *present_out) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_get(kSeenFamily, c->seen, sid, &rc);
    if (!S) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys || !present_out || !aligned16(keys)) return SKE_EINVAL;
    HIPCHK(c, launch_seen_test(tab_of(*S), keys, uint32_t(n), present_out, unsigned(c->seen_grid), c->cus, c->st));
    return SKE_OK;
}

int ske_seen_add(ske_ctx *c, uint32_t sid, const uint64_t *keys, uint64_t n, const uint8_t *mask, int want,
                 uint8_t *out, int mem) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_for_sync_call(c, kSeenFamily, c->seen, sid, "ske_seen_add", &rc);
    if (!S) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys || !out) return SKE_EINVAL;
    const uint64_t *d_keys = keys;
    const uint8_t *d_mask = mask;
    uint8_t *d_out = out;
    if (mem != SKE_MEM_DEVICE) {
        uint64_t *k = (uint64_t *)stage_buf(c, kStgSeenKeys, n * 16, &rc);
        if (rc) return rc;
        d_out = (uint8_t *)stage_buf(c, kStgSeenOut, n + 16, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(k, keys, n * 16, hipMemcpyHostToDevice, c->st));
        d_keys = k;
        if (mask) {
            uint8_t *m = (uint8_t *)stage_buf(c, kStgSeenMask, n + 16, &rc);
            if (rc) return rc;
            HIPCHK(c, hipMemcpyAsync(m, mask, n, hipMemcpyHostToDevice, c->st));
            d_mask = m;
        }
    } else if (!aligned16(keys)) {
        return SKE_EINVAL;
    }
    rc = seen_enqueue_add(c, *S, d_keys, n, d_mask, want, d_out);
    if (rc) return rc;
    if (mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_seen_test(ske_ctx *c, uint32_t sid, const uint64_t *keys, uint64_t n, uint8_t *present_out, int mem) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Seen *S = obj_for_sync_call(c, kSeenFamily, c->seen, sid, "ske_seen_test", &rc);
    if (!S) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!keys || !present_out) return SKE_EINVAL;
    const uint64_t *d_keys = keys;
    uint8_t *d_out = present_out;
    if (mem != SKE_MEM_DEVICE) {
        uint64_t *k = (uint64_t *)stage_buf(c, kStgSeenKeys, n * 16, &rc);
        if (rc) return rc;
        d_out = (uint8_t *)stage_buf(c, kStgSeenOut, n + 16, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(k, keys, n * 16, hipMemcpyHostToDevice, c->st));
        d_keys = k;
    } else if (!aligned16(keys)) {
        return SKE_EINVAL;
    }
    HIPCHK(c, launch_seen_test(tab_of(*S), d_keys, uint32_t(n), d_out, unsigned(c->seen_grid), c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(present_out, d_out, n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

}  // extern "C"
