// sketch_api_rows.cpp -- libsketch C-ABI (include/sketch.h): row logs, the
// attendance table's rows in arrival order (init, reset, info, the three
// appends, select, group, profile, compact, read), kernels in sketch_rows.hip.  A log is one device
// allocation owned by the context and addressed by rid.  ske_rows_group_merge, which sums several
// group-bys' outputs, needs no log: caller arrays and context scratch.
#include <stddef.h>
#include <string.h>

#include "sketch_ctx.h"

using namespace ske;

static_assert(kRowsBlock == SKE_ROWS_BLOCK, "sketch.h states the append's tile");
static_assert(SKE_MAX_ROWS == 8 && SKE_ROWS_MIN_LOG2 >= SKE_SEEN_MIN_LOG2 && SKE_ROWS_MAX_LOG2 <= 28,
              "the limits sketch.h states; a position fits a u32");
static_assert(sizeof(ske_rows_info_t) == 48, "six u64 words");
static_assert(SKE_EROWSNOLOG == -42 && SKE_EROWSEXISTS == -43 && SKE_EROWSCAP == -44 && SKE_EROWSSPACE == -45,
              "the row-log error codes");
static_assert(SKE_ROWS_ROW_BYTES == 25, "three words and a byte");
static_assert(SKE_ROWS_BY_STUDENT == kRowsByStudent && SKE_ROWS_BY_LECTURE == kRowsByLecture &&
                  SKE_ROWS_VALID_ANY == kRowsValidAny && SKE_ROWS_VALID_ONLY == kRowsValidOnly &&
                  SKE_ROWS_INVALID_ONLY == kRowsInvalidOnly,
              "the group-by's selectors as sketch.h states them");
static_assert(sizeof(ske_rows_compact_t) == 32 && sizeof(RowsCompactCounts) == sizeof(ske_rows_compact_t),
              "four u64 words");
static_assert(sizeof(ske_rows_group_stats_t) == 64&& SKE_TP_BINS == kTpBins, "eight u64 words; the profile's bins");

namespace {

constexpr size_t kRowsHeadBytes = 64;
static_assert(sizeof(RowsHead) <= kRowsHeadBytes, "the head fits its 64 bytes");

}  // namespace

static_assert(kRowsFamily.head_bytes == kRowsHeadBytes, "the allocation");

static RowsLog log_of(const Rows &R) {
    const uint64_t cap = uint64_t(1) << R.log2;
    RowsLog L{};
    L.head = reinterpret_cast<RowsHead *>(R.base);
    uint8_t *p = R.base + kRowsHeadBytes;
    L.lec = reinterpret_cast<unsigned long long *>(p);
    L.epoch = reinterpret_cast<long long *>(p + cap * 8);
    L.id = reinterpret_cast<long long *>(p + cap * 16);
    L.valid = p + cap * 24;
    L.capacity = cap;
    return L;
}

// the four kernels on the context stream; the per-item state is context
// scratch, ordered behind the previous append's on another stream
static int rows_enqueue(ske_ctx *c, const Rows &R, RowsItems I) {
    ScratchUser use(c, c->rw, c->st);
    if (use.rc) return use.rc;
    hipError_t e = hipSuccess;
    RowsWork W{};
    W.flag = (uint8_t *)scratch_get(c->scratch, kScrRowsFlag, I.n, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    W.idv = (long long *)scratch_get(c->scratch, kScrRowsIdv, uint64_t(I.n) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    W.cnt = (uint32_t *)scratch_get(c->scratch, kScrRowsCnt, rows_cnt_bytes(I.n), &e);
    if (e != hipSuccess) return scratch_error(c, e);
    HIPCHK(c, launch_rows_append(log_of(R), I, W, unsigned(c->rows_grid), c->cus, c->st));
    return SKE_OK;
}

static int append_args(ske_ctx *c, uint32_t rid, uint64_t n, const int64_t *epoch, Rows **R) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    *R = obj_get(kRowsFamily, c->rows, rid, &rc);
    if (!*R) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n && (!epoch || (reinterpret_cast<uintptr_t>(epoch) & 7))) return SKE_EINVAL;
    return SKE_OK;
}

// What the select, the group-by and the profile share (steps 1 to 4): the
// window's positions, sorted with one stable pass per key column, and the flag
// of each run's last-appended row.
struct RowsFront {
    uint32_t m;     // rows in the window before the collapse
    uint32_t runs;  //   after it
    uint32_t *pos;  // m positions in sorted order
    RowsWork W;     // flag[j] = pos[j] survives; cnt: the flags' totals and scanned tile counts
};

// id_last: the id is the most significant column (epoch, lecture, id) -- the
// rows lie grouped by id, ascending and signed; else the table's order (lecture,
// epoch, id).  Equal (lecture, epoch, id) are adjacent either way, the
// last-appended row last.  *complete is written; F->m == 0: nothing matches.
static int rows_front(ske_ctx *c, const Rows &R, const uint8_t *lec_bytes, uint32_t lec_len, int64_t since,
                      int64_t until, bool id_last, int *complete, RowsFront *F) {
    RowsHead h{};
    int rc = obj_read_head(c, R, &h, sizeof h);
    if (rc) return rc;
    *complete = h.overflow ? 0 : 1;
    const uint32_t used = uint32_t(h.used);  // <= 2^28
    if (used == 0) return SKE_OK;
    const RowsLog L = log_of(R);
    const bool by_lec = lec_bytes != nullptr || lec_len != 0;
    if (lec_len && !lec_bytes) return SKE_EINVAL;
    const unsigned long long digest = by_lec ? rows_lecture_digest(lec_bytes, lec_len) : 0;

    hipError_t e = hipSuccess;
    RowsWork W{};
    W.flag = (uint8_t *)scratch_get(c->scratch, kScrRowsSelFlag, used, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    W.cnt = (uint32_t *)scratch_get(c->scratch, kScrRowsSelCnt, rows_cnt_bytes(used), &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *pos = (uint32_t *)scratch_get(c->scratch, kScrVals, uint64_t(used) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    const unsigned grid = unsigned(c->rows_grid);

    // 1, 2: the matching positions, ascending
    HIPCHK(c, launch_rows_match(L, used, by_lec, digest, since, until, W, pos, grid, c->cus, c->st));
    uint32_t m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, W.cnt, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (m == 0) return SKE_OK;

    // 3: one stable pass per column (0 id, 1 epoch, 2 lecture), the least significant first; one
    // lecture's rows need no lecture pass
    unsigned long long *keys = (unsigned long long *)scratch_get(c->scratch, kScrKeysOrFirst, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    unsigned long long *keys_s = (unsigned long long *)scratch_get(c->scratch, kScrKeysSorted, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *pos_s = (uint32_t *)scratch_get(c->scratch, kScrValsSorted, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *cur = pos, *nxt = pos_s;
    int order[3], passes = 0;
    if (id_last) {
        order[passes++] = 1;
        if (!by_lec) order[passes++] = 2;
        order[passes++] = 0;
    } else {
        order[passes++] = 0;
        order[passes++] = 1;
        if (!by_lec) order[passes++] = 2;
    }
    for (int k = 0; k < passes; k++) {
        const int col = order[k];
        HIPCHK(c, launch_rows_keys(L, cur, m, col, keys, grid, c->cus, c->st));
        e = rows_sort_pairs(c->scratch, col < 2, keys, keys_s, cur, nxt, m, c->st);
        if (e == hipErrorStreamCaptureUnsupported) return scratch_error(c, e);
        HIPCHK(c, e);
        uint32_t *t = cur;
        cur = nxt;
        nxt = t;
    }

    // 4: the last-appended row of each run of equal keys
    HIPCHK(c, launch_rows_last(L, cur, m, W, grid, c->cus, c->st));
    uint32_t runs = 0;
    HIPCHK(c, hipMemcpyAsync(&runs, W.cnt, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    F->m = m;
    F->runs = runs;
    F->pos = cur;
    F->W = W;
    return SKE_OK;
}

static bool rows_filter_ok(int valid_filter, uint32_t sod_from) {
    return valid_filter >= SKE_ROWS_VALID_ANY && valid_filter <= SKE_ROWS_INVALID_ONLY && sod_from <= kRowsSodMax;
}

extern "C" {

int ske_rows_init(ske_ctx *c, uint32_t rid, uint32_t capacity_log2) {
    Rows R;
    R.log2 = capacity_log2;
    // an empty log: the head zero (the columns are read below `used` only)
    return obj_alloc(c, kRowsFamily, c->rows, rid, R, [c](const Rows &N) { return obj_zero(N, kRowsHeadBytes, c->st); });
}

int ske_rows_free(ske_ctx *c, uint32_t rid) { return obj_release(c, kRowsFamily, c->rows, rid); }

int ske_rows_reset(ske_ctx *c, uint32_t rid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_reset", &rc);
    if (!R) return rc;
    HIPCHK(c, obj_zero(*R, kRowsHeadBytes, c->st));
    return SKE_OK;
}

int ske_rows_info(ske_ctx *c, uint32_t rid, ske_rows_info_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_info", &rc, kRowsFamily.info_refuses);
    if (!R) return rc;
    RowsHead h{};
    rc = obj_read_head(c, *R, &h, sizeof h);
    if (rc) return rc;
    out->capacity = uint64_t(1) << R->log2;
    out->used = h.used;
    out->taken = h.taken;
    out->refused_ids = h.refused_ids;
    out->dropped = h.dropped;
    out->overflow = h.overflow;
    return SKE_OK;
}

int ske_rows_append_packed_async(ske_ctx *c, uint32_t rid, const uint8_t *lec_bytes, const uint32_t *lec_offs,
                                 const uint8_t *id_bytes, const uint32_t *id_offs, const int64_t *epoch,
                                 const uint8_t *valid, const uint8_t *mask, uint64_t n) {
    Rows *R = nullptr;
    const int rc = append_args(c, rid, n, epoch, &R);
    if (rc || n == 0) return rc;
    if (!lec_bytes || !lec_offs || !id_bytes || !id_offs) return SKE_EINVAL;
    RowsItems I{};
    I.kind = 0;
    I.lec_bytes = lec_bytes;
    I.lec_offs = lec_offs;
    I.id_bytes = id_bytes;
    I.id_offs = id_offs;
    I.epoch = epoch;
    I.valid = valid;
    I.mask = mask;
    I.n = uint32_t(n);
    return rows_enqueue(c, *R, I);
}

int ske_rows_append_spans_async(ske_ctx *c, uint32_t rid, const uint8_t *bytes, const uint32_t *lec_start,
                                const uint32_t *lec_len, const uint32_t *id_start, const uint32_t *id_len,
                                const uint8_t *status, const int64_t *epoch, const uint8_t *valid,
                                const uint8_t *mask, uint64_t n) {
    Rows *R = nullptr;
    const int rc = append_args(c, rid, n, epoch, &R);
    if (rc || n == 0) return rc;
    if (!bytes || !lec_start || !lec_len || !id_start || !id_len) return SKE_EINVAL;
    RowsItems I{};
    I.kind = 2;
    I.lec_bytes = bytes;
    I.lec_offs = lec_start;
    I.lec_len = lec_len;
    I.id_bytes = bytes;
    I.id_offs = id_start;
    I.id_len = id_len;
    I.status = status;
    I.epoch = epoch;
    I.valid = valid;
    I.mask = mask;
    I.n = uint32_t(n);
    return rows_enqueue(c, *R, I);
}

int ske_rows_append_fixed_async(ske_ctx *c, uint32_t rid, const uint8_t *lec_bytes, const uint32_t *lec_offs,
                                const uint8_t *ids, uint32_t width, const int64_t *epoch, const uint8_t *valid,
                                const uint8_t *mask, uint64_t n) {
    Rows *R = nullptr;
    const int rc = append_args(c, rid, n, epoch, &R);
    if (rc) return rc;
    if (width != 4 && width != 8) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!lec_bytes || !lec_offs || !ids) return SKE_EINVAL;
    RowsItems I{};
    I.kind = 1;
    I.lec_bytes = lec_bytes;
    I.lec_offs = lec_offs;
    I.id_bytes = ids;
    I.id_width = width;
    I.epoch = epoch;
    I.valid = valid;
    I.mask = mask;
    I.n = uint32_t(n);
    return rows_enqueue(c, *R, I);
}

// a packed host column on the device: the byte range [offs[0], offs[n]) and the
// offsets, the bytes pointer rebased so that offs[] index it unchanged
static int rows_stage_col(ske_ctx *c, const uint8_t *bytes, const uint32_t *offs, uint64_t n, StageSlot sb,
                          StageSlot so, const uint8_t **d_bytes, const uint32_t **d_offs) {
    if (!offs) return SKE_EINVAL;
    for (uint64_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i]) return SKE_EINVAL;
    const uint64_t b0 = offs[0], total = uint64_t(offs[n]) - b0;
    if (total && !bytes) return SKE_EINVAL;
    int rc = SKE_OK;
    uint8_t *db = (uint8_t *)stage_buf(c, sb, total + 16, &rc);
    if (rc) return rc;
    uint32_t *dof = (uint32_t *)stage_buf(c, so, (n + 1) * 4, &rc);
    if (rc) return rc;
    if (total) HIPCHK(c, hipMemcpyAsync(db, bytes + b0, total, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(dof, offs, (n + 1) * 4, hipMemcpyHostToDevice, c->st));
    *d_bytes = db - b0;
    *d_offs = dof;
    return SKE_OK;
}

int ske_rows_append(ske_ctx *c, uint32_t rid, const uint8_t *lec_bytes, const uint32_t *lec_offs,
                    const uint8_t *id_bytes, const uint32_t *id_offs, const int64_t *epoch, const uint8_t *valid,
                    const uint8_t *mask, uint64_t n, int mem) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_append", &rc);
    if (!R) return rc;
    if (n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!lec_offs || !id_offs || !epoch) return SKE_EINVAL;
    RowsItems I{};
    I.kind = 0;
    I.n = uint32_t(n);
    if (mem == SKE_MEM_DEVICE) {
        if (!lec_bytes || !id_bytes || (reinterpret_cast<uintptr_t>(epoch) & 7)) return SKE_EINVAL;
        I.lec_bytes = lec_bytes;
        I.lec_offs = lec_offs;
        I.id_bytes = id_bytes;
        I.id_offs = id_offs;
        I.epoch = epoch;
        I.valid = valid;
        I.mask = mask;
    } else {
        rc = rows_stage_col(c, lec_bytes, lec_offs, n, kStgRowsLec, kStgRowsLecOffs, &I.lec_bytes, &I.lec_offs);
        if (rc) return rc;
        rc = rows_stage_col(c, id_bytes, id_offs, n, kStgRowsId, kStgRowsIdOffs, &I.id_bytes, &I.id_offs);
        if (rc) return rc;
        int64_t *de = (int64_t *)stage_buf(c, kStgRowsEpoch, n * 8, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(de, epoch, n * 8, hipMemcpyHostToDevice, c->st));
        I.epoch = de;
        // the valid and mask bytes share one buffer: valid at 0, mask behind it
        if (valid || mask) {
            const size_t half = (n + 15) & ~size_t(15);
            uint8_t *dv = (uint8_t *)stage_buf(c, kStgRowsValid, 2 * half, &rc);
            if (rc) return rc;
            if (valid) {
                HIPCHK(c, hipMemcpyAsync(dv, valid, n, hipMemcpyHostToDevice, c->st));
                I.valid = dv;
            }
            if (mask) {
                HIPCHK(c, hipMemcpyAsync(dv + half, mask, n, hipMemcpyHostToDevice, c->st));
                I.mask = dv + half;
            }
        }
    }
    rc = rows_enqueue(c, *R, I);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_rows_read(ske_ctx *c, uint32_t rid, uint64_t first, uint64_t n, uint64_t *out_lec, int64_t *out_epoch,
                  int64_t *out_id, uint8_t *out_valid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_read", &rc);
    if (!R) return rc;
    RowsHead h{};
    rc = obj_read_head(c, *R, &h, sizeof h);
    if (rc) return rc;
    if (first > h.used || n > h.used - first) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!out_lec || !out_epoch || !out_id || !out_valid) return SKE_EINVAL;
    const RowsLog L = log_of(*R);
    HIPCHK(c, hipMemcpyAsync(out_lec, L.lec + first, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(out_epoch, L.epoch + first, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(out_id, L.id + first, n * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(out_valid, L.valid + first, n, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_rows_select(ske_ctx *c, uint32_t rid, const uint8_t *lec_bytes, uint32_t lec_len, int64_t since,
                    int64_t until, uint64_t *out_lec, int64_t *out_epoch, int64_t *out_id, uint8_t *out_valid,
                    uint64_t cap, uint64_t *n_out, int *complete, int mem) {
    if (!c || !n_out || !complete) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_select", &rc);
    if (!R) return rc;
    if (cap && (!out_lec || !out_epoch || !out_id || !out_valid)) return SKE_EINVAL;
    *n_out = 0;
    RowsFront F{};
    rc = rows_front(c, *R, lec_bytes, lec_len, since, until, false, complete, &F);
    if (rc || F.m == 0) return rc;
    const uint32_t runs = F.runs, m = F.m;
    const RowsLog L = log_of(*R);
    const unsigned grid = unsigned(c->rows_grid);
    *n_out = runs;
    if (runs > cap) return SKE_EROWSSPACE;

    // 5: the columns
    uint64_t *d_lec = out_lec;
    int64_t *d_epoch = out_epoch, *d_id = out_id;
    uint8_t *d_valid = out_valid;
    if (mem != SKE_MEM_DEVICE) {
        d_lec = (uint64_t *)stage_buf(c, kStgRowsLec, uint64_t(runs) * 8, &rc);
        if (rc) return rc;
        d_epoch = (int64_t *)stage_buf(c, kStgRowsEpoch, uint64_t(runs) * 8, &rc);
        if (rc) return rc;
        d_id = (int64_t *)stage_buf(c, kStgRowsId, uint64_t(runs) * 8, &rc);
        if (rc) return rc;
        d_valid = (uint8_t *)stage_buf(c, kStgRowsValid, runs, &rc);
        if (rc) return rc;
    }
    HIPCHK(c, launch_rows_gather(L, F.pos, m, F.W, (unsigned long long *)d_lec, (long long *)d_epoch,
                                 (long long *)d_id, d_valid, grid, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) {
        HIPCHK(c, hipMemcpyAsync(out_lec, d_lec, uint64_t(runs) * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(out_epoch, d_epoch, uint64_t(runs) * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(out_id, d_id, uint64_t(runs) * 8, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipMemcpyAsync(out_valid, d_valid, runs, hipMemcpyDeviceToHost, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_rows_compact(ske_ctx *c, uint32_t rid, int64_t keep_since, ske_rows_compact_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_compact", &rc);
    if (!R) return rc;
    memset(out, 0, sizeof *out);
    RowsHead h{};
    rc = obj_read_head(c, *R, &h, sizeof h);
    if (rc) return rc;
    const uint32_t used = uint32_t(h.used);  // <= 2^28
    // the select's own survivor rule, over every lecture from the cutoff on
    RowsFront F{};
    int complete = 1;
    rc = rows_front(c, *R, nullptr, 0, keep_since, INT64_MAX, false, &complete, &F);
    if (rc) return rc;
    const RowsCompactCounts n = rows_compact_counts(used, F.m, F.runs);
    out->before = n.before;
    out->kept = n.kept;
    out->superseded = n.superseded;
    out->expired = n.expired;
    if (n.kept == n.before) return SKE_OK;  // nothing to remove: no launch

    const uint32_t kept = uint32_t(n.kept);
    RowsCompactWork K{};
    if (kept) {
        hipError_t e = hipSuccess;
        K.keep = (uint8_t *)scratch_get(c->scratch, kScrRowsKeep, used, &e);
        if (e != hipSuccess) return scratch_error(c, e);
        K.cnt = (uint32_t *)scratch_get(c->scratch, kScrRowsKeepCnt, rows_cnt_bytes(used), &e);
        if (e != hipSuccess) return scratch_error(c, e);
        // the sort is over: its key buffers (m >= kept words each) carry the survivors
        K.tmp_a = scratch_get(c->scratch, kScrKeysOrFirst, uint64_t(F.m) * 8, &e);
        if (e != hipSuccess) return scratch_error(c, e);
        K.tmp_b = scratch_get(c->scratch, kScrKeysSorted, uint64_t(F.m) * 8, &e);
        if (e != hipSuccess) return scratch_error(c, e);
    }
    HIPCHK(c, launch_rows_compact(log_of(*R), used, F.pos, F.m, F.W, kept, K, unsigned(c->rows_grid), c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_rows_group(ske_ctx *c, uint32_t rid, int by, const uint8_t *lec_bytes, uint32_t lec_len, int64_t since,
                   int64_t until, int valid_filter, uint32_t sod_from, uint64_t *out_key, uint64_t *out_count,
                   uint64_t cap, uint64_t *n_out, ske_rows_group_stats_t *stats, int *complete, int mem) {
    if (!c || !n_out || !stats || !complete) return SKE_EINVAL;
    *n_out = 0;
    *complete = 1;
    memset(stats, 0, sizeof *stats);
    if (!rows_filter_ok(valid_filter, sod_from)) return SKE_EINVAL;
    if (by != SKE_ROWS_BY_STUDENT && by != SKE_ROWS_BY_LECTURE) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_group", &rc);
    if (!R) return rc;
    if (cap && (!out_key || !out_count)) return SKE_EINVAL;
    RowsFront F{};
    rc = rows_front(c, *R, lec_bytes, lec_len, since, until, by == SKE_ROWS_BY_STUDENT, complete, &F);
    if (rc || F.m == 0) return rc;
    stats->rows = F.runs;
    const uint32_t m = F.m;
    const RowsLog L = log_of(*R);
    const unsigned grid = unsigned(c->rows_grid);

    RowsGrpDev *D = (RowsGrpDev *)stage_buf(c, kStgRowsGrp, sizeof(RowsGrpDev), &rc);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    RowsGrpWork G{};
    G.gflag = (uint8_t *)scratch_get(c->scratch, kScrRowsGrpFlag, m, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    // the three tile-count arrays side by side (the listed groups are at most m)
    const size_t cb = (rows_cnt_bytes(m) + 15) & ~size_t(15);
    uint8_t *cnts = (uint8_t *)scratch_get(c->scratch, kScrRowsGrpCnt, 3 * cb, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.cnt_c = (uint32_t *)cnts;
    G.cnt_e = (uint32_t *)(cnts + cb);
    G.cnt_l = (uint32_t *)(cnts + 2 * cb);
    // the sort is over: its key buffers (m words each) hold the groups' keys
    G.gkey = (unsigned long long *)scratch_get(c->scratch, kScrKeysOrFirst, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.lkey = (unsigned long long *)scratch_get(c->scratch, kScrKeysSorted, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.gend = (uint32_t *)scratch_get(c->scratch, kScrRowsGrpEnds, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.lcount = (uint32_t *)scratch_get(c->scratch, kScrRowsGrpCounts, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);

    HIPCHK(c, launch_rows_grp_init(D, c->st));
    HIPCHK(c, launch_rows_grp_flags(L, F.pos, m, by, valid_filter, sod_from, F.W, G, grid, c->cus, c->st));
    uint32_t groups = 0;
    HIPCHK(c, hipMemcpyAsync(&groups, G.cnt_e, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    HIPCHK(c, launch_rows_grp_counts(G, groups, D, grid, c->cus, c->st));
    RowsGrpDev h{};
    const size_t head = offsetof(RowsGrpDev, hist);  // the accumulators and the select state
    HIPCHK(c, hipMemcpyAsync(&h, D, head, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    const uint32_t n = uint32_t(h.n);  // <= m
    if (n == 0) return SKE_OK;
    HIPCHK(c, launch_rows_grp_median(G, n, D, grid, c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(&h, D, head, hipMemcpyDeviceToHost, c->st));
    const bool fits = n <= cap;
    uint64_t *d_key = out_key, *d_count = out_count;
    if (fits) {
        if (mem != SKE_MEM_DEVICE) {
            d_key = (uint64_t *)stage_buf(c, kStgRowsLec, uint64_t(n) * 8, &rc);
            if (rc) return rc;
            d_count = (uint64_t *)stage_buf(c, kStgRowsEpoch, uint64_t(n) * 8, &rc);
            if (rc) return rc;
        }
        HIPCHK(c, launch_rows_grp_out(G, n, (unsigned long long *)d_key, (unsigned long long *)d_count, grid, c->cus,
                                      c->st));
        if (mem != SKE_MEM_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(out_key, d_key, uint64_t(n) * 8, hipMemcpyDeviceToHost, c->st));
            HIPCHK(c, hipMemcpyAsync(out_count, d_count, uint64_t(n) * 8, hipMemcpyDeviceToHost, c->st));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    *n_out = n;
    stats->n = h.n;
    stats->sum = h.sum;
    stats->sumsq = h.sumsq;
    stats->min = h.min;
    stats->max = h.max;
    stats->med_lo = h.sel.prefix[0];
    stats->med_hi = h.sel.prefix[1];
    return fits ? SKE_OK : SKE_EROWSSPACE;
}

int ske_rows_group_merge(ske_ctx *c, int by, const uint64_t *keys, const uint64_t *counts, uint64_t n_in,
                         uint64_t *out_key, uint64_t *out_count, uint64_t cap, uint64_t *n_out,
                         ske_rows_group_stats_t *stats, uint64_t *multi_out, int mem) {
    if (!c || !n_out || !stats || !multi_out) return SKE_EINVAL;
    *n_out = 0;
    *multi_out = 0;
    memset(stats, 0, sizeof *stats);
    if (by != SKE_ROWS_BY_STUDENT && by != SKE_ROWS_BY_LECTURE) return SKE_EINVAL;
    if (c->capturing) {
        c->last_hip = "ske_rows_group_merge waits for the stream and cannot be recorded";
        return SKE_EBUSY;
    }
    if (n_in > kRowsMergeMaxEntries) return SKE_EINVAL;
    if (n_in && (!keys || !counts)) return SKE_EINVAL;
    if (cap && (!out_key || !out_count)) return SKE_EINVAL;
    if (n_in == 0) return SKE_OK;
    const uint32_t m = uint32_t(n_in);
    const unsigned grid = unsigned(c->rows_grid);
    int rc = SKE_OK;

    const unsigned long long *d_keys = (const unsigned long long *)keys;
    const unsigned long long *d_counts = (const unsigned long long *)counts;
    if (mem != SKE_MEM_DEVICE) {
        void *k = stage_buf(c, kStgRowsId, uint64_t(m) * 8, &rc);
        if (rc) return rc;
        void *v = stage_buf(c, kStgRowsIdOffs, uint64_t(m) * 8, &rc);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(k, keys, uint64_t(m) * 8, hipMemcpyHostToDevice, c->st));
        HIPCHK(c, hipMemcpyAsync(v, counts, uint64_t(m) * 8, hipMemcpyHostToDevice, c->st));
        d_keys = (const unsigned long long *)k;
        d_counts = (const unsigned long long *)v;
    }
    RowsGrpDev *D = (RowsGrpDev *)stage_buf(c, kStgRowsGrp, sizeof(RowsGrpDev), &rc);
    if (rc) return rc;
    RowsMrgDev *M = (RowsMrgDev *)stage_buf(c, kStgRowsMrg, sizeof(RowsMrgDev), &rc);
    if (rc) return rc;

    // the select's sort and its slots: one pass over the caller's keys carries an iota
    hipError_t e = hipSuccess;
    unsigned long long *keys_s = (unsigned long long *)scratch_get(c->scratch, kScrKeysSorted, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *idx = (uint32_t *)scratch_get(c->scratch, kScrVals, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *idx_s = (uint32_t *)scratch_get(c->scratch, kScrValsSorted, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    RowsMrgWork W{};
    RowsGrpWork G{};
    W.counts = d_counts;
    W.keys_s = keys_s;
    W.idx_s = idx_s;
    // the four tile-count arrays side by side (the groups are at most m)
    const size_t cb = (rows_cnt_bytes(m) + 15) & ~size_t(15);
    uint8_t *cnts = (uint8_t *)scratch_get(c->scratch, kScrRowsGrpCnt, 4 * cb, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.cnt_c = W.cnt_v = (uint32_t *)cnts;
    G.cnt_e = (uint32_t *)(cnts + cb);
    G.cnt_l = (uint32_t *)(cnts + 2 * cb);
    W.cnt_z = (uint32_t *)(cnts + 3 * cb);
    G.gkey = (unsigned long long *)scratch_get(c->scratch, kScrKeysOrFirst, uint64_t(m) * 8, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.lkey = keys_s;  // the sorted keys are read last by the ends, the listed keys written behind them
    G.gend = (uint32_t *)scratch_get(c->scratch, kScrRowsGrpEnds, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    G.lcount = (uint32_t *)scratch_get(c->scratch, kScrRowsGrpCounts, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    W.zend = (uint32_t *)scratch_get(c->scratch, kScrRowsGrpFlag, uint64_t(m) * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);

    HIPCHK(c, launch_rows_iota(idx, m, grid, c->cus, c->st));
    e = rows_sort_pairs(c->scratch, by == SKE_ROWS_BY_STUDENT, d_keys, keys_s, idx, idx_s, m, c->st);
    if (e == hipErrorStreamCaptureUnsupported) return scratch_error(c, e);
    HIPCHK(c, e);
    HIPCHK(c, launch_rows_grp_init(D, c->st));
    HIPCHK(c, launch_rows_mrg_ends(W, G, m, M, grid, c->cus, c->st));
    // the first synchronisation: the groups and the total, before any output is written
    uint32_t groups = 0;
    RowsMrgDev hm{};
    HIPCHK(c, hipMemcpyAsync(&groups, G.cnt_e, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&hm, M, sizeof hm, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (!rows_merge_total_ok(hm.total, hm.wide)) return SKE_EINVAL;

    HIPCHK(c, launch_rows_grp_counts(G, groups, D, grid, c->cus, c->st));
    HIPCHK(c, launch_rows_mrg_multi(W, G, groups, M, grid, c->cus, c->st));
    RowsGrpDev h{};
    const size_t head = offsetof(RowsGrpDev, hist);  // the accumulators and the select state
    HIPCHK(c, hipMemcpyAsync(&h, D, head, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&hm, M, sizeof hm, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    const uint32_t n = uint32_t(h.n);  // <= m
    if (n == 0) return SKE_OK;
    HIPCHK(c, launch_rows_grp_median(G, n, D, grid, c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(&h, D, head, hipMemcpyDeviceToHost, c->st));
    const bool fits = n <= cap;
    uint64_t *d_key = out_key, *d_count = out_count;
    if (fits) {
        if (mem != SKE_MEM_DEVICE) {
            d_key = (uint64_t *)stage_buf(c, kStgRowsLec, uint64_t(n) * 8, &rc);
            if (rc) return rc;
            d_count = (uint64_t *)stage_buf(c, kStgRowsEpoch, uint64_t(n) * 8, &rc);
            if (rc) return rc;
        }
        HIPCHK(c, launch_rows_grp_out(G, n, (unsigned long long *)d_key, (unsigned long long *)d_count, grid, c->cus,
                                      c->st));
        if (mem != SKE_MEM_DEVICE) {
            HIPCHK(c, hipMemcpyAsync(out_key, d_key, uint64_t(n) * 8, hipMemcpyDeviceToHost, c->st));
            HIPCHK(c, hipMemcpyAsync(out_count, d_count, uint64_t(n) * 8, hipMemcpyDeviceToHost, c->st));
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    *n_out = n;
    *multi_out = hm.multi;
    stats->n = h.n;
    stats->sum = h.sum;
    stats->sumsq = h.sumsq;
    stats->min = h.min;
    stats->max = h.max;
    stats->med_lo = h.sel.prefix[0];
    stats->med_hi = h.sel.prefix[1];
    return fits ? SKE_OK : SKE_EROWSSPACE;
}

int ske_rows_profile(ske_ctx *c, uint32_t rid, const uint8_t *lec_bytes, uint32_t lec_len, int64_t since,
                     int64_t until, int valid_filter, uint32_t sod_from, uint64_t *out_bins, uint64_t *rows_out,
                     int *complete) {
    if (!c || !out_bins || !rows_out || !complete) return SKE_EINVAL;
    *rows_out = 0;
    *complete = 1;
    memset(out_bins, 0, SKE_TP_BINS * sizeof(uint64_t));
    if (!rows_filter_ok(valid_filter, sod_from)) return SKE_EINVAL;
    int rc = SKE_OK;
    Rows *R = obj_for_sync_call(c, kRowsFamily, c->rows, rid, "ske_rows_profile", &rc);
    if (!R) return rc;
    RowsFront F{};
    rc = rows_front(c, *R, lec_bytes, lec_len, since, until, false, complete, &F);
    if (rc || F.m == 0) return rc;
    *rows_out = F.runs;
    RowsGrpDev *D = (RowsGrpDev *)stage_buf(c, kStgRowsGrp, sizeof(RowsGrpDev), &rc);
    if (rc) return rc;
    HIPCHK(c, launch_rows_grp_init(D, c->st));
    HIPCHK(c, launch_rows_profile(log_of(*R), F.pos, F.m, valid_filter, sod_from, F.W, D, unsigned(c->rows_grid),
                                  c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(out_bins, D->bins, SKE_TP_BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

}  // extern "C"
