// sketch_rows_group.h -- the arithmetic of the row log's group-by
// (sketch_rows.hip, DESIGN.md "Row log group-by"): which surviving row counts,
// a group's count from the counted prefix at the group ends, which groups are
// listed, and the two median ranks' radix select over the u32 counts (the
// rounds of sketch_hh_select.h).  No device code of its own: the kernels call
// these functions, and tests/native/rowsgroup_host.cpp runs them on the host.
// csrc-internal.
#pragma once
#include "sketch_common.h"
#include "sketch_hh_select.h"

namespace ske {

constexpr int kRowsByStudent = 0, kRowsByLecture = 1;                      // SKE_ROWS_BY_*
constexpr int kRowsValidAny = 0, kRowsValidOnly = 1, kRowsInvalidOnly = 2;  // SKE_ROWS_VALID_* / INVALID_ONLY
constexpr uint32_t kRowsSodMax = 86399;

// whether a row that survived the upsert counts: its is_valid passes the
// filter and its floored UTC second of the day is at least sod_from
SKE_HD bool rows_counted(uint32_t valid, int64_t epoch, int valid_filter, uint32_t sod_from) {
    if (valid_filter == kRowsValidOnly && !valid) return false;
    if (valid_filter == kRowsInvalidOnly && valid) return false;
    return sod_from == 0 || tp_time(epoch).sod >= sod_from;
}

// ends[g] = the counted rows at or before group g's last position, in sorted
// order: group g's count is the step from the group before
SKE_HD uint32_t rows_group_count(const uint32_t *ends, uint64_t g) { return ends[g] - (g ? ends[g - 1] : 0u); }

// a group whose rows were all filtered out is not listed (df[mask].groupby().size())
SKE_HD bool rows_group_listed(uint32_t count) { return count != 0; }

// The state of the two median ranks, (n - 1) / 2 and n / 2 in ascending order:
// per rank the digits fixed so far and the rank left among the counts that
// carry them.
struct RowsSel {
    uint32_t prefix[2];
    unsigned long long left[2];
};

SKE_HD void rows_sel_begin(RowsSel *s, uint64_t n) {
    s->prefix[0] = s->prefix[1] = 0;
    s->left[0] = n ? (n - 1) / 2 : 0;
    s->left[1] = n / 2;
}

// one round: hist[r * kHhSelBins + d] = the counts that match rank r's prefix
// above the round's digit and carry digit d there
SKE_HD void rows_sel_step(RowsSel *s, const uint32_t *hist, uint32_t round) {
    const uint32_t shift = hh_sel_shift(round);
    for (int r = 0; r < 2; r++) {
        uint64_t left = 0;
        const uint32_t d = hh_sel_walk(hist + r * kHhSelBins, kHhSelBins, s->left[r], &left);
        s->prefix[r] |= d << shift;
        s->left[r] = left;
    }
}

}  // namespace ske
