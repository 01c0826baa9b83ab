// sketch_rows_compact.h -- the arithmetic of the row log's compaction
// (sketch_rows.hip, DESIGN.md "Row log compaction"): what one call removes, from
// the three numbers the front end yields, and how the head follows.  No device
// code of its own: the host side and the end kernel call these functions, and
// tests/native/rowscompact_host.cpp runs them on the host.  csrc-internal.
#pragma once
#include "sketch_common.h"

namespace ske {

// ske_rows_compact_t, field for field
struct RowsCompactCounts {
    uint64_t before, kept, superseded, expired;
};

// before: `used` when the call began; m: the rows at or after keep_since; runs:
// their runs of equal (lec, epoch, id), one survivor each (runs <= m <= before).
// A row below the cutoff is expired whether or not a later row superseded it.
SKE_HD RowsCompactCounts rows_compact_counts(uint64_t before, uint64_t m, uint64_t runs) {
    RowsCompactCounts c;
    c.before = before;
    c.kept = runs;
    c.superseded = m - runs;
    c.expired = before - m;
    return c;
}

// The head after the survivors lie at 0 .. kept - 1: `taken` forgets the rows
// removed, so used + refused_ids + dropped == taken holds on; the refused and
// dropped counts and the sticky overflow are not the compaction's to touch.
SKE_HD void rows_compact_head(unsigned long long *used, unsigned long long *taken, unsigned long long kept) {
    const unsigned long long removed = *used - kept;
    *used = kept;
    *taken -= removed;
}

}  // namespace ske
