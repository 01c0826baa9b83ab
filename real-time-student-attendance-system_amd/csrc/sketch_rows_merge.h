// sketch_rows_merge.h -- the arithmetic of the group merge (sketch_rows.hip
// "group merge", DESIGN.md "Exact insights across shards"): which entries and
// which total a call accepts, a merged group's sum and its number of nonzero
// entries from the two prefixes at the group ends, and which listed groups
// count as `multi`.  No device code of its own: the kernels call these
// functions, and tests/native/rowsmerge_host.cpp runs them on the host.
// csrc-internal.
#pragma once
#include "sketch_rows_group.h"

namespace ske {

constexpr uint64_t kRowsMergeMaxEntries = uint64_t(1) << 28;  // the sort's and the scans' 32-bit positions
constexpr uint64_t kRowsMergeMaxTotal = 0xffffffffull;        // every prefix of the counts fits a u32

// an entry's count alone may not pass the total's bound (a wider one would
// wrap the u32 tile sums before the total is looked at)
SKE_HD bool rows_merge_entry_ok(uint64_t count) { return count <= kRowsMergeMaxTotal; }

// total: the 64-bit sum of every entry's count (at most 2^28 entries below
// 2^32 each, so it never wraps when !wide); wide: some entry failed
// rows_merge_entry_ok.  With both satisfied every prefix is a u32 and the sum
// of the squares of the merged counts is at most total^2 < 2^64.
SKE_HD bool rows_merge_total_ok(uint64_t total, uint32_t wide) { return !wide && total <= kRowsMergeMaxTotal; }

// vend[g] = the inclusive prefix of the counts at group g's last sorted
// position: the merged count is the step from the group before -- the
// group-by's own rule over another prefix, so its back end runs unchanged
SKE_HD uint32_t rows_merge_sum(const uint32_t *vend, uint64_t g) { return rows_group_count(vend, g); }

// zend[g] = the inclusive prefix of the "count != 0" flags there: the group's
// nonzero entries
SKE_HD uint32_t rows_merge_entries(const uint32_t *zend, uint64_t g) { return zend[g] - (g ? zend[g - 1] : 0u); }

// a listed key that more than one nonzero entry fed (across ranks: a key that
// more than one rank held)
SKE_HD bool rows_merge_multi(uint32_t sum, uint32_t entries) { return rows_group_listed(sum) && entries > 1; }

}  // namespace ske
