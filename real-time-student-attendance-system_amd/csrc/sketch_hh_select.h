// sketch_hh_select.h -- the arithmetic of the heavy-hitter sets' rank
// selection (sketch_hh_stats.hip): a radix select over u32 values, most
// significant digit first, kHhSelBits bits a round.  A rank's state is the
// value's digits fixed so far (`prefix`, the digits not yet fixed zero) and the
// rank left among the values that carry those digits.  One round: count, per
// digit, the values that match the prefix above the round's digit
// (hh_sel_matches, hh_sel_digit), then walk the counts (hh_sel_walk).  No
// device code of its own: the kernels call these functions, and
// tests/native/hhstats_host.cpp runs the whole select on the host through
// them.  csrc-internal.
#pragma once
#include "sketch_common.h"

namespace ske {

constexpr uint32_t kHhSelBits = 8;                    // digit width
constexpr uint32_t kHhSelBins = 1u << kHhSelBits;     // counts per histogram
constexpr uint32_t kHhSelRounds = 32 / kHhSelBits;    // rounds of a select
constexpr uint32_t kHhMaxRanks = 16;                  // ranks one select carries (SKE_HH_MAX_RANKS)

// the shift of round r's digit (round 0: the most significant)
SKE_HD uint32_t hh_sel_shift(uint32_t round) { return 32 - kHhSelBits * (round + 1); }

// whether v carries the prefix's digits above the digit at `shift`
SKE_HD bool hh_sel_matches(uint32_t v, uint32_t prefix, uint32_t shift) {
    const uint32_t above = shift + kHhSelBits;
    return above >= 32 || ((v ^ prefix) >> above) == 0;
}

SKE_HD uint32_t hh_sel_digit(uint32_t v, uint32_t shift) { return (v >> shift) & (kHhSelBins - 1); }

// Given nbins counts and a rank below their sum: the digit whose bin holds the
// rank-th smallest value (0-based), *left = the rank inside that bin.  A rank
// at or above the sum (the callers rule it out) ends in the last bin, *left
// what remains.
SKE_HD uint32_t hh_sel_walk(const uint32_t *counts, uint32_t nbins, uint64_t rank, uint64_t *left) {
    uint32_t d = 0;
    for (; d + 1 < nbins; d++) {
        if (rank < counts[d]) break;
        rank -= counts[d];
    }
    *left = rank;
    return d;
}

}  // namespace ske
