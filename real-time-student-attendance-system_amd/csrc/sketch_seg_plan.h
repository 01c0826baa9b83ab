// sketch_seg_plan.h -- the segmented PFADD's host-side sizing: the geometry of
// one batch (seg_plan) and the chunk slots and rows its scratch needs
// (seg_slots).  No device code: sketch_seg.hip allocates what this header
// computes, and tests/native/seg_capacity.cpp checks it on the host against a
// model of what C1 and D do to the counters.  csrc-internal.
#pragma once
#include <algorithm>
#include <cstdint>

#include "sketch_internal.h"

namespace ske {

constexpr uint32_t kSegChunk = 8192;  // records per chunk (the arena's of r1, the rows of r2 / o2)
constexpr uint32_t kSegRun = 8192;    // swipes per C1 run (sketch_part.h: kSegRunSw)

// the segmented PFADD's geometry for one batch (seg_plan)
struct SegPlan {
    uint32_t s1, b1, wlog, klog, nb1, nwin, maxch, nsub, dense_min;
    uint32_t floor, hot_min;  // the per-key floors: on, and E's hint threshold (arrivals per key and group)
};

// Records C1 can reserve in one sub-batch of at most `sub` swipes, pads
// included.  C1 rounds every non-empty (run, bucket) reservation up to 4
// records (in both run layouts: the pad is stored as rank-0 records), so run
// r with v_r valid swipes reserves
//     P_r = sum_h roundup4(c[r][h]) <= v_r + 3 * (its non-empty buckets)
//                                   <= v_r + 3 * min(nb1, v_r),
// and v_r is at most the run's length L_r (8192, the last run's the rest).
// (A run in the padded layout has P_r <= 8192 on top of that, which the bound
// does not need.)  The bound is reached: nb1 buckets of counts = 1 (mod 4)
// that sum to 8192 reserve exactly 8192 + 3 * nb1 records.
inline uint64_t seg_fill_max(uint32_t nb1, uint64_t sub) {
    const uint64_t full = sub / kSegRun, tail = sub % kSegRun;
    return full * (kSegRun + 3 * std::min<uint64_t>(nb1, kSegRun)) + tail + 3 * std::min<uint64_t>(nb1, tail);
}

// Rows of r2 / o2 one sub-batch can need: D gives bucket h
// ceil(fill_h / 8192) rows, the fill counts are multiples of 4, so
//     sum_h ceil(fill_h / 8192) <= sum_h (fill_h + 8188) / 8192
//                               <= (seg_fill_max + nb1 * 8188) / 8192
// (rounded down: the left side is an integer).  Without the pads this is the
// ceil(sub / 8192) + nb1, the sizing up to round 8, which is too few once
// sum_h fill_h exceeds `sub`: at 512 buckets the pads add up to 18.75 %.
inline uint32_t seg_rows_max(uint32_t nb1, uint64_t sub) {
    return uint32_t((seg_fill_max(nb1, sub) + uint64_t(nb1) * (kSegChunk - 4)) / kSegChunk);
}

// The segmented PFADD's geometry for a slab of nslots keys and a batch of n
// swipes in sub-batches of `sub`: windows of 2^klog keys (W = slot >> klog);
// 2^b1 level-1 buckets of 2^wlog windows each, window W in bucket W mod
// 2^b1 (buckets interleave windows, so the consecutive windows of a hot
// lecture's day keys fall in different buckets and every bucket carries
// about the same records), b1 + wlog = ceil(log2(windows)) split evenly so
// that both levels' runs stay long; false when the slab needs more than 2^9
// buckets of 2^9 windows.
inline bool seg_plan(uint32_t nslots, uint64_t n, uint32_t sub, const SegOpts &so, SegPlan *P) {
    if (nslots == 0 || n == 0 || so.klog < 0 || so.klog > 3) return false;
    const uint32_t klog = uint32_t(so.klog);
    const uint32_t nwin = uint32_t((uint64_t(nslots) + (1u << klog) - 1) >> klog);
    uint32_t tb = 0;
    while ((uint64_t(1) << tb) < nwin) tb++;
    // windows per bucket 2^wlog: at least half the window bits, and at least
    // tb - 5 (2^25 sub-batches: level-2 sorts over more windows beat longer
    // level-1 segments up to 2^9; profiles/r05_ab_seg_b1.txt: b1 7 at C3's
    // 2^16 windows, 5 at the 8-way shard's 2^13)
    uint32_t wlog = std::max((tb + 1) / 2, tb > 5 ? tb - 5 : 0u), b1 = tb - wlog;
    if (wlog > 9) {
        wlog = 9;
        b1 = tb - 9;
    }
    if (so.b1 >= 0) {  // the option: level-1 buckets 2^b1 (windows per bucket 2^(tb - b1) <= 2^9)
        b1 = uint32_t(so.b1) < tb ? uint32_t(so.b1) : tb;
        wlog = tb - b1;
    }
    if (b1 > 9) {
        b1 = 9;
        wlog = tb - 9;
    }
    if (wlog > 9) return false;
    P->klog = klog;
    P->wlog = wlog;
    P->b1 = b1;
    P->s1 = klog + wlog;
    P->nwin = nwin;
    P->nb1 = 1u << b1;
    // rows of r2 / o2 per sub-batch, C1's pads counted (seg_rows_max); D
    // writes no row past them
    P->maxch = seg_rows_max(P->nb1, sub);
    // sub-batches per window pass: at most 64, and their level-2 records
    // within a 2^31-byte buffer range (the window pass's record loads); a
    // batch of more runs a window pass after every nsub of them
    const uint64_t kmax = ((uint64_t(1) << 29) - 1) / (uint64_t(P->maxch) * kSegChunk);
    const uint64_t ns = (n + sub - 1) / sub;
    if (kmax == 0) return false;
    P->nsub = uint32_t(std::min<uint64_t>(std::min<uint64_t>(ns, kmax), 64));
    const uint64_t dm = uint64_t(so.dense_min_x100) * ((uint64_t(1) << klog) * (kHllRegs / 128)) / 100;
    P->dense_min = dm < 1 ? 1u : (dm > 0xffffffffu ? 0xffffffffu : uint32_t(dm));
    P->floor = so.floor != 0;
    P->hot_min = so.hot_min;
    return true;
}

// The chunk slots of r1 for sub-batches of at most m = min(n, sub) swipes
// (ch = ceil(m / 8192) runs), and the rows of r2 / o2 of a window pass.
//   kstat   fixed slots per bucket: about twice a bucket's mean chunks, as
//           many as keep every slot number below 2^14 (k_seg_c1's packing).
//   kmaxc   columns of ctab.  A bucket gets at most roundup4(L_r) <= 8192
//           records per run, so at most ch chunks: chunk indices stay < ch + 1.
//   dyn     counted slots, ch + nb1.  A bucket that takes counted slots has
//           more than kstat chunks; if H buckets do, their chunks number at most
//               sum (fill_h / 8192 + 1) <= (m + H * 3 * ch) / 8192 + H
//           (fill_h = the bucket's valid swipes + at most 3 pad records per
//           run), of which H * kstat sit in fixed slots.  ch <= 8192 runs
//           (sub <= 2^26) makes the pads' share at most 3 chunks per bucket,
//           and kstat >= 3 always (4 uncapped; the cap leaves at least
//           (2^14 - 1 - 8704) / 512 = 14), so the counted chunks number at
//           most ch + H <= ch + nb1: the pads cost no counted slot.
//   rows    nsub sub-batches of maxch rows each.
struct SegSlots {
    uint32_t kstat, kmaxc, dyn;
    uint32_t r1_slots;  // nb1 * kstat + dyn
    uint64_t rows;      // nsub * maxch, of kSegChunk records (r2) and 2^wlog + 1 words (o2) each
};
inline SegSlots seg_slots(const SegPlan &P, uint32_t sub, uint64_t n) {
    const uint64_t m = n < sub ? n : sub;
    const uint64_t ch = (m + kSegChunk - 1) / kSegChunk, dyn = ch + P.nb1;
    uint64_t kst = 2 * ((ch + P.nb1 - 1) / P.nb1) + 2;
    kst = std::min<uint64_t>(kst, ((1u << 14) - 1 - dyn) / P.nb1);
    SegSlots L;
    L.kstat = uint32_t(kst);
    L.kmaxc = uint32_t(ch + 1);
    L.dyn = uint32_t(dyn);
    L.r1_slots = uint32_t(P.nb1 * kst + dyn);
    L.rows = uint64_t(P.nsub) * P.maxch;
    return L;
}

}  // namespace ske
