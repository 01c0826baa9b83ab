// sketch_internal.h -- launcher declarations shared by the libsketch TUs.
#pragma once
#include <cstddef>

#include "sketch_common.h"
#include "sketch_rows_compact.h"
#include "sketch_rows_group.h"
#include "sketch_rows_merge.h"

namespace ske {

// The grid rule of every launcher whose kernel walks n items in workgroups of
// `block`: the workgroups that cover n, at most `most` (the kernels stride over
// the rest).  n == 0 gives one workgroup, never none: most launchers return
// before they launch for nothing, and those that do launch then (the routing
// kernels, launch_hh_merge carrying only the overflow word) need the one.
inline unsigned grid_for(uint64_t n, unsigned block, unsigned most) {
    const uint64_t cover = (n + block - 1) / block;
    return unsigned(cover < most ? (cover ? cover : 1) : most);
}
// the same where the context carries an override of the most (`grid`; 0: `dflt`
// stands), itself held to `max`
inline unsigned grid_for(uint64_t n, unsigned block, unsigned grid, unsigned dflt, unsigned max) {
    const unsigned most = grid ? grid : dflt;
    return grid_for(n, block, most < max ? most : max);
}

// sketch_kernels.hip
hipError_t launch_swipes(int mode, const ChainDev &ch, bool lds, int tile, const uint8_t *bytes,
                         const uint32_t *offs, uint32_t fixed_w, const uint32_t *slot, uint64_t n,
                         uint8_t *regs,
                         uint32_t nslots, uint8_t *out, unsigned long long *stats, int cus,
                         hipStream_t st);
hipError_t lds_bloom_setup();
hipError_t set_stamp_buffer(void *p);  // -DSKE_STAMPS diagnostic build only
uint32_t lds_bloom_max();
hipError_t launch_pfadd(const uint32_t *slot, const uint8_t *bytes, const uint32_t *offs,
                        uint64_t n, uint8_t *regs, uint32_t nslots, unsigned int *err, int cus,
                        hipStream_t st);
hipError_t launch_pfcount(const uint8_t *regs, const uint32_t *slots, const uint32_t *goffs,
                          uint32_t ngroups, const double *tau, const double *sig, uint64_t *out,
                          int cus, hipStream_t st);
hipError_t launch_histogram(const uint8_t *regs, uint32_t *out64, hipStream_t st);
hipError_t launch_pfmerge(uint8_t *regs, uint32_t dst, const uint32_t *srcs, uint32_t n,
                          hipStream_t st);
uint32_t pfmerge_partitions(uint32_t n, int cus, uint32_t *per);
hipError_t launch_pfmerge_wide(uint8_t *regs, uint32_t dst, const uint32_t *srcs, uint32_t n,
                               uint8_t *partial, uint32_t per, uint32_t P, hipStream_t st);
hipError_t launch_slots_max(const uint32_t *slots, uint64_t n, unsigned int *out, int cus, hipStream_t st);
hipError_t launch_merge_groups(const uint8_t *regs, const uint32_t *slots, const uint32_t *goffs,
                               uint32_t ngroups, uint8_t *dst, int cus, hipStream_t st);
hipError_t launch_dense(const uint8_t *regs, uint8_t *dense, hipStream_t st);
hipError_t launch_gen_swipes(const GenDev &g, uint64_t start, uint64_t n, uint8_t *bytes,
                             uint32_t *offs, uint32_t *slot, int cus, hipStream_t st);
hipError_t launch_gen_members(const GenDev &g, uint64_t start, uint64_t n, uint8_t *bytes,
                              uint32_t *offs, int cus, hipStream_t st);

// sketch_k1.hip -- K1 for chains that fit the LDS image, short-id fast path
constexpr int kK1MaxLinks = 8;
constexpr int kLdsBloomMaxBytes = 152 * 1024;  // LDS image budget (160 KiB per CU)

struct K1Link {
    const uint8_t *bf;   // device bit array (readable to nbytes16)
    uint64_t m;          // Granlund-Montgomery magic of d
    uint32_t d;          // bloom->bits (<= 2^31)
    uint32_t t;          // 2^64 mod d
    uint32_t sh;         // l - 1 of the magic
    uint32_t k;          // bloom->hashes
    uint32_t nbytes16;   // bloom->bytes rounded up to 16
    uint32_t piece0;     // first 1 KiB LDS piece of the link (LDS offset piece0 * 1024)
};

struct K1Args {
    const uint8_t *bytes;
    const uint32_t *offs;   // nullptr: fixed-width ids (fixed_w bytes each)
    const uint32_t *slot;
    uint8_t *regs;
    uint8_t *out;           // may be nullptr
    unsigned int *err;      // set when a valid swipe names a slot >= nslots
    const uint8_t *zero16;  // 16 readable zero bytes (load address of empty ids)
    uint32_t n, nslots, fixed_w, nlinks, npieces;
    K1Link link[kK1MaxLinks];
};

// ske_swipes_many_async through the short-id LDS K1: one persistent launch over
// up to kK1ManyMax batches (passed by value: the kernel arguments are captured
// with a graph), tpre[j] = tiles of the batches before j
constexpr uint32_t kK1ManyMax = 48;
struct K1Batch {
    const uint8_t *bytes;
    const uint32_t *offs;  // nullptr: fixed-width ids
    const uint32_t *slot;
    uint8_t *out;          // may be nullptr
    uint32_t n, fixed_w;
};
struct K1Many {
    K1Batch b[kK1ManyMax];
    uint32_t tpre[kK1ManyMax + 1];
    uint32_t nb;
};
uint32_t k1_many_tile(int tile);  // swipes per tile of the many kernel
hipError_t launch_swipes_lds_many(const K1Args &A, const K1Many &M, int tile, int cus, hipStream_t st);

// sketch_route.hip -- unpartitioned swipes to their key owners (alltoallv halves)
hipError_t launch_route(const uint8_t *ids, uint32_t width, const uint32_t *slot, uint64_t n, uint32_t world,
                        const uint32_t *kown, const uint32_t *kloc, uint32_t nkeys, uint8_t *sids,
                        uint32_t *sslot, uint32_t *pos, uint32_t *hist, uint32_t *tot, hipStream_t st);
uint64_t route_hist_words(uint64_t n, uint32_t world);
// out (device) = answers in[0..n) packed 1 bit per swipe, LSB first; in must be 8-B aligned
hipError_t launch_pack_bits(const uint8_t *in, uint64_t n, uint8_t *out, int cus, hipStream_t st);
hipError_t launch_route_cap(const uint8_t *ids, uint32_t width, const uint32_t *slot, uint64_t n, uint32_t world,
                            const uint32_t *kroute, uint32_t nkeys, uint32_t cap, const uint32_t *sink, uint8_t *sids,
                            uint32_t *sslot, uint32_t *pos, uint32_t *hist, uint32_t *tot, int cus, hipStream_t st);
hipError_t launch_route_return(const uint8_t *ans, const uint32_t *pos, uint64_t n, uint8_t *out, int cus,
                               hipStream_t st);
hipError_t launch_route_slots(const uint32_t *gkey, uint64_t n, const uint32_t *kroute, uint32_t nkeys,
                              uint32_t world, uint32_t *out, int cus, hipStream_t st);

// fills A's chain fields; false when the chain does not fit this variant
bool k1_lds_plan(const ChainDev &ch, K1Args *A);
hipError_t launch_swipes_lds(const K1Args &A, bool hll, int tile, int cus, hipStream_t st);
hipError_t k1_lds_setup();
hipError_t set_k1_stamp_buffer(void *p);  // -DSKE_STAMPS diagnostic build only
hipError_t set_pb_stamp_buffer(void *p);  // -DSKE_STAMPS diagnostic build only
hipError_t set_seg_stamp_buffer(void *p);  // -DSKE_SEG_STAMPS diagnostic build only

// sketch_ingest.hip -- JSON event decode and key-slot resolution (device columns)
struct IngestCols {
    uint8_t *status;  // 0 decoded on the device, 1 for the host
    uint32_t *id_start, *id_len, *lec_start, *lec_len, *ts_start, *ts_len;
    int32_t *day;     // UTC day number (README key form)
    uint64_t *kh;     // 2 per message: key hash
};
hipError_t launch_ingest_parse(const uint8_t *msgs, const uint32_t *moffs, uint64_t n, int day_form,
                               const IngestCols &out, int cus, hipStream_t st);
hipError_t launch_keytab_insert(uint64_t *tk, uint32_t *tslot, uint64_t mask, const uint64_t *kh,
                                const uint32_t *slots, uint64_t n, int cus, hipStream_t st);
hipError_t launch_keytab_lookup(const uint64_t *tk, const uint32_t *tslot, uint64_t mask,
                                const uint64_t *kh, const uint8_t *status, const uint32_t *id_len,
                                uint64_t n, uint32_t *slot, uint32_t *flag, uint32_t *mlen, int cus,
                                hipStream_t st);
hipError_t launch_ingest_pack(const uint8_t *msgs, const IngestCols &c, const uint32_t *slot,
                              const uint32_t *flag_incl, const uint32_t *len_incl, uint64_t n,
                              uint8_t *ids, uint32_t *ids_offs, uint32_t *kslot, int cus,
                              hipStream_t st);
hipError_t launch_ingest_unpack(const IngestCols &c, const uint32_t *slot, const uint32_t *flag_incl,
                                const uint8_t *kvalid, uint64_t n, uint8_t *valid, int cus,
                                hipStream_t st);
// the decoded messages as one packed batch (ske_ingest_dense_t)
struct IngestDense {
    uint8_t *ids;
    uint32_t *offs;
    int64_t *epoch;
    uint8_t *valid;
    uint32_t *at;
};
// grid: workgroups (0: the launch shape of the kernels above)
hipError_t launch_ingest_times(const uint8_t *msgs, const IngestCols &c, uint64_t n, int64_t *epoch, int cus,
                               unsigned grid, hipStream_t st);
hipError_t launch_ingest_dense_flags(const IngestCols &c, uint64_t n, uint32_t *flag, uint32_t *mlen, int cus,
                                     unsigned grid, hipStream_t st);
hipError_t launch_ingest_dense(const uint8_t *msgs, const IngestCols &c, const uint32_t *flag_incl,
                               const uint32_t *len_incl, const uint8_t *valid, const int64_t *epoch, uint64_t n,
                               const IngestDense &out, int cus, unsigned grid, hipStream_t st);

// sketch_xr.hip -- XCD-partitioned K1 for chains larger than the LDS image
bool xr_supported(const ChainDev &ch);
uint64_t xr_scratch_bytes(uint64_t n, int nlinks);
hipError_t launch_swipes_xr(const ChainDev &ch, const uint8_t *bytes, const uint32_t *offs,
                            uint32_t fixed_w, const uint32_t *slot, uint64_t n, uint8_t *regs,
                            uint32_t nslots, uint8_t *out, void *scratch, unsigned int *err,
                            int cus, int region_u, int finish_u, hipStream_t st);

// sketch_part.hip -- partitioned K1 (probe records routed to LDS-resident
// 64 KiB slices of each link) for chains larger than the LDS image; its
// segmented PFADD is sketch_seg.hip, what the two share sketch_part.h
constexpr int kPSliceLog = 19;
constexpr uint32_t kPSliceBits = 1u << kPSliceLog;
constexpr uint32_t kPMaxSlices = 2047;
constexpr int kPMaxLinks = 8;
struct Scratch;
bool part_supported(const ChainDev &ch);
// The segmented PFADD (k_seg_*, the pass C of one-link chains when a batch's
// register updates are dense in the slab) -- options "hll_seg" (mode),
// "seg_density" and "seg_dense_min" (x100), "seg_klog", "seg_floor" and
// "seg_hot_min" (the per-key floors, sketch_seg.hip).
struct SegOpts {
    int mode = -1;                  // -1 auto, 0 never (pass C), 1 whenever the chain and slab allow
    uint32_t density_x100 = 600;    // auto: a batch's swipes per 128-B line of the slab, x100 (x2 when the
                                    // slab fits the Infinity Cache, where pass C's random requests are cheaper)
    uint32_t dense_min_x100 = 100;  // a window is staged in LDS from this many records per line, x100
    int klog = 1;                   // keys per window: 2^klog (16 KiB each; 0..3)
    int b1 = -1;  // option "seg_b1": 2^b1 level-1 buckets (-1: auto, seg_plan)
    int floor = 1;               // 1: D drops the records no register can rise from (per-key floors); 0: never
    uint32_t hot_min = 4096;     // a window is hinted for a floor from this many arrivals per key and group
};
// sizes the context scratch for batches of up to n swipes (no launch)
// sub: swipes per sub-batch of the three passes (0: the default, 2^25 = kPSubDefault)
hipError_t part_reserve(const ChainDev &ch, uint64_t n, uint32_t sub, uint32_t nslots, const SegOpts &so,
                        Scratch *scr);
// hook (may be null): called as hook(user, pass, 0) right before and
// hook(user, pass, 1) right after each pass's launch (pass 0..4 = A, B, C or
// the segmented C1, the segmented level-2 sort, the segmented window apply)
typedef void (*PassHook)(void *user, int pass, int end, hipStream_t st);
struct PartBatch {
    const uint8_t *bytes;
    const uint32_t *offs;  // nullptr: fixed-width ids
    uint32_t fixed_w;
    const uint32_t *slot;
    uint64_t n;
    uint8_t *out;          // may be nullptr
};
// every pass of every (batch, sub-batch) unit on st, in order
hipError_t launch_swipes_part(const ChainDev &ch, const PartBatch *bt, uint32_t nb, uint8_t *regs,
                              uint32_t nslots, Scratch *scr, unsigned int *err, int cus, uint32_t sub,
                              const SegOpts &so, hipStream_t st, PassHook hook = nullptr,
                              void *hook_user = nullptr);


// sketch_cms.hip -- Count-Min Sketch (RedisBloom src/cms.c): bulk add in two
// forms, the sequential add with replies, query, weighted merge
constexpr uint32_t kCmsLdsMaxBytes = 152 * 1024;         // the LDS form's private table (160 KiB per CU)
constexpr uint32_t kCmsLdsCells = kCmsLdsMaxBytes / 4;   // tables up to this many cells take the LDS form
constexpr int kCmsMaxMerge = 64;
struct CmsTable {
    uint32_t *cells;            // depth rows of width counters
    unsigned long long *count;  // sum of all increments
    Div32 div;                  // of width
    uint32_t depth, ncells;
};
struct CmsItems {
    const uint8_t *bytes;
    const uint32_t *offs;  // nullptr: fixed-width ids (fixed_w bytes each)
    uint32_t fixed_w;
    uint32_t n;
    const uint32_t *incr;  // nullptr: 1 each
    const uint8_t *mask;   // nullptr: every item counts; else those with mask[i] == want
    uint32_t want;
};
struct CmsMergeArgs {
    const uint32_t *src[kCmsMaxMerge];
    long long w[kCmsMaxMerge];
    uint32_t nsrc, ncells;
    uint32_t *dst;
    unsigned int *flag;  // set when a cell leaves [0, 2^32 - 1] (or the 64-bit sum overflows)
};
hipError_t cms_setup();
// order-free add; lds: each workgroup sums into a private LDS table first (T.ncells <= kCmsLdsCells)
hipError_t launch_cms_add(const CmsTable &T, const CmsItems &I, bool lds, int cus, hipStream_t st);
// items in order by one wavefront, reply[i] = min of item i's cells after its update
hipError_t launch_cms_seq(const CmsTable &T, const CmsItems &I, uint32_t *reply, hipStream_t st);
hipError_t launch_cms_query(const CmsTable &T, const CmsItems &I, uint32_t *out, int cus, hipStream_t st);
// write == false: only the range check into M.flag; true: dst = the weighted sums
hipError_t launch_cms_merge(const CmsMergeArgs &M, bool write, int cus, hipStream_t st);
// D's cells = min(sum over ntables tables, 2^32 - 1), table k at tables + k * stride (cells; stride a
// multiple of 4 and >= D.ncells, tables 16-byte aligned), *D.count = count
hipError_t launch_cms_sum(const CmsTable &D, const uint32_t *tables, uint64_t stride, uint32_t ntables,
                          unsigned long long count, int cus, hipStream_t st);

// sketch_hh.hip -- heavy-hitter sets beside a Count-Min Sketch table: ids whose
// estimate reached a threshold, in an insert-only open-addressing table
constexpr uint32_t kHhMaxProbes = 128;  // slots one insert looks at (SKE_HH_MAX_PROBES)
constexpr uint32_t kHhLoadDen = 2;      // new claims stop at capacity / kHhLoadDen (SKE_HH_LOAD_DEN)
// tables up to this many cells are copied into LDS by every workgroup of a
// track and queried there; larger ones (and all, when 0) are read from memory
constexpr uint32_t kHhLdsCells = kCmsLdsCells;
struct HhSet {
    unsigned long long *claim;  // per slot: the id's digest (hh_digest), 0 = empty
    uint64_t *ids;              // per slot: w0, w1 of the id (Item), written by the claim's winner
    uint32_t *len;              // per slot: the id's length
    unsigned int *used;         // slots claimed
    unsigned int *overflow;     // sticky: an insert was refused
    uint32_t mask;              // capacity - 1
    uint32_t limit;             // capacity / kHhLoadDen
};
hipError_t hh_setup();
// every item (mask as CmsItems) whose estimate in T is >= threshold joins S;
// toolong (may be null): set when an item is longer than 16 bytes (it is skipped)
hipError_t launch_hh_track(const CmsTable &T, const CmsItems &I, const HhSet &S, uint32_t threshold, bool lds,
                           unsigned int *toolong, int cus, hipStream_t st);
// members with estimate >= threshold, unordered: entry j < min(*out_n, cap) in
// out_ids[2j..], out_len[j], out_est[j]; *out_n (zeroed by the caller) counts all that pass
hipError_t launch_hh_list(const CmsTable &T, const HhSet &S, uint32_t threshold, uint32_t cap, uint64_t *out_ids,
                          uint32_t *out_len, uint32_t *out_est, unsigned int *out_n, hipStream_t st);
// every member, unordered, no table: entry j < min(*out_n, cap) in out_ids[2j..], out_len[j]
hipError_t launch_hh_export(const HhSet &S, uint32_t cap, uint64_t *out_ids, uint32_t *out_len, unsigned int *out_n,
                            hipStream_t st);
// every entry (16 padded id bytes at ids + 2i, len[i]) joins S, no threshold; len[i] > 16 is skipped
// and sets S's overflow word, as foreign_overflow != 0 does
hipError_t launch_hh_merge(const HhSet &S, const uint64_t *ids, const uint32_t *len, uint32_t n,
                           uint32_t foreign_overflow, int cus, hipStream_t st);

// sketch_hh_stats.hip -- moments and order statistics of a set's current
// estimates, all in integers.  One device record per
// call; the host reads its first kHhStatReplyBytes bytes once, at the end.
constexpr uint32_t kHhStatRanks = 16;  // ranks one select carries (SKE_HH_MAX_RANKS)
struct HhStatDev {
    // the estimate pass: one add of each per workgroup that has a passing slot
    unsigned long long sum;           // of the passing estimates
    unsigned long long sq_lo, sq_hi;  // of the low / high 32 bits of their squares
    unsigned int n;                   // how many pass = entries of the compacted array
    unsigned int nmin;                // max of ~estimate (zeroed with the record); k_hhs_begin turns it into
    unsigned int min, max;            //   min (0 when n == 0)
    unsigned int complete;            // the set's overflow word was 0 (k_hhs_begin)
    unsigned int bad;                 // a requested rank was >= n: nothing is selected
    unsigned int prefix[kHhStatRanks];  // per rank: the digits fixed so far; after the last round the value
    // -- up to here the host's copy (kHhStatReplyBytes)
    unsigned int nr;                         // ranks being selected (0: none)
    unsigned int lead[kHhStatRanks];         // the first rank with the same prefix: it owns the histogram
    unsigned long long rank[kHhStatRanks];   // the rank left among the values that match the prefix
    unsigned int hist[kHhStatRanks * 256];   // per leading rank: the round's digit counts
};
constexpr size_t kHhStatReplyBytes = offsetof(HhStatDev, nr);
struct HhRanks {
    unsigned long long r[kHhStatRanks];
    uint32_t n;  // 0: the two median ranks, (n - 1) / 2 and n / 2, derived on the device
};
// The whole chain on st, no host round trip: the estimate pass over S's slots
// (passing estimates compacted into est, 4 bytes per slot at most, order
// undefined), the ranks, then the select's rounds.  *D must be zeroed by the
// caller (stream order).
hipError_t launch_hh_stats(const CmsTable &T, const HhSet &S, uint32_t threshold, const HhRanks &R, HhStatDev *D,
                           uint32_t *est, int cus, hipStream_t st);

// sketch_tp.hip -- time profile: weekday x hour counters of a batch's swipe
// times, and the per-swipe "late" byte
struct TpArgs {
    unsigned long long *counts;  // kTpBins counters
    const int64_t *epoch;        // n seconds since 1970-01-01 UTC
    const uint8_t *mask;         // nullptr: every swipe counts; else those with mask[i] == want
    uint8_t *late;               // nullptr, or n bytes: second of the day >= late_from
    uint32_t n, want, late_from;
};
constexpr unsigned kTpMaxGrid = 4096;
// form 0: a wavefront whose tile falls into one bin adds it as one LDS atomic;
// 1: one LDS atomic per lane, always.  grid: workgroups (at most kTpMaxGrid; fewer for a small n)
hipError_t launch_tp_add(const TpArgs &A, int form, unsigned grid, hipStream_t st);

// sketch_tally.hip -- tallies: exact event counts per key (a byte string of at
// most kTallyKeyBytes), an insert-or-add open-addressing table
constexpr uint32_t kTallyKeyBytes = 8 * kTallyKeyWords;  // SKE_TALLY_KEY_BYTES
constexpr uint32_t kTallyMaxProbes = 128;  // slots one insert-or-add looks at (SKE_TALLY_MAX_PROBES)
constexpr uint32_t kTallyLoadDen = 2;      // new claims stop at capacity / kTallyLoadDen (SKE_TALLY_LOAD_DEN)
constexpr int kTallyLdsMinLog2 = 4;        // form 0: slots of a workgroup's LDS table, 2^4 ..
constexpr int kTallyLdsMaxLog2 = 12;       //   2^12 (20 bytes a slot: 80 KiB of the CU's 160)
constexpr unsigned kTallyMaxGrid = 4096;
struct TallyTab {
    unsigned long long *claim;   // per slot: the key's digest (tally_digest), 0 = empty
    uint64_t *keys;              // per slot: the key's four words, written by the claim's winner
    unsigned long long *events;  // per slot: items counted
    unsigned long long *valid;   // per slot: of those, the ones whose mask byte was 1
    uint32_t *len;               // per slot: the key's length
    unsigned int *used;          // slots claimed
    unsigned int *overflow;      // sticky: an item was refused (or its key too long)
    unsigned long long *taken;   // items looked at
    unsigned long long *dropped_events, *dropped_valid;  // the counts of refused items
    uint32_t mask;               // capacity - 1
    uint32_t limit;              // capacity / kTallyLoadDen
};
// where a batch's keys are: kind 0 packed (key i = bytes[offs[i] .. offs[i + 1])),
// 1 fixed width (bytes + i * fixed_w), 2 spans (bytes[start[i] .. start[i] +
// len[i]), taken only when status is null or status[i] == 0), 3 a listing
// (32 padded bytes a key at bytes + 32 i, len[i]; item i counts ev[i] / va[i])
struct TallyItems {
    int kind;
    const uint8_t *bytes;
    const uint32_t *offs;    // kind 0: offsets; kind 2: starts
    const uint32_t *len;     // kind 2, 3
    const uint8_t *status;   // kind 2, may be null
    const uint8_t *mask;     // may be null: no item is valid
    const uint64_t *ev, *va; // kind 3
    uint32_t fixed_w, n;
    unsigned int *toolong;   // may be null: set when a key is longer than kTallyKeyBytes
};
hipError_t tally_setup();
// form 0: one LDS table of 2^lds_log2 slots per workgroup, flushed at the end;
// 1: one insert-or-add in memory per item.  grid: workgroups of form 0 (at most kTallyMaxGrid)
hipError_t launch_tally_add(const TallyTab &T, const TallyItems &I, int form, unsigned grid, int lds_log2, int cus,
                            hipStream_t st);
// ev[i], va[i] = the counters of item i's key (0, 0 when absent or too long)
hipError_t launch_tally_query(const TallyTab &T, const TallyItems &I, uint64_t *ev, uint64_t *va, int cus,
                              hipStream_t st);
// entries with events >= min_events, unordered: entry j < min(*out_n, cap) in
// out_keys[4j..], out_len[j], out_ev[j], out_va[j]; *out_n (zeroed by the caller) counts all that pass
hipError_t launch_tally_list(const TallyTab &T, uint64_t min_events, uint32_t cap, uint64_t *out_keys,
                             uint32_t *out_len, uint64_t *out_ev, uint64_t *out_va, unsigned int *out_n,
                             hipStream_t st);
// the head takes another tally's refused counts: taken and dropped_events grow by dropped_events,
// dropped_valid by dropped_valid, overflow != 0 sets the overflow word
hipError_t launch_tally_head_add(const TallyTab &T, unsigned long long dropped_events,
                                 unsigned long long dropped_valid, uint32_t overflow, hipStream_t st);

// sketch_seen.hip -- seen-row sets: an exact insert-only set of 128-bit row keys
// whose add answers, per item, first sighting or repeat (DESIGN.md "Seen rows")
constexpr uint8_t kSeenFirst = 0, kSeenRepeat = 1, kSeenSkipped = 2;  // SKE_SEEN_*
constexpr uint32_t kSeenNoSlot = 0xffffffffu;    // per-item scratch: the walk found no slot
constexpr uint32_t kSeenSkipSlot = 0xfffffffeu;  //   the mask kept the item out
constexpr uint32_t kSeenLastCall = 0xfffffffeu;  // the call counter stops here: stamps stay below all ones
constexpr unsigned kSeenMaxGrid = 4096;
struct SeenHead {  // the first bytes of a set's allocation
    unsigned int used;            // slots claimed
    unsigned int pad_;
    unsigned long long calls;     // adds run so far: the number of the next one
    unsigned long long looked_at; // items the masks let through
    unsigned long long first;     // of those, answered first (the unplaced ones included)
    unsigned long long unplaced;  // of those, the ones that found no slot
};
struct SeenTab {
    SeenHead *head;
    unsigned long long *w0, *w1;  // per slot: the key's two words, 0 = not yet claimed
    unsigned long long *stamp;    // per slot: (call << 32) | item of the first sighting, all ones = none
    uint32_t mask;                // capacity - 1
    uint32_t limit;               // capacity / kSeenLoadDen
};
// where a fold's column is: kind 0 packed, 1 fixed width, 2 spans (item i is
// bytes[start[j] .. start[j] + len[j]), j = at ? at[i] : i), 3 epochs
struct SeenCol {
    int kind;
    const uint8_t *bytes;
    const uint32_t *offs;   // kind 0: offsets; kind 2: starts
    const uint32_t *len;    // kind 2
    const uint32_t *at;     // kind 2, may be null
    const int64_t *epoch;   // kind 3
    int64_t granularity;    // kind 3
    uint32_t fixed_w, n;
};
// keys[2i], keys[2i + 1] = fold(begin ? the seeds : the words there, column item i)
hipError_t launch_seen_fold(uint64_t *keys, const SeenCol &C, bool begin, unsigned grid, int cus, hipStream_t st);
// the walk and the stamps, the answers, then the call counter's bump; slot: n words of scratch
hipError_t launch_seen_add(const SeenTab &T, const uint64_t *keys, uint32_t n, const uint8_t *mask, uint32_t want,
                           uint32_t *slot, uint8_t *out, unsigned grid, int cus, hipStream_t st);
hipError_t launch_seen_test(const SeenTab &T, const uint64_t *keys, uint32_t n, uint8_t *present, unsigned grid,
                            int cus, hipStream_t st);

// sketch_rows.hip -- row logs: the attendance table's rows in arrival order, an
// append-only columnar log read back per lecture (DESIGN.md "Row log")
constexpr unsigned kRowsMaxGrid = 4096;
constexpr unsigned kRowsScanBlock = 1024;  // threads of the one workgroup that scans the tile counts
struct RowsHead {  // the first bytes of a log's allocation
    unsigned long long used;         // rows held: the next row's position
    unsigned long long taken;        // rows the statuses and masks let through
    unsigned long long refused_ids;  // of those, the ones whose id is not an integer
    unsigned long long dropped;      // of those, the ones that found the log full
    unsigned int overflow;           // sticky: a row was dropped
};
struct RowsLog {
    RowsHead *head;
    unsigned long long *lec;  // per row: the lecture's digest
    long long *epoch;         //   seconds
    long long *id;            //   the student id
    uint8_t *valid;           //   is_valid
    uint64_t capacity;
};
// where a batch's lecture and id columns are: kind 0 both packed, 1 lectures
// packed and ids fixed width (4 or 8 little-endian bytes), 2 both spans of bytes
struct RowsItems {
    int kind;
    const uint8_t *lec_bytes;
    const uint32_t *lec_offs;  // kind 0, 1: offsets; kind 2: starts
    const uint32_t *lec_len;   // kind 2
    const uint8_t *id_bytes;
    const uint32_t *id_offs;   // kind 0: offsets; kind 2: starts
    const uint32_t *id_len;    // kind 2
    uint32_t id_width;         // kind 1
    const int64_t *epoch;
    const uint8_t *valid;      // may be null: every row's is_valid is 0
    const uint8_t *status;     // may be null; else rows with status[i] == 0
    const uint8_t *mask;       // may be null; else rows with mask[i] == 1
    uint32_t n;
};
// per-call state of an append or a select: a flag byte and a parsed id per
// item, and per tile of kRowsBlock items two counts behind a 4-word total
struct RowsWork {
    uint8_t *flag;   // n bytes: 0 not taken, 1 placed, 2 refused
    long long *idv;  // n parsed ids (append)
    uint32_t *cnt;   // [0..3] totals, then tiles placed-counts, then tiles refused-counts
};
SKE_HD uint64_t rows_tiles(uint64_t n) { return (n + kRowsBlock - 1) / kRowsBlock; }
inline size_t rows_cnt_bytes(uint64_t n) { return (4 + 2 * rows_tiles(n)) * 4; }
// flag and count, scan, place, then the head's advance; grid: workgroups (0: eight per CU)
hipError_t launch_rows_append(const RowsLog &L, const RowsItems &I, const RowsWork &W, unsigned grid, int cus,
                              hipStream_t st);
// flag[i] = row i < m is of the lecture (any when !by_lec) and since <= epoch < until; then the scan:
// W.cnt[0] = matches, pos_out (positions ascending) filled
hipError_t launch_rows_match(const RowsLog &L, uint32_t m, bool by_lec, unsigned long long digest, long long since,
                             long long until, const RowsWork &W, uint32_t *pos_out, unsigned grid, int cus,
                             hipStream_t st);
// key_out[j] = column col (0 id, 1 epoch, 2 lec) of row pos[j]
hipError_t launch_rows_keys(const RowsLog &L, const uint32_t *pos, uint32_t m, int col, unsigned long long *key_out,
                            unsigned grid, int cus, hipStream_t st);
// over pos in sorted order: flag[j] = row pos[j] is the last of its run of equal (lec, epoch, id); the
// scan: W.cnt[0] = runs
hipError_t launch_rows_last(const RowsLog &L, const uint32_t *pos, uint32_t m, const RowsWork &W, unsigned grid,
                            int cus, hipStream_t st);
// the flagged rows' columns, in order, to the outputs (after launch_rows_last)
hipError_t launch_rows_gather(const RowsLog &L, const uint32_t *pos, uint32_t m, const RowsWork &W,
                              unsigned long long *out_lec, long long *out_epoch, long long *out_id,
                              uint8_t *out_valid, unsigned grid, int cus, hipStream_t st);
// The group-by over the sorted positions (DESIGN.md "Row log group-by"; the
// arithmetic is sketch_rows_group.h's).  The device state of one call: the
// statistics' accumulators, the median ranks' select state and histograms, and
// the profile's bins.
struct RowsGrpDev {
    unsigned long long n, sum, sumsq, min, max;
    RowsSel sel;
    uint32_t hist[2 * kHhSelBins];
    unsigned long long bins[kTpBins];
};
struct RowsGrpWork {
    uint8_t *gflag;    // m bytes: bit 0 counted, bit 1 the last position of its key run
    uint32_t *cnt_c;   // rows_cnt_bytes(m): the counted flags' tile counts,
    uint32_t *cnt_e;   //   the group ends',
    uint32_t *cnt_l;   //   the listed groups' (over the groups)
    unsigned long long *gkey;  // per group: its key,
    uint32_t *gend;            //   the counted prefix at its end
    unsigned long long *lkey;  // per listed group: its key,
    uint32_t *lcount;          //   its count
};
// D zeroed, min all ones
hipError_t launch_rows_grp_init(RowsGrpDev *D, hipStream_t st);
// after launch_rows_last (W.flag = survivor): the two flags per sorted position, their scans, then per
// group its key and counted prefix; G.cnt_e[0] = groups
hipError_t launch_rows_grp_flags(const RowsLog &L, const uint32_t *pos, uint32_t m, int by, int valid_filter,
                                 uint32_t sod_from, const RowsWork &W, const RowsGrpWork &G, unsigned grid, int cus,
                                 hipStream_t st);
// over the groups: the counts, the statistics into D, the listed groups compacted to lkey / lcount
hipError_t launch_rows_grp_counts(const RowsGrpWork &G, uint32_t groups, RowsGrpDev *D, unsigned grid, int cus,
                                  hipStream_t st);
// the two median ranks over lcount[0 .. n): D->sel.prefix = med_lo, med_hi
hipError_t launch_rows_grp_median(const RowsGrpWork &G, uint32_t n, RowsGrpDev *D, unsigned grid, int cus,
                                  hipStream_t st);
hipError_t launch_rows_grp_out(const RowsGrpWork &G, uint32_t n, unsigned long long *out_key,
                               unsigned long long *out_count, unsigned grid, int cus, hipStream_t st);
// D->bins[tp_bin] += the counted survivors (after launch_rows_last)
hipError_t launch_rows_profile(const RowsLog &L, const uint32_t *pos, uint32_t m, int valid_filter, uint32_t sod_from,
                               const RowsWork &W, RowsGrpDev *D, unsigned grid, int cus, hipStream_t st);
// The group merge (DESIGN.md "Exact insights across shards"; the arithmetic is
// sketch_rows_merge.h's): (key, count) entries in any order to one ascending
// list of the keys' sums.  The device state beside RowsGrpDev, and the arrays
// in front of the group-by's back end (launch_rows_grp_counts / _median / _out
// over G, whose gend is the prefix of the counts here).
struct RowsMrgDev {
    unsigned long long total;  // the 64-bit sum of every entry's count
    unsigned long long multi;  // listed groups with more than one nonzero entry
    unsigned int wide;         // some count fails rows_merge_entry_ok
    unsigned int pad;
};
struct RowsMrgWork {
    const unsigned long long *counts;  // n_in entries' counts, as given
    const unsigned long long *keys_s;  // their keys, sorted,
    const uint32_t *idx_s;             //   and the entry each sorted position came from
    uint32_t *cnt_v;  // rows_cnt_bytes(n_in): the counts' u32 tile sums,
    uint32_t *cnt_z;  //   the nonzero entries' tile counts
    uint32_t *zend;   // per group: the nonzero entries at or before its end
};
// idx[i] = i, i < n
hipError_t launch_rows_iota(uint32_t *idx, uint32_t n, unsigned grid, int cus, hipStream_t st);
// M zeroed; then over the sorted positions the tile sums, end counts and nonzero counts, M->total and
// M->wide, the three scans, and per group its key (G.gkey), the prefix of the counts (G.gend) and of the
// nonzero flags (W.zend); G.cnt_e[0] = groups
hipError_t launch_rows_mrg_ends(const RowsMrgWork &W, const RowsGrpWork &G, uint32_t n_in, RowsMrgDev *M,
                                unsigned grid, int cus, hipStream_t st);
// M->multi over the groups
hipError_t launch_rows_mrg_multi(const RowsMrgWork &W, const RowsGrpWork &G, uint32_t groups, RowsMrgDev *M,
                                 unsigned grid, int cus, hipStream_t st);
// The compaction (DESIGN.md "Row log compaction"; the arithmetic is
// sketch_rows_compact.h's), after launch_rows_last over the whole log from the
// cutoff on (W.flag = survivor per sorted position, `kept` of them among m).
struct RowsCompactWork {
    uint8_t *keep;  // used bytes: 1 at a survivor's log position
    uint32_t *cnt;  // rows_cnt_bytes(used): the keep bytes' tile counts, scanned in place
    void *tmp_a;    // 8 * kept bytes each: a pair of log columns' survivors on their way to the front
    void *tmp_b;
};
// the survivors of positions [0, used) to [0, kept) in position order, then the head: used = kept, taken
// less the rows removed.  kept == 0 launches the head's kernel alone.
hipError_t launch_rows_compact(const RowsLog &L, uint32_t used, const uint32_t *pos, uint32_t m, const RowsWork &W,
                               uint32_t kept, const RowsCompactWork &K, unsigned grid, int cus, hipStream_t st);
// stable radix sort of (key, pos) pairs by key, signed or unsigned 64 bits (sketch_order.hip; the
// temporary is kScrSortTmp)
hipError_t rows_sort_pairs(Scratch *s, bool is_signed, const unsigned long long *keys, unsigned long long *keys_s,
                           const uint32_t *pos, uint32_t *pos_s, uint32_t m, hipStream_t st);

// sketch_hll_fmt.hip -- HLL keys as Redis "HYLL" strings, one key per workgroup
// (DESIGN.md section 14); the opcode rules are sketch_hll_fmt.h's
// sizes[i] = length of key i's string (slots == nullptr: keys 0 .. nkeys - 1);
// smb: the longest sparse payload before a key is written dense
hipError_t launch_hll_fmt_sizes(const uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                                uint32_t smb, uint32_t *sizes, int cus, hipStream_t st);
// string i at out + offs[i], offs the exclusive scan of the sizes (nkeys + 1
// entries); card (may be null): the cardinality the header caches, per key
hipError_t launch_hll_fmt_dump(const uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                               uint32_t smb, const uint64_t *card, const uint32_t *offs, uint8_t *out, int cus,
                               hipStream_t st);
// row of slots[i] = the registers of the string blob[offs[i] .. offs[i + 1])
// when it is valid; status (may be null): kHllFmtOk / NotHll / Corrupt per key;
// *anybad (zeroed by the caller) |= 1 when a string was not loaded
hipError_t launch_hll_fmt_load(uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                               const uint8_t *blob, const uint32_t *offs, uint8_t *status, unsigned int *anybad,
                               int cus, hipStream_t st);
// *bad (zeroed by the caller) |= 1 when offs[0 .. n] decreases somewhere
hipError_t launch_hll_fmt_offs_check(const uint32_t *offs, uint32_t n, unsigned int *bad, int cus, hipStream_t st);

// sketch_order.hip -- order-exact paths (replies that depend on item order)
struct Scratch;  // growable device scratch, owned by the context
constexpr int kScratchSlots = 64;

// Every slot of the context scratch, by owner (who sizes it) and user.  The
// numbers carry no meaning beyond identity; a slot belongs to exactly one of
// these ordering groups:
//   sync  used only inside synchronous calls, which run on the context stream
//         and end with a stream synchronise, so two such calls never overlap;
//   xr    K1's per-launch state, ordered through ske_ctx::xr (ScratchUser);
//   rt    routing's, ordered through ske_ctx::rt;
//   sn    the seen sets' per-item slots, ordered through ske_ctx::sn;
//   rw    the row logs' per-append state, ordered through ske_ctx::rw.
// The rule: a slot reachable from an rt-ordered call may have no user ordered
// through xr, and the other way round -- routing runs beside K1 on another
// stream (distributed.SwipeExchange's pipelined form), and neither waits for
// the other.  Slots shared on purpose are one enumerator naming both users.
enum ScratchSlot : int {
    // -- sync
    kScrKeysOrFirst,   // pfadd_exact: sort keys | ske_bf_madd: a link's first-setter table
                       // (up to 4 x bits bytes) | ske_rows_select, ske_rows_group, ske_rows_profile: a
                       // pass's sort keys, then ske_rows_group's (ske_rows_group_merge's) key per
                       // group; synchronous calls all, never at once
    kScrKeysSorted,    // pfadd_exact (sketch_order.hip), the row log's reads: sorted keys, then
                       //   ske_rows_group's key per listed group,
    kScrVals,          //   element indices (ske_rows_select: row positions),
    kScrValsSorted,    //   sorted indices,
    kScrRank,          //   ranks,
    kScrRankSorted,    //   ranks in sorted order,
    kScrPrefMax,       //   running maximum per register,
    kScrSortTmp,       //   rocprim radix sort temporary (also ske_rows_select's),
    kScrScanKeyTmp,    //   rocprim scan-by-key temporary
    kScrScanTmp,       // scan_inclusive_u32's rocprim temporary: ske_bf_madd, ske_keytab_lookup,
                       // ske_ingest_swipes, ske_ingest_dense, ske_hll_dump_sizes, ske_hll_dump
                       // (synchronous calls, never at once)
    kScrBfHa,          // ske_bf_madd: item hashes a,
    kScrBfHb,          //   hashes b,
    kScrBfState,       //   candidate state,
    kScrBfRes,         //   replies,
    kScrBfAbsent,      //   absent flags,
    kScrBfPos,         //   their prefix count
    kScrMergePartial,  // ske_hll_pfmerge over > 256 sources: partial maxima
    kScrKtFlag,        // key table lookup (ske_keytab_lookup, ske_ingest_swipes): found flags,
    kScrKtLen,         //   id lengths of found keys | ske_ingest_dense: decoded flags, their id lengths
    kScrKtIncl,        // ske_keytab_lookup: prefix count of the flags
    kScrInSlot,        // ske_ingest_swipes: slot per message,
    kScrInFlagIncl,    //   prefix count of the flags,
    kScrInLenIncl,     //   prefix sum of the id lengths (both also ske_ingest_dense's),
    kScrInIds,         //   packed ids,
    kScrInOffs,        //   their offsets,
    kScrInKslot,       //   their slots,
    kScrInKvalid,      //   K1's answers
    kScrHllFmtSize,    // ske_hll_dump_sizes, ske_hll_dump (sketch_api_hll.cpp): a string length per key,
    kScrHllFmtOffs,    //   their exclusive scan (nkeys + 1 offsets),
    kScrHllFmtCard,    //   ske_hll_dump with SKE_HLL_DUMP_CARD: a PFCOUNT per key
    kScrRowsSelFlag,   // ske_rows_select, ske_rows_group, ske_rows_profile: a flag byte per row (match, then
                       //   last of its run),
    kScrRowsSelCnt,    //   the totals and the per-tile counts of the flags
    kScrRowsGrpFlag,   // ske_rows_group: the counted and group-end bits per sorted position
                       //   | ske_rows_group_merge: the nonzero-entry prefix at each group's end (u32),
    kScrRowsGrpCnt,    //   the three tile-count arrays (counted, group ends, listed groups; the merge: four,
                       //   the counts' sums, group ends, nonzero entries, listed groups),
    kScrRowsGrpEnds,   //   the counted prefix (the merge: the prefix of the counts) at each group's end,
    kScrRowsGrpCounts, //   the listed groups' counts (u32), which the median select reads
    kScrRowsKeep,      // ske_rows_compact: a keep byte per log position,
    kScrRowsKeepCnt,   //   the totals and the per-tile counts of the keep bytes
    // -- xr
    kScrXr,            // launch_k1: the XCD-partitioned K1's state (sketch_xr.hip)
    kScrPartRec,       // part_scratch (sketch_part.hip): probe records,
    kScrPartOff,       //   run boundaries,
    kScrPartFail,      //   fail bytes (chains without fail lists),
    kScrPartHllw,      //   HLL words,
    kScrPartFlist,     //   fail lists of one-link chains
    kScrSegR1,         // seg_scratch (sketch_seg.hip): level-1 chunk arena,
    kScrSegFill,       //   fill counts,
    kScrSegCtab,       //   chunk table,
    kScrSegR2,         //   level-2 chunk rows,
    kScrSegO2,         //   their window offsets,
    kScrSegCb,         //   chunk bases,
    kScrSegQ,          //   the window pass's queue word,
    kScrSegQitems,     //   queue entries,
    kScrSegMlist,      //   cut windows,
    kScrSegCopies,     //   their window copies,
    kScrSegFloor,      //   the per-key floors of a group (a byte per key slot, bucket-major),
    kScrSegHot,        //   the hint map (a header and a byte per window; survives between calls),
    kScrSegFstat,      //   the floor statistics (ske_seg_floor_stats)
    // -- rt
    kScrRouteHist,     // ske_route_swipes, ske_route_swipes_cap_async: per-block histogram,
    kScrRouteTot,      // ske_route_swipes: the owners' totals
    // -- sn
    kScrSeenSlot,      // ske_seen_add_async: the slot each item's walk ended at, from the walk to the answers
    // -- rw
    kScrRowsFlag,      // ske_rows_append_*_async: a flag byte per item (taken, refused), from the flags to the place,
    kScrRowsIdv,       //   the parsed id per item,
    kScrRowsCnt,       //   the totals and the per-tile counts, scanned in place
    kScratchSlotCount
};
static_assert(kScratchSlotCount <= kScratchSlots, "Scratch holds kScratchSlots slots");

// The context's staging buffers (ske_ctx::stg) by use; every user is a
// synchronous call on the context stream.
enum StageSlot : int {
    kStgBytes,     // item bytes (stage_items; the fixed-width ids of ske_swipes_fixed*; ske_hll_load's blob)
    kStgOffs,      // item offsets (stage_items; ske_hll_load's string offsets)
    kStgSlots,     // a slot per item
    kStgOut,       // per-item replies on their way to the host (answers, changed flags, packed bits)
    kStgAnswers,   // ske_swipes_fixed_bits: answer bytes before packing
    kStgReply,     // small replies: PFCOUNT results, a histogram, a dense export
    kStgList,      // a slot list (PFCOUNT / PFMERGE / ske_hll_dump* / ske_hll_load) or key hashes (ske_keytab_insert)
    kStgList2,     // group offsets (PFCOUNT) or key slots (ske_keytab_insert)
    kStgCheck,     // the device slot-range check word (check_slots_dev)
    kStgCmsIncr,   // ske_cms_incrby: an increment per item
    kStgCmsReply,  // ske_cms_incrby / ske_cms_query: a u32 reply per item on its way to the host
    kStgCmsFlag,   // ske_cms_merge: the overflow word of the check pass, then the sources' counts
    kStgHhFlag,    // ske_hh_track: the too-long word | ske_hh_list: the count of entries that pass
    kStgHhIds,     // ske_hh_list: the entries' id words,
    kStgHhLen,     //   lengths,
    kStgHhEst,     //   estimates
    kStgHhStat,    // ske_hh_stats / ske_hh_select: the accumulators, the rank state and the histograms (HhStatDev),
    kStgHhSelEst,  //   the passing estimates, compacted (4 bytes per slot of the set)
    kStgHllFmtBlob,    // ske_hll_dump: the strings on their way to the host
    kStgHllFmtStatus,  // ske_hll_load: a status byte per key on its way to the host
    kStgHllFmtFlag,    // ske_hll_load: the offsets-decrease word, then the any-string-refused word
    kStgTallyFlag,     // ske_tally_add: the too-long word | ske_tally_list / ske_tally_top: the count of entries that pass
    kStgTallyMask,     // ske_tally_add: a mask byte per item
    kStgTallyKeys,     // ske_tally_list / ske_tally_top: the entries' key words | ske_tally_import: the keys,
    kStgTallyLen,      //   lengths,
    kStgTallyEv,       //   events (also ske_tally_query's reply on its way to the host),
    kStgTallyVa,       //   valid (likewise)
    kStgSeenKeys,      // ske_seen_add / ske_seen_test: the keys,
    kStgSeenMask,      //   ske_seen_add: a mask byte per item,
    kStgSeenOut,       //   the answers on their way to the host
    kStgRowsLec,       // ske_rows_append: the lecture bytes | ske_rows_select / ske_rows_read: the digests on their way out
                       //   | ske_rows_group: the keys on their way to the host,
    kStgRowsLecOffs,   //   ske_rows_append: the lecture offsets,
    kStgRowsId,        //   the id bytes | ske_rows_select: the ids on their way to the host
                       //   | ske_rows_group_merge: host keys on their way in,
    kStgRowsIdOffs,    //   the id offsets | ske_rows_group_merge: host counts on their way in,
    kStgRowsEpoch,     //   the epochs (both directions) | ske_rows_group: the counts on their way to the host,
    kStgRowsValid,     //   the valid bytes (both directions)
    kStgRowsGrp,       // ske_rows_group / ske_rows_profile: the statistics, the select state and the bins (RowsGrpDev)
    kStgRowsMrg,       // ske_rows_group_merge: the total, the wide word and multi (RowsMrgDev)
    kStageSlotCount
};

Scratch *scratch_new();
void scratch_delete(Scratch *s);
void *scratch_get(Scratch *s, ScratchSlot slot, size_t bytes, hipError_t *err);
// the same for a slot whose content is kept from call to call: a buffer newly
// allocated (or grown) is handed out zeroed
void *scratch_get_zeroed(Scratch *s, ScratchSlot slot, size_t bytes, hipError_t *err);
void *scratch_peek(const Scratch *s, ScratchSlot slot);  // the slot's buffer as it stands (may be null)
void scratch_set_recording(Scratch *s, bool on);  // slots handed out now get pinned
void scratch_unpin(Scratch *s);                    // every graph freed: slots may grow

// PFADD with per-element "changed" flags in sequential order.
hipError_t pfadd_exact(Scratch *s, const uint32_t *slot, const uint8_t *bytes,
                       const uint32_t *offs, uint64_t n, uint8_t *regs, uint32_t nslots,
                       uint8_t *changed_dev, unsigned int *err_dev, int cus, hipStream_t st);

// BF.MADD helpers (the epoch driver lives in the API TU, which owns links)
hipError_t launch_bf_hash(const uint8_t *bytes, const uint32_t *offs, uint64_t n, uint64_t *ha,
                          uint64_t *hb, int cus, hipStream_t st);
// items with state==0 that are present in any of ch's links: state=1, res=0
hipError_t launch_bf_settle_present(const ChainDev &ch, uint64_t n, const uint64_t *ha,
                                    const uint64_t *hb, uint8_t *state, int8_t *res, int cus,
                                    hipStream_t st);
hipError_t launch_bf_first_setter(const LinkDev &L, uint64_t n, const uint64_t *ha,
                                  const uint64_t *hb, const uint8_t *state, uint32_t *first,
                                  int cus, hipStream_t st);
hipError_t launch_bf_absent(const LinkDev &L, uint64_t n, const uint64_t *ha, const uint64_t *hb,
                            const uint8_t *state, const uint32_t *first, uint32_t *absent,
                            int cus, hipStream_t st);
hipError_t scan_inclusive_u32(Scratch *s, const uint32_t *in, uint32_t *out, uint64_t n,
                              hipStream_t st);
// resolve candidates with index <= cutoff; absent ones are added (bits set)
hipError_t launch_bf_resolve(const LinkDev &L, uint64_t n, const uint64_t *ha, const uint64_t *hb,
                             uint8_t *state, const uint32_t *absent, const uint32_t *pos,
                             uint32_t cap, int8_t *res, uint8_t *bf_mut, int cus,
                             hipStream_t st);
// counter[0] += items with state == 0 (candidates not yet resolved)
hipError_t launch_bf_count_cands(uint64_t n, const uint8_t *state, unsigned long long *counter,
                                 int cus, hipStream_t st);
// mark every remaining candidate with a result code (non-scaling full)
hipError_t launch_bf_fill_rest(uint64_t n, uint8_t *state, int8_t *res, int8_t code, int cus,
                               hipStream_t st);

// host -> device staging of pageable caller buffers (sketch_host.cpp)
struct HostStager;
HostStager *stager_new();
void stager_delete(HostStager *s);
hipError_t stage_h2d(HostStager *s, void *dst, const void *src, size_t bytes, hipStream_t st, bool mono,
                     bool *ok);

}  // namespace ske
