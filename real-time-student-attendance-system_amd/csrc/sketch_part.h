// sketch_part.h -- what the two halves of the partitioned K1 share: passes
// A/B/C (sketch_part.hip) and the segmented PFADD that replaces pass C when a
// batch's register updates are dense in the slab (sketch_seg.hip).  Geometry,
// the kernels' argument structs, the device helpers both use, and the seg
// half's host entry points.  csrc-internal.
#pragma once
#include "sketch_common.h"
#include "sketch_internal.h"
#include "sketch_seg_plan.h"

namespace ske {

constexpr uint32_t kPSub = 1u << 26;                // swipes per sub-batch (passes A-B-C), at most
constexpr uint32_t kPbGroup = 8;                    // tiles a pass-B wave reads at once
constexpr uint32_t kPbLanes = 64 / kPbGroup;        // lanes per tile run
constexpr uint32_t kPTileLog = 10;
constexpr uint32_t kPTile = 1u << kPTileLog;        // swipes per tile, every chain's

struct PartLink {
    const uint8_t *bf;
    uint64_t m;          // Granlund-Montgomery magic of d
    uint32_t d;          // bloom->bits (<= 2^31)
    uint32_t t;          // 2^64 mod d
    uint32_t sh;         // l - 1 of the magic
    uint32_t k;          // bloom->hashes
    uint32_t slice0;     // first global slice of this link
    uint32_t nbytes16;   // bit-array bytes rounded up to 16 (readable)
};

struct PartArgs {
    const uint8_t *bytes;
    const uint32_t *offs;  // nullptr: fixed-width ids
    const uint32_t *slot;
    uint8_t *regs;
    uint8_t *out;          // may be nullptr
    unsigned int *err;
    uint32_t *rec;         // [ntiles][stride] probe records
    uint32_t *off;         // [nslices + 1][off_stride] run boundaries (slice-major)
    uint8_t *fail;         // [nlinks][fail_stride]
    uint32_t *hllw;        // [n] register | rank << 16
    uint32_t fixed_w, n, stride, ntiles, nslices, nlinks, ksum, nslots, fail_stride, off_stride;
    uint16_t *flist;       // [nunits][fl_stride][kPbLanes] fail lists (pass B -> pass C), or nullptr
    uint32_t nunits, fl_stride;
    PartLink link[kPMaxLinks];
};

// A workgroup barrier for hand-offs through LDS only: it waits for this
// wave's LDS operations (lgkmcnt(0)) and not for its global loads and stores
// in flight, which __syncthreads() drains too (vmcnt(0)).  The partitioned
// passes share nothing through global memory inside a block, so the next
// tile's prefetched ids (pass A), the next round's records (pass B) and the
// register CASes (pass C) stay in flight across their barriers.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Tiles are dealt to kPGroups contiguous groups, and every pass gives the
// blocks b with b % kPGroups == x the tiles of group x.  Blocks are dealt
// round-robin over the 8 XCDs, so a group's fail bytes (2 MB at C3) are
// written by pass A, set by pass B and read by pass C in one XCD's L2.  This
// is placement for speed only: every tile of a group is handled by exactly one
// block of the group, whichever XCD it runs on.
constexpr uint32_t kPGroups = 8;
// (group edges on multiples of 8 tiles: pass B's rounds of 8 tiles never
// straddle two XCD groups)
__device__ __forceinline__ void part_group(uint32_t ntiles, uint32_t x, uint32_t &t0, uint32_t &t1) {
    t0 = uint32_t(uint64_t(ntiles) * x / kPGroups) & ~7u;
    t1 = x + 1 == kPGroups ? ntiles : uint32_t(uint64_t(ntiles) * (x + 1) / kPGroups) & ~7u;
}

// Bit (pos & 31) of w: v_bfe_u32 reads only its offset operand's low 5 bits,
// so pos goes in as it is (the compiler's ubfe masks it first: one VALU per
// probe record in pass B)
__device__ __forceinline__ uint32_t part_bit(uint32_t w, uint32_t pos) {
    uint32_t r;
    asm("v_bfe_u32 %0, %1, %2, 1" : "=v"(r) : "v"(w), "v"(pos));
    return r;
}

// ((1 << width) - 1) << offset (width, offset < 32) as one v_bfm_b32
__device__ __forceinline__ uint32_t part_bfm(uint32_t width, uint32_t offset) {
    uint32_t r;
    asm("v_bfm_b32 %0, %1, %2" : "=v"(r) : "v"(width), "s"(offset));
    return r;
}

// Inclusive prefix sum over a wave's 64 lanes on DPP: row shifts 1, 2, 4, 8
// inside 16-lane rows, then row_bcast:15 / row_bcast:31 across rows (gfx9);
// a lane whose source is outside its row adds the identity.  VALU only.
__device__ __forceinline__ uint32_t part_wave_scan(uint32_t v) {
    v += __builtin_amdgcn_update_dpp(0u, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0u, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0u, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0u, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0u, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1, 3
    v += __builtin_amdgcn_update_dpp(0u, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2, 3
    return v;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t part_rsrc(const void *p, uint32_t nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, int(nbytes), 0x00020000);
}

// Streams read or written once take the non-temporal policy (`nt`); SKE_NT
// bits select them -- 1 pass B's run boundaries, 2 pass A's ids and offsets,
// 4 pass A's record copy-out, 8 pass A's HLL words and fail bytes, 16 pass
// C's streams (fail bytes, slots, HLL words, answers), 32 pass C's register
// pre-check loads, 64 pass B's probe records.  Measured at C3 (A/B,
// two alternations): records nt: pass B 0.276 -> 0.260 ms; + bits 1|2|4:
// 0.25 ms; bits 8 and 16 neutral to slightly slower; bit 32 makes pass C
// 0.39 -> 0.59 ms (the raising CAS no longer finds its line near).  Default 7.
// (Round 4, final kernels: 15 and 23 within 0.1 % of 7, profiles/r04_ab_nt.txt.)
// Bit 64 (pass B's records) was always on before round 5 (default 71).
// Round 6, the segmented PFADD at 2^28-swipe steps (profiles/r06_ab_nt.txt,
// three sessions, N = 1 and the 8-way shard): pass B's record loads without
// `nt` and the copy-out with it -- pass B 0.39 -> 0.37 ms per 2^25 sub-batch --
// and C1's streams (bit 16) with it -- C1 0.116 -> 0.099 -- and pass A's HLL
// words (bit 8) with it (pass B 0.370 -> 0.364): default 29 (1 | 4 | 8 | 16),
// step 9.2 -> 8.85-8.9 ms; without bit 4, or with bit 64, pass B is back at
// 0.38+; bit 2 (pass A's ids) costs pass B 0.01.
#ifndef SKE_NT
#define SKE_NT 29
#endif
typedef uint32_t part_u32x4 __attribute__((ext_vector_type(4)));
template <int BIT, class T> __device__ __forceinline__ T nt_ld(const T *p) {
    if constexpr ((SKE_NT & BIT) != 0) return __builtin_nontemporal_load(p);
    else return *p;
}
template <int BIT, class T> __device__ __forceinline__ void nt_st(T *p, T v) {
    if constexpr ((SKE_NT & BIT) != 0) __builtin_nontemporal_store(v, p);
    else *p = v;
}
// (the buffer builtins' cache-policy operand, an immediate: a constant, not a call)
template <int BIT> constexpr int kNtAux = (SKE_NT & BIT) ? 2 : 0;
// The segmented PFADD's streams (SKE_NT2 bits): 1 C1's level-1 record
// copy-out, 2 D's level-1 record loads, 4 D's level-2 record copy-out, 8 the
// window pass's record loads, 16 its register-image loads (LDS-DMA), 32 its
// line write-back.  Default 0 (round 5's policies).
#ifndef SKE_NT2
#define SKE_NT2 0
#endif
template <int BIT> constexpr int kNt2Aux = (SKE_NT2 & BIT) ? 2 : 0;
template <int BIT, class T> __device__ __forceinline__ void nt2_st(T *p, T v) {
    if constexpr ((SKE_NT2 & BIT) != 0) __builtin_nontemporal_store(v, p);
    else *p = v;
}

constexpr uint32_t kOOR = 0x80000000u;  // a buffer offset past every range: load 0, store dropped

// byte max of a register in the slab, by CAS from the pre-check load `old`
__device__ __forceinline__ void part_reg_max(uint32_t *w, uint32_t sh, uint32_t rank, uint32_t old) {
    while (((old >> sh) & 0xffu) < rank) {
        const uint32_t prev = atomicCAS(w, old, (old & ~(0xffu << sh)) | (rank << sh));
        if (prev == old) return;
        old = prev;
    }
}

constexpr uint32_t kSegRunTiles = kPbGroup;                 // tiles per level-1 run
constexpr uint32_t kSegRunSw = kSegRunTiles * kPTile;       // 8192 swipes
constexpr uint32_t kSegMaxB1 = 512;                         // level-1 buckets
constexpr uint32_t kSegMaxWpb = 512;                        // windows per bucket
// (kSegChunk, 8192 records per level-2 chunk: sketch_seg_plan.h)
static_assert(kSegRunSw == kSegRun, "sketch_seg_plan.h sizes the arena for runs of kSegRunSw swipes");
constexpr uint32_t kSegMaxRuns = kPSub / kSegRunSw;         // 8192 runs per sub-batch
constexpr uint32_t kSegRecShift = 20;                       // record: slot-in-bucket above bit 20
static_assert(kSegMaxRuns < 65536, "k_seg_c1's uint16 mark epochs (run + 1) would wrap");

struct SegArgs {
    uint32_t *r1;     // [chunk slots][kSegChunk] level-1 records of a sub-batch: each bucket's sequence in chunks
    uint32_t *r2;     // [nsub][maxch][kSegChunk] level-2 records, window-sorted per chunk
    uint32_t *o2;     // [nsub][maxch][wpb + 1] window w's start in chunk q
    uint32_t *cb;     // [nsub][nb1 + 1] first chunk of bucket h in sub-batch s (prefix)
    uint32_t nruns;   // level-1 runs of this sub-batch
    uint32_t nb1;     // level-1 buckets: 2^b1, window W = slot >> klog in bucket W & (nb1 - 1)
    uint32_t b1;      // log2(nb1)
    uint32_t s1;      // bits of a record's slot-in-bucket: (W >> b1) << klog | slot & (2^klog - 1) (<= 12)
    uint32_t wlog;    // windows per bucket = 1 << wlog
    uint32_t klog;    // keys per window = 1 << klog
    uint32_t s;       // this sub-batch's index in the call
    uint32_t nsub;    // sub-batches of the call
    uint32_t maxch;   // level-2 chunk slots per sub-batch
    uint32_t nwin;    // windows of the slab (E)
    uint32_t dense_min;  // E: records at which a window is staged in LDS
    uint32_t *q;      // window pass queue header: [0] queued slices, [1] copies, [2] cut windows, [5] E2 items
                      // and [8 + x] XCD x's E1 items claimed past the first gridDim.x (zeroed per window pass)
    uint4 *qitems;    // queued slices (window, slice, copy)
    uint4 *mlist;     // cut windows (window, first copy, slices)
    uint8_t *copies;  // [ccap][window bytes] LDS copies of cut windows' slices
    uint32_t ccap;    // copies (and queue entries) available
    // the arena: level-1 records in chunk slots of r1
    uint32_t *fill;   // [nsub][nb1 + 1] (x kSegFillStride words) records reserved per bucket; [s][nb1] =
                      // counted chunk slots taken
    uint32_t *ctab;   // [nb1][kmaxc] chunk c of bucket h: its slot + 1 (0: not yet placed)
    uint32_t kmaxc;   // chunks a bucket can have in a sub-batch
    uint32_t kstat;   // chunk c < kstat of bucket h sits in slot h * kstat + c; later chunks take
                      // slots nb1 * kstat + (counter), named in ctab
    unsigned int *err;  // the call's error word (D: bit 8, more chunks than maxch rows)
    // the per-key floors (sketch_seg.hip, k_seg_floor); all null with option "seg_floor" 0
    uint8_t *floor;   // [nb1 << s1] the group's floor of key slot (W & (nb1 - 1)) << s1 | slot-in-bucket
    uint8_t *hot;     // kSegHotHdr header bytes (the plan the map belongs to), then a hint byte per window
    unsigned long long *fstat;  // [0] windows floored, [1] records D saw, [2] records D dropped
    uint32_t hot_min;  // arrivals per key and group from which E hints a window
};
constexpr uint32_t kSegHotHdr = 16;          // the hint map's header: nwin, klog, b1, kSegHotMagic
constexpr uint32_t kSegHotMagic = 0x686f7431u;
constexpr uint32_t kSegHotAge = 4;           // groups a hint outlives E's last visit

// the fail-list instantiation: one link of k = 11 (C3/C5's filter), slice
// pairs (the sink pair must fit k_part_a3<11, 2048>'s counters)
inline bool part_flist(const PartArgs &A) { return A.nlinks == 1 && A.ksum == 11 && A.nslices <= 2046; }

// sketch_seg.hip -- host side.  hook: launch_swipes_part's pass-timing hook.
// segmented for this batch?  (fills P)
bool seg_use(const PartArgs &A, const SegOpts &so, uint32_t nslots, uint64_t n, uint32_t sub, SegPlan *P);
// the scratch of a batch of n swipes in sub-batches of `sub`, and S's geometry
hipError_t seg_scratch(const SegPlan &P, uint32_t sub, uint64_t n, Scratch *scr, SegArgs *S);
// C1 + D of the call's sub-batch si (A: the sub-batch after pass B); hook kinds 2 and 3
hipError_t launch_seg_sub(const PartArgs &A, SegArgs &S, const SegPlan &P, uint32_t si, int cus, hipStream_t st,
                          PassHook hook, void *hook_user);
// the window pass over the last ns sub-batches (E1, E2, M); hook kind 4
hipError_t launch_seg_windows(PartArgs A, SegArgs S, const SegPlan &P, uint32_t ns, int cus, hipStream_t st,
                              PassHook hook, void *hook_user);

}  // namespace ske
