// sketch_part.hip -- K1 for Bloom chains too large for one CU's LDS (C3/C5:
// the 19.8 MB RESERVE 0.001 / 1e7 filter), partitioned: every probe is tested
// against an LDS-resident 64 KiB slice of its link.
//
// Same answers as every K1 variant: per swipe BF.EXISTS (SBChain_Check: a link
// says "present" iff all k probe bits (a + i*b) mod 2^64 mod bits are set, the
// chain iff any link does -- attendance_processor.py:109-113) and, if present,
// PFADD (hllPatLen -> register max, :127-129).
//
// Why partitioned.  A random probe into a 19.8 MB bit array is a random line
// request: 55 G/s chip-wide from the Infinity Cache or HBM, 252 G/s from a
// slice kept L2-resident per XCD (tools/randbench.hip).  176 M probes per
// 16 M-swipe step are then 0.7 ms even at the L2 rate.  A random ds_read_u8
// from LDS runs at 4.6 T/s.  The whole filter (19.8 MB) fits in the chip's
// aggregate LDS (256 x 160 KiB), so the probes are routed to the CU holding
// their slice instead -- a radix partition of 4-byte probe records, streamed
// through HBM in whole lines:
//
//   pass A             per tile of 1024 swipes: hash each id (MurmurHash64A
//                      a, b, and the HLL hash), walk every link's k probes,
//                      and emit one 4-byte record per probe (its bit offset in
//                      the slice unit | the swipe's index in the tile),
//                      counting-sorted by slice in LDS and written out as one
//                      contiguous run per (tile, slice unit); off[slice][tile]
//                      holds the run boundaries.  Also the HLL word (register
//                      | rank << 16; one-link k = 11 chains: its top byte is
//                      the swipe's overflow flag) and, for other chains, a
//                      cleared fail byte per swipe.
//   pass B             per slice unit (one slice, or a pair of a one-link
//                      chain's adjacent slices), staged into LDS: the unit's
//                      run of every tile in the block's range; a failing
//                      probe's swipe goes to the tile's fail list (one-link
//                      k = 11 chains; a full list's overflow sets the HLL
//                      word's top byte) or sets its fail byte.
//   pass C             per swipe: valid = no failed probe in some link; the
//                      answer; register max (pre-check load, CAS).
//
// Two instantiations of the passes, picked by the host per chain:
//   * one link of k = 11 (C3/C5's RESERVE 0.001 / 1e7 filter, the headline):
//     k_part_a3 -> k_part_b<2, 4, true> -> k_part_c_fl (slice pairs, dense
//     pair runs, fail lists);
//   * any other chain the slice plan takes (several links, or k != 11; up to
//     22 probes per swipe): k_part_a -> k_part_b<1 or 2> -> k_part_c (fail
//     bytes).
// For the first, dense batches replace pass C by the segmented PFADD
// (sketch_seg.hip); sketch_part.h holds what the two files share.
// Variants measured slower were removed in round 4 (DESIGN.md §3 keeps their
// numbers): 512-thread pass A without fail lists, 2048-swipe tiles, the
// 16-copy counter table, pass A at three blocks per CU, the register
// pre-check in pass A, PFADD by owned register lines, pass C on a side or
// CU-masked stream; in round 4 also pair runs padded to 128-B lines, the
// tile parity unrolled, and a two-phase pass C.
// Round 8 removed the forms that had stayed selectable at build time after
// losing their A/B (their numbers stand in DESIGN.md §3 / §3a):
//   * pass A's sort as count, scan, place, also at three blocks per CU: 0.470
//     (two blocks) and 0.441 ms (three) against the rank sort's 0.426 ms per
//     2^25 sub-batch (profiles/r07_ab_pa_place.txt);
//   * pass A's ids one tile ahead instead of two (profiles/r05_ab_pass_a.txt,
//     profiles/r06_ab_split_ahead.txt), its wait for the atomics after every
//     swipe instead of after the last (0.226-0.230 -> 0.225 ms,
//     profiles/r04_ab_pa_wait.txt), and its sort phases at the hashing's wave
//     priority (0.428 -> 0.396 ms raised, profiles/r07_ab_pa_place.txt);
//   * 1536-swipe tiles for the fail-list chains: not kept in round 6
//     (profiles/r06_ab_tile1536.txt);
//   * pass B's block shares 0 (per XCD tile group, unit major), 1 (all tiles,
//     unit major) and 2 (units round robin, no equal shares of the rest):
//     0.368 -> 0.362 ms per 2^25 sub-batch for the one kept
//     (profiles/r05_ab_pass_b_split.txt);
//   * the segmented PFADD's run-table form (C1's runs as blocks, a scan pass
//     S, D gathering from the runs; with it D's pipelined table loads, 0.101
//     -> 0.106 ms, profiles/r06_ab_seg_c1d.txt): C1 + S + D 0.195 ms against
//     the arena's 0.169 per 2^25 sub-batch (profiles/r06_ab_seg_arena.txt);
//   * other block shapes of pass C (0.406 ms at 256 x 4 against 0.400 at 1024
//     x 1, profiles/r04_ab_pc_shape.txt), C1 and D at 1024 threads and two
//     blocks per CU (profiles/r06_ab_seg_c1_blocks.txt, r06_ab_seg_d_blocks.txt),
//     the window pass at every gridDim.x-th item instead of claimed ones
//     (profiles/r05_ab_seg_slice.txt), two records per thread at klog 1 (spills,
//     profiles/r06_ab_seg_e_rpt.txt) and slices of 8 k to 128 k records (0.930
//     -> 0.891 ms for 32 k << klog, profiles/r05_ab_seg_slice.txt).
// Round 19 removed the last form kept behind an option after losing its A/B:
//   * pass A's group layout (a slice unit's runs of 8 consecutive tiles
//     adjacent in a (group, unit) region, runs that do not fit in overflow
//     rows; taken on request only): pass B 0.194-0.195 -> 0.182-0.183 ms but
//     pass A 0.225-0.228 -> 0.380-0.388 ms per 16 M sub-batch, a net +0.14 ms
//     (profiles/r05_ab_rec_groups.txt; DESIGN.md §3 keeps the table).
//
// Placement of blocks on XCDs is a speed matter only; every (tile, slice) run
// is read by exactly one block, and fail marks are only ever set.
#include <algorithm>

#include "sketch_part.h"

namespace ske {

constexpr uint32_t kPaBlock = kPTile;         // k_part_a: one thread per swipe of a tile
constexpr uint32_t kPbBlock = 1024;
constexpr uint32_t kPcBlock = 256;            // k_part_c (fail bytes)
constexpr uint32_t kPSliceMask = kPSliceBits - 1;
constexpr uint32_t kPSliceBytes = kPSliceBits / 8;  // 64 KiB
// pass C (fail lists): 1024 threads x 1 swipe per tile (round 4 A/B, three
// alternations: 0.406-0.407 ms at 256 x 4, 0.402 at 512 x 2, 0.400 at 1024 x 1),
// 8 blocks' worth of runs per CU in the grid
constexpr uint32_t kPcFlT = 1024;
constexpr uint32_t kPcFlBlocksPerCu = 8;

__device__ __forceinline__ Divisor part_div(const PartLink &L) { return Divisor{L.d, L.m, L.t, L.sh, 0}; }

// ---------------------------------------------------------------------------
// ids of at most 8 bytes (every config's student ids), read and hashed the way
// the LDS K1 does (sketch_k1.hip): the one or two aligned 64-bit words holding
// the id (an empty or long id reads zeros past the range), a funnel shift and
// a length mask, MurmurHash64A in closed form h = ((seed ^ len*m) ^ t) * m then
// the finaliser, t the id word or (len 8) its mixed block, mixed once for the
// three hashes.  A wave holding a longer id takes the generic routines.
// ---------------------------------------------------------------------------
struct PartId {
    uint32_t b, len;
    uint64_t w0, w1;
};

__device__ __forceinline__ void part_id_load(const __amdgpu_buffer_rsrc_t &rb, uint32_t b, uint32_t e,
                                             PartId &d) {
    d.b = b;
    d.len = e - b;
    const uint32_t s8 = b & 7;
    const bool sh = d.len && d.len <= 8;
    const uint32_t o0 = sh ? (b & ~7u) : 0xfffffff8u;
    // (an id inside one aligned word needs no second word: its load goes
    // past the range, no memory access; the hash masks those bytes off)
    const uint32_t o1 = (sh && s8 + d.len > 8) ? o0 + 8 : 0xfffffff8u;
    d.w0 = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(rb, o0, 0, kNtAux<2>));
    d.w1 = __builtin_bit_cast(uint64_t, __builtin_amdgcn_raw_buffer_load_b64(rb, o1, 0, kNtAux<2>));
}

__device__ __forceinline__ void part_hash3(const uint8_t *bytes, const PartId &d, uint64_t &ha, uint64_t &hb,
                                           uint64_t &hh) {
    if (__any(d.len > 8)) {
        const Item it = load_item(bytes, d.b, d.b + d.len);
        ha = murmur_item(it, kBloomSeed);
        hb = murmur_item(it, ha);
        hh = murmur_item(it, kHllSeed);
        return;
    }
    const uint32_t sh = (d.b & 7) * 8;
    const bool hi = sh >= 32;
    const uint32_t a = hi ? uint32_t(d.w0 >> 32) : uint32_t(d.w0);
    const uint32_t bb = hi ? uint32_t(d.w1) : uint32_t(d.w0 >> 32);
    const uint32_t c = hi ? uint32_t(d.w1 >> 32) : uint32_t(d.w1);
    const uint64_t v = (uint64_t(__builtin_amdgcn_alignbit(c, bb, sh & 31)) << 32) |
                       __builtin_amdgcn_alignbit(bb, a, sh & 31);
    const uint32_t drop = (64 - d.len * 8) & 63;
    uint64_t tw = (v << drop) >> drop;
    if (__any(d.len == 8)) {
        uint64_t k = tw * kMurmurM;
        k ^= k >> 47;
        k *= kMurmurM;
        tw = d.len == 8 ? k : tw;
    }
    const uint64_t t = tw ^ (uint64_t(d.len) * kMurmurM);
    const bool nz = d.len != 0;
    ha = mm_final(nz ? (kBloomSeed ^ t) * kMurmurM : kBloomSeed);
    hb = mm_final(nz ? (ha ^ t) * kMurmurM : ha);
    hh = mm_final(nz ? (kHllSeed ^ t) * kMurmurM : kHllSeed);
}

// ---------------------------------------------------------------------------
// pass A: hash, probe records, counting sort by slice
// ---------------------------------------------------------------------------
// One tile = 1024 swipes, one per thread.  KM: the most probes per swipe the
// instantiation holds (every link's k summed); records of a tile live in LDS
// (KM = 11: 44 KiB, two blocks per CU, so one block's hashing overlaps the
// other's sort and copy-out).  One-link chains of k = 11 (C3/C5) take
// k_part_a2 below.
template <int KM>
__global__ void __launch_bounds__(kPaBlock, KM <= 11 ? 8 : 4) k_part_a(const PartArgs A) {
    __shared__ __attribute__((aligned(16))) uint32_t srec[kPTile * KM];
    // slice histogram, then run starts; two buffers used by alternate tiles,
    // so the one the next tile counts into is cleared while this tile still
    // reads its own (four barriers per tile)
    __shared__ uint32_t scnt2[2][kPMaxSlices + 1];
    __shared__ uint32_t swsum[kPaBlock / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t S = A.nslices;
    for (uint32_t g = tid; g <= kPMaxSlices; g += kPaBlock) scnt2[0][g] = scnt2[1][g] = 0;
    __syncthreads();
    // the next tile's ids are loaded while this tile sorts: its offsets at the
    // top of the iteration, its id words after the scan
    auto offsets = [&](uint32_t t, uint32_t &b, uint32_t &e) {
        const uint32_t i = t * kPTile + tid;
        const uint32_t ic = i < A.n ? i : A.n - 1;
        b = A.offs ? A.offs[ic] : ic * A.fixed_w;
        e = A.offs ? A.offs[ic + 1] : b + A.fixed_w;
    };
    uint32_t gt0, gt1;
    part_group(A.ntiles, blockIdx.x % kPGroups, gt0, gt1);
    const uint32_t tstep = gridDim.x / kPGroups;
    const __amdgpu_buffer_rsrc_t rbytes = part_rsrc(A.bytes, 0xfffffff0u);
    uint32_t par = 0, nb_ = 0, ne_ = 0;
    PartId it;
    {
        const uint32_t t = gt0 + blockIdx.x / kPGroups;
        offsets(t < gt1 ? t : gt0, nb_, ne_);
        part_id_load(rbytes, nb_, ne_, it);
    }
    for (uint32_t t = gt0 + blockIdx.x / kPGroups; t < gt1; t += tstep, par ^= 1) {
        uint32_t *scnt = scnt2[par];
        uint32_t rv[KM], rp[KM];
        const uint32_t tn = t + tstep < gt1 ? t + tstep : t;
        offsets(tn, nb_, ne_);
        {
            const uint32_t i = t * kPTile + tid;
            const bool act = i < A.n;
            uint64_t ha, hb, hh;
            part_hash3(A.bytes, it, ha, hb, hh);
            if (act) {
                uint32_t idx, rank;
                hll_patlen(hh, idx, rank);
                A.hllw[i] = idx | (rank << 16);
                for (uint32_t l = 0; l < A.nlinks; l++) A.fail[size_t(l) * A.fail_stride + i] = 0;
            }
            // every link's k probes in RedisBloom's order, newest link first
            // (the order is immaterial to the answer; records carry no link:
            // a slice belongs to one link)
            // bit 29 of a record: its slice's parity (pass B's slice pairs)
            const uint32_t rbase = (tid << kPSliceLog) | 0x80000000u;
            {
                uint32_t l = A.nlinks - 1, jl = 0;
                ProbeWalk32 wk;
                wk.init(ha, hb, part_div(A.link[l]));
#pragma unroll
                for (int q = 0; q < KM; q++) {
                    rp[q] = 0xffffffffu;
                    rv[q] = 0;
                    if (uint32_t(q) < A.ksum) {  // block-uniform
                        if (jl == A.link[l].k) {
                            l--;
                            jl = 0;
                            wk.init(ha, hb, part_div(A.link[l]));
                        }
                        const uint32_t x = wk.x;
                        const uint32_t g = A.link[l].slice0 + (x >> kPSliceLog);
                        rv[q] = (x & kPSliceMask) | ((g & 1u) << 29) | rbase;
                        if (act) rp[q] = (g << 16) | atomicAdd(&scnt[g], 1u);
                        wk.step(A.link[l].d);
                        jl++;
                    }
                }
            }
        }
        __syncthreads();
        part_id_load(rbytes, nb_, ne_, it);  // the next tile's ids
        // exclusive scan of scnt[0..S] (scnt[S] == 0 becomes the tile's total)
        constexpr int kPer = (kPMaxSlices + 1) / kPaBlock;
        uint32_t v[kPer], s = 0;
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            v[j] = scnt[tid * kPer + j];
            s += v[j];
        }
        uint32_t incl = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = __shfl_up(incl, o, 64);
            if (lane >= uint32_t(o)) incl += y;
        }
        if (lane == 63) swsum[wave] = incl;
        __syncthreads();
        uint32_t run = incl - s;
        for (uint32_t w = 0; w < wave; w++) run += swsum[w];
#pragma unroll
        for (int j = 0; j < kPer; j++) {
            scnt[tid * kPer + j] = run;
            run += v[j];
        }
        __syncthreads();
        // run boundaries, slice-major: off[g][t] (a pass-B wave reads the
        // boundaries of consecutive tiles of its slice as two short rows)
        for (uint32_t g = tid; g <= S; g += kPaBlock) A.off[size_t(g) * A.off_stride + t] = scnt[g];
#pragma unroll
        for (int q = 0; q < KM; q++)
            if (rp[q] != 0xffffffffu) srec[scnt[rp[q] >> 16] + (rp[q] & 0xffffu)] = rv[q];
        // the next tile's histogram (its previous readers passed two barriers ago)
        for (uint32_t g = tid; g <= S; g += kPaBlock) scnt2[par ^ 1][g] = 0;
        __syncthreads();
        // copy-out; the next tile places records only after three more barriers
        const uint32_t total = scnt[S];
        uint4 *dst = reinterpret_cast<uint4 *>(A.rec + size_t(t) * A.stride);
        const uint4 *src = reinterpret_cast<const uint4 *>(srec);
        for (uint32_t j = tid; j * 4 < total; j += kPaBlock) dst[j] = src[j];
    }
}

// Pass A of the fail-list path (one link, k = KM, slice pairs, 1024-swipe
// tiles, 512 threads x 2 swipes: a thread has 128 VGPRs and twice the
// independent work between barriers of a 1024 x 1 block; C3 0.315 -> 0.273
// ms, round 2):
//   * records are (bit offset in the slice PAIR: 20 bits) | swipe << 20,
//     one v_and_or per probe (pass B of the pair reads the offset as is);
//   * the sort places by the counting atomic's rank: a counter counts in 4s
//     from a bias of (its LDS word index) << 18, so an atomic's return value
//     >> 16 is its own byte offset in the counter array; after the scan the
//     counter holds 4 * start - bias, so a record's byte offset in the tile's
//     LDS record array is the atomic's return value plus that word: one shift
//     and one add per record.  The record and the rank of every probe (44
//     VGPRs) stay live across three barriers;
//   * from barrier 1 to the end of the copy-out a wave runs at priority 1
//     (round 7): the scan between barriers 1 and 3 is a few
//     dozen instructions per wave on which the block's other seven waves
//     wait, and at equal priority they queued behind the other block's
//     hashing.  0.428 -> 0.396 ms per sub-batch, 8.64-8.67 -> 8.38-8.47 ms
//     per 2^28 step; raised from barrier 3 on only, or to priority 3, it
//     changes nothing more;
//   * full tiles take a probe loop without the past-the-batch select;
//   * the two slices of a pair are counted apart but their runs are
//     adjacent with no gap (dense pair runs, round 4): pass B reads one word
//     per (pair, tile), off[pair][tile] = start | count << 16.  Runs padded
//     to 128-B lines made pass B read 12 % fewer lines but pass A write 21 %
//     more bytes, a net loss (A/B in DESIGN.md section 3);
//   * the counter scan's wave prefix is DPP (part_wave_scan) and a probe's
//     counter address is v_bfe + v_lshl_add (0.238 -> 0.222 ms, round 4).
// Counters of the two tile parities are one array (bias index par*kCnt + g);
// lanes past the batch count into the first pair past the chain (the sink),
// whose records land past the copy-out.  kCnt: 1024 (two counters per
// thread) for chains of < 512 pairs (C3/C5: 152), else 2048.
// The tile's four barriers and what each protects:
//   1  after the count: every probe of the tile is counted before the scan
//      reads the counters; a wave passes it only after its own copy-out
//      reads of the previous tile's srec have returned (lgkmcnt(0)), so with
//      barriers 2 and 3 behind it too no placement overwrites a record that a
//      copy-out has yet to read;
//   2  after the wave sums: swsum is complete before the block prefix, and
//      every thread has read its counts before barrier 3's writers;
//   3  after the scanned starts are written: placement reads only scanned
//      counters, and swsum / stot are read before the next tile
//      rewrites them (its barriers 1 and 2 come first);
//   4  after the placement: srec is complete before the copy-out reads it.
//      The other parity's counters are cleared between 3 and 4 -- their last
//      users, the placement reads of the tile before, ended before that
//      tile's barrier 4 -- so the next tile counts on clear counters right
//      after barrier 4 while this parity's scanned values are left alone
//      until the tile after next's clearing.
template <int KM, uint32_t kCnt>
__global__ void __launch_bounds__(512, 4) k_part_a3(const PartArgs A) {  // two blocks per CU
    constexpr uint32_t kT = 512;
    constexpr uint32_t kU = kPTile / kT;
    constexpr uint32_t kPer = kCnt / kT;  // counters per thread: kPer / 2 whole pairs
    constexpr uint32_t kRecWords = kPTile * KM;  // (the sink's records land past the copy-out)
    constexpr uint32_t kCo = (kRecWords / 4 + kT - 1) / kT;  // 16-B copy-out pieces per thread
    // the counter bias: counter c starts at c << kSB, so an atomic's return
    // value >> kRS (= kSB - 2) is its byte offset 4 c as long as 4 * rank
    // stays below bit kRS
    constexpr uint32_t kSB = 18, kRS = kSB - 2;
    static_assert(kCnt % (2 * kT) == 0 && kRecWords < 65536u && kPTile % kT == 0 && kPTile <= 2048,
                  "whole pairs per thread; starts fit 16 bits; a tile's swipes fit the 11-bit swipe field");
    static_assert(4u * kRecWords < (1u << kRS) && (2 * kCnt - 1) < (1u << (32 - kSB)),
                  "a rank * 4 below bit kRS; the bias of the last counter fits");
    // a counter's cleared value
    auto czero = [](uint32_t c) { return c << kSB; };
    // one LDS object, counters first: it sits at LDS address 0, so a probe's
    // counter address is its slice field shifted and added to the parity's
    // base (v_bfe + v_lshl_add: two VALU per probe)
    struct __attribute__((aligned(16))) Lds {
        uint32_t cnt[2 * kCnt];
        uint32_t srec[kRecWords];
        uint32_t swsum[kT / 64];
        uint32_t stot;
    };
    __shared__ Lds lds;
    uint32_t *const cnt = lds.cnt, *const srec = lds.srec, *const swsum = lds.swsum;
    uint32_t &stot = lds.stot;
    static_assert((kCnt & (kCnt - 1)) == 0, "parity base above the counter index bits");
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nunits = A.nunits;
    const uint32_t sink = 2 * nunits;  // the sink pair's first slice
    for (uint32_t c = tid; c < 2 * kCnt; c += kT) cnt[c] = czero(c);
    lds_barrier();
    // Every global load and store below is issued by every wave the same
    // number of times (buffer operations; a lane or a whole call with nothing
    // to move gives an offset past the range): vmcnt counts in issue order and
    // the compiler counts only what every path issues, so with a conditional
    // store between a load and its use the wait for the load also waited for
    // the stores (the copy-out's memory round trip, once per tile).
    const __amdgpu_buffer_rsrc_t roffs = part_rsrc(A.offs, A.offs ? (A.n + 1) * 4 : 0u);
    const __amdgpu_buffer_rsrc_t rhllw = part_rsrc(A.hllw, A.n * 4);
    const __amdgpu_buffer_rsrc_t roff = part_rsrc(A.off, nunits * A.off_stride * 4);
    auto offsets = [&](uint32_t t, uint32_t u, uint32_t &b, uint32_t &e) {
        const uint32_t i = t * kPTile + u * kT + tid;
        const uint32_t ic = i < A.n ? i : A.n - 1;
        // the swipe's two offsets in one 8-B load
        const uint2 lbe = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(roffs, ic * 4, 0, kNtAux<2>));
        b = A.offs ? lbe.x : ic * A.fixed_w;
        e = A.offs ? lbe.y : b + A.fixed_w;
    };
    uint32_t gt0, gt1;
    part_group(A.ntiles, blockIdx.x % kPGroups, gt0, gt1);
    const uint32_t tstep = gridDim.x / kPGroups;
    // this block's tiles: every tstep-th of its group's
    const uint32_t tfirst = gt0 + blockIdx.x / kPGroups;
    auto tnext = [&](uint32_t t) { return t + tstep; };
    const __amdgpu_buffer_rsrc_t rbytes = part_rsrc(A.bytes, 0xfffffff0u);
    const PartLink &L = A.link[0];
    uint32_t nb_[kU], ne_[kU];
    PartId it[kU];
    {
        // the first tile's ids, then the second tile's offsets (a tile's ids
        // load at the start of the tile before it, from offsets loaded one
        // tile earlier still)
        const uint32_t t = tfirst;
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) {
            offsets(t < gt1 ? t : gt0, u, nb_[u], ne_[u]);
            part_id_load(rbytes, nb_[u], ne_[u], it[u]);
        }
        const uint32_t t1 = t < gt1 && tnext(t) < gt1 ? tnext(t) : (t < gt1 ? t : gt0);
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) offsets(t1, u, nb_[u], ne_[u]);
    }
    const uint8_t *cntb = reinterpret_cast<const uint8_t *>(cnt);
    uint8_t *srecb = reinterpret_cast<uint8_t *>(srec);
    uint8_t *const cntw = reinterpret_cast<uint8_t *>(cnt);
    // a probe's slice (kCnt - 1 masks it: slices < kCnt), as one v_bfe the
    // compiler cannot fold into a shift and mask of the address
    auto part_slice = [](uint32_t x) {
        constexpr uint32_t kW = __builtin_ctz(kCnt);
        uint32_t r;
        asm("v_bfe_u32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "i"(kPSliceLog), "i"(kW));
        return r;
    };
    auto tile = [&](const uint32_t t, const uint32_t par) {
        const uint32_t cb = par * kCnt;
        const uint32_t pb = cb * 4;  // the parity's byte base, above (kCnt - 1) * 4
        uint32_t rv[kU][KM], rp[kU][KM];  // the probes' records and ranks
        const uint32_t tn = tnext(t) < gt1 ? tnext(t) : t;
        PartId itn[kU];
        // the next tile's ids (nb_ / ne_ hold its offsets), then the offsets
        // of the tile after it
        const uint32_t tn2 = tnext(tn) < gt1 ? tnext(tn) : tn;
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) part_id_load(rbytes, nb_[u], ne_[u], itn[u]);
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) offsets(tn2, u, nb_[u], ne_[u]);
        const bool full = (t + 1) * kPTile <= A.n;  // block-uniform
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) {
            const uint32_t lu = u * kT + tid;
            const uint32_t i = t * kPTile + lu;
            const bool act = i < A.n;
            uint64_t ha, hb, hh;
            part_hash3(A.bytes, it[u], ha, hb, hh);
            {
                uint32_t idx, rank;
                hll_patlen(hh, idx, rank);
                // (its top byte is the swipe's overflow flag, set by pass B)
                __builtin_amdgcn_raw_buffer_store_b32(idx | (rank << 16), rhllw, act ? i * 4 : kOOR, 0, kNtAux<8>);
            }
            const uint32_t lu20 = lu << 20;
            ProbeWalk32 wk;
            wk.init(ha, hb, part_div(L));
            if (full) {
#pragma unroll
                for (int q = 0; q < KM; q++) {
                    const uint32_t x = wk.x;
                    rv[u][q] = (x & 0xfffffu) | lu20;
                    rp[u][q] = atomicAdd(reinterpret_cast<uint32_t *>(cntw + part_slice(x) * 4 + pb), 4u);
                    if (q + 1 < KM) wk.step(L.d);
                }
            } else {
#pragma unroll
                for (int q = 0; q < KM; q++) {
                    const uint32_t x = wk.x;
                    rv[u][q] = (x & 0xfffffu) | lu20;
                    rp[u][q] =
                        atomicAdd(reinterpret_cast<uint32_t *>(cntw + (act ? part_slice(x) : sink) * 4 + pb), 4u);
                    if (q + 1 < KM) wk.step(L.d);
                }
            }
            // lgkmcnt(0): the atomics, once, after the last swipe only, so the
            // first one's atomics overlap the second one's hash
            if (u + 1 == kU) __builtin_amdgcn_s_waitcnt(0xc07f);
        }
        lds_barrier();  // 1
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) it[u] = itn[u];  // the next tile's ids
        // exclusive scan over pairs of their two slices' counts
        uint32_t v[kPer], s = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPer; j++) {
            const uint32_t c = cb + tid * kPer + j;
            v[j] = (cnt[c] - (c << kSB)) >> 2;
        }
#pragma unroll
        for (uint32_t j = 0; j < kPer; j += 2) s += v[j] + v[j + 1];
        const uint32_t incl = part_wave_scan(s);
        if (lane == 63) swsum[wave] = incl;
        lds_barrier();  // 2
        uint32_t run = incl - s;
        for (uint32_t w = 0; w < wave; w++) run += swsum[w];
#pragma unroll
        for (uint32_t j = 0; j < kPer; j += 2) {
            const uint32_t g = tid * kPer + j, c = cb + g, un = g / 2, n2 = v[j] + v[j + 1];
            // pass B's run: start | count << 16
            __builtin_amdgcn_raw_buffer_store_b32(run | (n2 << 16), roff, un < nunits ? (un * A.off_stride + t) * 4 : kOOR, 0, 0);
            if (g == sink) stot = run;
            // (the slice's start in bytes: where its first record goes)
            cnt[c] = 4 * run - czero(c);
            cnt[c + 1] = 4 * (run + v[j]) - czero(c + 1);
            run += n2;
        }
        lds_barrier();  // 3
#pragma unroll
        for (uint32_t u = 0; u < kU; u++) {
#pragma unroll
            for (int q = 0; q < KM; q++) {
                const uint32_t r = rp[u][q];
                *reinterpret_cast<uint32_t *>(srecb + (r + *reinterpret_cast<const uint32_t *>(cntb + (r >> kRS)))) =
                    rv[u][q];
            }
        }
        const uint32_t nb = (cb ^ kCnt);
        for (uint32_t g = tid; g <= sink + 1; g += kT) cnt[nb + g] = czero(nb + g);
        lds_barrier();  // 4
        const uint32_t total = stot;
        // a fixed number of 16-B pieces per thread (those past the tile's
        // total go out of range)
        const __amdgpu_buffer_rsrc_t rdst = part_rsrc(A.rec + size_t(t) * A.stride, A.stride * 4);
        // (a piece past the records reads the last piece instead: an LDS read
        // past srec would be undefined behaviour, from which the compiler may
        // infer a bound on tid for the rest of the kernel -- round 4 had one:
        // the unclamped index read past srec for the last pieces, and the
        // partitioned-K1 answers of some A/B builds were wrong; the
        // 2048-counter case of tests/test_k1_partitioned.py pins the fix)
        const part_u32x4 *src = reinterpret_cast<const part_u32x4 *>(srec);
        constexpr uint32_t kLast = kRecWords / 4 - 1;
        static_assert(kRecWords % 4 == 0 && kCo * kT >= kLast + 1, "the copy-out covers srec in 16-B pieces");
        static_assert([] {  // every piece index the copy-out reads is inside srec
            for (uint32_t c = 0; c < kCo; c++)
                for (uint32_t t = 0; t < kT; t++) {
                    const uint32_t j = c * kT + t;
                    if (((c + 1) * kT <= kLast + 1 ? j : (j < kLast ? j : kLast)) > kLast) return false;
                }
            return true;
        }(), "copy-out LDS index bound");
#pragma unroll
        for (uint32_t c = 0; c < kCo; c++) {
            const uint32_t j = c * kT + tid;
            const uint32_t jr = (c + 1) * kT <= kLast + 1 ? j : (j < kLast ? j : kLast);
            const uint32_t at = j * 16;
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned int, src[jr]),
                                                   rdst, j * 4 < total ? at : kOOR, 0, kNtAux<4>);
        }
        __builtin_amdgcn_s_setprio(0);
    };
    uint32_t par = 0;
    for (uint32_t t = tfirst; t < gt1; t = tnext(t), par ^= 1) tile(t, par);
}

// ---------------------------------------------------------------------------
// pass B: LDS-resident slices, probe their runs
// ---------------------------------------------------------------------------
// The (slice, tile) space is cut into gridDim.x equal contiguous ranges, slice
// major: a block probes one or two slices (restaging the LDS image once) over
// a range of tiles, so the resident grid is balanced to the tile and no block
// waits for a tail.
//
// Memory instructions are what this pass is made of (PMC: the address unit
// busy 84 % of the time, stalled behind L1 misses, when lanes read 4-byte
// pieces), so each one is made to move whole lines: within a slice (or slice
// pair) a wave takes kPbGroup consecutive tiles at a time, 8 lanes per tile
// run, and a lane loads 16 bytes (4 records) -- one instruction reads one
// whole 128-B line of each of 8 runs (pieces start at the line holding the
// run's first record).  2*SP such pieces cover a run of up to 64*SP records
// from its line (37 / 74 at C3 for single slices / pairs); longer runs finish
// in a tail loop.  The few failing
// probes (a member never fails; a non-member's probes fail about half the
// time) are compacted through LDS so a group ends in one fail-byte store
// instruction.  Loads and stores are buffer operations whose out-of-range
// lanes read 0 / are dropped, so every wave issues a fixed number per group
// and the pipeline keeps exact waits: the run boundaries of the group after
// next and the records of the next group are in flight while a group is
// tested.
constexpr uint32_t kPbQueue = 64;  // compacted fail stores per wave and group

// Fail lists (FL, one-link chains in slice pairs, 1024-swipe tiles): instead
// of one byte store per failing probe -- gfx950's L2 passes every store on to
// memory, so 8.8 M scattered byte stores per C3 step were 8.8 M partial-line
// fabric writes (WRITE_SIZE 251 MB for a 16 MB fail array, PMC r02) -- the
// failing swipes of each (slice unit, tile) go to a fixed list of kPbLanes
// u16 swipe indices, flist[unit][tile][], 0xffff = none.  A wave's round
// covers kPbGroup consecutive tiles of one unit, so its lists are one
// 128-byte span, written by one 2-byte-per-lane store instruction.  The
// failures past a list's kPbLanes entries (Poisson(3.7) at C3: ~2 % of the
// lists overflow) and those of the rare long runs keep the byte store; pass C
// (k_part_c_fl) folds the lists of a tile into LDS flags.
// Diagnostic block stamps of pass B (tools/stamps/run_pb_stamps.py; built only
// with -DSKE_STAMPS, the product library has none): thread 0 of every block
// records s_memrealtime (100 MHz) at entry and exit and the block's XCD into a
// side buffer no output depends on.
#ifdef SKE_STAMPS
__device__ unsigned long long *ske_pb_stamp_buf;
hipError_t set_pb_stamp_buffer(void *p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(ske_pb_stamp_buf), &p, sizeof(void *));
}
#define PB_STAMP(k)                                                                                    \
    do {                                                                                               \
        if ((k) == 1) __syncthreads();                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        unsigned long long t_;                                                                         \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        if (threadIdx.x == 0 && ske_pb_stamp_buf) {                                                    \
            ske_pb_stamp_buf[blockIdx.x * 4 + (k)] = t_;                                               \
            ske_pb_stamp_buf[blockIdx.x * 4 + 2] = __builtin_amdgcn_s_getreg((3 << 11) | 20);         \
        }                                                                                              \
    } while (0)
#else
#define PB_STAMP(k) \
    do {            \
    } while (0)
#endif
// The fail-list pass B's 8-lane prefix runs on DPP row shifts instead of three
// ds_bpermute rounds and a broadcast (0.1966 -> 0.1946 ms, round 3); the
// slice-pair image is copied as one batch of buffer loads (0.195 -> 0.190 ms).
// How pass B's blocks share the (slice unit, tile) space: XCD x (blocks b % 8
// == x) takes tile group x and its 32 blocks take units round robin, so
// adjacent units' runs, which share their boundary lines, are read by
// neighbouring CUs of one XCD at about the same time (round 4, A/B of three
// alternations on one box: 0.211 -> 0.200 ms; 128-B read requests 8.34 ->
// 8.06 M, L2 hits 0.65 -> 1.84 M per dispatch) -- while every block gets a
// whole unit (4 rounds of 32 of C3's 152); then the remaining units' (unit,
// 8-tile group) space in equal contiguous shares, so no block runs a fifth
// unit while the others wait (round 5: pass B 0.368 -> 0.362 ms per 2^25
// sub-batch, three alternations; profiles/r05_ab_pass_b_split.txt)
template <int SP, int R = 2 * SP, bool FL = false>  // R: 16-byte pieces per lane and run (runs of SP slices)
__global__ void __launch_bounds__(kPbBlock, SP == 1 ? 8 : 4) k_part_b(const PartArgs A) {
    PB_STAMP(0);
    const uint32_t tmask = kPTile - 1;
    __shared__ __attribute__((aligned(16))) uint8_t img[kPSliceBytes * SP];
    __shared__ uint32_t fq[kPbBlock / 64][kPbQueue];
    // this block's share of the (slice unit, tile) space: XCD x (blocks b % 8
    // == x) takes tile group x, and its blocks take whole units round robin
    // (block j: units j, j + 32, ...), so the 32 CUs of an XCD sweep the same
    // tiles of 32 ADJACENT units at about the same pace: a line two
    // neighbouring runs share is read while the other block's read of it is
    // still in the XCD's L2
    uint32_t gt0, gt1;
    part_group(A.ntiles, blockIdx.x % kPGroups, gt0, gt1);
    const uint32_t nblk = gridDim.x / kPGroups, bi = blockIdx.x / kPGroups;
    const uint32_t gn = gt1 - gt0;
    // (an empty XCD tile group -- a sub-batch of fewer than 64 tiles: the
    // whole block leaves before the split arithmetic divides by gn8 = 0)
    if (gn == 0) return;
    const uint32_t nunits = (A.nslices + SP - 1) / SP;
    const uint32_t total = nunits * gn;
    // block bi's equal share of a space of n items is [n * bi0 / nblk64,
    // n * bi1 / nblk64) in 64-bit products.  The operands are named here,
    // ahead of take_rest, on purpose: the compiler then forms them in the
    // entry block, as it did up to round 7 (a share initialiser of the removed
    // forms stood here), and every instantiation keeps that instruction
    // stream exactly (profiles/r08_refactor_ab.txt).  Folding them into
    // take_rest changes the scalar prologue; re-measure pass B if you do.
    const uint64_t bi0 = bi, nblk64 = nblk, bi1 = bi + 1;
    uint32_t w, wend;  // this block's current share of the space
    uint32_t su = bi;  // this block's current unit
    // units round robin while every block gets a whole one, then the
    // remaining units' (unit, 8-tile group) space in equal contiguous
    // shares, so no block waits with a fifth unit while others idle
    const uint32_t full = nunits / nblk * nblk;
    const uint32_t gn8 = (gn + 7) / 8;
    auto lin = [&](uint32_t c) {  // the remaining space's 8-tile group c as a (unit, tile) index
        const uint32_t t8 = (c % gn8) * 8;
        return (full + c / gn8) * gn + (t8 < gn ? t8 : gn);
    };
    bool rest = false;
    auto take_rest = [&]() {
        const uint32_t space = (nunits - full) * gn8;
        w = lin(uint32_t(space * bi0 / nblk64));
        wend = lin(uint32_t(space * bi1 / nblk64));
        rest = true;
    };
    w = su < full ? su * gn : total;
    wend = su < full ? w + gn : total;
    if (su >= full) take_rest();
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t k = lane / kPbLanes, qq = lane % kPbLanes;
    constexpr uint32_t kWaves = kPbBlock / 64, kStep = kWaves * kPbGroup;
    // the records of this block's tile group (offsets from its first tile,
    // so a 2^26-swipe sub-batch's 2.95 GB stay 32-bit)
    const size_t rbase = size_t(gt0) * A.stride;
    const __amdgpu_buffer_rsrc_t rrec = part_rsrc(A.rec + rbase, (gt1 - gt0) * A.stride * 4);
    const __amdgpu_buffer_rsrc_t roff = part_rsrc(A.off, (A.nslices + 1) * A.off_stride * 4);
    const __amdgpu_buffer_rsrc_t rfl = part_rsrc(A.flist, FL ? A.nunits * A.fl_stride * kPbLanes * 2 : 0);
    uint32_t *q = fq[wave];
    while (true) {
        if (w >= wend) {
            if (rest) break;
            su += nblk;  // block-uniform
            if (su < full) {
                w = su * gn;
                wend = w + gn;
            } else {
                take_rest();
                if (w >= wend) break;
            }
        }
        // slices g .. g + SP - 1 (SP = 2: one link only, host-checked), so
        // one run per tile covers them all
        const uint32_t unit = w / gn, g = unit * SP, ta = gt0 + w % gn;
        const uint32_t tb = gt1 - ta < wend - w ? gt1 : ta + (wend - w);
        const uint32_t ge = g + SP < A.nslices ? g + SP : A.nslices;
        w += tb - ta;
        uint32_t l = 0;
        while (l + 1 < A.nlinks && g >= A.link[l + 1].slice0) l++;
        const PartLink &L = A.link[l];
        const uint32_t b0 = (g - L.slice0) * kPSliceBytes;
        const uint32_t nb = L.nbytes16 - b0 < kPSliceBytes * SP ? L.nbytes16 - b0 : kPSliceBytes * SP;
        lds_barrier();  // every wave is done with the previous slice
        {
            // the pair image in one batch of fixed-count buffer loads (past nb
            // the range check returns zeros, which no record addresses): one
            // memory round trip per unit instead of one per 16 KiB piece
            constexpr uint32_t kCp = kPSliceBytes * SP / (kPbBlock * 16);
            static_assert(kCp * kPbBlock * 16 == kPSliceBytes * SP, "image pieces");
            const __amdgpu_buffer_rsrc_t rimg = part_rsrc(L.bf + b0, nb);
            uint4 piece[kCp];
#pragma unroll
            for (uint32_t c = 0; c < kCp; c++)
                piece[c] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         rimg, (c * kPbBlock + threadIdx.x) * 16, 0, 0));
#pragma unroll
            for (uint32_t c = 0; c < kCp; c++)
                *reinterpret_cast<uint4 *>(img + (c * kPbBlock + threadIdx.x) * 16) = piece[c];
        }
        lds_barrier();
        // failures that do not fit a fail list: a byte store of 1 (FL: into
        // the top byte of the swipe's HLL word -- byte 4 i + 3, which pass A
        // wrote 0 -- so pass A writes no fail bytes and C reads none)
        const __amdgpu_buffer_rsrc_t rfail =
            FL ? part_rsrc(A.hllw, A.n * 4) : part_rsrc(A.fail + size_t(l) * A.fail_stride, A.fail_stride);
        auto fail_at = [](uint32_t i) { return FL ? i * 4 + 3 : i; };
        const uint32_t orow = (FL ? unit : g) * A.off_stride, erow = ge * A.off_stride;
        // run boundaries of 8 rounds at once: lane L holds those of tile
        // tg0 + (L / 8) * kStep + L % 8 (0, 0 past tb); a round's lanes take
        // theirs from it with a cross-lane read, so boundary loads are one
        // instruction (FL: start | count << 16 per pair run) or one pair per
        // 8 rounds
        auto load_be8 = [&](uint32_t tg0, uint32_t &B, uint32_t &E) {
            const uint32_t t = tg0 + (lane / kPbGroup) * kStep + lane % kPbGroup;
            const bool in = t < tb;
            if constexpr (FL) {
                const uint32_t W = __builtin_amdgcn_raw_buffer_load_b32(roff, in ? (orow + t) * 4 : kOOR, 0, kNtAux<1>);
                B = W & 0xffffu;
                E = B + (W >> 16);
            } else {
                B = __builtin_amdgcn_raw_buffer_load_b32(roff, in ? (orow + t) * 4 : kOOR, 0, kNtAux<1>);
                E = __builtin_amdgcn_raw_buffer_load_b32(roff, in ? (erow + t) * 4 : kOOR, 0, kNtAux<1>);
            }
        };
        // 16-byte pieces qq, qq + 8, ... of the run from the 128-B line holding
        // its start: every piece is one whole line (one request, not two)
        // (one byte offset per lane; piece c adds 128 c, an immediate of the
        // load; a piece past the run's end goes out of range)
        // the word where tile t's run of this unit is placed from
        auto row = [&](uint32_t t) { return (t - gt0) * A.stride; };
        auto load_recs = [&](uint32_t tg, uint32_t b, uint32_t e, uint4 (&r)[R]) {
            const uint32_t i0 = (b & ~31u) + qq * 4;
            const uint32_t v0 = (row(tg + k) + i0) * 4;
            const int32_t left = int32_t(e) - int32_t(i0);
#pragma unroll
            for (uint32_t c = 0; c < R; c++)
                r[c] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(
                                                     rrec, (left > int32_t(32 * c) ? v0 : kOOR) + 128 * c, 0, kNtAux<64>));
        };
        uint32_t tg = ta + wave * kPbGroup;
        uint32_t Bc, Ec, Bn, En;  // boundaries of rounds [8q, 8q + 8) and of the 8 after
        load_be8(tg, Bc, Ec);
        load_be8(tg + kPbGroup * kStep, Bn, En);
        uint32_t bc = __shfl(Bc, k, 64), ec = __shfl(Ec, k, 64);
        // one round = kPbGroup tiles' runs of this unit; the next round's
        // records load while this one is tested.  Two rounds per loop
        // iteration with the record buffers in turn (no register copies).
        uint32_t rr = 0;
        auto round = [&](const uint4 (&r)[R], uint4 (&rn)[R]) {
            const uint32_t nr = (rr + 1) % kPbGroup;
            if (nr == 0) {  // wave-uniform
                Bc = Bn;
                Ec = En;
                load_be8(tg + (kPbGroup + 1) * kStep, Bn, En);
            }
            const uint32_t b1 = __shfl(Bc, nr * kPbGroup + k, 64), e1 = __shfl(Ec, nr * kPbGroup + k, 64);
            load_recs(tg + kStep, b1, e1, rn);
            // the (up to) 4R records of this lane: piece c starts at record
            // lo_c = s0 + c*32 + qq*4; bit j of vm: record j in [bc, ec)
            const uint32_t s0 = bc & ~31u;
            uint32_t rec[4 * R];
#pragma unroll
            for (uint32_t c = 0; c < R; c++) {
                rec[4 * c] = r[c].x;
                rec[4 * c + 1] = r[c].y;
                rec[4 * c + 2] = r[c].z;
                rec[4 * c + 3] = r[c].w;
            }
            // bit 4c + j: record lo0 + 32c + j lies in [bc, ec).  Only piece 0
            // can start before bc (s0 = bc & ~31), so the lower bound masks
            // piece 0 alone; the upper bound clamps every piece.
            // (v_bfm: ((1 << width) - 1) << offset in one VALU)
            auto clamp4 = [](int32_t v) { return uint32_t(v < 0 ? 0 : (v > 4 ? 4 : v)); };
            const uint32_t lo0 = s0 + qq * 4;
            const int32_t dh = int32_t(ec) - int32_t(lo0);
            uint32_t vm = 0;
#pragma unroll
            for (uint32_t c = 0; c < R; c++) vm |= part_bfm(clamp4(dh - int32_t(32 * c)), 4 * c);
            vm &= ~part_bfm(clamp4(int32_t(bc) - int32_t(lo0)), 0);
            // bit set in the image: its 32-bit word, bit (offset & 31); with
            // slice pairs the record's parity bit selects the image half
            const uint32_t *img32 = reinterpret_cast<const uint32_t *>(img);
            uint32_t okm = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4 * R; j++) {
                const uint32_t rr = rec[j];
                const uint32_t o = FL ? (rr & 0xfffffu)  // k_part_a3: the offset in the pair
                                      : SP == 1 ? (rr & kPSliceMask)
                                                : ((rr & kPSliceMask) | ((rr >> kPTileLog) & kPSliceBits));
                okm |= part_bit(img32[o >> 5], rr) << j;
            }
            uint32_t fm = vm & ~okm;
            const uint32_t tbase = (tg + k) << kPTileLog;
            const uint32_t cnt = __builtin_popcount(fm);
            // the record a lane's next failing probe sits in, by a select
            // tree on its index bits (no compare chain)
            auto pick = [&](uint32_t j) {
                constexpr uint32_t kNR = 4 * R, kL = kNR <= 8 ? 3 : (kNR <= 16 ? 4 : 5);
                uint32_t tt[1u << kL];
#pragma unroll
                for (uint32_t i = 0; i < (1u << kL); i++) tt[i] = rec[i < kNR ? i : 0];
#pragma unroll
                for (uint32_t l = 0; l < kL; l++) {
                    const bool bit = (j >> l) & 1u;
#pragma unroll
                    for (uint32_t i = 0; i < ((1u << kL) >> (l + 1)); i++) tt[i] = bit ? tt[2 * i + 1] : tt[2 * i];
                }
                return tt[0];
            };
            if constexpr (FL) {
                // this tile's failures (its kPbLanes lanes): positions by a
                // segment prefix; the first kPbLanes go to the tile's list
                uint32_t incl = cnt;
                // 8-lane segment prefix by DPP row shifts (VALU, no LDS round
                // trip); the list slots start as 0xffff and get the failures
                q[lane] = 0xffffu;
                __builtin_amdgcn_wave_barrier();
                {
                    uint32_t y = __builtin_amdgcn_update_dpp(0u, incl, 0x111, 0xf, 0xf, true);  // row_shr:1
                    incl += qq >= 1 ? y : 0u;
                    y = __builtin_amdgcn_update_dpp(0u, incl, 0x112, 0xf, 0xf, true);  // row_shr:2
                    incl += qq >= 2 ? y : 0u;
                    y = __builtin_amdgcn_update_dpp(0u, incl, 0x114, 0xf, 0xf, true);  // row_shr:4
                    incl += qq >= 4 ? y : 0u;
                }
                uint32_t pos = incl - cnt;
                while (fm) {
                    const uint32_t j = __builtin_ctz(fm);
                    fm &= fm - 1;
                    const uint32_t at = (pick(j) >> 20) & 0x7ffu;  // k_part_a3's swipe field
                    if (pos < kPbLanes) q[k * kPbLanes + pos] = at;
                    else __builtin_amdgcn_raw_buffer_store_b8(uint8_t(1), rfail, fail_at(tbase + at), 0, 0);  // overflow
                    pos++;
                }
                __builtin_amdgcn_wave_barrier();
                // lane (k, qq) writes entry qq of tile tg + k's list (tiles past
                // this block's range belong to another wave: not written)
                const uint32_t v = q[lane];
                const uint32_t fo = ((unit * A.fl_stride + tg + k) * kPbLanes + qq) * 2;
                __builtin_amdgcn_raw_buffer_store_b16(uint16_t(v), rfl, tg + k < tb ? fo : kOOR, 0, 0);
                __builtin_amdgcn_wave_barrier();
            } else {
                // compact the failing swipes of the wave: this lane's count, the
                // wave's exclusive prefix, one store instruction per 64 of them
                uint32_t incl = cnt;
#pragma unroll
                for (uint32_t o = 1; o < 64; o <<= 1) {
                    const uint32_t y = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += y;
                }
                const uint32_t nq = __shfl(incl, 63, 64);
                uint32_t pos = incl - cnt;
                while (fm) {
                    const uint32_t j = __builtin_ctz(fm);
                    fm &= fm - 1;
                    const uint32_t at = tbase + ((pick(j) >> kPSliceLog) & tmask);
                    if (pos < kPbQueue) q[pos] = at;
                    else __builtin_amdgcn_raw_buffer_store_b8(uint8_t(1), rfail, at, 0, 0);  // overflow
                    pos++;
                }
                __builtin_amdgcn_wave_barrier();
                if (nq) {
                    const uint32_t at = q[lane];
                    __builtin_amdgcn_raw_buffer_store_b8(uint8_t(1), rfail, lane < nq ? at : kOOR, 0, 0);
                }
                __builtin_amdgcn_wave_barrier();
            }
            if (ec - s0 > 32 * R) {  // rare: a long run
                const uint32_t base = row(tg + k);
                for (uint32_t i = s0 + 32 * R + qq; i < ec; i += kPbLanes) {
                    const uint32_t rr = __builtin_amdgcn_raw_buffer_load_b32(rrec, (base + i) * 4, 0, 0);
                    const uint32_t o = FL ? (rr & 0xfffffu)
                                          : SP == 1 ? (rr & kPSliceMask)
                                                    : ((rr & kPSliceMask) | ((rr >> kPTileLog) & kPSliceBits));
                    if (!((img[o >> 3] >> (o & 7)) & 1))
                        __builtin_amdgcn_raw_buffer_store_b8(uint8_t(1), rfail,
                                                             fail_at(tbase + (FL ? (rr >> 20) & 0x7ffu : (rr >> kPSliceLog) & tmask)), 0, 0);
                }
            }
            bc = b1;
            ec = e1;
            tg += kStep;
            rr++;
        };
        uint4 ra[R], rb[R];
        load_recs(tg, bc, ec, ra);
        while (tg < tb) {
            round(ra, rb);
            if (tg >= tb) break;  // wave-uniform
            round(rb, ra);
        }
    }
    PB_STAMP(1);
}

// ---------------------------------------------------------------------------
// pass C: answers and register max
// ---------------------------------------------------------------------------
template <int U>
__global__ void __launch_bounds__(kPcBlock) k_part_c(const PartArgs A) {
    const uint32_t T = kPcBlock, tid = threadIdx.x;
    uint32_t gt0, gt1;
    part_group(A.ntiles, blockIdx.x % kPGroups, gt0, gt1);
    const uint64_t tile = kPTile;
    const uint64_t end = uint64_t(gt1) * tile < A.n ? uint64_t(gt1) * tile : A.n;
    const uint64_t stride = uint64_t(gridDim.x / kPGroups) * T * U;
    for (uint64_t base = uint64_t(gt0) * tile + uint64_t(blockIdx.x / kPGroups) * T * U; base < end;
         base += stride) {
        bool valid[U];
        uint32_t *w[U];
        uint32_t rank[U], sh[U], cur[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t i = base + uint64_t(u) * T + tid;
            valid[u] = false;
            w[u] = nullptr;
            rank[u] = 0;
            sh[u] = 0;
            cur[u] = 0;
            if (i < end) {
                for (uint32_t l = 0; l < A.nlinks; l++) valid[u] |= nt_ld<16>(A.fail + size_t(l) * A.fail_stride + i) == 0;
                if (valid[u]) {
                    const uint32_t s = nt_ld<16>(A.slot + i);
                    if (s >= A.nslots) {
                        atomicOr(A.err, 1u);
                    } else {
                        const uint32_t hv = nt_ld<16>(A.hllw + i);
                        const uint32_t ridx = hv & 0xffffu;
                        w[u] = reinterpret_cast<uint32_t *>(A.regs + (uint64_t(s) << kHllP) + (ridx & ~3u));
                        sh[u] = (ridx & 3) * 8;
                        rank[u] = hv >> 16;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) cur[u] = w[u] ? nt_ld<32>(w[u]) : 0xffffffffu;
#pragma unroll
        for (int u = 0; u < U; u++)
            if (w[u]) part_reg_max(w[u], sh[u], rank[u], cur[u]);
        if (A.out) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint64_t i = base + uint64_t(u) * T + tid;
                if (i < end) nt_st<16>(A.out + i, uint8_t(valid[u]));
            }
        }
    }
}

// Pass C over pass B's fail lists (one-link chains, 1024-swipe tiles): a
// block takes runs of kPbGroup consecutive tiles of its XCD group (the span
// one pass-B round writes, so a unit's lists for the run are one 128-byte
// line, loaded by 8 lanes together), marks the listed swipes in LDS, and
// after one barrier runs k_part_c's per-swipe answer and register max over
// the run's tiles -- the next tile's fail bytes (list overflows), slots and
// HLL words in flight while a tile's CASes are, every CAS of a tile issued
// before any is settled.  Marks carry the run's index: nothing is cleared.
// (Its loads and stores at a fixed count per tile, as pass A's, measured
// equal, 0.408 vs 0.409 ms: pass C is bound by the memory side's random
// requests, not by its waves' waits.)
// (A two-phase form -- the answers and the rank-1 raises as plain byte
// stores first, the rank >= 2 raises by CAS in a second kernel -- measured
// slower, 0.409 -> 0.436 ms, round 4: the line traffic, not the CAS count,
// holds this pass.)  U swipes per thread per tile, kPcFlBlock * U = 1024
// (1024 x 1 since round 4; see kPcFlT).
template <uint32_t BT, int U>
__global__ void __launch_bounds__(BT) k_part_c_fl(const PartArgs A) {
    constexpr uint32_t TILE = kPTile;
    static_assert(BT * U == TILE, "one tile per sub-step");
    constexpr uint32_t kPcFlBlock = BT;
    constexpr uint32_t kRun = kPbGroup;  // tiles per block iteration
    __shared__ uint16_t mark[kRun * TILE];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < kRun * TILE; j += kPcFlBlock) mark[j] = 0;
    uint32_t gt0, gt1;
    part_group(A.ntiles, blockIdx.x % kPGroups, gt0, gt1);
    const uint32_t nblk = gridDim.x / kPGroups;
    const uint32_t npieces = A.nunits * kRun;  // 16-B lists of one run
    const __amdgpu_buffer_rsrc_t rfl = part_rsrc(A.flist, A.nunits * A.fl_stride * kPbLanes * 2);
    struct In {
        uint32_t fb[U], sl[U], hv[U];
    };
    auto load = [&](uint32_t t, uint32_t tend, In &in) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t i = t * TILE + uint32_t(u) * kPcFlBlock + tid;
            const bool act = t < tend && i < A.n;
            in.sl[u] = act ? nt_ld<16>(A.slot + i) : 0u;
            in.hv[u] = act ? nt_ld<16>(A.hllw + i) : 0xff000000u;  // (top byte: pass B's overflow flag)
            in.fb[u] = in.hv[u] >> 24;
        }
    };
    lds_barrier();
    for (uint32_t r0 = gt0 + (blockIdx.x / kPGroups) * kRun; r0 < gt1; r0 += nblk * kRun) {
        const uint32_t r1 = r0 + kRun < gt1 ? r0 + kRun : gt1;
        const uint16_t ep = uint16_t(r0 / kRun + 1);  // < 2^16: sub-batches hold <= 16384 tiles
        In cur;
        load(r0, r1, cur);
        // the run's lists: piece p = (unit p / kRun, tile r0 + p % kRun)
        for (uint32_t p0 = 0; p0 < npieces; p0 += 4 * kPcFlBlock) {
            part_u32x4 e[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t p = p0 + uint32_t(j) * kPcFlBlock + tid;
                const uint32_t un = p / kRun, tt = r0 + p % kRun;
                ok[j] = p < npieces && tt < r1;
                e[j] = __builtin_bit_cast(part_u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         rfl, ok[j] ? (un * A.fl_stride + tt) * kPbLanes * 2 : kOOR, 0, 0));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t base = ((p0 + uint32_t(j) * kPcFlBlock + tid) % kRun) * TILE;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lo = e[j][c] & 0xffffu, hi = e[j][c] >> 16;
                    if (ok[j] && lo < TILE) mark[base + lo] = ep;  // (0xffff: no entry)
                    if (ok[j] && hi < TILE) mark[base + hi] = ep;
                }
            }
        }
        lds_barrier();
        for (uint32_t t = r0; t < r1; t++) {
            In nxt;
            load(t + 1, r1, nxt);
            const uint16_t *mk = mark + (t - r0) * TILE;
            bool valid[U];
            uint32_t *w[U];
            uint32_t rank[U], sh[U], cw[U], seen[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t i = t * TILE + uint32_t(u) * kPcFlBlock + tid;
                valid[u] = i < A.n && cur.fb[u] == 0 && mk[uint32_t(u) * kPcFlBlock + tid] != ep;
                w[u] = nullptr;
                rank[u] = sh[u] = 0;
                if (valid[u]) {
                    const uint32_t rk = (cur.hv[u] >> 16) & 0xffu;
                    if (cur.sl[u] >= A.nslots) {
                        atomicOr(A.err, 1u);
                    } else {
                        const uint32_t ridx = cur.hv[u] & 0xffffu;
                        w[u] = reinterpret_cast<uint32_t *>(A.regs + (uint64_t(cur.sl[u]) << kHllP) + (ridx & ~3u));
                        sh[u] = (ridx & 3) * 8;
                        rank[u] = rk;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) cw[u] = w[u] ? nt_ld<32>(w[u]) : 0xffffffffu;
            // every raising CAS of the tile in flight at once, then settled
            // (a lost race retries from the word the CAS returned)
#pragma unroll
            for (int u = 0; u < U; u++) {
                seen[u] = cw[u];
                if (w[u] && ((cw[u] >> sh[u]) & 0xffu) < rank[u])
                    seen[u] = atomicCAS(w[u], cw[u], (cw[u] & ~(0xffu << sh[u])) | (rank[u] << sh[u]));
            }
            if (A.out) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t i = t * TILE + uint32_t(u) * kPcFlBlock + tid;
                    if (i < A.n) nt_st<16>(A.out + i, uint8_t(valid[u]));
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++)
                if (w[u] && seen[u] != cw[u]) part_reg_max(w[u], sh[u], rank[u], seen[u]);
            cur = nxt;
        }
        lds_barrier();  // the marks are rewritten by the next run
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// probes per swipe an instantiation of pass A holds: 11 (C3/C5's k = 11
// filter; two blocks per CU) or 22; 0: the chain is not supported
static uint32_t part_km(uint32_t ksum) {
    if (ksum == 0) return 0;
    if (ksum <= 11) return 11;
    if (ksum <= 22) return 22;
    return 0;
}

// records per tile, rounded so tiles start on 128-B lines
static uint32_t part_stride(uint32_t ksum, uint32_t tile) { return ((ksum * tile) + 31) & ~31u; }

static bool part_plan(const ChainDev &ch, PartArgs *A) {
    if (ch.nlinks < 1 || ch.nlinks > kPMaxLinks) return false;
    uint32_t slices = 0, ksum = 0;
    for (int l = 0; l < ch.nlinks; l++) {
        const LinkDev &L = ch.link[l];
        if (L.div.d > (uint64_t(1) << 31) || L.div.d < 64 || L.k == 0 || L.k > 64) return false;
        PartLink &P = A->link[l];
        P.bf = L.bf;
        P.m = L.div.m;
        P.d = uint32_t(L.div.d);
        P.t = uint32_t(L.div.t);
        P.sh = L.div.sh;
        P.k = L.k;
        P.slice0 = slices;
        P.nbytes16 = uint32_t((((L.div.d >> 3) + 15) >> 4) << 4);
        slices += uint32_t((L.div.d + kPSliceBits - 1) / kPSliceBits);
        ksum += L.k;
    }
    if (slices > kPMaxSlices || part_km(ksum) == 0) return false;
    A->nlinks = uint32_t(ch.nlinks);
    A->nslices = slices;
    A->ksum = ksum;
    A->nunits = (slices + 1) / 2;
    A->stride = part_stride(ksum, kPTile);
    return true;
}

bool part_supported(const ChainDev &ch) {
    PartArgs A{};
    return part_plan(ch, &A);
}

// the scratch of a sub-batch of up to `sub` swipes (context scratch slots
// kScrPart*: probe records, run boundaries, fail bytes, HLL words, and the
// fail lists of one-link chains)
static hipError_t part_scratch(PartArgs *A, uint64_t n, uint32_t sub, Scratch *scr) {
    const uint32_t m = n < sub ? uint32_t(n) : sub;
    const uint32_t tile = kPTile;
    const uint32_t ntiles_max = (m + tile - 1) / tile;
    const uint32_t fstride = (m + 255) & ~255u;
    A->off_stride = (ntiles_max + 15) & ~15u;
    hipError_t e = hipSuccess;
    A->rec = (uint32_t *)scratch_get(scr, kScrPartRec, size_t(ntiles_max) * A->stride * 4, &e);
    if (e == hipSuccess) A->off = (uint32_t *)scratch_get(scr, kScrPartOff, size_t(A->off_stride) * (A->nslices + 1) * 4, &e);
    // (fail bytes: the fail-list chains keep their overflow flags in the HLL words)
    A->fail = nullptr;
    if (e == hipSuccess && !part_flist(*A))
        A->fail = (uint8_t *)scratch_get(scr, kScrPartFail, size_t(fstride) * A->nlinks, &e);
    if (e == hipSuccess) A->hllw = (uint32_t *)scratch_get(scr, kScrPartHllw, size_t(m) * 4, &e);
    A->fail_stride = fstride;
    A->fl_stride = A->off_stride;
    A->flist = nullptr;
    if (e == hipSuccess && A->nlinks == 1)
        A->flist = (uint16_t *)scratch_get(scr, kScrPartFlist, size_t(A->nunits) * A->fl_stride * kPbLanes * 2, &e);
    return e;
}

// swipes per sub-batch: the option (at most the largest, kPSub, whose probe
// records of one XCD tile group stay within a 2^31-byte buffer range --
// k_part_b's rsrc, relative to the group's first tile -- 2^26 for every chain the plan takes), or kPSubDefault: 2^25
// measured as fast as 2^26 at C3 and faster than 2^24 (profiles/r05_ab_subbatch.txt)
constexpr uint32_t kPSubDefault = 1u << 25;
static uint32_t part_sub(uint32_t sub_opt, const PartArgs &A) {
    const uint64_t tiles = ((uint64_t(1) << 31) - 1) / (uint64_t(A.stride) * 4);
    const uint64_t span = (tiles - 8) * kPGroups;  // tiles a sub-batch may have
    const uint32_t tile = kPTile;
    const uint32_t cap = uint32_t(std::min<uint64_t>(kPSub / tile * tile, span / 8 * 8 * tile));
    uint32_t sub = sub_opt ? sub_opt : std::min(cap, kPSubDefault);
    sub = (sub + tile - 1) / tile * tile;
    return sub < tile ? tile : (sub > cap ? cap : sub);
}

// the scratch before the first launch (so a graph recorded later holds it)
hipError_t part_reserve(const ChainDev &ch, uint64_t n, uint32_t sub_opt, uint32_t nslots, const SegOpts &so,
                        Scratch *scr) {
    PartArgs A{};
    if (!part_plan(ch, &A)) return hipErrorInvalidValue;
    const uint32_t sub = part_sub(sub_opt, A);
    hipError_t e = part_scratch(&A, n ? n : 1, sub, scr);
    SegPlan P;
    if (e == hipSuccess && seg_use(A, so, nslots, n ? n : 1, sub, &P)) {
        SegArgs S{};
        e = seg_scratch(P, sub, n, scr, &S);
        // scratch that cannot grow under a recorded graph: such a batch takes
        // pass C instead (launch_swipes_part decides the same way)
        if (e == hipErrorStreamCaptureUnsupported) e = hipSuccess;
    }
    return e;
}

// Units = (batch, sub-batch of at most `sub` swipes), in order, each as the
// three passes on `st`.  `hook` (pass timing) brackets every kernel.
hipError_t launch_swipes_part(const ChainDev &ch, const PartBatch *bt, uint32_t nb, uint8_t *regs,
                              uint32_t nslots, Scratch *scr, unsigned int *err, int cus, uint32_t sub_opt,
                              const SegOpts &so, hipStream_t st, PassHook hook, void *hook_user) {
    PartArgs A{};
    if (!part_plan(ch, &A)) return hipErrorInvalidValue;
    const uint32_t sub = part_sub(sub_opt, A);
    uint64_t nmax = 0;
    for (uint32_t j = 0; j < nb; j++) nmax = bt[j].n > nmax ? bt[j].n : nmax;
    if (nmax == 0) return hipSuccess;
    hipError_t e = part_scratch(&A, nmax, sub, scr);
    if (e != hipSuccess) return e;
    const uint32_t tile = kPTile;
    A.regs = regs;
    A.nslots = nslots;
    A.err = err;
    const uint32_t km = part_km(A.ksum);
    // one link of k = 11 (C3/C5): slice pairs and fail lists
    const bool flist = part_flist(A) && A.flist != nullptr;
    const bool pairs = A.nlinks == 1;  // a one-link chain is probed in slice pairs (128 KiB images)
    const unsigned ga = unsigned(cus) * (km <= 11 ? 2u : 1u) / kPGroups * kPGroups;  // blocks past a group's tiles exit
    const unsigned ga3 = unsigned(cus) * 2 / kPGroups * kPGroups;  // k_part_a3: the resident set, two blocks per CU
    const unsigned gb = unsigned(cus) * (pairs ? 1 : 2) / kPGroups * kPGroups;  // all resident
    for (uint32_t j = 0; j < nb; j++) {
        const PartBatch &B = bt[j];
        // fixed-width ids: a sub-batch's byte offsets (swipe * width) stay 32-bit
        uint32_t subj = sub;
        if (!B.offs && B.fixed_w) {
            const uint64_t cap = (0xffffff00ull / B.fixed_w) / tile * tile;
            subj = cap < sub ? uint32_t(cap < tile ? tile : cap) : sub;
        }
        // sub-batches of even size (a 17.6 M batch as 2 x 8.8 M, not 16 M +
        // 1.6 M: a small last sub-batch cannot fill the chip)
        if (B.n > subj) {
            const uint64_t ns = (B.n + subj - 1) / subj;
            subj = uint32_t(((B.n + ns - 1) / ns + tile - 1) / tile * tile);
        }
        // the segmented PFADD (k_seg_*) for this batch, or pass C per sub-batch
        SegPlan P;
        SegArgs S{};
        bool seg = flist && seg_use(A, so, nslots, B.n, subj, &P);
        if (seg) {
            e = seg_scratch(P, subj, B.n, scr, &S);
            // (recording a graph with scratch too small for this batch's
            // segmented PFADD: the batch takes pass C, same answers and registers)
            if (e == hipErrorStreamCaptureUnsupported) {
                seg = false;
                e = hipSuccess;
            }
            if (e != hipSuccess) return e;
        }
        uint32_t si = 0;
        for (uint64_t s0 = 0; s0 < B.n; s0 += subj, si++) {
            const uint32_t ms = B.n - s0 < subj ? uint32_t(B.n - s0) : subj;
            A.fixed_w = B.fixed_w;
            A.n = ms;
            A.ntiles = (ms + tile - 1) / tile;
            A.bytes = B.offs ? B.bytes : B.bytes + s0 * B.fixed_w;
            A.offs = B.offs ? B.offs + s0 : nullptr;
            A.slot = B.slot + s0;
            A.out = B.out ? B.out + s0 : nullptr;
            if (hook) hook(hook_user, 0, 0, st);
            if (flist && A.nunits < 512)  // C3/C5: 152 pairs, two counters per thread
                hipLaunchKernelGGL((k_part_a3<11, 1024>), dim3(ga3), dim3(512), 0, st, A);
            else if (flist)
                hipLaunchKernelGGL((k_part_a3<11, 2048>), dim3(ga3), dim3(512), 0, st, A);
            else if (km <= 11)
                hipLaunchKernelGGL(k_part_a<11>, dim3(ga), dim3(kPaBlock), 0, st, A);
            else
                hipLaunchKernelGGL(k_part_a<22>, dim3(ga), dim3(kPaBlock), 0, st, A);
            if (hook) hook(hook_user, 0, 1, st);
            if (hook) hook(hook_user, 1, 0, st);
            if (flist)
                // (4 pieces per lane: a (pair, tile) run of ~74 records from the
                // line holding its start)
                hipLaunchKernelGGL((k_part_b<2, 4, true>), dim3(gb), dim3(kPbBlock), 0, st, A);
            else if (pairs)
                hipLaunchKernelGGL(k_part_b<2>, dim3(gb), dim3(kPbBlock), 0, st, A);
            else
                hipLaunchKernelGGL(k_part_b<1>, dim3(gb), dim3(kPbBlock), 0, st, A);
            if (hook) hook(hook_user, 1, 1, st);
            if (seg) {  // C1 + D
                e = launch_seg_sub(A, S, P, si, cus, st, hook, hook_user);
                if (e != hipSuccess) return e;
                // every window of the slab once after each group of P.nsub
                // sub-batches (the whole batch unless it is very large)
                if ((si + 1) % P.nsub == 0 || s0 + subj >= B.n) {
                    e = launch_seg_windows(A, S, P, si % P.nsub + 1, cus, st, hook, hook_user);
                    if (e != hipSuccess) return e;
                }
                continue;
            }
            if (hook) hook(hook_user, 2, 0, st);
            if (flist) {
                const unsigned gc =
                    (grid_for(ms, kPTile * kPbGroup, unsigned(cus) * kPcFlBlocksPerCu) + kPGroups - 1) /
                    kPGroups * kPGroups;
                hipLaunchKernelGGL((k_part_c_fl<kPcFlT, kPTile / kPcFlT>), dim3(gc), dim3(kPcFlT), 0, st, A);
            } else {
                const unsigned gc = (grid_for(ms, kPcBlock * 2, unsigned(cus) * 8) + kPGroups - 1) / kPGroups * kPGroups;
                hipLaunchKernelGGL(k_part_c<2>, dim3(gc), dim3(kPcBlock), 0, st, A);
            }
            if (hook) hook(hook_user, 2, 1, st);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

}  // namespace ske
