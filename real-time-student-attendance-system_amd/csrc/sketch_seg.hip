// sketch_seg.hip -- the segmented PFADD (north_star's HLL kernel form), its
// kernels C1, D, E, M and their host side: pass C of the one-link
// partitioned K1 (sketch_part.hip's launch_swipes_part launches it) when the
// call's register updates are dense in the slab -- the batch is segmented by
// key, each key window's registers are staged in LDS, raised there, and
// flushed to HBM as whole lines.  Same result as
// k_part_c_fl (hllAdd's register max, attendance_processor.py:127-129; max is
// commutative, so the order of updates is free).
//
// Why.  k_part_c_fl costs one random 128-B line read per valid swipe (its
// register's pre-check) plus one memory-side CAS per raise: 14.4 M + 7 M
// random requests per 16 M-swipe C3 step.  When a call's updates are dense
// in the slab -- an 8-way shard (12.5 k keys, 205 MB, ~9 updates per 128-B
// line per 16 M swipes) or a large batch -- reading every line of the slab
// once and writing back the lines that rose costs fewer bytes than the
// random requests, and no atomics reach memory.
//
//   C1 (k_seg_c1)   per run of 8 tiles (8192 swipes; pass B's fail lists of a
//                   run are one line per unit): the answers as k_part_c_fl,
//                   and for each valid swipe one 4-byte record
//                   (slot-in-bucket << 20 | register << 6 | rank),
//                   counting-sorted in LDS by level-1 bucket (slot >> s1,
//                   <= 512 buckets); each bucket's records of the run
//                   reserved in the bucket's contiguous sequence of the
//                   sub-batch (one atomic add) and stored into its
//                   8192-record chunk slots (the arena).
//   D  (k_seg_da)   per chunk: its records, read whole, counting-sorted in
//                   LDS by window (2^klog keys) within the bucket;
//                   o2[chunk][window] = the window's start.
//   E  (k_seg_e)    per window, once per call (after every sub-batch's C1
//                   and D): its records' runs over every chunk of its bucket;
//                   with at least dense_min records the window's registers
//                   (2^klog x 16 KiB) are loaded into LDS in whole lines,
//                   raised there (LDS CAS; registers only grow), and the
//                   lines that rose are stored back; a sparse window raises
//                   its records in place (pre-check load + CAS, as pass C).
//   F  (k_seg_floor) per window-pass group, before its first C1: the byte
//                   minimum (floor) of every hinted key's registers, from the
//                   slab as it stands; D drops the records at or under their
//                   key's floor, which can raise nothing (see k_seg_floor).
//                   Measured at the 2^28 default step against the build
//                   without it (profiles/r21_ab_seg_floor.txt): step 8.40-8.44
//                   -> 8.13-8.15 ms, E 1.05 -> 0.82, D 0.059 -> 0.053 per
//                   sub-batch, the floor pass +0.03 ms per step, 50.4 % of the
//                   timed steps' records dropped.
//                   Measured and removed: the same test in C1 before its
//                   store (a 1-byte gather from the floor table per valid
//                   swipe; 84 VGPRs' worth in an 80-VGPR kernel, 4 spilled):
//                   C1 0.111 -> 0.148 ms per sub-batch against D 0.053 ->
//                   0.036 and E 0.81 -> 0.76, step 8.08-8.13 -> 8.21-8.23 ms,
//                   same registers (three alternations, same file).
#include <algorithm>
#include <type_traits>

#include "sketch_part.h"
#include "sketch_seg_plan.h"

namespace ske {

// Exclusive prefix of one value per thread over the block (blockDim a
// multiple of 64); every thread also gets the total.  `ws`: blockDim / 64
// words of LDS.  LDS-only barriers (global loads and stores stay in flight).
__device__ __forceinline__ uint32_t seg_scan(uint32_t v, uint32_t *ws, uint32_t &total) {
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const uint32_t inc = part_wave_scan(v);
    lds_barrier();  // the previous scan's readers of ws are done
    if (lane == 63) ws[wave] = inc;
    lds_barrier();
    uint32_t pre = 0, tot = 0;
    for (uint32_t w = 0; w < nw; w++) {
        const uint32_t x = ws[w];
        pre += w < wave ? x : 0;
        tot += x;
    }
    total = tot;
    return pre + inc - v;
}

// index of the last entry of a[0..n) that is <= v (a ascending, a[0] <= v)
__device__ __forceinline__ uint32_t seg_last_le(const uint32_t *a, uint32_t n, uint32_t v) {
    uint32_t lo = 0, len = n;
    while (len > 1) {
        const uint32_t half = len >> 1;
        if (a[lo + half] <= v) lo += half;
        len -= half;
    }
    return lo;
}

// The arena of C1 -> D.  C1 reserves each bucket's records of a run with one
// atomic add on the bucket's fill count (issued before the run's scan and
// placement, which hide its latency), so a bucket's records are one
// contiguous sequence of the sub-batch; the sequence lives in 8 192-record
// chunks.  The first kstat chunks of bucket h have the fixed slots
// h * kstat + c of r1 (about twice a bucket's mean); a later
// chunk of a heavy bucket takes a slot from a counter, claimed by the run
// whose reservation holds the chunk's first record, which publishes it in
// ctab before it waits for any other.  D then reads whole chunks: no scan
// pass S, no run tables, no gather.
// Measured at the 2^28 default step against round 6's run-table form
// (profiles/r06_ab_seg_arena.txt): C1 + D 0.195 -> 0.169 ms per 2^25
// sub-batch at N = 1 (C1 0.100 -> 0.110, S + D 0.095 -> 0.059), 0.193 ->
// 0.172 at the 8-way shard; step 8.87 -> 8.63 ms.
//
// Arena: the slots of the (at most two) chunks that bucket h's cv records
// of a run, from sequence index base on, fall in, packed as slot0 | slot1 <<
// 14 | (chunk0 & 1) << 28.  A fixed chunk (c < kstat) needs nothing; a
// counted chunk whose first record is in this reservation takes its slot
// here and publishes it; one begun by an earlier reservation is waited for
// (its owner took its fill index before this one did, so it is resident and
// publishes without waiting on anything).  A wait that never ends sets error
// bit 4 (reported as the call's error) after ~1 s.
static_assert(kSegChunk == 8192, "the arena's chunk arithmetic");
static_assert(kSegRunSw <= kSegChunk, "the arena: a run's records of one bucket span at most two chunks");
// fill counts 256 B apart: every run adds to every bucket's, and counters
// packed in a few lines would queue on the few memory channels holding them
constexpr uint32_t kSegFillStride = 64;
__device__ __forceinline__ uint32_t seg_fill_at(const SegArgs &S, uint32_t h) {
    return (S.s * (S.nb1 + 1) + h) * kSegFillStride;
}
__device__ __forceinline__ uint32_t seg_arena_slot(const SegArgs &S, unsigned int *err, uint32_t h, uint32_t c,
                                                   bool own) {
    if (c < S.kstat) return h * S.kstat + c;
    uint32_t *ct = S.ctab + size_t(h) * S.kmaxc + c;
    if (own) {
        const uint32_t d = atomicAdd(S.fill + seg_fill_at(S, S.nb1), 1u);
        __hip_atomic_store(ct, d + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return S.nb1 * S.kstat + d;
    }
    uint32_t v = 0;
    for (uint32_t it = 0; it < (1u << 22); it++) {
        v = __hip_atomic_load(ct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v) break;
        __builtin_amdgcn_s_sleep(8);
    }
    if (!v) {
        atomicOr(err, 4u);
        v = 1;
    }
    return S.nb1 * S.kstat + v - 1;
}
__device__ __forceinline__ uint32_t seg_arena_slots(const SegArgs &S, unsigned int *err, uint32_t h, uint32_t cv,
                                                    uint32_t base) {
    const uint32_t c0 = base >> 13, c1 = (base + cv - 1) >> 13;  // cv <= 8192: c1 <= c0 + 1
    // (chunk c1 > c0 starts inside this reservation: it is ours, published
    // before we wait for c0)
    const uint32_t s1 = c1 != c0 ? seg_arena_slot(S, err, h, c1, true) : 0u;
    __asm__ volatile("" ::: "memory");
    const uint32_t s0 = seg_arena_slot(S, err, h, c0, (base & (kSegChunk - 1)) == 0);
    return s0 | ((c1 != c0 ? s1 : s0) << 14) | ((c0 & 1u) << 28);
}

// C1's block: T threads, U = kSegRunSw / T swipes of a run each: 512 x 16 at
// three blocks per CU, three runs in flight per CU
constexpr uint32_t kSegC1T = 512;
template <uint32_t T> struct SegC1 {
    static constexpr uint32_t U = kSegRunSw / T;  // swipes per thread per run
    static constexpr uint32_t PT = kPTile / T;   // swipes per thread per tile
    static constexpr uint32_t BPC = 3;            // blocks per CU
    static constexpr uint32_t WPE = BPC * (T / 64) / 4;
    static_assert(T == 512, "three blocks per CU");
    static_assert(kPTile % T == 0, "whole tile slices per thread");
};
template <uint32_t T>
__global__ void __launch_bounds__(T, SegC1<T>::WPE) k_seg_c1(const PartArgs A, const SegArgs S) {
    constexpr uint32_t U = SegC1<T>::U, PT = SegC1<T>::PT;
    __shared__ __attribute__((aligned(16))) uint16_t mark[kSegRunSw];
    __shared__ __attribute__((aligned(16))) uint32_t srec[kSegRunSw];
    __shared__ uint32_t cnt[kSegMaxB1 + 1];
    __shared__ uint32_t slt[kSegMaxB1];
    __shared__ uint32_t ws[T / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t j = tid; j < kSegRunSw; j += T) mark[j] = 0;
    const uint32_t npieces = A.nunits * kSegRunTiles;  // 16-B lists of one run
    const __amdgpu_buffer_rsrc_t rfl = part_rsrc(A.flist, A.nunits * A.fl_stride * kPbLanes * 2);
    const uint32_t kmask = (1u << S.klog) - 1, bmask = S.nb1 - 1;
    lds_barrier();  // marks cleared before any run sets one
    for (uint32_t r = blockIdx.x; r < S.nruns; r += gridDim.x) {
        const uint32_t t0 = r * kSegRunTiles;
        const uint32_t t1 = t0 + kSegRunTiles < A.ntiles ? t0 + kSegRunTiles : A.ntiles;
        const uint16_t ep = uint16_t(r + 1);  // <= kSegMaxRuns (8192) < 2^16: marks are never cleared
        // the run's streams, every tile's in flight together (the HLL
        // word's top byte is pass B's overflow flag)
        uint32_t sl[U], hv[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {  // swipe u: tile u / PT, its (u % PT)-th T-thread slice
            const uint32_t i = (t0 + u / PT) * kPTile + (u % PT) * T + tid;
            const bool act = t0 + u / PT < t1 && i < A.n;
            sl[u] = act ? nt_ld<16>(A.slot + i) : 0u;
            hv[u] = act ? nt_ld<16>(A.hllw + i) : 0xff000000u;
        }
        for (uint32_t j = tid; j <= S.nb1; j += T) cnt[j] = 0;
        // the run's fail lists -> marks (piece p = unit p / 8, tile t0 + p % 8)
        for (uint32_t p0 = 0; p0 < npieces; p0 += 4 * T) {
            part_u32x4 e[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t p = p0 + uint32_t(j) * T + tid;
                const uint32_t un = p / kSegRunTiles, tt = t0 + p % kSegRunTiles;
                ok[j] = p < npieces && tt < t1;
                e[j] = __builtin_bit_cast(part_u32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                         rfl, ok[j] ? (un * A.fl_stride + tt) * kPbLanes * 2 : kOOR, 0, 0));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const uint32_t base = ((p0 + uint32_t(j) * T + tid) % kSegRunTiles) * kPTile;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const uint32_t lo = e[j][c] & 0xffffu, hi = e[j][c] >> 16;
                    if (ok[j] && lo < kPTile) mark[base + lo] = ep;  // (0xffff: no entry)
                    if (ok[j] && hi < kPTile) mark[base + hi] = ep;
                }
            }
        }
        lds_barrier();
        uint32_t rec[U], pos[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint32_t lt = (u / PT) * kPTile + (u % PT) * T + tid;  // the swipe's place in the run
            const uint32_t i = t0 * kPTile + lt;
            const bool act = t0 + u / PT < t1 && i < A.n;
            const bool valid = act && (hv[u] >> 24) == 0 && mark[lt] != ep;
            if (A.out && act) nt_st<16>(A.out + i, uint8_t(valid));
            pos[u] = 0xffffffffu;
            rec[u] = 0;
            if (valid) {
                if (sl[u] >= A.nslots) {
                    atomicOr(A.err, 1u);
                } else {
                    const uint32_t w = sl[u] >> S.klog, b = w & bmask;
                    const uint32_t sib = ((w >> S.b1) << S.klog) | (sl[u] & kmask);
                    rec[u] = (sib << kSegRecShift) | ((hv[u] & 0x3fffu) << 6) | (hv[u] >> 16);
                    pos[u] = (b << 16) | atomicAdd(&cnt[b], 1u);
                }
            }
        }
        lds_barrier();
        uint32_t total;
        const uint32_t cv = tid < S.nb1 ? cnt[tid] : 0u;
        // Each bucket's reservation is rounded up to 4 records, so every
        // reservation starts 16-B aligned; the pad holds records of rank 0 (a
        // real record's rank is >= 1), which D skips.  The reservation is a
        // buffer atomic issued here and first waited for after the placement
        // (its address is one VGPR rebuilt from tid: no 64-bit pointer is kept
        // live -- and spilled -- across the run).
        const uint32_t cvp = (cv + 3) & ~3u;
        uint32_t abase = 0;
        if (cv)
            abase = uint32_t(__builtin_amdgcn_raw_ptr_buffer_atomic_add_i32(
                int(cvp), part_rsrc(S.fill, S.nsub * (S.nb1 + 1) * kSegFillStride * 4), int(seg_fill_at(S, tid) * 4), 0,
                0));
        // one scan for both run layouts (the padded prefix in the high half;
        // both totals stay below 2^16)
        uint32_t tot2;
        const uint32_t ex2 = seg_scan((cvp << 16) | cv, ws, tot2);
        const uint32_t ex = ex2 & 0xffffu, exp = ex2 >> 16;
        total = tot2 & 0xffffu;
        // (the padded layout when it fits the run's LDS, else the unpadded one:
        // block-uniform)
        const bool padded = (tot2 >> 16) <= kSegRunSw;
        if (tid < S.nb1) {
            cnt[tid] = padded ? exp : ex;
            if (padded)
                for (uint32_t k = cv; k < cvp; k++) srec[exp + k] = 0u;
        }
        lds_barrier();
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (pos[u] != 0xffffffffu) {
                const uint32_t b = pos[u] >> 16, at = cnt[b] + (pos[u] & 0xffffu);
                srec[at] = rec[u];
                // (the record's bucket, tagged so that no run's epoch
                // (<= kSegMaxRuns < 0x8000) ever equals it; the padded layout
                // reads it at group starts only)
                if (!padded || (at & 3u) == 0) mark[at] = uint16_t(0x8000u | b);
            }
        // the run's chunk slots (after the placement, so that no record
        // registers are live across them); record j of the run (bucket h)
        // is then the bucket's sequence index i = j + (base - start of h
        // in the run), in the bucket's first or second chunk of this
        // reservation (told apart by i's chunk parity)
        const uint32_t aslot = cv ? seg_arena_slots(S, A.err, tid, cvp, abase) : 0u;
        lds_barrier();  // the placement's reads of cnt are done
        if (tid < S.nb1) {
            cnt[tid] = abase - (padded ? exp : ex);
            slt[tid] = aslot;
        }
        lds_barrier();
        auto slot_of = [](uint32_t i, uint32_t v) {
            return ((i >> 13) & 1u) == (v >> 28) ? (v & 0x3fffu) : ((v >> 14) & 0x3fffu);
        };
        if (padded) {
            // every 4-record group lies in one bucket and one chunk, 16-B
            // aligned at both ends (a group's first record is never a pad)
            const uint32_t ng = (tot2 >> 16) / 4;
            for (uint32_t g = tid; g < ng; g += T) {
                const uint32_t h = mark[4 * g] & (kSegMaxB1 - 1), i = 4 * g + cnt[h];
                nt2_st<1>(reinterpret_cast<part_u32x4 *>(S.r1 + size_t(slot_of(i, slt[h])) * kSegChunk +
                                                         (i & (kSegChunk - 1))),
                          reinterpret_cast<const part_u32x4 *>(srec)[g]);
            }
        } else {
            // (a run too full for its pads in LDS) four records per
            // thread: one 16-B store when they share a bucket and a chunk,
            // else one store each; each bucket's pad stored by its thread
            typedef uint32_t u32x4a __attribute__((ext_vector_type(4), aligned(4)));
            for (uint32_t g = tid; g * 4 < total; g += T) {
                const uint32_t j = g * 4;
                const part_u32x4 v = reinterpret_cast<const part_u32x4 *>(srec)[g];
                const uint2 mk = reinterpret_cast<const uint2 *>(mark)[g];
                const uint32_t m[4] = {mk.x & 0xffffu, mk.x >> 16, mk.y & 0xffffu, mk.y >> 16};
                const uint32_t h0 = m[0] & (kSegMaxB1 - 1), i0 = j + cnt[h0];
                if (j + 4 <= total && m[3] == m[0] && (i0 & (kSegChunk - 1)) <= kSegChunk - 4) {
                    *reinterpret_cast<u32x4a *>(S.r1 + size_t(slot_of(i0, slt[h0])) * kSegChunk +
                                                (i0 & (kSegChunk - 1))) = u32x4a{v.x, v.y, v.z, v.w};
                } else {
#pragma unroll
                    for (uint32_t e = 0; e < 4; e++) {
                        if (j + e >= total) break;
                        const uint32_t h = m[e] & (kSegMaxB1 - 1), i = j + e + cnt[h];
                        S.r1[size_t(slot_of(i, slt[h])) * kSegChunk + (i & (kSegChunk - 1))] = v[e];
                    }
                }
            }
            if (tid < S.nb1)
                for (uint32_t k = cv; k < cvp; k++)
                    S.r1[size_t(slot_of(abase + k, aslot)) * kSegChunk + ((abase + k) & (kSegChunk - 1))] = 0u;
        }
        lds_barrier();  // cnt, slt and marks are rewritten by the next run
        // (the next run rewrites cnt, marks and srec only behind barriers
        // that every reader of this run's values has passed)
    }
}

// The per-key floors.  A record (slot, register, rank) matters only if rank >
// register.  A key that has seen many distinct ids has every one of its
// 16 384 registers at or above some value f, its floor, and a record of rank
// <= f for that key raises nothing: D drops it (P(rank <= f) = 1 - 2^-f), so
// it is neither written to r2 nor read and compared by E.
// Exact because the floor is never a cached fact about the registers:
// k_seg_floor derives it from the slab as it stands at the start of every
// window-pass group, registers only rise until the group's E has run, and the
// next group derives it again -- whatever wrote the slab before the call
// (ske_hll_clear, an import, a load, growth, a store through ske_hll_slab's
// pointer) is seen.  No floor survives a group.
// Deriving a floor reads the key's 16 KiB, so only hinted windows get one
// (the others: floor 0, nothing dropped).  The hint map -- a byte per window,
// kept from call to call behind a header naming the plan (nwin, klog, b1) it
// belongs to -- decides cost only, never a result: E1 sets a window's byte to
// kSegHotAge when (kept records << the window's floor), its estimate of the
// arrivals before the filter, reaches hot_min per key (a cut window: always),
// clears it under half of that, and k_seg_floor counts it down by one per
// group, so a window E has not seen a record of for kSegHotAge groups stops
// costing reads.  A map whose header names another plan counts as all zero:
// E1 then writes every window's byte and M the header.
__device__ __forceinline__ bool seg_hot_valid(const SegArgs &S) {
    const uint32_t *h = reinterpret_cast<const uint32_t *>(S.hot);
    return h[0] == S.nwin && h[1] == S.klog && h[2] == S.b1 && h[3] == kSegHotMagic;
}
// the floor table's entry of key k of window w (bucket-major: D's floors of
// one bucket are contiguous, indexed by the record's slot-in-bucket)
__device__ __forceinline__ uint32_t seg_floor_at(const SegArgs &S, uint32_t w, uint32_t k) {
    return ((w & (S.nb1 - 1)) << S.s1) | ((w >> S.b1) << S.klog) | k;
}
__device__ __forceinline__ part_u32x4 seg_min16(part_u32x4 a, part_u32x4 b) {
    typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));
    return __builtin_bit_cast(part_u32x4,
                              __builtin_elementwise_min(__builtin_bit_cast(u8x16, a), __builtin_bit_cast(u8x16, b)));
}
// the least of a wave's 64 x 16 bytes, in every lane
__device__ __forceinline__ uint32_t seg_wave_min8(part_u32x4 v) {
    uint32_t x = 0xffu;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++)
#pragma unroll
        for (uint32_t sh = 0; sh < 32; sh += 8) {
            const uint32_t y = (v[c] >> sh) & 0xffu;
            x = x < y ? x : y;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t z = uint32_t(__shfl_xor(int(x), o));
        x = x < z ? x : z;
    }
    return x;
}
constexpr uint32_t kSegFloorHead = 4;  // 1 KiB pieces of a key read before the rest
// One wave per hinted window (windows dealt to the waves interleaved, w mod
// waves: the hot windows are neighbours in slot order), a key's 16 KiB as 16
// loads of 16 B per lane: 4 in flight, then 12.  The table was zeroed before.
// (The reduction of a piece to one byte is plain shifts: the 4-byte vector
// form of it compiled to loads of each piece's first word only.)
constexpr uint32_t kSegFT = 256;
__global__ void __launch_bounds__(kSegFT) k_seg_floor(const uint8_t *regs, uint32_t nslots, const SegArgs S) {
    __shared__ uint32_t nfl;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t nwaves = gridDim.x * (kSegFT / 64), gw = blockIdx.x * (kSegFT / 64) + (tid >> 6);
    if (tid == 0) nfl = 0;
    __syncthreads();
    uint8_t *hot = S.hot + kSegHotHdr;
    uint32_t mine = 0;
    if (seg_hot_valid(S)) {
        // 64 of the wave's windows at a time: lane l holds the hint of window w0 + l * nwaves
        for (uint32_t w0 = gw; w0 < S.nwin; w0 += nwaves * 64) {
            const uint32_t wl = w0 + lane * nwaves;
            const uint32_t hv = wl < S.nwin ? hot[wl] : 0u;
            if (hv) hot[wl] = uint8_t((hv < kSegHotAge ? hv : kSegHotAge) - 1);
            for (uint64_t m = __ballot(hv != 0); m; m &= m - 1) {
                const uint32_t w = w0 + uint32_t(__builtin_ctzll(m)) * nwaves;
                mine++;
                for (uint32_t k = 0; k < (1u << S.klog); k++) {
                    const uint32_t slot = (w << S.klog) | k;
                    if (slot >= nslots) break;
                    const part_u32x4 *p = reinterpret_cast<const part_u32x4 *>(regs + (size_t(slot) << kHllP));
                    // the first quarter alone first: a key not yet saturated
                    // (floor 0, the table's value already) mostly shows a zero there
                    part_u32x4 v = p[lane];
#pragma unroll
                    for (uint32_t i = 1; i < kSegFloorHead; i++) v = seg_min16(v, p[i * 64 + lane]);
                    if (seg_wave_min8(v) == 0) continue;
#pragma unroll
                    for (uint32_t i = kSegFloorHead; i < (kHllRegs / 16) / 64; i++) v = seg_min16(v, p[i * 64 + lane]);
                    const uint32_t x = seg_wave_min8(v);
                    if (lane == 0) S.floor[seg_floor_at(S, w, k)] = uint8_t(x);
                }
            }
        }
    }
    if (lane == 0 && mine) atomicAdd(&nfl, mine);
    __syncthreads();
    if (tid == 0 && nfl) atomicAdd(S.fstat, (unsigned long long)nfl);
}

// D: one block per chunk of the sub-batch (grid-stride, in bucket order), its
// slot fixed or from ctab, its records read whole (16-B loads) and
// counting-sorted by window within the bucket (o2 / r2 row q = the bucket's
// first chunk + chunk).  It clears the chunk's ctab entry for the next
// sub-batch.  512 threads x 16 records at three blocks per CU: three chunks
// in flight per CU.
constexpr uint32_t kSegDT = 512;
template <uint32_t T> struct SegDA {
    static constexpr uint32_t R = kSegChunk / T;  // records per thread
    static constexpr uint32_t BPC = 3;            // blocks per CU (80 VGPRs; LDS ~39 KiB each)
    static constexpr uint32_t WPE = BPC * (T / 64) / 4;
    static_assert(T == 512, "three blocks per CU");
};
template <uint32_t T>
__global__ void __launch_bounds__(T, SegDA<T>::WPE) k_seg_da(const SegArgs S) {
    constexpr uint32_t R = SegDA<T>::R;
    static_assert(R % 4 == 0 && kSegMaxWpb <= T && kSegMaxB1 <= T, "D geometry");
    __shared__ uint32_t tot[kSegMaxB1], cbl[kSegMaxB1 + 1];
    __shared__ uint32_t c2[kSegMaxWpb + 1];
    __shared__ __attribute__((aligned(16))) uint32_t sb[kSegChunk];
    __shared__ uint32_t ws[T / 64];
    __shared__ __attribute__((aligned(16))) uint8_t fls[kSegMaxWpb * 8];  // the bucket's floors by slot-in-bucket
    __shared__ uint32_t nst[2];
    const uint32_t tid = threadIdx.x, wpb = 1u << S.wlog;
    const bool ff = S.floor != nullptr;
    uint32_t nsaw = 0, ndrop = 0;  // this thread's records seen / dropped (the floor statistics)
    if (tid < 2) nst[tid] = 0;
    const uint32_t *fl = S.fill + seg_fill_at(S, 0);
    uint32_t t = 0;
    if (tid < S.nb1) {
        t = fl[tid * kSegFillStride];
        tot[tid] = t;
    }
    uint32_t nqa;
    const uint32_t cbase = seg_scan(tid < S.nb1 ? (t + kSegChunk - 1) / kSegChunk : 0u, ws, nqa);
    // The sub-batch's region has maxch rows, which seg_rows_max
    // (sketch_seg_plan.h) proves enough for any input; were there more chunks
    // all the same, the rows stop at maxch (no row and no chunk base leaves
    // the region) and error bit 8 is set, reported as the call's error.
    const uint32_t nq = nqa < S.maxch ? nqa : S.maxch;
    if (tid < S.nb1) {
        cbl[tid] = cbase;
        if (blockIdx.x == 0) S.cb[size_t(S.s) * (S.nb1 + 1) + tid] = cbase < S.maxch ? cbase : S.maxch;
    }
    if (tid == 0 && blockIdx.x == 0) {
        S.cb[size_t(S.s) * (S.nb1 + 1) + S.nb1] = nq;
        if (nqa > S.maxch) atomicOr(S.err, 8u);
    }
    lds_barrier();
    uint32_t *r2 = S.r2 + size_t(S.s) * S.maxch * kSegChunk;
    uint32_t *o2 = S.o2 + size_t(S.s) * S.maxch * (wpb + 1);
    // chunk q of the sub-batch (bucket order, dealt round robin): bucket h,
    // its chunk c, in a fixed slot or (c >= kstat) the counted one ctab names
    const uint32_t nstat = S.nb1 * S.kstat, nslot = nstat + fl[S.nb1 * kSegFillStride];
    const __amdgpu_buffer_rsrc_t rr1 = part_rsrc(S.r1, nslot * kSegChunk * 4);
    for (uint32_t q = blockIdx.x; q < nq; q += gridDim.x) {
        const uint32_t h = __builtin_amdgcn_readfirstlane(seg_last_le(cbl, S.nb1, q));  // (empty buckets share
        const uint32_t c = q - cbl[h];                                                   // the next one's base)
        uint32_t p = h * S.kstat + c;
        if (c >= S.kstat) {
            p = nstat + __builtin_amdgcn_readfirstlane(S.ctab[size_t(h) * S.kmaxc + c]) - 1;
            lds_barrier();  // every lane has read the entry
            if (tid == 0) S.ctab[size_t(h) * S.kmaxc + c] = 0;
        }
        const uint32_t w0 = c * kSegChunk, th = tot[h];
        const uint32_t n = th - w0 < kSegChunk ? th - w0 : kSegChunk;
        uint32_t rec[R];
#pragma unroll
        for (uint32_t k = 0; k < R / 4; k++) {
            const uint32_t x = (k * T + tid) * 4;  // the piece's first record in the chunk
            const part_u32x4 v = __builtin_bit_cast(
                part_u32x4, __builtin_amdgcn_raw_buffer_load_b128(rr1, x < n ? (p * kSegChunk + x) * 4 : kOOR, 0,
                                                                  kNt2Aux<2>));
            rec[4 * k] = v.x;
            rec[4 * k + 1] = v.y;
            rec[4 * k + 2] = v.z;
            rec[4 * k + 3] = v.w;
        }
        for (uint32_t j = tid; j <= wpb; j += T) c2[j] = 0;
        // the bucket's floors (2^s1 <= 4096 bytes, contiguous in the table)
        if (ff) {
            const uint8_t *fb = S.floor + (size_t(h) << S.s1);
            if (S.s1 >= 4) {
                if (tid < (1u << (S.s1 - 4)))
                    reinterpret_cast<part_u32x4 *>(fls)[tid] = reinterpret_cast<const part_u32x4 *>(fb)[tid];
            } else if (tid < (1u << S.s1)) {
                fls[tid] = fb[tid];
            }
        }
        lds_barrier();
        uint32_t pos[R];
#pragma unroll
        for (uint32_t j = 0; j < R; j++) {
            pos[j] = 0xffffffffu;
            if ((j / 4 * T + tid) * 4 + j % 4 < n && (rec[j] & 63u) != 0) {  // (rank 0: a C1 pad)
                // a record at or under its key's floor raises nothing: dropped
                const uint32_t f = ff ? fls[rec[j] >> kSegRecShift] : 0u;
                nsaw++;
                if ((rec[j] & 63u) > f) {
                    const uint32_t w2 = (rec[j] >> (kSegRecShift + S.klog)) & (wpb - 1);
                    pos[j] = (w2 << 16) | atomicAdd(&c2[w2], 1u);
                } else {
                    ndrop++;
                }
            }
        }
        lds_barrier();
        uint32_t total;
        const uint32_t ex = seg_scan(tid < wpb ? c2[tid] : 0u, ws, total);
        if (tid < wpb) {
            c2[tid] = ex;
            o2[size_t(q) * (wpb + 1) + tid] = ex;
        }
        if (tid == 0) o2[size_t(q) * (wpb + 1) + wpb] = total;
        lds_barrier();
#pragma unroll
        for (uint32_t j = 0; j < R; j++)
            if (pos[j] != 0xffffffffu) sb[c2[pos[j] >> 16] + (pos[j] & 0xffffu)] = rec[j];
        lds_barrier();
        part_u32x4 *dst = reinterpret_cast<part_u32x4 *>(r2 + size_t(q) * kSegChunk);
        const part_u32x4 *src = reinterpret_cast<const part_u32x4 *>(sb);
        for (uint32_t j = tid; j * 4 < total; j += T) nt2_st<4>(dst + j, src[j]);
        // (the next chunk rewrites c2 and fls before its first barrier: the
        // readers of this chunk's passed the barrier before the copy-out; sb
        // is rewritten only after two more barriers)
    }
    // the floor statistics: one add per counter, block and launch
    if (ff) {
        if (nsaw) atomicAdd(&nst[0], nsaw);
        if (ndrop) atomicAdd(&nst[1], ndrop);
        __syncthreads();
        if (tid < 2 && nst[tid]) atomicAdd(S.fstat + 1 + tid, (unsigned long long)nst[tid]);
    }
}

// byte max of an LDS register (the window's copy); true if it rose
__device__ __forceinline__ bool seg_lds_max(uint32_t *w, uint32_t sh, uint32_t rank) {
    uint32_t old = *w;
    while (((old >> sh) & 0xffu) < rank) {
        const uint32_t prev = atomicCAS(w, old, (old & ~(0xffu << sh)) | (rank << sh));
        if (prev == old) return true;
        old = prev;
    }
    return false;
}

// The window pass.  A window whose records exceed its slice (a hot key's:
// at the 8-way shard the hottest lecture's day keys take ~1.8 M records of
// one window per step) is cut into slices so that no block reads more than
// slice of records (seg_slice): pass E1 (QUEUE = false) takes every window's first
// slice and queues the others; E2 (QUEUE = true) takes the queued slices;
// each slice of a cut window raises its own LDS copy of the window, stored
// whole to a copy buffer, and M (k_seg_m) stores the byte max of the copies.
// An uncut window's risen lines go straight back to the slab.
//
// Per window the block (1) issues the window's register loads (whole lines,
// 8 x 16 B per thread, kept in registers) and, at the same time, (2) reads
// the window's run table -- o2[chunk][window] of every chunk of its bucket
// in every sub-batch, the chunk bases from an LDS copy of cb -- then (3)
// reads the records 16 consecutive ones per thread (one search of the run
// prefix per thread, all 16 loads in flight), raises them in LDS and (4)
// stores the risen lines.  A window with fewer than dense_min records is
// raised in place instead (its register loads are dropped).
// Diagnostic per-item stamps of the window pass (-DSKE_SEG_STAMPS builds only;
// tools/stamps/run_seg_stamps.py): thread 0 records s_memrealtime (100 MHz)
// at 5 points of every window / queued slice, its record and run counts and
// its block and XCD, into a side buffer no output depends on.
#ifdef SKE_SEG_STAMPS
__device__ unsigned long long *ske_seg_stamp_buf;
hipError_t set_seg_stamp_buffer(void *p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(ske_seg_stamp_buf), &p, sizeof(void *));
}
#define SEG_STAMP(slot, k, v)                                                                  \
    do {                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        unsigned long long t_;                                                                 \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");        \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        if (threadIdx.x == 0 && ske_seg_stamp_buf) {                                           \
            ske_seg_stamp_buf[size_t(slot) * 8 + (k)] = t_;                                    \
            if ((k) == 4) {                                                                    \
                ske_seg_stamp_buf[size_t(slot) * 8 + 5] = (v);                                 \
                ske_seg_stamp_buf[size_t(slot) * 8 + 6] =                                      \
                    blockIdx.x | (uint64_t(__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15) << 32); \
            }                                                                                  \
        }                                                                                      \
    } while (0)
#else
hipError_t set_seg_stamp_buffer(void *) { return hipErrorNotSupported; }
#define SEG_STAMP(slot, k, v) \
    do {                      \
    } while (0)
#endif
// Block shape per window size: windows of 2^KLOG keys (16 KiB each) in
// blocks of T threads, BPC blocks resident per CU (LDS: the window + its
// staging), so that small windows keep more windows in flight per CU.
template <int KLOG> struct SegE {
    static constexpr uint32_t T = KLOG >= 2 ? 1024 : (KLOG == 1 ? 512 : 256);
    static constexpr uint32_t BPC = KLOG >= 3 ? 1 : (KLOG == 2 ? 2 : (KLOG == 1 ? 4 : 8));
    static constexpr uint32_t WPS = T / 64 * BPC / 4;  // waves per SIMD (launch bounds)
    static constexpr uint32_t RPT = KLOG >= 3 ? 16 : (KLOG == 2 ? 8 : 4);  // records per thread per round
    static constexpr uint32_t EP = KLOG == 2 ? 512 : T;  // runs staged at once
};
// records per slice of a cut window: 32 k << min(klog, 2) (64 k at klog 1:
// the window pass 0.930 -> 0.891 ms at N = 1 and 0.477 -> 0.427 ms at
// the 8-way shard against 32 k; 16 k / 8 k / 128 k slower --
// profiles/r05_ab_seg_slice.txt)
__host__ __device__ constexpr uint32_t seg_slice(uint32_t klog) { return 32768u << (klog < 2 ? klog : 2); }

template <int KLOG, bool QUEUE>
__global__ void __launch_bounds__(SegE<KLOG>::T, SegE<KLOG>::WPS) k_seg_e(const PartArgs A, const SegArgs S) {
    using E = SegE<KLOG>;
    constexpr uint32_t T = E::T;
    constexpr uint32_t KW = 1u << KLOG, WB = KW << kHllP, NPC = WB / 16 / T;  // 16-B pieces per thread
    constexpr uint32_t NL = KW * (kHllRegs / 128);                              // 128-B lines
    constexpr uint32_t RPT = E::RPT, EP = E::EP;
    constexpr uint32_t SLICE = seg_slice(KLOG);
    __shared__ __attribute__((aligned(16))) uint8_t win[WB];
    __shared__ uint8_t dirty[NL];
    __shared__ uint32_t rb[EP], rp[EP + 1];
    __shared__ uint32_t spre[2][65], cq0[2][64], ws[T / 64], hdr[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nb1m = S.nb1 - 1;  // buckets: a power of two, window W in bucket W & nb1m
    const uint32_t nitems = QUEUE ? S.q[0] : S.nwin;
    // E1 keeps the hint map (a map of another plan counts as all zero and is rewritten whole)
    const bool hinting = !QUEUE && S.hot != nullptr, hot_ok = hinting && seg_hot_valid(S);
    const __amdgpu_buffer_rsrc_t rr2 = part_rsrc(S.r2, S.nsub * S.maxch * kSegChunk * 4);
    // Items (E1: windows, E2: queued slices) go round robin over the blocks.
    // Each item's layout -- its bucket's chunk counts per sub-batch (spre:
    // prefix, cq0: the first chunk; nsub <= 64), double-buffered by item
    // parity -- its first EP runs and its window's registers are fetched in
    // phases while the previous item's records are raised and its lines
    // stored:
    //   P1  the bucket's chunk columns (loads), while the records are raised;
    //   P2  the column prefix (scan), then the item's first EP runs (loads),
    //       while the lines are stored; then the window's registers by
    //       LDS-DMA into `win`;
    //   P3  the runs' prefix (scan) and record count, when the item starts.
    // (Buckets interleave windows, so a hot key's windows fall in different
    // buckets and every bucket has about the same chunks: a window's runs
    // rarely exceed EP; more are counted and staged in batches.)
    uint32_t cq = 0, cc = 0;                // P1: this thread's sub-batch column
    uint32_t pbase = 0, plen = 0, pnp = 0;  // P2: this thread's run, the item's runs
    uint32_t hint_n = 0, floor_n = 0;       // P1 (E1, thread 0): the item's hint byte, its keys' highest floor
    auto item = [&](uint32_t it, uint32_t &wi, uint32_t &sl, uint32_t &copy) {
        wi = it;
        sl = 0;
        copy = 0xffffffffu;
        if (QUEUE) {
            const uint4 e = S.qitems[it];
            wi = e.x;
            sl = e.y;
            copy = e.z;
        }
    };
    auto p1 = [&](uint32_t wi) {
        const uint32_t h = wi & nb1m;
        if (tid < S.nsub) {
            cq = S.cb[size_t(tid) * (S.nb1 + 1) + h];
            cc = S.cb[size_t(tid) * (S.nb1 + 1) + h + 1];
        }
        if (hinting && tid == 0) {
            hint_n = hot_ok ? S.hot[kSegHotHdr + wi] : 0u;
            floor_n = 0;
            for (uint32_t k = 0; k < KW && (wi << KLOG) + k < A.nslots; k++) {
                const uint32_t fk = S.floor[seg_floor_at(S, wi, k)];
                floor_n = fk > floor_n ? fk : floor_n;
            }
        }
    };
    // the window's registers into `win` by LDS-DMA (1 KiB per wave
    // instruction, no VGPRs; bytes past the slab read as zero), waited for by
    // the __syncthreads() before the records are raised
    auto image = [&](uint32_t wi) {
        const uint32_t slot0 = wi << KLOG;
        const uint32_t nk = A.nslots - slot0 < KW ? A.nslots - slot0 : KW;
        const __amdgpu_buffer_rsrc_t r = part_rsrc(A.regs + (size_t(slot0) << kHllP), nk << kHllP);
#pragma unroll
        for (uint32_t i = 0; i < NPC; i++) {
            const uint32_t piece = i * (T / 64) + wave;  // 1 KiB pieces
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                r, (__attribute__((address_space(3))) void *)(win + piece * 1024), 16,
                int(piece * 1024 + lane * 16), 0, 0, kNt2Aux<16>);
        }
    };
    // run x of window column w2 of the bucket staged in buffer pb
    const uint32_t orow = (1u << S.wlog) + 1;
    auto run_of = [&](uint32_t pb, uint32_t x, uint32_t w2, uint32_t &base) -> uint32_t {
        const uint32_t s = seg_last_le(spre[pb], S.nsub, x);
        const size_t row = size_t(s) * S.maxch + cq0[pb][s] + (x - spre[pb][s]);
        const uint32_t *o = S.o2 + row * orow + w2;
        const uint32_t b = o[0];
        base = uint32_t(row * kSegChunk + b);  // < 2^32: the host plan checks nsub * maxch * kSegChunk
        return o[1] - b;
    };
    auto p2 = [&](uint32_t pb, uint32_t wi) {  // block-uniform; buffer pb is free
        const uint32_t c = tid < S.nsub ? cc - cq : 0u;
        const uint32_t ex = seg_scan(c, ws, pnp);
        if (tid < S.nsub) {
            spre[pb][tid] = ex;
            cq0[pb][tid] = cq;
        }
        lds_barrier();
        plen = 0;
        if (tid < EP && tid < pnp) plen = run_of(pb, tid, wi >> S.b1, pbase);
    };
    uint32_t it = blockIdx.x, par = 0;
    uint32_t wi_n = 0, sl_n = 0, copy_n = 0;
    if (it < nitems) {
        item(it, wi_n, sl_n, copy_n);
        p1(wi_n);
        p2(0, wi_n);
        image(wi_n);
    }
    // items past the first gridDim.x are claimed one ahead from a counter, so
    // a block that drew a hot window's long first slice takes fewer of the rest
    uint32_t nit = 0;
    for (; it < nitems; it = nit, par ^= 1) {
        const uint32_t wi = wi_n, sl = sl_n;
        uint32_t copy = copy_n;
        const uint32_t np = pnp;
        const uint32_t hv = hint_n, fw = floor_n;
        const uint32_t stamp = QUEUE ? S.nwin + it : wi;
        (void)stamp;
        SEG_STAMP(stamp, 0, 0);
        const uint32_t w2 = wi >> S.b1;
        const uint32_t slot0 = wi << KLOG;
        const uint32_t nk = A.nslots - slot0 < KW ? A.nslots - slot0 : KW;
        uint8_t *g = A.regs + (size_t(slot0) << kHllP);
        const uint32_t npc = nk << (kHllP - 4);  // the window's 16-B pieces in the slab
        // P3: the record count (the first batch of runs stays staged)
        uint32_t nrec, nrec0;
        {
            const uint32_t ex = seg_scan(plen, ws, nrec0);
            if (tid < EP) {
                rb[tid] = pbase;
                rp[tid] = ex;
            }
            if (tid == 0) rp[np < EP ? np : EP] = nrec0;
            nrec = nrec0;
            for (uint32_t x0 = EP; x0 < np; x0 += EP) {  // (more than EP runs: count the rest)
                uint32_t base = 0, len = 0, t;
                if (tid < EP && x0 + tid < np) len = run_of(par, x0 + tid, w2, base);
                (void)seg_scan(len, ws, t);
                nrec += t;
            }
        }
        SEG_STAMP(stamp, 1, 0);
        if (!QUEUE && nrec > SLICE) {
            // a hot window: cut into slices, the others queued for E2
            const uint32_t nsl = (nrec + SLICE - 1) / SLICE;
            if (tid == 0) {
                uint32_t base = atomicAdd(&S.q[1], nsl);
                if (base + nsl > S.ccap) {
                    base = 0xffffffffu;  // out of copies (cannot happen: see seg_scratch): one slice
                } else {
                    const uint32_t qp = atomicAdd(&S.q[0], nsl - 1);
                    for (uint32_t k = 1; k < nsl; k++) S.qitems[qp + k - 1] = make_uint4(wi, k, base + k, 0);
                    S.mlist[atomicAdd(&S.q[2], 1u)] = make_uint4(wi, base, nsl, 0);
                }
                hdr[0] = base;
            }
            lds_barrier();
            copy = hdr[0];
        }
        const bool cut = copy != 0xffffffffu;
        if (hinting && tid == 0) {
            uint32_t nv = hv;
            if (nrec) {  // (no record kept: not a visit, the hint ages)
                const uint64_t est = uint64_t(nrec) << (fw < 31 ? fw : 31), thr = uint64_t(S.hot_min) * nk;
                nv = cut || est >= thr ? kSegHotAge : (2 * est < thr ? 0u : (hv ? kSegHotAge : 0u));
            }
            if (nv != hv || !hot_ok) S.hot[kSegHotHdr + wi] = uint8_t(nv);
        }
        const uint32_t lo = cut ? sl * SLICE : 0;
        const uint32_t hi = cut ? (nrec - lo < SLICE ? nrec : lo + SLICE) : nrec;
        const bool dense = nrec > 0 && (cut || nrec >= S.dense_min);
        if (dense)
            for (uint32_t j = tid; j < NL; j += T) dirty[j] = 0;
        // (E1: per XCD -- block b takes items i = b mod 8 from counter b mod 8,
        // so the windows of a bucket (W mod nb1) stay on one XCD, whose L2
        // then serves the chunk lines two neighbouring windows' runs share)
        // (every residue mod 8 needs a block: a grid under 8 takes one counter)
        if (tid == 0)
            hdr[1] = QUEUE || gridDim.x < kPGroups
                         ? gridDim.x + atomicAdd(&S.q[QUEUE ? 5 : 4], 1u)
                         : gridDim.x + kPGroups * atomicAdd(&S.q[8 + blockIdx.x % kPGroups], 1u) +
                               blockIdx.x % kPGroups;
        __syncthreads();  // the window's registers landed in LDS (vmcnt), its first runs staged
        // P1 of the next item: its loads fly while this item's records are raised
        nit = hdr[1];
        if (nit < nitems) {
            item(nit, wi_n, sl_n, copy_n);
            p1(wi_n);
        }
        SEG_STAMP(stamp, 2, 0);
        // records [lo, hi) of the concatenated runs, runs staged EP at a time
        for (uint32_t x0 = 0, p0 = 0; x0 < np && p0 < hi; x0 += EP) {
            const uint32_t nx = np - x0 < EP ? np - x0 : EP;
            uint32_t btot = nrec0;
            if (x0 > 0) {  // (a window with more than EP runs: restage)
                lds_barrier();
                uint32_t base = 0, len = 0;
                if (tid < nx) len = run_of(par, x0 + tid, w2, base);
                const uint32_t ex = seg_scan(len, ws, btot);
                if (tid < nx) {
                    rb[tid] = base;
                    rp[tid] = ex;
                }
                if (tid == 0) rp[nx] = btot;
                lds_barrier();
            }
            // this batch's records [p0, p0 + btot) of the window; ours: [lo, hi).
            // A wave takes 64 * RPT consecutive records per round, lane l the
            // ones at l + 64 c (coalesced loads); the run of the wave's first
            // record is searched once and every lane walks on from it.
            const uint32_t f_lo = lo > p0 ? lo - p0 : 0, f_hi = hi - p0 < btot ? hi - p0 : btot;
            // (dense: the window's registers in LDS; sparse: in place, in HBM)
            const __amdgpu_buffer_rsrc_t rgw = part_rsrc(g, npc * 16);
            auto round = [&](auto dense_c) {
                constexpr bool D = decltype(dense_c)::value;
                for (uint32_t r0 = f_lo + wave * 64 * RPT; r0 - wave * 64 * RPT < f_hi; r0 += T * RPT) {
                    uint32_t rec[RPT];
#pragma unroll
                    for (uint32_t c = 0; c < RPT; c++) rec[c] = 0;
                    if (r0 < f_hi) {  // wave-uniform
                        uint32_t j = seg_last_le(rp, nx, r0);
#pragma unroll
                        for (uint32_t c = 0; c < RPT; c++) {
                            const uint32_t f = r0 + c * 64 + lane;
                            if (f < f_hi) {
                                while (rp[j + 1] <= f) j++;
                                rec[c] = __builtin_amdgcn_raw_buffer_load_b32(rr2, (rb[j] + (f - rp[j])) * 4, 0, kNt2Aux<8>);
                            }
                        }
                    }
                    // the registers' words, all read before any CAS (a raise
                    // is rare once the slab is warm)
                    uint32_t old[RPT];
#pragma unroll
                    for (uint32_t c = 0; c < RPT; c++) {
                        const uint32_t a = (((rec[c] >> kSegRecShift) & (KW - 1)) << kHllP) | ((rec[c] >> 6) & 0x3fffu);
                        old[c] = 0xffffffffu;
                        if (rec[c] & 63u)
                            old[c] = D ? reinterpret_cast<const uint32_t *>(win)[a >> 2]
                                       : __builtin_amdgcn_raw_buffer_load_b32(rgw, a & ~3u, 0, 0);
                    }
#pragma unroll
                    for (uint32_t c = 0; c < RPT; c++) {
                        const uint32_t a = (((rec[c] >> kSegRecShift) & (KW - 1)) << kHllP) | ((rec[c] >> 6) & 0x3fffu);
                        const uint32_t rank = rec[c] & 63u, sh = (a & 3u) * 8;
                        if (((old[c] >> sh) & 0xffu) >= rank) continue;
                        if constexpr (D) {
                            if (seg_lds_max(reinterpret_cast<uint32_t *>(win + (a & ~3u)), sh, rank)) dirty[a >> 7] = 1;
                        } else {
                            part_reg_max(reinterpret_cast<uint32_t *>(g + (a & ~3u)), sh, rank, old[c]);
                        }
                    }
                }
            };
            if (dense)
                round(std::true_type{});
            else
                round(std::false_type{});
            p0 += btot;
        }
        lds_barrier();  // every raise in LDS done; rb / rp free
        SEG_STAMP(stamp, 3, 0);
        // P2 of the next item (its layout into the other buffer), its runs'
        // loads flying while this item's lines are stored
        if (nit < nitems) p2(par ^ 1, wi_n);
        if (cut) {
            // a slice of a cut window: the whole LDS copy, merged by k_seg_m
            part_u32x4 *dst = reinterpret_cast<part_u32x4 *>(S.copies + size_t(copy) * WB);
#pragma unroll
            for (uint32_t i = 0; i < NPC; i++) dst[i * T + tid] = reinterpret_cast<const part_u32x4 *>(win)[i * T + tid];
        } else if (dense) {
            // the lines that rose, stored back whole
#pragma unroll
            for (uint32_t i = 0; i < NPC; i++) {
                const uint32_t j = i * T + tid;
                if (j < npc && dirty[j >> 3])
                    nt2_st<32>(reinterpret_cast<part_u32x4 *>(g) + j, reinterpret_cast<const part_u32x4 *>(win)[j]);
            }
        }
        lds_barrier();  // win, dirty and hdr are rewritten by the next item
        if (nit < nitems) image(wi_n);
        SEG_STAMP(stamp, 4, uint64_t(nrec) | (uint64_t(np) << 32) | (uint64_t(dense) << 63));
    }
}

// bytewise max of two 16-byte pieces
__device__ __forceinline__ part_u32x4 seg_max16(part_u32x4 a, part_u32x4 b) {
    typedef unsigned char u8x16 __attribute__((ext_vector_type(16)));
    return __builtin_bit_cast(part_u32x4,
                              __builtin_elementwise_max(__builtin_bit_cast(u8x16, a), __builtin_bit_cast(u8x16, b)));
}

// M: every cut window = the byte max of its slices' copies (each started
// from the slab's registers, so the max holds every slice's raises)
template <int KLOG>
__global__ void __launch_bounds__(1024) k_seg_m(const PartArgs A, const SegArgs S) {
    constexpr uint32_t KW = 1u << KLOG, WB = KW << kHllP;
    const uint32_t nm = S.q[2];
    // (E1 has written every window's hint by now: the map belongs to this plan)
    if (S.hot != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {
        uint32_t *h = reinterpret_cast<uint32_t *>(S.hot);
        h[0] = S.nwin;
        h[1] = S.klog;
        h[2] = S.b1;
        h[3] = kSegHotMagic;
    }
    for (uint32_t m = blockIdx.x; m < nm; m += gridDim.x) {
        const uint4 e = S.mlist[m];
        const uint32_t slot0 = e.x << KLOG;
        const uint32_t nk = A.nslots - slot0 < KW ? A.nslots - slot0 : KW;
        part_u32x4 *g = reinterpret_cast<part_u32x4 *>(A.regs + (size_t(slot0) << kHllP));
        for (uint32_t j = threadIdx.x; j < (nk << (kHllP - 4)); j += 1024) {
            part_u32x4 v = reinterpret_cast<const part_u32x4 *>(S.copies + size_t(e.y) * WB)[j];
            for (uint32_t c = 1; c < e.z; c++)
                v = seg_max16(v, reinterpret_cast<const part_u32x4 *>(S.copies + size_t(e.y + c) * WB)[j]);
            g[j] = v;
        }
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// (the geometry, seg_plan, and the slot sizing, seg_slots: sketch_seg_plan.h)

// segmented for this batch: the fail-list chain, the option, and (auto) at
// least density_x100 / 100 swipes per 128-B register line of the slab
bool seg_use(const PartArgs &A, const SegOpts &so, uint32_t nslots, uint64_t n, uint32_t sub, SegPlan *P) {
    if (so.mode == 0 || !part_flist(A) || !seg_plan(nslots, n, sub, so, P)) return false;
    if (so.mode == 1) return true;
    // break-evens measured at C3: ~5 swipes per line over a
    // 1.6 GB slab, ~12 over the 8-way shard's 205 MB one, which the 256 MiB
    // Infinity Cache holds (pass C's random requests are served there): the
    // threshold doubles for a slab of at most 256 MiB, so the shard's 16 M
    // step (~11 per line) takes pass C and its 2^27 step (~92) this form
    const uint64_t thr = uint64_t(so.density_x100) * ((uint64_t(nslots) << kHllP) <= (256ull << 20) ? 2 : 1);
    return n * 100 >= thr * nslots * (kHllRegs / 128);
}

// the segmented PFADD's scratch (context slots kScrSeg*, ordered with K1's
// through ske_ctx::xr; routing has slots of its own)
hipError_t seg_scratch(const SegPlan &P, uint32_t sub, uint64_t n, Scratch *scr, SegArgs *S) {
    const uint64_t mg = std::min<uint64_t>(n, uint64_t(P.nsub) * sub);  // swipes of one window pass
    hipError_t e = hipSuccess;
    // chunk slots and rows: seg_slots (sketch_seg_plan.h)
    const SegSlots L = seg_slots(P, sub, n);
    S->kstat = L.kstat;
    S->kmaxc = L.kmaxc;
    S->r1 = (uint32_t *)scratch_get(scr, kScrSegR1, size_t(L.r1_slots) * kSegChunk * 4, &e);
    if (e == hipSuccess)
        S->fill = (uint32_t *)scratch_get(scr, kScrSegFill, size_t(P.nsub) * (P.nb1 + 1) * kSegFillStride * 4, &e);
    if (e == hipSuccess) S->ctab = (uint32_t *)scratch_get(scr, kScrSegCtab, size_t(P.nb1) * S->kmaxc * 4, &e);
    if (e == hipSuccess)
        S->r2 = (uint32_t *)scratch_get(scr, kScrSegR2, size_t(L.rows) * kSegChunk * 4, &e);
    if (e == hipSuccess)
        S->o2 = (uint32_t *)scratch_get(scr, kScrSegO2, size_t(L.rows) * ((1u << P.wlog) + 1) * 4, &e);
    if (e == hipSuccess) S->cb = (uint32_t *)scratch_get(scr, kScrSegCb, size_t(P.nsub) * (P.nb1 + 1) * 4, &e);
    // the window pass's cut windows: a cut window has > slice records and
    // ceil(records / slice) < 2 records / slice slices, so 2 n / slice
    // copies, queue entries and cut windows always suffice
    const uint32_t ccap = uint32_t(2 * ((mg + seg_slice(P.klog) - 1) / seg_slice(P.klog)) + 2);
    const size_t wb = size_t(1) << (P.klog + kHllP);
    if (e == hipSuccess) S->q = (uint32_t *)scratch_get(scr, kScrSegQ, 64, &e);
    if (e == hipSuccess) S->qitems = (uint4 *)scratch_get(scr, kScrSegQitems, size_t(ccap) * 16, &e);
    if (e == hipSuccess) S->mlist = (uint4 *)scratch_get(scr, kScrSegMlist, size_t(ccap) * 16, &e);
    if (e == hipSuccess) S->copies = (uint8_t *)scratch_get(scr, kScrSegCopies, size_t(ccap) * wb, &e);
    // the per-key floors: the group's table, the hint map (kept from call to
    // call: zeroed when allocated) and the statistics
    S->floor = nullptr;
    S->hot = nullptr;
    S->fstat = nullptr;
    S->hot_min = P.hot_min;
    if (P.floor) {
        if (e == hipSuccess) S->floor = (uint8_t *)scratch_get(scr, kScrSegFloor, size_t(P.nb1) << P.s1, &e);
        if (e == hipSuccess) S->hot = (uint8_t *)scratch_get_zeroed(scr, kScrSegHot, kSegHotHdr + size_t(P.nwin), &e);
        if (e == hipSuccess) S->fstat = (unsigned long long *)scratch_get_zeroed(scr, kScrSegFstat, 3 * 8, &e);
    }
    S->ccap = ccap;
    S->nb1 = P.nb1;
    S->s1 = P.s1;
    S->b1 = P.b1;
    S->wlog = P.wlog;
    S->klog = P.klog;
    S->nsub = P.nsub;
    S->maxch = P.maxch;
    S->nwin = P.nwin;
    S->dense_min = P.dense_min;
    return e;
}

hipError_t launch_seg_sub(const PartArgs &A, SegArgs &S, const SegPlan &P, uint32_t si, int cus, hipStream_t st,
                          PassHook hook, void *hook_user) {
    if (hook) hook(hook_user, 2, 0, st);
    S.s = si % P.nsub;
    S.err = A.err;
    S.nruns = (A.ntiles + kSegRunTiles - 1) / kSegRunTiles;
    if (S.s == 0) {
        // the group's fill counts, and the chunk table (D clears what C1
        // published, so this only matters for a fresh buffer or a call that
        // stopped between C1 and D)
        hipError_t e = hipMemsetAsync(S.fill, 0, size_t(P.nsub) * (P.nb1 + 1) * kSegFillStride * 4, st);
        if (e == hipSuccess) e = hipMemsetAsync(S.ctab, 0, size_t(P.nb1) * S.kmaxc * 4, st);
        // the group's floors, from the slab as it stands now
        if (e == hipSuccess && S.floor) e = hipMemsetAsync(S.floor, 0, size_t(P.nb1) << P.s1, st);
        if (e != hipSuccess) return e;
        if (S.floor)
            hipLaunchKernelGGL(k_seg_floor, dim3(unsigned(cus) * 4), dim3(kSegFT), 0, st, A.regs, A.nslots, S);
    }
    hipLaunchKernelGGL(k_seg_c1<kSegC1T>, dim3(std::min(S.nruns, unsigned(cus) * SegC1<kSegC1T>::BPC)), dim3(kSegC1T),
                       0, st, A, S);
    if (hook) hook(hook_user, 2, 1, st);
    if (hook) hook(hook_user, 3, 0, st);
    hipLaunchKernelGGL(k_seg_da<kSegDT>, dim3(unsigned(cus) * SegDA<kSegDT>::BPC), dim3(kSegDT), 0, st, S);
    if (hook) hook(hook_user, 3, 1, st);
    return hipGetLastError();
}

// every window of the slab once after each group of P.nsub sub-batches (the
// whole batch unless it is very large): E1 (first slices), E2 (queued slices
// of cut windows), M (cut windows merged)
template <int K> static void seg_e_launch(const PartArgs &A, const SegArgs &S, int cus, hipStream_t st) {
    hipLaunchKernelGGL((k_seg_e<K, false>), dim3(unsigned(cus) * SegE<K>::BPC), dim3(SegE<K>::T), 0, st, A, S);
    hipLaunchKernelGGL((k_seg_e<K, true>), dim3(unsigned(cus) * SegE<K>::BPC), dim3(SegE<K>::T), 0, st, A, S);
    hipLaunchKernelGGL(k_seg_m<K>, dim3(unsigned(cus)), dim3(1024), 0, st, A, S);
}
hipError_t launch_seg_windows(PartArgs A, SegArgs S, const SegPlan &P, uint32_t ns, int cus, hipStream_t st,
                              PassHook hook, void *hook_user) {
    S.nsub = ns;
    A.n = 0;
    if (hook) hook(hook_user, 4, 0, st);
    const hipError_t e = hipMemsetAsync(S.q, 0, 64, st);
    if (e != hipSuccess) return e;
    switch (P.klog) {
        case 0: seg_e_launch<0>(A, S, cus, st); break;
        case 1: seg_e_launch<1>(A, S, cus, st); break;
        case 2: seg_e_launch<2>(A, S, cus, st); break;
        case 3: seg_e_launch<3>(A, S, cus, st); break;
    }
    if (hook) hook(hook_user, 4, 1, st);
    return hipGetLastError();
}

}  // namespace ske
