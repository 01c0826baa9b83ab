// sketch_hh_stats.hip -- moments and order statistics of a heavy-hitter set's
// current estimates, computed where the estimates are.
// All of it is integer arithmetic, so every result is independent of thread
// order and identical from run to run.
//
//   k_hhs_est    a thread per slot as k_hh_list (up to 16 slots a thread in the
//                largest sets): an occupied slot recomputes its estimate; over
//                those that pass (estimate >= threshold) the workgroup sums n,
//                the estimates, the two halves of their squares, min and max
//                -- per lane, inside the wavefront, then across the workgroup's
//                four -- and issues one set of global atomics.  The add of n
//                returns the workgroup's place in the compacted array of
//                passing estimates (ballot, leader add, lane rank; the leader
//                is the workgroup's, not the wavefront's).
//   k_hhs_begin  the ranks: those the caller gave, or the two median ranks
//                derived from n; a rank >= n turns the select off.
//   k_hhs_hist   a round of the radix select (sketch_hh_select.h): per rank a
//                histogram in LDS of the round's digit over the estimates that
//                carry the rank's prefix, flushed with global atomics.  Ranks
//                with equal prefixes share the first one's histogram.
//   k_hhs_walk   one workgroup: walks each rank's histogram to fix its next
//                digit, regroups the ranks by prefix, zeroes the histograms.
//
// Nothing waits on another workgroup: the kernels of a call follow each other
// on the stream, and the host copies the record once, after the last.
#include "sketch_cms_dev.h"
#include "sketch_hh_select.h"

namespace ske {
namespace {

constexpr int kHhsBlock = 256;
constexpr int kHhsWaves = kHhsBlock / 64;
constexpr uint32_t kHhsMaxIters = 16;     // slots per thread of the estimate pass, at most (16 KiB of LDS)
constexpr uint32_t kHhsEstGrid = 1024;    // a thread takes more than one slot only past this many workgroups
static_assert(kHhStatRanks == kHhMaxRanks && kHhSelBins == 256, "HhStatDev holds kHhMaxRanks histograms of 256 counts");

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_max32(uint32_t v) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o, 64);
        v = v > w ? v : w;
    }
    return v;
}

// Workgroup b takes the `iters` * 256 slots from b * iters * 256 on, 256 at a
// time (the launcher makes the grid cover the slots exactly, so every lane
// reaches every ballot and barrier).  Per step, the passing estimates are
// compacted into LDS -- ballot, the wavefronts' counts through LDS, lane rank;
// the counts are double-buffered by the step's parity, so one barrier a step
// is enough -- and every lane keeps private sums.  At the end the sums are
// reduced inside the wavefront, then across the workgroup's four, and the
// workgroup issues ONE set of global atomics; the add of n returns its place
// in the compacted array, to which it copies its LDS piece.
//
// Why more than one slot per thread: with one (the first form measured, 65 536
// workgroups at 2^24 slots) the call took 4.8 ms, of which the hashing and the
// 28 bytes per slot were 0.27 ms -- the rest was 6 x 65 536 atomics queueing on
// one 64-byte line.  kHhsMaxIters = 16 leaves at most 4096 workgroups.
//
// A square is below 2^64, each of its halves below 2^32: a lane's sums over 16
// slots stay below 2^36, a workgroup's below 2^44 and a whole set's (2^24
// slots) below 2^56 -- sq_lo and sq_hi never carry into each other, so they are
// two independent atomic sums.  The minimum is kept as the maximum of
// ~estimate: the record starts zeroed, and 0 is that maximum's neutral value.
__global__ void __launch_bounds__(kHhsBlock) k_hhs_est(const CmsTable T, const HhSet S, uint32_t threshold,
                                                       HhStatDev *D, uint32_t *out, uint32_t iters) {
    __shared__ uint32_t s_est[kHhsMaxIters * kHhsBlock];
    __shared__ unsigned long long w_sum[kHhsWaves], w_lo[kHhsWaves], w_hi[kHhsWaves];
    __shared__ uint32_t w_n[2][kHhsWaves], w_nmin[kHhsWaves], w_max[kHhsWaves];
    __shared__ uint32_t s_base;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long sum = 0, lo = 0, hi = 0;
    uint32_t nmin = 0, mx = 0;
    uint32_t run = 0;  // entries of s_est so far: the same in every thread; at most iters * 256
    for (uint32_t it_no = 0; it_no < iters; it_no++) {
        const uint32_t slot = (blockIdx.x * iters + it_no) * kHhsBlock + threadIdx.x;
        uint32_t est = 0;
        bool pass = false;
        if (S.claim[slot] != 0) {
            Item it{};
            it.w0 = S.ids[2 * uint64_t(slot)];
            it.w1 = S.ids[2 * uint64_t(slot) + 1];
            it.len = S.len[slot];
            est = 0xffffffffu;
            for (uint32_t r = 0; r < T.depth; r++) est = umin32(est, T.cells[cms_cell(T, it, r)]);
            pass = est >= threshold;
        }
        // not wave_append: the base is the workgroup's running count in LDS, no counter in memory is added to
        const unsigned long long votes = __ballot(pass);
        if (lane == 0) w_n[it_no & 1][wave] = uint32_t(__popcll(votes));
        __syncthreads();
        uint32_t at = run + uint32_t(__popcll(votes & ((1ull << lane) - 1)));
        for (uint32_t w = 0; w < kHhsWaves; w++) {
            const uint32_t c = w_n[it_no & 1][w];
            if (w < wave) at += c;
            run += c;
        }
        if (pass) {
            s_est[at] = est;
            const unsigned long long sq = (unsigned long long)est * est;
            sum += est;
            lo += sq & 0xffffffffull;
            hi += sq >> 32;
            nmin = nmin > ~est ? nmin : ~est;
            mx = mx > est ? mx : est;
        }
    }
    sum = wave_sum64(sum);
    lo = wave_sum64(lo);
    hi = wave_sum64(hi);
    nmin = wave_max32(nmin);
    mx = wave_max32(mx);
    if (lane == 0) {
        w_sum[wave] = sum;
        w_lo[wave] = lo;
        w_hi[wave] = hi;
        w_nmin[wave] = nmin;
        w_max[wave] = mx;
    }
    __syncthreads();  // also: every s_est entry is written
    if (threadIdx.x == 0) {
        unsigned long long bs = 0, bl = 0, bh = 0;
        uint32_t bnmin = 0, bmax = 0;
        for (int w = 0; w < kHhsWaves; w++) {
            bs += w_sum[w];
            bl += w_lo[w];
            bh += w_hi[w];
            bnmin = bnmin > w_nmin[w] ? bnmin : w_nmin[w];
            bmax = bmax > w_max[w] ? bmax : w_max[w];
        }
        uint32_t base = 0;
        if (run) {
            base = atomicAdd(&D->n, run);
            atomicAdd(&D->sum, bs);
            atomicAdd(&D->sq_lo, bl);
            atomicAdd(&D->sq_hi, bh);
            atomicMax(&D->nmin, bnmin);
            atomicMax(&D->max, bmax);
        }
        s_base = base;
    }
    __syncthreads();
    // s_base + i < the number of passing slots <= the slots: out holds one entry per slot
    for (uint32_t i = threadIdx.x; i < run; i += kHhsBlock) out[s_base + i] = s_est[i];
}


// one wavefront; R.n == 0: the median ranks from n
__global__ void __launch_bounds__(64) k_hhs_begin(const HhSet S, const HhRanks R, HhStatDev *D) {
    __shared__ uint32_t s_bad;
    const uint32_t j = threadIdx.x, n = D->n;
    if (j == 0) s_bad = 0;
    __syncthreads();
    const uint32_t nr = R.n ? R.n : (n ? 2u : 0u);
    unsigned long long r = 0;
    if (j < nr) {
        r = R.n ? R.r[j] : (j == 0 ? (n - 1) / 2 : n / 2);
        if (r >= n) atomicOr(&s_bad, 1u);
    }
    __syncthreads();
    const bool bad = s_bad != 0;
    if (j < kHhStatRanks) {
        D->prefix[j] = 0;
        D->lead[j] = 0;  // no digit is fixed yet: every rank reads the first one's histogram
        D->rank[j] = j < nr && !bad ? r : 0;
    }
    if (j == 0) {
        D->min = n ? ~D->nmin : 0u;
        D->complete = *S.overflow == 0;
        D->bad = bad;
        D->nr = bad ? 0u : nr;
    }
}

// Workgroup b takes the estimates b * 256 .. + 255, then strides by the grid;
// those that start past n leave at once (n is the same for the whole
// workgroup).  A wavefront steps through the array together -- its loop bound
// is the wavefront's first index -- so every lane reaches the ballots.  A
// wavefront whose matching estimates all have one digit (the high digits of
// counts are mostly 0) adds them as one LDS atomic.
__global__ void __launch_bounds__(kHhsBlock) k_hhs_hist(const uint32_t *est, HhStatDev *D, uint32_t shift) {
    __shared__ uint32_t h[kHhStatRanks * kHhSelBins];
    __shared__ uint32_t s_prefix[kHhStatRanks], s_lead[kHhStatRanks];
    const uint32_t nr = D->nr, n = D->n;
    if (nr == 0 || blockIdx.x * uint32_t(kHhsBlock) >= n) return;
    for (uint32_t i = threadIdx.x; i < nr * kHhSelBins; i += kHhsBlock) h[i] = 0;
    if (threadIdx.x < nr) {
        s_prefix[threadIdx.x] = D->prefix[threadIdx.x];
        s_lead[threadIdx.x] = D->lead[threadIdx.x];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, stride = gridDim.x * uint32_t(kHhsBlock);
    for (uint32_t base = blockIdx.x * uint32_t(kHhsBlock) + (threadIdx.x & ~63u); base < n; base += stride) {
        const bool live = base + lane < n;
        const uint32_t v = live ? est[base + lane] : 0u;
        const uint32_t d = hh_sel_digit(v, shift);
        for (uint32_t j = 0; j < nr; j++) {
            if (s_lead[j] != j) continue;
            const bool m = live && hh_sel_matches(v, s_prefix[j], shift);
            const unsigned long long mv = __ballot(m);
            if (mv == 0) continue;
            const uint32_t first = uint32_t(__builtin_ctzll(mv));
            const uint32_t d0 = __shfl(d, int(first), 64);
            if (__ballot(m && d == d0) == mv) {
                if (lane == first) atomicAdd(&h[j * kHhSelBins + d0], uint32_t(__popcll(mv)));
            } else if (m) {
                atomicAdd(&h[j * kHhSelBins + d], 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nr * kHhSelBins; i += kHhsBlock) {
        const uint32_t j = i / kHhSelBins;
        if (s_lead[j] == j && h[i]) atomicAdd(&D->hist[i], h[i]);
    }
}

// one workgroup
__global__ void __launch_bounds__(kHhsBlock) k_hhs_walk(HhStatDev *D, uint32_t shift) {
    __shared__ uint32_t h[kHhStatRanks * kHhSelBins];
    __shared__ uint32_t s_prefix[kHhStatRanks];
    const uint32_t nr = D->nr;
    if (nr == 0) return;
    for (uint32_t i = threadIdx.x; i < nr * kHhSelBins; i += kHhsBlock) {
        h[i] = D->hist[i];
        D->hist[i] = 0;  // for the next round
    }
    __syncthreads();
    const uint32_t j = threadIdx.x;
    if (j < nr) {
        uint64_t left = 0;
        const uint32_t d = hh_sel_walk(h + D->lead[j] * kHhSelBins, kHhSelBins, D->rank[j], &left);
        const uint32_t p = D->prefix[j] | d << shift;
        D->rank[j] = left;
        D->prefix[j] = p;
        s_prefix[j] = p;
    }
    __syncthreads();
    if (j < nr) {
        uint32_t l = j;
        for (uint32_t i = 0; i < j; i++)
            if (s_prefix[i] == s_prefix[j]) {
                l = i;
                break;
            }
        D->lead[j] = l;
    }
}

}  // namespace

hipError_t launch_hh_stats(const CmsTable &T, const HhSet &S, uint32_t threshold, const HhRanks &R, HhStatDev *D,
                           uint32_t *est, int cus, hipStream_t st) {
    const uint32_t slots = S.mask + 1;
    if (slots % kHhsBlock || R.n > kHhStatRanks) return hipErrorInvalidValue;
    // 256 slots a workgroup up to kHhsEstGrid workgroups (2^18 slots), then 2, 4, .. kHhsMaxIters steps of
    // 256: the capacity is a power of two, so the steps are one and divide it
    uint32_t iters = slots / (kHhsBlock * kHhsEstGrid);
    if (iters > kHhsMaxIters) iters = kHhsMaxIters;
    if (iters < 1) iters = 1;
    if (slots % (iters * kHhsBlock)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hhs_est, dim3(slots / (iters * kHhsBlock)), dim3(kHhsBlock), 0, st, T, S, threshold, D, est,
                       iters);
    hipLaunchKernelGGL(k_hhs_begin, dim3(1), dim3(64), 0, st, S, R, D);
    // a histogram workgroup per 2048 slots, four per CU at most: each then strides
    uint32_t grid = slots / (8 * kHhsBlock);
    if (cus > 0 && grid > uint32_t(cus) * 4) grid = uint32_t(cus) * 4;
    if (grid < 1) grid = 1;
    for (uint32_t r = 0; r < kHhSelRounds; r++) {
        hipLaunchKernelGGL(k_hhs_hist, dim3(grid), dim3(kHhsBlock), 0, st, est, D, hh_sel_shift(r));
        hipLaunchKernelGGL(k_hhs_walk, dim3(1), dim3(kHhsBlock), 0, st, D, hh_sel_shift(r));
    }
    return hipGetLastError();
}

}  // namespace ske
