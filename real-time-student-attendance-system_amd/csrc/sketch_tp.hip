// sketch_tp.hip -- time profile kernel (DESIGN.md "Time profile"): the batch's
// swipe times (int64 seconds since 1970-01-01 UTC) are binned by weekday and
// hour (tp_time, sketch_common.h) into 168 u64 counters, and every swipe gets a
// "late" byte (its second of the day >= late_from), whatever the mask says.
//
// Outline of the Count-Min Sketch LDS form (sketch_cms.hip): one workgroup per
// CU sums its share of the batch into 168 private u32 bins in LDS, then adds
// its non-zero bins to the counters in memory, one 64-bit atomic each.  The
// batch has fewer than 2^32 - 1 swipes, so no LDS bin wraps.
//
// A real batch is a degenerate histogram: its swipes share one or two bins.
// Form 0 therefore tests, once per tile, whether the 256 swipes a wavefront
// holds all fall into one bin; then one lane adds their number with a single
// LDS atomic, otherwise every lane adds its own.  Form 1 is the plain add per
// lane, always.
#include "sketch_common.h"
#include "sketch_internal.h"

namespace ske {
namespace {

constexpr int kTpBlock = 1024;  // one workgroup per CU
constexpr int kTpPer = 4;       // swipes per thread and tile: 32 B of epochs, 4 mask bytes, 4 late bytes

typedef long long tp_ll2 __attribute__((ext_vector_type(2)));

// How the batch is cut: swipes [0, head) and [head + 4 * ngroups, n) go one by
// one (at most 6), the groups of four between them through wide accesses where
// the pointers allow: head is chosen for the mask (else late, else the epochs).
struct TpPlan {
    uint32_t head, ngroups;
    bool e16;  // epoch + head is 16-byte aligned: two 16-byte loads (else 8 + 16 + 8)
    bool m4;   // mask + head is 4-byte aligned: one load
    bool l4;   // late + head is 4-byte aligned: one store
};

struct TpTile {
    long long e[kTpPer];
    uint32_t m;  // the four mask bytes, swipe j in byte j
};

__device__ __forceinline__ TpTile tp_load(const TpArgs &A, const TpPlan &P, uint64_t g, bool ok) {
    TpTile t{};
    if (!ok) return t;
    const size_t i = size_t(P.head) + size_t(g) * kTpPer;
    const long long *p = reinterpret_cast<const long long *>(A.epoch) + i;
    if (P.e16) {
        const tp_ll2 a = *reinterpret_cast<const tp_ll2 *>(p);
        const tp_ll2 b = *reinterpret_cast<const tp_ll2 *>(p + 2);
        t.e[0] = a.x, t.e[1] = a.y, t.e[2] = b.x, t.e[3] = b.y;
    } else {  // an odd first element: the middle pair is the aligned one
        const tp_ll2 a = *reinterpret_cast<const tp_ll2 *>(p + 1);
        t.e[0] = p[0], t.e[1] = a.x, t.e[2] = a.y, t.e[3] = p[3];
    }
    if (A.mask) {
        const uint8_t *m = A.mask + i;
        if (P.m4)
            t.m = *reinterpret_cast<const uint32_t *>(m);
        else
            t.m = uint32_t(m[0]) | uint32_t(m[1]) << 8 | uint32_t(m[2]) << 16 | uint32_t(m[3]) << 24;
    }
    return t;
}

// tab[bin[j]] += 1 for every swipe j of every lane that is on[j].  Called by
// whole wavefronts.
template <int kForm>
__device__ __forceinline__ void tp_bump(uint32_t *tab, const uint32_t (&bin)[kTpPer], const bool (&on)[kTpPer]) {
    if (kForm == 0) {
        const uint32_t b = uint32_t(__builtin_amdgcn_readfirstlane(int(bin[0])));
        bool same = true;
#pragma unroll
        for (int j = 0; j < kTpPer; j++) same = same && bin[j] == b;
        if (__all(same)) {  // one bin for the wavefront's tile: a lane past the batch holds epoch 0's
            uint32_t cnt = 0;
#pragma unroll
            for (int j = 0; j < kTpPer; j++) cnt += uint32_t(__popcll(__ballot(on[j])));
            if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&tab[b], cnt);
            return;
        }
    }
#pragma unroll
    for (int j = 0; j < kTpPer; j++)
        if (on[j]) atomicAdd(&tab[bin[j]], 1u);
}

template <int kForm>
__global__ void __launch_bounds__(kTpBlock) k_tp_add(const TpArgs A, const TpPlan P) {
    __shared__ uint32_t tab[kTpBins];
    if (threadIdx.x < kTpBins) tab[threadIdx.x] = 0;
    __syncthreads();
    // the scalar head and tail, by the first workgroup
    if (blockIdx.x == 0) {
        const uint32_t body_end = P.head + P.ngroups * kTpPer;
        if (threadIdx.x < P.head + (A.n - body_end)) {
            const uint32_t i = threadIdx.x < P.head ? threadIdx.x : body_end + (threadIdx.x - P.head);
            const TpTime t = tp_time(A.epoch[i]);
            if (A.late) A.late[i] = t.sod >= A.late_from ? 1 : 0;
            if (!A.mask || A.mask[i] == A.want) atomicAdd(&tab[tp_bin(t)], 1u);
        }
    }
    // the groups of four: grid-stride over tiles, the next tile's loads in
    // flight while this one is binned
    const uint64_t stride = uint64_t(gridDim.x) * kTpBlock;
    uint64_t g = uint64_t(blockIdx.x) * kTpBlock + threadIdx.x;
    TpTile cur = tp_load(A, P, g, g < P.ngroups);
    for (uint64_t g0 = uint64_t(blockIdx.x) * kTpBlock; g0 < P.ngroups; g0 += stride, g += stride) {
        const bool ok = g < P.ngroups;
        const TpTile nxt = tp_load(A, P, g + stride, g + stride < P.ngroups);
        uint32_t bin[kTpPer], late = 0;
#pragma unroll
        for (int j = 0; j < kTpPer; j++) {
            const TpTime t = tp_time(cur.e[j]);
            bin[j] = tp_bin(t);
            late |= uint32_t(t.sod >= A.late_from) << (8 * j);
        }
        if (ok && A.late) {
            uint8_t *l = A.late + size_t(P.head) + size_t(g) * kTpPer;
            if (P.l4) {
                *reinterpret_cast<uint32_t *>(l) = late;
            } else {
#pragma unroll
                for (int j = 0; j < kTpPer; j++) l[j] = uint8_t(late >> (8 * j));
            }
        }
        bool on[kTpPer];
#pragma unroll
        for (int j = 0; j < kTpPer; j++) on[j] = ok && (!A.mask || ((cur.m >> (8 * j)) & 0xffu) == A.want);
        tp_bump<kForm>(tab, bin, on);
        cur = nxt;
    }
    __syncthreads();
    if (threadIdx.x < kTpBins) {
        const uint32_t v = tab[threadIdx.x];
        if (v) atomicAdd(A.counts + threadIdx.x, (unsigned long long)v);
    }
}

}  // namespace

hipError_t launch_tp_add(const TpArgs &A, int form, unsigned grid, hipStream_t st) {
    if (A.n == 0) return hipSuccess;
    const uintptr_t e = reinterpret_cast<uintptr_t>(A.epoch), m = reinterpret_cast<uintptr_t>(A.mask),
                    l = reinterpret_cast<uintptr_t>(A.late);
    if (e & 7) return hipErrorInvalidValue;
    TpPlan P{};
    P.head = A.mask ? uint32_t(-m & 3) : A.late ? uint32_t(-l & 3) : uint32_t((e >> 3) & 1);
    if (P.head > A.n) P.head = A.n;
    P.ngroups = (A.n - P.head) / kTpPer;
    P.e16 = ((e + 8 * uintptr_t(P.head)) & 15) == 0;
    P.m4 = A.mask && ((m + P.head) & 3) == 0;
    P.l4 = A.late && ((l + P.head) & 3) == 0;
    const uint64_t tiles = (uint64_t(P.ngroups) + kTpBlock - 1) / kTpBlock;
    if (grid > kTpMaxGrid) grid = kTpMaxGrid;
    if (grid > tiles) grid = unsigned(tiles);
    if (grid == 0) grid = 1;
    if (form == 1)
        hipLaunchKernelGGL(k_tp_add<1>, dim3(grid), dim3(kTpBlock), 0, st, A, P);
    else
        hipLaunchKernelGGL(k_tp_add<0>, dim3(grid), dim3(kTpBlock), 0, st, A, P);
    return hipGetLastError();
}

}  // namespace ske
