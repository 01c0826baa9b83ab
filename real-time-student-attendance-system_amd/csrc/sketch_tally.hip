// sketch_tally.hip -- tallies (DESIGN.md "Lecture tallies"): exact event counts
// per key, the group-by-count of a string column.  A key is a byte string of at
// most kTallyKeyBytes; every item of a batch adds 1 to its key's `events` and,
// when its mask byte is 1, 1 to its key's `valid`.
//
//   k_tally_add    the batch's keys from one of four sources (TallyItems), in
//                  two forms: 0 sums into a hash table in the workgroup's LDS
//                  first and flushes it, 1 is one insert-or-add in memory per item
//   k_tally_query  the counters of each key of a batch
//   k_tally_list   one thread per slot: the entries with events >= a minimum,
//                  appended to the output through one counter add per wavefront
//
// The table is an insert-only open-addressing table, structure of arrays.  A
// slot is a claim word (the key's 64-bit digest, 0 = empty), the key as four
// zero-padded words, its length, and two u64 counters.
#include "sketch_common.h"
#include "sketch_internal.h"

namespace ske {
namespace {

constexpr int kTallyLdsBlock = 1024;  // form 0: one workgroup per CU owns the CU's LDS
constexpr int kTallyBlock = 256;
constexpr uint32_t kTallyLdsProbes = 8;  // LDS slots one item looks at before it goes to memory

struct TallyKey {
    uint64_t w[kTallyKeyWords];
    uint32_t len;
};

// key bytes [p, p + len), len <= kTallyKeyBytes: only the aligned 8-byte words
// that hold a byte of the key are read (load_le)
__device__ __forceinline__ void tally_words(const uint8_t *p, uint32_t len, uint64_t (&w)[kTallyKeyWords]) {
#pragma unroll
    for (uint32_t j = 0; j < kTallyKeyWords; j++) {
        const uint32_t at = 8 * j;
        w[j] = len > at ? load_le(p + at, len - at < 8 ? len - at : 8) : 0;
    }
}

// Item i of the batch: is it taken, its key (len > kTallyKeyBytes: no words),
// and what it counts.
template <int kKind>
struct TallySrc {
    const TallyItems &I;
    __device__ __forceinline__ bool takes(uint32_t i) const {
        return kKind != 2 || !I.status || I.status[i] == 0;
    }
    __device__ __forceinline__ TallyKey key(uint32_t i) const {
        TallyKey k{};
        const uint8_t *p;
        if (kKind == 0) {
            const uint32_t b = I.offs[i], e = I.offs[i + 1];
            p = I.bytes + b;
            k.len = e - b;
        } else if (kKind == 1) {
            p = I.bytes + uint64_t(i) * I.fixed_w;
            k.len = I.fixed_w;
        } else if (kKind == 2) {
            p = I.bytes + I.offs[i];
            k.len = I.len[i];
        } else {
            p = I.bytes + uint64_t(i) * kTallyKeyBytes;
            k.len = I.len[i];
        }
        if (k.len <= kTallyKeyBytes) tally_words(p, k.len, k.w);
        return k;
    }
    __device__ __forceinline__ unsigned long long events(uint32_t i) const { return kKind == 3 ? I.ev[i] : 1ull; }
    __device__ __forceinline__ unsigned long long valid(uint32_t i) const {
        if (kKind == 3) return I.va[i];
        return I.mask && I.mask[i] == 1 ? 1ull : 0ull;
    }
};

__device__ __forceinline__ void tally_refuse(const TallyTab &T, unsigned long long ev, unsigned long long va) {
    if (ev) atomicAdd(T.dropped_events, ev);
    if (va) atomicAdd(T.dropped_valid, va);
    atomicOr(T.overflow, 1u);
}

// Insert-or-add in memory: the entry of digest d counts ev / va more.  The
// claim protocol is hh_insert's (sketch_hh.hip), and its argument holds
// unchanged: a claim word changes once, from 0 to a digest, so a plain load
// returns the final value or a stale 0, and a stale 0 only leads to the
// compare-and-swap, which answers with the truth; every walk for d ends at the
// slot the first claim for d took.  What the tally adds:
//   * the counters are words of their own, zero since init, so an adder never
//     waits for the claim's winner: it adds as soon as the claim word reads d,
//     whether or not the winner has written the key words yet (nobody reads
//     those in this launch);
//   * `rep` is an item of the batch that carries this key: only the winner of a
//     new claim loads its bytes again, to write the key words;
//   * a refused item (the load bound, read before the claim, or the probe walk)
//     goes to the dropped totals, so sum(events) + dropped_events == taken
//     holds whatever was refused.  One thread may be refused a key that another
//     claims at that moment (the bound is read before the claim): once the
//     overflow word is set a listed count is a lower bound.
template <class Src>
__device__ __forceinline__ void tally_add_global(const TallyTab &T, unsigned long long d, unsigned long long ev,
                                                 unsigned long long va, const Src &S, uint32_t rep) {
    uint32_t slot = uint32_t(d) & T.mask;
    for (uint32_t p = 0; p < kTallyMaxProbes; p++, slot = (slot + 1) & T.mask) {
        unsigned long long cur = T.claim[slot];
        if (cur == 0) {
            if (__hip_atomic_load(T.used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= T.limit) break;
            cur = atomicCAS(T.claim + slot, 0ull, d);
            if (cur == 0) {
                const TallyKey k = S.key(rep);
#pragma unroll
                for (uint32_t j = 0; j < kTallyKeyWords; j++) T.keys[kTallyKeyWords * uint64_t(slot) + j] = k.w[j];
                T.len[slot] = k.len;
                atomicAdd(T.used, 1u);
                cur = d;
            }
        }
        if (cur == d) {
            if (ev) atomicAdd(T.events + slot, ev);
            if (va) atomicAdd(T.valid + slot, va);
            return;
        }
    }
    tally_refuse(T, ev, va);
}

// one item, decoded
struct TallyOne {
    unsigned long long d;
    uint32_t va;
    bool on;    // taken and its key fits: it is grouped
    bool seen;  // taken
};

template <int kKind>
__device__ __forceinline__ TallyOne tally_load(const TallySrc<kKind> &S, uint64_t i, uint32_t n) {
    TallyOne o{};
    if (i >= n || !S.takes(uint32_t(i))) return o;
    o.seen = true;
    o.va = uint32_t(S.valid(uint32_t(i)));
    const TallyKey k = S.key(uint32_t(i));
    if (k.len > kTallyKeyBytes) return o;
    o.on = true;
    o.d = tally_digest(k.w, k.len);
    return o;
}

// The workgroup's LDS table: digest (0 = empty), u32 events, u32 valid and the
// batch index of one item that carries the key.  A batch has fewer than
// 2^32 - 1 items, so no LDS counter wraps.
struct TallyLds {
    unsigned long long *dig;
    uint32_t *ev, *va, *rep;
    uint32_t mask;
};

// false: the walk found no place, the item goes to memory
__device__ __forceinline__ bool tally_add_lds(const TallyLds &L, unsigned long long d, uint32_t ev, uint32_t va,
                                              uint32_t rep) {
    uint32_t slot = uint32_t(d >> 32) & L.mask;  // not the bits the table in memory starts from
    for (uint32_t p = 0; p < kTallyLdsProbes; p++, slot = (slot + 1) & L.mask) {
        unsigned long long cur = __hip_atomic_load(L.dig + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == 0) {
            cur = atomicCAS(L.dig + slot, 0ull, d);
            if (cur == 0) {
                L.rep[slot] = rep;  // read after the barrier before the flush
                cur = d;
            }
        }
        if (cur == d) {
            atomicAdd(L.ev + slot, ev);
            if (va) atomicAdd(L.va + slot, va);
            return true;
        }
    }
    return false;
}

// Form 0.  Grid-stride over the batch, the next item's loads in flight while
// this one is counted; whole wavefronts walk the loop together, so the ballots
// see every lane.  When every grouped item of a wavefront's 64 holds one digest
// (a real batch comes from one or two lectures) one lane adds the popcounts.
template <int kKind>
__global__ void __launch_bounds__(kTallyLdsBlock) k_tally_add_lds(const TallyTab T, const TallyItems I,
                                                                   uint32_t lds_log2) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long tally_smem[];
    __shared__ uint32_t s_taken, s_long_ev, s_long_va;
    const uint32_t slots = 1u << lds_log2;
    TallyLds L;
    L.dig = tally_smem;
    L.ev = reinterpret_cast<uint32_t *>(tally_smem + slots);
    L.va = L.ev + slots;
    L.rep = L.va + slots;
    L.mask = slots - 1;
    for (uint32_t s = threadIdx.x; s < slots; s += kTallyLdsBlock) {
        L.dig[s] = 0;
        L.ev[s] = 0;
        L.va[s] = 0;
    }
    if (threadIdx.x == 0) s_taken = 0, s_long_ev = 0, s_long_va = 0;
    __syncthreads();
    const TallySrc<kKind> S{I};
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = uint64_t(gridDim.x) * kTallyLdsBlock;
    uint64_t i = uint64_t(blockIdx.x) * kTallyLdsBlock + threadIdx.x;
    uint32_t taken = 0, long_ev = 0, long_va = 0;
    TallyOne cur = tally_load(S, i, I.n);
    for (uint64_t i0 = uint64_t(blockIdx.x) * kTallyLdsBlock; i0 < I.n; i0 += stride, i += stride) {
        const TallyOne nxt = tally_load(S, i + stride, I.n);
        if (cur.seen) {
            taken++;
            if (!cur.on) long_ev++, long_va += cur.va;
        }
        const unsigned long long votes = __ballot(cur.on);
        if (votes) {
            const int first = __ffsll((long long)votes) - 1;
            const unsigned long long d0 = __shfl(cur.d, first, 64);
            const bool one = __ballot(cur.on && cur.d != d0) == 0;
            const unsigned long long vvotes = __ballot(cur.on && cur.va);
            if (one) {
                if (lane == uint32_t(first)) {
                    const uint32_t ev = uint32_t(__popcll(votes)), va = uint32_t(__popcll(vvotes));
                    if (!tally_add_lds(L, d0, ev, va, uint32_t(i))) tally_add_global(T, d0, ev, va, S, uint32_t(i));
                }
            } else if (cur.on) {
                if (!tally_add_lds(L, cur.d, 1u, cur.va, uint32_t(i)))
                    tally_add_global(T, cur.d, 1ull, cur.va, S, uint32_t(i));
            }
        }
        cur = nxt;
    }
    if (taken) atomicAdd(&s_taken, taken);
    if (long_ev) atomicAdd(&s_long_ev, long_ev);
    if (long_va) atomicAdd(&s_long_va, long_va);
    __syncthreads();
    // the flush: one insert-or-add in memory per occupied LDS slot
    for (uint32_t s = threadIdx.x; s < slots; s += kTallyLdsBlock) {
        const unsigned long long d = L.dig[s];
        if (d) tally_add_global(T, d, L.ev[s], L.va[s], S, L.rep[s]);
    }
    if (threadIdx.x == 0) {
        if (s_taken) atomicAdd(T.taken, (unsigned long long)s_taken);
        if (s_long_ev) {
            tally_refuse(T, s_long_ev, s_long_va);
            if (I.toolong) atomicOr(I.toolong, 1u);
        }
    }
}

// Form 1 (and a listing's import, kKind 3): one insert-or-add in memory per item.
template <int kKind>
__global__ void __launch_bounds__(kTallyBlock) k_tally_add_global(const TallyTab T, const TallyItems I) {
    __shared__ unsigned long long s_taken;
    if (threadIdx.x == 0) s_taken = 0;
    __syncthreads();
    const TallySrc<kKind> S{I};
    const uint64_t stride = uint64_t(gridDim.x) * kTallyBlock;
    unsigned long long taken = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * kTallyBlock + threadIdx.x; i < I.n; i += stride) {
        if (!S.takes(uint32_t(i))) continue;
        const unsigned long long ev = S.events(uint32_t(i)), va = S.valid(uint32_t(i));
        taken += ev;
        const TallyKey k = S.key(uint32_t(i));
        if (k.len > kTallyKeyBytes) {
            tally_refuse(T, ev, va);
            if (I.toolong) atomicOr(I.toolong, 1u);
            continue;
        }
        tally_add_global(T, tally_digest(k.w, k.len), ev, va, S, uint32_t(i));
    }
    if (taken) atomicAdd(&s_taken, taken);
    __syncthreads();
    if (threadIdx.x == 0 && s_taken) atomicAdd(T.taken, s_taken);
}

template <int kKind>
__global__ void __launch_bounds__(kTallyBlock) k_tally_query(const TallyTab T, const TallyItems I, uint64_t *ev,
                                                              uint64_t *va) {
    const TallySrc<kKind> S{I};
    const uint64_t stride = uint64_t(gridDim.x) * kTallyBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kTallyBlock + threadIdx.x; i < I.n; i += stride) {
        const TallyKey k = S.key(uint32_t(i));
        uint64_t e = 0, v = 0;
        if (k.len <= kTallyKeyBytes) {
            const unsigned long long d = tally_digest(k.w, k.len);
            uint32_t slot = uint32_t(d) & T.mask;
            for (uint32_t p = 0; p < kTallyMaxProbes; p++, slot = (slot + 1) & T.mask) {
                const unsigned long long cur = T.claim[slot];
                if (cur == 0) break;
                if (cur == d) {
                    e = T.events[slot];
                    v = T.valid[slot];
                    break;
                }
            }
        }
        ev[i] = e;
        va[i] = v;
    }
}

// The grid covers the slots exactly (the capacity is a multiple of the block),
// so every lane of every wavefront reaches the append.
__global__ void __launch_bounds__(kTallyBlock) k_tally_list(const TallyTab T, uint64_t min_events, uint32_t cap,
                                                             uint64_t *out_keys, uint32_t *out_len, uint64_t *out_ev,
                                                             uint64_t *out_va, unsigned int *out_n) {
    const uint32_t slot = blockIdx.x * kTallyBlock + threadIdx.x;
    uint64_t ev = 0;
    bool pass = false;
    if (T.claim[slot] != 0) {
        ev = T.events[slot];
        pass = ev >= min_events;
    }
    const uint32_t at = wave_append(pass, out_n);
    if (at >= cap) return;  // also the lanes that do not pass
#pragma unroll
    for (uint32_t j = 0; j < kTallyKeyWords; j++)
        out_keys[kTallyKeyWords * uint64_t(at) + j] = T.keys[kTallyKeyWords * uint64_t(slot) + j];
    out_len[at] = T.len[slot];
    out_ev[at] = ev;
    out_va[at] = T.valid[slot];
}

// the head of a tally that takes another tally's entries takes its refused
// counts too, so sum(events) + dropped_events == taken holds across the merge
__global__ void k_tally_head_add(const TallyTab T, unsigned long long dropped_events,
                                 unsigned long long dropped_valid, uint32_t overflow) {
    if (blockIdx.x || threadIdx.x) return;
    if (dropped_events) {
        atomicAdd(T.taken, dropped_events);
        atomicAdd(T.dropped_events, dropped_events);
    }
    if (dropped_valid) atomicAdd(T.dropped_valid, dropped_valid);
    if (overflow) atomicOr(T.overflow, 1u);
}

constexpr size_t tally_lds_bytes(int lds_log2) { return (size_t(1) << lds_log2) * 20; }

template <int kKind>
hipError_t tally_launch_kind(const TallyTab &T, const TallyItems &I, int form, unsigned grid, int lds_log2, int cus,
                             hipStream_t st) {
    if constexpr (kKind != 3) {  // a listing is imported through form 1 alone
        if (form == 0) {
            grid = grid_for(I.n, kTallyLdsBlock, grid, unsigned(cus), kTallyMaxGrid);
            hipLaunchKernelGGL(k_tally_add_lds<kKind>, dim3(grid), dim3(kTallyLdsBlock), tally_lds_bytes(lds_log2),
                               st, T, I, uint32_t(lds_log2));
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(k_tally_add_global<kKind>, dim3(grid_for(I.n, kTallyBlock, unsigned(cus) * 8)),
                       dim3(kTallyBlock), 0, st, T, I);
    return hipGetLastError();
}

}  // namespace

hipError_t tally_setup() {
    const int bytes = int(tally_lds_bytes(kTallyLdsMaxLog2));
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tally_add_lds<0>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tally_add_lds<1>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess)
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(&k_tally_add_lds<2>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    return e;
}

hipError_t launch_tally_add(const TallyTab &T, const TallyItems &I, int form, unsigned grid, int lds_log2, int cus,
                            hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    if (lds_log2 < kTallyLdsMinLog2 || lds_log2 > kTallyLdsMaxLog2) return hipErrorInvalidValue;
    switch (I.kind) {
    case 0: return tally_launch_kind<0>(T, I, form, grid, lds_log2, cus, st);
    case 1: return tally_launch_kind<1>(T, I, form, grid, lds_log2, cus, st);
    case 2: return tally_launch_kind<2>(T, I, form, grid, lds_log2, cus, st);
    case 3: return tally_launch_kind<3>(T, I, 1, grid, lds_log2, cus, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_tally_query(const TallyTab &T, const TallyItems &I, uint64_t *ev, uint64_t *va, int cus,
                              hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    if (I.kind != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tally_query<0>, dim3(grid_for(I.n, kTallyBlock, unsigned(cus) * 8)), dim3(kTallyBlock), 0, st,
                       T, I, ev, va);
    return hipGetLastError();
}

hipError_t launch_tally_list(const TallyTab &T, uint64_t min_events, uint32_t cap, uint64_t *out_keys,
                             uint32_t *out_len, uint64_t *out_ev, uint64_t *out_va, unsigned int *out_n,
                             hipStream_t st) {
    const uint32_t slots = T.mask + 1;
    if (slots % kTallyBlock) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tally_list, dim3(slots / kTallyBlock), dim3(kTallyBlock), 0, st, T, min_events, cap, out_keys,
                       out_len, out_ev, out_va, out_n);
    return hipGetLastError();
}

hipError_t launch_tally_head_add(const TallyTab &T, unsigned long long dropped_events,
                                 unsigned long long dropped_valid, uint32_t overflow, hipStream_t st) {
    if (!dropped_events && !dropped_valid && !overflow) return hipSuccess;
    hipLaunchKernelGGL(k_tally_head_add, dim3(1), dim3(64), 0, st, T, dropped_events, dropped_valid, overflow);
    return hipGetLastError();
}

}  // namespace ske
