// sketch_seen.hip -- seen-row sets (DESIGN.md "Seen rows"): an exact, insert-only
// set of 128-bit row keys whose add answers, per item, "first sighting or
// repeat", so the counters beside the swipe path count a redelivered row once.
//
//   k_seen_fold     folds one column of a batch into the batch's keys (16-byte
//                   key loads and stores; the column through load_item)
//   k_seen_walk     per item the mask lets through: the walk that finds or
//                   claims the key's slot, then the stamp
//   k_seen_resolve  per item: its answer from its slot's stamp; the counts
//   k_seen_end      one thread: the call counter's bump
//   k_seen_test     the walk without claims: is the key in the set
//
// A slot is three 64-bit words in three arrays: w0 and w1, the key's two words
// (0 = not yet claimed; a key word 0 is read as 1), and stamp, (call << 32) |
// item of the key's first sighting (all ones = none yet).
//
// The walk.  Linear probing from the low bits of k0.  At a slot: w0 is loaded;
// a 0 sends the thread to atomicCAS(w0, 0, k0).  When the slot's w0 is k0 the
// same is done with w1 and k1.  The slot is the key's when w1 is k1; any other
// outcome passes on.  Each word changes once, from 0 to a key word, and never
// again (nothing is removed), so a plain load returns the word's final value or
// a stale 0, and a stale 0 only leads to the compare-and-swap, which answers
// with the truth.  Every walk for one key therefore takes the same decision at
// every slot it looks at, whatever the interleaving: a slot whose w0 holds
// another word is passed by all of them; a slot whose w0 is k0 is decided by w1
// alone, and w1 is final once any walk has looked at it (the look is the
// compare-and-swap or a load of a non-zero word).  So all walks for a key end
// at the slot the first of them took, before any empty slot behind it.  Two
// keys with equal k0 may race for one slot's w1: the compare-and-swap orders
// them, the loser passes on.  No thread waits for another: a slot whose w0 is
// claimed and whose w1 is still 0 is not waited for, it is completed by
// whoever gets there (its claimer or another key with the same k0).
//
// Visibility across XCDs: w0, w1 and stamp are changed only by device-scope
// atomics (atomicCAS, atomicMin on global memory), which act at the memory side
// of the per-XCD L2s.  The plain loads in front of them may be served from a
// CU's L1 or an XCD's L2 and be stale; the only stale values possible are a 0
// (claim words) and a larger stamp, and both only send the thread to the atomic,
// which is then decisive.  k_seen_resolve is a later launch on the same stream
// and reads the stamps the walk's launch left.
//
// The stamp.  atomicMin(stamp[slot], (call << 32) | i).  A member from an
// earlier call holds a smaller stamp (call numbers grow), so it never reads as
// first; within a call the lowest index wins.  The stamp is read first and the
// atomic skipped when it is below the item's already; a wavefront whose items
// all ended at one slot sends its lowest item alone.  Items are answered
// FIRST exactly when their slot's stamp is their own: one item per new key, the
// lowest -- the same from run to run.
//
// Bounds.  A walk looks at kSeenMaxProbes slots, new claims stop at `limit`
// (`used` is read once per wavefront and turn, before its claims, and grows by
// a wavefront's claims at once: claims racing at that moment may pass the limit,
// the capacity never, since each claim takes an empty slot).  An item that finds no
// slot is answered FIRST and counted in `unplaced`: it fails open -- a count is
// never lost, and a REPEAT is never false, because REPEAT needs a slot that
// holds the item's very key with another item's stamp.
#include "sketch_common.h"
#include "sketch_internal.h"

namespace ske {
namespace {

constexpr int kSeenBlock = 256;

__device__ __forceinline__ SeenKey seen_load_key(const uint64_t *keys, uint32_t i) {
    const ulonglong2 v = reinterpret_cast<const ulonglong2 *>(keys)[i];
    return SeenKey{v.x, v.y};
}
__device__ __forceinline__ void seen_store_key(uint64_t *keys, uint32_t i, const SeenKey &k) {
    reinterpret_cast<ulonglong2 *>(keys)[i] = make_ulonglong2(k.k0, k.k1);
}

template <int kKind>
__global__ void __launch_bounds__(kSeenBlock) k_seen_fold(uint64_t *keys, const SeenCol C, int begin) {
    const uint64_t stride = uint64_t(gridDim.x) * kSeenBlock;
    for (uint64_t i64 = uint64_t(blockIdx.x) * kSeenBlock + threadIdx.x; i64 < C.n; i64 += stride) {
        const uint32_t i = uint32_t(i64);
        const SeenKey k = begin ? seen_begin() : seen_load_key(keys, i);
        SeenKey r;
        if (kKind == 3) {
            r = seen_fold_epoch(k, C.epoch[i], C.granularity);
        } else {
            uint32_t b, e;
            if (kKind == 0) {
                b = C.offs[i];
                e = C.offs[i + 1];
            } else if (kKind == 1) {
                b = 0;
                e = C.fixed_w;
            } else {
                const uint32_t j = C.at ? C.at[i] : i;
                b = C.offs[j];
                e = b + C.len[j];
            }
            const uint8_t *base = kKind == 1 ? C.bytes + uint64_t(i) * C.fixed_w : C.bytes;
            const Item it = load_item(base, b, e);
            r = SeenKey{murmur_item(it, k.k0), murmur_item(it, k.k1)};
        }
        seen_store_key(keys, i, r);
    }
}

// The slot of key (k0, k1), found or claimed; kSeenNoSlot when the walk's bounds
// end it.  room: the wavefront read `used` below the limit, new claims are allowed.
// claimed: set when this walk claimed a slot that `used` does not count yet (the
// wavefront adds those up); a walk that claims again -- it lost its first slot's
// w1 to another key with the same k0 -- counts the further claims itself.
__device__ __forceinline__ uint32_t seen_walk(const SeenTab &T, unsigned long long k0, unsigned long long k1,
                                              bool room, bool &claimed) {
    uint32_t slot = uint32_t(k0) & T.mask;
    for (uint32_t p = 0; p < kSeenMaxProbes; p++, slot = (slot + 1) & T.mask) {
        unsigned long long c0 = T.w0[slot];
        if (c0 == 0) {
            if (!room) {
                // no new claim: the walk goes on only over what is claimed for sure (the 0 may be stale)
                c0 = __hip_atomic_load(T.w0 + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (c0 == 0) break;
            } else {
                c0 = atomicCAS(T.w0 + slot, 0ull, k0);
                if (c0 == 0) {
                    if (claimed) atomicAdd(&T.head->used, 1u);
                    claimed = true;
                    c0 = k0;
                }
            }
        }
        if (c0 != k0) continue;
        unsigned long long c1 = T.w1[slot];
        if (c1 == 0) {
            c1 = atomicCAS(T.w1 + slot, 0ull, k1);
            if (c1 == 0) c1 = k1;
        }
        if (c1 == k1) return slot;
    }
    return kSeenNoSlot;
}

// Whole wavefronts walk the loop together (its bound is the wavefront's first
// item), so the ballots see every lane.  Per turn a wavefront reads `used` once
// for its 64 items and adds its claims to it once; when all its items carry one
// key (a hot row) one lane walks for all.
__global__ void __launch_bounds__(kSeenBlock) k_seen_walk(const SeenTab T, const uint64_t *keys, uint32_t n,
                                                           const uint8_t *mask, uint32_t want, uint32_t *slot_out) {
    const unsigned long long call = T.head->calls;  // left by the previous add's last kernel
    const bool open = call < kSeenLastCall;         // else: every item goes unplaced
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t stride = uint64_t(gridDim.x) * kSeenBlock;
    uint64_t i = uint64_t(blockIdx.x) * kSeenBlock + threadIdx.x;
    for (uint64_t i0 = i - lane; i0 < n; i0 += stride, i += stride) {
        const bool in = i < n;
        const bool takes = in && (!mask || mask[i] == want);
        const bool walks = takes && open;
        unsigned long long k0 = 0, k1 = 0;
        if (walks) {
            const SeenKey k = seen_load_key(keys, uint32_t(i));
            k0 = seen_word(k.k0);
            k1 = seen_word(k.k1);
        }
        uint32_t slot = kSeenNoSlot;
        const unsigned long long walkers = __ballot(walks);
        if (walkers) {
            const int lead = __ffsll((long long)walkers) - 1;
            uint32_t used = 0;
            if (lane == uint32_t(lead))
                used = __hip_atomic_load(&T.head->used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const bool room = __shfl(used, lead, 64) < T.limit;
            const unsigned long long f0 = __shfl(k0, lead, 64), f1 = __shfl(k1, lead, 64);
            const bool same = __ballot(walks && (k0 != f0 || k1 != f1)) == 0;
            bool claimed = false;
            if (same) {
                if (lane == uint32_t(lead)) slot = seen_walk(T, k0, k1, room, claimed);
                slot = __shfl(slot, lead, 64);
                if (!walks) slot = kSeenNoSlot;
            } else if (walks) {
                slot = seen_walk(T, k0, k1, room, claimed);
            }
            const unsigned long long claims = __ballot(claimed);
            if (claims && lane == uint32_t(__ffsll((long long)claims) - 1))
                atomicAdd(&T.head->used, uint32_t(__popcll(claims)));
        }
        const bool placed = slot != kSeenNoSlot;
        const unsigned long long votes = __ballot(placed);
        if (votes) {
            // the lanes' items ascend with the lane: the lowest placed lane is its slot's lowest item
            const int low = __ffsll((long long)votes) - 1;
            const uint32_t s0 = __shfl(slot, low, 64);
            const bool one = __ballot(placed && slot != s0) == 0;
            if (placed && (!one || lane == uint32_t(low))) {
                const unsigned long long mine = (call << 32) | i;
                if (__hip_atomic_load(T.stamp + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > mine)
                    atomicMin(T.stamp + slot, mine);
            }
        }
        if (in) slot_out[i] = takes ? slot : kSeenSkipSlot;
    }
}

__global__ void __launch_bounds__(kSeenBlock) k_seen_resolve(const SeenTab T, uint32_t n, const uint32_t *slot_in,
                                                              uint8_t *out) {
    __shared__ unsigned int s_looked, s_first, s_unplaced;
    if (threadIdx.x == 0) s_looked = 0, s_first = 0, s_unplaced = 0;
    __syncthreads();
    const unsigned long long call = T.head->calls;  // k_seen_end bumps it behind this launch
    const uint64_t stride = uint64_t(gridDim.x) * kSeenBlock;
    unsigned int looked = 0, first = 0, unplaced = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * kSeenBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t slot = slot_in[i];
        uint8_t r = kSeenSkipped;
        if (slot != kSeenSkipSlot) {
            looked++;
            if (slot == kSeenNoSlot) {
                unplaced++;
                r = kSeenFirst;
            } else {
                r = T.stamp[slot] == ((call << 32) | i) ? kSeenFirst : kSeenRepeat;
            }
            first += r == kSeenFirst;
        }
        out[i] = r;
    }
    // a block's share of one launch is below 2^32 items
    if (looked) atomicAdd(&s_looked, looked);
    if (first) atomicAdd(&s_first, first);
    if (unplaced) atomicAdd(&s_unplaced, unplaced);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_looked) atomicAdd(&T.head->looked_at, (unsigned long long)s_looked);
        if (s_first) atomicAdd(&T.head->first, (unsigned long long)s_first);
        if (s_unplaced) atomicAdd(&T.head->unplaced, (unsigned long long)s_unplaced);
    }
}

// The call counter lives in the set, not in a launch argument: a recorded graph
// that replays the add sees a new call each time.
__global__ void k_seen_end(const SeenTab T) {
    if (blockIdx.x || threadIdx.x) return;
    const unsigned long long call = T.head->calls;
    if (call < kSeenLastCall) T.head->calls = call + 1;
}

__global__ void __launch_bounds__(kSeenBlock) k_seen_test(const SeenTab T, const uint64_t *keys, uint32_t n,
                                                           uint8_t *present) {
    const uint64_t stride = uint64_t(gridDim.x) * kSeenBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kSeenBlock + threadIdx.x; i < n; i += stride) {
        const SeenKey k = seen_load_key(keys, uint32_t(i));
        const unsigned long long k0 = seen_word(k.k0), k1 = seen_word(k.k1);
        uint32_t slot = uint32_t(k0) & T.mask;
        uint8_t r = 0;
        for (uint32_t p = 0; p < kSeenMaxProbes; p++, slot = (slot + 1) & T.mask) {
            const unsigned long long c0 = T.w0[slot];
            if (c0 == 0) break;
            if (c0 == k0 && T.w1[slot] == k1) {
                r = 1;
                break;
            }
        }
        present[i] = r;
    }
}

// workgroups of a kernel over n items: the context's override, else eight per CU
unsigned grid_of(uint32_t n, unsigned grid, int cus) {
    return grid_for(n, kSeenBlock, grid, unsigned(cus) * 8, kSeenMaxGrid);
}

template <int kKind>
hipError_t seen_fold_kind(uint64_t *keys, const SeenCol &C, bool begin, unsigned grid, int cus, hipStream_t st) {
    hipLaunchKernelGGL(k_seen_fold<kKind>, dim3(grid_of(C.n, grid, cus)), dim3(kSeenBlock), 0, st, keys, C,
                       begin ? 1 : 0);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_seen_fold(uint64_t *keys, const SeenCol &C, bool begin, unsigned grid, int cus, hipStream_t st) {
    if (C.n == 0) return hipSuccess;
    switch (C.kind) {
    case 0: return seen_fold_kind<0>(keys, C, begin, grid, cus, st);
    case 1: return seen_fold_kind<1>(keys, C, begin, grid, cus, st);
    case 2: return seen_fold_kind<2>(keys, C, begin, grid, cus, st);
    case 3: return seen_fold_kind<3>(keys, C, begin, grid, cus, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_seen_add(const SeenTab &T, const uint64_t *keys, uint32_t n, const uint8_t *mask, uint32_t want,
                           uint32_t *slot, uint8_t *out, unsigned grid, int cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const unsigned g = grid_of(n, grid, cus);
    hipLaunchKernelGGL(k_seen_walk, dim3(g), dim3(kSeenBlock), 0, st, T, keys, n, mask, want, slot);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_seen_resolve, dim3(g), dim3(kSeenBlock), 0, st, T, n, slot, out);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_seen_end, dim3(1), dim3(64), 0, st, T);
    return hipGetLastError();
}

hipError_t launch_seen_test(const SeenTab &T, const uint64_t *keys, uint32_t n, uint8_t *present, unsigned grid,
                            int cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seen_test, dim3(grid_of(n, grid, cus)), dim3(kSeenBlock), 0, st, T, keys, n, present);
    return hipGetLastError();
}

}  // namespace ske
