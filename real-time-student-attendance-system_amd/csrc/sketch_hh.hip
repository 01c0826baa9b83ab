// sketch_hh.hip -- heavy-hitter sets beside a Count-Min Sketch table (DESIGN.md
// "Heavy hitters"): the classic Count-Min construction -- keep the ids whose
// estimate crossed a threshold, read their estimates back when asked.
//
//   k_hh_track  per item of a batch: est = the row minimum of its cells (the
//               arithmetic of the add, sketch_cms_dev.h); est >= threshold:
//               hh_insert.  Two forms, as the add has: the table copied into
//               LDS by every workgroup and read there, or read from memory.
//   k_hh_list   one thread per slot: an occupied slot recomputes its estimate
//               from the stored words; those that pass are appended to the
//               output through one counter add per wavefront.
//   k_hh_export every member into caller-owned device arrays (no table), and
//   k_hh_merge  such arrays into a set: the union of sets across contexts.
//
// The set is an insert-only open-addressing table.  A slot is a claim word (the
// id's 64-bit digest, 0 = empty), 16 id bytes as two words, and the length.
#include "sketch_cms_dev.h"

namespace ske {
namespace {

constexpr int kHhLdsBlock = 1024;  // one workgroup per CU owns the CU's LDS
constexpr int kHhBlock = 256;

// The id joins the set unless it is there already.  Linear probing from
// hh_start: a slot that holds the digest ends the walk, an empty slot is
// claimed by a 64-bit compare-and-swap, any other slot is passed.
//
// No id lands twice, whatever the interleaving: a claim word changes once, from
// 0 to a digest, and never again (nothing is removed).  So a plain load returns
// either the slot's final value or a stale 0, and a stale 0 only sends the
// thread to the compare-and-swap, which answers with the true value.  The
// thread that claimed digest D at the j-th slot of D's path saw every earlier
// slot of the path hold another digest; those slots keep it, so every later
// walk for D passes them too and ends at the j-th slot -- on D (by the load, or
// as the compare-and-swap's answer) -- before it meets any empty slot behind.
// Two walks for D that race for the same empty slot are ordered by the
// compare-and-swap: one claims, the other is answered D.
//
// No thread waits for another: the winner alone writes the id words and the
// length, and nobody reads them in this launch (readers are later kernels on
// the stream), so there is nothing to wait for -- no spin, no sleep.  A hot id
// costs its first insert one atomic; every later occurrence ends at the plain
// load.  The walk is bounded by kHhMaxProbes, new claims by S.limit (read
// before the claim: claims racing at that moment may pass it, the capacity
// never, since each claim takes an empty slot); either bound drops the id and
// sets the sticky overflow word.
__device__ __forceinline__ void hh_insert(const HhSet &S, const Item &it) {
    const unsigned long long d = hh_digest(it.w0, it.w1, it.len);
    uint32_t slot = uint32_t(d) & S.mask;
    for (uint32_t p = 0; p < kHhMaxProbes; p++, slot = (slot + 1) & S.mask) {
        unsigned long long cur = S.claim[slot];
        if (cur == d) return;
        if (cur != 0) continue;
        if (__hip_atomic_load(S.used, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= S.limit) break;
        cur = atomicCAS(S.claim + slot, 0ull, d);
        if (cur == 0) {
            S.ids[2 * uint64_t(slot)] = it.w0;
            S.ids[2 * uint64_t(slot) + 1] = it.w1;
            S.len[slot] = it.len;
            atomicAdd(S.used, 1u);
            return;
        }
        if (cur == d) return;
    }
    atomicOr(S.overflow, 1u);
}

// is item i looked at
__device__ __forceinline__ bool hh_takes(const CmsItems &I, uint32_t i) { return !I.mask || I.mask[i] == I.want; }

// LDS form: the workgroup's copy of the table (reads only, no LDS atomics)
__global__ void __launch_bounds__(kHhLdsBlock) k_hh_track_lds(const CmsTable T, const CmsItems I, const HhSet S,
                                                               uint32_t threshold, unsigned int *toolong) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];
    // 16 bytes a load; the table's allocation is padded to the next 16 bytes
    const uint4 *src = reinterpret_cast<const uint4 *>(T.cells);
    uint4 *dst = reinterpret_cast<uint4 *>(tab);
    for (uint32_t v = threadIdx.x; v < (T.ncells + 3) / 4; v += kHhLdsBlock) dst[v] = src[v];
    __syncthreads();
    const uint64_t stride = uint64_t(gridDim.x) * kHhLdsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kHhLdsBlock + threadIdx.x; i < I.n; i += stride) {
        if (!hh_takes(I, uint32_t(i))) continue;
        const Item it = cms_item(I, uint32_t(i));
        if (it.len > 16) {
            if (toolong) atomicOr(toolong, 1u);
            continue;
        }
        uint32_t mn = 0xffffffffu;
        for (uint32_t r = 0; r < T.depth; r++) mn = umin32(mn, tab[cms_cell(T, it, r)]);
        if (mn >= threshold) hh_insert(S, it);
    }
}

// memory form
__global__ void __launch_bounds__(kHhBlock) k_hh_track_global(const CmsTable T, const CmsItems I, const HhSet S,
                                                               uint32_t threshold, unsigned int *toolong) {
    const uint64_t stride = uint64_t(gridDim.x) * kHhBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kHhBlock + threadIdx.x; i < I.n; i += stride) {
        if (!hh_takes(I, uint32_t(i))) continue;
        const Item it = cms_item(I, uint32_t(i));
        if (it.len > 16) {
            if (toolong) atomicOr(toolong, 1u);
            continue;
        }
        uint32_t mn = 0xffffffffu;
        for (uint32_t r = 0; r < T.depth; r++) mn = umin32(mn, T.cells[cms_cell(T, it, r)]);
        if (mn >= threshold) hh_insert(S, it);
    }
}

// The grid covers the slots exactly (the capacity is a multiple of the block),
// so every lane of every wavefront reaches the append.
__global__ void __launch_bounds__(kHhBlock) k_hh_list(const CmsTable T, const HhSet S, uint32_t threshold,
                                                       uint32_t cap, uint64_t *out_ids, uint32_t *out_len,
                                                       uint32_t *out_est, unsigned int *out_n) {
    const uint32_t slot = blockIdx.x * kHhBlock + threadIdx.x;
    Item it{};
    uint32_t est = 0;
    bool pass = false;
    if (S.claim[slot] != 0) {
        it.w0 = S.ids[2 * uint64_t(slot)];
        it.w1 = S.ids[2 * uint64_t(slot) + 1];
        it.len = S.len[slot];
        est = 0xffffffffu;
        for (uint32_t r = 0; r < T.depth; r++) est = umin32(est, T.cells[cms_cell(T, it, r)]);
        pass = est >= threshold;
    }
    const uint32_t at = wave_append(pass, out_n);
    if (at >= cap) return;  // also the lanes that do not pass
    out_ids[2 * uint64_t(at)] = it.w0;
    out_ids[2 * uint64_t(at) + 1] = it.w1;
    out_len[at] = it.len;
    out_est[at] = est;
}

// k_hh_list without a table: every member, unordered (the whole set on its way
// to another context).  The same grid, the same append.
__global__ void __launch_bounds__(kHhBlock) k_hh_export(const HhSet S, uint32_t cap, uint64_t *out_ids,
                                                         uint32_t *out_len, unsigned int *out_n) {
    const uint32_t slot = blockIdx.x * kHhBlock + threadIdx.x;
    const bool pass = S.claim[slot] != 0;
    const uint32_t at = wave_append(pass, out_n);
    if (at >= cap) return;  // also the lanes that do not pass
    out_ids[2 * uint64_t(at)] = S.ids[2 * uint64_t(slot)];
    out_ids[2 * uint64_t(at) + 1] = S.ids[2 * uint64_t(slot) + 1];
    out_len[at] = S.len[slot];
}

// Another set's export joins S: hh_insert per entry, no threshold and no table.
// The bytes behind an entry's length are masked, not trusted -- they take part
// in the digest.  A length over 16 is skipped and is a refused insert.
__global__ void __launch_bounds__(kHhBlock) k_hh_merge(const HhSet S, const uint64_t *ids, const uint32_t *len,
                                                        uint32_t n, uint32_t foreign_overflow) {
    if (foreign_overflow && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(S.overflow, 1u);
    const uint64_t stride = uint64_t(gridDim.x) * kHhBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kHhBlock + threadIdx.x; i < n; i += stride) {
        Item it{};
        it.len = len[i];
        if (it.len > 16) {
            atomicOr(S.overflow, 1u);
            continue;
        }
        it.w0 = ids[2 * i];
        it.w1 = ids[2 * i + 1];
        if (it.len < 8) it.w0 = it.len ? it.w0 & ((uint64_t(1) << (it.len * 8)) - 1) : 0;
        if (it.len <= 8)
            it.w1 = 0;
        else if (it.len < 16)
            it.w1 &= (uint64_t(1) << ((it.len - 8) * 8)) - 1;
        hh_insert(S, it);
    }
}

}  // namespace

hipError_t hh_setup() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hh_track_lds),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kCmsLdsMaxBytes);
}

hipError_t launch_hh_track(const CmsTable &T, const CmsItems &I, const HhSet &S, uint32_t threshold, bool lds,
                           unsigned int *toolong, int cus, hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    if (lds) {
        if (T.ncells > kCmsLdsCells) return hipErrorInvalidValue;
        const unsigned grid = grid_for(I.n, kHhLdsBlock, unsigned(cus));
        const size_t lds_bytes = (size_t(T.ncells) * 4 + 15) & ~size_t(15);
        hipLaunchKernelGGL(k_hh_track_lds, dim3(grid), dim3(kHhLdsBlock), lds_bytes, st, T, I, S, threshold, toolong);
    } else {
        hipLaunchKernelGGL(k_hh_track_global, dim3(grid_for(I.n, kHhBlock, unsigned(cus) * 8)), dim3(kHhBlock), 0, st,
                           T, I, S, threshold, toolong);
    }
    return hipGetLastError();
}

hipError_t launch_hh_list(const CmsTable &T, const HhSet &S, uint32_t threshold, uint32_t cap, uint64_t *out_ids,
                          uint32_t *out_len, uint32_t *out_est, unsigned int *out_n, hipStream_t st) {
    const uint32_t slots = S.mask + 1;
    if (slots % kHhBlock) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hh_list, dim3(slots / kHhBlock), dim3(kHhBlock), 0, st, T, S, threshold, cap, out_ids,
                       out_len, out_est, out_n);
    return hipGetLastError();
}

hipError_t launch_hh_export(const HhSet &S, uint32_t cap, uint64_t *out_ids, uint32_t *out_len, unsigned int *out_n,
                            hipStream_t st) {
    const uint32_t slots = S.mask + 1;
    if (slots % kHhBlock) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hh_export, dim3(slots / kHhBlock), dim3(kHhBlock), 0, st, S, cap, out_ids, out_len, out_n);
    return hipGetLastError();
}

hipError_t launch_hh_merge(const HhSet &S, const uint64_t *ids, const uint32_t *len, uint32_t n,
                           uint32_t foreign_overflow, int cus, hipStream_t st) {
    if (n == 0 && !foreign_overflow) return hipSuccess;
    const unsigned grid = grid_for(n, kHhBlock, unsigned(cus) * 8);  // n == 0: the one workgroup sets the word
    hipLaunchKernelGGL(k_hh_merge, dim3(grid), dim3(kHhBlock), 0, st, S, ids, len, n, foreign_overflow);
    return hipGetLastError();
}

}  // namespace ske
