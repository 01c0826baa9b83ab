// sketch_cms.hip -- Count-Min Sketch kernels (RedisBloom src/cms.c semantics,
// DESIGN.md "Count-Min Sketch"): the cell of an item in row i is
// MurmurHash2(item, len, seed = i) % width; an add raises every row's cell, a
// cell that would pass 2^32 - 1 stays there; a query is the row minimum.
//
// The bulk add is order-free: whatever the interleaving, a cell ends at
// min(true sum, 2^32 - 1).  Two forms:
//   LDS     each workgroup sums its share of the batch into a private table
//           in LDS (non-returning ds adds), then adds its non-zero cells to
//           the table in memory;
//   global  one atomic per (item, row).
// Every add to the table in memory is cms_sat_add below.
#include "sketch_cms_dev.h"

namespace ske {
namespace {

constexpr int kCmsLdsBlock = 1024;  // one workgroup per CU owns the CU's LDS
constexpr int kCmsBlock = 256;

// cell += v with the cell pinned at 2^32 - 1 once it would pass it, for any
// interleaving of such adds on the cell: an add that wraps is followed by its
// own pin (a max with 2^32 - 1), and an add that finds the pinned value wraps
// again (v >= 1) and pins again, so in the cell's modification order the last
// operation that changes it is a pin as soon as any add wrapped; when the true
// sum stays below 2^32 no add wraps and no pin happens.  Callers skip v == 0.
__device__ __forceinline__ void cms_sat_add(uint32_t *cell, uint32_t v) {
    const uint32_t old = atomicAdd(cell, v);
    if (old + v < old) atomicMax(cell, 0xffffffffu);
}

// does item i count, and by how much (0: skip it)
__device__ __forceinline__ uint32_t cms_incr(const CmsItems &I, uint32_t i) {
    if (I.mask && I.mask[i] != I.want) return 0;
    return I.incr ? I.incr[i] : 1u;
}

// the workgroup's increment sum into *count: one atomic per workgroup
__device__ __forceinline__ void cms_count(unsigned long long sum, unsigned long long *wsum,
                                          unsigned long long *count) {
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(wsum, sum);
    __syncthreads();
    if (threadIdx.x == 0 && *wsum) atomicAdd(count, *wsum);
}

// LDS form.  lds_max: the largest increment that may go through the private
// table -- (items one workgroup can meet) * lds_max < 2^32, so no LDS partial
// wraps; a larger increment (explicit increments only) goes to memory directly.
__global__ void __launch_bounds__(kCmsLdsBlock) k_cms_add_lds(const CmsTable T, const CmsItems I, uint32_t lds_max) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tab[];
    __shared__ unsigned long long wsum;
    for (uint32_t c = threadIdx.x; c < T.ncells; c += kCmsLdsBlock) tab[c] = 0;
    if (threadIdx.x == 0) wsum = 0;
    __syncthreads();
    unsigned long long sum = 0;
    const uint64_t stride = uint64_t(gridDim.x) * kCmsLdsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kCmsLdsBlock + threadIdx.x; i < I.n; i += stride) {
        const uint32_t v = cms_incr(I, uint32_t(i));
        if (!v) continue;
        sum += v;
        const Item it = cms_item(I, uint32_t(i));
        if (v <= lds_max) {
            for (uint32_t r = 0; r < T.depth; r++) atomicAdd(&tab[cms_cell(T, it, r)], v);
        } else {
            for (uint32_t r = 0; r < T.depth; r++) cms_sat_add(T.cells + cms_cell(T, it, r), v);
        }
    }
    __syncthreads();
    // flush, each workgroup starting at another part of the table
    const uint32_t rot = uint32_t(uint64_t(blockIdx.x) * T.ncells / gridDim.x);
    for (uint32_t j = threadIdx.x; j < T.ncells; j += kCmsLdsBlock) {
        uint32_t c = j + rot;
        if (c >= T.ncells) c -= T.ncells;
        const uint32_t v = tab[c];
        if (v) cms_sat_add(T.cells + c, v);
    }
    cms_count(sum, &wsum, T.count);
}

// global form
__global__ void __launch_bounds__(kCmsBlock) k_cms_add_global(const CmsTable T, const CmsItems I) {
    __shared__ unsigned long long wsum;
    if (threadIdx.x == 0) wsum = 0;
    __syncthreads();
    unsigned long long sum = 0;
    const uint64_t stride = uint64_t(gridDim.x) * kCmsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kCmsBlock + threadIdx.x; i < I.n; i += stride) {
        const uint32_t v = cms_incr(I, uint32_t(i));
        if (!v) continue;
        sum += v;
        const Item it = cms_item(I, uint32_t(i));
        for (uint32_t r = 0; r < T.depth; r++) cms_sat_add(T.cells + cms_cell(T, it, r), v);
    }
    cms_count(sum, &wsum, T.count);
}

// Sequential form: one wavefront, lane = row (looping past 64 rows), items in
// order.  A row's cells are only ever touched by the row's lane, in program
// order, so plain loads and stores carry the sequence.
__global__ void __launch_bounds__(64) k_cms_seq(const CmsTable T, const CmsItems I, uint32_t *reply) {
    unsigned long long sum = 0;
    for (uint32_t i = 0; i < I.n; i++) {
        const uint32_t v = I.incr ? I.incr[i] : 1u;
        const Item it = cms_item(I, i);
        uint32_t mn = 0xffffffffu;
        for (uint32_t r = threadIdx.x; r < T.depth; r += 64) {
            uint32_t *cell = T.cells + cms_cell(T, it, r);
            const uint32_t cur = *cell;
            uint32_t nv = cur + v;
            if (nv < cur) nv = 0xffffffffu;
            *cell = nv;
            mn = umin32(mn, nv);
        }
        for (int o = 32; o > 0; o >>= 1) mn = umin32(mn, __shfl_xor(mn, o, 64));
        if (threadIdx.x == 0) reply[i] = mn;
        sum += v;
    }
    if (threadIdx.x == 0 && sum) atomicAdd(T.count, sum);
}

__global__ void __launch_bounds__(kCmsBlock) k_cms_query(const CmsTable T, const CmsItems I, uint32_t *out) {
    const uint64_t stride = uint64_t(gridDim.x) * kCmsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kCmsBlock + threadIdx.x; i < I.n; i += stride) {
        const Item it = cms_item(I, uint32_t(i));
        uint32_t mn = 0xffffffffu;
        for (uint32_t r = 0; r < T.depth; r++) mn = umin32(mn, T.cells[cms_cell(T, it, r)]);
        out[i] = mn;
    }
}

// Weighted merge, cell by cell: the check pass flags a sum outside a cell's
// range (or a 64-bit overflow on the way), the write pass stores the sums.  A
// thread reads every source's cell c before it writes dst's cell c, and no
// other thread touches cell c, so dst may be one of the sources.
template <bool kWrite>
__global__ void __launch_bounds__(kCmsBlock) k_cms_merge(const CmsMergeArgs M) {
    bool bad = false;
    const uint32_t stride = gridDim.x * kCmsBlock;
    for (uint32_t c = blockIdx.x * kCmsBlock + threadIdx.x; c < M.ncells; c += stride) {
        long long acc = 0;
        for (uint32_t k = 0; k < M.nsrc; k++) {
            long long term;
            bad |= __builtin_mul_overflow((long long)M.src[k][c], M.w[k], &term);
            bad |= __builtin_add_overflow(acc, term, &acc);
        }
        bad |= acc < 0 || acc > 0xffffffffLL;
        if (kWrite) M.dst[c] = uint32_t(acc);
    }
    if (!kWrite && bad) atomicOr(M.flag, 1u);
}

// The saturating sum of caller-owned tables (the ranks' tables after an
// all-gather): a stream over the cells, 16 bytes a load from every table, the
// sums in 64 bits (at most 64 tables of 32-bit cells: no overflow), a cell that
// would pass 2^32 - 1 stays there -- the table one context's bulk adds build.
// Apart from k_cms_merge: no weights, no check pass, no failure.  Thread c reads
// every table's cells before it writes dst's, and nobody else touches them, so
// dst's own cells may be one of the tables.
__device__ __forceinline__ uint32_t cms_sat32(unsigned long long v) {
    return v > 0xffffffffull ? 0xffffffffu : uint32_t(v);
}

__global__ void __launch_bounds__(kCmsBlock) k_cms_sum(uint32_t *dst, unsigned long long *dst_count,
                                                        const uint32_t *tables, uint64_t stride, uint32_t ntables,
                                                        uint32_t ncells, unsigned long long count) {
    const uint32_t nvec = ncells >> 2;
    const uint32_t step = gridDim.x * kCmsBlock;
    for (uint32_t v = blockIdx.x * kCmsBlock + threadIdx.x; v < nvec; v += step) {
        unsigned long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        for (uint32_t k = 0; k < ntables; k++) {
            const uint4 x = reinterpret_cast<const uint4 *>(tables + k * stride)[v];
            a0 += x.x;
            a1 += x.y;
            a2 += x.z;
            a3 += x.w;
        }
        reinterpret_cast<uint4 *>(dst)[v] = make_uint4(cms_sat32(a0), cms_sat32(a1), cms_sat32(a2), cms_sat32(a3));
    }
    if (blockIdx.x == 0) {
        // the tail: ncells & 3 cells behind the last whole vector
        const uint32_t c = (nvec << 2) + threadIdx.x;
        if (threadIdx.x < 4 && c < ncells) {
            unsigned long long a = 0;
            for (uint32_t k = 0; k < ntables; k++) a += tables[k * stride + c];
            dst[c] = cms_sat32(a);
        }
        if (threadIdx.x == 0) *dst_count = count;
    }
}

}  // namespace

hipError_t cms_setup() {
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_cms_add_lds),
                               hipFuncAttributeMaxDynamicSharedMemorySize, kCmsLdsMaxBytes);
}

hipError_t launch_cms_add(const CmsTable &T, const CmsItems &I, bool lds, int cus, hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    if (lds) {
        if (T.ncells > kCmsLdsCells) return hipErrorInvalidValue;
        // one workgroup per CU (fewer when the batch is smaller than that)
        const unsigned grid = grid_for(I.n, kCmsLdsBlock, unsigned(cus));
        const uint64_t per_wg = (uint64_t(I.n) + uint64_t(grid) * kCmsLdsBlock - 1) / (uint64_t(grid) * kCmsLdsBlock) * kCmsLdsBlock;
        const uint32_t lds_max = uint32_t(0xffffffffull / per_wg);
        hipLaunchKernelGGL(k_cms_add_lds, dim3(grid), dim3(kCmsLdsBlock), size_t(T.ncells) * 4, st, T, I, lds_max);
    } else {
        hipLaunchKernelGGL(k_cms_add_global, dim3(grid_for(I.n, kCmsBlock, unsigned(cus) * 8)), dim3(kCmsBlock), 0, st,
                           T, I);
    }
    return hipGetLastError();
}

hipError_t launch_cms_seq(const CmsTable &T, const CmsItems &I, uint32_t *reply, hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cms_seq, dim3(1), dim3(64), 0, st, T, I, reply);
    return hipGetLastError();
}

hipError_t launch_cms_query(const CmsTable &T, const CmsItems &I, uint32_t *out, int cus, hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cms_query, dim3(grid_for(I.n, kCmsBlock, unsigned(cus) * 8)), dim3(kCmsBlock), 0, st, T, I,
                       out);
    return hipGetLastError();
}

hipError_t launch_cms_merge(const CmsMergeArgs &M, bool write, int cus, hipStream_t st) {
    const unsigned grid = grid_for(M.ncells, kCmsBlock, unsigned(cus) * 4);
    if (write)
        hipLaunchKernelGGL(k_cms_merge<true>, dim3(grid), dim3(kCmsBlock), 0, st, M);
    else
        hipLaunchKernelGGL(k_cms_merge<false>, dim3(grid), dim3(kCmsBlock), 0, st, M);
    return hipGetLastError();
}

hipError_t launch_cms_sum(const CmsTable &D, const uint32_t *tables, uint64_t stride, uint32_t ntables,
                          unsigned long long count, int cus, hipStream_t st) {
    const unsigned grid = grid_for(D.ncells / 4, kCmsBlock, unsigned(cus) * 8);
    hipLaunchKernelGGL(k_cms_sum, dim3(grid), dim3(kCmsBlock), 0, st, D.cells, D.count, tables, stride, ntables,
                       D.ncells, count);
    return hipGetLastError();
}

}  // namespace ske
