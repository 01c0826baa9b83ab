// sketch_cms_dev.h -- what the kernels that read a Count-Min Sketch table
// share (sketch_cms.hip, sketch_hh.hip): an item of a batch, its cell in a row.
#pragma once
#include "sketch_internal.h"

namespace ske {

__device__ __forceinline__ Item cms_item(const CmsItems &I, uint32_t i) {
    if (I.offs) return load_item(I.bytes, I.offs[i], I.offs[i + 1]);
    return load_item(I.bytes + uint64_t(i) * I.fixed_w, 0, I.fixed_w);
}

// the item's cell index in row r of the whole table
__device__ __forceinline__ uint32_t cms_cell(const CmsTable &T, const Item &it, uint32_t r) {
    const uint32_t h = it.len <= 16 ? murmur2_32_words(it.w0, it.w1, it.len, r) : murmur2_32(it.p, it.len, r);
    return r * T.div.d + fastmod32(h, T.div);
}

}  // namespace ske
