// sketch_rows.hip -- row logs (DESIGN.md "Row log"): the attendance table's rows
// (lecture digest, epoch, student id, is_valid) as four device columns, appended
// in arrival order and read back per lecture in the table's clustering order.
//
// An append is four launches on one stream, none of which waits for a block of
// its own launch (sketch_hh.hip's rule: no thread spins on another's progress):
//   k_rows_flag   per item: taken (status 0, mask 1)?  its id parsed (canonical
//                 decimal text, or 4 / 8 little-endian bytes); a flag byte and the
//                 id to scratch, and per tile of kRowsBlock items the count of
//                 the rows to place and of the refused ids
//   k_rows_scan   one workgroup: the tile counts to their exclusive prefix, in
//                 place, kRowsScanBlock tiles a pass; the two totals
//   k_rows_place  per tile: a row's rank among the tile's rows (wave64 ballot
//                 and popcount, the waves' totals through LDS), its position
//                 used + prefix[tile] + rank; rows inside the capacity get their
//                 lecture's digest and are written
//   k_rows_end    one thread: the head's advance
// Every position is a function of the batch and of `used` alone, so the log's
// contents and layout are the same from run to run, and position order is
// arrival order within a call and across calls.  `used` lives in the log and
// is advanced by k_rows_end, never passed as a launch argument: a recorded
// append that is replayed appends behind what is there.
//
// A select reuses the same flag / count / scan machinery twice: over the log's
// rows (which match), and over the matching positions in sorted order (which
// is the last of its run of equal keys).  The sort between the two is
// rows_sort_pairs (sketch_order.hip), one stable pass per key column.  The
// group-by and the profile (below, "group-by") start from that same front end.
// The group merge ("group merge") sums several group-bys' outputs per key: the
// same sort over the caller's keys, its own flags and prefixes, then the
// group-by's back end.
#include "sketch_common.h"
#include "sketch_internal.h"

namespace ske {
namespace {

constexpr int kRowsWaves = kRowsBlock / 64;
static_assert(kRowsBlock % 64 == 0 && kRowsScanBlock % 64 == 0, "whole wavefronts");

// the tile's two counts to cnt (every thread of the workgroup calls it)
__device__ __forceinline__ void rows_tile_count(bool ok, bool ref, uint32_t *cnt, uint64_t tiles, uint64_t t,
                                                unsigned int *s_ok, unsigned int *s_ref) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b_ok = __ballot(ok), b_ref = __ballot(ref);
    if (lane == 0) {
        s_ok[w] = uint32_t(__popcll(b_ok));
        s_ref[w] = uint32_t(__popcll(b_ref));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, r = 0;
#pragma unroll
        for (int k = 0; k < kRowsWaves; k++) a += s_ok[k], r += s_ref[k];
        cnt[4 + t] = a;
        cnt[4 + tiles + t] = r;
    }
    __syncthreads();  // the LDS words are written again in the next turn
}

// the rank of a flagged item among the tile's flagged items, in item order
__device__ __forceinline__ uint32_t rows_tile_rank(bool ok, unsigned int *s_ok) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long b = __ballot(ok);
    if (lane == 0) s_ok[w] = uint32_t(__popcll(b));
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (int k = 0; k < kRowsWaves; k++)
        if (uint32_t(k) < w) before += s_ok[k];
    const uint32_t r = before + uint32_t(__popcll(b & ((1ull << lane) - 1)));
    __syncthreads();
    return r;
}

// the id text of at most kRowsIdMaxLen bytes as three words (only the aligned
// words that hold a byte of it are read)
__device__ __forceinline__ bool rows_id_text(const uint8_t *p, uint32_t len, int64_t *out) {
    if (len == 0 || len > kRowsIdMaxLen) return false;
    const uint64_t w0 = load_le(p, len < 8 ? len : 8);
    const uint64_t w1 = len > 8 ? load_le(p + 8, len < 16 ? len - 8 : 8) : 0;
    const uint64_t w2 = len > 16 ? load_le(p + 16, len - 16) : 0;
    return rows_parse_id(w0, w1, w2, len, out);
}

template <int kKind>
__global__ void __launch_bounds__(kRowsBlock) k_rows_flag(const RowsItems I, const RowsWork W) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    const uint64_t tiles = rows_tiles(I.n);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        const bool in = i < I.n;
        const bool takes = in && (!I.status || I.status[i] == 0) && (!I.mask || I.mask[i] == 1);
        int64_t v = 0;
        bool ok = false;
        if (takes) {
            if (kKind == 0) {
                const uint32_t b = I.id_offs[i], e = I.id_offs[i + 1];
                ok = rows_id_text(I.id_bytes + b, e - b, &v);
            } else if (kKind == 1) {
                const uint8_t *p = I.id_bytes + i * I.id_width;
                v = I.id_width == 8 ? int64_t(load_le(p, 8)) : int64_t(int32_t(uint32_t(load_le(p, 4))));
                ok = true;
            } else {
                ok = rows_id_text(I.id_bytes + I.id_offs[i], I.id_len[i], &v);
            }
        }
        if (in) {
            W.flag[i] = takes ? (ok ? 1 : 2) : 0;
            W.idv[i] = v;
        }
        rows_tile_count(ok, takes && !ok, W.cnt, tiles, t, s_ok, s_ref);
    }
}

// cnt[4 + t] = the placed-counts of the tiles before t; cnt[0] = their total,
// cnt[1] = the refused-counts' total.  One workgroup: a pass scans
// kRowsScanBlock tiles (an inclusive scan per wavefront by shuffles, the
// wavefronts' totals through LDS) and carries its total into the next.
__global__ void __launch_bounds__(kRowsScanBlock) k_rows_scan(uint32_t *cnt, uint64_t tiles) {
    constexpr int kWaves = kRowsScanBlock / 64;
    __shared__ unsigned int s_w[kWaves];
    __shared__ unsigned int s_ref;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_ref = 0;
    uint32_t carry = 0, ref = 0;
    for (uint64_t base = 0; base < tiles; base += kRowsScanBlock) {
        const uint64_t t = base + threadIdx.x;
        const uint32_t a = t < tiles ? cnt[4 + t] : 0;
        if (t < tiles) ref += cnt[4 + tiles + t];
        uint32_t x = a;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= uint32_t(d)) x += y;
        }
        if (lane == 63) s_w[w] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; k++) {
            const uint32_t s = s_w[k];
            if (uint32_t(k) < w) before += s;
            all += s;
        }
        if (t < tiles) cnt[4 + t] = carry + before + x - a;
        carry += all;
        __syncthreads();
    }
    if (ref) atomicAdd(&s_ref, ref);
    __syncthreads();
    if (threadIdx.x == 0) {
        cnt[0] = carry;
        cnt[1] = s_ref;
    }
}

template <int kKind>
__global__ void __launch_bounds__(kRowsBlock) k_rows_place(const RowsLog L, const RowsItems I, const RowsWork W) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(I.n);
    const unsigned long long used = L.head->used;  // k_rows_end advances it behind this launch
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        const bool ok = i < I.n && W.flag[i] == 1;
        const uint32_t rank = rows_tile_rank(ok, s_ok);
        if (!ok) continue;
        const unsigned long long pos = used + W.cnt[4 + t] + rank;
        if (pos >= L.capacity) continue;  // the batch's tail: k_rows_end counts it
        uint32_t b, e;
        if (kKind == 2) {
            b = I.lec_offs[i];
            e = b + I.lec_len[i];
        } else {
            b = I.lec_offs[i];
            e = I.lec_offs[i + 1];
        }
        const Item it = load_item(I.lec_bytes, b, e);
        L.lec[pos] = rows_lecture_word(murmur_item(it, kBloomSeed));
        L.epoch[pos] = I.epoch[i];
        L.id[pos] = W.idv[i];
        L.valid[pos] = I.valid && I.valid[i] ? 1 : 0;
    }
}

__global__ void k_rows_end(const RowsLog L, const uint32_t *cnt) {
    if (blockIdx.x || threadIdx.x) return;
    RowsHead *h = L.head;
    const unsigned long long ok = cnt[0], ref = cnt[1];
    const unsigned long long room = L.capacity - h->used;
    const unsigned long long kept = ok < room ? ok : room;
    h->used += kept;
    h->taken += ok + ref;
    h->refused_ids += ref;
    if (ok > kept) {
        h->dropped += ok - kept;
        h->overflow = 1;
    }
}

// ---- select

__global__ void __launch_bounds__(kRowsBlock) k_rows_match(const RowsLog L, uint32_t m, int by_lec,
                                                            unsigned long long digest, long long since,
                                                            long long until, const RowsWork W) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    const bool open_end = until == INT64_MAX;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        bool ok = false;
        if (i < m) {
            const long long e = L.epoch[i];
            ok = (!by_lec || L.lec[i] == digest) && e >= since && (open_end || e < until);
            W.flag[i] = ok ? 1 : 0;
        }
        rows_tile_count(ok, false, W.cnt, tiles, t, s_ok, s_ref);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_positions(uint32_t m, const RowsWork W, uint32_t *pos_out) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        const bool ok = i < m && W.flag[i] == 1;
        const uint32_t rank = rows_tile_rank(ok, s_ok);
        if (ok) pos_out[W.cnt[4 + t] + rank] = uint32_t(i);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_keys(const RowsLog L, const uint32_t *pos, uint32_t m, int col,
                                                           unsigned long long *key_out) {
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t j = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; j < m; j += stride) {
        const uint32_t p = pos[j];
        key_out[j] = col == 0 ? (unsigned long long)L.id[p] : col == 1 ? (unsigned long long)L.epoch[p] : L.lec[p];
    }
}

// pos is sorted by (lec, epoch, id, position): the last row of a run of equal
// (lec, epoch, id) is the one appended last -- the upsert's survivor
__global__ void __launch_bounds__(kRowsBlock) k_rows_last(const RowsLog L, const uint32_t *pos, uint32_t m,
                                                           const RowsWork W) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        bool last = false;
        if (j < m) {
            last = true;
            if (j + 1 < m) {
                const uint32_t p = pos[j], q = pos[j + 1];
                last = L.id[p] != L.id[q] || L.epoch[p] != L.epoch[q] || L.lec[p] != L.lec[q];
            }
            W.flag[j] = last ? 1 : 0;
        }
        rows_tile_count(last, false, W.cnt, tiles, t, s_ok, s_ref);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gather(const RowsLog L, const uint32_t *pos, uint32_t m,
                                                             const RowsWork W, unsigned long long *out_lec,
                                                             long long *out_epoch, long long *out_id,
                                                             uint8_t *out_valid) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        const bool ok = j < m && W.flag[j] == 1;
        const uint32_t rank = rows_tile_rank(ok, s_ok);
        if (!ok) continue;
        const uint32_t p = pos[j];
        const uint64_t o = uint64_t(W.cnt[4 + t]) + rank;
        out_lec[o] = L.lec[p];
        out_epoch[o] = L.epoch[p];
        out_id[o] = L.id[p];
        out_valid[o] = L.valid[p];
    }
}

// ---- group-by (the arithmetic is sketch_rows_group.h's)
//
// Over the sorted positions, after k_rows_last flagged each run's survivor.
// For BY_STUDENT the id is the sort's last (most significant) pass, for
// BY_LECTURE the digest, so the rows of a key lie in one run, the keys
// ascending, and nothing is sorted or moved again:
//   k_rows_gflag   per position two bits -- counted (survivor and passes the
//                  filters), group end (the last position of its key run) --
//                  and per tile the count of each
//   k_rows_scan    twice: the two tile counts to their prefixes
//   k_rows_gends   per group end: (key, counted prefix at the end) to its group rank
//   k_rows_gcount  per group: the count is the step from the group before;
//                  listed = count > 0, its tile counts; n, sum, sumsq, min, max
//                  (per thread over its tiles, then the wavefront, then the
//                  workgroup through LDS, then one set of 64-bit integer
//                  atomics per workgroup: identical from run to run)
//   k_rows_scan, k_rows_gplace   the listed groups, compacted in key order
//   k_rows_sel_hist / k_rows_sel_walk   four rounds: the two median ranks
// No thread waits for another workgroup.

__device__ __forceinline__ unsigned long long rows_key_of(const RowsLog &L, uint32_t p, int by) {
    return by == kRowsByStudent ? (unsigned long long)L.id[p] : L.lec[p];
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_ginit(RowsGrpDev *D) {
    uint32_t *w = reinterpret_cast<uint32_t *>(D);
    for (uint32_t i = threadIdx.x; i < sizeof(RowsGrpDev) / 4; i += kRowsBlock) w[i] = 0;
    __syncthreads();
    if (threadIdx.x == 0) D->min = ~0ull;
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gflag(const RowsLog L, const uint32_t *pos, uint32_t m, int by,
                                                            int valid_filter, uint32_t sod_from, const uint8_t *surv,
                                                            const RowsGrpWork G) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        bool counted = false, gend = false;
        if (j < m) {
            const uint32_t p = pos[j];
            counted = surv[j] == 1 && rows_counted(L.valid[p], L.epoch[p], valid_filter, sod_from);
            gend = j + 1 == m || rows_key_of(L, p, by) != rows_key_of(L, pos[j + 1], by);
            G.gflag[j] = uint8_t((counted ? 1 : 0) | (gend ? 2 : 0));
        }
        rows_tile_count(counted, false, G.cnt_c, tiles, t, s_ok, s_ref);
        rows_tile_count(gend, false, G.cnt_e, tiles, t, s_ok, s_ref);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gends(const RowsLog L, const uint32_t *pos, uint32_t m, int by,
                                                            const RowsGrpWork G) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(m);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        const uint32_t f = j < m ? G.gflag[j] : 0;
        const bool counted = f & 1, gend = f & 2;
        const uint32_t rc = rows_tile_rank(counted, s_ok);
        const uint32_t re = rows_tile_rank(gend, s_ok);
        if (!gend) continue;
        const uint64_t g = uint64_t(G.cnt_e[4 + t]) + re;
        G.gkey[g] = rows_key_of(L, pos[j], by);
        G.gend[g] = G.cnt_c[4 + t] + rc + (counted ? 1u : 0u);
    }
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long wave_min64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gcount(const RowsGrpWork G, uint32_t groups, RowsGrpDev *D) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    __shared__ unsigned long long s_acc[kRowsWaves][5];
    const uint64_t tiles = rows_tiles(groups);
    unsigned long long n = 0, sum = 0, sq = 0, mn = ~0ull, mx = 0;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t g = t * kRowsBlock + threadIdx.x;
        const uint32_t c = g < groups ? rows_group_count(G.gend, g) : 0;
        const bool listed = rows_group_listed(c);
        if (listed) {
            n += 1;
            sum += c;
            sq += (unsigned long long)c * c;
            mn = c < mn ? c : mn;
            mx = c > mx ? c : mx;
        }
        rows_tile_count(listed, false, G.cnt_l, tiles, t, s_ok, s_ref);
    }
    n = wave_sum64(n), sum = wave_sum64(sum), sq = wave_sum64(sq), mn = wave_min64(mn), mx = wave_max64(mx);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_acc[w][0] = n, s_acc[w][1] = sum, s_acc[w][2] = sq, s_acc[w][3] = mn, s_acc[w][4] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kRowsWaves; k++) {
            n += s_acc[k][0], sum += s_acc[k][1], sq += s_acc[k][2];
            mn = s_acc[k][3] < mn ? s_acc[k][3] : mn;
            mx = s_acc[k][4] > mx ? s_acc[k][4] : mx;
        }
        if (n) {
            atomicAdd(&D->n, n);
            atomicAdd(&D->sum, sum);
            atomicAdd(&D->sumsq, sq);
            atomicMin(&D->min, mn);
            atomicMax(&D->max, mx);
        }
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gplace(const RowsGrpWork G, uint32_t groups) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(groups);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t g = t * kRowsBlock + threadIdx.x;
        const uint32_t c = g < groups ? rows_group_count(G.gend, g) : 0;
        const bool listed = rows_group_listed(c);
        const uint32_t rank = rows_tile_rank(listed, s_ok);
        if (!listed) continue;
        const uint64_t o = uint64_t(G.cnt_l[4 + t]) + rank;
        G.lkey[o] = G.gkey[g];
        G.lcount[o] = c;
    }
}

__global__ void k_rows_sel_begin(RowsGrpDev *D) {
    if (blockIdx.x == 0 && threadIdx.x == 0) rows_sel_begin(&D->sel, D->n);
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_sel_hist(const uint32_t *counts, uint32_t n, RowsGrpDev *D,
                                                               uint32_t round) {
    __shared__ unsigned int s_h[2 * kHhSelBins];
    for (uint32_t i = threadIdx.x; i < 2 * kHhSelBins; i += kRowsBlock) s_h[i] = 0;
    __syncthreads();
    const uint32_t shift = hh_sel_shift(round);
    const uint32_t p0 = D->sel.prefix[0], p1 = D->sel.prefix[1];
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; i < n; i += stride) {
        const uint32_t v = counts[i], d = hh_sel_digit(v, shift);
        if (hh_sel_matches(v, p0, shift)) atomicAdd(&s_h[d], 1u);
        if (hh_sel_matches(v, p1, shift)) atomicAdd(&s_h[kHhSelBins + d], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * kHhSelBins; i += kRowsBlock)
        if (s_h[i]) atomicAdd(&D->hist[i], s_h[i]);
}

// one workgroup: the walk, then the histograms zero for the next round
__global__ void __launch_bounds__(kRowsBlock) k_rows_sel_walk(RowsGrpDev *D, uint32_t round) {
    if (blockIdx.x) return;
    if (threadIdx.x == 0) rows_sel_step(&D->sel, D->hist, round);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 2 * kHhSelBins; i += kRowsBlock) D->hist[i] = 0;
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_gout(const RowsGrpWork G, uint32_t n, unsigned long long *out_key,
                                                           unsigned long long *out_count) {
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; i < n; i += stride) {
        out_key[i] = G.lkey[i];
        out_count[i] = G.lcount[i];
    }
}

// the counted survivors by weekday and hour: a histogram per workgroup in LDS
// (a workgroup sees fewer than 2^32 rows), flushed with 64-bit adds
__global__ void __launch_bounds__(kRowsBlock) k_rows_profile(const RowsLog L, const uint32_t *pos, uint32_t m,
                                                              int valid_filter, uint32_t sod_from, const uint8_t *surv,
                                                              RowsGrpDev *D) {
    __shared__ unsigned int s_b[kTpBins];
    for (uint32_t i = threadIdx.x; i < kTpBins; i += kRowsBlock) s_b[i] = 0;
    __syncthreads();
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t j = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; j < m; j += stride) {
        if (surv[j] != 1) continue;
        const uint32_t p = pos[j];
        const long long e = L.epoch[p];
        if (rows_counted(L.valid[p], e, valid_filter, sod_from)) atomicAdd(&s_b[tp_bin(tp_time(e))], 1u);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < kTpBins; i += kRowsBlock)
        if (s_b[i]) atomicAdd(&D->bins[i], (unsigned long long)s_b[i]);
}

// ---- group merge (the arithmetic is sketch_rows_merge.h's)
//
// (key, count) entries in any order -- several group-bys' outputs, end to end
// -- to one ascending list of the keys' sums.  After one rows_sort_pairs of an
// iota by the keys:
//   k_rows_mflag   per sorted position the entry's count v, group end, v != 0;
//                  per tile the u32 sum of v (the wavefront by shuffles, the
//                  wavefronts through LDS) and the counts of the two flags; per
//                  workgroup one 64-bit add of the true total and an OR of
//                  "some v >= 2^32", which the host reads before any output
//   k_rows_scan    three times: the tile sums and counts to their prefixes
//   k_rows_mends   per group end, at its group rank: the key, the inclusive
//                  prefix of v (tile prefix + the earlier wavefronts' totals +
//                  a wave64 inclusive scan) and of the nonzero flags
//   k_rows_mmulti  per group: listed with more than one nonzero entry?
// and the group-by's back end over the prefix of v (k_rows_gcount, k_rows_scan,
// k_rows_gplace, the select rounds, k_rows_gout).  No thread waits for another
// workgroup; every accumulation is an integer's, so the answer does not depend
// on the order of the entries or of the workgroups.

__global__ void __launch_bounds__(kRowsBlock) k_rows_iota(uint32_t *idx, uint32_t n) {
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; i < n; i += stride) idx[i] = uint32_t(i);
}

__global__ void k_rows_minit(RowsMrgDev *M) {
    if (blockIdx.x == 0 && threadIdx.x == 0) M->total = 0, M->multi = 0, M->wide = 0, M->pad = 0;
}

// the inclusive prefix of v over the tile's threads (every thread of the
// workgroup calls it); *all = the tile's sum.  u32 arithmetic: the caller
// bounds the total.
__device__ __forceinline__ uint32_t rows_tile_prefix(uint32_t v, unsigned int *s_w, uint32_t *all) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= uint32_t(d)) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (int k = 0; k < kRowsWaves; k++) {
        const uint32_t s = s_w[k];
        if (uint32_t(k) < w) before += s;
        sum += s;
    }
    __syncthreads();  // the LDS words are written again in the next turn
    *all = sum;
    return before + x;
}

// what sorted position j < n holds: the entry's count and whether it ends its key's run
__device__ __forceinline__ unsigned long long rows_mrg_entry(const RowsMrgWork &W, uint64_t j, uint32_t n,
                                                             bool *gend) {
    *gend = j + 1 == n || W.keys_s[j] != W.keys_s[j + 1];
    return W.counts[W.idx_s[j]];
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_mflag(const RowsMrgWork W, const RowsGrpWork G, uint32_t n,
                                                            RowsMrgDev *M) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    __shared__ unsigned long long s_tot[kRowsWaves];
    __shared__ unsigned int s_wide;
    if (threadIdx.x == 0) s_wide = 0;
    __syncthreads();
    const uint64_t tiles = rows_tiles(n);
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long tot = 0;
    bool wide = false;
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        unsigned long long v = 0;
        bool gend = false;
        if (j < n) {
            v = rows_mrg_entry(W, j, n, &gend);
            if (rows_merge_entry_ok(v)) tot += v;
            else wide = true;
        }
        // the tile's u32 sum: the wavefront by shuffles, the wavefronts through LDS
        uint32_t x = uint32_t(v);
        for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) s_ok[w] = x;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t a = 0;
#pragma unroll
            for (int k = 0; k < kRowsWaves; k++) a += s_ok[k];
            G.cnt_c[4 + t] = a;
            G.cnt_c[4 + tiles + t] = 0;
        }
        __syncthreads();
        rows_tile_count(gend, false, G.cnt_e, tiles, t, s_ok, s_ref);
        rows_tile_count(v != 0, false, W.cnt_z, tiles, t, s_ok, s_ref);
    }
    tot = wave_sum64(tot);
    const unsigned long long any_wide = __ballot(wide);
    if (lane == 0) {
        s_tot[w] = tot;
        if (any_wide) atomicOr(&s_wide, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kRowsWaves; k++) tot += s_tot[k];
        if (tot) atomicAdd(&M->total, tot);
        if (s_wide) atomicOr(&M->wide, 1u);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_mends(const RowsMrgWork W, const RowsGrpWork G, uint32_t n) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(n);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t j = t * kRowsBlock + threadIdx.x;
        unsigned long long v = 0;
        bool gend = false;
        if (j < n) v = rows_mrg_entry(W, j, n, &gend);
        const bool nz = v != 0;
        uint32_t all;
        const uint32_t pv = rows_tile_prefix(uint32_t(v), s_ok, &all);
        const uint32_t rz = rows_tile_rank(nz, s_ok);
        const uint32_t re = rows_tile_rank(gend, s_ok);
        if (!gend) continue;
        const uint64_t g = uint64_t(G.cnt_e[4 + t]) + re;
        G.gkey[g] = W.keys_s[j];
        G.gend[g] = G.cnt_c[4 + t] + pv;
        W.zend[g] = W.cnt_z[4 + t] + rz + (nz ? 1u : 0u);
    }
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_mmulti(const RowsMrgWork W, const RowsGrpWork G, uint32_t groups,
                                                             RowsMrgDev *M) {
    __shared__ unsigned long long s_m[kRowsWaves];
    unsigned long long m = 0;
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t g = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; g < groups; g += stride)
        if (rows_merge_multi(rows_merge_sum(G.gend, g), rows_merge_entries(W.zend, g))) m += 1;
    m = wave_sum64(m);
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kRowsWaves; k++) m += s_m[k];
        if (m) atomicAdd(&M->multi, m);
    }
}

// ---- compaction (the arithmetic is sketch_rows_compact.h's)
//
// After the front end over the whole log (every lecture, epoch >= keep_since,
// table order) flagged each run's survivor per sorted position:
//   k_rows_ckeep   per sorted position: a survivor's log position gets its keep
//                  byte (the bytes were cleared)
//   k_rows_ccount  per tile of log positions: the count of keep bytes
//   k_rows_scan    the tile counts to their prefixes
//   k_rows_cmove   two columns a launch: the survivor at position i to
//                  prefix[tile] + rank in tile of two scratch columns
//   k_rows_cback   the scratch columns' [0, kept) back over the log's
//   k_rows_cend    one thread: the head
// A launch that reads the log writes scratch only, and the other way round, so
// no workgroup reads a log location another of its launch writes.  The target of
// a survivor is a function of the keep bytes alone: position order stays arrival
// order and the compacted log is the same from run to run.

__global__ void __launch_bounds__(kRowsBlock) k_rows_ckeep(const uint32_t *pos, uint32_t m, const uint8_t *surv,
                                                            uint8_t *keep) {
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t j = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; j < m; j += stride)
        if (surv[j] == 1) keep[pos[j]] = 1;
}

__global__ void __launch_bounds__(kRowsBlock) k_rows_ccount(const uint8_t *keep, uint32_t used, uint32_t *cnt) {
    __shared__ unsigned int s_ok[kRowsWaves], s_ref[kRowsWaves];
    const uint64_t tiles = rows_tiles(used);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        rows_tile_count(i < used && keep[i] == 1, false, cnt, tiles, t, s_ok, s_ref);
    }
}

template <typename A, typename B>
__global__ void __launch_bounds__(kRowsBlock) k_rows_cmove(const A *a, const B *b, uint32_t used, const uint8_t *keep,
                                                            const uint32_t *cnt, A *out_a, B *out_b) {
    __shared__ unsigned int s_ok[kRowsWaves];
    const uint64_t tiles = rows_tiles(used);
    for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const uint64_t i = t * kRowsBlock + threadIdx.x;
        const bool ok = i < used && keep[i] == 1;
        const uint32_t rank = rows_tile_rank(ok, s_ok);
        if (!ok) continue;
        const uint64_t o = uint64_t(cnt[4 + t]) + rank;
        out_a[o] = a[i];
        out_b[o] = b[i];
    }
}

template <typename A, typename B>
__global__ void __launch_bounds__(kRowsBlock) k_rows_cback(const A *a, const B *b, uint32_t kept, A *out_a, B *out_b) {
    const uint64_t stride = uint64_t(gridDim.x) * kRowsBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kRowsBlock + threadIdx.x; i < kept; i += stride) {
        out_a[i] = a[i];
        out_b[i] = b[i];
    }
}

__global__ void k_rows_cend(const RowsLog L, unsigned long long kept) {
    if (blockIdx.x || threadIdx.x) return;
    rows_compact_head(&L.head->used, &L.head->taken, kept);
}

// workgroups of a kernel over n items: the context's override, else eight per CU
unsigned grid_of(uint64_t n, unsigned grid, int cus) {
    return grid_for(n, kRowsBlock, grid, unsigned(cus) * 8, kRowsMaxGrid);
}

hipError_t rows_scan(uint32_t *cnt, uint64_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(kRowsScanBlock), 0, st, cnt, rows_tiles(n));
    return hipGetLastError();
}

template <int kKind>
hipError_t rows_append_kind(const RowsLog &L, const RowsItems &I, const RowsWork &W, unsigned g, hipStream_t st) {
    hipLaunchKernelGGL(k_rows_flag<kKind>, dim3(g), dim3(kRowsBlock), 0, st, I, W);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rows_scan(W.cnt, I.n, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_place<kKind>, dim3(g), dim3(kRowsBlock), 0, st, L, I, W);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_end, dim3(1), dim3(64), 0, st, L, (const uint32_t *)W.cnt);
    return hipGetLastError();
}

// the survivors of two log columns to the front, by way of the two scratch columns
template <typename A, typename B>
hipError_t rows_compact_pair(A *a, B *b, uint32_t used, uint32_t kept, const RowsCompactWork &K, unsigned g,
                             unsigned g_kept, hipStream_t st) {
    A *ta = reinterpret_cast<A *>(K.tmp_a);
    B *tb = reinterpret_cast<B *>(K.tmp_b);
    hipLaunchKernelGGL((k_rows_cmove<A, B>), dim3(g), dim3(kRowsBlock), 0, st, (const A *)a, (const B *)b, used,
                       (const uint8_t *)K.keep, (const uint32_t *)K.cnt, ta, tb);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_rows_cback<A, B>), dim3(g_kept), dim3(kRowsBlock), 0, st, (const A *)ta, (const B *)tb, kept,
                       a, b);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_rows_compact(const RowsLog &L, uint32_t used, const uint32_t *pos, uint32_t m, const RowsWork &W,
                               uint32_t kept, const RowsCompactWork &K, unsigned grid, int cus, hipStream_t st) {
    if (kept > 0) {
        const unsigned g = grid_of(used, grid, cus);
        hipError_t e = hipMemsetAsync(K.keep, 0, used, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rows_ckeep, dim3(grid_of(m, grid, cus)), dim3(kRowsBlock), 0, st, pos, m,
                           (const uint8_t *)W.flag, K.keep);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rows_ccount, dim3(g), dim3(kRowsBlock), 0, st, (const uint8_t *)K.keep, used, K.cnt);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        e = rows_scan(K.cnt, used, st);
        if (e != hipSuccess) return e;
        const unsigned g_kept = grid_of(kept, grid, cus);
        e = rows_compact_pair(L.lec, L.epoch, used, kept, K, g, g_kept, st);
        if (e != hipSuccess) return e;
        e = rows_compact_pair(L.id, L.valid, used, kept, K, g, g_kept, st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_rows_cend, dim3(1), dim3(64), 0, st, L, (unsigned long long)kept);
    return hipGetLastError();
}

hipError_t launch_rows_append(const RowsLog &L, const RowsItems &I, const RowsWork &W, unsigned grid, int cus,
                              hipStream_t st) {
    if (I.n == 0) return hipSuccess;
    const unsigned g = grid_of(I.n, grid, cus);
    switch (I.kind) {
    case 0: return rows_append_kind<0>(L, I, W, g, st);
    case 1: return rows_append_kind<1>(L, I, W, g, st);
    case 2: return rows_append_kind<2>(L, I, W, g, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_rows_match(const RowsLog &L, uint32_t m, bool by_lec, unsigned long long digest, long long since,
                             long long until, const RowsWork &W, uint32_t *pos_out, unsigned grid, int cus,
                             hipStream_t st) {
    if (m == 0) return hipSuccess;
    const unsigned g = grid_of(m, grid, cus);
    hipLaunchKernelGGL(k_rows_match, dim3(g), dim3(kRowsBlock), 0, st, L, m, by_lec ? 1 : 0, digest, since, until, W);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rows_scan(W.cnt, m, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_positions, dim3(g), dim3(kRowsBlock), 0, st, m, W, pos_out);
    return hipGetLastError();
}

hipError_t launch_rows_keys(const RowsLog &L, const uint32_t *pos, uint32_t m, int col, unsigned long long *key_out,
                            unsigned grid, int cus, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_keys, dim3(grid_of(m, grid, cus)), dim3(kRowsBlock), 0, st, L, pos, m, col, key_out);
    return hipGetLastError();
}

hipError_t launch_rows_last(const RowsLog &L, const uint32_t *pos, uint32_t m, const RowsWork &W, unsigned grid,
                            int cus, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_last, dim3(grid_of(m, grid, cus)), dim3(kRowsBlock), 0, st, L, pos, m, W);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rows_scan(W.cnt, m, st);
}

hipError_t launch_rows_gather(const RowsLog &L, const uint32_t *pos, uint32_t m, const RowsWork &W,
                              unsigned long long *out_lec, long long *out_epoch, long long *out_id,
                              uint8_t *out_valid, unsigned grid, int cus, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_gather, dim3(grid_of(m, grid, cus)), dim3(kRowsBlock), 0, st, L, pos, m, W, out_lec,
                       out_epoch, out_id, out_valid);
    return hipGetLastError();
}

hipError_t launch_rows_grp_init(RowsGrpDev *D, hipStream_t st) {
    hipLaunchKernelGGL(k_rows_ginit, dim3(1), dim3(kRowsBlock), 0, st, D);
    return hipGetLastError();
}

hipError_t launch_rows_grp_flags(const RowsLog &L, const uint32_t *pos, uint32_t m, int by, int valid_filter,
                                 uint32_t sod_from, const RowsWork &W, const RowsGrpWork &G, unsigned grid, int cus,
                                 hipStream_t st) {
    if (m == 0) return hipSuccess;
    const unsigned g = grid_of(m, grid, cus);
    hipLaunchKernelGGL(k_rows_gflag, dim3(g), dim3(kRowsBlock), 0, st, L, pos, m, by, valid_filter, sod_from,
                       (const uint8_t *)W.flag, G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rows_scan(G.cnt_c, m, st);
    if (e != hipSuccess) return e;
    e = rows_scan(G.cnt_e, m, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_gends, dim3(g), dim3(kRowsBlock), 0, st, L, pos, m, by, G);
    return hipGetLastError();
}

hipError_t launch_rows_grp_counts(const RowsGrpWork &G, uint32_t groups, RowsGrpDev *D, unsigned grid, int cus,
                                  hipStream_t st) {
    if (groups == 0) return hipSuccess;
    const unsigned g = grid_of(groups, grid, cus);
    hipLaunchKernelGGL(k_rows_gcount, dim3(g), dim3(kRowsBlock), 0, st, G, groups, D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rows_scan(G.cnt_l, groups, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_gplace, dim3(g), dim3(kRowsBlock), 0, st, G, groups);
    return hipGetLastError();
}

hipError_t launch_rows_grp_median(const RowsGrpWork &G, uint32_t n, RowsGrpDev *D, unsigned grid, int cus,
                                  hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_sel_begin, dim3(1), dim3(64), 0, st, D);
    hipError_t e = hipGetLastError();
    const unsigned g = grid_of(n, grid, cus);
    for (uint32_t round = 0; round < kHhSelRounds && e == hipSuccess; round++) {
        hipLaunchKernelGGL(k_rows_sel_hist, dim3(g), dim3(kRowsBlock), 0, st, (const uint32_t *)G.lcount, n, D, round);
        e = hipGetLastError();
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(k_rows_sel_walk, dim3(1), dim3(kRowsBlock), 0, st, D, round);
        e = hipGetLastError();
    }
    return e;
}

hipError_t launch_rows_grp_out(const RowsGrpWork &G, uint32_t n, unsigned long long *out_key,
                               unsigned long long *out_count, unsigned grid, int cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_gout, dim3(grid_of(n, grid, cus)), dim3(kRowsBlock), 0, st, G, n, out_key, out_count);
    return hipGetLastError();
}

hipError_t launch_rows_iota(uint32_t *idx, uint32_t n, unsigned grid, int cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_iota, dim3(grid_of(n, grid, cus)), dim3(kRowsBlock), 0, st, idx, n);
    return hipGetLastError();
}

hipError_t launch_rows_mrg_ends(const RowsMrgWork &W, const RowsGrpWork &G, uint32_t n_in, RowsMrgDev *M,
                                unsigned grid, int cus, hipStream_t st) {
    hipLaunchKernelGGL(k_rows_minit, dim3(1), dim3(64), 0, st, M);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_in == 0) return e;
    const unsigned g = grid_of(n_in, grid, cus);
    hipLaunchKernelGGL(k_rows_mflag, dim3(g), dim3(kRowsBlock), 0, st, W, G, n_in, M);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = rows_scan(G.cnt_c, n_in, st);
    if (e != hipSuccess) return e;
    e = rows_scan(G.cnt_e, n_in, st);
    if (e != hipSuccess) return e;
    e = rows_scan(W.cnt_z, n_in, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_rows_mends, dim3(g), dim3(kRowsBlock), 0, st, W, G, n_in);
    return hipGetLastError();
}

hipError_t launch_rows_mrg_multi(const RowsMrgWork &W, const RowsGrpWork &G, uint32_t groups, RowsMrgDev *M,
                                 unsigned grid, int cus, hipStream_t st) {
    if (groups == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_mmulti, dim3(grid_of(groups, grid, cus)), dim3(kRowsBlock), 0, st, W, G, groups, M);
    return hipGetLastError();
}

hipError_t launch_rows_profile(const RowsLog &L, const uint32_t *pos, uint32_t m, int valid_filter, uint32_t sod_from,
                               const RowsWork &W, RowsGrpDev *D, unsigned grid, int cus, hipStream_t st) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(k_rows_profile, dim3(grid_of(m, grid, cus)), dim3(kRowsBlock), 0, st, L, pos, m, valid_filter,
                       sod_from, (const uint8_t *)W.flag, D);
    return hipGetLastError();
}

}  // namespace ske
