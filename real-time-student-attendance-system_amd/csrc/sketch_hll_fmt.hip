// sketch_hll_fmt.hip -- HLL keys as Redis strings, many keys a launch
// (DESIGN.md section 14): "HYLL" strings encoded from and decoded into the
// register slab on the device, one key per workgroup of kHllFmtThreads threads.
//
//   k_hll_fmt_sizes  the length of every key's string
//   k_hll_fmt_dump   the strings, back to back at the offsets a scan of the sizes gave
//   k_hll_fmt_load   strings at any byte offset of a blob -> slab rows (SET)
//
// The opcode rules are sketch_hll_fmt.h's.  Encoding: a thread owns kHllFmtSpan
// consecutive registers of the row (held in LDS); the start of the run its
// first register lies in and the end of the run its last register lies in come
// from a maximum scan and a (reverse) minimum scan over per-thread values, the
// offsets of its bytes from a sum scan of its byte count.  Decoding: a thread
// owns a stretch of the payload's bytes; which of them start an opcode follows
// from the last byte before them that is not 01xxxxxx (a maximum scan), the
// first register of every opcode from a sum scan of the run lengths.
#include "sketch_hll_fmt.h"

#include "sketch_internal.h"

namespace ske {
namespace {

constexpr uint32_t kT = kHllFmtThreads;
constexpr uint32_t kWaves = kT / 64;
static_assert(kT == 256 && kHllFmtSpan == 64, "the kernels below are written for 256 threads of 64 registers");

struct OpMax {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; }
};
struct OpMin {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; }
};
struct OpAdd {
    __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a + b; }
};

// Inclusive scan of one value per thread over the workgroup in thread order
// (kRev: from the last thread down), op associative and commutative: inside a
// wavefront by shuffles, then the wavefronts' totals through wtmp[kWaves].
// Every thread of the workgroup calls it.
template <bool kRev, class Op>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, Op op, uint32_t *wtmp) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t o = 1; o < 64; o <<= 1) {
        const uint32_t y = kRev ? __shfl_down(v, o, 64) : __shfl_up(v, o, 64);
        if (kRev ? lane + o < 64 : lane >= o) v = op(y, v);
    }
    if (lane == (kRev ? 0u : 63u)) wtmp[wave] = v;
    __syncthreads();
    if (kRev) {
        for (uint32_t w = wave + 1; w < kWaves; w++) v = op(v, wtmp[w]);
    } else {
        for (uint32_t w = 0; w < wave; w++) v = op(wtmp[w], v);
    }
    __syncthreads();  // wtmp is free again
    return v;
}

// The encoders' LDS image of a row: one pad word after every span, so that the
// threads' spans start 17 words apart and lanes that read the same byte of
// their spans hit different banks.  rpos: where register i lies.
constexpr uint32_t kRowBytes = kHllFmtRegs + kT * 4;
__device__ __forceinline__ uint32_t rpos(uint32_t i) { return i + (i / kHllFmtSpan) * 4; }

// A key's 16 KiB row on its way into the image: read coalesced (16 B per lane
// and step) into registers, so that the next key's row is in flight while this
// key is encoded, and written to LDS when its turn comes.
struct RowRegs {
    uint4 x[kHllFmtRegs / 16 / kT];
};
// key's row (slots == nullptr: the key is the slot); zeros for a slot outside
// the slab (the calls check their lists: never taken)
__device__ __forceinline__ RowRegs fetch_row(const uint8_t *__restrict__ regs, const uint32_t *__restrict__ slots,
                                             uint32_t key, uint32_t nslots) {
    const uint32_t slot = slots ? slots[key] : key;
    RowRegs r;
#pragma unroll
    for (uint32_t k = 0; k < kHllFmtRegs / 16 / kT; k++) r.x[k] = make_uint4(0, 0, 0, 0);
    if (slot < nslots) {
        const uint4 *s = reinterpret_cast<const uint4 *>(regs + size_t(slot) * kHllFmtRegs);
#pragma unroll
        for (uint32_t k = 0; k < kHllFmtRegs / 16 / kT; k++) r.x[k] = s[k * kT + threadIdx.x];
    }
    return r;
}
__device__ __forceinline__ void store_row(const RowRegs &r, uint8_t *row) {
#pragma unroll
    for (uint32_t k = 0; k < kHllFmtRegs / 16 / kT; k++) {
        const uint32_t c = k * kT + threadIdx.x;  // registers 16c .. 16c + 15, inside one span
        uint32_t *d = reinterpret_cast<uint32_t *>(row + rpos(16 * c));
        d[0] = r.x[k].x, d[1] = r.x[k].y, d[2] = r.x[k].z, d[3] = r.x[k].w;
    }
}

// What a thread knows about its span after the scans.
struct EncSpan {
    uint32_t start;  // of the run its first register lies in (may lie in an earlier span)
    uint32_t end;    // of the run its last register lies in (may lie in a later span)
    uint64_t runs;   // bit k (1 .. 63): register k of the span differs from the one before it
    uint32_t bytes;  // sparse bytes its registers emit
    uint32_t big;    // a register above kHllFmtValMax: the key has no sparse form
};

// The bytes the registers [base, base + kHllFmtSpan) emit, run by run; kWrite:
// stored at dst[0 ..), else only counted.  S / runs / E as EncSpan's fields: the
// runs' ends come from the bit mask, so a run costs one LDS read (its value),
// at an address that depends on no earlier read.
template <bool kWrite>
__device__ __forceinline__ uint32_t enc_walk(const uint8_t *row, uint32_t base, uint32_t S, uint64_t runs, uint32_t E,
                                             uint8_t *dst) {
    const uint32_t lim = base + kHllFmtSpan;
    const uint8_t *r = row + rpos(base) - base;  // r[i]: register i of this span
    uint32_t n = 0, p = base;
    while (p < lim) {
        const uint32_t v = r[p];
        const uint32_t q = runs ? base + uint32_t(__builtin_ctzll(runs)) : lim;
        runs &= runs - 1;
        const uint32_t s = p == base ? S : p, e = q == lim ? E : q;
        uint8_t b[2];
        if (v == 0) {
            if (p == s) {  // the zero run starts here: its one opcode
                const uint32_t c = hll_fmt_emit(0, p, s, e, b);
                if (kWrite) {
                    dst[n] = b[0];
                    if (c == 2) dst[n + 1] = b[1];
                }
                n += c;
            }
        } else if (kWrite) {
            // the registers of [p, q) at a distance from s that is a multiple of 4
            for (uint32_t i = p + ((s - p) & (kHllFmtValLen - 1)); i < q; i += kHllFmtValLen) {
                hll_fmt_emit(v, i, s, e, b);
                dst[n++] = b[0];
            }
        } else {
            const uint32_t i0 = p + ((s - p) & (kHllFmtValLen - 1));
            if (i0 < q) n += (q - i0 + kHllFmtValLen - 1) / kHllFmtValLen;
        }
        p = q;
    }
    return n;
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
    return (x | ((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) & 0x80808080u;
}

// The two run scans and the byte count of this thread's span.  row: the key's
// registers in LDS (stored, and a barrier passed); sB / sA: kT words each.
__device__ __forceinline__ EncSpan enc_span(const uint8_t *row, uint32_t *wtmp, uint32_t *sB, uint32_t *sA) {
    const uint32_t tid = threadIdx.x, base = tid * kHllFmtSpan, lim = base + kHllFmtSpan;
    const uint32_t *x = reinterpret_cast<const uint32_t *>(row + rpos(base));
    // runs: where a register differs from the one before it; big: a byte above 32
    // (adding 95 sets its bit 7; a carry into the next byte takes a byte above 160,
    // which is big itself)
    uint64_t runs = 0;
    uint32_t big = 0, before = x[0] << 24;  // the byte before the word, in the top byte: register 0 meets itself
#pragma unroll
    for (uint32_t k = 0; k < kHllFmtSpan / 4; k++) {
        const uint32_t w = x[k];
        const uint32_t m = nonzero_bytes(w ^ ((w << 8) | (before >> 24)));
        runs |= uint64_t(((m >> 7) & 1) | ((m >> 14) & 2) | ((m >> 21) & 4) | ((m >> 28) & 8)) << (4 * k);
        big |= (w + 0x5F5F5F5Fu) & 0x80808080u;
        big |= w & 0x80808080u;
        before = w;
    }
    const uint32_t first = x[0] & 0xFF, last = before >> 24;
    // tail: where the span's last run starts; head: where its first run ends
    const uint32_t tail = runs ? base + 63 - uint32_t(__builtin_clzll(runs)) : base;
    const uint32_t head = runs ? base + uint32_t(__builtin_ctzll(runs)) : lim;
    const bool whole = runs == 0;  // one run covers the span
    const bool joins_left = tid > 0 && row[rpos(base - 1)] == first;
    const bool joins_right = tid + 1 < kT && row[rpos(lim)] == last;
    // B[t]: start of the run thread t's last register lies in = the latest
    // tail among the threads up to t that do not pass their left neighbour's on
    const uint32_t B = block_scan<false>(whole && joins_left ? 0u : tail, OpMax(), wtmp);
    // A[t]: end of the run thread t's first register lies in, the mirror image
    const uint32_t A = block_scan<true>(whole && joins_right ? 0xFFFFFFFFu : head, OpMin(), wtmp);
    sB[tid] = B;
    sA[tid] = A;
    __syncthreads();
    EncSpan sp;
    sp.start = joins_left ? sB[tid - 1] : base;
    sp.end = joins_right ? sA[tid + 1] : lim;
    sp.runs = runs;
    sp.big = big != 0;
    sp.bytes = enc_walk<false>(row, base, sp.start, runs, sp.end, nullptr);
    return sp;
}

constexpr uint32_t kStageBytes = 16 + kHllFmtHdr + kHllFmtMaxCanon + 16;  // shift, header, payload, slack

struct EncShared {
    __attribute__((aligned(16))) uint8_t row[kRowBytes];
    uint32_t sB[kT], sA[kT];
    uint32_t wtmp[kWaves];
    uint32_t total;
};

// payload bytes of the key in LDS row S.row (uniform over the workgroup), and
// whether they are the sparse form; *incl: this thread's inclusive byte offset
__device__ __forceinline__ uint32_t enc_key(EncShared &S, uint32_t smb, EncSpan *sp, uint32_t *incl, bool *sparse) {
    *sp = enc_span(S.row, S.wtmp, S.sB, S.sA);
    *incl = block_scan<false>(sp->bytes, OpAdd(), S.wtmp);
    if (threadIdx.x == kT - 1) S.total = *incl;
    const int big = __syncthreads_or(int(sp->big));  // also publishes S.total
    const uint32_t total = S.total;
    *sparse = !big && total <= smb;
    return *sparse ? total : kHllFmtDenseBytes;
}

__global__ void __launch_bounds__(kT, 4)
    k_hll_fmt_sizes(const uint8_t *__restrict__ regs, const uint32_t *__restrict__ slots, uint32_t nkeys,
                    uint32_t nslots, uint32_t smb, uint32_t *__restrict__ sizes) {
    __shared__ EncShared S;
    uint32_t key = blockIdx.x;
    RowRegs next;
    if (key < nkeys) next = fetch_row(regs, slots, key, nslots);
    for (; key < nkeys; key += gridDim.x) {
        store_row(next, S.row);
        if (key + gridDim.x < nkeys) next = fetch_row(regs, slots, key + gridDim.x, nslots);
        __syncthreads();
        EncSpan sp;
        uint32_t incl;
        bool sparse;
        const uint32_t payload = enc_key(S, smb, &sp, &incl, &sparse);
        if (threadIdx.x == 0) sizes[key] = kHllFmtHdr + payload;
        __syncthreads();  // S.row, S.total are read until here
    }
}

__global__ void __launch_bounds__(kT, 4)
    k_hll_fmt_dump(const uint8_t *__restrict__ regs, const uint32_t *__restrict__ slots, uint32_t nkeys,
                   uint32_t nslots, uint32_t smb, const uint64_t *__restrict__ card,
                   const uint32_t *__restrict__ offs, uint8_t *__restrict__ out) {
    __shared__ EncShared S;
    // the string, byte k at stage[a + k] with a = its global address mod 16:
    // 16-byte pieces of the LDS image and of memory line up
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStageBytes];
    const uint32_t tid = threadIdx.x;
    uint32_t key = blockIdx.x;
    RowRegs next;
    if (key < nkeys) next = fetch_row(regs, slots, key, nslots);
    for (; key < nkeys; key += gridDim.x) {
        const uint32_t slot = slots ? slots[key] : key;
        const uint32_t o0 = offs[key], o1 = offs[key + 1];
        const uint32_t len = o1 - o0;
        store_row(next, S.row);
        if (key + gridDim.x < nkeys) next = fetch_row(regs, slots, key + gridDim.x, nslots);
        __syncthreads();
        EncSpan sp;
        uint32_t incl;
        bool sparse;
        const uint32_t payload = enc_key(S, smb, &sp, &incl, &sparse);
        uint8_t *dst = out + o0;
        const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(dst) & 15);
        // the sizes launch saw the same row, so the lengths agree; a string of
        // another length is not written at all (no byte outside [o0, o1)), nor
        // one of a slot outside the slab (the call checked the list)
        if (slot < nslots && o1 >= o0 && len == kHllFmtHdr + payload) {
            if (tid == 0) hll_fmt_header(stage + a, sparse ? kHllFmtSparse : kHllFmtDense, card != nullptr,
                                         card ? card[key] : 0);
            uint8_t *pay = stage + a + kHllFmtHdr;
            if (sparse) {
                enc_walk<true>(S.row, tid * kHllFmtSpan, sp.start, sp.runs, sp.end, pay + (incl - sp.bytes));
            } else {
#pragma unroll 4
                for (uint32_t j = tid; j < kHllFmtRegs / 4; j += kT) {
                    const uint32_t w = *reinterpret_cast<const uint32_t *>(S.row + rpos(4 * j));
                    const uint32_t bits = hll_fmt_dense_pack(w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF, w >> 24);
                    pay[3 * j] = uint8_t(bits);
                    pay[3 * j + 1] = uint8_t(bits >> 8);
                    pay[3 * j + 2] = uint8_t(bits >> 16);
                }
            }
            __syncthreads();
            // memory [dst - a + lo, dst - a + hi) <- stage[lo, hi): whole 16-byte
            // pieces where both ends allow, single bytes before and after
            uint8_t *g = dst - a;
            const uint32_t lo = a, hi = a + len;
            const uint32_t flo = (lo + 15) & ~15u, fhi = hi & ~15u;
            if (flo >= fhi) {
                for (uint32_t x = lo + tid; x < hi; x += kT) g[x] = stage[x];
            } else {
                if (lo + tid < flo) g[lo + tid] = stage[lo + tid];
                if (fhi + tid < hi) g[fhi + tid] = stage[fhi + tid];
                for (uint32_t x = flo + 16 * tid; x < fhi; x += 16 * kT)
                    *reinterpret_cast<uint4 *>(g + x) = *reinterpret_cast<const uint4 *>(stage + x);
            }
        }
        __syncthreads();  // S and stage are read until here
    }
}

constexpr uint32_t kInBytes = 16 + kHllFmtHdr + kHllFmtMaxSparse + 16;  // shift, header, payload, slack

__global__ void __launch_bounds__(kT)
    k_hll_fmt_load(uint8_t *__restrict__ regs, const uint32_t *__restrict__ slots, uint32_t nkeys, uint32_t nslots,
                   const uint8_t *__restrict__ blob, const uint32_t *__restrict__ offs, uint8_t *__restrict__ status,
                   unsigned int *__restrict__ anybad) {
    __shared__ __attribute__((aligned(16))) uint8_t in[kInBytes];  // the string, byte k at in[a + k]
    __shared__ __attribute__((aligned(16))) uint8_t row[kHllFmtRegs];
    __shared__ uint32_t sZ[kT];
    __shared__ uint32_t wtmp[kWaves];
    __shared__ uint32_t total_s;
    const uint32_t tid = threadIdx.x;
    for (uint32_t key = blockIdx.x; key < nkeys; key += gridDim.x) {
        const uint32_t slot = slots ? slots[key] : key;
        const uint32_t o0 = offs[key], o1 = offs[key + 1];
        const uint32_t len = o1 > o0 ? o1 - o0 : 0;
        const uint8_t *src = blob + o0;
        const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(src) & 15);
        // every status below is decided from values all threads see alike
        uint32_t st = kHllFmtOk;
        if (len < kHllFmtHdr) {
            st = kHllFmtNotHll;
        } else {
            // the 16-byte pieces of memory that hold a byte of the string, at most
            // the header and the longest payload that can be valid
            const uint32_t take = len < kHllFmtHdr + kHllFmtMaxSparse ? len : kHllFmtHdr + kHllFmtMaxSparse;
            const uint8_t *g = src - a;
            for (uint32_t x = 16 * tid; x < a + take; x += 16 * kT)
                *reinterpret_cast<uint4 *>(in + x) = *reinterpret_cast<const uint4 *>(g + x);
            __syncthreads();
            const uint8_t *h = in + a;
            const uint32_t enc = h[4], n = len - kHllFmtHdr;
            const uint8_t *P = h + kHllFmtHdr;
            if (h[0] != 'H' || h[1] != 'Y' || h[2] != 'L' || h[3] != 'L') {
                st = kHllFmtNotHll;
            } else if (enc == kHllFmtDense) {
                int bad = 0;
                if (n != kHllFmtDenseBytes) {
                    st = kHllFmtCorrupt;
                } else {
#pragma unroll 4
                    for (uint32_t j = tid; j < kHllFmtRegs / 4; j += kT) {
                        const uint32_t bits = uint32_t(P[3 * j]) | uint32_t(P[3 * j + 1]) << 8 | uint32_t(P[3 * j + 2]) << 16;
                        uint32_t w = 0;
#pragma unroll
                        for (uint32_t k = 0; k < 4; k++) {
                            const uint32_t r = hll_fmt_dense_reg(bits, k);
                            bad |= r > 51;  // no register can exceed Q + 1
                            w |= r << (8 * k);
                        }
                        reinterpret_cast<uint32_t *>(row)[j] = w;
                    }
                    if (__syncthreads_or(bad)) st = kHllFmtCorrupt;
                }
            } else if (enc == kHllFmtSparse && n <= kHllFmtMaxSparse) {
                // this thread's stretch of the payload
                const uint32_t per = (n + kT - 1) / kT;
                const uint32_t j0 = tid * per < n ? tid * per : n, j1 = j0 + per < n ? j0 + per : n;
                uint32_t lz = 0;  // one past the last byte of the stretch that is not 01xxxxxx
                for (uint32_t j = j0; j < j1; j++)
                    if (!hll_fmt_is_x(P[j])) lz = j + 1;
                sZ[tid] = block_scan<false>(lz, OpMax(), wtmp);
                __syncthreads();
                const uint32_t zin = tid ? sZ[tid - 1] : 0;
                // pass 1: the registers the stretch's opcodes cover
                uint32_t sum = 0, nz = zin;
                int trunc = 0;
                for (uint32_t j = j0; j < j1; j++) {
                    const uint32_t b = P[j];
                    if (hll_fmt_is_start(j, nz)) {
                        if (hll_fmt_is_x(b) && j + 1 >= n) {
                            trunc = 1;  // an XZERO without its second byte
                        } else {
                            uint32_t val;
                            sum += hll_fmt_op(b, hll_fmt_is_x(b) ? P[j + 1] : 0, &val);
                        }
                    }
                    if (!hll_fmt_is_x(b)) nz = j + 1;
                }
                const uint32_t incl = block_scan<false>(sum, OpAdd(), wtmp);
                if (tid == kT - 1) total_s = incl;
                trunc = __syncthreads_or(trunc);  // also publishes total_s
                // every run is at least 1, so the runs pass no register past
                // 16384 and end there exactly when their sum is 16384
                if (trunc || total_s != kHllFmtRegs) {
                    st = kHllFmtCorrupt;
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < kHllFmtRegs / 16 / kT; k++)
                        reinterpret_cast<uint4 *>(row)[k * kT + tid] = make_uint4(0, 0, 0, 0);
                    __syncthreads();
                    // pass 2: every VAL opcode writes its (at most four) registers
                    uint32_t idx = incl - sum;
                    nz = zin;
                    for (uint32_t j = j0; j < j1; j++) {
                        const uint32_t b = P[j];
                        if (hll_fmt_is_start(j, nz)) {
                            uint32_t val;
                            const uint32_t run = hll_fmt_op(b, hll_fmt_is_x(b) ? P[j + 1] : 0, &val);
                            if (val)
                                for (uint32_t r = 0; r < run && idx + r < kHllFmtRegs; r++) row[idx + r] = uint8_t(val);
                            idx += run;
                        }
                        if (!hll_fmt_is_x(b)) nz = j + 1;
                    }
                }
            } else {
                st = kHllFmtCorrupt;  // an unknown encoding, or longer than any valid sparse payload
            }
        }
        __syncthreads();  // row is complete
        if (st == kHllFmtOk && slot < nslots) {
            uint4 *d = reinterpret_cast<uint4 *>(regs + size_t(slot) * kHllFmtRegs);
#pragma unroll
            for (uint32_t k = 0; k < kHllFmtRegs / 16 / kT; k++) d[k * kT + tid] = reinterpret_cast<const uint4 *>(row)[k * kT + tid];
        }
        if (tid == 0) {
            if (status) status[key] = uint8_t(st);
            if (st != kHllFmtOk) atomicOr(anybad, 1u);
        }
        __syncthreads();  // in, row are read until here
    }
}

// *bad |= 1 when offs[0 .. n] decreases somewhere
__global__ void __launch_bounds__(256) k_hll_fmt_offs_check(const uint32_t *__restrict__ offs, uint32_t n, unsigned int *bad) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
        if (offs[i + 1] < offs[i]) atomicOr(bad, 1u);
}

unsigned key_grid(uint32_t nkeys, int cus) {
    const unsigned cap = unsigned(cus) * 16;
    return nkeys < cap ? nkeys : cap;
}

}  // namespace

hipError_t launch_hll_fmt_sizes(const uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                                uint32_t smb, uint32_t *sizes, int cus, hipStream_t st) {
    if (nkeys == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hll_fmt_sizes, dim3(key_grid(nkeys, cus)), dim3(kT), 0, st, regs, slots, nkeys, nslots, smb,
                       sizes);
    return hipGetLastError();
}

hipError_t launch_hll_fmt_dump(const uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                               uint32_t smb, const uint64_t *card, const uint32_t *offs, uint8_t *out, int cus,
                               hipStream_t st) {
    if (nkeys == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hll_fmt_dump, dim3(key_grid(nkeys, cus)), dim3(kT), 0, st, regs, slots, nkeys, nslots, smb,
                       card, offs, out);
    return hipGetLastError();
}

hipError_t launch_hll_fmt_load(uint8_t *regs, const uint32_t *slots, uint32_t nkeys, uint32_t nslots,
                               const uint8_t *blob, const uint32_t *offs, uint8_t *status, unsigned int *anybad,
                               int cus, hipStream_t st) {
    if (nkeys == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hll_fmt_load, dim3(key_grid(nkeys, cus)), dim3(kT), 0, st, regs, slots, nkeys, nslots, blob,
                       offs, status, anybad);
    return hipGetLastError();
}

hipError_t launch_hll_fmt_offs_check(const uint32_t *offs, uint32_t n, unsigned int *bad, int cus, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_hll_fmt_offs_check, dim3(grid_for(n, 256, unsigned(cus) * 4)), dim3(256), 0, st, offs, n, bad);
    return hipGetLastError();
}

}  // namespace ske
