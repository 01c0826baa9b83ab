// sketch_hll_fmt.h -- the opcode rules of Redis' HyperLogLog strings
// (src/hyperloglog.c; formats.py restates them in Python), both directions,
// written per register and per byte so that no lane has to walk a string:
//
//   encode  a register emits 0, 1 or 2 bytes given the start and the end of its
//           run of equal registers (hll_fmt_emit);
//   decode  a byte starts an opcode iff an even number of 01xxxxxx bytes stands
//           directly before it (hll_fmt_is_start); an opcode's run and value
//           (hll_fmt_op);
//   dense   the 6-bit packing, four registers in three bytes.
//
// No device code of its own and no HIP runtime dependency: the kernels of
// sketch_hll_fmt.hip call these functions, and tests/native/hllfmt_host.cpp
// runs them serially over whole rows and strings on the host.  csrc-internal.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SKE_FMT_HD __host__ __device__ inline
#else
#define SKE_FMT_HD inline
#endif

namespace ske {

constexpr uint32_t kHllFmtRegs = 16384;          // registers of a key
constexpr uint32_t kHllFmtHdr = 16;              // "HYLL", encoding, 3 unused, 8 cardinality bytes
constexpr uint32_t kHllFmtDenseBytes = 12288;    // HLL_DENSE payload
constexpr uint32_t kHllFmtDense = 0, kHllFmtSparse = 1;  // the encoding byte
constexpr uint32_t kHllFmtValMax = 32;           // largest value a VAL opcode carries
constexpr uint32_t kHllFmtValLen = 4;            // longest VAL run
constexpr uint32_t kHllFmtZeroLen = 64;          // longest ZERO run; longer ones are XZERO
// the longest sparse payload that can be valid: every opcode covers at least
// one register in at most two bytes (16384 XZERO opcodes of run 1)
constexpr uint32_t kHllFmtMaxSparse = 2 * kHllFmtRegs;
// the longest payload the canonical encoder writes (alternating registers)
constexpr uint32_t kHllFmtMaxCanon = kHllFmtRegs;

// The kernels' tiling (one key per workgroup): a thread owns kHllFmtSpan
// consecutive registers, a wavefront 64 threads' worth, and the scans combine
// per-thread values inside a wavefront, then the wavefronts' totals.
constexpr uint32_t kHllFmtThreads = 256;
constexpr uint32_t kHllFmtSpan = kHllFmtRegs / kHllFmtThreads;  // 64
constexpr uint32_t kHllFmtWaveSpan = 64 * kHllFmtSpan;          // 4096

// status of a decoded key (ske_hll_load)
constexpr uint32_t kHllFmtOk = 0, kHllFmtNotHll = 1, kHllFmtCorrupt = 2;

// ---- encode: register i of value v, whose maximal run of equal registers is
// [start, end).  Returns the bytes it emits (0, 1 or 2) into b[0..1].
//   zero run of length L: its first register emits ZERO (L <= 64) or XZERO;
//   value run: the registers at distance 0, 4, 8, ... from the start emit one
//   VAL each, carrying min(4, end - i) registers.
SKE_FMT_HD uint32_t hll_fmt_emit(uint32_t v, uint32_t i, uint32_t start, uint32_t end, uint8_t *b) {
    if (v == 0) {
        if (i != start) return 0;
        const uint32_t l1 = end - start - 1;
        if (l1 < kHllFmtZeroLen) {
            b[0] = uint8_t(l1);
            return 1;
        }
        b[0] = uint8_t(0x40 | (l1 >> 8));
        b[1] = uint8_t(l1 & 0xFF);
        return 2;
    }
    if ((i - start) % kHllFmtValLen) return 0;
    const uint32_t left = end - i, n = left < kHllFmtValLen ? left : kHllFmtValLen;
    b[0] = uint8_t(0x80 | ((v - 1) << 2) | (n - 1));
    return 1;
}
// the same count without the bytes
SKE_FMT_HD uint32_t hll_fmt_emit_count(uint32_t v, uint32_t i, uint32_t start, uint32_t end) {
    if (v == 0) return i != start ? 0 : (end - start > kHllFmtZeroLen ? 2 : 1);
    return (i - start) % kHllFmtValLen ? 0 : 1;
}

// the header: card_valid == false writes the invalid-cache mark
SKE_FMT_HD void hll_fmt_header(uint8_t *h, uint32_t enc, bool card_valid, uint64_t card) {
    h[0] = 'H', h[1] = 'Y', h[2] = 'L', h[3] = 'L';
    h[4] = uint8_t(enc);
    h[5] = h[6] = h[7] = 0;
    if (!card_valid) card = uint64_t(1) << 63;      // HLL_INVALIDATE_CACHE: bit 7 of byte 15
    else card &= (uint64_t(1) << 63) - 1;
    for (int k = 0; k < 8; k++) h[8 + k] = uint8_t(card >> (8 * k));
}

// ---- decode
SKE_FMT_HD bool hll_fmt_is_x(uint32_t byte) { return (byte & 0xC0) == 0x40; }  // 01xxxxxx
// Byte j starts an opcode iff the 01xxxxxx bytes directly before it are even
// in number.  nonx_end: one past the last byte before j that is not 01xxxxxx
// (0 when there is none), so j - nonx_end such bytes stand before j: the first
// of them is a start (it follows a byte that ends an opcode either way), and
// from there XZERO opcodes and their second bytes alternate.
SKE_FMT_HD bool hll_fmt_is_start(uint32_t j, uint32_t nonx_end) { return ((j - nonx_end) & 1) == 0; }
// run and value (0 for the zero opcodes) of the opcode whose first byte is b0;
// b1: the byte after it (read only for XZERO: the caller checks that it exists)
SKE_FMT_HD uint32_t hll_fmt_op(uint32_t b0, uint32_t b1, uint32_t *val) {
    if (b0 & 0x80) {
        *val = ((b0 >> 2) & 0x1F) + 1;
        return (b0 & 3) + 1;
    }
    *val = 0;
    if (b0 & 0x40) return (((b0 & 0x3F) << 8) | b1) + 1;
    return (b0 & 0x3F) + 1;
}

// ---- dense: registers 4j .. 4j+3 <-> the 24 bits of bytes 3j .. 3j+2
SKE_FMT_HD uint32_t hll_fmt_dense_pack(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
    return (r0 & 63) | ((r1 & 63) << 6) | ((r2 & 63) << 12) | ((r3 & 63) << 18);
}
SKE_FMT_HD uint32_t hll_fmt_dense_reg(uint32_t bits, uint32_t k) { return (bits >> (6 * k)) & 63; }

}  // namespace ske
