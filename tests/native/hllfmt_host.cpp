// hllfmt_host.cpp -- the opcode rules of csrc/sketch_hll_fmt.h run serially on
// the host over whole register rows and whole strings: what the kernels of
// sketch_hll_fmt.hip compute per thread, without a device.  Stand-alone (its
// own main), so it can also be built with -fsanitize=address,undefined.
//
//   hllfmt_host enc IN OUT SMB [CARD]   IN: rows of 16384 register bytes.  OUT: per row a
//                                       u32 length and the "HYLL" string (sparse payloads up
//                                       to SMB bytes; CARD: the cached cardinality, else invalid)
//   hllfmt_host dec IN OUT              IN: a u32 count, then per string a u32 length and its
//                                       bytes.  OUT: per string a status byte (0 loaded, 1 not
//                                       an HLL string, 2 corrupted) and 16384 registers
//   hllfmt_host spans                   prints the kernels' tiling constants
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../real-time-student-attendance-system_amd/csrc/sketch_hll_fmt.h"

using namespace ske;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(2);
    }
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

static void put_u32(std::vector<uint8_t> &o, uint32_t x) {
    for (int k = 0; k < 4; k++) o.push_back(uint8_t(x >> (8 * k)));
}

static std::vector<uint8_t> encode(const uint8_t *r, uint32_t smb, bool card_valid, uint64_t card) {
    // the two segmented scans: start and end of every register's run
    std::vector<uint32_t> start(kHllFmtRegs), end(kHllFmtRegs);
    for (uint32_t i = 0; i < kHllFmtRegs; i++) start[i] = (i && r[i] == r[i - 1]) ? start[i - 1] : i;
    for (uint32_t i = kHllFmtRegs; i-- > 0;) end[i] = (i + 1 < kHllFmtRegs && r[i] == r[i + 1]) ? end[i + 1] : i + 1;
    uint32_t total = 0, mx = 0;
    for (uint32_t i = 0; i < kHllFmtRegs; i++) {
        total += hll_fmt_emit_count(r[i], i, start[i], end[i]);
        if (r[i] > mx) mx = r[i];
    }
    const bool sparse = mx <= kHllFmtValMax && total <= smb;
    std::vector<uint8_t> s(kHllFmtHdr + (sparse ? total : kHllFmtDenseBytes));
    hll_fmt_header(s.data(), sparse ? kHllFmtSparse : kHllFmtDense, card_valid, card);
    if (sparse) {
        uint32_t at = kHllFmtHdr;
        for (uint32_t i = 0; i < kHllFmtRegs; i++) {
            uint8_t b[2];
            const uint32_t c = hll_fmt_emit(r[i], i, start[i], end[i], b);
            if (c != hll_fmt_emit_count(r[i], i, start[i], end[i])) {
                fprintf(stderr, "emit and emit_count disagree at register %u\n", i);
                exit(3);
            }
            for (uint32_t k = 0; k < c; k++) s.at(at++) = b[k];
        }
        if (at != s.size()) {
            fprintf(stderr, "wrote %u of %zu bytes\n", at, s.size());
            exit(3);
        }
    } else {
        for (uint32_t j = 0; j < kHllFmtRegs / 4; j++) {
            const uint32_t bits = hll_fmt_dense_pack(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3]);
            for (uint32_t k = 0; k < 3; k++) s.at(kHllFmtHdr + 3 * j + k) = uint8_t(bits >> (8 * k));
        }
    }
    return s;
}

static uint32_t decode(const uint8_t *s, uint32_t len, uint8_t *regs) {
    if (len < kHllFmtHdr || memcmp(s, "HYLL", 4) != 0) return kHllFmtNotHll;
    const uint8_t *p = s + kHllFmtHdr;
    const uint32_t n = len - kHllFmtHdr, enc = s[4];
    if (enc == kHllFmtDense) {
        if (n != kHllFmtDenseBytes) return kHllFmtCorrupt;
        for (uint32_t j = 0; j < kHllFmtRegs / 4; j++) {
            const uint32_t bits = uint32_t(p[3 * j]) | uint32_t(p[3 * j + 1]) << 8 | uint32_t(p[3 * j + 2]) << 16;
            for (uint32_t k = 0; k < 4; k++) {
                regs[4 * j + k] = uint8_t(hll_fmt_dense_reg(bits, k));
                if (regs[4 * j + k] > 51) return kHllFmtCorrupt;
            }
        }
        return kHllFmtOk;
    }
    if (enc != kHllFmtSparse || n > kHllFmtMaxSparse) return kHllFmtCorrupt;
    // pass 1: the registers the opcodes cover; pass 2 writes them
    uint64_t total = 0;
    uint32_t nonx_end = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (hll_fmt_is_start(j, nonx_end)) {
            if (hll_fmt_is_x(p[j]) && j + 1 >= n) return kHllFmtCorrupt;
            uint32_t val;
            total += hll_fmt_op(p[j], hll_fmt_is_x(p[j]) ? p[j + 1] : 0, &val);
        }
        if (!hll_fmt_is_x(p[j])) nonx_end = j + 1;
    }
    if (total != kHllFmtRegs) return kHllFmtCorrupt;
    uint32_t idx = 0;
    nonx_end = 0;
    for (uint32_t j = 0; j < n; j++) {
        if (hll_fmt_is_start(j, nonx_end)) {
            uint32_t val;
            const uint32_t run = hll_fmt_op(p[j], hll_fmt_is_x(p[j]) ? p[j + 1] : 0, &val);
            if (idx + run > kHllFmtRegs) {
                fprintf(stderr, "a run passes the last register although the runs sum to it\n");
                exit(3);
            }
            if (val) memset(regs + idx, int(val), run);
            idx += run;
        }
        if (!hll_fmt_is_x(p[j])) nonx_end = j + 1;
    }
    return kHllFmtOk;
}

static void write_file(const char *path, const std::vector<uint8_t> &o) {
    FILE *f = fopen(path, "wb");
    if (!f || fwrite(o.data(), 1, o.size(), f) != o.size()) {
        perror(path);
        exit(2);
    }
    fclose(f);
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "spans") {
        printf("threads %u\nspan %u\nwave %u\n", kHllFmtThreads, kHllFmtSpan, kHllFmtWaveSpan);
        return 0;
    }
    if (mode == "enc" && argc >= 5) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        const uint32_t smb = uint32_t(strtoul(argv[4], nullptr, 10));
        const bool card_valid = argc > 5;
        const uint64_t card = card_valid ? strtoull(argv[5], nullptr, 10) : 0;
        if (in.size() % kHllFmtRegs) {
            fprintf(stderr, "%s: not whole rows\n", argv[2]);
            return 2;
        }
        std::vector<uint8_t> out;
        for (size_t r = 0; r < in.size() / kHllFmtRegs; r++) {
            const std::vector<uint8_t> s = encode(in.data() + r * kHllFmtRegs, smb, card_valid, card);
            put_u32(out, uint32_t(s.size()));
            out.insert(out.end(), s.begin(), s.end());
        }
        write_file(argv[3], out);
        return 0;
    }
    if (mode == "dec" && argc >= 4) {
        const std::vector<uint8_t> in = read_file(argv[2]);
        auto u32_at = [&](size_t at) {
            if (at + 4 > in.size()) {
                fprintf(stderr, "%s: truncated\n", argv[2]);
                exit(2);
            }
            return uint32_t(in[at]) | uint32_t(in[at + 1]) << 8 | uint32_t(in[at + 2]) << 16 | uint32_t(in[at + 3]) << 24;
        };
        const uint32_t count = u32_at(0);
        size_t at = 4;
        std::vector<uint8_t> out;
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t len = u32_at(at);
            at += 4;
            if (at + len > in.size()) {
                fprintf(stderr, "%s: truncated\n", argv[2]);
                return 2;
            }
            // an exact-size copy: a read past the string's end is a read past an allocation
            const std::vector<uint8_t> s(in.begin() + at, in.begin() + at + len);
            at += len;
            std::vector<uint8_t> regs(kHllFmtRegs, 0);
            const uint32_t st = decode(s.data(), len, regs.data());
            if (st != kHllFmtOk) std::fill(regs.begin(), regs.end(), 0);
            out.push_back(uint8_t(st));
            out.insert(out.end(), regs.begin(), regs.end());
        }
        write_file(argv[3], out);
        return 0;
    }
    fprintf(stderr, "usage: hllfmt_host enc IN OUT SMB [CARD] | dec IN OUT | spans\n");
    return 2;
}
