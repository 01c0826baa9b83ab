// Host-side check of the seen-row arithmetic in sketch_common.h: the fold of a
// column of at most 16 bytes from its two zero-padded words (seen_fold_words),
// the time column's bucket by floor division (seen_bucket, seen_fold_epoch), the
// 0-to-1 remap (seen_word), the probe start (seen_start) and the limit
// (seen_limit).  Built by tests/test_seen_host.py with hipcc -Xarch_host
// -fsanitize=address,undefined (host code only, no GPU needed).
//
//   seen_host fold <hexcol|->...        the key after folding the columns in order from the seeds:
//                                       one line "<k0> <k1>" after each column
//   seen_host epoch <gran> <epoch>...   per epoch: "<bucket> <k0> <k1>", the key = the seeds folded once
//   seen_host word <u64>...             per word: seen_word
//   seen_host limit <log2>...           per log2: "<capacity> <limit> <start of k0 = 2^64 - 1>"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../real-time-student-attendance-system_amd/csrc/sketch_common.h"

static bool parse_hex(const char *s, uint8_t (&col)[16], uint32_t *len) {
    memset(col, 0, sizeof col);
    *len = 0;
    if (strcmp(s, "-") == 0) return true;
    const size_t n = strlen(s);
    if (n % 2 || n / 2 > 16) return false;
    for (size_t i = 0; i < n / 2; i++) {
        unsigned v = 0;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        col[i] = uint8_t(v);
    }
    *len = uint32_t(n / 2);
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (strcmp(argv[1], "fold") == 0) {
        ske::SeenKey k = ske::seen_begin();
        for (int a = 2; a < argc; a++) {
            uint8_t col[16];
            uint32_t len;
            if (!parse_hex(argv[a], col, &len)) return 2;
            uint64_t w[2];
            memcpy(w, col, sizeof w);  // little-endian words: the column bytes in order, zero padded
            k = ske::seen_fold_words(k, w[0], w[1], len);
            printf("%llu %llu\n", (unsigned long long)k.k0, (unsigned long long)k.k1);
        }
        return 0;
    }
    if (strcmp(argv[1], "epoch") == 0 && argc >= 3) {
        const int64_t gran = strtoll(argv[2], nullptr, 10);
        if (gran < 1) return 2;
        for (int a = 3; a < argc; a++) {
            const int64_t e = strtoll(argv[a], nullptr, 10);
            const ske::SeenKey k = ske::seen_fold_epoch(ske::seen_begin(), e, gran);
            printf("%lld %llu %llu\n", (long long)ske::seen_bucket(e, gran), (unsigned long long)k.k0,
                   (unsigned long long)k.k1);
        }
        return 0;
    }
    if (strcmp(argv[1], "word") == 0) {
        for (int a = 2; a < argc; a++)
            printf("%llu\n", (unsigned long long)ske::seen_word(strtoull(argv[a], nullptr, 10)));
        return 0;
    }
    if (strcmp(argv[1], "limit") == 0) {
        for (int a = 2; a < argc; a++) {
            const uint32_t log2 = uint32_t(atoi(argv[a]));
            printf("%llu %llu %u\n", (unsigned long long)(uint64_t(1) << log2),
                   (unsigned long long)ske::seen_limit(log2), ske::seen_start(~uint64_t(0), log2));
        }
        return 0;
    }
    return 2;
}
