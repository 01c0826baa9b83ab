// Host-side check of the row-log arithmetic in sketch_common.h: the id rule
// (rows_parse_id: canonical decimal text that fits int64, from the text's three
// little-endian words) and the lecture digest (rows_lecture_digest: the tally's
// identity rule over a lecture of any length, 0 mapped to 1).  Built by
// tests/test_rows_host.py with hipcc -Xarch_host -fsanitize=address,undefined
// (host code only, no GPU needed).
//
//   rows_host id <hextext|->...       per text: "ok <value>" or "refused"
//   rows_host digest <hexbytes|->...  per lecture: its digest
//   rows_host word <u64>...           per word: rows_lecture_word
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../real-time-student-attendance-system_amd/csrc/sketch_common.h"

static bool parse_hex(const char *s, std::vector<uint8_t> *out) {
    out->clear();
    if (strcmp(s, "-") == 0) return true;
    const size_t n = strlen(s);
    if (n % 2) return false;
    for (size_t i = 0; i < n / 2; i++) {
        unsigned v = 0;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out->push_back(uint8_t(v));
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    std::vector<uint8_t> b;
    if (strcmp(argv[1], "id") == 0) {
        for (int a = 2; a < argc; a++) {
            if (!parse_hex(argv[a], &b)) return 2;
            // the kernel's view: the first 24 bytes as three little-endian words, zero padded
            uint8_t head[24] = {};
            if (!b.empty()) memcpy(head, b.data(), b.size() < sizeof head ? b.size() : sizeof head);
            uint64_t w[3];
            memcpy(w, head, sizeof w);
            int64_t v = 0;
            if (ske::rows_parse_id(w[0], w[1], w[2], uint32_t(b.size()), &v))
                printf("ok %lld\n", (long long)v);
            else
                printf("refused\n");
        }
        return 0;
    }
    if (strcmp(argv[1], "digest") == 0) {
        for (int a = 2; a < argc; a++) {
            if (!parse_hex(argv[a], &b)) return 2;
            // an exact-size copy: a read past the lecture's last byte is the sanitizer's to find
            uint8_t *p = (uint8_t *)malloc(b.size() ? b.size() : 1);
            if (!b.empty()) memcpy(p, b.data(), b.size());
            printf("%llu\n", (unsigned long long)ske::rows_lecture_digest(p, uint32_t(b.size())));
            free(p);
        }
        return 0;
    }
    if (strcmp(argv[1], "word") == 0) {
        for (int a = 2; a < argc; a++)
            printf("%llu\n", (unsigned long long)ske::rows_lecture_word(strtoull(argv[a], nullptr, 10)));
        return 0;
    }
    return 2;
}
