// Host-side check of the row log compaction's arithmetic
// (sketch_rows_compact.h): what a call removes, from the three numbers the
// front end yields, and the head's update as the end kernel applies it.  Built
// by tests/test_rows_compact_host.py with hipcc -Xarch_host
// -fsanitize=address,undefined (host code only, no GPU needed).
//
//   rowscompact_host counts <before>:<m>:<runs>...     per triple: "before kept superseded expired"
//   rowscompact_host head <used>:<taken>:<kept>...     per triple: "used taken"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../real-time-student-attendance-system_amd/csrc/sketch_rows_compact.h"

static bool triple(const char *arg, unsigned long long *v) {
    char *end = nullptr;
    for (int k = 0; k < 3; k++) {
        v[k] = strtoull(arg, &end, 10);
        if (end == arg || *end != (k < 2 ? ':' : '\0')) return false;
        arg = end + 1;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const bool counts = strcmp(argv[1], "counts") == 0;
    if (!counts && strcmp(argv[1], "head") != 0) return 2;
    for (int a = 2; a < argc; a++) {
        unsigned long long v[3];
        if (!triple(argv[a], v)) return 2;
        if (counts) {
            const ske::RowsCompactCounts c = ske::rows_compact_counts(v[0], v[1], v[2]);
            printf("%llu %llu %llu %llu\n", (unsigned long long)c.before, (unsigned long long)c.kept,
                   (unsigned long long)c.superseded, (unsigned long long)c.expired);
        } else {
            // the head's two words on the heap, exactly sized
            unsigned long long *h = (unsigned long long *)malloc(2 * sizeof(unsigned long long));
            h[0] = v[0], h[1] = v[1];
            ske::rows_compact_head(&h[0], &h[1], v[2]);
            printf("%llu %llu\n", h[0], h[1]);
            free(h);
        }
    }
    return 0;
}
