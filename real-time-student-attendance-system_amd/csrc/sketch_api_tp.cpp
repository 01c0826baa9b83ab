// sketch_api_tp.cpp -- libsketch C-ABI (include/sketch.h): time profiles, the
// weekday x hour counters of the swipes' times (init, reset, read, import, add),
// kernel in sketch_tp.hip.  A profile is SKE_TP_BINS u64 counters on the device,
// owned by the context and addressed by tid.
#include "sketch_ctx.h"

using namespace ske;

static_assert(kTpBins == SKE_TP_BINS, "sketch.h states the kernel's bin count");

namespace ske {

void free_tp(Tp &P) {
    if (P.counts) (void)hipFree(P.counts);
    P = Tp{};
}

}  // namespace ske

static Tp *get_tp(ske_ctx *c, uint32_t tid) { return tid < c->tp.size() && c->tp[tid].counts ? &c->tp[tid] : nullptr; }

// the profile of a tid in use for a call that waits for the stream (so it
// cannot be recorded); rc: why not
static Tp *tp_for_sync_call(ske_ctx *c, uint32_t tid, const char *what, int *rc) {
    if (tid >= SKE_MAX_TP) return *rc = SKE_EINVAL, nullptr;
    Tp *P = get_tp(c, tid);
    if (!P) return *rc = SKE_ETPNOSET, nullptr;
    if (c->capturing) {
        c->last_hip = std::string(what) + " waits for the stream and cannot be recorded";
        return *rc = SKE_EBUSY, nullptr;
    }
    return P;
}

extern "C" {

int ske_tp_init(ske_ctx *c, uint32_t tid) {
    if (!c || tid >= SKE_MAX_TP) return SKE_EINVAL;
    if (get_tp(c, tid)) return SKE_ETPEXISTS;
    if (c->tp.size() <= tid) c->tp.resize(SKE_MAX_TP);
    Tp P;
    hipError_t e = hipMalloc(&P.counts, kTpBins * sizeof(unsigned long long));
    if (e != hipSuccess) {
        c->last_hip = std::string("hipMalloc(tp): ") + hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    e = hipMemsetAsync(P.counts, 0, kTpBins * sizeof(unsigned long long), c->st);
    if (e == hipSuccess) e = hipStreamSynchronize(c->st);
    if (e != hipSuccess) {
        free_tp(P);
        c->last_hip = std::string("hipMemset(tp): ") + hipGetErrorString(e);
        return SKE_EHIP;
    }
    c->tp[tid] = P;
    return SKE_OK;
}

int ske_tp_free(ske_ctx *c, uint32_t tid) {
    if (!c || tid >= SKE_MAX_TP) return SKE_EINVAL;
    Tp *P = get_tp(c, tid);
    if (!P) return SKE_ETPNOSET;
    if (c->live_graphs > 0 || c->capturing) {
        c->last_hip = "a time profile cannot be freed while a recorded graph may point to it";
        return SKE_EBUSY;
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    free_tp(*P);
    return SKE_OK;
}

int ske_tp_reset(ske_ctx *c, uint32_t tid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = tp_for_sync_call(c, tid, "ske_tp_reset", &rc);
    if (!P) return rc;
    HIPCHK(c, hipMemsetAsync(P->counts, 0, kTpBins * sizeof(unsigned long long), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tp_read(ske_ctx *c, uint32_t tid, uint64_t *out168) {
    if (!c || !out168) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = tp_for_sync_call(c, tid, "ske_tp_read", &rc);
    if (!P) return rc;
    HIPCHK(c, hipMemcpyAsync(out168, P->counts, kTpBins * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tp_import(ske_ctx *c, uint32_t tid, const uint64_t *in168) {
    if (!c || !in168) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = tp_for_sync_call(c, tid, "ske_tp_import", &rc);
    if (!P) return rc;
    HIPCHK(c, hipMemcpyAsync(P->counts, in168, kTpBins * sizeof(uint64_t), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tp_add_async(ske_ctx *c, uint32_t tid, const int64_t *epoch, uint64_t n, const uint8_t *mask, int want,
                     uint32_t late_from, uint8_t *late) {
    if (!c || tid >= SKE_MAX_TP) return SKE_EINVAL;
    Tp *P = get_tp(c, tid);
    if (!P) return SKE_ETPNOSET;
    if ((want != 0 && want != 1) || late_from > 86400 || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!epoch || (reinterpret_cast<uintptr_t>(epoch) & 7)) return SKE_EINVAL;
    TpArgs A{};
    A.counts = P->counts;
    A.epoch = epoch;
    A.mask = mask;
    A.late = late;
    A.n = uint32_t(n);
    A.want = uint32_t(want);
    A.late_from = late_from;
    HIPCHK(c, launch_tp_add(A, c->tp_form, c->tp_grid ? unsigned(c->tp_grid) : unsigned(c->cus), c->st));
    return SKE_OK;
}

}  // extern "C"
