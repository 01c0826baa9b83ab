// sketch_api_tp.cpp -- libsketch C-ABI (include/sketch.h): time profiles, the
// weekday x hour counters of the swipes' times (init, reset, read, import, add),
// kernel in sketch_tp.hip.  A profile is SKE_TP_BINS u64 counters on the device,
// owned by the context and addressed by tid.
#include "sketch_ctx.h"

using namespace ske;

static_assert(kTpBins == SKE_TP_BINS, "sketch.h states the kernel's bin count");

static unsigned long long *counts_of(const Tp &P) { return reinterpret_cast<unsigned long long *>(P.base); }

extern "C" {

int ske_tp_init(ske_ctx *c, uint32_t tid) {
    Tp P;
    P.bytes = kTpBins * sizeof(unsigned long long);
    return obj_alloc(c, kTpFamily, c->tp, tid, P, [c](const Tp &N) { return obj_zero(N, N.bytes, c->st); });
}

int ske_tp_free(ske_ctx *c, uint32_t tid) { return obj_release(c, kTpFamily, c->tp, tid); }

int ske_tp_reset(ske_ctx *c, uint32_t tid) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = obj_for_sync_call(c, kTpFamily, c->tp, tid, "ske_tp_reset", &rc);
    if (!P) return rc;
    HIPCHK(c, obj_zero(*P, P->bytes, c->st));
    return SKE_OK;
}

int ske_tp_read(ske_ctx *c, uint32_t tid, uint64_t *out168) {
    if (!c || !out168) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = obj_for_sync_call(c, kTpFamily, c->tp, tid, "ske_tp_read", &rc, kTpFamily.info_refuses);
    if (!P) return rc;
    return obj_read_head(c, *P, out168, P->bytes);
}

int ske_tp_import(ske_ctx *c, uint32_t tid, const uint64_t *in168) {
    if (!c || !in168) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = obj_for_sync_call(c, kTpFamily, c->tp, tid, "ske_tp_import", &rc);
    if (!P) return rc;
    HIPCHK(c, hipMemcpyAsync(counts_of(*P), in168, kTpBins * sizeof(uint64_t), hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_tp_add_async(ske_ctx *c, uint32_t tid, const int64_t *epoch, uint64_t n, const uint8_t *mask, int want,
                     uint32_t late_from, uint8_t *late) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    Tp *P = obj_get(kTpFamily, c->tp, tid, &rc);
    if (!P) return rc;
    if ((want != 0 && want != 1) || late_from > 86400 || n >= 0xffffffffull) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (!epoch || (reinterpret_cast<uintptr_t>(epoch) & 7)) return SKE_EINVAL;
    TpArgs A{};
    A.counts = counts_of(*P);
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
