// sketch_api_ctx.cpp -- libsketch C-ABI (include/sketch.h): the context's
// lifecycle, options, the sticky error word, streams, host -> device staging,
// pass timing, the scratch-use ordering and graph capture.  The other
// subsystems are sketch_api_{bloom,hll,swipes,ingest,cms,hh,tp,tally,seen,rows}.cpp (map: sketch_ctx.h).
#include <stdlib.h>
#include <string.h>

#include "sketch_ctx.h"

using namespace ske;

namespace ske {

// ---- staging
void *stage_buf(ske_ctx *c, StageSlot slot, size_t bytes, int *rc) {
    if (bytes < 64) bytes = 64;
    if (c->stg_cap[slot] < bytes) {
        if (c->stg[slot]) (void)hipFree(c->stg[slot]);
        c->stg[slot] = nullptr;
        c->stg_cap[slot] = 0;
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&c->stg[slot], want);
        if (e != hipSuccess) {
            c->last_hip = std::string("hipMalloc(staging): ") + hipGetErrorString(e);
            *rc = SKE_ENOMEM;
            return nullptr;
        }
        c->stg_cap[slot] = want;
    }
    return c->stg[slot];
}

int stage_items(ske_ctx *c, const uint8_t *bytes, const uint32_t *offs, uint64_t n, int mem, Staged *out) {
    if (mem == SKE_MEM_DEVICE) {
        out->bytes = bytes;
        out->offs = offs;
        return SKE_OK;
    }
    if (!offs || (!bytes && offs[n] != offs[0]) || offs[n] < offs[0]) return SKE_EINVAL;
    const uint64_t b0 = offs[0], total = uint64_t(offs[n]) - b0;
    int rc = SKE_OK;
    uint8_t *db = (uint8_t *)stage_buf(c, kStgBytes, total + 16, &rc);
    uint32_t *dof = (uint32_t *)stage_buf(c, kStgOffs, (n + 1) * 4, &rc);
    if (rc) return rc;
    if (!c->hs) c->hs = stager_new();
    // the offsets are checked (never decreasing) as they are copied; no
    // kernel reads them before this returns
    // (bytes first: a direct offsets copy is checked while both DMAs run)
    bool ok = true;
    if (total) HIPCHK(c, stage_h2d(c->hs, db, bytes + b0, total, c->st, false, nullptr));
    HIPCHK(c, stage_h2d(c->hs, dof, offs, (n + 1) * 4, c->st, true, &ok));
    if (!ok) {
        HIPCHK(c, hipStreamSynchronize(c->st));  // the copies may still read the caller's buffers
        return SKE_EINVAL;
    }
    out->bytes = db - b0;
    out->offs = dof;
    return SKE_OK;
}

int stage_u32(ske_ctx *c, const uint32_t *p, uint64_t n, int mem, StageSlot slot, const uint32_t **out) {
    if (mem == SKE_MEM_DEVICE || n == 0) {
        *out = p;
        return SKE_OK;
    }
    int rc = SKE_OK;
    uint32_t *d = (uint32_t *)stage_buf(c, slot, n * 4, &rc);
    if (rc) return rc;
    if (!c->hs) c->hs = stager_new();
    HIPCHK(c, stage_h2d(c->hs, d, p, n * 4, c->st, false, nullptr));
    *out = d;
    return SKE_OK;
}

// ---- pass timing
static hipEvent_t ev_get(ske_ctx *c) {
    if (!c->ev_pool.empty()) {
        hipEvent_t e = c->ev_pool.back();
        c->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

// a mark's events back to the pool (a shared start event is its first owner's)
static void mark_recycle(ske_ctx *c, const ske_ctx::Mark &m) {
    if (m.own_a) c->ev_pool.push_back(m.a);
    c->ev_pool.push_back(m.b);
}

void PassMark::begin(ske_ctx *c, int pass, hipStream_t st, hipEvent_t start) {
    abandon();
    b_ = nullptr;
    if (!c->timing || c->capturing) return;
    hipEvent_t a = start ? start : ev_get(c), b = ev_get(c);
    if (!a || !b || (!start && hipEventRecord(a, st) != hipSuccess)) {
        if (a && !start) c->ev_pool.push_back(a);
        if (b) c->ev_pool.push_back(b);
        return;
    }
    idx_ = c->marks.size();
    c->marks.push_back({pass, a, b, start == nullptr});
    c_ = c;
    b_ = b;
    st_ = st;
    open_ = true;
}

void PassMark::end() {
    if (!open_) return;
    open_ = false;
    if (hipEventRecord(b_, st_) != hipSuccess) c_->marks[idx_].pass = -1;
}

void PassMark::abandon() {
    if (!open_) return;
    open_ = false;
    (void)hipEventRecord(b_, st_);
    for (size_t i = idx_; i < c_->marks.size(); i++) c_->marks[i].pass = -1;
    b_ = nullptr;
}

// ---- the scratch-use ordering
//
// A ScratchUse's done event is recorded lazily: only when a use on another stream needs it (or
// ske_set_stream leaves the stream), not after every call -- a marker packet
// per call costs ~6 us of GPU time between back-to-back steps.  Recording it
// later on its stream still covers the last use (it covers everything enqueued
// there so far).  A stream whose capture state changed since that use needs
// no wait: recording a graph starts from a synchronised stream.
static unsigned long long capture_id(hipStream_t st, hipError_t *e) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    unsigned long long cid = 0;
    *e = hipStreamGetCaptureInfo(st, &cs, &cid);
    return cs == hipStreamCaptureStatusActive ? cid : 0;
}

// cover u.stream's last scratch use by u.done (false: no wait is needed)
static int xr_flush(ske_ctx *c, ScratchUse &u, bool *covered) {
    *covered = false;
    if (!u.stream) return SKE_OK;
    if (!u.pending) {
        *covered = true;
        return SKE_OK;
    }
    hipError_t e = hipSuccess;
    const unsigned long long now = capture_id(u.stream, &e);
    HIPCHK(c, e);
    u.pending = false;
    if (now != u.cap) {
        u.stream = nullptr;
        return SKE_OK;
    }
    HIPCHK(c, hipEventRecord(u.done, u.stream));
    *covered = true;
    return SKE_OK;
}

static int scratch_user_begin(ske_ctx *c, ScratchUse &u, hipStream_t st, unsigned long long *cid_out) {
    if (!u.done) HIPCHK(c, hipEventCreateWithFlags(&u.done, hipEventDisableTiming));
    hipError_t e = hipSuccess;
    const unsigned long long cid = capture_id(st, &e);
    HIPCHK(c, e);
    if (u.stream && u.stream != st && u.cap == cid) {
        bool covered = false;
        const int rc = xr_flush(c, u, &covered);
        if (rc) return rc;
        if (covered) HIPCHK(c, hipStreamWaitEvent(st, u.done, 0));
    }
    *cid_out = cid;
    return SKE_OK;
}

// the bit of a group in ske_ctx::cap_users / graph_users
static unsigned scratch_use_bit(const ske_ctx *c, const ScratchUse *u) {
    return u == &c->rw ? 8u : u == &c->sn ? 4u : u == &c->rt ? 2u : 1u;
}

ScratchUser::ScratchUser(ske_ctx *c, ScratchUse &u, hipStream_t st) : c_(c), u_(u), st_(st) {
    rc = scratch_user_begin(c, u, st, &cid_);
}

ScratchUser::~ScratchUser() {
    if (rc) return;
    if (cid_) c_->cap_users |= scratch_use_bit(c_, &u_);
    u_.stream = st_;
    u_.cap = cid_;
    u_.pending = true;
}

int scratch_error(ske_ctx *c, hipError_t e) {
    if (e == hipErrorStreamCaptureUnsupported) {
        c->last_hip = "scratch too small while a graph is recorded or alive: run the same call "
                      "(same or larger batch) once before recording, or free the graphs";
        return SKE_EBUSY;
    }
    c->last_hip = hipGetErrorString(e);
    return SKE_ENOMEM;
}

}  // namespace ske

// ---- the error word
//
// The device error word err[0] is sticky: kernels only ever set it (a valid
// swipe naming a slot outside the slab).  It is read and cleared only by
// device-side exchanges (atomicExch), so a flag set by a kernel on any stream
// is never lost between a read and a clear:
//   * a synchronous call (K1, PFADD, ingest) first takes what earlier
//     enqueue-only calls left into err[kErrPrior] (k_err_begin, OR-ed), and at
//     its end takes its own flag into the report word (k_err_end); the prior
//     flag is then held on the host (c->err_pending) for the next ske_sync /
//     ske_check_errors -- a synchronous call reports only its own slots;
//   * ske_sync / ske_check_errors report everything not yet reported.
namespace {

constexpr int kErrPrior = 16, kErrOut = 32;  // word offsets in c->err (64 words)

__global__ void k_err_begin(unsigned int *err) {
    const unsigned int v = atomicExch(err, 0u);
    if (v) atomicOr(err + kErrPrior, v);
}
// out[0] = the prior word (then cleared), out[1] = the live word (then cleared)
__global__ void k_err_end(unsigned int *err) {
    err[kErrOut] = atomicExch(err + kErrPrior, 0u);
    err[kErrOut + 1] = atomicExch(err, 0u);
}

}  // namespace

namespace ske {

int err_begin(ske_ctx *c) {
    hipLaunchKernelGGL(k_err_begin, dim3(1), dim3(1), 0, c->st, c->err);
    HIPCHK(c, hipGetLastError());
    return SKE_OK;
}

// the two words after this call's work: {earlier enqueue-only calls, this call}
static int err_end(ske_ctx *c, unsigned int h[2]) {
    hipLaunchKernelGGL(k_err_end, dim3(1), dim3(1), 0, c->st, c->err);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h, c->err + kErrOut, 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

// end of a synchronous call that did err_begin(): its own slot errors only
int check_call_err(ske_ctx *c) {
    unsigned int h[2] = {0, 0};
    const int rc = err_end(c, h);
    if (rc) return rc;
    if (h[0]) c->err_pending = true;
    return h[1] ? SKE_ERANGE : SKE_OK;
}

// ske_sync / ske_check_errors: everything not yet reported
static int check_err_flag(ske_ctx *c, int code_if_set) {
    unsigned int h[2] = {0, 0};
    const int rc = err_end(c, h);
    if (rc) return rc;
    const bool set = h[0] || h[1] || c->err_pending;
    c->err_pending = false;
    return set ? code_if_set : SKE_OK;
}

}  // namespace ske

extern "C" {

const char *ske_strerror(int code) {
    switch (code) {
    case SKE_OK: return "OK";
    case SKE_EINVAL: return "ERR invalid argument";
    case SKE_ENOMEM: return "ERR out of device memory";
    case SKE_EHIP: return "ERR HIP runtime error";
    case SKE_ENOFILTER: return "ERR not found";
    case SKE_EEXISTS: return "ERR item exists";
    case SKE_EFULL: return "ERR non scaling filter is full";
    case SKE_ERANGE: return "ERR HLL slot out of range";
    case SKE_EBADRATE: return "ERR (0 < error rate range < 1)";
    case SKE_EBADCAP: return "ERR (capacity should be larger than 0)";
    case SKE_EBADEXP: return "ERR expansion should be greater or equal to 1";
    case SKE_EBADHLL: return "INVALIDOBJ Corrupted HLL object detected";
    case SKE_ETOOLONG: return "ERR item too long";
    case SKE_EBUSY: return "ERR device buffers in use by a recorded graph";
    // RedisBloom's Count-Min Sketch texts (src/rm_cms.c)
    case SKE_ECMSNOKEY: return "CMS: key does not exist";
    case SKE_ECMSEXISTS: return "CMS: key already exists";
    case SKE_ECMSWIDTH: return "CMS: invalid width";
    case SKE_ECMSDEPTH: return "CMS: invalid depth";
    case SKE_ECMSDIMS: return "CMS: width/depth is not equal";
    case SKE_ECMSNEG: return "CMS: Number cannot be negative";
    case SKE_ECMSOVERFLOW: return "CMS: MERGE overflow";
    case SKE_ECMSERROR: return "CMS: invalid overestimation value";
    case SKE_ECMSPROB: return "CMS: invalid prob value";
    case SKE_ECMSPARSE: return "CMS: Cannot parse number";
    case SKE_EHHNOSET: return "ERR heavy-hitter set does not exist";
    case SKE_EHHEXISTS: return "ERR heavy-hitter set already exists";
    case SKE_EHHCAP: return "ERR heavy-hitter capacity out of range";
    case SKE_EHHSPACE: return "ERR heavy-hitter list does not fit the output";
    case SKE_ETPNOSET: return "ERR time profile does not exist";
    case SKE_ETPEXISTS: return "ERR time profile already exists";
    case SKE_ETALLYNOSET: return "ERR tally does not exist";
    case SKE_ETALLYEXISTS: return "ERR tally already exists";
    case SKE_ETALLYCAP: return "ERR tally capacity out of range";
    case SKE_ETALLYSPACE: return "ERR tally list does not fit the output";
    case SKE_ESEENNOSET: return "ERR seen set does not exist";
    case SKE_ESEENEXISTS: return "ERR seen set already exists";
    case SKE_ESEENCAP: return "ERR seen set capacity out of range";
    case SKE_ESEENCALLS: return "ERR seen set has run out of call numbers";
    case SKE_EROWSNOLOG: return "ERR row log does not exist";
    case SKE_EROWSEXISTS: return "ERR row log already exists";
    case SKE_EROWSCAP: return "ERR row log capacity out of range";
    case SKE_EROWSSPACE: return "ERR row log selection does not fit the output";
    default: return "ERR unknown";
    }
}

const char *ske_last_hip_error(ske_ctx *c) { return c ? c->last_hip.c_str() : ""; }

int ske_open(int device, ske_ctx **out) {
    if (!out) return SKE_EINVAL;
    *out = nullptr;
    ske_ctx *c = new ske_ctx();
    c->device = device;
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) {
        delete c;
        return SKE_EHIP;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return SKE_EHIP;
    }
    c->st = c->own;
    c->filters.resize(SKE_MAX_FILTERS);
    c->scratch = scratch_new();
    if (hipMalloc(&c->err, 256) != hipSuccess || hipMalloc(&c->stats, 64) != hipSuccess ||
        hipMemset(c->err, 0, 256) != hipSuccess) {
        ske_close(c);
        return SKE_ENOMEM;
    }
    c->lds_ok = lds_bloom_setup() == hipSuccess;
    c->k1_ok = c->lds_ok && k1_lds_setup() == hipSuccess;
    if (const char *v = getenv("SKE_CMS_LDS_CELLS")) {
        const unsigned long long cells = strtoull(v, nullptr, 10);
        if (cells < c->cms_lds_cells) c->cms_lds_cells = uint32_t(cells);
    }
    if (const char *v = getenv("SKE_HH_LDS_CELLS")) {
        const unsigned long long cells = strtoull(v, nullptr, 10);
        c->hh_lds_cells = cells < kCmsLdsCells ? uint32_t(cells) : kCmsLdsCells;
    }
    if (const char *v = getenv("SKE_TP_GRID")) {
        const unsigned long long grid = strtoull(v, nullptr, 10);
        c->tp_grid = int(grid < kTpMaxGrid ? grid : kTpMaxGrid);
    }
    if (const char *v = getenv("SKE_INGEST_GRID")) {
        const unsigned long long grid = strtoull(v, nullptr, 10);
        c->ingest_grid = int(grid < 65536 ? grid : 65536);
    }
    if (const char *v = getenv("SKE_TP_FORM")) c->tp_form = strtoull(v, nullptr, 10) == 1 ? 1 : 0;
    if (const char *v = getenv("SKE_TALLY_FORM")) c->tally_form = strtoull(v, nullptr, 10) == 1 ? 1 : 0;
    if (const char *v = getenv("SKE_TALLY_GRID")) {
        const unsigned long long grid = strtoull(v, nullptr, 10);
        c->tally_grid = int(grid < kTallyMaxGrid ? grid : kTallyMaxGrid);
    }
    if (const char *v = getenv("SKE_TALLY_LDS_LOG2")) {
        const unsigned long long l = strtoull(v, nullptr, 10);
        c->tally_lds_log2 = l < kTallyLdsMinLog2 ? kTallyLdsMinLog2 : l > kTallyLdsMaxLog2 ? kTallyLdsMaxLog2 : int(l);
    }
    if (const char *v = getenv("SKE_SEEN_GRID")) {
        const unsigned long long grid = strtoull(v, nullptr, 10);
        c->seen_grid = int(grid < kSeenMaxGrid ? grid : kSeenMaxGrid);
    }
    if (const char *v = getenv("SKE_ROWS_GRID")) {
        const unsigned long long grid = strtoull(v, nullptr, 10);
        c->rows_grid = int(grid < kRowsMaxGrid ? grid : kRowsMaxGrid);
    }
    if (hipMalloc(&c->zero16, 64) != hipSuccess || hipMemset(c->zero16, 0, 64) != hipSuccess) {
        ske_close(c);
        return SKE_ENOMEM;
    }
    *out = c;
    return SKE_OK;
}

int ske_close(ske_ctx *c) {
    if (!c) return SKE_EINVAL;
    (void)hipSetDevice(c->device);
    if (c->st) (void)hipStreamSynchronize(c->st);
    for (auto &F : c->filters) free_filter(F);
    for (auto &T : c->cms) obj_free(T);
    for (auto &H : c->hh) obj_free(H);
    for (auto &P : c->tp) obj_free(P);
    for (auto &Y : c->tally) obj_free(Y);
    for (auto &S : c->seen) obj_free(S);
    for (auto &R : c->rows) obj_free(R);
    if (c->regs) (void)hipFree(c->regs);
    if (c->tau) (void)hipFree(c->tau);
    if (c->sig) (void)hipFree(c->sig);
    for (int i = 0; i < kStageSlotCount; i++)
        if (c->stg[i]) (void)hipFree(c->stg[i]);
    stager_delete(c->hs);
    if (c->err) (void)hipFree(c->err);
    if (c->zero16) (void)hipFree(c->zero16);
    if (c->xr.done) (void)hipEventDestroy(c->xr.done);
    if (c->rt.done) (void)hipEventDestroy(c->rt.done);
    if (c->sn.done) (void)hipEventDestroy(c->sn.done);
    if (c->rw.done) (void)hipEventDestroy(c->rw.done);
    for (auto &m : c->marks) {
        if (m.own_a) (void)hipEventDestroy(m.a);
        (void)hipEventDestroy(m.b);
    }
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < c->many_n; i++) {
        (void)hipStreamDestroy(c->many_st[i]);
        (void)hipEventDestroy(c->many_join[i]);
    }
    if (c->many_fork) (void)hipEventDestroy(c->many_fork);
    for (hipEvent_t e : c->chunk_ev) (void)hipEventDestroy(e);
    if (c->copy_st) (void)hipStreamDestroy(c->copy_st);
    if (c->kt_key) (void)hipFree(c->kt_key);
    if (c->kt_slot) (void)hipFree(c->kt_slot);
    if (c->stats) (void)hipFree(c->stats);
    if (c->scratch) scratch_delete(c->scratch);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
    return SKE_OK;
}

int ske_set_stream(ske_ctx *c, void *stream) {
    if (!c) return SKE_EINVAL;
    hipStream_t next = stream ? (hipStream_t)stream : c->own;
    // leaving the stream of the last scratch use: cover it now, while the
    // stream is known to be alive
    for (ScratchUse *u : {&c->xr, &c->rt, &c->sn, &c->rw})
        if (next != c->st && u->pending && u->stream == c->st) {
            bool covered = false;
            const int rc = xr_flush(c, *u, &covered);
            if (rc) return rc;
        }
    c->st = next;
    return SKE_OK;
}

int ske_get_stream(ske_ctx *c, void **stream) {
    if (!c || !stream) return SKE_EINVAL;
    *stream = c->st == c->own ? nullptr : (void *)c->st;
    return SKE_OK;
}

int ske_sync(ske_ctx *c) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return check_err_flag(c, SKE_ERANGE);
}

int ske_check_errors(ske_ctx *c) {
    if (!c) return SKE_EINVAL;
    return check_err_flag(c, SKE_ERANGE);
}

int ske_pass_times(ske_ctx *c, double *ms, uint64_t *count, int reset) {
    if (!c || !ms || !count) return SKE_EINVAL;
    // a void mark (an abandoned guard's) or one that cannot be read (its
    // events failed) is dropped with the rest, not kept to fail every later call
    for (auto &m : c->marks) {
        float t = 0;
        if (m.pass >= 0 && hipEventSynchronize(m.b) == hipSuccess &&
            hipEventElapsedTime(&t, m.a, m.b) == hipSuccess) {
            c->pass_ms[m.pass] += t;
            c->pass_n[m.pass]++;
        }
        mark_recycle(c, m);
    }
    c->marks.clear();
    for (int i = 0; i < kPassKinds; i++) {
        ms[i] = c->pass_ms[i];
        count[i] = c->pass_n[i];
        if (reset) {
            c->pass_ms[i] = 0;
            c->pass_n[i] = 0;
        }
    }
    return SKE_OK;
}

int ske_seg_floor_stats(ske_ctx *c, uint64_t out[3]) {
    if (!c || !out) return SKE_EINVAL;
    out[0] = out[1] = out[2] = 0;
    void *p = scratch_peek(c->scratch, kScrSegFstat);
    if (!p) return SKE_OK;  // no segmented batch with floors yet
    if (c->xr.stream && c->xr.stream != c->st) HIPCHK(c, hipStreamSynchronize(c->xr.stream));
    HIPCHK(c, hipMemcpyAsync(out, p, 3 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemsetAsync(p, 0, 3 * sizeof(uint64_t), c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_device_alloc(ske_ctx *c, uint64_t bytes, void **out) {
    if (!c || !out) return SKE_EINVAL;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e != hipSuccess) {
        c->last_hip = std::string("hipMalloc: ") + hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    return SKE_OK;
}

int ske_device_free(ske_ctx *c, void *p) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, hipFree(p));
    return SKE_OK;
}

int ske_memcpy(ske_ctx *c, void *dst, const void *src, uint64_t bytes, int kind) {
    if (!c) return SKE_EINVAL;
    if (!bytes) return SKE_OK;
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice
                      : kind == 1 ? hipMemcpyDeviceToHost
                                  : hipMemcpyDeviceToDevice;
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, k, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_set_option(ske_ctx *c, const char *name, int64_t value) {
    if (!c || !name) return SKE_EINVAL;
    static const struct {
        const char *name;
        int64_t min, max;
        void (*set)(ske_ctx *, int64_t);
    } options[] = {
        // K1 tile, swipes per thread in flight: 1, 2, 4 or 8 (checked below)
        {"tile", 1, 8, [](ske_ctx *x, int64_t v) { x->pb = int(v); }},
        // 1: bracket every K1 kernel with HIP events
        {"pass_timing", 0, 1, [](ske_ctx *x, int64_t v) { x->timing = v != 0; }},
        // partitioned K1 sub-batch (swipes; 0 = default)
        {"part_sub", 0, int64_t(1) << 26, [](ske_ctx *x, int64_t v) { x->part_sub = uint32_t(v); }},
        // segmented PFADD: -1 auto, 0 never, 1 when the chain and slab allow
        {"hll_seg", -1, 1, [](ske_ctx *x, int64_t v) { x->seg.mode = int(v); }},
        // auto threshold: swipes per slab line x100
        {"seg_density", 0, 1000000, [](ske_ctx *x, int64_t v) { x->seg.density_x100 = uint32_t(v); }},
        // records per window line x100 to stage a window in LDS
        {"seg_dense_min", 0, 1000000, [](ske_ctx *x, int64_t v) { x->seg.dense_min_x100 = uint32_t(v); }},
        // keys per window 2^klog
        {"seg_klog", 0, 3, [](ske_ctx *x, int64_t v) { x->seg.klog = int(v); }},
        // segmented PFADD: 2^b1 level-1 buckets, -1 auto
        {"seg_b1", -1, 9, [](ske_ctx *x, int64_t v) { x->seg.b1 = int(v); }},
        // segmented PFADD: 1 D drops the records under their key's floor, 0 never
        {"seg_floor", 0, 1, [](ske_ctx *x, int64_t v) { x->seg.floor = int(v); }},
        // arrivals per key and window-pass group from which a window is hinted for a floor
        {"seg_hot_min", 0, int64_t(1) << 31, [](ske_ctx *x, int64_t v) { x->seg.hot_min = uint32_t(v); }},
        // blocks of the short-id LDS K1 (0: one per CU)
        {"k1_grid", 0, 65535, [](ske_ctx *x, int64_t v) { x->k1_grid = int(v); }},
        // 0: many-batch calls launch K1 per batch
        {"k1_persistent", 0, 1, [](ske_ctx *x, int64_t v) { x->k1_persistent = int(v); }},
        // K1 variant: -1 auto, 0 global, 1 LDS, 2 XCD-partitioned, 3 partitioned
        {"variant", -1, 3, [](ske_ctx *x, int64_t v) { x->variant = int(v); }},
    };
    for (const auto &o : options) {
        if (strcmp(name, o.name)) continue;
        if (value < o.min || value > o.max) return SKE_EINVAL;
        if (!strcmp(name, "tile") && (value & (value - 1))) return SKE_EINVAL;
        o.set(c, value);
        return SKE_OK;
    }
    return SKE_EINVAL;
}

// ------------------------------------------------------------------ graphs
int ske_capture_begin(ske_ctx *c) {
    if (!c) return SKE_EINVAL;
    HIPCHK(c, hipStreamBeginCapture(c->st, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    c->cap_users = 0;
    scratch_set_recording(c->scratch, true);
    return SKE_OK;
}

int ske_capture_end(ske_ctx *c, void **graph_out) {
    if (!c || !graph_out) return SKE_EINVAL;
    *graph_out = nullptr;
    hipGraph_t g = nullptr;
    c->capturing = false;
    scratch_set_recording(c->scratch, false);
    hipError_t e = hipStreamEndCapture(c->st, &g);
    hipGraphExec_t ge = nullptr;
    const char *what = "hipStreamEndCapture";
    if (e == hipSuccess) {
        what = "hipGraphInstantiate";
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
    }
    if (e == hipSuccess) {
        what = "hipGraphUpload";
        e = hipGraphUpload(ge, c->st);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st);
        if (e != hipSuccess) (void)hipGraphExecDestroy(ge);
    }
    if (e != hipSuccess) {
        // no graph holds what this capture pinned
        if (c->live_graphs == 0) scratch_unpin(c->scratch);
        c->last_hip = std::string(what) + ": " + hipGetErrorString(e);
        return SKE_EHIP;
    }
    *graph_out = ge;
    c->graph_users[(void *)ge] = c->cap_users;
    c->live_graphs++;  // the slots it pinned stay pinned until every graph is freed
    return SKE_OK;
}

int ske_graph_launch(ske_ctx *c, void *graph) {
    if (!c || !graph) return SKE_EINVAL;
    // a direct scratch use on another stream before the replay
    for (ScratchUse *u : {&c->xr, &c->rt, &c->sn, &c->rw})
        if (u->done && u->stream && u->stream != c->st && u->cap == 0) {
            bool covered = false;
            const int rc = xr_flush(c, *u, &covered);
            if (rc) return rc;
            if (covered) HIPCHK(c, hipStreamWaitEvent(c->st, u->done, 0));
        }
    HIPCHK(c, hipGraphLaunch(hipGraphExec_t(graph), c->st));
    // a replay may hold scratch users (the partitioned / XCD-partitioned K1,
    // routing): a later direct launch on another stream waits for it.  Only
    // the users the graph recorded are marked (a graph of unknown origin:
    // all).  Two replays of graphs holding scratch users on different
    // streams are not ordered by this; replay such graphs on one stream.
    const auto gu = c->graph_users.find(graph);
    const unsigned users = gu == c->graph_users.end() ? 15u : gu->second;
    for (ScratchUse *u : {&c->xr, &c->rt, &c->sn, &c->rw})
        if (u->done && (users & scratch_use_bit(c, u))) {
            HIPCHK(c, hipEventRecord(u->done, c->st));
            u->stream = c->st;
            u->cap = 0;
            u->pending = false;
        }
    return SKE_OK;
}

int ske_graph_free(ske_ctx *c, void *graph) {
    if (!c) return SKE_EINVAL;
    if (graph) {
        HIPCHK(c, hipGraphExecDestroy(hipGraphExec_t(graph)));
        c->graph_users.erase(graph);
        if (c->live_graphs > 0) c->live_graphs--;
        if (c->live_graphs == 0 && !c->capturing) scratch_unpin(c->scratch);
    }
    return SKE_OK;
}

}  // extern "C"
