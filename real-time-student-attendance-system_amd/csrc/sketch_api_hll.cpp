// sketch_api_hll.cpp -- libsketch C-ABI (include/sketch.h): the HLL register
// slab, PFADD, PFCOUNT, PFMERGE, export / import, and many keys as Redis
// strings (ske_hll_dump*, ske_hll_load over sketch_hll_fmt.hip).
//
// The PFCOUNT estimator's m*tau(.) / m*sigma(.) tables (src/hyperloglog.c
// hllTau / hllSigma) are built here with the same libm calls as Redis.
// Compiled with -ffp-contract=off.
#include <math.h>

#include <algorithm>
#include <memory>

#include "sketch_ctx.h"

using namespace ske;

// hllTau / hllSigma exactly as Redis src/hyperloglog.c (glibc sqrt, pow).
static double redis_sigma(double x) {
    if (x == 1.) return INFINITY;
    double zPrime, y = 1, z = x;
    do {
        x *= x;
        zPrime = z;
        z += x * y;
        y += y;
    } while (zPrime != z);
    return z;
}
static double redis_tau(double x) {
    if (x == 0. || x == 1.) return 0.;
    double zPrime, y = 1.0, z = 1 - x;
    do {
        x = sqrt(x);
        zPrime = z;
        y *= 0.5;
        z -= pow(1 - x, 2) * y;
    } while (zPrime != z);
    return z / 3;
}

static int ensure_tables(ske_ctx *c) {
    if (c->tau) return SKE_OK;
    const int M = SKE_HLL_REGISTERS;
    std::vector<double> tau(M + 1), sig(M + 1);
    const double m = M;
    for (int j = 0; j <= M; j++) {
        tau[j] = m * redis_tau((m - j) / (double)m);  // z = m * hllTau((m-H[Q+1])/m)
        sig[j] = m * redis_sigma(j / (double)m);      // z += m * hllSigma(H[0]/m)
    }
    HIPCHK(c, hipMalloc(&c->tau, (M + 1) * sizeof(double)));
    HIPCHK(c, hipMalloc(&c->sig, (M + 1) * sizeof(double)));
    HIPCHK(c, hipMemcpy(c->tau, tau.data(), (M + 1) * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->sig, sig.data(), (M + 1) * sizeof(double), hipMemcpyHostToDevice));
    return SKE_OK;
}

static int pfcount_impl(ske_ctx *c, const uint8_t *regs, const uint32_t *slots,
                        const uint32_t *goffs, uint32_t ngroups, uint64_t *out, int mem) {
    int rc = ensure_tables(c);
    if (rc) return rc;
    uint64_t *dout = out;
    if (mem != SKE_MEM_DEVICE) {
        dout = (uint64_t *)stage_buf(c, kStgReply, uint64_t(ngroups) * 8, &rc);
        if (rc) return rc;
    }
    HIPCHK(c, launch_pfcount(regs, slots, goffs, ngroups, c->tau, c->sig, dout, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE)
        HIPCHK(c, hipMemcpyAsync(out, dout, uint64_t(ngroups) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

static int check_slots_host(ske_ctx *c, const uint32_t *slots, uint64_t n) {
    for (uint64_t i = 0; i < n; i++)
        if (slots[i] >= c->nslots) return SKE_ERANGE;
    return SKE_OK;
}

// a device-resident slot list in range of the slab (one reduction kernel and
// a 4-byte read back): SKE_ERANGE before any kernel addresses the slab with it
static int check_slots_dev(ske_ctx *c, const uint32_t *slots, uint64_t n) {
    if (n == 0) return SKE_OK;
    int rc = SKE_OK;
    unsigned int *d = (unsigned int *)stage_buf(c, kStgCheck, 4, &rc);
    if (rc) return rc;
    unsigned int mx = 0;
    HIPCHK(c, launch_slots_max(slots, n, d, c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(&mx, d, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return mx >= c->nslots ? SKE_ERANGE : SKE_OK;
}

// the slot list of a bulk call (nullptr: keys 0 .. nkeys - 1) in range of the
// slab, and on the device
static int bulk_slots(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, int mem, const uint32_t **ds) {
    *ds = nullptr;
    if (!slots) return nkeys > c->nslots ? SKE_ERANGE : SKE_OK;
    int rc = mem == SKE_MEM_DEVICE ? check_slots_dev(c, slots, nkeys) : check_slots_host(c, slots, nkeys);
    if (rc) return rc;
    return stage_u32(c, slots, nkeys, mem, kStgList, ds);
}

// The string offsets of the listed keys (device, nkeys + 1 entries, in the
// context scratch) and their last entry, the total.  Returns after a stream
// synchronise.
static int dump_offsets(ske_ctx *c, const uint32_t *ds, uint32_t nkeys, uint32_t smb, uint32_t **doffs,
                        uint32_t *total) {
    hipError_t e = hipSuccess;
    uint32_t *sizes = (uint32_t *)scratch_get(c->scratch, kScrHllFmtSize, size_t(nkeys) * 4 + 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    uint32_t *offs = (uint32_t *)scratch_get(c->scratch, kScrHllFmtOffs, size_t(nkeys) * 4 + 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    HIPCHK(c, hipMemsetAsync(offs, 0, 4, c->st));
    HIPCHK(c, launch_hll_fmt_sizes(c->regs, ds, nkeys, c->nslots, smb, sizes, c->cus, c->st));
    HIPCHK(c, scan_inclusive_u32(c->scratch, sizes, offs + 1, nkeys, c->st));
    HIPCHK(c, hipMemcpyAsync(total, offs + nkeys, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *doffs = offs;
    return SKE_OK;
}

static int copy_out(ske_ctx *c, void *dst, const void *dev, size_t bytes, int mem) {
    if (bytes == 0) return SKE_OK;
    HIPCHK(c, hipMemcpyAsync(dst, dev, bytes, mem == SKE_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             c->st));
    return SKE_OK;
}

static int pfmerge_impl(ske_ctx *c, uint32_t dst, const uint32_t *srcs, uint32_t n, int mem) {
    if (!c || (n && !srcs)) return SKE_EINVAL;
    if (dst >= c->nslots) return SKE_ERANGE;
    int rc = mem == SKE_MEM_DEVICE ? check_slots_dev(c, srcs, n) : check_slots_host(c, srcs, n);
    if (rc) return rc;
    if (n == 0) return SKE_OK;
    const uint32_t *ds;
    rc = stage_u32(c, srcs, n, mem, kStgList, &ds);
    if (rc) return rc;
    if (n <= 256) {
        HIPCHK(c, launch_pfmerge(c->regs, dst, ds, n, c->st));
    } else {
        // campus-wide merges (C5: 1.8M day keys): a two-level parallel max
        uint32_t per = 0;
        const uint32_t P = pfmerge_partitions(n, c->cus, &per);
        hipError_t e = hipSuccess;
        uint8_t *partial = (uint8_t *)scratch_get(c->scratch, kScrMergePartial, size_t(P) * SKE_HLL_REGISTERS, &e);
        if (e != hipSuccess) {
            c->last_hip = hipGetErrorString(e);
            return SKE_ENOMEM;
        }
        HIPCHK(c, launch_pfmerge_wide(c->regs, dst, ds, n, partial, per, P, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

extern "C" {

int ske_hll_reserve(ske_ctx *c, uint32_t nslots) {
    if (!c) return SKE_EINVAL;
    if (nslots <= c->nslots) return SKE_OK;
    if (c->live_graphs > 0 || c->capturing) {
        c->last_hip = "the HLL slab cannot move while a recorded graph points to it";
        return SKE_EBUSY;
    }
    uint64_t want = std::max<uint64_t>(nslots, uint64_t(c->nslots) * 3 / 2);
    want = std::max<uint64_t>(want, 16);
    uint8_t *nr = nullptr;
    hipError_t e = hipMalloc(&nr, want * SKE_HLL_REGISTERS);
    if (e != hipSuccess) {
        c->last_hip = std::string("hipMalloc(hll slab): ") + hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    struct DevFree {
        void operator()(void *p) const { (void)hipFree(p); }
    };
    std::unique_ptr<uint8_t, DevFree> slab(nr);  // freed on every failure below
    HIPCHK(c, hipMemsetAsync(nr, 0, want * SKE_HLL_REGISTERS, c->st));
    if (c->regs) {
        HIPCHK(c, hipMemcpyAsync(nr, c->regs, uint64_t(c->nslots) * SKE_HLL_REGISTERS,
                                 hipMemcpyDeviceToDevice, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->regs) (void)hipFree(c->regs);
    c->regs = slab.release();
    c->nslots = uint32_t(want);
    return SKE_OK;
}

uint32_t ske_hll_capacity(ske_ctx *c) { return c ? c->nslots : 0; }

int ske_hll_clear(ske_ctx *c, uint32_t slot) {
    if (!c) return SKE_EINVAL;
    if (slot >= c->nslots) return SKE_ERANGE;
    HIPCHK(c, hipMemsetAsync(c->regs + uint64_t(slot) * SKE_HLL_REGISTERS, 0, SKE_HLL_REGISTERS,
                             c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_pfadd(ske_ctx *c, const uint32_t *slot, const uint8_t *bytes, const uint32_t *offs,
                  uint64_t n, uint8_t *changed, int mem) {
    if (!c || !slot) return SKE_EINVAL;
    if (n == 0) return SKE_OK;
    if (const int erc = err_begin(c)) return erc;  // earlier enqueue-only calls' slot errors
    if (n >= 0xffffffffull) return SKE_EINVAL;
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    const uint32_t *dslot;
    rc = stage_u32(c, slot, n, mem, kStgSlots, &dslot);
    if (rc) return rc;
    if (changed) {
        uint8_t *dch = changed;
        if (mem != SKE_MEM_DEVICE) {
            dch = (uint8_t *)stage_buf(c, kStgOut, n, &rc);
            if (rc) return rc;
        }
        HIPCHK(c, pfadd_exact(c->scratch, dslot, s.bytes, s.offs, n, c->regs, c->nslots, dch,
                              c->err, c->cus, c->st));
        if (mem != SKE_MEM_DEVICE)
            HIPCHK(c, hipMemcpyAsync(changed, dch, n, hipMemcpyDeviceToHost, c->st));
    } else {
        HIPCHK(c, launch_pfadd(dslot, s.bytes, s.offs, n, c->regs, c->nslots, c->err, c->cus,
                               c->st));
    }
    return check_call_err(c);
}

int ske_hll_pfcount(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, uint64_t *out) {
    if (!c || !slots || !out || nkeys == 0) return SKE_EINVAL;
    int rc = check_slots_host(c, slots, nkeys);
    if (rc) return rc;
    const uint32_t *ds;
    rc = stage_u32(c, slots, nkeys, SKE_MEM_HOST, kStgList, &ds);
    if (rc) return rc;
    const uint32_t go[2] = {0, nkeys};
    const uint32_t *dg;
    rc = stage_u32(c, go, 2, SKE_MEM_HOST, kStgList2, &dg);
    if (rc) return rc;
    return pfcount_impl(c, c->regs, ds, dg, 1, out, SKE_MEM_HOST);
}

int ske_hll_pfcount_each(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, uint64_t *out,
                         int mem) {
    if (!c || !out) return SKE_EINVAL;
    if (nkeys == 0) return SKE_OK;
    if (slots) {
        int rc = mem == SKE_MEM_DEVICE ? check_slots_dev(c, slots, nkeys) : check_slots_host(c, slots, nkeys);
        if (rc) return rc;
    }
    const uint32_t *ds = nullptr;
    if (slots) {
        int rc = stage_u32(c, slots, nkeys, mem, kStgList, &ds);
        if (rc) return rc;
    } else if (nkeys > c->nslots) {
        return SKE_ERANGE;
    }
    return pfcount_impl(c, c->regs, ds, nullptr, nkeys, out, mem);
}

int ske_hll_pfcount_groups(ske_ctx *c, const uint32_t *slots, const uint32_t *goffs,
                           uint32_t ngroups, uint64_t *out, int mem) {
    if (!c || !slots || !goffs || !out) return SKE_EINVAL;
    if (ngroups == 0) return SKE_OK;
    int rc;
    if (mem != SKE_MEM_DEVICE) {
        for (uint32_t g = 0; g < ngroups; g++)
            if (goffs[g + 1] < goffs[g]) return SKE_EINVAL;
        rc = check_slots_host(c, slots + goffs[0], goffs[ngroups] - goffs[0]);
        if (rc) return rc;
    }
    const uint32_t *ds, *dg;
    const uint64_t nslots_total = mem == SKE_MEM_DEVICE ? 0 : goffs[ngroups];
    if (mem == SKE_MEM_DEVICE) {
        ds = slots;
        dg = goffs;
    } else {
        rc = stage_u32(c, slots, nslots_total, mem, kStgList, &ds);
        if (rc) return rc;
        rc = stage_u32(c, goffs, uint64_t(ngroups) + 1, mem, kStgList2, &dg);
        if (rc) return rc;
    }
    return pfcount_impl(c, c->regs, ds, dg, ngroups, out, mem);
}

int ske_hll_merge_groups_dev(ske_ctx *c, const uint32_t *slots, const uint32_t *goffs,
                             uint32_t ngroups, uint8_t *dst_dev) {
    if (!c || !goffs || !dst_dev) return SKE_EINVAL;
    if (ngroups == 0) return SKE_OK;
    for (uint32_t g = 0; g < ngroups; g++)
        if (goffs[g + 1] < goffs[g]) return SKE_EINVAL;
    const uint64_t total = goffs[ngroups];
    if (total && !slots) return SKE_EINVAL;
    int rc = check_slots_host(c, slots, total);
    if (rc) return rc;
    const uint32_t *ds, *dg;
    rc = stage_u32(c, slots, total, SKE_MEM_HOST, kStgList, &ds);
    if (rc) return rc;
    rc = stage_u32(c, goffs, uint64_t(ngroups) + 1, SKE_MEM_HOST, kStgList2, &dg);
    if (rc) return rc;
    HIPCHK(c, launch_merge_groups(c->regs, ds, dg, ngroups, dst_dev, c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_count_raw_dev(ske_ctx *c, const uint8_t *regs_dev, uint32_t nkeys, uint64_t *out) {
    if (!c || !regs_dev || !out) return SKE_EINVAL;
    if (nkeys == 0) return SKE_OK;
    return pfcount_impl(c, regs_dev, nullptr, nullptr, nkeys, out, SKE_MEM_HOST);
}

int ske_hll_pfmerge(ske_ctx *c, uint32_t dst, const uint32_t *srcs, uint32_t n) {
    return pfmerge_impl(c, dst, srcs, n, SKE_MEM_HOST);
}

int ske_hll_pfmerge_dev(ske_ctx *c, uint32_t dst, const uint32_t *srcs_dev, uint32_t n) {
    return pfmerge_impl(c, dst, srcs_dev, n, SKE_MEM_DEVICE);
}

int ske_hll_histogram(ske_ctx *c, uint32_t slot, uint32_t *out64) {
    if (!c || !out64) return SKE_EINVAL;
    if (slot >= c->nslots) return SKE_ERANGE;
    int rc = SKE_OK;
    uint32_t *d = (uint32_t *)stage_buf(c, kStgReply, 256, &rc);
    if (rc) return rc;
    HIPCHK(c, launch_histogram(c->regs + uint64_t(slot) * SKE_HLL_REGISTERS, d, c->st));
    HIPCHK(c, hipMemcpyAsync(out64, d, 256, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_export_raw(ske_ctx *c, uint32_t slot, uint8_t *out) {
    if (!c || !out) return SKE_EINVAL;
    if (slot >= c->nslots) return SKE_ERANGE;
    HIPCHK(c, hipMemcpyAsync(out, c->regs + uint64_t(slot) * SKE_HLL_REGISTERS, SKE_HLL_REGISTERS,
                             hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_export_dense(ske_ctx *c, uint32_t slot, uint8_t *out) {
    if (!c || !out) return SKE_EINVAL;
    if (slot >= c->nslots) return SKE_ERANGE;
    int rc = SKE_OK;
    uint8_t *d = (uint8_t *)stage_buf(c, kStgReply, SKE_HLL_DENSE_BYTES, &rc);
    if (rc) return rc;
    HIPCHK(c, launch_dense(c->regs + uint64_t(slot) * SKE_HLL_REGISTERS, d, c->st));
    HIPCHK(c, hipMemcpyAsync(out, d, SKE_HLL_DENSE_BYTES, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_import_raw(ske_ctx *c, uint32_t slot, const uint8_t *in) {
    if (!c || !in) return SKE_EINVAL;
    if (slot >= c->nslots) return SKE_ERANGE;
    for (int i = 0; i < SKE_HLL_REGISTERS; i++)
        if (in[i] > 51) return SKE_EBADHLL;  // no register can exceed Q+1
    HIPCHK(c, hipMemcpyAsync(c->regs + uint64_t(slot) * SKE_HLL_REGISTERS, in, SKE_HLL_REGISTERS,
                             hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_dump_sizes(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, uint32_t sparse_max_bytes,
                       uint32_t *offs_out, int mem) {
    if (!c || !offs_out || nkeys > SKE_HLL_DUMP_MAX_KEYS) return SKE_EINVAL;
    const uint32_t *ds;
    int rc = bulk_slots(c, slots, nkeys, mem, &ds);
    if (rc) return rc;
    uint32_t *doffs, total = 0;
    rc = dump_offsets(c, ds, nkeys, sparse_max_bytes, &doffs, &total);
    if (rc) return rc;
    rc = copy_out(c, offs_out, doffs, size_t(nkeys) * 4 + 4, mem);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_dump(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, uint32_t sparse_max_bytes, int flags,
                 uint8_t *out, uint64_t cap, uint32_t *offs_out, int mem) {
    if (!c || !offs_out || nkeys > SKE_HLL_DUMP_MAX_KEYS || (flags & ~SKE_HLL_DUMP_CARD)) return SKE_EINVAL;
    const uint32_t *ds;
    int rc = bulk_slots(c, slots, nkeys, mem, &ds);
    if (rc) return rc;
    uint32_t *doffs, total = 0;
    rc = dump_offsets(c, ds, nkeys, sparse_max_bytes, &doffs, &total);
    if (rc) return rc;
    if (cap < total || (total && !out)) return SKE_EINVAL;
    uint8_t *dout = out;
    if (mem != SKE_MEM_DEVICE && total) {
        dout = (uint8_t *)stage_buf(c, kStgHllFmtBlob, total, &rc);
        if (rc) return rc;
    }
    const uint64_t *card = nullptr;
    if ((flags & SKE_HLL_DUMP_CARD) && nkeys) {
        rc = ensure_tables(c);
        if (rc) return rc;
        hipError_t e = hipSuccess;
        uint64_t *dc = (uint64_t *)scratch_get(c->scratch, kScrHllFmtCard, size_t(nkeys) * 8, &e);
        if (e != hipSuccess) return scratch_error(c, e);
        HIPCHK(c, launch_pfcount(c->regs, ds, nullptr, nkeys, c->tau, c->sig, dc, c->cus, c->st));
        card = dc;
    }
    HIPCHK(c, launch_hll_fmt_dump(c->regs, ds, nkeys, c->nslots, sparse_max_bytes, card, doffs, dout, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) {
        rc = copy_out(c, out, dout, total, mem);
        if (rc) return rc;
    }
    rc = copy_out(c, offs_out, doffs, size_t(nkeys) * 4 + 4, mem);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_hll_load(ske_ctx *c, const uint32_t *slots, uint32_t nkeys, const uint8_t *blob, const uint32_t *offs,
                 uint8_t *status, int mem) {
    if (!c || !offs || nkeys > SKE_HLL_DUMP_MAX_KEYS) return SKE_EINVAL;
    if (nkeys == 0) return SKE_OK;
    const uint32_t *ds;
    int rc = bulk_slots(c, slots, nkeys, mem, &ds);
    if (rc) return rc;
    unsigned int *flag = (unsigned int *)stage_buf(c, kStgHllFmtFlag, 4, &rc);
    if (rc) return rc;
    unsigned int word = 0;
    Staged s;
    if (mem == SKE_MEM_DEVICE) {  // host offsets are checked as stage_items copies them
        if (!blob) return SKE_EINVAL;
        HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->st));
        HIPCHK(c, launch_hll_fmt_offs_check(offs, nkeys, flag, c->cus, c->st));
        HIPCHK(c, hipMemcpyAsync(&word, flag, 4, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        if (word) return SKE_EINVAL;
    }
    rc = stage_items(c, blob, offs, nkeys, mem, &s);
    if (rc) return rc;
    uint8_t *dstat = status;
    if (status && mem != SKE_MEM_DEVICE) {
        dstat = (uint8_t *)stage_buf(c, kStgHllFmtStatus, nkeys, &rc);
        if (rc) return rc;
    }
    HIPCHK(c, hipMemsetAsync(flag, 0, 4, c->st));
    HIPCHK(c, launch_hll_fmt_load(c->regs, ds, nkeys, c->nslots, s.bytes, s.offs, dstat, flag, c->cus, c->st));
    if (status && mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(status, dstat, nkeys, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&word, flag, 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return word ? SKE_EBADHLL : SKE_OK;
}

int ske_hll_slab(ske_ctx *c, void **p, uint64_t *bytes) {
    if (!c || !p || !bytes) return SKE_EINVAL;
    *p = c->regs;
    *bytes = uint64_t(c->nslots) * SKE_HLL_REGISTERS;
    return SKE_OK;
}

}  // extern "C"
