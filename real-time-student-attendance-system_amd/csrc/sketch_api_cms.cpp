// sketch_api_cms.cpp -- libsketch C-ABI (include/sketch.h): Count-Min Sketch
// tables (RedisBloom src/cms.c: CMS.INITBYDIM / INITBYPROB / INCRBY / QUERY /
// MERGE / INFO), kernels in sketch_cms.hip.
#include <math.h>

#include "sketch_ctx.h"

using namespace ske;

namespace ske {

CmsTable table_of(const Cms &T) {
    CmsTable D{};
    D.cells = cms_cells(T);
    D.count = cms_count(T);
    D.div = T.div;
    D.depth = T.depth;
    D.ncells = T.width * T.depth;
    return D;
}

}  // namespace ske

// the bulk form of this table: private LDS tables up to the threshold
static bool cms_use_lds(const ske_ctx *c, const Cms &T) {
    return uint64_t(T.width) * T.depth <= c->cms_lds_cells;
}

extern "C" {

int ske_cms_dims_from_prob(double error, double prob, uint32_t *width, uint32_t *depth) {
    if (!width || !depth) return SKE_EINVAL;
    if (!(error > 0 && error < 1)) return SKE_ECMSERROR;
    if (!(prob > 0 && prob < 1)) return SKE_ECMSPROB;
    // CMS_DimFromProb: width = ceil(2 / error), depth = ceil(log10f(prob) / log10f(0.5f))
    const double w = ceil(2 / error);
    if (w >= 4294967296.0) return SKE_ECMSWIDTH;
    *width = uint32_t(w);
    *depth = uint32_t(ceil(log10f(float(prob)) / log10f(0.5f)));
    return SKE_OK;
}

int ske_cms_init(ske_ctx *c, uint32_t cid, uint32_t width, uint32_t depth) {
    if (!c || cid >= SKE_MAX_CMS) return SKE_EINVAL;
    if (width == 0) return SKE_ECMSWIDTH;
    if (depth == 0 || depth > SKE_CMS_MAX_DEPTH) return SKE_ECMSDEPTH;
    if (uint64_t(width) * depth >= SKE_CMS_MAX_CELLS) return SKE_ECMSWIDTH;
    Cms T;
    T.bytes = ((uint64_t(width) * depth * 4 + 15) & ~uint64_t(15)) + 16;  // the cells, then the count
    T.width = width;
    T.depth = depth;
    T.div = make_div32(width);
    return obj_alloc(c, kCmsFamily, c->cms, cid, T, [c](const Cms &N) { return obj_zero(N, N.bytes, c->st); });
}

int ske_cms_free(ske_ctx *c, uint32_t cid) { return obj_release(c, kCmsFamily, c->cms, cid); }

int ske_cms_info(ske_ctx *c, uint32_t cid, ske_cms_info_t *out) {
    if (!c || !out) return SKE_EINVAL;
    int rc = SKE_OK;
    Cms *T = obj_for_sync_call(c, kCmsFamily, c->cms, cid, "ske_cms_info", &rc, kCmsFamily.info_refuses);
    if (!T) return rc;
    unsigned long long cnt = 0;
    HIPCHK(c, hipMemcpyAsync(&cnt, cms_count(*T), 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    out->width = T->width;
    out->depth = T->depth;
    out->count = cnt;
    return SKE_OK;
}

int ske_cms_incrby(ske_ctx *c, uint32_t cid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                   const uint32_t *incr, uint32_t *reply, int mem) {
    if (!c) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (n == 0) return SKE_OK;
    if (n >= 0xffffffffull || !offs) return SKE_EINVAL;
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    CmsItems I{};
    I.bytes = s.bytes;
    I.offs = s.offs;
    I.n = uint32_t(n);
    rc = stage_u32(c, incr, incr ? n : 0, mem, kStgCmsIncr, &I.incr);
    if (rc) return rc;
    const CmsTable D = table_of(*T);
    if (reply) {
        uint32_t *dr = reply;
        if (mem != SKE_MEM_DEVICE) {
            dr = (uint32_t *)stage_buf(c, kStgCmsReply, n * 4, &rc);
            if (rc) return rc;
        }
        HIPCHK(c, launch_cms_seq(D, I, dr, c->st));
        if (mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(reply, dr, n * 4, hipMemcpyDeviceToHost, c->st));
    } else {
        HIPCHK(c, launch_cms_add(D, I, cms_use_lds(c, *T), c->cus, c->st));
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_cms_add_fixed_async(ske_ctx *c, uint32_t cid, const uint8_t *ids, uint32_t width, uint64_t n,
                            const uint32_t *incr, const uint8_t *mask, int want) {
    if (!c) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (n == 0) return SKE_OK;
    if (!ids || width == 0 || n >= 0xffffffffull || (want != 0 && want != 1)) return SKE_EINVAL;
    CmsItems I{};
    I.bytes = ids;
    I.fixed_w = width;
    I.n = uint32_t(n);
    I.incr = incr;
    I.mask = mask;
    I.want = uint32_t(want);
    HIPCHK(c, launch_cms_add(table_of(*T), I, cms_use_lds(c, *T), c->cus, c->st));
    return SKE_OK;
}

int ske_cms_add_packed_async(ske_ctx *c, uint32_t cid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                             const uint32_t *incr, const uint8_t *mask, int want) {
    if (!c) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (n == 0) return SKE_OK;
    if (!bytes || !offs || n >= 0xffffffffull || (want != 0 && want != 1)) return SKE_EINVAL;
    CmsItems I{};
    I.bytes = bytes;
    I.offs = offs;
    I.n = uint32_t(n);
    I.incr = incr;
    I.mask = mask;
    I.want = uint32_t(want);
    HIPCHK(c, launch_cms_add(table_of(*T), I, cms_use_lds(c, *T), c->cus, c->st));
    return SKE_OK;
}

int ske_cms_query(ske_ctx *c, uint32_t cid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                  uint32_t *out, int mem) {
    if (!c) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (n == 0) return SKE_OK;
    if (n >= 0xffffffffull || !offs || !out) return SKE_EINVAL;
    Staged s;
    int rc = stage_items(c, bytes, offs, n, mem, &s);
    if (rc) return rc;
    CmsItems I{};
    I.bytes = s.bytes;
    I.offs = s.offs;
    I.n = uint32_t(n);
    uint32_t *dout = out;
    if (mem != SKE_MEM_DEVICE) {
        dout = (uint32_t *)stage_buf(c, kStgCmsReply, n * 4, &rc);
        if (rc) return rc;
    }
    HIPCHK(c, launch_cms_query(table_of(*T), I, dout, c->cus, c->st));
    if (mem != SKE_MEM_DEVICE) HIPCHK(c, hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_cms_merge(ske_ctx *c, uint32_t dst, const uint32_t *srcs, const int64_t *weights, uint32_t nsrc) {
    if (!c || !srcs || nsrc == 0 || nsrc > SKE_CMS_MAX_MERGE) return SKE_EINVAL;
    Cms *D = get_cms(c, dst);
    if (!D) return SKE_ECMSNOKEY;
    CmsMergeArgs M{};
    for (uint32_t k = 0; k < nsrc; k++) {
        Cms *S = get_cms(c, srcs[k]);
        if (!S) return SKE_ECMSNOKEY;
        if (S->width != D->width || S->depth != D->depth) return SKE_ECMSDIMS;
        M.src[k] = cms_cells(*S);
        M.w[k] = weights ? weights[k] : 1;
    }
    M.nsrc = nsrc;
    M.ncells = D->width * D->depth;
    M.dst = cms_cells(*D);
    int rc = SKE_OK;
    // [0] the check pass's overflow word, [2 + 2k] source k's count
    uint32_t *stg = (uint32_t *)stage_buf(c, kStgCmsFlag, 8 + size_t(nsrc) * 8, &rc);
    if (rc) return rc;
    M.flag = stg;
    HIPCHK(c, hipMemsetAsync(stg, 0, 4, c->st));
    for (uint32_t k = 0; k < nsrc; k++)
        HIPCHK(c, hipMemcpyAsync(stg + 2 + 2 * k, cms_count(*get_cms(c, srcs[k])), 8, hipMemcpyDeviceToDevice, c->st));
    HIPCHK(c, launch_cms_merge(M, false, c->cus, c->st));
    uint64_t h[1 + SKE_CMS_MAX_MERGE];
    HIPCHK(c, hipMemcpyAsync(h, stg, 8 + size_t(nsrc) * 8, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (uint32_t(h[0])) return SKE_ECMSOVERFLOW;
    __int128 cnt = 0;
    for (uint32_t k = 0; k < nsrc; k++) cnt += (__int128)h[1 + k] * M.w[k];
    if (cnt < 0 || cnt > (__int128)~0ull) return SKE_ECMSOVERFLOW;
    const unsigned long long cnt64 = (unsigned long long)cnt;
    HIPCHK(c, launch_cms_merge(M, true, c->cus, c->st));
    HIPCHK(c, hipMemcpyAsync(cms_count(*D), &cnt64, 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_cms_export(ske_ctx *c, uint32_t cid, uint32_t *out, uint64_t cap_cells) {
    if (!c || !out) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    const uint64_t ncells = uint64_t(T->width) * T->depth;
    if (cap_cells < ncells) return SKE_EINVAL;
    HIPCHK(c, hipMemcpyAsync(out, cms_cells(*T), ncells * 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_cms_import(ske_ctx *c, uint32_t cid, const uint32_t *in, uint64_t ncells, uint64_t count) {
    if (!c || !in) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    if (ncells != uint64_t(T->width) * T->depth) return SKE_ECMSDIMS;
    HIPCHK(c, hipMemcpyAsync(cms_cells(*T), in, ncells * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(cms_count(*T), &count, 8, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_cms_table_dev(ske_ctx *c, uint32_t cid, void **cells_dev, uint64_t *ncells) {
    if (!c || !cells_dev || !ncells) return SKE_EINVAL;
    Cms *T = get_cms(c, cid);
    if (!T) return SKE_ECMSNOKEY;
    *cells_dev = cms_cells(*T);
    *ncells = uint64_t(T->width) * T->depth;
    return SKE_OK;
}

int ske_cms_sum_dev(ske_ctx *c, uint32_t dst_cid, const uint32_t *tables_dev, uint64_t stride_cells, uint32_t ntables,
                    const uint64_t *counts) {
    if (!c || !tables_dev || !counts || ntables == 0 || ntables > SKE_CMS_MAX_MERGE) return SKE_EINVAL;
    Cms *D = get_cms(c, dst_cid);
    if (!D) return SKE_ECMSNOKEY;
    const uint64_t ncells = uint64_t(D->width) * D->depth;
    if ((stride_cells & 3) || stride_cells < ncells || (reinterpret_cast<uintptr_t>(tables_dev) & 15))
        return SKE_EINVAL;
    unsigned long long cnt = 0;
    for (uint32_t k = 0; k < ntables; k++)
        if (__builtin_add_overflow(cnt, (unsigned long long)counts[k], &cnt)) return SKE_ECMSOVERFLOW;
    HIPCHK(c, launch_cms_sum(table_of(*D), tables_dev, stride_cells, ntables, cnt, c->cus, c->st));
    return SKE_OK;
}

}  // extern "C"
