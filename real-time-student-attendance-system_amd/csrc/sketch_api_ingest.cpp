// sketch_api_ingest.cpp -- libsketch C-ABI (include/sketch.h): JSON event
// ingest, the key table, and the synthetic workload generator.
#include "sketch_ctx.h"

using namespace ske;

// ------------------------------------------------------------------ ingest
static IngestCols ingest_cols(const ske_ingest_cols_t *c) {
    IngestCols k;
    k.status = c->status;
    k.id_start = c->id_start;
    k.id_len = c->id_len;
    k.lec_start = c->lec_start;
    k.lec_len = c->lec_len;
    k.ts_start = c->ts_start;
    k.ts_len = c->ts_len;
    k.day = c->day;
    k.kh = c->kh;
    return k;
}

static int keytab_lookup(ske_ctx *c, const ske_ingest_cols_t *cols, uint64_t n, uint32_t *slot,
                         uint32_t **flag, uint32_t **mlen) {
    hipError_t e = hipSuccess;
    *flag = (uint32_t *)scratch_get(c->scratch, kScrKtFlag, n * 4, &e);
    *mlen = (uint32_t *)scratch_get(c->scratch, kScrKtLen, n * 4, &e);
    if (e != hipSuccess) {
        c->last_hip = hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    HIPCHK(c, launch_keytab_lookup(c->kt_key, c->kt_slot, c->kt_cap ? c->kt_cap - 1 : 0, cols->kh,
                                   cols->status, cols->id_len, n, slot, *flag, *mlen, c->cus, c->st));
    return SKE_OK;
}

static int keytab_grow(ske_ctx *c, uint64_t want) {
    uint64_t cap = 1024;
    while (cap < want * 2) cap <<= 1;
    if (cap <= c->kt_cap) return SKE_OK;
    uint64_t *nk = nullptr;
    uint32_t *ns = nullptr;
    hipError_t e = hipMalloc(&nk, cap * 16);
    if (e == hipSuccess) e = hipMalloc(&ns, cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(nk, 0, cap * 16, c->st);
    if (e != hipSuccess) {
        if (nk) (void)hipFree(nk);
        if (ns) (void)hipFree(ns);
        c->last_hip = std::string("key table: ") + hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    if (c->kt_cap)  // rehash the old entries (empty ones are skipped)
        HIPCHK(c, launch_keytab_insert(nk, ns, cap - 1, c->kt_key, c->kt_slot, c->kt_cap, c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    if (c->kt_key) (void)hipFree(c->kt_key);
    if (c->kt_slot) (void)hipFree(c->kt_slot);
    c->kt_key = nk;
    c->kt_slot = ns;
    c->kt_cap = cap;
    return SKE_OK;
}

// ------------------------------------------------------------------ generator
static int gen_dev(const ske_gen_params_t *p, GenDev *g) {
    const int w = ske_gen_id_width(p);
    if (w < 1 || w > 19) return SKE_EINVAL;
    uint64_t p10 = 1;
    for (int i = 0; i < 20; i++) {
        g->pow10[i] = p10;
        if (i < 19) p10 *= 10;
    }
    if (p->id_lo < g->pow10[w - 1]) return SKE_EINVAL;  // all IDs share the digit count
    const uint64_t R = p->id_hi - p->id_lo;
    if (R >= (uint64_t(1) << 32) || p->n_members == 0 || p->n_members > R) return SKE_EINVAL;
    if (p->perm_mul % R == 0 || (unsigned __int128)(p->perm_mul % R) * (p->perm_mul_inv % R) % R != 1 % R)
        return SKE_EINVAL;
    if (p->n_keys == 0) return SKE_EINVAL;
    g->seed = p->seed;
    g->lo = p->id_lo;
    g->R = R;
    g->N = p->n_members;
    g->mul = p->perm_mul % R;
    g->add = p->perm_add % R;
    g->inv = p->perm_mul_inv % R;
    g->inv_thr = p->invalid_thresh;
    g->near_thr = p->near_thresh;
    g->n_keys = p->n_keys;
    g->slot_base = p->slot_base;
    g->width = uint32_t(w);
    g->key_cdf = p->key_cdf;
    return SKE_OK;
}

extern "C" {

int ske_ingest_parse(ske_ctx *c, const uint8_t *msgs, const uint32_t *moffs, uint64_t n,
                     int day_form, const ske_ingest_cols_t *cols) {
    if (!c || !cols || (n && (!msgs || !moffs))) return SKE_EINVAL;
    HIPCHK(c, launch_ingest_parse(msgs, moffs, n, day_form, ingest_cols(cols), c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_keytab_lookup(ske_ctx *c, const ske_ingest_cols_t *cols, uint64_t n, uint32_t *slot_dev,
                      uint64_t *nmiss) {
    if (!c || !cols || !slot_dev) return SKE_EINVAL;
    if (nmiss) *nmiss = 0;
    if (!n) return SKE_OK;
    uint32_t *flag, *mlen;
    int rc = keytab_lookup(c, cols, n, slot_dev, &flag, &mlen);
    if (rc) return rc;
    if (nmiss) {
        // decoded - found = misses (flag is 1 for found keys)
        hipError_t e = hipSuccess;
        uint32_t *incl = (uint32_t *)scratch_get(c->scratch, kScrKtIncl, n * 4, &e);
        if (!incl) {
            c->last_hip = hipGetErrorString(e);
            return SKE_ENOMEM;
        }
        HIPCHK(c, scan_inclusive_u32(c->scratch, flag, incl, n, c->st));
        uint32_t found = 0;
        HIPCHK(c, hipMemcpyAsync(&found, incl + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
        std::vector<uint8_t> st(n);
        HIPCHK(c, hipMemcpyAsync(st.data(), cols->status, n, hipMemcpyDeviceToHost, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
        uint64_t decoded = 0;
        for (uint64_t i = 0; i < n; i++) decoded += st[i] == 0;
        *nmiss = decoded - found;
    } else {
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    return SKE_OK;
}

int ske_keytab_insert(ske_ctx *c, const uint64_t *kh_host, const uint32_t *slots_host, uint64_t n) {
    if (!c || (n && (!kh_host || !slots_host))) return SKE_EINVAL;
    if (!n) return SKE_OK;
    for (uint64_t i = 0; i < n; i++)
        if ((kh_host[2 * i] & 1) == 0) return SKE_EINVAL;  // kh0 is odd by construction
    int rc = keytab_grow(c, c->kt_count + n);
    if (rc) return rc;
    int r2 = SKE_OK;
    uint64_t *dk = (uint64_t *)stage_buf(c, kStgList, n * 16, &r2);
    uint32_t *ds = (uint32_t *)stage_buf(c, kStgList2, n * 4, &r2);
    if (r2) return r2;
    HIPCHK(c, hipMemcpyAsync(dk, kh_host, n * 16, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, hipMemcpyAsync(ds, slots_host, n * 4, hipMemcpyHostToDevice, c->st));
    HIPCHK(c, launch_keytab_insert(c->kt_key, c->kt_slot, c->kt_cap - 1, dk, ds, n, c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    c->kt_count += n;
    return SKE_OK;
}

int ske_keytab_clear(ske_ctx *c) {
    if (!c) return SKE_EINVAL;
    if (c->kt_cap) {
        HIPCHK(c, hipMemsetAsync(c->kt_key, 0, c->kt_cap * 16, c->st));
        HIPCHK(c, hipStreamSynchronize(c->st));
    }
    c->kt_count = 0;
    return SKE_OK;
}

int ske_ingest_swipes(ske_ctx *c, uint32_t fid, const uint8_t *msgs, const ske_ingest_cols_t *cols,
                      uint64_t n, uint8_t *valid_dev, uint64_t *ntaken) {
    if (!c || !cols || !valid_dev || (n && !msgs)) return SKE_EINVAL;
    Filter *F = get_filter(c, fid);
    if (!F) return SKE_EINVAL;
    if (ntaken) *ntaken = 0;
    if (!n) return SKE_OK;
    if (const int erc = err_begin(c)) return erc;  // earlier enqueue-only calls' slot errors
    if (n >= (uint64_t(1) << 31)) return SKE_EINVAL;
    hipError_t e = hipSuccess;
    uint32_t *slot = (uint32_t *)scratch_get(c->scratch, kScrInSlot, n * 4, &e);
    uint32_t *flag_incl = (uint32_t *)scratch_get(c->scratch, kScrInFlagIncl, n * 4, &e);
    uint32_t *len_incl = (uint32_t *)scratch_get(c->scratch, kScrInLenIncl, n * 4, &e);
    if (e != hipSuccess) {
        c->last_hip = hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    uint32_t *flag, *mlen;
    int rc = keytab_lookup(c, cols, n, slot, &flag, &mlen);
    if (rc) return rc;
    HIPCHK(c, scan_inclusive_u32(c->scratch, flag, flag_incl, n, c->st));
    HIPCHK(c, scan_inclusive_u32(c->scratch, mlen, len_incl, n, c->st));
    uint32_t tot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&tot[0], flag_incl + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&tot[1], len_incl + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    const uint32_t taken = tot[0], nbytes = tot[1];
    uint8_t *ids = (uint8_t *)scratch_get(c->scratch, kScrInIds, size_t(nbytes) + 16, &e);
    uint32_t *ids_offs = (uint32_t *)scratch_get(c->scratch, kScrInOffs, (size_t(taken) + 1) * 4, &e);
    uint32_t *kslot = (uint32_t *)scratch_get(c->scratch, kScrInKslot, size_t(taken) * 4 + 4, &e);
    uint8_t *kvalid = (uint8_t *)scratch_get(c->scratch, kScrInKvalid, size_t(taken) + 4, &e);
    if (e != hipSuccess) {
        c->last_hip = hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    const IngestCols k = ingest_cols(cols);
    HIPCHK(c, launch_ingest_pack(msgs, k, slot, flag_incl, len_incl, n, ids, ids_offs, kslot, c->cus,
                                 c->st));
    HIPCHK(c, hipMemsetAsync(kvalid, 0, size_t(taken) + 4, c->st));
    if (taken && F->exists) {
        rc = launch_k1(c, chain_of(F), PartBatch{ids, ids_offs, 0, kslot, taken, kvalid}, c->st, k1_grid(c));
        if (rc) return rc;
    }
    HIPCHK(c, launch_ingest_unpack(k, slot, flag_incl, kvalid, n, valid_dev, c->cus, c->st));
    if (ntaken) *ntaken = taken;
    return check_call_err(c);
}

int ske_ingest_times(ske_ctx *c, const uint8_t *msgs, const ske_ingest_cols_t *cols, uint64_t n,
                     int64_t *epoch_dev) {
    if (!c || !cols || (n && (!msgs || !epoch_dev))) return SKE_EINVAL;
    if (reinterpret_cast<uintptr_t>(epoch_dev) & 7) return SKE_EINVAL;
    HIPCHK(c, launch_ingest_times(msgs, ingest_cols(cols), n, epoch_dev, c->cus, unsigned(c->ingest_grid), c->st));
    return SKE_OK;
}

int ske_ingest_dense(ske_ctx *c, const uint8_t *msgs, const ske_ingest_cols_t *cols, uint64_t n,
                     const uint8_t *valid_dev, const int64_t *epoch_dev, const ske_ingest_dense_t *out,
                     uint64_t cap_bytes, uint64_t *ndense, uint64_t *nbytes) {
    if (!c || !cols || !out || !ndense || !nbytes) return SKE_EINVAL;
    *ndense = *nbytes = 0;
    if (!n) return SKE_OK;
    if (!msgs || !out->ids || !out->offs || !out->epoch || !out->valid || !out->at) return SKE_EINVAL;
    if ((reinterpret_cast<uintptr_t>(out->epoch) & 7) || n >= (uint64_t(1) << 31)) return SKE_EINVAL;
    if (c->capturing) {
        c->last_hip = "ske_ingest_dense waits for the stream and cannot be recorded";
        return SKE_EBUSY;
    }
    hipError_t e = hipSuccess;
    uint32_t *flag = (uint32_t *)scratch_get(c->scratch, kScrKtFlag, n * 4, &e);
    uint32_t *mlen = (uint32_t *)scratch_get(c->scratch, kScrKtLen, n * 4, &e);
    uint32_t *flag_incl = (uint32_t *)scratch_get(c->scratch, kScrInFlagIncl, n * 4, &e);
    uint32_t *len_incl = (uint32_t *)scratch_get(c->scratch, kScrInLenIncl, n * 4, &e);
    if (e != hipSuccess) return scratch_error(c, e);
    const IngestCols k = ingest_cols(cols);
    const unsigned grid = unsigned(c->ingest_grid);
    HIPCHK(c, launch_ingest_dense_flags(k, n, flag, mlen, c->cus, grid, c->st));
    HIPCHK(c, scan_inclusive_u32(c->scratch, flag, flag_incl, n, c->st));
    HIPCHK(c, scan_inclusive_u32(c->scratch, mlen, len_incl, n, c->st));
    uint32_t tot[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&tot[0], flag_incl + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipMemcpyAsync(&tot[1], len_incl + (n - 1), 4, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    *ndense = tot[0];
    *nbytes = tot[1];
    if (tot[1] > cap_bytes) return SKE_EINVAL;  // nothing written; *nbytes is the need
    const IngestDense D{out->ids, out->offs, out->epoch, out->valid, out->at};
    HIPCHK(c, launch_ingest_dense(msgs, k, flag_incl, len_incl, valid_dev, epoch_dev, n, D, c->cus, grid, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_gen_id_width(const ske_gen_params_t *p) {
    if (!p || p->id_hi <= p->id_lo) return SKE_EINVAL;
    uint64_t x = p->id_hi - 1;
    int w = 1;
    while (x >= 10) {
        x /= 10;
        w++;
    }
    return w;
}

int ske_gen_members(ske_ctx *c, const ske_gen_params_t *p, uint64_t start, uint64_t n,
                    uint8_t *bytes_dev, uint32_t *offs_dev) {
    if (!c || !p || !bytes_dev || !offs_dev) return SKE_EINVAL;
    GenDev g{};
    int rc = gen_dev(p, &g);
    if (rc) return rc;
    if (start + n > g.N || n * g.width >= 0xffffffffull) return SKE_EINVAL;
    HIPCHK(c, launch_gen_members(g, start, n, bytes_dev, offs_dev, c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

int ske_gen_swipes(ske_ctx *c, const ske_gen_params_t *p, uint64_t start, uint64_t n,
                   uint8_t *bytes_dev, uint32_t *offs_dev, uint32_t *slot_dev) {
    if (!c || !p || !bytes_dev || !offs_dev || !slot_dev) return SKE_EINVAL;
    GenDev g{};
    int rc = gen_dev(p, &g);
    if (rc) return rc;
    if (n * g.width >= 0xffffffffull) return SKE_EINVAL;
    HIPCHK(c, launch_gen_swipes(g, start, n, bytes_dev, offs_dev, slot_dev, c->cus, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

}  // extern "C"
