/*
 * sketch.h -- C-ABI of libsketch, the MI355X (gfx950) sketch engine for the
 * attendance validate-and-count hot path.
 *
 * The reference (devarshpatel1506/Real-Time-Student-Attendance-System) reaches
 * this path through a redis-py client object (attendance_processor.py:37-41,
 * data_generator.py:45-49).  Each entry point below replaces one family of the
 * RESP round trips that client makes; the Python facade
 * (real-time-student-attendance-system_amd/client.py, client_*.py) keeps the redis-py call
 * surface and binds these symbols through ctypes (INTEGRATION.md shows the
 * binding).
 *
 * Conventions
 *   - return 0 (SKE_OK) or a negative SKE_E* code; no exception crosses the ABI;
 *     ske_strerror() maps a code to the Redis / RedisBloom error text.
 *   - the caller owns every input / output buffer.  `mem` says where the
 *     buffers live: SKE_MEM_HOST (host memory, staged through the context's
 *     device buffers; pageable inputs above 8 MB go through two pinned 32 MB
 *     buffers filled by up to 8 host threads the context starts on first use)
 *     or SKE_MEM_DEVICE (HIP device pointers, e.g. torch-ROCm data_ptr(), used
 *     in place on the context stream).  SKE_MEM_HOST inputs must not be
 *     modified until the call returns (pinned ones are read by the DMA engine
 *     directly; the offsets are checked on the copy that is moved).
 *   - packed items: `bytes` + `offs[n+1]` (u32 byte offsets, offs[0] may be
 *     non-zero).  Device byte buffers must stay readable up to the next 8-byte
 *     boundary after bytes+offs[n] (any hipMalloc / torch allocation is).
 *   - a context is single-threaded and stream-ordered; every call returns
 *     after its work on the context stream completed, except ske_swipes_async.
 *   - filters are addressed by a caller-chosen id `fid` < SKE_MAX_FILTERS, HLL
 *     keys by a caller-chosen register-slab slot, Count-Min Sketch tables by a
 *     caller-chosen `cid` < SKE_MAX_CMS, heavy-hitter sets by a caller-chosen
 *     `hid` < SKE_MAX_HH, time profiles by a caller-chosen `tid` < SKE_MAX_TP,
 *     tallies by a caller-chosen `tid` < SKE_MAX_TALLY, seen-row sets by a
 *     caller-chosen `sid` < SKE_MAX_SEEN, row logs by a caller-chosen `rid` <
 *     SKE_MAX_ROWS (spaces of their own).
 *     The facade maps Redis key names to fids / slots /
 *     cids.
 */
#ifndef SKETCH_H
#define SKETCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKE_OK 0
#define SKE_EINVAL -1        /* bad argument */
#define SKE_ENOMEM -2        /* device or host allocation failed */
#define SKE_EHIP -3          /* HIP runtime error (see ske_last_hip_error) */
#define SKE_ENOFILTER -4     /* fid not reserved */
#define SKE_EEXISTS -5       /* BF.RESERVE on an existing key: "ERR item exists" */
#define SKE_EFULL -6         /* non-scaling filter full */
#define SKE_ERANGE -7        /* HLL slot outside the reserved slab */
#define SKE_EBADRATE -8      /* "ERR (0 < error rate range < 1)" */
#define SKE_EBADCAP -9       /* "ERR (capacity should be larger than 0)" */
#define SKE_EBADEXP -10      /* "ERR expansion should be greater or equal to 1" */
#define SKE_EBADHLL -11      /* corrupted HLL string on import */
#define SKE_ETOOLONG -12     /* item longer than the supported maximum */
#define SKE_EBUSY -13        /* device buffers (scratch, HLL slab) pinned by a recorded graph */
#define SKE_ECMSNOKEY -14    /* "CMS: key does not exist" */
#define SKE_ECMSEXISTS -15   /* "CMS: key already exists" */
#define SKE_ECMSWIDTH -16    /* "CMS: invalid width" */
#define SKE_ECMSDEPTH -17    /* "CMS: invalid depth" */
#define SKE_ECMSDIMS -18     /* "CMS: width/depth is not equal" */
#define SKE_ECMSNEG -19      /* "CMS: Number cannot be negative" */
#define SKE_ECMSOVERFLOW -20 /* "CMS: MERGE overflow" */
#define SKE_ECMSERROR -21    /* "CMS: invalid overestimation value" (CMS.INITBYPROB error) */
#define SKE_ECMSPROB -22     /* "CMS: invalid prob value" (CMS.INITBYPROB probability) */
#define SKE_ECMSPARSE -23    /* "CMS: Cannot parse number" */
#define SKE_EHHNOSET -24     /* heavy-hitter set id not in use */
#define SKE_EHHEXISTS -25    /* ske_hh_init on an id in use */
#define SKE_EHHCAP -26       /* capacity_log2 outside [SKE_HH_MIN_LOG2, SKE_HH_MAX_LOG2] */
#define SKE_EHHSPACE -27     /* ske_hh_list: more entries pass than the output arrays hold */
/* -28 is not assigned */
#define SKE_ETPNOSET -29     /* time profile id not in use */
#define SKE_ETPEXISTS -30    /* ske_tp_init on an id in use */
/* -31 is not assigned */
#define SKE_ETALLYNOSET -32  /* tally id not in use */
#define SKE_ETALLYEXISTS -33 /* ske_tally_init on an id in use */
#define SKE_ETALLYCAP -34    /* capacity_log2 outside [SKE_TALLY_MIN_LOG2, SKE_TALLY_MAX_LOG2] */
#define SKE_ETALLYSPACE -35  /* ske_tally_list: more entries pass than the output arrays hold */
/* -36 is not assigned */
#define SKE_ESEENNOSET -37   /* seen set id not in use */
#define SKE_ESEENEXISTS -38  /* ske_seen_init on an id in use */
#define SKE_ESEENCAP -39     /* capacity_log2 outside [SKE_SEEN_MIN_LOG2, SKE_SEEN_MAX_LOG2] */
#define SKE_ESEENCALLS -40   /* the set's 32-bit call counter would wrap: ske_seen_reset starts it again */

/* -41 is not assigned */
#define SKE_EROWSNOLOG -42   /* row log id not in use */
#define SKE_EROWSEXISTS -43  /* ske_rows_init on an id in use */
#define SKE_EROWSCAP -44     /* capacity_log2 outside [SKE_ROWS_MIN_LOG2, SKE_ROWS_MAX_LOG2] */
#define SKE_EROWSSPACE -45   /* ske_rows_select / ske_rows_group: more rows (groups) pass than the output arrays hold */

#define SKE_MEM_HOST 0
#define SKE_MEM_DEVICE 1

#define SKE_MAX_FILTERS 4096
#define SKE_MAX_LINKS 48
#define SKE_MAX_CMS 4096
#define SKE_CMS_MAX_DEPTH 64
#define SKE_CMS_MAX_CELLS (1u << 28) /* width * depth stays below this */
#define SKE_CMS_MAX_MERGE 64
#define SKE_MAX_HH 256
#define SKE_HH_MIN_LOG2 8
#define SKE_HH_MAX_LOG2 24
#define SKE_HH_ID_BYTES 16   /* the longest id a heavy-hitter set holds */
#define SKE_HH_MAX_PROBES 128 /* slots one insert looks at before it gives up */
#define SKE_HH_LOAD_DEN 2    /* new ids are refused once used >= capacity / SKE_HH_LOAD_DEN */
#define SKE_HH_MAX_RANKS 16  /* ranks one ske_hh_select carries */
#define SKE_MAX_TP 256
#define SKE_TP_BINS 168      /* weekday * 24 + hour, Monday = 0 */
#define SKE_MAX_TALLY 256
#define SKE_TALLY_KEY_BYTES 32 /* the longest key a tally groups */
#define SKE_TALLY_MIN_LOG2 8
#define SKE_TALLY_MAX_LOG2 24
#define SKE_TALLY_MAX_PROBES 128 /* slots one insert-or-add looks at before it gives up */
#define SKE_TALLY_LOAD_DEN 2   /* new keys are refused once used >= capacity / SKE_TALLY_LOAD_DEN */
#define SKE_TALLY_MAX_TOP 16   /* entries per end one ske_tally_top returns */
#define SKE_MAX_SEEN 256
#define SKE_SEEN_MIN_LOG2 8
#define SKE_SEEN_MAX_LOG2 30
#define SKE_SEEN_MAX_PROBES 128 /* slots one walk looks at before it gives up */
#define SKE_SEEN_LOAD_DEN 2    /* new keys find no slot once used >= capacity / SKE_SEEN_LOAD_DEN */
#define SKE_SEEN_FIRST 0       /* ske_seen_add's answer bytes: count this row, */
#define SKE_SEEN_REPEAT 1      /*   a repeat, */
#define SKE_SEEN_SKIPPED 2     /*   the mask kept the item out */
#define SKE_MAX_ROWS 8
#define SKE_ROWS_MIN_LOG2 8
#define SKE_ROWS_MAX_LOG2 28   /* a position fits a u32 */
#define SKE_ROWS_BLOCK 256     /* items per workgroup and tile of an append: positions are tile prefix + rank */
#define SKE_ROWS_ROW_BYTES 25  /* lec 8, epoch 8, id 8, valid 1 */
#define SKE_ROWS_BY_STUDENT 0   /* ske_rows_group: key = id, groups ascending, signed */
#define SKE_ROWS_BY_LECTURE 1   /*   key = lecture digest, groups ascending, unsigned */
#define SKE_ROWS_VALID_ANY 0    /* ske_rows_group / ske_rows_profile: rows of either validity count, */
#define SKE_ROWS_VALID_ONLY 1   /*   rows with is_valid 1, */
#define SKE_ROWS_INVALID_ONLY 2 /*   rows with is_valid 0 */
#define SKE_HLL_REGISTERS 16384
#define SKE_HLL_DENSE_BYTES 12288
#define SKE_HLL_DUMP_MAX_KEYS (1u << 18)   /* 2^18 * 12304 B < 2^32: u32 offsets suffice */
#define SKE_HLL_DUMP_CARD 1                /* flags: write the cached cardinality */

typedef struct ske_ctx ske_ctx;

typedef struct {
    uint64_t capacity;      /* sum of link entries   (BF.INFO Capacity) */
    uint64_t size_bytes;    /* bytes of all bit arrays + headers (BF.INFO Size) */
    uint32_t nfilters;      /* links in the chain    (BF.INFO Number of filters) */
    uint32_t expansion;     /* growth factor         (BF.INFO Expansion rate) */
    uint64_t inserted;      /* items added           (BF.INFO Number of items inserted) */
    int32_t nonscaling;
    int32_t pad_;
} ske_bf_info_t;

typedef struct {
    uint64_t entries;  /* bloom->entries */
    uint64_t bytes;    /* bloom->bytes */
    uint64_t bits;     /* bloom->bits (modulus of the probe sequence) */
    uint64_t size;     /* SBLink.size (items added to this link) */
    double error;      /* bloom->error */
    double bpe;        /* bloom->bpe */
    int32_t hashes;    /* bloom->hashes (k) */
    int32_t pad_;
} ske_bf_link_t;

/* Synthetic swipe stream (counter-based, device-side).  See DESIGN.md
 * "Synthetic workload" for the exact definition; tests restate it in numpy. */
typedef struct {
    uint64_t seed;
    uint64_t id_lo, id_hi;        /* IDs in [id_lo, id_hi), all with the same digit count */
    uint64_t n_members;           /* valid population: first n_members of the permutation */
    uint64_t perm_mul, perm_add;  /* member(i) = id_lo + (perm_mul*i + perm_add) mod R */
    uint64_t perm_mul_inv;        /* perm_mul^-1 mod R (R = id_hi - id_lo < 2^32) */
    uint32_t invalid_thresh;      /* P(invalid) * 2^32 */
    uint32_t near_thresh;         /* P(near-collision | invalid) * 2^32 */
    uint32_t n_keys;              /* HLL keys of this stream: slot_base + [0, n_keys) */
    uint32_t slot_base;
    const uint32_t *key_cdf;      /* optional device table (n_keys u32 CDF * 2^32); NULL = uniform */
} ske_gen_params_t;

/* ---- context ---- */
int ske_open(int device, ske_ctx **out);
int ske_close(ske_ctx *ctx);
const char *ske_strerror(int code);
const char *ske_last_hip_error(ske_ctx *ctx);
int ske_set_stream(ske_ctx *ctx, void *hip_stream); /* NULL = the context's own stream */
int ske_get_stream(ske_ctx *ctx, void **hip_stream); /* the stream calls enqueue on now */
/* Wait for the context stream.  Also reports (and clears) the sticky device
 * error word that enqueue-only calls leave set: SKE_ERANGE when a valid swipe
 * named an HLL slot outside the slab since the last check.  The word is read
 * and cleared by device-side atomic exchanges (no flag set concurrently on
 * another stream is lost).  A synchronous K1 / PFADD / ingest call reports
 * the out-of-range slots flagged while it ran: its own, and those of any work
 * that was running at the same time on other streams (enqueue-only calls
 * still in flight may be attributed to it -- the flag is one device word);
 * what finished before it began is kept for the next ske_sync /
 * ske_check_errors. */
int ske_sync(ske_ctx *ctx);
int ske_check_errors(ske_ctx *ctx);  /* the same check: sync + report + clear */
int ske_device_alloc(ske_ctx *ctx, uint64_t bytes, void **out); /* device scratch for callers */
int ske_device_free(ske_ctx *ctx, void *p);
int ske_memcpy(ske_ctx *ctx, void *dst, const void *src, uint64_t bytes, int kind); /* 0 H2D 1 D2H 2 D2D */

/* ---- Bloom (RedisBloom SBChain) ----
 * BF.RESERVE key error_rate capacity [EXPANSION e] [NONSCALING]
 *   replaces: execute_command('BF.RESERVE', ...) attendance_processor.py:83-88
 *   (also the implicit auto-create of BF.ADD: data_generator.py:59-63). */
int ske_bf_reserve(ske_ctx *ctx, uint32_t fid, double error_rate, uint64_t capacity,
                   uint32_t expansion, int nonscaling);
int ske_bf_exists_key(ske_ctx *ctx, uint32_t fid); /* 1 if reserved, 0 if not */
int ske_bf_free(ske_ctx *ctx, uint32_t fid);
/* BF.MADD key item...  (BF.ADD = n 1), sequential RedisBloom semantics:
 *   out[i] = 1 added, 0 already present, -2 non-scaling filter full.
 *   replaces: execute_command('BF.ADD', BLOOM_FILTER_KEY, id) data_generator.py:59-63 */
int ske_bf_madd(ske_ctx *ctx, uint32_t fid, const uint8_t *bytes, const uint32_t *offs,
                uint64_t n, int8_t *out_or_null, int mem);
/* BF.MEXISTS key item...  (BF.EXISTS = n 1); a missing key answers 0s.
 *   replaces: execute_command('BF.EXISTS', BLOOM_FILTER_KEY, student_id)
 *   attendance_processor.py:109-113 and the probe at :78 */
int ske_bf_mexists(ske_ctx *ctx, uint32_t fid, const uint8_t *bytes, const uint32_t *offs,
                   uint64_t n, uint8_t *out, int mem);
/* BF.INFO / BF.DEBUG and BF.SCANDUMP-style raw bit arrays */
int ske_bf_info(ske_ctx *ctx, uint32_t fid, ske_bf_info_t *out);
int ske_bf_link_info(ske_ctx *ctx, uint32_t fid, uint32_t link, ske_bf_link_t *out);
int ske_bf_export_link(ske_ctx *ctx, uint32_t fid, uint32_t link, uint8_t *out, uint64_t cap);
int ske_bf_import_link(ske_ctx *ctx, uint32_t fid, uint32_t link, const uint8_t *in,
                       uint64_t nbytes);
/* BF.LOADCHUNK key <iter> <data>: bytes [offset, offset + nbytes) of one link's
 * bit array (SBChain_LoadEncodedChunk); the range must lie inside the link. */
int ske_bf_link_write(ske_ctx *ctx, uint32_t fid, uint32_t link, uint64_t offset,
                      const uint8_t *in, uint64_t nbytes);
/* BF.LOADCHUNK key 1 <header>: a chain with exactly the given links (geometry
 * and sizes as dumped by BF.SCANDUMP's header chunk, zeroed bit arrays; the
 * data chunks then go in through ske_bf_import_link / the facade).  Each
 * link needs bits == bytes * 8, 1 <= hashes <= 64.  SKE_EEXISTS if fid exists.
 *   replaces: SB_NewChainFromHeader (RedisBloom src/sb.c) behind BF.LOADCHUNK */
int ske_bf_load_header(ske_ctx *ctx, uint32_t fid, const ske_bf_link_t *links, uint32_t nlinks,
                       uint64_t inserted, uint32_t expansion, int nonscaling);

/* ---- HyperLogLog register slab (Redis p=14, one byte per register) ---- */
int ske_hll_reserve(ske_ctx *ctx, uint32_t nslots);  /* grow the slab to >= nslots keys */
uint32_t ske_hll_capacity(ske_ctx *ctx);
int ske_hll_clear(ske_ctx *ctx, uint32_t slot);      /* new / deleted key: zero registers */
/* PFADD key element...  for many (key, element) pairs at once.
 *   changed_or_null: per-element "this element raised a register" in the
 *   given order (sequential Redis semantics); the facade folds it per call.
 *   replaces: redis_client.pfadd(hll_key, student_id) attendance_processor.py:127-129 */
int ske_hll_pfadd(ske_ctx *ctx, const uint32_t *slot, const uint8_t *bytes,
                  const uint32_t *offs, uint64_t n, uint8_t *changed_or_null, int mem);
/* PFCOUNT key [key ...] (union), one answer.  attendance_processor.py:152 */
int ske_hll_pfcount(ske_ctx *ctx, const uint32_t *slots, uint32_t nkeys, uint64_t *out);
/* PFCOUNT of each key separately (rankings, attendance_analysis.py:87-97 as
 * README.md:179 describes); slots == NULL: keys 0..nkeys-1 of the slab.
 * Group form: union over slots[goffs[g]..goffs[g+1]).  With SKE_MEM_DEVICE the
 * slot list of the each form is range-checked on the device (SKE_ERANGE). */
int ske_hll_pfcount_each(ske_ctx *ctx, const uint32_t *slots, uint32_t nkeys, uint64_t *out,
                         int mem);
int ske_hll_pfcount_groups(ske_ctx *ctx, const uint32_t *slots, const uint32_t *goffs,
                           uint32_t ngroups, uint64_t *out, int mem);
/* PFMERGE dst src...  (dst's own registers take part, as in Redis) */
int ske_hll_pfmerge(ske_ctx *ctx, uint32_t dst, const uint32_t *srcs, uint32_t n);
/* the same with a device-resident source list (a plan kept on the GPU, e.g.
 * the campus PFMERGE of C5's 1.8M day keys): its range is checked on the
 * device (SKE_ERANGE), nothing is staged from the host.
 *   replaces: PFMERGE (north star; attendance_analysis.py:87-97 as README.md:179) */
int ske_hll_pfmerge_dev(ske_ctx *ctx, uint32_t dst, const uint32_t *srcs_dev, uint32_t n);
int ske_hll_histogram(ske_ctx *ctx, uint32_t slot, uint32_t *out64);
int ske_hll_export_raw(ske_ctx *ctx, uint32_t slot, uint8_t *out16384);
int ske_hll_export_dense(ske_ctx *ctx, uint32_t slot, uint8_t *out12288);
int ske_hll_import_raw(ske_ctx *ctx, uint32_t slot, const uint8_t *regs16384);
/* raw device pointer of the slab (slot s at + s*16384), for RCCL max-reduce */
int ske_hll_slab(ske_ctx *ctx, void **dev_ptr, uint64_t *bytes);
/* dst_dev[g*16384 ..] = register max over slots[goffs[g]..goffs[g+1]) (K3 into an
 * external device buffer, e.g. a torch tensor that RCCL then max-reduces);
 * an empty group yields zeros.  slots / goffs are host arrays. */
int ske_hll_merge_groups_dev(ske_ctx *ctx, const uint32_t *slots, const uint32_t *goffs,
                             uint32_t ngroups, uint8_t *dst_dev);
/* estimator only: PFCOUNT of raw register arrays already on the device */
int ske_hll_count_raw_dev(ske_ctx *ctx, const uint8_t *regs_dev, uint32_t nkeys, uint64_t *out);
/* Many keys as Redis stores them (GET of an HLL key), encoded on the device:
 * a 16-byte header ("HYLL", encoding 0 dense / 1 sparse, 3 zero bytes, 8
 * cardinality bytes: cache-invalid, or with SKE_HLL_DUMP_CARD the key's PFCOUNT)
 * and the canonical sparse payload (maximal runs) when every register is <= 32
 * and it is at most sparse_max_bytes long (server.hll_sparse_max_bytes, 3000 in
 * Redis), else the 12288-byte dense payload.  slots == NULL: keys 0..nkeys-1; a
 * slot may repeat.  mem covers every array argument.  At most
 * SKE_HLL_DUMP_MAX_KEYS keys a call (SKE_EINVAL); a slot outside the slab gives
 * SKE_ERANGE and nothing is written.  Synchronous on the context stream.
 *   ske_hll_dump_sizes: offs_out[nkeys+1], the byte offset of every key's
 *     string, offs_out[nkeys] = total.  Writes no strings.
 *   ske_hll_dump: the strings, back to back in out[0 .. total), and the same
 *     offsets; cap < total -> SKE_EINVAL, out and offs_out untouched.
 *   replaces: GET key on an HLL key, per key dump_hll */
int ske_hll_dump_sizes(ske_ctx *ctx, const uint32_t *slots, uint32_t nkeys, uint32_t sparse_max_bytes,
                       uint32_t *offs_out, int mem);
int ske_hll_dump(ske_ctx *ctx, const uint32_t *slots, uint32_t nkeys, uint32_t sparse_max_bytes, int flags,
                 uint8_t *out, uint64_t cap, uint32_t *offs_out, int mem);
/* SET of nkeys HLL strings, decoded on the device: string i is
 * blob[offs[i] .. offs[i+1]) (any byte alignment; offs never decreasing, else
 * SKE_EINVAL), either encoding, canonical or not.  status_or_null[i] = 0
 * loaded (the row of slots[i] is replaced), 1 not an HLL string (shorter than
 * 16 bytes or another magic), 2 corrupted (a dense payload not 12288 bytes or
 * a register above 51; sparse runs that do not end exactly at register 16384,
 * an XZERO without its second byte; another encoding byte); the row of a key
 * with a non-zero status is untouched, every other key of the call is loaded.
 * Returns SKE_EBADHLL when any status is non-zero.  The slots must be distinct
 * (with a repeated slot which string it ends up holding is unspecified);
 * slots == NULL: keys 0..nkeys-1.  Limits, range check and mem as ske_hll_dump.
 *   replaces: SET key <HYLL string>, per key load_hll */
int ske_hll_load(ske_ctx *ctx, const uint32_t *slots, uint32_t nkeys, const uint8_t *blob,
                 const uint32_t *offs, uint8_t *status_or_null, int mem);

/* ---- Count-Min Sketch (RedisBloom src/cms.c) ----
 * A table of `depth` rows of `width` u32 counters (row-major) and a u64 count
 * of all increments; the cell of an item in row i is
 * MurmurHash2(item, len, seed = i) % width (the 32-bit MurmurHash2).  Tables
 * are addressed by a caller-chosen cid < SKE_MAX_CMS; the context owns them.
 * No reference counterpart in its Redis calls: the per-student counts of
 * attendance_analysis.py:99-118 and :65-75 come from pandas over Cassandra
 * rows; these entry points keep them beside the swipe path instead.
 * Limits of this build: depth <= SKE_CMS_MAX_DEPTH, width * depth <
 * SKE_CMS_MAX_CELLS, n < 2^32 - 1 items per call. */
typedef struct {
    uint64_t width;
    uint64_t depth;
    uint64_t count;
} ske_cms_info_t;
/* CMS.INITBYPROB's dimensions: width = ceil(2 / error), depth =
 * ceil(log10f(prob) / log10f(0.5f)); both arguments in (0, 1), else
 * SKE_ECMSERROR / SKE_ECMSPROB.  Host only, no context. */
int ske_cms_dims_from_prob(double error, double prob, uint32_t *width, uint32_t *depth);
/* CMS.INITBYDIM key width depth (a zeroed table).  SKE_ECMSEXISTS when cid is
 * in use, SKE_ECMSWIDTH / SKE_ECMSDEPTH for a zero or out-of-limit dimension. */
int ske_cms_init(ske_ctx *ctx, uint32_t cid, uint32_t width, uint32_t depth);
int ske_cms_free(ske_ctx *ctx, uint32_t cid);
/* CMS.INFO key */
int ske_cms_info(ske_ctx *ctx, uint32_t cid, ske_cms_info_t *out);
/* CMS.INCRBY key item increment [item increment ...]: every row's cell of
 * item i += incr[i] (1 each when incr is NULL), a cell that would pass
 * 0xffffffff stays there; count += incr[i].
 *   reply != NULL: the sequential form -- items in order, reply[i] = the
 *     minimum of item i's cells right after its update (repeats and
 *     collisions inside the call show); one wavefront, not a throughput path;
 *   reply == NULL: the bulk form -- order-free, every cell ends at
 *     min(true sum, 2^32 - 1), the same table the sequential form leaves. */
int ske_cms_incrby(ske_ctx *ctx, uint32_t cid, const uint8_t *bytes, const uint32_t *offs,
                   uint64_t n, const uint32_t *incr_or_null, uint32_t *reply_or_null, int mem);
/* The bulk form over fixed-width ids on the device (id i = the `width` bytes
 * at ids + i * width), enqueue only and graph-capturable: the form that
 * follows ske_swipes*_async on the same stream.  mask (may be NULL): only
 * items with mask[i] == want (0 or 1) count -- K1's answer bytes read in
 * place ("count this swipe's student if it was invalid", or valid). */
int ske_cms_add_fixed_async(ske_ctx *ctx, uint32_t cid, const uint8_t *ids, uint32_t width,
                            uint64_t n, const uint32_t *incr_or_null, const uint8_t *mask_or_null,
                            int want);
/* The same over packed ids on the device (id i = bytes[offs[i] .. offs[i + 1]),
 * offs n + 1 entries; bytes readable to the next 8-byte boundary behind the
 * last id), enqueue only and graph-capturable: the form that follows
 * ske_ingest_dense.  An empty id counts as the empty string, as in
 * ske_cms_incrby. */
int ske_cms_add_packed_async(ske_ctx *ctx, uint32_t cid, const uint8_t *bytes_dev, const uint32_t *offs_dev,
                             uint64_t n, const uint32_t *incr_or_null, const uint8_t *mask_or_null,
                             int want);
/* CMS.QUERY key item...: out[i] = the minimum of item i's cells */
int ske_cms_query(ske_ctx *ctx, uint32_t cid, const uint8_t *bytes, const uint32_t *offs,
                  uint64_t n, uint32_t *out, int mem);
/* CMS.MERGE dst nsrc src... [WEIGHTS w...]: dst[cell] = sum of src_k[cell] *
 * w_k (weights NULL: 1 each), count likewise; dst is overwritten and takes
 * part only when listed as a source.  SKE_ECMSDIMS unless every table has
 * dst's dimensions.  Sums are formed in signed 64-bit arithmetic; a cell
 * outside [0, 2^32 - 1], a count outside [0, 2^64 - 1] or a 64-bit overflow
 * on the way fails the call with SKE_ECMSOVERFLOW before dst is written.
 * 1 <= nsrc <= SKE_CMS_MAX_MERGE. */
int ske_cms_merge(ske_ctx *ctx, uint32_t dst, const uint32_t *srcs, const int64_t *weights_or_null,
                  uint32_t nsrc);
/* the whole table, row-major (cap_cells >= width * depth), and back: import
 * overwrites cells and count (ncells must equal width * depth) */
int ske_cms_export(ske_ctx *ctx, uint32_t cid, uint32_t *out, uint64_t cap_cells);
int ske_cms_import(ske_ctx *ctx, uint32_t cid, const uint32_t *in, uint64_t ncells, uint64_t count);
/* The table's device pointer (row-major cells, *ncells = width * depth), as
 * ske_hll_slab gives the slab's: the source of an all-gather across contexts.
 * The allocation is padded to the next 16 bytes, so ((*ncells + 3) & ~3) cells
 * are readable.  The count is not part of it (ske_cms_info). */
int ske_cms_table_dev(ske_ctx *ctx, uint32_t cid, void **cells_dev, uint64_t *ncells);
/* dst = the saturating sum of ntables caller-owned device tables (several
 * contexts' tables, gathered): table k is the cells at tables_dev + k *
 * stride_cells, stride_cells a multiple of 4 and at least dst's width * depth,
 * tables_dev 16-byte aligned (else SKE_EINVAL); counts is a HOST array of
 * ntables counts.  dst is overwritten: cell = min(sum over the tables,
 * 2^32 - 1), count = sum of counts.  Saturation, not ske_cms_merge's overflow
 * error: the bulk add saturates, and this is the table one context would have
 * built from all the increments.  A count sum beyond 2^64 - 1: SKE_ECMSOVERFLOW
 * before dst is written.  1 <= ntables <= SKE_CMS_MAX_MERGE.  Enqueue only. */
int ske_cms_sum_dev(ske_ctx *ctx, uint32_t dst_cid, const uint32_t *tables_dev, uint64_t stride_cells,
                    uint32_t ntables, const uint64_t *counts);

/* ---- heavy hitters beside a Count-Min Sketch table ----
 * A set of distinct ids (at most SKE_HH_ID_BYTES bytes each) in 2^capacity_log2
 * device slots, addressed by a caller-chosen hid < SKE_MAX_HH; the context owns
 * it.  A track adds the ids of a batch whose estimate in table `cid` (CMS.QUERY,
 * the table as it stands in stream order, so after the batch's adds) reaches
 * `threshold`; a list reads the members' current estimates back.  The result
 * depends on the sequence of batches, never on the order inside one: cells only
 * grow, and an id is judged at the batches it occurs in (an id seen only early,
 * below the threshold, is not added when later collisions raise its cells).
 * No reference counterpart in its Redis calls; the lists are those of
 * attendance_analysis.py:99-118.  RedisBloom's TOPK (HeavyKeeper) draws random
 * numbers per colliding increment and is not offered.
 *
 * Limits: ids with the same 64-bit digest (MurmurHash64A, the Bloom seed; 0
 * mapped to 1) are one entry, the first to claim the slot names it.  An insert
 * looks at SKE_HH_MAX_PROBES slots at most and new ids are refused once
 * capacity / SKE_HH_LOAD_DEN slots are used (a batch in flight may pass that
 * mark by the claims racing at that moment, never the capacity); a refused id is
 * dropped and the set's sticky overflow word is set: `complete` is 0 from then
 * on, until ske_hh_reset.  Entries are never removed one by one.
 * Guarantee while complete: every id whose true count reaches T, and whose
 * occurrences all went through a track with threshold <= T, is listed at T --
 * at its last occurrence its estimate is at least its true count. */
typedef struct {
    uint64_t capacity;  /* slots */
    uint64_t used;      /* ids held */
    uint64_t overflow;  /* non-zero once an insert was refused */
} ske_hh_info_t;
/* SKE_EHHEXISTS when hid is in use, SKE_EHHCAP for a capacity out of range */
int ske_hh_init(ske_ctx *ctx, uint32_t hid, uint32_t capacity_log2);
/* SKE_EBUSY while a recorded graph is alive or being recorded */
int ske_hh_free(ske_ctx *ctx, uint32_t hid);
/* an empty, complete set again (slots, used and overflow zeroed) */
int ske_hh_reset(ske_ctx *ctx, uint32_t hid);
int ske_hh_info(ske_ctx *ctx, uint32_t hid, ske_hh_info_t *out);
/* Fixed-width ids on the device (id i = the `width` bytes at ids + i * width),
 * enqueue only and graph-capturable: the form that follows
 * ske_swipes_fixed_async + ske_cms_add_fixed_async on the same stream.  mask
 * (may be NULL): only items with mask[i] == want (0 or 1) are looked at.
 * width > SKE_HH_ID_BYTES: SKE_ETOOLONG; threshold == 0, width == 0 or another
 * want: SKE_EINVAL; a missing table: SKE_ECMSNOKEY (the table is looked up by
 * cid at every call). */
int ske_hh_track_fixed_async(ske_ctx *ctx, uint32_t hid, uint32_t cid, const uint8_t *ids, uint32_t width,
                             uint64_t n, const uint8_t *mask_or_null, int want, uint32_t threshold);
/* The same over packed ids on the device (bytes + offs[n + 1], as
 * ske_cms_add_packed_async), enqueue only and graph-capturable.  It has no
 * wait and so no error of its own for an id longer than SKE_HH_ID_BYTES: the
 * id is skipped and the set's sticky overflow word is set, so listings answer
 * complete = 0 ("may miss students") until ske_hh_reset.  An empty id is
 * tracked as the empty string, as in ske_hh_track. */
int ske_hh_track_packed_async(ske_ctx *ctx, uint32_t hid, uint32_t cid, const uint8_t *bytes_dev,
                              const uint32_t *offs_dev, uint64_t n, const uint8_t *mask_or_null, int want,
                              uint32_t threshold);
/* The packed form (bytes + offs[n + 1]); returns when done.  An id longer than
 * SKE_HH_ID_BYTES fails the call with SKE_ETOOLONG: with SKE_MEM_HOST before
 * anything is tracked, with SKE_MEM_DEVICE after the batch's other ids were. */
int ske_hh_track(ske_ctx *ctx, uint32_t hid, uint32_t cid, const uint8_t *bytes, const uint32_t *offs,
                 uint64_t n, uint32_t threshold, int mem);
/* Every member whose current estimate in table cid is >= threshold, sorted by
 * estimate descending, then id bytes ascending (host arrays: out_ids cap x
 * SKE_HH_ID_BYTES bytes, zero padded; out_lens and out_est cap entries).
 * *n_out = how many pass; more than cap: SKE_EHHSPACE and nothing is written
 * (cap >= used always suffices).  *complete = 0 once an insert was refused. */
int ske_hh_list(ske_ctx *ctx, uint32_t hid, uint32_t cid, uint32_t threshold, uint8_t *out_ids,
                uint32_t *out_lens, uint32_t *out_est, uint64_t cap, uint64_t *n_out, int *complete);
/* The statistics of a set's current estimates, computed on the device: over
 * the members whose estimate in table cid is >= threshold (0 is legal: every
 * member), their number, the exact sums of the estimates and of their squares,
 * the extremes and the two middle order statistics (the median is their mean).
 * A set tracked at threshold 1 holds every id that ever counted, so these are
 * the population statistics of attendance_analysis.py:68-69 and :99-103.  All
 * integer arithmetic: exact, and identical from run to run.  A square is
 * split into its low and high 32 bits and the halves are summed apart; at the
 * largest set (2^SKE_HH_MAX_LOG2 members) each sum stays below 2^56, so
 * neither overflows nor carries into the other.  Nothing but this struct
 * crosses to the host.  Neither call changes the set or the table; both
 * return when done and, as ske_hh_reset, answer SKE_EBUSY while a capture is
 * recording.  SKE_EHHNOSET / SKE_ECMSNOKEY as ske_hh_list. */
typedef struct {
    uint64_t n;              /* members whose current estimate is >= threshold */
    uint64_t sum;            /* of those estimates */
    uint64_t sq_lo, sq_hi;   /* sum of squares = sq_hi * 2^32 + sq_lo (each word below 2^56) */
    uint32_t min, max;       /* 0, 0 when n == 0 */
    uint32_t med_lo, med_hi; /* the (n-1)/2-th and n/2-th smallest (0-based); 0, 0 when n == 0 */
    uint32_t complete;       /* 0 once an insert was refused, as ske_hh_list */
    uint32_t reserved;       /* 0 */
} ske_hh_stats_t;            /* 56 bytes */
int ske_hh_stats(ske_ctx *ctx, uint32_t hid, uint32_t cid, uint32_t threshold, ske_hh_stats_t *out);
/* out_est[j] = the ranks[j]-th smallest passing estimate (0-based; ranks in any
 * order, repeats allowed; 1 <= nranks <= SKE_HH_MAX_RANKS, else SKE_EINVAL): a
 * radix select on the device, 8 bits a round.  *n_out = how many pass; any
 * ranks[j] >= *n_out: SKE_EINVAL, *n_out is still written and out_est is not
 * touched. */
int ske_hh_select(ske_ctx *ctx, uint32_t hid, uint32_t cid, uint32_t threshold, const uint64_t *ranks,
                  uint32_t nranks, uint32_t *out_est, uint64_t *n_out);
/* The union of sets across contexts.  Export: every member, unordered, into
 * caller-owned device arrays (ids_dev 8-byte aligned, cap x SKE_HH_ID_BYTES
 * zero-padded bytes; lens_dev cap entries); no table, no estimates.  *n_out =
 * the members, *overflow_out = the sticky overflow word; more members than
 * cap: SKE_EHHSPACE with both still written (cap >= used always suffices).
 * Returns when done; SKE_EBUSY while a capture is recording.
 * Merge: every entry of such arrays joins the set, with no threshold; the same
 * id any number of times lands once.  The bytes behind an entry's length are
 * masked, not trusted; an entry with a length over SKE_HH_ID_BYTES is skipped
 * and sets the overflow word, as ske_hh_track_packed_async does; the load limit
 * and the probe bound refuse as a track's do.  foreign_overflow != 0 (the
 * source's overflow word) sets the overflow word: a source that refused an id
 * makes the union incomplete.  n < 2^32 - 1.  Enqueue only. */
int ske_hh_export_dev(ske_ctx *ctx, uint32_t hid, uint8_t *ids_dev, uint32_t *lens_dev, uint64_t cap,
                      uint64_t *n_out, uint32_t *overflow_out);
int ske_hh_merge_dev(ske_ctx *ctx, uint32_t hid, const uint8_t *ids_dev, const uint32_t *lens_dev, uint64_t n,
                     uint32_t foreign_overflow);

/* ---- time profile: weekday x hour counters of the swipes' times ----
 * SKE_TP_BINS u64 counters on the device, addressed by a caller-chosen tid <
 * SKE_MAX_TP; the context owns them.  A swipe's time is an int64_t `epoch`,
 * seconds since 1970-01-01T00:00:00 UTC; every value is legal.  By floor
 * division (a negative epoch does not truncate toward zero):
 *   day = floor(epoch / 86400), sod = epoch - day * 86400 in [0, 86400),
 *   hour = sod / 3600, dow = (day + 3) mod 7 in [0, 7) with Monday = 0
 *   (datetime.weekday(); 1970-01-01 was a Thursday), bin = dow * 24 + hour.
 * No reference counterpart in its Redis calls: "Attendance by Day"
 * (attendance_analysis.py:77-85) is the counters summed per weekday, and the
 * late bytes turn ske_cms_add_fixed_async / ske_hh_track_fixed_async into the
 * counters of "Habitual Latecomers" (:65-75). */
int ske_tp_init(ske_ctx *ctx, uint32_t tid);  /* zeroed; SKE_ETPEXISTS when tid is in use */
/* SKE_EBUSY while a recorded graph is alive or being recorded */
int ske_tp_free(ske_ctx *ctx, uint32_t tid);
int ske_tp_reset(ske_ctx *ctx, uint32_t tid); /* every counter zero again */
/* the counters into a host array of SKE_TP_BINS entries; returns when done */
int ske_tp_read(ske_ctx *ctx, uint32_t tid, uint64_t *out168);
/* overwrite the counters from a host array (restore; the sum of several ranks'
 * profiles, formed on the host) */
int ske_tp_import(ske_ctx *ctx, uint32_t tid, const uint64_t *in168);
/* One batch of times on the device (epoch 8-byte aligned), enqueue only and
 * graph-capturable.  counts[bin(epoch[i])] += 1 for every i the mask lets
 * through (mask NULL, or mask[i] == want, want 0 or 1).  late (may be NULL):
 * late[i] = sod(epoch[i]) >= late_from ? 1 : 0 for EVERY i, whatever the mask
 * says (the reference counts valid and invalid rows alike); late_from in
 * [0, 86400], 86400: nobody is late.  n == 0 only checks the arguments.
 * Another want, late_from > 86400, n >= 2^32 - 1 or epoch NULL with n > 0:
 * SKE_EINVAL; a tid not in use: SKE_ETPNOSET. */
int ske_tp_add_async(ske_ctx *ctx, uint32_t tid, const int64_t *epoch, uint64_t n,
                     const uint8_t *mask_or_null, int want, uint32_t late_from, uint8_t *late_or_null);

/* ---- tallies: exact event counts per key ----
 * The group-by-count of a string column: every item of a batch adds 1 to its
 * key's `events` and, when the batch has a mask and the item's mask byte is 1,
 * 1 to its key's `valid` (invalid = events - valid; a caller without validity
 * passes no mask and reads `events` alone).  A key is any byte string of at
 * most SKE_TALLY_KEY_BYTES bytes; the empty string is a key and counts; the
 * length takes part in identity (b"A" and b"A\0" are two keys).  A tally is an
 * insert-only open-addressing table of 2^capacity_log2 device slots, addressed
 * by a caller-chosen tid < SKE_MAX_TALLY; the context owns it.
 *   replaces: df.groupby('lecture_id').size() of "Lecture Attendance Rankings"
 *   (attendance_analysis.py:87-97, there pandas over Cassandra rows), and the
 *   attendance_records count of attendance_processor.py:154-165.
 * Results are integers and order-free inside and across batches: identical from
 * run to run, apart from which of two digest-colliding keys names an entry.
 *
 * Limits: keys with the same 64-bit digest (MurmurHash64A of the key bytes, the
 * Bloom seed; 0 mapped to 1) are one entry, the first to claim the slot names
 * it.  An insert-or-add looks at SKE_TALLY_MAX_PROBES slots at most, and new
 * keys are refused once capacity / SKE_TALLY_LOAD_DEN slots are used (a batch in
 * flight may pass that mark by the claims racing at that moment, never the
 * capacity).  A refused item is not grouped: its counts go to dropped_events /
 * dropped_valid and the sticky overflow word is set, as for a key longer than
 * SKE_TALLY_KEY_BYTES.  So always, complete or not,
 *   sum of all events + dropped_events == taken,  the same for valid,
 * where taken counts every item looked at.  While overflow is 0 every listed
 * count is exact.  Once it is set listed counts are lower bounds, also those of
 * keys the table holds: the load bound is read before the claim, so one thread
 * can be refused a key at the moment another claims it.  Entries are never
 * removed one by one; ske_tally_reset empties the tally. */
typedef struct {
    uint64_t capacity;        /* slots */
    uint64_t used;            /* keys held */
    uint64_t overflow;        /* non-zero once an item was refused */
    uint64_t taken;           /* items looked at */
    uint64_t dropped_events;  /* items not grouped */
    uint64_t dropped_valid;   /* of those, the ones whose mask byte was 1 */
} ske_tally_info_t;
/* zeroed; SKE_ETALLYEXISTS when tid is in use, SKE_ETALLYCAP for a capacity out of range */
int ske_tally_init(ske_ctx *ctx, uint32_t tid, uint32_t capacity_log2);
/* SKE_EBUSY while a recorded graph is alive or being recorded */
int ske_tally_free(ske_ctx *ctx, uint32_t tid);
/* an empty, complete tally again (slots, counters and the head zeroed) */
int ske_tally_reset(ske_ctx *ctx, uint32_t tid);
int ske_tally_info(ske_ctx *ctx, uint32_t tid, ske_tally_info_t *out);
/* One batch of keys on the device, enqueue only and graph-capturable; n < 2^32 - 1;
 * mask NULL or one byte per item.  A key longer than SKE_TALLY_KEY_BYTES has no
 * error path here: it is not grouped, counts as dropped and sets overflow.
 *   packed: key i = bytes[offs[i] .. offs[i + 1]) (offs n + 1 entries; bytes
 *     readable to the next 8-byte boundary behind the last key);
 *   fixed: key i = the `width` bytes at keys + i * width (width 0: SKE_EINVAL);
 *   spans: key i = bytes[start[i] .. start[i] + len[i]), taken only when status
 *     is NULL or status[i] == 0 -- a column of ske_ingest_parse read in place
 *     (lec_start / lec_len, masked by the BF.EXISTS bytes).  Only the aligned
 *     8-byte words that hold a byte of the span are read, never past the 8-byte
 *     boundary behind bytes. */
int ske_tally_add_packed_async(ske_ctx *ctx, uint32_t tid, const uint8_t *bytes_dev, const uint32_t *offs_dev,
                               uint64_t n, const uint8_t *mask_or_null);
int ske_tally_add_fixed_async(ske_ctx *ctx, uint32_t tid, const uint8_t *keys_dev, uint32_t width, uint64_t n,
                              const uint8_t *mask_or_null);
int ske_tally_add_spans_async(ske_ctx *ctx, uint32_t tid, const uint8_t *bytes_dev, const uint32_t *start_dev,
                              const uint32_t *len_dev, uint64_t n, const uint8_t *status_or_null,
                              const uint8_t *mask_or_null);
/* The packed form over host or device arrays (mem covers bytes, offs and mask);
 * returns when done.  A key longer than SKE_TALLY_KEY_BYTES fails the call with
 * SKE_ETOOLONG: with SKE_MEM_HOST before anything is counted, with
 * SKE_MEM_DEVICE after the batch was (the long keys as dropped). */
int ske_tally_add(ske_ctx *ctx, uint32_t tid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                  const uint8_t *mask_or_null, int mem);
/* events_out[i], valid_out[i] = the counters of key i; 0, 0 for an absent (or too long) key */
int ske_tally_query(ske_ctx *ctx, uint32_t tid, const uint8_t *bytes, const uint32_t *offs, uint64_t n,
                    uint64_t *events_out, uint64_t *valid_out, int mem);
/* Every entry with events >= min_events (0: all), sorted by events descending,
 * then key bytes ascending, a shorter key first when it is a prefix of the other
 * (host arrays: out_keys cap x SKE_TALLY_KEY_BYTES bytes, zero padded; the
 * others cap entries).  *n_out = how many pass; more than cap: SKE_ETALLYSPACE
 * and nothing is written (cap >= used always suffices).  *complete = 0 once an
 * item was refused. */
int ske_tally_list(ske_ctx *ctx, uint32_t tid, uint64_t min_events, uint8_t *out_keys, uint32_t *out_lens,
                   uint64_t *out_events, uint64_t *out_valid, uint64_t cap, uint64_t *n_out, int *complete);
/* The first k and the last k entries of that order, by events (by == 0) or with
 * valid in the place of events (by == 1); 1 <= k <= SKE_TALLY_MAX_TOP, host
 * arrays of k entries each.  *n_out = entries written to each end: min(k, keys
 * held).  The tail comes in list order (its last entry is the listing's last),
 * as .tail(k) prints it. */
int ske_tally_top(ske_ctx *ctx, uint32_t tid, uint32_t k, int by, uint8_t *head_keys, uint32_t *head_lens,
                  uint64_t *head_events, uint64_t *head_valid, uint8_t *tail_keys, uint32_t *tail_lens,
                  uint64_t *tail_events, uint64_t *tail_valid, uint64_t *n_out, int *complete);
/* Host arrays in the listing's layout: insert-or-ADD of n entries (a restore
 * into an empty tally; the sum of several ranks' listings).  taken grows by the
 * events.  A length over SKE_TALLY_KEY_BYTES: SKE_ETOOLONG; valid[i] >
 * events[i] or non-zero padding: SKE_EINVAL; nothing is added then. */
int ske_tally_import(ske_ctx *ctx, uint32_t tid, const uint8_t *keys, const uint32_t *lens, const uint64_t *events,
                     const uint64_t *valid, uint64_t n);
/* The sum of tallies across contexts.  Export: every entry, unordered, in the
 * listing's layout, into caller-owned device arrays (keys_dev 8-byte aligned,
 * cap x SKE_TALLY_KEY_BYTES zero-padded bytes; the others cap entries).
 * *n_out = the entries; more than cap: SKE_ETALLYSPACE, *n_out still written.
 * Returns when done; SKE_EBUSY while a capture is recording.
 * Merge: insert-or-add of n such entries, and the head receives the source's
 * refused counts: taken grows by the events and by dropped_events,
 * dropped_events / dropped_valid by theirs, foreign_overflow != 0 sets the
 * overflow word.  So sum of events + dropped_events == taken still holds after
 * the merge, and the same for valid.  Precondition: valid[i] <= events[i] --
 * the arrays are another tally's export, not outside input, and are not
 * checked.  A length over SKE_TALLY_KEY_BYTES goes the too-long way: dropped,
 * overflow set.  A refusal at this tally's load limit or probe bound moves the
 * entry's counts to dropped_*.  n < 2^32 - 1.  Enqueue only. */
int ske_tally_export_dev(ske_ctx *ctx, uint32_t tid, uint8_t *keys_dev, uint32_t *lens_dev, uint64_t *events_dev,
                         uint64_t *valid_dev, uint64_t cap, uint64_t *n_out);
int ske_tally_merge_dev(ske_ctx *ctx, uint32_t tid, const uint8_t *keys_dev, const uint32_t *lens_dev,
                        const uint64_t *events_dev, const uint64_t *valid_dev, uint64_t n, uint64_t dropped_events,
                        uint64_t dropped_valid, uint32_t foreign_overflow);

/* ---- seen-row sets: count each row once under redelivery ----
 * An exact, insert-only set of 128-bit row keys on the device whose add
 * answers, per item, first sighting or repeat.  The counters (Count-Min, time
 * profile, tallies) add 1 per item, so a redelivered batch counts twice; the
 * reference's analytics do not, they read Cassandra rows keyed (lecture_id,
 * timestamp, student_id), where a redelivered row overwrites itself
 * (attendance_processor.py:64-72, :134-136).  The answer bytes of an add are
 * usable as a status column: 0 means count it.
 *
 * Keys.  A key is two u64 words, item i at keys[2i], keys[2i + 1]; keys_dev is
 * 16-byte aligned and holds 2n words.  A fold with begin != 0 starts every key
 * at two fixed seeds, else at the words that are there; folding a column
 * replaces each word k by MurmurHash64A(the item's column bytes, seed = k).  A
 * row is whatever the caller folds, in that order; the attendance row is the
 * lecture bytes, the id bytes, then the 8 little-endian bytes of int64
 * floor(epoch / granularity) (granularity >= 1; the floor also for a negative
 * epoch; 1: the row of the reference, 86400: one per UTC day).  The set reads a
 * word 0 as 1 (0 marks an empty slot).  Two rows are the same when their keys
 * are: an accidental match needs a 128-bit collision.
 *   packed: column item i = bytes[offs[i] .. offs[i + 1]) (bytes readable to the
 *     next 8-byte boundary behind the last item);
 *   fixed: the `width` bytes at bytes + i * width (width 0: the empty string);
 *   spans: bytes[start[j] .. start[j] + len[j]) with j = at[i], or i when at is
 *     NULL -- a column of ske_ingest_parse read in place.  Only the aligned
 *     8-byte words that hold a byte of the item are read.
 * All four are enqueue only and graph-capturable; n < 2^32 - 1.
 *
 * The set.  2^capacity_log2 slots of 24 bytes, addressed by a caller-chosen
 * sid < SKE_MAX_SEEN; the context owns it.  Linear probing from the low bits of
 * the first word; a walk looks at SKE_SEEN_MAX_PROBES slots, and new keys find
 * no slot once capacity / SKE_SEEN_LOAD_DEN are used (`limit`; the adds in flight
 * at that moment may pass it, the capacity never).  An item that finds no slot is
 * answered SKE_SEEN_FIRST and counted in `unplaced`: the set fails open, a count
 * is never lost and a SKE_SEEN_REPEAT is never false.  While unplaced is 0 the
 * answers are exact and identical from run to run.  Nothing is removed one by
 * one; ske_seen_reset empties the set. */
typedef struct {
    uint64_t capacity;   /* slots */
    uint64_t limit;      /* keys it takes: capacity / SKE_SEEN_LOAD_DEN */
    uint64_t used;       /* keys held */
    uint64_t calls;      /* adds run so far (those with n > 0; replays of a recorded add included) */
    uint64_t looked_at;  /* items the masks let through */
    uint64_t first;      /* of those, answered SKE_SEEN_FIRST (the unplaced ones included) */
    uint64_t unplaced;   /* of those, the ones that found no slot */
} ske_seen_info_t;
/* empty; SKE_ESEENEXISTS when sid is in use, SKE_ESEENCAP for a capacity out of range */
int ske_seen_init(ske_ctx *ctx, uint32_t sid, uint32_t capacity_log2);
/* SKE_EBUSY while a recorded graph is alive or being recorded */
int ske_seen_free(ske_ctx *ctx, uint32_t sid);
/* an empty set again, its counts and its call counter zeroed */
int ske_seen_reset(ske_ctx *ctx, uint32_t sid);
int ske_seen_info(ske_ctx *ctx, uint32_t sid, ske_seen_info_t *out);
int ske_seen_fold_packed_async(ske_ctx *ctx, uint64_t *keys_dev, const uint8_t *bytes_dev, const uint32_t *offs_dev,
                               uint64_t n, int begin);
int ske_seen_fold_fixed_async(ske_ctx *ctx, uint64_t *keys_dev, const uint8_t *bytes_dev, uint32_t width, uint64_t n,
                              int begin);
int ske_seen_fold_spans_async(ske_ctx *ctx, uint64_t *keys_dev, const uint8_t *bytes_dev, const uint32_t *start_dev,
                              const uint32_t *len_dev, const uint32_t *at_or_null, uint64_t n, int begin);
int ske_seen_fold_epoch_async(ske_ctx *ctx, uint64_t *keys_dev, const int64_t *epoch_dev, int64_t granularity,
                              uint64_t n, int begin);
/* One batch of keys on the device, enqueue only and graph-capturable; n < 2^32 - 1.
 * out_dev[i] =
 *   SKE_SEEN_SKIPPED  mask_or_null is given and mask[i] != want: the key is not inserted;
 *   SKE_SEEN_FIRST    the key was not in the set before this call and i is the
 *                     lowest index among this call's items with that key;
 *   SKE_SEEN_REPEAT   otherwise.
 * After the call every key that was let through is in the set (unless it found
 * no slot).  Each call takes the next number of the set's 32-bit call counter,
 * which lives on the device, so a recorded add sees a new call at every replay;
 * SKE_ESEENCALLS once the numbers run out.  The per-item state between the
 * call's kernels is context scratch: record the call after one direct call of at
 * least its size. */
int ske_seen_add_async(ske_ctx *ctx, uint32_t sid, const uint64_t *keys_dev, uint64_t n, const uint8_t *mask_or_null,
                       int want, uint8_t *out_dev);
/* present_out[i] = 1 when key i is in the set, else 0; nothing is inserted.  Enqueue only, capturable. */
int ske_seen_test_async(ske_ctx *ctx, uint32_t sid, const uint64_t *keys_dev, uint64_t n, uint8_t *present_out);
/* The same over host or device arrays (mem covers keys, mask and the output); return when done. */
int ske_seen_add(ske_ctx *ctx, uint32_t sid, const uint64_t *keys, uint64_t n, const uint8_t *mask_or_null, int want,
                 uint8_t *out, int mem);
int ske_seen_test(ske_ctx *ctx, uint32_t sid, const uint64_t *keys, uint64_t n, uint8_t *present_out, int mem);

/* ---- row logs: the attendance rows themselves, in arrival order ----
 * The counterpart of the reference's Cassandra table (attendance_processor.py:
 * 64-72 the schema, :134-136 the insert, :154-165 the per-lecture read;
 * attendance_analysis.py:19-52 the whole-table read): a device-resident,
 * append-only log of (lecture, timestamp, student_id, is_valid) in four columns
 * of 2^capacity_log2 entries, SKE_ROWS_ROW_BYTES a row, addressed by a
 * caller-chosen rid < SKE_MAX_ROWS; the context owns it.
 *   lec    u64  the lecture's digest: MurmurHash64A of the lecture bytes (any
 *               length), the Bloom seed, 0 mapped to 1 -- a tally's identity rule,
 *               so a tally listing names the log's partitions.  Two lectures with
 *               equal digests are one partition (the tally's limit).
 *   epoch  i64  seconds since 1970-01-01T00:00:00 UTC
 *   id     i64  the student id as an integer (the table's `student_id int`)
 *   valid  u8   is_valid, 0 or 1
 * A row's position is its arrival sequence number; nothing else orders rows.
 *
 * Append.  Row i is taken when status_or_null is NULL or status[i] == 0 and
 * mask_or_null is NULL or mask[i] == 1.  Its id must be an integer:
 *   packed, spans: canonical decimal text -- "-"? then digits, no leading zero
 *     except "0" itself, no "-0", no "+", no blanks, fitting int64.  Anything
 *     else is not a Cassandra int: the row is refused and counted (refused_ids),
 *     there is no error path.
 *   fixed: `width` bytes at ids + i * width; 8 a little-endian int64, 4 a
 *     little-endian int32, sign-extended; other widths SKE_EINVAL.
 * The taken rows with an integer id land at used + (their rank among such rows
 * of the batch): a stable compaction, so the log's contents and layout are the
 * same from run to run and position order is arrival order within and across
 * calls.  Rows that do not fit are dropped from the batch's tail (the prefix
 * that fits is kept, in order), counted in `dropped`, and set the sticky
 * `overflow`.  Always used + refused_ids + dropped == taken.  valid_dev_or_null
 * NULL stores 0 (as a missing Bloom key answers).  The head lives in the log
 * and is advanced by the call's own last kernel, so a recorded append appends
 * again at every replay.  Enqueue only and graph-capturable; n < 2^32 - 1.  The
 * per-item state between the call's kernels is context scratch: record the
 * call after one direct call of at least its size.
 *   packed: lecture i = lec_bytes[lec_offs[i] .. lec_offs[i + 1]), id likewise;
 *   spans: lecture i = bytes[lec_start[i] .. lec_start[i] + lec_len[i]), id
 *     likewise -- the columns of ske_ingest_parse read in place, with its status;
 *     only the aligned 8-byte words that hold a byte of an item are read, and no
 *     span of a row that is not taken is looked at;
 *   fixed: lectures packed, ids fixed width.
 *
 * Select.  The rows of one lecture (lec_bytes_or_null NULL: of every lecture)
 * with since <= epoch < until (INT64_MIN / INT64_MAX leave that end open), in
 * the table's order: (epoch, id) ascending, both signed, and with no lecture
 * given the digest, compared unsigned, in front (Cassandra orders partitions
 * by token, which is arbitrary; digest order is the counterpart).  Each run of
 * equal (lec, epoch, id) collapses to its last-appended row -- the table's
 * upsert: a redelivered row overwrites itself, is_valid included.  *n_out = the
 * rows after the collapse, *complete = 0 once the log's overflow is set; both
 * are always written.  More than cap: SKE_EROWSSPACE with no output array
 * touched, so cap = 0 (every output pointer may be NULL then) is the count; it
 * succeeds when *n_out is 0.  mem says where the four output arrays are.
 * Waits for the stream: SKE_EBUSY while a capture records. */
typedef struct {
    uint64_t capacity;     /* rows it holds */
    uint64_t used;         /* rows held: the next row's position */
    uint64_t taken;        /* rows the statuses and masks let through */
    uint64_t refused_ids;  /* of those, the ones whose id is not an integer */
    uint64_t dropped;      /* of those, the ones that found the log full */
    uint64_t overflow;     /* sticky: a row was dropped */
} ske_rows_info_t;
/* empty; SKE_EROWSEXISTS when rid is in use, SKE_EROWSCAP for a capacity out of range */
int ske_rows_init(ske_ctx *ctx, uint32_t rid, uint32_t capacity_log2);
/* SKE_EBUSY while a recorded graph is alive or being recorded */
int ske_rows_free(ske_ctx *ctx, uint32_t rid);
/* an empty log again, its counts zeroed */
int ske_rows_reset(ske_ctx *ctx, uint32_t rid);
int ske_rows_info(ske_ctx *ctx, uint32_t rid, ske_rows_info_t *out);
int ske_rows_append_packed_async(ske_ctx *ctx, uint32_t rid, const uint8_t *lec_bytes_dev,
                                 const uint32_t *lec_offs_dev, const uint8_t *id_bytes_dev,
                                 const uint32_t *id_offs_dev, const int64_t *epoch_dev,
                                 const uint8_t *valid_dev_or_null, const uint8_t *mask_or_null, uint64_t n);
int ske_rows_append_spans_async(ske_ctx *ctx, uint32_t rid, const uint8_t *bytes_dev, const uint32_t *lec_start_dev,
                                const uint32_t *lec_len_dev, const uint32_t *id_start_dev,
                                const uint32_t *id_len_dev, const uint8_t *status_or_null, const int64_t *epoch_dev,
                                const uint8_t *valid_dev_or_null, const uint8_t *mask_or_null, uint64_t n);
int ske_rows_append_fixed_async(ske_ctx *ctx, uint32_t rid, const uint8_t *lec_bytes_dev,
                                const uint32_t *lec_offs_dev, const uint8_t *ids_dev, uint32_t width,
                                const int64_t *epoch_dev, const uint8_t *valid_dev_or_null,
                                const uint8_t *mask_or_null, uint64_t n);
/* The packed form over host or device arrays (mem covers every input); returns
 * when done.  Appending what ske_rows_read returned, ids as text, restores a log. */
int ske_rows_append(ske_ctx *ctx, uint32_t rid, const uint8_t *lec_bytes, const uint32_t *lec_offs,
                    const uint8_t *id_bytes, const uint32_t *id_offs, const int64_t *epoch,
                    const uint8_t *valid_or_null, const uint8_t *mask_or_null, uint64_t n, int mem);
int ske_rows_select(ske_ctx *ctx, uint32_t rid, const uint8_t *lec_bytes_or_null, uint32_t lec_len, int64_t since,
                    int64_t until, uint64_t *out_lec, int64_t *out_epoch, int64_t *out_id, uint8_t *out_valid,
                    uint64_t cap, uint64_t *n_out, int *complete, int mem);
/* The raw columns of positions [first, first + n) to host arrays (a checkpoint);
 * SKE_EINVAL when first + n passes `used`. */
int ske_rows_read(ske_ctx *ctx, uint32_t rid, uint64_t first, uint64_t n, uint64_t *out_lec, int64_t *out_epoch,
                  int64_t *out_id, uint8_t *out_valid);

/* Group-by.  The reference's analysis is five groupby(...).size() calls over
 * the de-duplicated table (attendance_analysis.py:65-118); these two calls give
 * them exactly, and only the groups leave the device.  The lecture and the
 * [since, until) window are ske_rows_select's and the upsert collapse runs
 * first: the validity filter, the sod_from filter and the count look at each
 * run's surviving (last-appended) row only.  A survivor is counted when it
 * passes valid_filter (SKE_ROWS_VALID_*) and its floored UTC second of the day
 * is at least sod_from (0: no filter; above 86399: SKE_EINVAL).
 *
 * ske_rows_group: out_key[g], out_count[g] = the groups that have at least one
 * counted row, ascending by key (pandas' group order; a group whose rows are all
 * filtered out does not appear, as in df[mask].groupby().size()).  by =
 * SKE_ROWS_BY_LECTURE: the key is the digest, compared unsigned; by =
 * SKE_ROWS_BY_STUDENT: the id's two's-complement bits, the order signed.
 * *n_out (= stats->n), *stats and *complete are always written.  More groups
 * than cap: SKE_EROWSSPACE with no output array touched, so cap = 0 (both arrays
 * may be NULL then) is the statistics alone; it succeeds when no group is
 * listed.  mem says where the two output arrays are.  An unknown by or
 * valid_filter is SKE_EINVAL.  Integer arithmetic throughout: the answer is the
 * same from run to run.
 *
 * ske_rows_profile: out_bins[weekday * 24 + hour] (SKE_TP_BINS host words,
 * Monday first, UTC, the time profile's layout) = the counted rows by their
 * epoch's bin; *rows_out = the rows after the collapse.
 *
 * Both wait for the stream: SKE_EBUSY while a capture records. */
typedef struct {
    uint64_t rows;      /* rows in the window after the upsert collapse (what ske_rows_select would return) */
    uint64_t n;         /* groups with at least one counted row */
    uint64_t sum;       /* counted rows = sum of the counts */
    uint64_t sumsq;     /* sum of count^2 (sum <= 2^28, so it fits) */
    uint64_t min, max;  /* of the counts; 0, 0 when n == 0 */
    uint64_t med_lo, med_hi; /* counts of 0-based rank (n-1)/2 and n/2 in ascending order; 0, 0 when n == 0 */
} ske_rows_group_stats_t;
int ske_rows_group(ske_ctx *ctx, uint32_t rid, int by, const uint8_t *lec_bytes_or_null, uint32_t lec_len,
                   int64_t since, int64_t until, int valid_filter, uint32_t sod_from, uint64_t *out_key,
                   uint64_t *out_count, uint64_t cap, uint64_t *n_out, ske_rows_group_stats_t *stats, int *complete,
                   int mem);
int ske_rows_profile(ske_ctx *ctx, uint32_t rid, const uint8_t *lec_bytes_or_null, uint32_t lec_len, int64_t since,
                     int64_t until, int valid_filter, uint32_t sod_from, uint64_t *out_bins, uint64_t *rows_out,
                     int *complete);
/* Group merge: many (key, count) lists summed into one -- what joins the
 * ske_rows_group outputs of several contexts (ranks that each hold the rows of
 * the lectures they own) into the group-by of all their rows.  It needs no log:
 * it works on caller arrays and context scratch.
 *   keys[i], counts[i], i < n_in: entries in any order, the same key any number
 * of times (the intended input is several ske_rows_group outputs end to end,
 * but no order is required); mem says where these two arrays and the two
 * output arrays are.  The inputs are not modified; inputs and outputs must not
 * overlap.
 *   The merged count of a key is the sum of its entries' counts; a key is
 * listed when that sum is nonzero, so zero-count entries are padding that
 * vanishes.  out_key[g], out_count[g] = the listed keys ascending -- by =
 * SKE_ROWS_BY_LECTURE unsigned, SKE_ROWS_BY_STUDENT signed, ske_rows_group's
 * order -- and their sums.  *stats is over the listed sums, each field as
 * ske_rows_group defines it, except stats->rows, which is written 0 (the caller
 * sums the parts' rows).  *multi_out = the listed keys that received more than
 * one entry with a nonzero count.  *n_out (= stats->n), *stats and *multi_out
 * are always written.
 *   Capacity: ske_rows_group's protocol.  More listed keys than cap:
 * SKE_EROWSSPACE with no output array touched; cap = 0 (both arrays may be NULL
 * then) is the statistics alone and succeeds when nothing is listed.
 *   n_in == 0: SKE_OK with everything zero.  SKE_EINVAL: an unknown by; a NULL
 * n_out, stats or multi_out; NULL inputs with n_in > 0; n_in > 2^28; a total of
 * the counts above 2^32 - 1 (which keeps every prefix in 32 bits and sumsq in
 * 64, as "sum <= 2^28" does for ske_rows_group) -- the total is found on the
 * device and looked at before any output is written.  Waits for the stream:
 * SKE_EBUSY while a capture records.
 *   Integer arithmetic throughout: the answer is the same from run to run and
 * does not depend on the order of the entries.
 *   Identity: merging the output of one ske_rows_group call alone returns it
 * unchanged -- the keys, the counts and every statistic except rows -- with
 * *multi_out == 0.
 *   Additivity: when every (lecture, epoch, id) lies in one part only -- rows
 * sharded by lecture -- the merge of the parts' ske_rows_group outputs is the
 * ske_rows_group of all the rows in one log, for either by and every filter. */
int ske_rows_group_merge(ske_ctx *ctx, int by, const uint64_t *keys, const uint64_t *counts, uint64_t n_in,
                         uint64_t *out_key, uint64_t *out_count, uint64_t cap, uint64_t *n_out,
                         ske_rows_group_stats_t *stats, uint64_t *multi_out, int mem);

/* Compaction: the table's overwrite and its TTL, on the device.  A row survives
 * when epoch >= keep_since (INT64_MIN expires nothing) and it is the
 * last-appended row of its run of equal (lec, epoch, id) -- ske_rows_select's
 * survivor rule.  A row below keep_since counts as expired whether or not it
 * was also superseded.  The survivors keep their relative arrival order and
 * occupy positions 0 .. kept - 1, so position order is still arrival order and
 * a later append still wins over them; the compacted log depends on the log's
 * contents and keep_since alone and is the same from run to run.
 *   Head: used = kept; taken decreases by the rows removed, so used +
 * refused_ids + dropped == taken holds on; refused_ids, dropped and the sticky
 * overflow are untouched (dropped rows stay lost: a select's *complete stays 0
 * until ske_rows_reset).
 *   For every lecture, every window with since >= keep_since, every
 * valid_filter and sod_from, ske_rows_select, ske_rows_group and
 * ske_rows_profile answer after the call what they answered before it.
 *   An empty log, or one with nothing to remove, returns kept == before and
 * moves nothing.  A recorded append stays valid and appends at the new `used`
 * when replayed (the head lives in the log).  Waits for the stream: SKE_EBUSY
 * while a capture records; SKE_EINVAL for a NULL out. */
typedef struct {
    uint64_t before;      /* used when the call began */
    uint64_t kept;        /* used when it returned */
    uint64_t superseded;  /* removed: a later-appended row has the same (lec, epoch, id) */
    uint64_t expired;     /* removed: epoch < keep_since */
} ske_rows_compact_t;     /* before == kept + superseded + expired */
int ske_rows_compact(ske_ctx *ctx, uint32_t rid, int64_t keep_since, ske_rows_compact_t *out);

/* ---- the fused hot path (K1) ----
 * For every swipe i: v = BF.EXISTS fid id_i; if v: PFADD slot_i id_i.
 *   replaces the per-event pair attendance_processor.py:109-113 + :127-129.
 * out_valid (may be NULL) receives v per swipe. */
int ske_swipes(ske_ctx *ctx, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
               const uint32_t *offs, uint64_t n, uint8_t *out_valid, int mem);
/* device-pointer form that only enqueues (no sync); for the benchmark */
int ske_swipes_async(ske_ctx *ctx, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                     const uint32_t *offs, uint64_t n, uint8_t *out_valid);
/* fixed-width form: id i is the `width` bytes at bytes + i*width (no offset
 * array -- e.g. fixed-digit student ids, which every config uses).  Same
 * semantics as ske_swipes; the id load needs no offset load first. */
int ske_swipes_fixed(ske_ctx *ctx, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                     uint32_t width, uint64_t n, uint8_t *out_valid, int mem);
int ske_swipes_fixed_async(ske_ctx *ctx, uint32_t fid, const uint32_t *slot,
                           const uint8_t *bytes, uint32_t width, uint64_t n, uint8_t *out_valid);
/* Fixed-width swipes with the answers packed 1 bit per swipe (bit i & 7 of
 * out_bits[i >> 3], LSB first -- numpy packbits(bitorder="little")).  Same
 * BF.EXISTS / PFADD semantics as ske_swipes.  With host memory the batch is
 * pipelined in chunks: a chunk's ids and slots cross the host link while K1
 * runs on the previous one; the link carries width + 4 bytes per swipe in and
 * 1/8 byte out (the offsets-and-bytes form: width + 9).  Synchronous; reports
 * the out-of-range slots flagged while it ran (SKE_ERANGE; see ske_sync).
 *   replaces the per-event pair attendance_processor.py:109-113 + :127-129
 *   for a batch of fixed-digit student ids (every config's ids) */
int ske_swipes_fixed_bits(ske_ctx *ctx, uint32_t fid, const uint32_t *slot, const uint8_t *bytes,
                          uint32_t width, uint64_t n, uint8_t *out_bits, int mem);
/* Swipes that arrive NOT partitioned by key owner (one
 * alltoallv per batch; distributed.SwipeExchange; no reference counterpart --
 * the reference's Shared subscription hands any event to any consumer,
 * attendance_processor.py:30-34).  Device pointers.  Swipe i (fixed-width id,
 * GLOBAL key index g into the job's key universe) goes to rank key_owner[g]
 * as local slot key_local[g] -- the key map every multi-GPU path shares
 * (distributed.KeyMap: owner = MurmurHash64A(key name, 0) mod world).  An
 * index g >= nkeys goes to rank 0 with local slot 0xffffffff (K1 answers it
 * and reports SKE_ERANGE for its PFADD).  send_ids / send_slots are filled
 * owner by owner (the alltoallv input), pos[i] = the swipe's position there,
 * counts[o] (host) = swipes for owner o (the split sizes; the call
 * synchronizes the context stream for them).  world <= 64, n < 2^32. */
int ske_route_swipes(ske_ctx *ctx, const uint8_t *ids, uint32_t width, const uint32_t *gkey, uint64_t n,
                     uint32_t world, const uint32_t *key_owner, const uint32_t *key_local, uint32_t nkeys,
                     uint8_t *send_ids, uint32_t *send_slots, uint32_t *pos, uint64_t *counts);
/* The same routing with no host synchronisation (enqueue only), through one
 * packed route word per key: key_route[g] = owner << 26 | local slot (local
 * slot < 2^26), or 0xffffffff for a key no rank owns (rank 0, slot
 * 0xffffffff, as above) -- one gather per swipe instead of two.  Owner o's
 * swipes fill rows [o*cap, o*cap + counts[o]) of send_ids / send_slots (device,
 * world*cap rows), so every peer pair exchanges exactly `cap` rows (an
 * all_to_all of equal splits the host sizes without reading the device).
 * Rows [counts[o], cap) get zero id bytes and slot sink_slots[o] (device,
 * [world]: a slot owner o keeps for no key, so padding changes no key's
 * registers).  counts (device, [world]) = swipes per owner; counts[o] > cap
 * means the swipes ranked past cap were NOT sent (their answers are another
 * row's): the caller re-runs the batch with ske_route_swipes, which is safe
 * (PFADD is idempotent, answers are rewritten).  world*cap < 2^32.
 * Replaces the per-event consumer loop's hand-off, attendance_processor.py:30-34. */
int ske_route_swipes_cap_async(ske_ctx *ctx, const uint8_t *ids, uint32_t width, const uint32_t *gkey, uint64_t n,
                               uint32_t world, const uint32_t *key_route, uint32_t nkeys, uint32_t cap,
                               const uint32_t *sink_slots, uint8_t *send_ids, uint32_t *send_slots, uint32_t *pos,
                               uint32_t *counts);
/* The routing of a one-rank world, where the exchange is the identity (K1
 * reads the batch in place, answers come in input order): out_slots[i] = the
 * local slot of global key gkey[i] from key_route (as above), or 0xffffffff
 * for a key past the table or owned by no rank < world (K1 reports it as
 * SKE_ERANGE).  key_route NULL (world 1 only): the identity table of a
 * one-rank key map, slot = gkey for gkey < nkeys (< 2^26).  Device arrays,
 * enqueue only. */
int ske_route_slots_async(ske_ctx *ctx, const uint32_t *gkey, uint64_t n, const uint32_t *key_route, uint32_t nkeys,
                          uint32_t world, uint32_t *out_slots);
/* out[i] = answers[pos[i]]: the owners' BF.EXISTS answers, received back in
 * send order, into input order (enqueue only). */
int ske_route_return_async(ske_ctx *ctx, const uint8_t *answers, const uint32_t *pos, uint64_t n,
                           uint8_t *out);
/* Several device-resident batches in one call (enqueue only, graph-capturable):
 * batch j runs on branch j mod `branches` (0: SKE_MANY_DEFAULT_BRANCHES), each
 * branch a side stream forked from and joined back into the context stream.
 * With more than one branch the short-id K1 runs on one block per two CUs
 * (unless the "k1_grid" option is set), so two batches share the chip.  A
 * batch with width > 0 is fixed-width (offs unused), else bytes + offsets.
 * Same answers and registers as calling ske_swipes_async per batch in order
 * (the register update is a commutative max).  nbatch == 0 only creates the
 * branches' side streams (do that once before recording the call into a
 * graph).  No reference counterpart: the
 * reference's processor handles one Pulsar message per loop iteration
 * (attendance_processor.py:100-137); this is its batched-throughput form. */
#define SKE_MANY_MAX_BRANCHES 32
#define SKE_MANY_DEFAULT_BRANCHES 16
typedef struct ske_swipe_batch {
    const uint32_t *slot;
    const uint8_t *bytes;
    const uint32_t *offs;
    uint32_t width;
    uint64_t n;
    uint8_t *out_valid;
} ske_swipe_batch;
int ske_swipes_many_async(ske_ctx *ctx, uint32_t fid, const ske_swipe_batch *batches,
                          uint32_t nbatch, uint32_t branches);
/* probe statistics of the same swipes (untimed): Bloom bit tests performed
 * and valid count, to price the algorithmic bytes of the roofline. */
int ske_swipes_stats(ske_ctx *ctx, uint32_t fid, const uint8_t *bytes, const uint32_t *offs,
                     uint64_t n, uint64_t *probes, uint64_t *nvalid);
/* which K1 variant the current chain and options select:
 *   0 = generic LDS / global-memory K1 (sketch_kernels.hip),
 *   1 = short-id LDS K1, the chain staged in LDS (sketch_k1.hip; C1/C2/C4),
 *   2 = XCD-partitioned K1 (sketch_xr.hip),
 *   3 = partitioned K1, passes A/B/C over LDS slices (sketch_part.hip; C3/C5) */
int ske_swipes_variant(ske_ctx *ctx, uint32_t fid);
/* Tuning options (no reference counterpart): "variant" (-1 auto, 0..3 as
 * above), "tile" (LDS K1 swipes per thread: 1, 2, 4, 8), "k1_grid" (LDS K1
 * blocks, 0 = one per CU), "k1_persistent" (0/1), "part_sub" (partitioned K1
 * swipes per sub-batch, at most 2^26; 0 = 2^25), "pass_timing" (0/1); the
 * partitioned K1's
 * segmented PFADD: "hll_seg" (-1 auto, 0 never, 1 whenever the
 * chain and slab allow), "seg_density" (auto: swipes per 128-B slab line at
 * which a batch is segmented, x100, default 600, doubled for a slab of at
 * most 192 MB), "seg_dense_min" (records per window line at which a window
 * is staged in LDS, x100), "seg_klog" (0..3: keys per window 1, 2, 4, 8;
 * default 1), "seg_b1" (-1 auto, 0..9: 2^b1 level-1 buckets), "seg_floor"
 * (1, the default: records that cannot raise a register, because their rank
 * is at or under the minimum of their key's registers, are dropped before the
 * window pass; 0: never), "seg_hot_min" (arrivals per key and window pass from
 * which a window's minimum is derived, default 4096, up to 2^31).  Any other
 * name or an out-of-range value: SKE_EINVAL.  None changes an answer or a
 * register. */
int ske_set_option(ske_ctx *ctx, const char *name, int64_t value);
/* Kernel timing for the benchmark's roofline: with option "pass_timing" = 1
 * every K1 kernel launched outside a capture is bracketed by a HIP event pair
 * recorded on the stream it runs on.  ske_pass_times waits for them and
 * returns, per pass kind, the summed milliseconds and the kernel count:
 * [0] single-kernel K1 (LDS / global / XCD-partitioned variants), [1] [2] [3]
 * the partitioned K1's passes A (hash + probe records), B (slice probes),
 * C (answers + register max, or the segmented PFADD's answers + level-1
 * records), [4] the segmented PFADD's level-2 sort, [5] its window apply;
 * and the stages of a host-fed call (ske_swipes / ske_swipes_fixed_bits with
 * SKE_MEM_HOST): [6] its host -> device copies (per chunk, on the copy
 * stream), [7] its device -> host copies of the answers, [8] the whole call
 * (from its first enqueued operation to the end of its last).
 * reset != 0 zeroes the sums after reading. */
#define SKE_PASS_KINDS 9
int ske_pass_times(ske_ctx *ctx, double *ms_out, uint64_t *count_out, int reset);
/* The segmented PFADD's floor statistics since the last read (waits for the
 * context's stream): out[0] key windows whose register minimum was derived,
 * out[1] level-1 records the level-2 sort saw, out[2] those it dropped as
 * unable to raise a register.  All zero with "seg_floor" 0. */
int ske_seg_floor_stats(ske_ctx *ctx, uint64_t out[3]);

/* ---- ingest: JSON event decode + key-slot resolution ----
 * The reference decodes each Pulsar payload on the CPU (attendance_processor.py
 * :103-106) and builds the HLL key from lecture_id (:128; README.md:105-106
 * adds the UTC day).  ske_ingest_parse decodes a batch of messages on the
 * device: for each message, status 0 = decoded (the fast JSON / ISO-8601 path,
 * see sketch_ingest.hip), 1 = left for the host (Python semantics), and for a
 * decoded one the spans of student_id / lecture_id / timestamp inside msgs,
 * the UTC day number and a 128-bit key hash.  The context's key table maps
 * key hashes to HLL slots; the host inserts a key the first time it misses.
 * All column pointers are device pointers owned by the caller (n entries,
 * kh 2n); msgs must stay readable to the next 8-byte boundary. */
typedef struct {
    uint8_t *status;
    uint32_t *id_start, *id_len, *lec_start, *lec_len, *ts_start, *ts_len;
    int32_t *day;
    uint64_t *kh;
} ske_ingest_cols_t;
int ske_ingest_parse(ske_ctx *ctx, const uint8_t *msgs, const uint32_t *moffs, uint64_t n,
                     int day_form, const ske_ingest_cols_t *cols);
/* slot_dev[i] = the slot of message i's key, 0xffffffff when not in the table
 * (or not decoded); *nmiss = decoded messages whose key missed */
int ske_keytab_lookup(ske_ctx *ctx, const ske_ingest_cols_t *cols, uint64_t n, uint32_t *slot_dev,
                      uint64_t *nmiss);
int ske_keytab_insert(ske_ctx *ctx, const uint64_t *kh_host, const uint32_t *slots_host, uint64_t n);
int ske_keytab_clear(ske_ctx *ctx);
/* the fused path (K1) over the decoded messages whose key is in the table:
 * valid_dev[i] = BF.EXISTS of message i's id (0 for the others); PFADD of the
 * valid ones.  *ntaken = messages that went through K1. */
int ske_ingest_swipes(ske_ctx *ctx, uint32_t fid, const uint8_t *msgs,
                      const ske_ingest_cols_t *cols, uint64_t n, uint8_t *valid_dev,
                      uint64_t *ntaken);

/* The decoded messages' times: epoch_dev[i] (8-byte aligned, n entries) = the
 * timestamp span of message i as seconds since 1970-01-01T00:00:00 UTC when
 * status[i] == 0, else 0 -- analysis.epoch_seconds(datetime.fromisoformat(text)):
 * a naive timestamp is UTC as written, an offset is subtracted, a date-only
 * form is midnight, a fraction is dropped (the floor, also before 1970).  The
 * span was validated by ske_ingest_parse and is decoded by position; at most
 * five aligned 8-byte words of it are read.  Enqueue only. */
int ske_ingest_times(ske_ctx *ctx, const uint8_t *msgs, const ske_ingest_cols_t *cols, uint64_t n,
                     int64_t *epoch_dev);
/* The decoded messages (status 0), in message order, as one packed batch on the
 * device -- the input of ske_cms_add_packed_async / ske_hh_track_packed_async /
 * ske_tp_add_async.  All pointers are device pointers owned by the caller:
 * ids cap_bytes bytes and readable to the next 8-byte boundary, offs n + 1
 * entries, epoch (8-byte aligned), valid and at n entries.  Entry r of the
 * *ndense decoded messages: its id bytes at ids[offs[r] .. offs[r + 1]), its
 * epoch (epoch_dev of its message; 0 when that is NULL), its BF.EXISTS byte
 * (valid_dev of its message; 0 when NULL) and its message index at[r].
 * *nbytes = offs[*ndense].  More than cap_bytes: SKE_EINVAL with both totals
 * set and nothing written.  Waits for the stream (it returns the totals), so
 * it cannot be recorded: SKE_EBUSY. */
typedef struct {
    uint8_t *ids;
    uint32_t *offs;
    int64_t *epoch;
    uint8_t *valid;
    uint32_t *at;
} ske_ingest_dense_t;
int ske_ingest_dense(ske_ctx *ctx, const uint8_t *msgs, const ske_ingest_cols_t *cols, uint64_t n,
                     const uint8_t *valid_dev_or_null, const int64_t *epoch_dev_or_null,
                     const ske_ingest_dense_t *out, uint64_t cap_bytes, uint64_t *ndense, uint64_t *nbytes);

/* ---- stream capture (HIP graphs) ----
 * Record the device work of the calls made between begin and end on the
 * context stream (only enqueue-only calls: ske_swipes_async,
 * ske_swipes_fixed_async, ske_cms_add_fixed_async, ske_cms_add_packed_async,
 * ske_hh_track_fixed_async, ske_hh_track_packed_async, ske_tp_add_async,
 * ske_tally_add_packed_async, ske_tally_add_fixed_async, ske_tally_add_spans_async,
 * ske_seen_fold_packed_async, ske_seen_fold_fixed_async, ske_seen_fold_spans_async,
 * ske_seen_fold_epoch_async, ske_seen_add_async, ske_seen_test_async,
 * ske_rows_append_packed_async, ske_rows_append_spans_async, ske_rows_append_fixed_async,
 * ske_ingest_times) into an executable graph, uploaded to the device;
 * each ske_graph_launch replays it on the context stream.  A consumer that
 * processes a ring of fixed device batch slots replays one graph per turn of
 * the ring instead of one launch per batch (SURVEY.md §8a-1's processor loop at
 * batch granularity).  The graph keeps the pointers it was recorded with. */
int ske_capture_begin(ske_ctx *ctx);
int ske_capture_end(ske_ctx *ctx, void **graph_out);
int ske_graph_launch(ske_ctx *ctx, void *graph);
int ske_graph_free(ske_ctx *ctx, void *graph);

/* ---- synthetic stream (device buffers) ---- */
int ske_gen_members(ske_ctx *ctx, const ske_gen_params_t *p, uint64_t start, uint64_t n,
                    uint8_t *bytes_dev, uint32_t *offs_dev);
int ske_gen_swipes(ske_ctx *ctx, const ske_gen_params_t *p, uint64_t start, uint64_t n,
                   uint8_t *bytes_dev, uint32_t *offs_dev, uint32_t *slot_dev);
int ske_gen_id_width(const ske_gen_params_t *p); /* digits per ID */

#ifdef __cplusplus
}
#endif
#endif
