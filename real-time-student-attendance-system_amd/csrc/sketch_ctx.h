// sketch_ctx.h -- the context and what the sketch_api_*.cpp units share.
//
// The C-ABI of include/sketch.h is split by subsystem:
//   sketch_api_ctx.cpp     lifecycle, options, the error word, streams, staging,
//                          pass timing, the scratch-use ordering, graphs
//   sketch_api_bloom.cpp   link geometry, chain growth, export / import,
//                          BF.MEXISTS and BF.MADD
//   sketch_api_hll.cpp     the register slab, PFADD, PFCOUNT, PFMERGE, export / import
//   sketch_api_swipes.cpp  K1: variant choice, launch_k1, ske_swipes*, ske_route_*
//   sketch_api_ingest.cpp  ingest, the key table, the generator
//   sketch_api_cms.cpp     Count-Min Sketch tables: init, add, query, merge, export / import
//   sketch_api_hh.cpp      heavy-hitter sets beside a table: init, track, list, stats, select
//   sketch_api_tp.cpp      time profiles (weekday x hour counters): init, add, read / import
//   sketch_api_tally.cpp   tallies (exact event counts per key): init, add, query, list, top, import
//   sketch_api_seen.cpp    seen-row sets (exact sets of 128-bit row keys): init, the folds, add, test
//   sketch_api_rows.cpp    row logs (the attendance rows in arrival order): init, append, select, read
// A helper used by one unit is static there; what crosses units is declared here.
// The last six keep "a device allocation owned by the context and addressed by
// an id": one struct (DevObj), one description per family (ObjFamily) and one
// set of helpers (obj_get, obj_for_sync_call, obj_alloc, obj_release,
// obj_read_head) carry the lifecycle; the units hold what is their own.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/sketch.h"
#include "sketch_common.h"
#include "sketch_internal.h"

// pass kinds of ske_pass_times: 0 a single-kernel K1 (LDS / global /
// XCD-partitioned), 1-3 the partitioned K1's passes A, B, C
constexpr int kPassKinds = SKE_PASS_KINDS;

namespace ske {

struct Link {
    uint8_t *bf = nullptr;  // device
    uint64_t entries = 0, bytes = 0, bits = 0, size = 0;
    double error = 0, bpe = 0;
    int hashes = 0;
    Divisor div{};
};

struct Filter {
    bool exists = false;
    bool dev_ok = false;  // `dev` matches `links`
    ChainDev dev{};       // cached kernel view of the chain (rebuilt on growth)
    std::vector<Link> links;
    uint64_t size = 0;
    uint32_t growth = 2;
    bool nonscaling = false;
};

// One device object addressed by an id: one allocation owned by the context
// (base == nullptr: the id is free), its size and, where the family has one,
// its capacity exponent.  The six families below are this struct, kept in one
// vector per family (ske_ctx) and handled by the obj_* helpers further down.
struct DevObj {
    uint8_t *base = nullptr;  // device
    size_t bytes = 0;
    uint32_t log2 = 0;
};

// one Count-Min Sketch table: depth rows of width counters, then the count on
// the next 16-byte boundary (the allocation's last 16 bytes)
struct Cms : DevObj {
    uint32_t width = 0, depth = 0;
    Div32 div{};
};
inline uint32_t *cms_cells(const Cms &T) { return reinterpret_cast<uint32_t *>(T.base); }
inline unsigned long long *cms_count(const Cms &T) {
    return reinterpret_cast<unsigned long long *>(T.base + T.bytes - 16);
}

// one heavy-hitter set: a 16-byte head (used, overflow), then the claim words,
// the id words, the lengths
using Hh = DevObj;

// one time profile: kTpBins u64 counters
using Tp = DevObj;

// one tally: a 64-byte head (used, overflow, taken, the dropped totals), then
// the claim words, the key words, the two counters and the lengths
using Tally = DevObj;

// one seen-row set: a 64-byte head (SeenHead), then the w0 words, the w1 words
// and the stamps
struct Seen : DevObj {
    // the call counter as the host knows it: the device's at the last ske_seen_info
    // plus the adds enqueued since (a graph's replays are not counted here; the
    // kernels stop the counter themselves)
    uint64_t calls_host = 0;
};

// one row log: a 64-byte head (RowsHead), then the lec, epoch and id words and
// the valid bytes
using Rows = DevObj;

struct Staged {
    const uint8_t *bytes = nullptr;
    const uint32_t *offs = nullptr;
};

// The last use of one ordering group of context scratch slots (ScratchSlot,
// sketch_internal.h): a use on another stream first waits for it (ScratchUser).
struct ScratchUse {
    hipEvent_t done = nullptr;
    hipStream_t stream = nullptr;
    unsigned long long cap = 0;  // capture id of stream's last scratch use (0: none)
    bool pending = false;        // that use is not yet covered by done (recorded lazily)
};

}  // namespace ske

struct ske_ctx {
    int device = 0;
    int cus = 256;
    hipStream_t own = nullptr;
    hipStream_t st = nullptr;
    std::vector<ske::Filter> filters;
    std::vector<ske::Cms> cms;  // by cid (sized on first use)
    bool cms_lds_ready = false;  // cms_setup() done (first ske_cms_init; a failure fails that call)
    // tables up to this many cells take the LDS form (the environment variable
    // SKE_CMS_LDS_CELLS, read by ske_open, lowers it for A/B timing; 0: never)
    uint32_t cms_lds_cells = ske::kCmsLdsCells;
    std::vector<ske::Hh> hh;    // by hid (sized on first use)
    bool hh_lds_ready = false;  // hh_setup() done (first ske_hh_init)
    // a track copies tables up to this many cells into LDS (SKE_HH_LDS_CELLS,
    // read by ske_open, sets it for A/B timing, at most kCmsLdsCells; 0: never)
    uint32_t hh_lds_cells = ske::kHhLdsCells;
    std::vector<ske::Tp> tp;    // by tid (sized on first use)
    // workgroups of a time-profile add (SKE_TP_GRID, read by ske_open; 0: one
    // per CU) and its form (SKE_TP_FORM: 0 a one-bin wavefront adds once, 1 per
    // lane); for small-shape tests and A/B timing, neither changes a result
    int tp_grid = 0;
    int tp_form = 0;
    std::vector<ske::Tally> tally;  // by tid (sized on first use)
    bool tally_ready = false;       // tally_setup() done (first ske_tally_init)
    // a tally add's form (SKE_TALLY_FORM, read by ske_open: 0 a hash table in
    // each workgroup's LDS first, 1 one insert-or-add in memory per item), form
    // 0's workgroups (SKE_TALLY_GRID; 0: one per CU) and the slots of its LDS
    // table (SKE_TALLY_LDS_LOG2); for small-shape tests and A/B timing, none changes a result
    int tally_form = 0;
    int tally_grid = 0;
    int tally_lds_log2 = ske::kTallyLdsMaxLog2;
    std::vector<ske::Seen> seen;  // by sid (sized on first use)
    // workgroups of the seen sets' kernels (SKE_SEEN_GRID, read by ske_open; 0:
    // eight per CU); for small-shape tests, changes no result
    int seen_grid = 0;
    std::vector<ske::Rows> rows;  // by rid (sized on first use)
    // workgroups of the row logs' kernels (SKE_ROWS_GRID, read by ske_open; 0:
    // eight per CU); for small-shape tests, changes no result
    int rows_grid = 0;
    // workgroups of ske_ingest_times / ske_ingest_dense (SKE_INGEST_GRID, read by
    // ske_open; 0: the ingest kernels' launch shape); for small-shape tests, changes no result
    int ingest_grid = 0;
    uint8_t *regs = nullptr;  // nslots * 16384
    uint32_t nslots = 0;
    double *tau = nullptr, *sig = nullptr;  // device estimator tables (lazy)
    ske::Scratch *scratch = nullptr;
    // staging buffers by use (grow on demand)
    void *stg[ske::kStageSlotCount] = {};
    size_t stg_cap[ske::kStageSlotCount] = {};
    ske::HostStager *hs = nullptr;  // pinned double buffer + copy threads for pageable inputs (lazy)
    unsigned int *err = nullptr;  // [0] sticky slot-error word; see check_call_err
    bool err_pending = false;     // taken from the device, not yet reported by ske_sync
    unsigned long long *stats = nullptr;
    int pb = 2;           // K1 tile: swipes per thread in flight (1, 2, 4, 8)
    int variant = -1;     // -1 auto, 0 global, 1 LDS, 2 XCD-partitioned, 3 partitioned
    uint32_t part_sub = 0;  // partitioned K1: swipes per sub-batch (0: default)
    ske::SegOpts seg;       // partitioned K1: the segmented PFADD's options
    bool lds_ok = false;
    bool k1_ok = false;       // short-id LDS K1 (sketch_k1.hip) usable
    int k1_grid = 0;          // blocks of the short-id LDS K1 (0: one per CU)
    int k1_persistent = 1;    // ske_swipes_many_async: one LDS K1 launch over all batches
    uint8_t *zero16 = nullptr;  // 16 zero bytes on the device
    // the XCD-partitioned and partitioned K1 and routing keep per-launch state
    // in the context scratch: a launch on another stream first waits for the
    // previous one of its group (ScratchSlot's ordering rule, sketch_internal.h)
    ske::ScratchUse xr;  // K1's slots (kScrXr, kScrPart*, kScrSeg*)
    ske::ScratchUse rt;  // routing's slots (kScrRoute*): ordered among routing calls, not behind K1
    ske::ScratchUse sn;  // the seen sets' slot (kScrSeenSlot): ordered among seen adds alone
    ske::ScratchUse rw;  // the row logs' slots (kScrRowsFlag, Idv, Cnt): ordered among appends alone
    // executable graphs alive (recorded, not yet freed): they hold pointers to
    // the scratch and the register slab, so neither may be reallocated
    int live_graphs = 0;
    bool capturing = false;
    // scratch users recorded into the graph being captured (bit 0: xr,
    // bit 1: rt, bit 2: sn, bit 3: rw), and per live graph the users its replays hold: a replay
    // records only their events, so a graph without routing does not order
    // the next routing call behind itself
    unsigned cap_users = 0;
    std::unordered_map<void *, unsigned> graph_users;
    // pass timing (option "pass_timing"): HIP event pairs around every K1
    // kernel, recorded on the stream the kernel runs on (never inside a
    // capture); ske_pass_times() sums them per pass
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;
    struct Mark { int pass; hipEvent_t a, b; bool own_a; };  // pass < 0: void (an abandoned mark)
    std::vector<Mark> marks;
    double pass_ms[kPassKinds] = {};
    uint64_t pass_n[kPassKinds] = {};
    // ske_swipes_many_async: side streams of the fork/join branches (lazy)
    hipStream_t many_st[SKE_MANY_MAX_BRANCHES - 1] = {};
    hipEvent_t many_join[SKE_MANY_MAX_BRANCHES - 1] = {};
    hipEvent_t many_fork = nullptr;
    int many_n = 0;
    // host-fed chunk pipeline (ske_swipes_fixed_bits): a copy stream and one
    // event per chunk in flight (lazy)
    hipStream_t copy_st = nullptr;
    std::vector<hipEvent_t> chunk_ev;
    // ingest key table (open addressing on the 128-bit key hash)
    uint64_t *kt_key = nullptr;  // 2 per entry, kh0 == 0: empty
    uint32_t *kt_slot = nullptr;
    uint64_t kt_cap = 0, kt_count = 0;
    std::string last_hip;
};

#define HIPCHK(ctx, expr)                                                                         \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) {                                                                   \
            (ctx)->last_hip = std::string(#expr) + ": " + hipGetErrorString(_e);                  \
            return SKE_EHIP;                                                                      \
        }                                                                                         \
    } while (0)

namespace ske {

// ---- sketch_api_ctx.cpp

// staging buffer `slot` of at least `bytes` (nullptr and *rc set on failure)
void *stage_buf(ske_ctx *c, StageSlot slot, size_t bytes, int *rc);
// Items to device.  SKE_MEM_DEVICE pointers are used in place; host items are
// copied as the byte range [offs[0], offs[n]) plus offsets, and the device
// bytes pointer is rebased so that offs[] index it unchanged.
int stage_items(ske_ctx *c, const uint8_t *bytes, const uint32_t *offs, uint64_t n, int mem, Staged *out);
int stage_u32(ske_ctx *c, const uint32_t *p, uint64_t n, int mem, StageSlot slot, const uint32_t **out);

// One pass-timing mark: the event pair around what is enqueued on `st`
// between begin() and end().  Inert when not timing, or capturing.  No exit
// leaves a mark half-recorded: the destructor of a guard not yet ended (an
// error return) records the end event and voids the mark with every mark
// begun after it (those of the failed scope), so ske_pass_times recycles their
// events and counts none -- a failed host-fed call contributes nothing.
class PassMark {
public:
    PassMark() = default;
    PassMark(ske_ctx *c, int pass, hipStream_t st) { begin(c, pass, st); }
    PassMark(const PassMark &) = delete;
    PassMark &operator=(const PassMark &) = delete;
    ~PassMark() { abandon(); }
    // `start`: an end event just recorded on st with nothing enqueued since
    // (the previous kernel's), reused as this mark's start: one marker packet fewer
    void begin(ske_ctx *c, int pass, hipStream_t st, hipEvent_t start = nullptr);
    void end();  // records the end event; the mark counts
    hipEvent_t end_event() const { return b_; }  // once ended (nullptr when inert)

private:
    void abandon();
    ske_ctx *c_ = nullptr;
    hipEvent_t b_ = nullptr;
    hipStream_t st_ = nullptr;
    size_t idx_ = 0;     // of this mark in c_->marks (which only grows while a guard lives)
    bool open_ = false;  // begun, end event not yet recorded
};

// One use of an ordering group of the context scratch (c->xr, c->rt, c->sn or c->rw) by what
// is enqueued on `st` while the guard lives: the constructor makes st wait for
// the group's last use on another stream (rc != 0: it failed, nothing may be
// launched), the destructor notes this use on every exit after that.
//
// The wait only links launches of the same capture (or of none): an event
// recorded outside a capture cannot be waited on inside it, nor the reverse
// (the caller synchronises before recording a graph, as engine.capture does;
// ske_graph_launch records the event after a replay).
class ScratchUser {
public:
    ScratchUser(ske_ctx *c, ScratchUse &u, hipStream_t st);
    ~ScratchUser();
    ScratchUser(const ScratchUser &) = delete;
    ScratchUser &operator=(const ScratchUser &) = delete;
    int rc = SKE_OK;

private:
    ske_ctx *c_;
    ScratchUse &u_;
    hipStream_t st_;
    unsigned long long cid_ = 0;
};

// scratch that cannot grow (a graph is being recorded, or alive) -> SKE_EBUSY
int scratch_error(ske_ctx *c, hipError_t e);

inline Filter *get_filter(ske_ctx *c, uint32_t fid) { return fid < c->filters.size() ? &c->filters[fid] : nullptr; }

// the sticky slot-error word around a synchronous call (see k_err_begin)
int err_begin(ske_ctx *c);
int check_call_err(ske_ctx *c);

// ---- sketch_api_bloom.cpp
void free_filter(Filter &F);
// the kernel view of F's chain (cached; the empty chain for a missing key)
const ChainDev &chain_of(Filter *F);

// ---- the device-object table (Count-Min tables, heavy-hitter sets, time
// profiles, tallies, seen-row sets, row logs): what a family's calls answer and
// say.  The two flags are behaviour the families differ in, kept as it is.
struct ObjFamily {
    uint32_t max_id;             // ids are 0 .. max_id - 1
    int e_nosuch, e_exists;      // no object under the id; init of an id in use
    int e_cap;                   // init with capacity_log2 outside [min_log2, max_log2]
    uint32_t min_log2, max_log2; //   (max_log2 == 0: the family has no capacity exponent and sizes itself)
    size_t head_bytes, slot_bytes;  // the allocation: a head, then 2^capacity_log2 slots
    const char *tag;             // "hipMalloc(tag): ..."
    const char *noun;            // "<noun> cannot be freed while ..."
    hipError_t (*setup)();       // the kernels' one-time setup, run by the first init that gets that far
    bool ske_ctx::*ready;        //   (nullptr: none) and the context's flag that it is done
    bool id_checked;             // an id >= max_id is SKE_EINVAL in every call (false: only in init; elsewhere e_nosuch)
    bool info_refuses;           // info refuses while a graph is being recorded (false: it fails on its stream wait)
};
constexpr ObjFamily kCmsFamily{SKE_MAX_CMS, SKE_ECMSNOKEY, SKE_ECMSEXISTS, 0, 0, 0, 0, 0, "cms", "a Count-Min Sketch table",
                               cms_setup, &ske_ctx::cms_lds_ready, false, false};
constexpr ObjFamily kHhFamily{SKE_MAX_HH, SKE_EHHNOSET, SKE_EHHEXISTS, SKE_EHHCAP, SKE_HH_MIN_LOG2, SKE_HH_MAX_LOG2,
                              16, 28, "hh", "a heavy-hitter set", hh_setup, &ske_ctx::hh_lds_ready, false, false};
constexpr ObjFamily kTpFamily{SKE_MAX_TP, SKE_ETPNOSET, SKE_ETPEXISTS, 0, 0, 0, 0, 0, "tp", "a time profile",
                              nullptr, nullptr, true, true};
constexpr ObjFamily kTallyFamily{SKE_MAX_TALLY, SKE_ETALLYNOSET, SKE_ETALLYEXISTS, SKE_ETALLYCAP, SKE_TALLY_MIN_LOG2,
                                 SKE_TALLY_MAX_LOG2, 64, 60, "tally", "a tally", tally_setup, &ske_ctx::tally_ready,
                                 true, true};
constexpr ObjFamily kSeenFamily{SKE_MAX_SEEN, SKE_ESEENNOSET, SKE_ESEENEXISTS, SKE_ESEENCAP, SKE_SEEN_MIN_LOG2,
                                SKE_SEEN_MAX_LOG2, 64, 24, "seen", "a seen set", nullptr, nullptr, true, true};
constexpr ObjFamily kRowsFamily{SKE_MAX_ROWS, SKE_EROWSNOLOG, SKE_EROWSEXISTS, SKE_EROWSCAP, SKE_ROWS_MIN_LOG2,
                                SKE_ROWS_MAX_LOG2, 64, SKE_ROWS_ROW_BYTES, "rows", "a row log", nullptr, nullptr, true, true};

// the object of an id in use, else nullptr and *rc: why not
template <class T>
T *obj_get(const ObjFamily &F, std::vector<T> &v, uint32_t id, int *rc) {
    if (F.id_checked && id >= F.max_id) return *rc = SKE_EINVAL, nullptr;
    if (id < v.size() && v[id].base) return &v[id];
    return *rc = F.e_nosuch, nullptr;
}

// the same for a call that waits for the stream, so it cannot be recorded
// (refuse == false: an info that takes no notice of a recording)
template <class T>
T *obj_for_sync_call(ske_ctx *c, const ObjFamily &F, std::vector<T> &v, uint32_t id, const char *what, int *rc,
                     bool refuse = true) {
    T *o = obj_get(F, v, id, rc);
    if (o && refuse && c->capturing) {
        c->last_hip = std::string(what) + " waits for the stream and cannot be recorded";
        return *rc = SKE_EBUSY, nullptr;
    }
    return o;
}

template <class T>
void obj_free(T &o) {
    if (o.base) (void)hipFree(o.base);
    o = T{};
}

// A new object under a free id: o carries log2 (or, in a family without one,
// bytes) and the family's own fields; clear(o) -- a hipError_t -- makes the
// allocation an empty object and waits for that.  Stored only when all of it
// succeeded.
template <class T, class Clear>
int obj_alloc(ske_ctx *c, const ObjFamily &F, std::vector<T> &v, uint32_t id, T o, Clear clear) {
    if (!c || id >= F.max_id) return SKE_EINVAL;
    if (F.max_log2) {
        if (o.log2 < F.min_log2 || o.log2 > F.max_log2) return F.e_cap;
        o.bytes = F.head_bytes + (size_t(1) << o.log2) * F.slot_bytes;
    }
    if (id < v.size() && v[id].base) return F.e_exists;
    if (v.size() <= id) v.resize(F.max_id);
    if (F.setup && !(c->*F.ready)) {  // an LDS form larger than the default LDS limit
        const hipError_t e = F.setup();
        if (e != hipSuccess) {
            c->last_hip = std::string(F.tag) + "_setup(): " + hipGetErrorString(e);
            return SKE_EHIP;
        }
        c->*F.ready = true;
    }
    hipError_t e = hipMalloc(&o.base, o.bytes);
    if (e != hipSuccess) {
        c->last_hip = std::string("hipMalloc(") + F.tag + "): " + hipGetErrorString(e);
        return SKE_ENOMEM;
    }
    e = clear(o);
    if (e != hipSuccess) {
        obj_free(o);
        c->last_hip = std::string("hipMemset(") + F.tag + "): " + hipGetErrorString(e);
        return SKE_EHIP;
    }
    v[id] = o;
    return SKE_OK;
}
// the usual clear: `bytes` zero bytes from the base, waited for
inline hipError_t obj_zero(const DevObj &o, size_t bytes, hipStream_t st) {
    hipError_t e = hipMemsetAsync(o.base, 0, bytes, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

// ske_X_free: not while a graph that may point to the object is recorded or alive
template <class T>
int obj_release(ske_ctx *c, const ObjFamily &F, std::vector<T> &v, uint32_t id) {
    if (!c) return SKE_EINVAL;
    int rc = SKE_OK;
    T *o = obj_get(F, v, id, &rc);
    if (!o) return rc;
    if (c->live_graphs > 0 || c->capturing) {
        c->last_hip = std::string(F.noun) + " cannot be freed while a recorded graph may point to it";
        return SKE_EBUSY;
    }
    HIPCHK(c, hipStreamSynchronize(c->st));
    obj_free(*o);
    return SKE_OK;
}

// the first `bytes` of the allocation on the host, waited for
inline int obj_read_head(ske_ctx *c, const DevObj &o, void *dst, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, o.base, bytes, hipMemcpyDeviceToHost, c->st));
    HIPCHK(c, hipStreamSynchronize(c->st));
    return SKE_OK;
}

// ---- sketch_api_cms.cpp
// the table of a cid in use, else nullptr (SKE_ECMSNOKEY: the family has no other answer); its kernel view
inline Cms *get_cms(ske_ctx *c, uint32_t cid) {
    int rc = SKE_OK;
    return obj_get(kCmsFamily, c->cms, cid, &rc);
}
CmsTable table_of(const Cms &T);

// ---- sketch_api_swipes.cpp
bool use_lds(const ske_ctx *c, const ChainDev &ch);
// The short-id LDS kernel (sketch_k1.hip) when the chain, the batch and the
// options allow it; false: use the generic kernels.
bool k1_fast_args(ske_ctx *c, const ChainDev &ch, const PartBatch &b, K1Args *A);
// blocks of the short-id LDS K1: option "k1_grid", or one per CU
inline int k1_grid(const ske_ctx *c) { return c->k1_grid ? c->k1_grid : c->cus; }
// Enqueue K1 (mode swipes) over b on st with the variant the chain selects;
// `grid`: blocks of the short-id LDS K1
int launch_k1(ske_ctx *c, const ChainDev &ch, const PartBatch &b, hipStream_t st, int grid);

}  // namespace ske
