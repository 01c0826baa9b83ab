// sketch_common.h -- shared host/device arithmetic for libsketch (gfx950).
//
// Everything here is the bit-exact arithmetic of the upstream routines the
// reference reaches through redis-py (attendance_processor.py:109-113 BF.EXISTS,
// :127-129 PFADD; data_generator.py:57-63 BF.ADD), re-expressed for 64-wide
// wavefronts: items are loaded as aligned little-endian 64-bit words, the
// Bloom probe sequence (a + i*b) mod 2^64 mod bits is stepped incrementally
// with an exact carry correction instead of k 64-bit divisions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define SKE_HD __host__ __device__ __forceinline__

namespace ske {

constexpr uint64_t kMurmurM = 0xc6a4a7935bd1e995ULL;
constexpr uint64_t kBloomSeed = 0xc6a4a7935bd1e995ULL;  // bloom_calc_hash64() first seed
constexpr uint64_t kHllSeed = 0xadc83b19ULL;            // hllPatLen() seed
constexpr int kHllP = 14;
constexpr int kHllQ = 64 - kHllP;
constexpr uint32_t kHllRegs = 1u << kHllP;
constexpr int kMaxLinks = 48;

// ---------------------------------------------------------------------------
// MurmurHash64A (Redis src/hyperloglog.c MurmurHash64A, RedisBloom
// deps/murmur2/MurmurHash2.c MurmurHash64A_Bloom -- identical arithmetic).
// ---------------------------------------------------------------------------
SKE_HD uint64_t mm_block(uint64_t h, uint64_t k) {
    k *= kMurmurM;
    k ^= k >> 47;
    k *= kMurmurM;
    h ^= k;
    h *= kMurmurM;
    return h;
}
SKE_HD uint64_t mm_final(uint64_t h) {
    h ^= h >> 47;
    h *= kMurmurM;
    h ^= h >> 47;
    return h;
}

// Little-endian value of nb (1..8) bytes at p, zero padded, from aligned
// 64-bit words only (never touches a word that holds no byte of the item).
// (pointer arithmetic on p itself, never an integer round trip, so the load
// stays a global_load and does not become a flat_load.)
__device__ __forceinline__ uint64_t load_le(const uint8_t *p, uint32_t nb) {
    const uint32_t off = uint32_t(reinterpret_cast<uintptr_t>(p) & 7);
    const uint64_t *w = reinterpret_cast<const uint64_t *>(p - off);
    uint64_t v = w[0] >> (off * 8);
    if (off + nb > 8) v |= w[1] << (64 - off * 8);
    if (nb < 8) v &= (uint64_t(1) << (nb * 8)) - 1;
    return v;
}

// The wavefront append: one entry per passing lane behind *counter.  The passing
// lanes are counted by one ballot, lane 0 adds the count to *counter once, and a
// passing lane's entry is the sum before that add plus the passing lanes below
// it.  Returns the entry's index -- the caller drops an index at or beyond its
// capacity, so *counter counts all that pass -- or kNoAppend in a lane that does
// not pass.  Every lane of the wavefront must reach the call (workgroups are
// whole wavefronts of one dimension).
constexpr uint32_t kNoAppend = 0xffffffffu;
__device__ __forceinline__ uint32_t wave_append(bool pass, unsigned int *counter) {
    const unsigned long long votes = __ballot(pass);
    if (votes == 0) return kNoAppend;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, uint32_t(__popcll(votes)));
    base = __shfl(base, 0, 64);
    return pass ? base + uint32_t(__popcll(votes & ((1ull << lane) - 1))) : kNoAppend;
}

// An item held as its first two 8-byte blocks (enough for every student id
// of the configs: 5..8 decimal digits); longer items re-read blocks 2.. .
struct Item {
    const uint8_t *p;
    uint32_t len;
    uint64_t w0, w1;
};

__device__ __forceinline__ Item load_item(const uint8_t *bytes, uint32_t b, uint32_t e) {
    Item it;
    it.p = bytes + b;
    it.len = e - b;
    it.w0 = it.len ? load_le(it.p, it.len < 8 ? it.len : 8) : 0;
    it.w1 = it.len > 8 ? load_le(it.p + 8, it.len < 16 ? it.len - 8 : 8) : 0;
    return it;
}

__device__ __forceinline__ uint64_t murmur_item(const Item &it, uint64_t seed) {
    uint64_t h = seed ^ (uint64_t(it.len) * kMurmurM);
    const uint32_t nblk = it.len >> 3, rem = it.len & 7;
    if (nblk >= 1) h = mm_block(h, it.w0);
    if (nblk >= 2) h = mm_block(h, it.w1);
    for (uint32_t j = 2; j < nblk; j++) h = mm_block(h, load_le(it.p + 8 * j, 8));
    if (rem) {
        uint64_t t = nblk == 0 ? it.w0 : (nblk == 1 ? it.w1 : load_le(it.p + 8 * nblk, rem));
        h ^= t;
        h *= kMurmurM;
    }
    return mm_final(h);
}

// murmur_item for an item of at most 16 bytes from its two words alone (no
// memory access; host-callable).
SKE_HD uint64_t murmur_words(uint64_t w0, uint64_t w1, uint32_t len, uint64_t seed) {
    uint64_t h = seed ^ (uint64_t(len) * kMurmurM);
    const uint32_t nblk = len >> 3;
    if (nblk >= 1) h = mm_block(h, w0);
    if (nblk >= 2) h = mm_block(h, w1);
    if (len & 7) {
        h ^= nblk == 0 ? w0 : w1;
        h *= kMurmurM;
    }
    return mm_final(h);
}

// Heavy-hitter sets (sketch_hh.hip): an id's claim word is its digest -- the
// Bloom path's hash of the id bytes, 0 (the empty slot) mapped to 1 -- and its
// probe path starts at the digest's low bits.
SKE_HD uint64_t hh_digest(uint64_t w0, uint64_t w1, uint32_t len) {
    const uint64_t d = murmur_words(w0, w1, len, kBloomSeed);
    return d ? d : 1;
}
SKE_HD uint32_t hh_start(uint64_t digest, uint32_t capacity_log2) {
    return uint32_t(digest) & ((1u << capacity_log2) - 1);
}

// Tallies (sketch_tally.hip): a key of at most 32 bytes is held as four
// little-endian words, zero padded.  Its claim word is its digest -- the general
// item hash (MurmurHash64A of the key bytes, the Bloom seed; the length enters
// through the seed word, so b"A" and b"A\0" differ), 0 (the empty slot) mapped
// to 1 -- and its probe path starts at the digest's low bits.
constexpr uint32_t kTallyKeyWords = 4;
SKE_HD uint64_t tally_digest(const uint64_t (&w)[kTallyKeyWords], uint32_t len) {
    uint64_t h = kBloomSeed ^ (uint64_t(len) * kMurmurM);
    const uint32_t nblk = len >> 3;
    uint64_t tail = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTallyKeyWords; j++) {
        if (j < nblk)
            h = mm_block(h, w[j]);
        else if (j == nblk)
            tail = w[j];
    }
    if (len & 7) {
        h ^= tail;
        h *= kMurmurM;
    }
    h = mm_final(h);
    return h ? h : 1;
}
SKE_HD uint32_t tally_start(uint64_t digest, uint32_t capacity_log2) {
    return uint32_t(digest) & ((1u << capacity_log2) - 1);
}
// The order of a listing: count descending, then key bytes ascending (a prefix
// before its extensions: the padding is zero, so the padded bytes decide all
// but that, and there the shorter key is first).  ka, kb: 32 padded bytes.
inline bool tally_before(uint64_t ca, const uint8_t *ka, uint32_t la, uint64_t cb, const uint8_t *kb, uint32_t lb) {
    if (ca != cb) return ca > cb;
    for (uint32_t j = 0; j < 8 * kTallyKeyWords; j++)
        if (ka[j] != kb[j]) return ka[j] < kb[j];
    return la < lb;
}

// MurmurHash64A of an item of at most 8 bytes held in w (zero padded).
SKE_HD uint64_t murmur_short(uint64_t w, uint32_t len, uint64_t seed) {
    uint64_t h = seed ^ (uint64_t(len) * kMurmurM);
    if (len == 8) {
        h = mm_block(h, w);
    } else if (len) {
        h ^= w;
        h *= kMurmurM;
    }
    return mm_final(h);
}

// Seen-row sets (sketch_seen.hip): a row key is two 64-bit words.  It starts at
// the two seeds; folding a column replaces each word k by MurmurHash64A(the
// column's bytes, seed = k), so the key is a function of the columns' bytes,
// their lengths and their order.  The set reads a word 0 (the empty slot) as 1.
// A row's probe path starts at the low bits of its first word.
constexpr uint64_t kSeenSeed0 = 0x9e3779b97f4a7c15ULL;
constexpr uint64_t kSeenSeed1 = 0xd1b54a32d192ed03ULL;
constexpr uint32_t kSeenMaxProbes = 128;  // slots one walk looks at (SKE_SEEN_MAX_PROBES)
constexpr uint32_t kSeenLoadDen = 2;      // new claims stop at capacity / kSeenLoadDen (SKE_SEEN_LOAD_DEN)
struct SeenKey {
    uint64_t k0, k1;
};
SKE_HD SeenKey seen_begin() { return SeenKey{kSeenSeed0, kSeenSeed1}; }
// one column of at most 16 bytes from its two zero-padded words
SKE_HD SeenKey seen_fold_words(SeenKey k, uint64_t w0, uint64_t w1, uint32_t len) {
    return SeenKey{murmur_words(w0, w1, len, k.k0), murmur_words(w0, w1, len, k.k1)};
}
// floor(epoch / granularity), granularity >= 1, also for a negative epoch
SKE_HD int64_t seen_bucket(int64_t epoch, int64_t granularity) {
    int64_t q = epoch / granularity;  // toward zero
    if (epoch % granularity < 0) q -= 1;
    return q;
}
// the time column: the bucket's 8 little-endian bytes
SKE_HD SeenKey seen_fold_epoch(SeenKey k, int64_t epoch, int64_t granularity) {
    const uint64_t b = uint64_t(seen_bucket(epoch, granularity));
    return SeenKey{murmur_short(b, 8, k.k0), murmur_short(b, 8, k.k1)};
}
SKE_HD uint64_t seen_word(uint64_t k) { return k ? k : 1; }
SKE_HD uint32_t seen_start(uint64_t k0, uint32_t capacity_log2) {
    return uint32_t(k0 & ((uint64_t(1) << capacity_log2) - 1));
}
SKE_HD uint64_t seen_limit(uint32_t capacity_log2) { return (uint64_t(1) << capacity_log2) / kSeenLoadDen; }

// Row logs (sketch_rows.hip): the attendance table's rows, appended in arrival
// order.  A row's partition is its lecture's digest -- the tally's identity rule
// (tally_digest above) over a lecture of any length: MurmurHash64A of the
// lecture bytes, the Bloom seed, 0 mapped to 1 -- so a tally listing names the
// log's partitions.  Two lectures with equal digests are one partition.
constexpr int kRowsBlock = 256;         // items per workgroup and tile of an append (SKE_ROWS_BLOCK)
constexpr uint32_t kRowsIdMaxLen = 20;  // "-9223372036854775808"
SKE_HD uint64_t rows_lecture_word(uint64_t murmur) { return murmur ? murmur : 1; }
// the digest from byte loads alone (host restatement of murmur_item's arithmetic)
SKE_HD uint64_t rows_lecture_digest(const uint8_t *p, uint32_t len) {
    uint64_t h = kBloomSeed ^ (uint64_t(len) * kMurmurM);
    const uint32_t nblk = len >> 3, rem = len & 7;
    for (uint32_t j = 0; j < nblk; j++, p += 8) {
        uint64_t k = 0;
        for (uint32_t b = 0; b < 8; b++) k |= uint64_t(p[b]) << (8 * b);
        h = mm_block(h, k);
    }
    if (rem) {
        uint64_t t = 0;
        for (uint32_t b = 0; b < rem; b++) t |= uint64_t(p[b]) << (8 * b);
        h ^= t;
        h *= kMurmurM;
    }
    return rows_lecture_word(mm_final(h));
}
// The id column is Cassandra's `student_id int`: the id's text must be canonical
// decimal -- "-"? then digits, no leading zero except "0" itself, no "-0", no
// "+", no blanks -- and fit int64.  The text is its first 24 bytes as three
// little-endian words, zero padded (len <= kRowsIdMaxLen matters, longer is
// refused unread).  false: not an integer, the row is refused.
SKE_HD bool rows_parse_id(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t len, int64_t *out) {
    if (len == 0 || len > kRowsIdMaxLen) return false;
    const uint32_t neg = (w0 & 0xff) == '-' ? 1u : 0u;
    const uint32_t ndig = len - neg;
    if (ndig == 0 || ndig > 19) return false;
    uint64_t v = 0;
    bool ok = true;
    uint32_t first = 0;
    for (uint32_t j = neg; j < len; j++) {
        const uint64_t w = j < 8 ? w0 : (j < 16 ? w1 : w2);
        const uint32_t ch = uint32_t(w >> (8 * (j & 7))) & 0xff;
        const uint32_t d = ch - '0';
        ok = ok && d <= 9;
        if (j == neg) first = d;
        v = v * 10 + d;  // 19 digits stay below 2^64
    }
    if (!ok) return false;
    if (first == 0 && (ndig > 1 || neg)) return false;
    if (neg) {
        if (v > (uint64_t(1) << 63)) return false;
        *out = int64_t(~v + 1);
    } else {
        if (v > (uint64_t(1) << 63) - 1) return false;
        *out = int64_t(v);
    }
    return true;
}

// ---------------------------------------------------------------------------
// MurmurHash2, the 32-bit form (RedisBloom deps/murmur2/MurmurHash2.c
// MurmurHash2): the Count-Min Sketch's row hash, cell of row i =
// MurmurHash2(item, len, seed = i) % width (src/cms.c).  Little-endian 4-byte
// blocks, a tail of 3 / 2 / 1 bytes, then the final mix.
// ---------------------------------------------------------------------------
constexpr uint32_t kMurmur2M = 0x5bd1e995u;

SKE_HD uint32_t mm2_block(uint32_t h, uint32_t k) {
    k *= kMurmur2M;
    k ^= k >> 24;
    k *= kMurmur2M;
    h *= kMurmur2M;
    h ^= k;
    return h;
}
// t: the rem (1..3) tail bytes, little-endian, zero padded
SKE_HD uint32_t mm2_tail(uint32_t h, uint32_t t) {
    h ^= t;
    h *= kMurmur2M;
    return h;
}
SKE_HD uint32_t mm2_final(uint32_t h) {
    h ^= h >> 13;
    h *= kMurmur2M;
    h ^= h >> 15;
    return h;
}

// the routine itself over any byte string (byte loads only: no alignment and
// no readable byte past the item is assumed)
SKE_HD uint32_t murmur2_32(const uint8_t *p, uint32_t len, uint32_t seed) {
    uint32_t h = seed ^ len;
    const uint32_t nblk = len >> 2, rem = len & 3;
    for (uint32_t j = 0; j < nblk; j++, p += 4)
        h = mm2_block(h, uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24);
    if (rem) {
        uint32_t t = p[0];
        if (rem >= 2) t |= uint32_t(p[1]) << 8;
        if (rem == 3) t |= uint32_t(p[2]) << 16;
        h = mm2_tail(h, t);
    }
    return mm2_final(h);
}

// The same hash of an item of at most 16 bytes held as two little-endian
// 64-bit words, zero padded (Item::w0 / w1): no memory access per row.
SKE_HD uint32_t murmur2_32_words(uint64_t w0, uint64_t w1, uint32_t len, uint32_t seed) {
    uint32_t h = seed ^ len;
    const uint32_t nblk = len >> 2;
    if (nblk >= 1) h = mm2_block(h, uint32_t(w0));
    if (nblk >= 2) h = mm2_block(h, uint32_t(w0 >> 32));
    if (nblk >= 3) h = mm2_block(h, uint32_t(w1));
    if (nblk >= 4) h = mm2_block(h, uint32_t(w1 >> 32));
    if (len & 3) {
        // the padding above the tail bytes is zero, so the block that holds
        // them is the tail value
        const uint64_t w = nblk >= 2 ? w1 : w0;
        h = mm2_tail(h, uint32_t(nblk & 1 ? w >> 32 : w));
    }
    return mm2_final(h);
}

// Exact n mod d for 32-bit n and a runtime divisor 1 <= d < 2^32 (the same
// Granlund-Montgomery form as Divisor below, in 32 bits: l = ceil(log2 d),
// m = floor(2^32 (2^l - d) / d) + 1, t = mulhi(m, n),
// q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0)).
struct Div32 {
    uint32_t d, m, sh1, sh2;
};
SKE_HD uint32_t fastmod32(uint32_t n, const Div32 &D) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t t = __umulhi(D.m, n);
#else
    const uint32_t t = uint32_t(uint64_t(D.m) * n >> 32);
#endif
    const uint32_t q = (t + ((n - t) >> D.sh1)) >> D.sh2;
    return n - q * D.d;
}
inline Div32 make_div32(uint32_t d) {
    Div32 D{};
    D.d = d;
    uint32_t l = 0;
    while (l < 32 && (uint64_t(1) << l) < d) l++;
    D.m = uint32_t(((uint64_t(1) << 32) * ((uint64_t(1) << l) - d)) / d + 1);
    D.sh1 = l < 1 ? l : 1;
    D.sh2 = l > 1 ? l - 1 : 0;
    return D;
}

// hllPatLen(): index = low 14 bits, count = 1 + trailing zeros of
// (hash >> 14) | 1<<50, in [1, 51].
SKE_HD void hll_patlen(uint64_t hash, uint32_t &idx, uint32_t &rank) {
    idx = uint32_t(hash & (kHllRegs - 1));
    uint64_t w = (hash >> kHllP) | (uint64_t(1) << kHllQ);
#ifdef __HIP_DEVICE_COMPILE__
    rank = uint32_t(__builtin_ctzll(w)) + 1;
#else
    rank = uint32_t(__builtin_ctzll(w)) + 1;
#endif
}

// ---------------------------------------------------------------------------
// Exact n mod d for a runtime divisor (Granlund-Montgomery, "Division by
// invariant integers using multiplication", fig. 4.1): l = ceil(log2 d),
// m = floor(2^64 (2^l - d) / d) + 1, q = (t + ((n - t) >> 1)) >> (l - 1),
// t = mulhi(m, n).  Valid for every 64-bit n and 2 <= d < 2^63.
// ---------------------------------------------------------------------------
struct Divisor {
    uint64_t d;    // bloom->bits
    uint64_t m;    // magic
    uint64_t t;    // 2^64 mod d (carry correction of the probe stepping)
    uint32_t sh;   // l - 1
    uint32_t pad_;
};

SKE_HD uint64_t mulhi64(uint64_t a, uint64_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return uint64_t((unsigned __int128)a * b >> 64);
#endif
}

SKE_HD uint64_t fastmod(uint64_t n, const Divisor &D) {
    uint64_t t1 = mulhi64(D.m, n);
    uint64_t q = (t1 + ((n - t1) >> 1)) >> D.sh;
    return n - q * D.d;
}

inline Divisor make_divisor(uint64_t d) {
    Divisor D{};
    D.d = d;
    uint32_t l = 0;
    while (l < 64 && (uint64_t(1) << l) < d) l++;
    unsigned __int128 num = ((unsigned __int128)1 << 64) * ((uint64_t(1) << l) - d);
    D.m = uint64_t(num / d) + 1;
    D.sh = l - 1;
    D.t = uint64_t((((unsigned __int128)1) << 64) % d);
    return D;
}

// Probe cursor over x_i = (a + i*b) mod 2^64 mod d  (CHECK_ADD_FUNC with
// bloom_check_add_compat's modulus bloom->bits).  step() keeps v_i = a+i*b
// (mod 2^64) and x_i; when v wraps, x drops by 2^64 mod d.
struct ProbeCursor {
    uint64_t v, b, x, bm;
    SKE_HD void init(uint64_t a, uint64_t b_, const Divisor &D) {
        v = a;
        b = b_;
        x = fastmod(a, D);
        bm = fastmod(b_, D);
    }
    SKE_HD void step(const Divisor &D) {
        uint64_t vn = v + b;
        bool carry = vn < v;
        v = vn;
        x += bm;
        if (x >= D.d) x -= D.d;
        if (carry) x = (x >= D.t) ? x - D.t : x + D.d - D.t;
    }
};

SKE_HD uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }  // v_min_u32

// The same cursor with x kept in 32 bits, valid when d <= 2^31 (every Bloom
// link up to ~2^31 bits: all configs; x + bm < 2^32 cannot overflow).  v, the
// 64-bit running sum a + i*b, is still tracked for its carry.
struct ProbeCursor32 {
    uint64_t v, b;
    uint32_t x, bm;
    SKE_HD void init(uint64_t a, uint64_t b_, const Divisor &D) {
        v = a;
        b = b_;
        x = uint32_t(fastmod(a, D));
        bm = uint32_t(fastmod(b_, D));
    }
    SKE_HD void step(const Divisor &D) { step(uint32_t(D.d), uint32_t(D.t)); }
    // x, bm < d <= 2^31: "x = min(x, x - d)" is the conditional subtract (a
    // wrapped x - d is the larger one); the wrap of v subtracts t = 2^64 mod d,
    // and "min(x, x + d)" undoes an underflow the same way.
    SKE_HD void step(uint32_t d, uint32_t t) {
        const uint64_t vn = v + b;
        const uint32_t tsel = vn < v ? t : 0u;
        v = vn;
        x += bm;
        x = umin32(x, x - d);
        x -= tsel;
        x = umin32(x, x + d);
    }
};

// The same walk with both increments precomputed: the step whose a + i*b
// wraps 2^64 adds inc1 = (bm - 2^64 mod d) mod d, every other step inc0 = bm,
// so a step is the 64-bit add (its carry selects the increment), one 32-bit
// add and one conditional subtract.  d <= 2^31.
struct ProbeWalk32 {
    uint64_t v, b;
    uint32_t x, inc0, inc1;
    SKE_HD void init(uint64_t a, uint64_t b_, const Divisor &D) {
        v = a;
        b = b_;
        x = uint32_t(fastmod(a, D));
        inc0 = uint32_t(fastmod(b_, D));
        const uint32_t m = inc0 - uint32_t(D.t);
        inc1 = umin32(m, m + uint32_t(D.d));
    }
    SKE_HD void step(uint32_t d) {
        const uint64_t vn = v + b;
        x += vn < v ? inc1 : inc0;
        v = vn;
        x = umin32(x, x - d);
    }
};

// One link of a RedisBloom scalable chain (SBLink.inner), device view.
struct LinkDev {
    const uint8_t *bf;  // bit array (bytes multiple of 8; LSB-first bits)
    Divisor div;
    uint32_t k;          // bloom->hashes
    uint32_t lds_off;    // byte offset of this link inside the LDS image
    uint32_t rmul;       // XCD-region split: region(x) = umulhi(x, rmul) in [0, 8)
    uint32_t pad_;
};

constexpr int kRegions = 8;  // one slice of every link per XCD

struct ChainDev {
    int32_t nlinks;
    uint32_t lds_bytes;  // sum of link bytes, 16-B aligned per link
    uint32_t pad_[2];
    LinkDev link[kMaxLinks];
};

// ---------------------------------------------------------------------------
// Synthetic stream (counter based).  mix(seed, i, j) = SplitMix64 finaliser
// of seed + golden * (i*256 + j + 1).  Restated in tests/golden/gen_ref.py.
// ---------------------------------------------------------------------------
SKE_HD uint64_t splitmix_fin(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
SKE_HD uint64_t mix(uint64_t seed, uint64_t i, uint32_t j) {
    return splitmix_fin(seed + 0x9e3779b97f4a7c15ULL * (i * 256 + j + 1));
}

struct GenDev {
    uint64_t seed, lo, R, N, mul, add, inv;
    uint32_t inv_thr, near_thr, n_keys, slot_base, width;
    const uint32_t *key_cdf;
    uint64_t pow10[20];
};

SKE_HD uint64_t gen_member(const GenDev &g, uint64_t i) { return g.lo + (g.mul * i + g.add) % g.R; }
SKE_HD bool gen_is_member(const GenDev &g, uint64_t x) {
    if (x < g.lo || x >= g.lo + g.R) return false;
    uint64_t r = (x - g.lo + g.R - g.add % g.R) % g.R;
    return (r * g.inv) % g.R < g.N;
}

// ---------------------------------------------------------------------------
// Time profile (sketch_tp.hip): a swipe's time, seconds since 1970-01-01T00:00:00
// UTC (any int64_t), as weekday (Monday = 0, datetime.weekday()), hour and
// second of the day, all by floor division.  One 64-bit division by the constant
// 86400 (a multiply-high), the rest in 32 bits:
//   sod   the low words of epoch - day * 86400 decide it (its range is 17 bits);
//   dow   (day + 3) mod 7, 1970-01-01 being a Thursday.  |day| < 1.07e14, so
//         d = day + 3 + 7 * 2e13 is positive and below 2^48, and with
//         2^32 = 4 and 2^16 = 2 (mod 7) its three 16-bit digits fold into one
//         19-bit sum with the same remainder.
// ---------------------------------------------------------------------------
constexpr uint32_t kTpBins = 168;  // weekday * 24 + hour (SKE_TP_BINS)
struct TpTime {
    uint32_t dow, hour, sod;
};
SKE_HD TpTime tp_time(int64_t epoch) {
    int64_t day = epoch / 86400;  // toward zero; corrected to the floor below
    int32_t sod = int32_t(uint32_t(uint64_t(epoch)) - uint32_t(uint64_t(day)) * 86400u);
    if (sod < 0) {
        sod += 86400;
        day -= 1;
    }
    const uint64_t d = uint64_t(day + 3 + 140000000000000LL);
    const uint32_t fold = uint32_t(d >> 32) * 4u + (uint32_t(d >> 16) & 0xffffu) * 2u + (uint32_t(d) & 0xffffu);
    TpTime t;
    t.dow = fold % 7u;
    t.sod = uint32_t(sod);
    t.hour = t.sod / 3600u;
    return t;
}
SKE_HD uint32_t tp_bin(const TpTime &t) { return t.dow * 24u + t.hour; }

// ---------------------------------------------------------------------------
// ISO-8601 timestamps of the ingest fast path (sketch_ingest.hip): the fields
// of an accepted "YYYY-MM-DD[?HH:MM:SS[.fff[fff]][+HH:MM|-HH:MM]]" as seconds
// since 1970-01-01T00:00:00 UTC -- analysis.epoch_seconds(datetime.
// fromisoformat(text)): a naive timestamp is UTC as written, an offset is
// subtracted, a date-only form is midnight (hh = mm = ss = 0), the fraction is
// dropped (it is non-negative, so that is the floor, also before 1970).
// ---------------------------------------------------------------------------
// days since 1970-01-01 of a proleptic Gregorian date (H. Hinnant's days_from_civil)
SKE_HD int32_t days_from_civil(int32_t y, uint32_t m, uint32_t d) {
    y -= m <= 2;
    const int32_t era = (y >= 0 ? y : y - 399) / 400;
    const uint32_t yoe = uint32_t(y - era * 400);
    const uint32_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const uint32_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + int32_t(doe) - 719468;
}
// off_sign: +1 / -1 for a "+HH:MM" / "-HH:MM" offset of oh hours om minutes, 0 for none
SKE_HD int64_t iso_epoch(uint32_t y, uint32_t mo, uint32_t d, uint32_t hh, uint32_t mi, uint32_t ss,
                         int32_t off_sign, uint32_t oh, uint32_t om) {
    const int64_t local = int64_t(days_from_civil(int32_t(y), mo, d)) * 86400 + int32_t(hh * 3600 + mi * 60 + ss);
    return local - int64_t(off_sign) * int32_t(oh * 3600 + om * 60);
}

}  // namespace ske
