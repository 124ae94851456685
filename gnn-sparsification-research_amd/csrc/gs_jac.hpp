// gs_jac.hpp -- Jaccard (metrics.py:17-64) on symmetric graphs, whole edge set: the
// rules, the plan and the state its units share.
//
// For a symmetric graph |out(u) ∩ in(v)| = |N(u) ∩ N(v)| is symmetric in (u, v),
// so each undirected pair is intersected ONCE, at its owner: the endpoint of
// larger degree (ties: smaller id).  The owner row's neighbour set is put in a
// hash table (LDS) or a bitmap (global, for rows too large for LDS) and the
// other endpoint's -- shorter -- list is streamed and probed.  Work is
// sum over pairs of min(d_u, d_v) probes instead of the d_u + d_v of a merge
// (RMAT-22: 1.24e10 vs 2.9e11), and the same value is written to both CSR
// entries (u,v) and (v,u) (rev(e) = tpos[e] on a symmetric graph).
//
// Rows are classed by degree:
//   light (d <= 32): one thread per owned entry, sorted-list merge
//   hash  (d <= 16384): tasks = (row, slice of its entries) sized to ~max(64K, 8 d)
//                   probes; the workgroup builds the row's table in LDS
//                   (capacity 2d..4d slots, 8 / 32 / 128 KiB classes), then each
//                   wave takes one owned entry at a time, 64 list elements per step
//   giant (d > 16384): same tasks against an n-bit bitmap of the row (global, L2)
// Counts are integers and the value is the reference's single fp64 division,
// so the output is bit-identical to the per-entry kernel in gs_scores.hip.
//
// Units: gs_jaccard.hip (knobs, driver), gs_jac_plan.hip (row classes, task lists,
// bitmap batches), gs_jac_hash.hip (light rows, LDS tables), gs_jac_bitmap.hip (giant
// rows), gs_jac_shares.hip (the sharded form's row ranges and owner lists).  A unit
// launches its own kernels only; the others call its host launchers below.  The
// __host__ __device__ rules are also compiled for the host by tools/jac_host_check.cpp.
#pragma once
#include "gs_internal.hpp"
#include "gs_util.hpp"

namespace gs {

static constexpr int64_t kJacLight = 32;
static constexpr int64_t kJacGiant = 16384;
static constexpr int64_t kJacTaskMin = 65536;
static constexpr int kJacClasses = 5;  // 4 LDS table sizes + bitmap
static constexpr int kJacBitmap = 4;
static constexpr int kJacMaxEnt = 1024;  // entries per task (LDS staging)
static constexpr int64_t kJacSmall = 16;  // d_v <= this: 16-lane groups

// Quotient tables (k_jac_hashq) for the classes in this mask, when the ids fit
#ifndef GS_JAC_Q16
#define GS_JAC_Q16 0xE  // classes 1, 2, 3
#endif

__host__ __device__ __forceinline__ bool jac_owns(int64_t du, int64_t dv, int32_t u, int32_t v) {
    return du > dv || (du == dv && u <= v);
}

__host__ __device__ __forceinline__ double jac_value(int64_t inter, int64_t du, int64_t dv) {
    double uni = (double)du + (double)dv - (double)inter;
    return uni > 0.0 ? (double)inter / uni : 0.0;
}

// counts != 0: the raw |N(u) ∩ N(v)| (gs_common_neighbors) instead of the ratio
__host__ __device__ __forceinline__ double jac_out(int counts, int64_t inter, int64_t du, int64_t dv) {
    return counts ? (double)inter : jac_value(inter, du, dv);
}

// Where a pair's result goes: both CSR entries of the full score vector (out,
// rev = tpos), or -- the sharded form (gs_jaccard_part_counts) -- the raw count
// into this part's compact owner-entry array cc[opre[e] - obase]
struct JacSink {
    double *out;
    const int64_t *rev;
    int counts;
    uint32_t *cc;
    const int64_t *opre;
    int64_t obase;
    __device__ __forceinline__ void put(int64_t e, int64_t cnt, int64_t du, int64_t dv) const {
        if (cc) {
            cc[opre[e] - obase] = (uint32_t)cnt;
            return;
        }
        const double val = jac_out(counts, cnt, du, dv);
        out[e] = val;
        out[rev[e]] = val;
    }
};

__host__ __device__ __forceinline__ int jac_class(int64_t d) {
    if (d <= kJacLight) return -1;
    if (d <= 1024) return 0;
    if (d <= 4096) return 1;
    if (d <= 8192) return 2;
    if (d <= kJacGiant) return 3;
    return kJacBitmap;
}

// probes per task: enough to amortise clearing the C-slot table and the d_u inserts
__host__ __device__ __forceinline__ int64_t jac_task_probes(int k, int64_t du) {
    const int64_t tab = k == 0 ? 2048 : k == 1 ? 8192 : k == 2 ? 16384 : k == 3 ? 32768 : 0;
    int64_t t = 16 * tab > 8 * du ? 16 * tab : 8 * du;
    return t > kJacTaskMin ? t : kJacTaskMin;
}

// task count of a row of class k >= 0 with owned-entry probe work w (sum of d_v)
__host__ __device__ __forceinline__ int64_t jac_row_tasks(int k, int64_t du, int64_t w) {
    if (k < 0 || !w) return 0;
    const int64_t t = jac_task_probes(k, du);
    int64_t nt = (w + t - 1) / t;
    const int64_t ne = (du + kJacMaxEnt - 1) / kJacMaxEnt;
    if (nt < ne) nt = ne;
    if (nt > du) nt = du;
    return nt;
}

// The tables' multiplicative hash with a 24-bit odd multiplier (v_mul_u32_u24, full rate,
// instead of v_mul_lo_u32, quarter rate): (x * K) mod 2^b is still a bijection of
// [0, 2^b) for the quotient tables, whose ids are < 2^24 (jac_qparams); the int32
// tables compare whole ids, so any hash is exact there
static constexpr uint32_t kJacMul24 = 0x9E3779u;  // odd
__host__ __device__ __forceinline__ uint32_t jac_mul(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(x, kJacMul24);
#else
    return (x & 0xFFFFFFu) * kJacMul24;
#endif
}

// Quotient tables (classes in GS_JAC_Q16, when the ids fit): 16-bit slots, so the
// same LDS holds twice the slots -- half the load factor, and the 32K-slot class
// runs two workgroups per CU instead of one.  h = (x * K) mod 2^b (jac_mul) is a
// bijection of [0, 2^b) (odd multiplier, n <= 2^b); its top bits pick the home
// bucket, the low qb bits (the remainder) go into the slot with the bucket's
// distance from home: slot = (d + 1) << qb | rem, 0 = empty.  (bucket, slot)
// gives h back, so a match is exact.  Buckets of 8 slots (one 16-B LDS read per
// probe step) fill from slot 0 up; a free slot 7 ends an unsuccessful search.
// An insert that would go past the largest distance a slot can encode flags the
// task, which then probes the owner's sorted list instead (never seen in practice).
struct JacQParams {
    uint32_t hmask, qb, rmask, dmax;  // 2^b - 1, remainder bits, 2^qb - 1, largest distance
};

// quotient-table parameters for C 16-bit slots and ids < n; false when the
// remainder leaves too few distance bits (n past ~2^24)
__host__ __device__ inline bool jac_qparams(int64_t n, int C, JacQParams &p) {
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < n) ++b;
    const int bb = __builtin_ctz((unsigned)(C / 8));
    if (b < bb) b = bb;
    const int qb = b - bb;
    if (16 - qb < 4) return false;
    p.hmask = b >= 32 ? 0xFFFFFFFFu : (uint32_t)(((uint64_t)1 << b) - 1);
    p.qb = (uint32_t)qb;
    p.rmask = (1u << qb) - 1;
    uint32_t dmax = (1u << (16 - qb)) - 2;
    if (dmax > (uint32_t)(C / 8 - 1)) dmax = (uint32_t)(C / 8 - 1);
    p.dmax = dmax;
    return true;
}

// the slot of remainder rem in the bucket d past its home bucket
__host__ __device__ __forceinline__ uint32_t jac_qslot(uint32_t qb, uint32_t d, uint32_t rem) {
    return ((d + 1) << qb) | rem;
}

// any zero 16-bit half in v
__host__ __device__ __forceinline__ uint32_t jac_hz16(uint32_t v) {
    return (v - 0x00010001u) & ~v & 0x80008000u;
}

// any of the 8 16-bit slots of a bucket equal to t (t2 = t in both halves): the packed
// 16-bit minimum of the four XORed words (v_pk_min_u16) has a zero half iff some slot
// matches -- 4 XOR + 3 packed minima + one zero-half test instead of four zero-half
// tests and their ORs
__host__ __device__ __forceinline__ bool jac_bucket_has(const uint4 &q, uint32_t t2) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const u16x2 a = __builtin_bit_cast(u16x2, q.x ^ t2), b = __builtin_bit_cast(u16x2, q.y ^ t2);
    const u16x2 c = __builtin_bit_cast(u16x2, q.z ^ t2), d = __builtin_bit_cast(u16x2, q.w ^ t2);
    const u16x2 m = __builtin_elementwise_min(__builtin_elementwise_min(a, b), __builtin_elementwise_min(c, d));
    return jac_hz16(__builtin_bit_cast(uint32_t, m)) != 0;
}

// Row ranges of the sharded form (gs_jaccard_shares): cuts = [R | E | O], P + 1
// values each -- cut rows, their first CSR entries, owner entries before them
struct JacShares {
    std::vector<int64_t> cuts;
    int P() const { return (int)(cuts.size() / 3) - 1; }
    int64_t R(int r) const { return cuts[r]; }
    int64_t E(int r) const { return cuts[P() + 1 + r]; }
    int64_t O(int r) const { return cuts[2 * (P() + 1) + r]; }
};
// the part that holds owner entry i: the last r < P of the ascending O with O[r] <= i
__host__ __device__ __forceinline__ int jac_part_of(const int64_t *O, int P, int64_t i) {
    return partition_point(P - 1, [=](int r) { return O[r + 1] <= i; });
}

// The GSPARSE_JAC* variables as they are now.  jac_knobs() (gs_jaccard.hip) is the only
// reader of the environment in the Jaccard units; an entry point calls it once.
struct JacKnobs {
    bool merge_only = false;  // GSPARSE_JACCARD=merge: gs_jaccard takes the per-entry kernel
    bool concurrent = true;   // GSPARSE_JAC_CONCURRENT=0: every class on the context stream
    // test hooks; each can only lower the value it caps
    int64_t qdmax = -1;   // GSPARSE_JAC_QDMAX >= 0: the quotient tables' largest distance
    int64_t bmrows = -1;  // GSPARSE_JAC_BMROWS >= 1: rows per bitmap batch
};
JacKnobs jac_knobs();

// Row classes, per-class task lists and bitmap batches of rows [r0, r1): a function of
// the graph and the rows only, so a repeated call on the same rows launches the class
// kernels from the kept lists -- no planning kernels, no host round trip.  The device
// arrays are the context's "jac_*" buffers (named where jac_plan allocates them).
struct JacPlan {
    bool valid = false;
    int64_t epoch = -1, r0 = 0, r1 = 0, n = 0, nnz = 0;  // the key ...
    int64_t bmrows = -1;  // ... and the batch cap the batches were cut with (JacKnobs)
    int64_t tot[kJacClasses] = {};                       // tasks per class
    int64_t ngiant = 0;                                  // rows with bitmap tasks
    struct Batch {
        int64_t g0, g1, t0, t1;  // bitmap rows grow[g0, g1), their tasks [t0, t1) of class 4
    };
    std::vector<Batch> batches;
    int8_t *cls = nullptr;     // [n] class of each row (rows [r0, r1) filled)
    int32_t *ntask = nullptr;  // [n] its task count
    int32_t *trow[kJacClasses] = {}, *ti[kJacClasses] = {};  // [tot[k]] row and index of each task
    int32_t *tslot = nullptr;  // [tot[kJacBitmap]] bitmap row (index into grow) of each task
    int32_t *grow = nullptr;   // [ngiant] the bitmap rows
    bool has(int64_t e, int64_t a, int64_t b, int64_t n_, int64_t z, int64_t cap) const {
        return valid && epoch == e && r0 == a && r1 == b && n == n_ && nnz == z && bmrows == cap;
    }
};

// owner lists of the sharded form (owner entry i in CSR order): CSR position, reverse
// entry, d_u + d_v; opre [nnz + 1] = owner entries before each CSR entry.  The lists
// exist (and nown is set) where positions fit int32
struct JacOwners {
    const int32_t *opos = nullptr, *orev = nullptr, *osum = nullptr;
    const int64_t *opre = nullptr;
    int64_t nown = 0;
};

struct JacState {
    JacPlan plan;
    std::map<int, JacShares> shares;  // row ranges by part count ...
    int64_t shares_epoch = -1;        // ... of this graph epoch, as the owner lists
    JacOwners own;
    double deg2 = 0.0;  // sum of squared degrees (the profile's byte count) ...
    int64_t deg2_epoch = -1;  // ... of this graph epoch
    // side streams of the hash classes, created on first concurrent use
    hipStream_t aux[kJacBitmap] = {};
    hipEvent_t aux_ev[kJacBitmap] = {};
    ~JacState() {
        for (auto &a : aux)
            if (a) (void)hipStreamDestroy(a);
        for (auto &e : aux_ev)
            if (e) (void)hipEventDestroy(e);
    }
};

inline JacState &jac_state(gs_ctx *c) {
    if (!c->jac) c->jac = std::make_shared<JacState>();
    return *c->jac;
}

// gs_jaccard.hip
// Whole-graph Jaccard of a symmetric graph into device out[nnz], or part `part` of
// `nparts` of it.  counts != 0: |N(u) ∩ N(v)| per entry instead of the Jaccard ratio;
// cc != nullptr: the part's raw counts into its compact owner-entry array
void jaccard_symmetric(gs_ctx *c, const JacKnobs &k, double *out, int part, int nparts,
                       int counts = 0, uint32_t *cc = nullptr);
// gs_jac_plan.hip: the kept plan of rows [r0, r1), or a new one; sum of squared degrees
const JacPlan &jac_plan(gs_ctx *c, const JacKnobs &k, int64_t r0, int64_t r1);
double jac_deg2(gs_ctx *c);
// gs_jac_hash.hip: light rows of entries [e0, e1); hash class k < kJacBitmap on stream s
void jac_launch_light(gs_ctx *c, int64_t e0, int64_t e1, const JacSink &sk);
void jac_launch_class(gs_ctx *c, int k, const JacPlan &p, const JacKnobs &kn, const JacSink &sk,
                      hipStream_t s);
// gs_jac_bitmap.hip: the plan's bitmap batches, on the context stream
void jac_launch_bitmap(gs_ctx *c, const JacPlan &p, const JacSink &sk);
// gs_jac_shares.hip
const JacShares &jaccard_shares(gs_ctx *c, int P);
const JacOwners &jac_owners(gs_ctx *c);  // after jaccard_shares on this graph
void jaccard_from_counts(gs_ctx *c, int P, const uint32_t *cc, int64_t stride, double *out);

}  // namespace gs
