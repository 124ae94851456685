// gs_cg.hpp -- what the ApproxER CG units share (gs_er.hip, gs_cg_stream.hip,
// gs_cg_res.hip, gs_cg_reg.hip): the BLAS chunk table, the per-column state, the lane
// geometry and the OpenBLAS ddot finish of the chain kernels, the plan of a solve
// (cg_plan: the only place that reads a GSPARSE_CG_* / GSPARSE_RES_* / GSPARSE_REG_*
// variable) and the three solvers' entry points.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <cstdlib>

#include "gs_internal.hpp"

namespace gs {

static constexpr int kMaxChunks = 64;
static constexpr int64_t kStoreQRowLen = 8;  // L_reg entries per row above which q is stored

// The BLAS thread chunks of a length-n ddot: chunk t is rows [a[t], a[t] + len[t]).
// Passed to the chain kernels by value.
struct ChunkArg {
    int32_t count;
    int64_t a[kMaxChunks];
    int64_t len[kMaxChunks];
};
static_assert(offsetof(ChunkArg, len) == offsetof(ChunkArg, a) + sizeof(int64_t) * kMaxChunks,
              "chunks_to_device copies a and len as one block");

inline ChunkArg make_chunks(int64_t n, int32_t threads) {
    ChunkArg ch{};
    if (n <= 10000 || threads <= 1) {
        ch.count = 1;
        ch.a[0] = 0;
        ch.len[0] = n;
        return ch;
    }
    // OpenBLAS's own thread limit (MAX_THREADS=64 in NumPy's build): more threads
    // cannot occur in the reference and are capped in cg_plan
    int64_t lo = 0, rem = n;
    int32_t cnt = 0;
    for (int32_t t = threads; t > 0 && rem > 0; --t) {
        int64_t w = (rem + t - 1) / t;
        ch.a[cnt] = lo;
        ch.len[cnt] = w;
        ++cnt;
        lo += w;
        rem -= w;
    }
    ch.count = cnt;
    return ch;
}

// The device copy the finish kernels read: starts at [0, kMaxChunks), lengths at
// [kMaxChunks, 2 kMaxChunks).  The copy is stream-ordered: ch must outlive the solve
// (it is the plan's, which gs_er_solve holds).
inline const int64_t *chunks_to_device(gs_ctx *c, const ChunkArg &ch) {
    const size_t bytes = sizeof(int64_t) * 2 * kMaxChunks;
    auto *dch = (int64_t *)c->buf("er_chunks").ensure(bytes);
    GS_HIP(hipMemcpyAsync(dch, ch.a, bytes, hipMemcpyHostToDevice, c->stream));
    return dch;
}

// per-column state, structure of arrays inside one buffer
struct ColPtrs {
    double *bn, *atol, *rho, *rho_prev, *alpha;
    int32_t *active, *iters;
    int32_t *xstep;    // iteration whose (alpha, p) is still to be added to x
    int32_t *nactive;  // single counter
};

static ColPtrs col_ptrs(ErState &er) {
    int64_t k = er.k;
    char *b = (char *)er.colstate.ptr;
    ColPtrs p;
    p.bn = (double *)b;
    p.atol = p.bn + k;
    p.rho = p.atol + k;
    p.rho_prev = p.rho + k;
    p.alpha = p.rho_prev + k;
    p.active = (int32_t *)(p.alpha + k);
    p.iters = p.active + k;
    p.xstep = p.iters + k;
    p.nactive = p.xstep + k;
    return p;
}

// ---------------------------------------------------------------- chain kernels' geometry
// Geometry of one batched-CG launch.  Lane layout: a wave owns ONE residue
// j (rows j, j+32, ... of a BLAS chunk -- that row sequence IS the OpenBLAS
// accumulator chain j) for CPL*64 consecutive columns, CPL columns per lane
// (CPL=2: 16-byte loads, two independent chains per lane).  A 256-thread
// workgroup holds 4 residues; the 8 workgroups of one (column block, chunk)
// pair get block ids b, b+8, ..., b+56 -- under the round-robin dispatch over
// the 8 XCDs they share one XCD's L2, so the neighbour rows a chain's SpMV
// gathers (mostly rows i-1, i+1, i+chord: other residues) are L2 hits.
struct CgGeom {
    int64_t n, k, ld, col0, col1;
    int32_t ncb;     // column blocks of CPL*64
    int32_t npairs;  // ncb * chunks
};

struct CgLane {
    int64_t c;   // first column of this lane
    int j, t;    // residue, chunk
    bool ok;
};

template <int CPL>
__device__ __forceinline__ CgLane cg_lane(const CgGeom &G) {
    const int b = blockIdx.x;
    const int grp = b >> 6, r = b & 63;
    const int sub = r & 7, part = r >> 3;  // part: which 4 of the 32 residues
    const int pair = grp * 8 + sub;
    CgLane L;
    L.ok = pair < G.npairs;
    const int cb = pair % G.ncb;
    L.t = pair / G.ncb;
    L.j = __builtin_amdgcn_readfirstlane(part * 4 + (int)(threadIdx.x >> 6));
    L.c = G.col0 + (int64_t)cb * (64 * CPL) + (int64_t)(threadIdx.x & 63) * CPL;
    return L;
}

template <int CPL>
struct Vec;
template <>
struct Vec<1> {
    double v[1];
    __device__ __forceinline__ void load(const double *p) { v[0] = *p; }
    __device__ __forceinline__ void store(double *p) const { *p = v[0]; }
};
template <>
struct Vec<2> {
    double v[2];
    __device__ __forceinline__ void load(const double *p) {
        double2 t = *reinterpret_cast<const double2 *>(p);
        v[0] = t.x;
        v[1] = t.y;
    }
    __device__ __forceinline__ void store(double *p) const {
        *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
    }
};

// OpenBLAS ddot finish (see oracle_ddot), one wave per column, one lane per
// BLAS chunk t: fold of the chunk's 32 chains, its optional 16-row block and
// FMA tail, then the chunk dots added in order from 0.0 (a single chunk is
// returned as is).  Values of the (< 32) leftover rows of chunk t are A[row]
// and, when Bside != nullptr, Bside[(t*32 + row - a - n32) * ld] (else B[row]).
__device__ __forceinline__ double chunk_dot(const double *__restrict__ a32, int64_t a, int64_t L,
                                            int t, int64_t ld, int64_t c,
                                            const double *__restrict__ A,
                                            const double *__restrict__ B,
                                            const double *__restrict__ Bside) {
    const int64_t n1 = L & ~(int64_t)15, n32 = n1 & ~(int64_t)31;
    auto bval = [&](int64_t row) {
        return Bside ? Bside[((int64_t)t * 32 + (row - a - n32)) * ld + c] : B[row * ld + c];
    };
    double dot = 0.0;
    if (n1) {
        double b[16];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int l = 0; l < 4; ++l) b[4 * q + l] = a32[8 * q + l] + a32[8 * q + 4 + l];
        if (n1 > n32) {
#pragma unroll
            for (int jj = 0; jj < 16; ++jj) {
                const int64_t row = a + n32 + jj;
                b[jj] = __builtin_fma(A[row * ld + c], bval(row), b[jj]);
            }
        }
        double c4[4];
#pragma unroll
        for (int l = 0; l < 4; ++l) c4[l] = ((b[l] + b[4 + l]) + b[8 + l]) + b[12 + l];
        dot = (c4[0] + c4[2]) + (c4[1] + c4[3]);
    }
    double tv[15], ta[15];  // tail loads first, then the dependent FMA chain
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        const int64_t row = a + n1 + i;
        const bool in = row < a + L;
        tv[i] = in ? bval(row) : 0.0;
        ta[i] = in ? A[row * ld + c] : 0.0;
    }
#pragma unroll
    for (int i = 0; i < 15; ++i)
        if (n1 + i < L) dot = __builtin_fma(tv[i], ta[i], dot);
    return dot;
}

// value of column c's dot product; call with the whole wave (lane = chunk)
__device__ __forceinline__ double ddot_finish_impl(const double *__restrict__ acc_c,
                                                   const int64_t *__restrict__ ca,
                                                   const int64_t *__restrict__ cl, int count,
                                                   int64_t ld, int64_t c,
                                                   const double *__restrict__ A,
                                                   const double *__restrict__ B,
                                                   const double *__restrict__ Bside) {
    const int lane = threadIdx.x & 63;
    double d = 0.0;
    if (lane < count) d = chunk_dot(acc_c + lane * 32, ca[lane], cl[lane], lane, ld, c, A, B, Bside);
    if (count == 1) return __shfl(d, 0);
    double total = 0.0;
    for (int t = 0; t < count; ++t) total = total + __shfl(d, t);
    return total;
}

// ---------------------------------------------------------------- the plan of one solve
// Which solver runs columns of an n-row system with lnnz entries of L_reg, ncols of them,
// and how; with every knob the solvers consult.  Mode:
//   0  short rows (default): q recomputed in k_cg_upd from the stored p (one gather per
//      entry is cheaper than 16 B/entry more of stream); only the q of the < 32
//      leftover rows per chunk is kept, for the finish
//   1  q stored by the fused p/q kernel (GSPARSE_CG_STOREQ=1 selects it)
//   2  split p stream + SpMV on the stored p (long rows: one gather per entry instead
//      of the fused kernel's two)
//   3  as 2 with the SpMV in column-block-major order (gathers served by the Infinity
//      Cache) and a separate dot(p,q) pass -- the default for long rows
//   4  resident solver (gs_cg_res.hip)
//   5  register-resident solver (gs_cg_reg.hip)
struct CgPlan {
    ChunkArg ch;
    int mode;
    int cpl;      // columns per lane of the chain kernels: 1, 2 (GSPARSE_CG_CPL)
    int ru;       // chain rows per trip of the fused kernels: 1, 2, 4, 8 (GSPARSE_CG_RU)
    bool storeq;  // q stored: every mode but 0
    // modes 4, 5
    int64_t slots;      // workgroups, each with one column in flight (GSPARSE_CG_SLOTS)
    bool slots_forced;  // ... as the variable says, not levelled over the rounds
    bool res_unit;      // GSPARSE_RES_UNIT=0: the weighted form even for unit weights
    bool res_dcount;    // GSPARSE_RES_DCOUNT=0: the diagonal loaded, not derived from the entry count
    bool res_prof;      // GSPARSE_RES_PROF: workgroup 0's phase clock, printed
    // mode 4
    bool res_ell;   // GSPARSE_RES_ELL=1: the ELL copy where every row has <= 16 entries
    bool res_stab;  // GSPARSE_RES_STAB=0: the SELL slice table read from global memory
    bool res_qlds;  // GSPARSE_RES_QLDS=0: no q mirror in LDS
    int res_rbw;    // GSPARSE_RES_RBW: 44, 27, 26, else 28; 0 (unset): from the slice widths
    // mode 5
    int reg_nt;              // GSPARSE_REG_NT=256: only the 256-thread form; else 512
    int64_t reg_keep;        // GSPARSE_REG_KEEP: most rows of a chunk whose p is in LDS
    int reg_split;           // GSPARSE_REG_SPLIT: 0 never, P >= 2 every column in P parts; -1 unset
    bool reg_split_auto;     // GSPARSE_REG_SPLIT_AUTO: two parts per tail column when they fit
    int32_t reg_split_spin;  // GSPARSE_REG_SPLIT_SPIN: a hand-off's wait budget; INT32_MIN unset
    int reg_window;          // GSPARSE_REG_WINDOW: 0 never, 3 / 4 that window wherever the kernel
                             // has one; -1 (unset): where it leaves fewer slow wave-slots
};

// Register-resident CG (mode 5, gs_cg_reg.hip): applies when the T BLAS chunks (lengths
// len[t]) fit its thread geometry; reg_nt = 256 leaves only its 256-thread form
bool cg_regres_applies(int64_t n, int T, const int64_t *len, int reg_nt);
bool cg_regres_wide(int64_t n, int T, const int64_t *len, int reg_nt);  // its 512-thread form applies

// ---------------------------------------------------------------- mode 5's LDS layout
// Pure host code (gs_er_reg_layout exposes it; tests/test_er_reg_layout_host.py pins it).
static constexpr int kRegLayoutChunks = 16;           // gs_cg_reg.hpp's kRegMaxChunks
static constexpr size_t kRegLdsBytes = 160 * 1024;    // LDS of a CU

// threads per chain for T chunks on an NT-thread workgroup (power of two, 32 T G <= NT,
// G <= 8) and register row slots per thread (the chain rows); -1 when it does not apply
inline int reg_geometry(int NT, int T, const int64_t *len, int &G) {
    if (T < 1 || 32 * T > NT) return -1;
    G = 1;
    while (G < 8 && 32 * T * (2 * G) <= NT) G *= 2;
    int64_t smax = 0;
    for (int t = 0; t < T; ++t) smax = std::max<int64_t>(smax, (len[t] & ~(int64_t)31) >> 5);
    return (int)((smax + G - 1) / G);
}

// workgroup size and slots: 512 threads (two waves per SIMD, k_cg_regwide) where the
// slots fit 44, else 256 threads (one wave per SIMD, 512 registers per lane,
// k_cg_regres) with up to 88.  reg_nt = 256 (the plan's, GSPARSE_REG_NT) forces the
// one-wave form.
inline bool reg_pick(int64_t n, int T, const int64_t *len, int reg_nt, int &NT, int &G, int &R) {
    if (n <= 0 || n >= 0x8000) return false;
    int g = 0;
    const bool narrow_only = reg_nt == 256;
    int r = narrow_only ? -1 : reg_geometry(512, T, len, g);
    if (r >= 0 && r <= 44) {
        NT = 512, G = g;
        R = r <= 16 ? 16 : r <= 24 ? 24 : r <= 32 ? 32 : 44;
        return true;
    }
    r = reg_geometry(256, T, len, g);
    if (r < 0 || r > 88) return false;
    NT = 256, G = g;
    R = r <= 24 ? 24 : r <= 48 ? 48 : r <= 64 ? 64 : 88;
    return true;
}

// Where p lives in a whole-column workgroup.  Chunk t keeps its first keep[t] rows (a
// multiple of 32 G unless the whole chunk fits or GSPARSE_REG_KEEP caps it) in LDS from
// slot lbase[t]; its other rows live in the workgroup's global slot.  After the prefixes:
// the zero slot (zslot) and a scratch slot, dsl diagonal slots, 6 x 32 T doubles of chain
// sums and tail rows, the chunk table.
// With a window (W > 0; two threads per chain, unit form) every chunk also owns W x 32 G
// slots from wbase[t], between the prefixes and the zero slot: a rotating read-only cache
// of the own p rows of the wave-slots around the one its wave works on (k_cg_regwide<WIN>).
struct RegLayout {
    int NT, G, R, T;
    int64_t keep[kRegLayoutChunks], lbase[kRegLayoutChunks];
    int64_t zslot;  // LDS slots of p (prefixes and windows)
    int dsl;        // diagonal slots
    size_t dyn;     // LDS bytes of the launch
    int W;          // window size in wave-slots, 0: none
    int64_t wbase[kRegLayoutChunks];
};

// ufast: the unit kernels that derive every diagonal from the entry count; reg_keep: the
// most rows of a chunk kept in LDS (GSPARSE_REG_KEEP); win: the window asked for (3 or 4
// wave-slots per chunk, reserved before the prefixes are apportioned; else none).  The
// window kernel streams every row past the prefix from the global slot, so a window is
// laid out only where it exists (512 threads, G == 2, unit) and every prefix is a whole
// number of wave-slots; otherwise L.W == 0 and the layout is the plain one.  False when
// mode 5 does not apply.
inline bool reg_layout(int64_t n, const ChunkArg &ch, int reg_nt, int64_t reg_keep, bool ufast,
                       RegLayout &L, int win = 0) {
    L = RegLayout{};
    const int T = ch.count;
    if (T > kRegLayoutChunks || !reg_pick(n, T, ch.len, reg_nt, L.NT, L.G, L.R)) return false;
    L.T = T;
    const int nch = 32 * T;
    L.dsl = L.NT == 256 ? 2 * L.NT : ufast ? L.NT : 0;
    const int64_t cap0 =
        (int64_t)((kRegLdsBytes - (6 * (size_t)nch + 2 * kRegLayoutChunks + 2 + L.dsl) * 8) / 8);
    int64_t tot = 0;
    for (int t = 0; t < T; ++t) tot += ch.len[t];
    const int64_t align = 32 * L.G;
    int W = ((win == 3 || win == 4) && L.NT == 512 && L.G == 2 && ufast) ? win : 0;
    if (cap0 < (int64_t)T * W * align) W = 0;
    for (;;) {
        const int64_t cap = cap0 - (int64_t)T * W * align;
        // prefixes in proportion to the chunk lengths, whole wave-slots (32 G rows) when
        // they cannot all fit
        for (int t = 0; t < T; ++t)
            L.keep[t] = tot <= cap ? ch.len[t] : (cap * ch.len[t] / tot) / align * align;
        if (tot > cap) {
            // the capacity the rounding left: one more wave-slot each for the chunks with the
            // most rows outside LDS (Roman, 8 chunks: 7 x 64 more rows in LDS)
            int64_t left = cap;
            for (int t = 0; t < T; ++t) left -= L.keep[t];
            while (left >= align) {
                int best = -1;
                for (int t = 0; t < T; ++t)
                    if (L.keep[t] + align <= ch.len[t] &&
                        (best < 0 || ch.len[t] - L.keep[t] > ch.len[best] - L.keep[best]))
                        best = t;
                if (best < 0) break;
                L.keep[best] += align;
                left -= align;
            }
        }
        for (int t = 0; t < T; ++t) L.keep[t] = std::min<int64_t>(L.keep[t], reg_keep);
        bool whole = true;
        for (int t = 0; t < T; ++t) whole = whole && L.keep[t] % align == 0;
        if (W == 0 || whole) break;
        W = 0;  // a prefix ends inside a wave-slot: the plain layout
    }
    int64_t zs = 0;
    for (int t = 0; t < T; ++t) {
        L.lbase[t] = zs;
        zs += L.keep[t];
    }
    L.W = W;
    for (int t = 0; t < T && W > 0; ++t) {
        L.wbase[t] = zs;  // a multiple of 32 G: every prefix is
        zs += W * align;
    }
    L.zslot = zs;
    L.dyn = sizeof(double) * ((size_t)zs + 2 + L.dsl + 6 * (size_t)nch + 2 * kRegLayoutChunks);
    return true;
}

// Pure host code.  The variables are read on every call: a process may change them
// between solves.
inline CgPlan cg_plan(int64_t n, int64_t lnnz, int64_t ncols, int32_t blas_threads) {
    CgPlan p{};
    // OpenBLAS caps its thread count at MAX_THREADS (64 in NumPy's build): a larger
    // request runs -- and orders the ddot sums -- as 64 threads
    if (blas_threads > kMaxChunks) blas_threads = kMaxChunks;
    p.ch = make_chunks(n, blas_threads);
    const ChunkArg &ch = p.ch;

    const char *e;
    p.res_unit = !(e = getenv("GSPARSE_RES_UNIT")) || atoi(e) != 0;
    p.res_dcount = !(e = getenv("GSPARSE_RES_DCOUNT")) || atoi(e) != 0;
    p.res_prof = getenv("GSPARSE_RES_PROF") != nullptr;
    p.res_ell = (e = getenv("GSPARSE_RES_ELL")) && atoi(e) != 0;
    p.res_stab = !(e = getenv("GSPARSE_RES_STAB")) || atoi(e) != 0;
    p.res_qlds = !(e = getenv("GSPARSE_RES_QLDS")) || atoi(e) != 0;
    p.res_rbw = 0;
    if ((e = getenv("GSPARSE_RES_RBW")))
        p.res_rbw = atoi(e) == 44 ? 44 : atoi(e) == 27 ? 27 : atoi(e) == 26 ? 26 : 28;
    p.reg_nt = ((e = getenv("GSPARSE_REG_NT")) && atoi(e) == 256) ? 256 : 512;
    p.reg_keep = (e = getenv("GSPARSE_REG_KEEP")) ? atoll(e) : INT64_MAX;
    p.reg_split = (e = getenv("GSPARSE_REG_SPLIT")) ? atoi(e) : -1;
    p.reg_split_auto = getenv("GSPARSE_REG_SPLIT_AUTO") != nullptr;
    p.reg_split_spin = (e = getenv("GSPARSE_REG_SPLIT_SPIN")) ? atoi(e) : INT32_MIN;
    p.reg_window = -1;
    if ((e = getenv("GSPARSE_REG_WINDOW"))) p.reg_window = atoi(e) == 3 ? 3 : atoi(e) == 4 ? 4 : 0;

    // two columns per lane (16-B accesses) unless that leaves too few waves
    const int64_t waves2 = ((ncols + 127) / 128) * 32 * (int64_t)ch.count;
    p.cpl = waves2 >= 4096 ? 2 : 1;
    if ((e = getenv("GSPARSE_CG_CPL"))) p.cpl = atoi(e) == 1 ? 1 : 2;
    const int64_t ncb = (int32_t)((ncols + 64 * p.cpl - 1) / (64 * p.cpl));  // column blocks

    // Short rows: recompute (0) while the chains give enough waves; fewer
    // columns (a rank's share on N GPUs) -> stored q (1), then the split
    // kernels (3); measured on Roman at k/1, k/2, k/4, k/8 columns.
    // Resident solver (4) where its 256 columns in flight fit the Infinity Cache
    // (4 vectors x 8 B x n x 256 <= ~200 MB) and the BLAS chunks give >= 128 chains:
    // Roman size, 2,674 columns: 0.51 s vs 0.53 s for mode 0; k/8 columns ~0.09 s vs 0.12 s.
    const bool resident = n > 10000 && n <= 24576 && ch.count >= 4 && lnnz <= kStoreQRowLen * n;
    // register-resident solver (5) where its 512-thread form applies (Roman size:
    // 55.7 vs 76.4 us per column-iteration for mode 4); its
    // 256-thread form (more rows per thread) is no faster than mode 4: opt-in
    const bool regres = cg_regres_applies(n, ch.count, ch.len, p.reg_nt);
    const bool regwide = cg_regres_wide(n, ch.count, ch.len, p.reg_nt);
    p.mode = resident && regwide                   ? 5
             : resident                            ? 4
             : (n > 0 && lnnz > kStoreQRowLen * n) ? 3
             : ncols >= 2048                       ? 0
             : ncols >= 512                        ? 1
                                                   : 3;
    if ((e = getenv("GSPARSE_CG_MODE"))) {
        const int v = atoi(e);
        p.mode = (v >= 0 && v <= 5) ? v : 0;
        if (p.mode == 5 && !regres) p.mode = 4;
    }
    if ((e = getenv("GSPARSE_CG_STOREQ"))) p.mode = atoi(e) != 0 ? 1 : 0;
    p.storeq = p.mode != 0;

    // chain rows per trip in the fused kernels (loads of all of them in flight)
    // (fewer waves -> more rows per trip; measured on Roman at k/1 .. k/8 columns)
    const int64_t cg_waves = ncb * ch.count * 32;
    p.ru = cg_waves >= 4096 ? 1 : cg_waves >= 2048 ? 2 : 4;
    if ((e = getenv("GSPARSE_CG_RU"))) {
        const int v = atoi(e);
        p.ru = (v == 1 || v == 2 || v == 4 || v == 8) ? v : p.ru;
    }

    // resident solvers: one workgroup per CU, whole columns per workgroup
    p.slots = 256;
    p.slots_forced = (e = getenv("GSPARSE_CG_SLOTS")) != nullptr;
    if (e) p.slots = atoi(e) > 0 ? atoi(e) : p.slots;
    if (p.slots > ncols) p.slots = ncols;
    // as few workgroups as the round count allows (every workgroup then owns the
    // same number of columns, and fewer CUs share the Infinity Cache in each round)
    if (p.slots > 0 && !p.slots_forced) {
        const int64_t rounds = (ncols + p.slots - 1) / p.slots;
        p.slots = (ncols + rounds - 1) / rounds;
    }
    return p;
}

// ---------------------------------------------------------------- the solvers
// Each solves columns [col0, col1) of the prepared and projected state c->er, which
// gs_er_solve has checked, on c->stream: x into er.X, the iteration counts into the
// column state (col_ptrs).  gs_er_solve copies the counts out and waits.
void cg_solve_streamed(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                       double rtol);  // modes 0-3, gs_cg_stream.hip
void cg_solve_resident(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                       double rtol);  // mode 4, gs_cg_res.hip
void cg_regres_solve(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                     double rtol);  // mode 5, gs_cg_reg.hip

// What the resident solvers share (gs_cg_res.hip): x of the solve's columns in
// column-major form, and what they need to know about L_reg's weights
struct ResCommon {
    int64_t ldn;           // column stride of Xc: n rounded up to 8
    double *Xc;            // column col0 + i at Xc + i * ldn
    const double *sdiag;   // [n] L_reg_ii (0.0 where the diagonal entry was dropped)
    const int32_t *swid;   // SELL-16 slices of L_reg (mode 4): width (longest row) of each,
    const int64_t *soff;   // its entry offset,
    int64_t nbk;           // their number
    int32_t unit, dcount;  // unit-weight form / every L_reg_ii == entries - 1 + 1e-6 (after the knobs)
    long long *prof;       // plan.res_prof: where workgroup 0 leaves its phase clock
};
ResCommon res_begin(gs_ctx *c, const CgPlan &plan, int64_t ncols);
// after the launch, profiled from t0 as `name`: x back to er.X's row-major columns,
// the profile entry's bytes (per executed iteration, summed on the device)
void res_end(gs_ctx *c, const ResCommon &rc, hipEvent_t t0, const char *name, int64_t col0,
             int64_t ncols);

}  // namespace gs
