// gs_cg_reg.hip -- host side of the register-resident CG (ApproxER mode 5): the
// ELL-8 copy of L_reg with p codes, the LDS plan, geometry and launch.  The kernel
// and its design notes are in gs_cg_reg.hpp.
#include "gs_cg.hpp"
#include "gs_cg_reg.hpp"

#ifndef GS_CG_XG
#define GS_CG_XG 0
#endif

namespace gs {

// ELL-8 copy of L_reg: overflow entry counts (rows longer than 8)
__global__ void k_ell8_count(int32_t n, const int64_t *__restrict__ lp, int64_t *__restrict__ cnt,
                             uint16_t *__restrict__ rlen) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t len = lp[i + 1] - lp[i];
        cnt[i] = len > 8 ? len - 8 : 0;
        rlen[i] = (uint16_t)len;
    }
}

// p code of column c: its LDS slot when c is in its chunk's LDS-resident prefix,
// else 0x8000 | c (chunk table: starts, lengths, prefixes, LDS bases).  A split part's
// table holds only its own chunks: columns outside them are global (other parts' rows)
// Window (W > 0: two threads per chain, wave-slots of 64 rows, every prefix a whole number
// of them; the table's fifth row holds the window bases): an entry of row i that names a
// chain row c past the prefix of i's own chunk, at most one wave-slot from i's, with i a
// chain row too, gets the LDS slot where the chunk's wave keeps c's p while it works on
// i's slot -- position (slot(c) - prefix slots) mod W of the window, offset c's in its
// wave-slot (k_cg_regwide<WIN>).  nwin counts these codes.
__device__ __forceinline__ uint32_t p_code(int32_t c, int32_t i, int T, const int64_t *__restrict__ tab,
                                           int W, int &nwin) {
    if (c < tab[0] || c >= tab[T - 1] + tab[kRegMaxChunks + T - 1]) return 0x8000u | (uint32_t)c;
    int t = 0;
    while (t + 1 < T && c >= tab[t + 1]) ++t;
    const int64_t o = c - tab[t], keep = tab[2 * kRegMaxChunks + t];
    if (o < keep) return (uint32_t)(tab[3 * kRegMaxChunks + t] + o);
    if (W > 0) {
        const int64_t oi = (int64_t)i - tab[t], n32 = tab[kRegMaxChunks + t] & ~(int64_t)31;
        if (oi >= 0 && oi < n32 && o < n32) {
            const int64_t sc = o >> 6, si = oi >> 6;
            if (sc - si <= 1 && si - sc <= 1) {
                ++nwin;
                return (uint32_t)(tab[4 * kRegMaxChunks + t] + ((sc - (keep >> 6)) % W) * 64 + (o & 63));
            }
        }
    }
    return 0x8000u | (uint32_t)c;
}

// diagonal slot index of row c: 2 tid + parity in k_cg_regres (dmul 2), tid in
// k_cg_regwide (dmul 1), G threads per chain:
// chain row s of chain (t, j) is slot s / G of thread g = s % G; a chunk's tail rows
// belong to g = 0 with parity 0
__device__ __forceinline__ int row_dslot(int32_t c, int T, const int64_t *__restrict__ tab, int G,
                                         int dmul, int32_t d0 = 0) {
    int t = 0;
    while (t + 1 < T && c >= tab[t + 1]) ++t;
    const int o = (int)(c - tab[t]), n32 = (int)(tab[kRegMaxChunks + t] & ~(int64_t)31);
    const bool in = o < n32;
    const int j = in ? (o & 31) : o - n32, g = in ? (o >> 5) % G : 0;
    const int par = in ? ((o >> 5) / G) & 1 : 0;
    const int chain = t * 32 + j, CW = 64 / G;
    const int tid = (chain / CW) * 64 + (chain % CW) + CW * g;
    if (dmul == 3) {  // k_cg_regwide's V2 two-per-chain layout (DBANK): bank of own p + 1
        const int lb = (int)tab[3 * kRegMaxChunks + t];
        const int s0 = d0 + (tid & ~31);
        return (tid & ~31) + ((lb + (tid & 31) + 1 - s0) & 31);
    }
    return dmul == 2 ? 2 * tid + par : tid;
}

// dslot0 >= 0 (unit form): the diagonal entry's code is the owner thread's diagonal
// slot dslot0 + tid instead of the row's p code
__global__ void k_ell8_fill(int32_t r0, int32_t n, int T, const int64_t *__restrict__ tab, uint32_t pad,
                            int G, int dmul, int32_t dslot0, const int64_t *__restrict__ lp,
                            const int32_t *__restrict__ li, const double *__restrict__ lv,
                            const int64_t *__restrict__ optr, uint4 *__restrict__ ell,
                            double *__restrict__ ellv, uint16_t *__restrict__ ocol,
                            double *__restrict__ oval, uint8_t *__restrict__ rflag, int W,
                            unsigned long long *__restrict__ wcount) {
    for (int64_t i = r0 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e0 = lp[i], len = lp[i + 1] - e0;
        const uint32_t dcode = dslot0 >= 0 ? (uint32_t)(dslot0 + row_dslot((int32_t)i, T, tab, G, dmul, dslot0)) : 0u;
        int nwin = 0;
        auto code = [&](int64_t e) -> uint32_t {
            return (dslot0 >= 0 && li[e] == i) ? dcode : p_code(li[e], (int32_t)i, T, tab, W, nwin);
        };
        uint32_t w[4] = {0, 0, 0, 0};
        bool glob = false;
        for (int k = 0; k < 8; ++k) {
            const uint32_t cc = k < len ? code(e0 + k) : pad;
            glob = glob || (cc & 0x8000u) != 0;
            w[k >> 1] |= cc << (16 * (k & 1));
            if (ellv) ellv[i * 8 + k] = k < len ? lv[e0 + k] : 0.0;
        }
        ell[i] = make_uint4(w[0], w[1], w[2], w[3]);
        if (rflag) rflag[i] = (uint8_t)((glob ? 1 : 0) | (len > 8 ? 2 : 0));
        for (int64_t k = 8; k < len; ++k) {
            ocol[optr[i] + k - 8] = (uint16_t)code(e0 + k);
            if (oval) oval[optr[i] + k - 8] = lv[e0 + k];
        }
        if (wcount && nwin) atomicAdd(wcount, (unsigned long long)nwin);
    }
}

// wave-slots (64 consecutive chain rows of a chunk, two threads per chain) with a global p
// code among their rows' first 8 entries: the slots whose gathers k_cg_regwide's V2 form
// fixes up from the global slot (its gmask)
__global__ void k_reg_slow_slots(int T, const int64_t *__restrict__ tab, const uint8_t *__restrict__ rflag,
                                 unsigned long long *__restrict__ out) {
    const int t = blockIdx.x;
    if (t >= T) return;
    const int64_t a = tab[t], n32 = tab[kRegMaxChunks + t] & ~(int64_t)31;
    for (int64_t u = threadIdx.x; u * 64 < n32; u += blockDim.x) {
        bool any = false;
        for (int64_t o = u * 64; o < n32 && o < u * 64 + 64; ++o) any = any || (rflag[a + o] & 1);
        if (any) atomicAdd(out, 1ull);
    }
}

static_assert(kRegLayoutChunks == kRegMaxChunks, "reg_layout sizes its tables for kRegMaxChunks");

bool cg_regres_applies(int64_t n, int T, const int64_t *len, int reg_nt) {
    int NT, G, R;
    return reg_pick(n, T, len, reg_nt, NT, G, R);
}

bool cg_regres_wide(int64_t n, int T, const int64_t *len, int reg_nt) {
    int NT = 0, G, R;
    return reg_pick(n, T, len, reg_nt, NT, G, R) && NT == 512;
}

// columns [col0, col0 + ncols) of L_reg (CSR lp/li/lv, n > 0 rows) into Xc (column-major,
// ldn per column), the iterations each ran into iters
static void regres_run(gs_ctx *c, const CgPlan &plan, int64_t n, const int64_t *lp, const int32_t *li,
                       const double *lv, int unit, int dcount, const double *diag, const double *Rr,
                       int64_t ld, int64_t col0, int64_t ncols, int32_t maxiter, double rtol,
                       double *Xc, int64_t ldn, int32_t *iters, long long *prof) {
    hipStream_t s = c->stream;
    const int T = plan.ch.count;
    const int64_t *ha = plan.ch.a, *hlen = plan.ch.len;
    const int64_t slots = plan.slots;
    const bool ufast = unit && dcount;  // the unit kernels derive every diagonal from the entry count
    // LDS: p (each chunk's LDS-resident prefix, in chunk order; with a window, the chunks'
    // windows), the zero and scratch slots, the diagonal slots, 6 x 32 T doubles of chain
    // sums / tail rows, the chunk table (reg_layout, gs_cg.hpp)
    RegLayout lay0, layw;
    GS_CHECK(reg_layout(n, plan.ch, plan.reg_nt, plan.reg_keep, ufast, lay0), GS_EUNSUPPORTED,
             "register-resident CG: n=%lld, %d chunks out of range", (long long)n, T);
    const int NT = lay0.NT, G = lay0.G, rsel = lay0.R;
    // The p window (GSPARSE_REG_WINDOW; the whole-column unit kernel with two threads per
    // chain only): unset, the default window is weighed against the plain layout when the
    // ELL copy is rebuilt and used only if it leaves strictly fewer wave-slots with a global
    // p code -- the count is the cost a window removes, and a graph without band locality
    // keeps the plain layout and kernel; 3 / 4: that window wherever the kernel has one.
    const int wask = !kRegWindowBuilt ? 0 : plan.reg_window < 0 ? kRegWindowDefault : plan.reg_window;
    const bool have_w = wask > 0 && reg_layout(n, plan.ch, plan.reg_nt, plan.reg_keep, ufast, layw, wask) &&
                        layw.W > 0;
    // (512 threads, two per chain, unit: the diagonal slots bank-permuted -- the same
    // condition as k_cg_regwide's DBANK = GS_CG_V2 && UNIT && G == 2, so an A/B build with
    // -DGS_CG_V2=0 codes the diagonal where its kernel reads it)
    const bool dbank = GS_CG_V2 && NT == 512 && G == 2 && ufast;
    const int dsl = lay0.dsl;
    const size_t lds_max = kRegLdsBytes;
    // ELL-8 copy (uint16 p codes), overflow entries in CSR form: rebuilt only when the
    // graph, L_reg's shift, the chunk / LDS layout or the window asked for changed (the key)
    double regv = c->er.reg;
    int64_t regbits;
    memcpy(&regbits, &regv, sizeof(regbits));
    std::vector<int64_t> key = {c->g.epoch, regbits, n, T, G, NT, ufast ? 1 : 0, unit, dcount, dbank ? 1 : 0,
                                have_w ? layw.W : 0, plan.reg_window};
    for (int t = 0; t < T; ++t) key.insert(key.end(), {ha[t], hlen[t], lay0.keep[t]});
    auto *ocnt = (int64_t *)c->buf("er_reg_ocnt").ensure(sizeof(int64_t) * (n + 1));
    auto *optr = (int64_t *)c->buf("er_reg_optr").ensure(sizeof(int64_t) * (n + 1));
    auto *rlen = (uint16_t *)c->buf("er_reg_rlen").ensure(sizeof(uint16_t) * n);
    const bool fresh = key != c->reg_ell_key;
    if (fresh) {
        c->reg_ell_key.clear();
        c->reg_split_key.clear();
        GS_HIP(hipMemsetAsync(ocnt, 0, sizeof(int64_t) * (n + 1), s));
        k_ell8_count<<<grid_for(n, 256, 8192), 256, 0, s>>>((int32_t)n, lp, ocnt, rlen);
        exclusive_scan_i64(c, ocnt, optr, n + 1);
        GS_HIP(hipMemcpyAsync(&c->reg_nov, optr + n, sizeof(int64_t), hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
    }
    const int64_t nov = c->reg_nov;
    // chunk table: starts, lengths, prefixes, LDS bases, window bases
    constexpr size_t kTabBytes = sizeof(int64_t) * 5 * kRegMaxChunks;
    auto *dch = (int64_t *)c->buf("er_reg_chunks").ensure(kTabBytes);
    auto upload = [&](const RegLayout &L, std::vector<int64_t> &host, int64_t *dev) {
        host.assign(5 * kRegMaxChunks, 0);
        for (int t = 0; t < T; ++t) {
            host[t] = ha[t];
            host[kRegMaxChunks + t] = hlen[t];
            host[2 * kRegMaxChunks + t] = L.keep[t];
            host[3 * kRegMaxChunks + t] = L.lbase[t];
            host[4 * kRegMaxChunks + t] = L.wbase[t];
        }
        // stream-ordered; the host table lives in the context until the next solve
        GS_HIP(hipMemcpyAsync(dev, host.data(), kTabBytes, hipMemcpyHostToDevice, s));
    };
    auto *ell = (uint4 *)c->buf("er_reg_ell").ensure(sizeof(uint4) * n);
    auto *rflag = (uint8_t *)c->buf("er_reg_rflag").ensure((size_t)n + 64);
    double *ellv = ufast ? nullptr : (double *)c->buf("er_reg_ellv").ensure(sizeof(double) * 8 * n);
    auto *ocol = (uint16_t *)c->buf("er_reg_ocol").ensure(sizeof(uint16_t) * (nov + 1));
    double *oval = ufast ? nullptr : (double *)c->buf("er_reg_oval").ensure(sizeof(double) * (nov + 1));
    auto fill = [&](const RegLayout &L, const int64_t *dev, unsigned long long *wcount) {
        k_ell8_fill<<<grid_for(n, 256, 8192), 256, 0, s>>>(0, (int32_t)n, T, dev, (uint32_t)L.zslot, G,
                                                          NT == 256 ? 2 : dbank ? 3 : 1,
                                                          ufast ? (int32_t)L.zslot + 2 : -1,
                                                          lp, li, lv, optr, ell, ellv, ocol, oval, rflag, L.W,
                                                          wcount);
        GS_HIP(hipGetLastError());
    };
    if (fresh && have_w) {
        // both layouts' ELL copies in turn: the wave-slots with a global p code under each,
        // the window codes; one wait, once per graph, beside the rebuild's own
        auto *dch2 = (int64_t *)c->buf("er_reg_chunks2").ensure(kTabBytes);
        auto *dcnt = (unsigned long long *)c->buf("er_reg_wcnt").ensure(sizeof(unsigned long long) * 3);
        unsigned long long hcnt[3] = {0, 0, 0};
        GS_HIP(hipMemsetAsync(dcnt, 0, sizeof(hcnt), s));
        upload(lay0, c->reg_hch2, dch2);
        fill(lay0, dch2, nullptr);
        k_reg_slow_slots<<<T, 64, 0, s>>>(T, dch2, rflag, dcnt);
        upload(layw, c->reg_hch, dch);
        fill(layw, dch, dcnt + 2);
        k_reg_slow_slots<<<T, 64, 0, s>>>(T, dch, rflag, dcnt + 1);
        GS_HIP(hipGetLastError());
        GS_HIP(hipMemcpyAsync(hcnt, dcnt, sizeof(hcnt), hipMemcpyDeviceToHost, s));
        GS_HIP(hipStreamSynchronize(s));
        const bool use_w = plan.reg_window > 0 || hcnt[1] < hcnt[0];
        c->reg_win[0] = use_w ? layw.W : 0;
        c->reg_win[1] = (int64_t)hcnt[0];
        c->reg_win[2] = (int64_t)hcnt[1];
        c->reg_win[3] = use_w ? (int64_t)hcnt[2] : 0;
        if (!use_w) {
            upload(lay0, c->reg_hch, dch);
            fill(lay0, dch, nullptr);
        }
        c->reg_ell_key = key;
    } else if (fresh) {
        c->reg_win[0] = 0, c->reg_win[1] = c->reg_win[2] = -1, c->reg_win[3] = 0;
        upload(lay0, c->reg_hch, dch);
        fill(lay0, dch, nullptr);
        c->reg_ell_key = key;
    }
    const RegLayout &lay = (have_w && c->reg_win[0] > 0) ? layw : lay0;
    if (!fresh) upload(lay, c->reg_hch, dch);
    const uint32_t pad = (uint32_t)lay.zslot;  // the zero slot
    const size_t dyn = lay.dyn;
    RegArgs A{};
    // 512-thread form, whole columns: x in registers, q recomputed in the r update
    // (GSPARSE_REG_QR=1: q kept in registers from the SpMV pass, x read-modify-written
    // in Xc every iteration -- ~6x the fabric traffic for a wash in time).
    // The split form always keeps q in registers (its x lives in Xc).
    // (round 3 measured the whole-column q-in-registers form -- x read-modify-written in
    // Xc every iteration -- at parity with x in registers and 6x the fabric traffic; it
    // is no longer built, GSPARSE_REG_QR is ignored)
    A.qreg = 0;
    // Split plan: the last round of columns, when it leaves at least half the CUs idle,
    // runs as groups of P workgroups per column (k_cg_regwide<..., SPLIT>), each part a
    // contiguous range of the BLAS chunks with all its rows' p in LDS.
    // GSPARSE_REG_SPLIT=0: never; =P (>= 2): every column in P parts (tests);
    // GSPARSE_REG_SPLIT_AUTO=1: the round-5 rule, two parts per tail column when they fit.
    int ncu = 256;
    GS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device));
    int P = 0;
    int64_t W = ncols;  // columns solved whole (the first W), the rest split
    split_abort_poll(c, false);
    if (c->reg_split_off && c->reg_split_off_epoch != c->g.epoch) c->reg_split_off = false;  // new graph
    if (NT == 512 && T >= 2 && ncols > 0 && !c->reg_split_off) {
        const int forced = plan.reg_split;
        if (forced >= 2) {
            P = std::min(forced, T);
            W = 0;
        } else if (forced < 0 && !plan.slots_forced && plan.reg_split_auto) {
            // (round 6: off by default.  With one SpMV per iteration a whole column-iteration
            // takes ~31 us, and the last round solved whole inside the same launch -- each CU
            // starts its tail column as soon as its own columns are done -- matches or beats
            // the two-part split launch at every rank share: Roman 334 / 669 / 1,337 / 2,674
            // columns 28.6 / 44.0 / 88.1 / 164.2 ms whole vs 29.8 / 44.0 / 90.6 / 164.9 ms
            // split; profiles/r06_cg_ab/rankcols_*.  Round 3, at 44 us: 78 tail columns in 2
            // / 3 / 4 parts 13.9 / 14.5 / 30.2 ms, whole 21.8 ms.)
            const int64_t rounds = (ncols + ncu - 1) / ncu;
            const int64_t tailc = ncols - (rounds - 1) * ncu;
            if (2 * tailc <= ncu) {
                P = 2;
                W = (rounds - 1) * ncu;
            }
        }
    }
    // parts: chunk ranges as equal as possible; one geometry (G, R) for all of them
    int pc0[kRegMaxChunks + 1] = {}, Gs = 0, Rs = 0;
    size_t dyns = 0;
    if (P >= 2) {
        int tmax = 0;
        for (int h = 0, at = 0; h < P; ++h) {
            pc0[h] = at;
            at += T / P + (h < T % P ? 1 : 0);
            tmax = std::max(tmax, at - pc0[h]);
        }
        pc0[P] = T;
        int64_t plen[kRegMaxChunks];
        for (int t = 0; t < tmax; ++t) plen[t] = 0;
        for (int h = 0; h < P; ++h)
            for (int t = pc0[h]; t < pc0[h + 1]; ++t)
                plen[t - pc0[h]] = std::max<int64_t>(plen[t - pc0[h]], hlen[t]);
        const int rr = reg_geometry(512, tmax, plen, Gs);
        Rs = rr < 0 ? -1 : rr <= 16 ? 16 : rr <= 24 ? 24 : rr <= 32 ? 32 : rr <= 44 ? 44 : -1;
        for (int h = 0; h < P; ++h) {
            int64_t rows = 0;
            for (int t = pc0[h]; t < pc0[h + 1]; ++t) rows += hlen[t];
            const int th = pc0[h + 1] - pc0[h];
            dyns = std::max(dyns, sizeof(double) * ((size_t)rows + 2 + dsl + 6 * 32 * (size_t)th +
                                                    2 * kRegMaxChunks + 1));
        }
        if (Rs < 0 || Gs < 4 || dyns > lds_max) {  // does not fit: solve every column whole
            P = 0;
            W = ncols;
        }
    }
    const int64_t wslots = P ? std::min<int64_t>(ncu, std::max<int64_t>(W, 1)) : slots;
    // (-DGS_CG_XG: the second half holds each whole-column workgroup's q scratch)
    double *pg = (double *)c->buf("er_reg_pg").ensure(sizeof(double) * (GS_CG_XG ? 2 : 1) *
                                                      (size_t)std::max<int64_t>(std::max<int64_t>(wslots, slots), 1) * ldn);
    A.ld = ld;
    A.ldn = ldn;
    A.col0 = col0;
    A.ncols = W;
    A.n = (int32_t)n;
    A.Rr = Rr;
    A.Xc = Xc;
    A.pg = pg;
    A.ell = ell;
    A.ellv = ellv;
    A.optr = optr;
    A.rlen = rlen;
    A.ocol = ocol;
    A.oval = oval;
    A.diag = diag;  // L_reg's diagonal (k_l_unit), read by the whole-column unit form
    A.rflag = rflag;

    A.zslot = (int32_t)pad;
    A.maxiter = maxiter;
    A.rtol = rtol;
    A.iters = iters;
    A.T = T;
    A.ca = dch;
    A.cl = dch + kRegMaxChunks;
    A.ck = dch + 2 * kRegMaxChunks;
    A.cb = dch + 3 * kRegMaxChunks;
    A.cw = dch + 4 * kRegMaxChunks;
    A.W = lay.W;
    A.prof = prof;
    // the whole-column launch (the first W columns); with a split tail it is issued
    // after the tail's tables and ELL are prepared, so the split launch follows it at once
    auto launch_whole = [&]() {
        if (W <= 0) return;
        if (NT == 512) {
            if (G == 1) regwide_launch_g1(A, rsel, ufast, dyn, (unsigned)wslots, s);
            else if (G == 2) regwide_launch_g2(A, rsel, ufast, dyn, (unsigned)wslots, s);
            else if (G == 4) regwide_launch_g4(A, rsel, ufast, dyn, (unsigned)wslots, s);
            else regwide_launch_g8(A, rsel, ufast, dyn, (unsigned)wslots, s);
        } else if (G == 1) regres_launch_g1(A, rsel, ufast, dyn, (unsigned)wslots, s);
        else if (G == 2) regres_launch_g2(A, rsel, ufast, dyn, (unsigned)wslots, s);
        else if (G == 4) regres_launch_g4(A, rsel, ufast, dyn, (unsigned)wslots, s);
        else regres_launch_g8(A, rsel, ufast, dyn, (unsigned)wslots, s);
        GS_HIP(hipGetLastError());
    };
    if (P < 2) {
        launch_whole();
        return;
    }

    // split tail: per-part chunk tables (LDS layout: the part's rows from slot 0, then
    // the zero slot) and an ELL whose codes each row's part resolves
    const int64_t tailn = ncols - W;
    const int64_t groups = std::min<int64_t>(tailn, ncu / P);
    int32_t hpt[kRegMaxChunks * kRegPartTab] = {};
    int64_t htab[kRegMaxChunks][4 * kRegMaxChunks] = {};
    for (int h = 0; h < P; ++h) {
        int32_t *pt = hpt + h * kRegPartTab;
        int64_t zsh = 0;
        for (int t = pc0[h]; t < pc0[h + 1]; ++t) {
            const int tl = t - pc0[h];
            pt[tl] = (int32_t)ha[t];
            pt[kRegMaxChunks + tl] = (int32_t)hlen[t];
            pt[2 * kRegMaxChunks + tl] = (int32_t)hlen[t];
            pt[3 * kRegMaxChunks + tl] = (int32_t)zsh;
            htab[h][tl] = ha[t];
            htab[h][kRegMaxChunks + tl] = hlen[t];
            htab[h][2 * kRegMaxChunks + tl] = hlen[t];
            htab[h][3 * kRegMaxChunks + tl] = zsh;
            zsh += hlen[t];
        }
        pt[4 * kRegMaxChunks] = pc0[h + 1] - pc0[h];
        pt[4 * kRegMaxChunks + 1] = (int32_t)zsh;
        pt[4 * kRegMaxChunks + 2] = pc0[h];
    }
    auto *dpt = (int32_t *)c->buf("er_reg_split_ptab").ensure(sizeof(hpt));
    auto *dtab = (int64_t *)c->buf("er_reg_split_tab").ensure(sizeof(htab));
    // stream-ordered copies from host tables the context keeps (they outlive the copies:
    // nothing below waits for the stream)
    c->reg_split_hpt.assign(hpt, hpt + sizeof(hpt) / sizeof(hpt[0]));
    c->reg_split_htab.assign(&htab[0][0], &htab[0][0] + sizeof(htab) / sizeof(int64_t));
    GS_HIP(hipMemcpyAsync(dpt, c->reg_split_hpt.data(), sizeof(hpt), hipMemcpyHostToDevice, s));
    GS_HIP(hipMemcpyAsync(dtab, c->reg_split_htab.data(), sizeof(htab), hipMemcpyHostToDevice, s));
    auto *ells = (uint4 *)c->buf("er_reg_split_ell").ensure(sizeof(uint4) * n);
    double *ellvs = ufast ? nullptr : (double *)c->buf("er_reg_split_ellv").ensure(sizeof(double) * 8 * n);
    auto *ocols = (uint16_t *)c->buf("er_reg_split_ocol").ensure(sizeof(uint16_t) * (nov + 1));
    double *ovals = ufast ? nullptr : (double *)c->buf("er_reg_split_oval").ensure(sizeof(double) * (nov + 1));
    std::vector<int64_t> skey = {P, Gs};
    skey.insert(skey.end(), pc0, pc0 + P + 1);
    const bool sfresh = skey != c->reg_split_key;
    for (int h = 0; h < P && sfresh; ++h) {
        const int32_t r0 = (int32_t)ha[pc0[h]];
        const int32_t r1 = (int32_t)(ha[pc0[h + 1] - 1] + hlen[pc0[h + 1] - 1]);
        const int32_t zsh = hpt[h * kRegPartTab + 4 * kRegMaxChunks + 1];
        k_ell8_fill<<<grid_for(r1 - r0, 256, 8192), 256, 0, s>>>(
            r0, r1, pc0[h + 1] - pc0[h], dtab + h * 4 * kRegMaxChunks, (uint32_t)zsh, Gs, 1,
            ufast ? zsh + 2 : -1, lp, li, lv, optr, ells, ellvs, ocols, ovals, nullptr, 0, nullptr);
        GS_HIP(hipGetLastError());
    }
    c->reg_split_key = skey;
    double *pgs = (double *)c->buf("er_reg_split_pg").ensure(sizeof(double) * (size_t)groups * 2 * ldn);
    double *xch = (double *)c->buf("er_reg_split_xch").ensure(sizeof(double) * (size_t)groups * 2 * kRegMaxChunks);
    auto *flg = (int32_t *)c->buf("er_reg_split_flags").ensure(sizeof(int32_t) * ((size_t)groups * P + 1));
    GS_HIP(hipMemsetAsync(flg, 0, sizeof(int32_t) * ((size_t)groups * P + 1), s));
    RegArgs B = A;
    B.col0 = col0 + W;
    B.ncols = tailn;
    B.Xc = Xc + W * ldn;
    B.pg = pgs;
    B.ell = ells;
    B.ellv = ellvs;
    B.ocol = ocols;
    B.oval = ovals;
    B.prof = nullptr;
    B.P = P;
    B.ptab = dpt;
    B.xch = xch;
    B.flags = flg;
    B.abortf = flg + (size_t)groups * P;
    // a hand-off waits at most 20 ms (a column-iteration of a split column takes
    // ~30 us; a part that is not resident never arrives)
    int wclk_khz = 100000;
    GS_HIP(hipDeviceGetAttribute(&wclk_khz, hipDeviceAttributeWallClockRate, c->device));
    B.spinmax = 20 * std::max(wclk_khz, 1);
    if (plan.reg_split_spin != INT32_MIN) B.spinmax = plan.reg_split_spin;
    const unsigned grid = (unsigned)(groups * P);
    launch_whole();
    if (Gs == 4) regwide_split_launch_g4(B, Rs, ufast, dyns, grid, s);
    else regwide_split_launch_g8(B, Rs, ufast, dyns, grid, s);
    GS_HIP(hipGetLastError());
    // If the parts of a column could not all be resident at once (another process or
    // stream held CUs), the hand-offs gave up and set the abort word: the tail columns
    // are then solved again, whole, one workgroup each -- by a launch gated on that
    // word on the device (it exits at once when the split form completed), so no host
    // round trip.  The host reads the word later, without waiting (split_abort_poll),
    // counts the abort and keeps the split form off for this graph.
    RegArgs Cw = A;
    Cw.col0 = col0 + W;
    Cw.ncols = tailn;
    Cw.Xc = Xc + W * ldn;
    Cw.prof = nullptr;
    Cw.gate = B.abortf;
    const int64_t ts = std::min<int64_t>(tailn, wslots > 1 ? wslots : slots);
    if (G == 1) regwide_launch_g1(Cw, rsel, ufast, dyn, (unsigned)ts, s);
    else if (G == 2) regwide_launch_g2(Cw, rsel, ufast, dyn, (unsigned)ts, s);
    else if (G == 4) regwide_launch_g4(Cw, rsel, ufast, dyn, (unsigned)ts, s);
    else regwide_launch_g8(Cw, rsel, ufast, dyn, (unsigned)ts, s);
    GS_HIP(hipGetLastError());
    if (!c->split_abort_host) {
        GS_HIP(hipHostMalloc((void **)&c->split_abort_host, sizeof(int32_t), hipHostMallocDefault));
        GS_HIP(hipEventCreateWithFlags(&c->split_abort_ev, hipEventDisableTiming));
    }
    // the previous split launch's word must be read before its pinned slot is reused
    // (ADVICE r04): the copy may still be pending when a new launch is queued
    if (c->split_abort_pending) split_abort_poll(c, true);
    *c->split_abort_host = 0;
    GS_HIP(hipMemcpyAsync(c->split_abort_host, B.abortf, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    GS_HIP(hipEventRecord(c->split_abort_ev, s));
    c->split_abort_pending = true;
    c->split_abort_parts = P;
}

void cg_regres_solve(gs_ctx *c, const CgPlan &plan, int64_t col0, int64_t col1, int32_t maxiter,
                     double rtol) {
    ErState &er = c->er;
    const int64_t ncols = col1 - col0;
    int32_t *iters = col_ptrs(er).iters;
    const ResCommon rc = res_begin(c, plan, ncols);
    GS_HIP(hipMemsetAsync(iters + col0, 0, sizeof(int32_t) * ncols, c->stream));
    hipEvent_t t0 = prof_begin(c);
    if (er.n)
        regres_run(c, plan, er.n, er.lp.as<int64_t>(), er.li.as<int32_t>(), er.lv.as<double>(),
                   rc.unit, rc.dcount, rc.sdiag, er.Rr.as<double>(), er.ld, col0, ncols, maxiter, rtol,
                   rc.Xc, rc.ldn, iters, rc.prof);
    res_end(c, rc, t0, "cg_reg", col0, ncols);
}

// The abort word of the last split launch, once its copy has landed (never waits unless
// `wait`): an abort turns the split form off for the graph it happened on.
void split_abort_poll(gs_ctx *c, bool wait) {
    if (!c->split_abort_pending) return;
    if (!wait && hipEventQuery(c->split_abort_ev) != hipSuccess) return;
    if (wait) GS_HIP(hipEventSynchronize(c->split_abort_ev));
    c->split_abort_pending = false;
    if (*c->split_abort_host) {
        c->reg_split_off = true;
        c->reg_split_off_epoch = c->g.epoch;
        c->split_aborts += 1;
        prof_note(c, "cg_split_abort");
        fprintf(stderr, "[gsparse] split CG hand-off timed out (%d parts); tail re-solved whole, "
                        "split form off for this graph\n", c->split_abort_parts);
    }
}

}  // namespace gs
