// Where everything of the single-workgroup node kernels (k_small.hip) lives: the LDS images, the left-looking kernel's scratch
// and a node's pinned staging.  Each is written down here once and read by the kernels, the host's size functions and api_score.hip
// (DESIGN.md §24).  Plain C++17: tests/c/sm_layout_test.cpp compiles it with g++.  Offsets are in doubles unless named bytes.
#pragma once
#include <cstddef>
#ifdef __HIPCC__
#define SML_HD __host__ __device__
#else
#define SML_HD
#endif

constexpr int kSmB = 16;                         // block size: one f64 MFMA tile, 256 doubles packed column-major
constexpr int kSmWaves = 8;                      // wave64s per workgroup, each with a 16-double multiplier broadcast line
constexpr size_t kLdsCapBytes = 160 * 1024;      // LDS of one CU: a workgroup may opt in to all of it
constexpr int kMidMaxRows = 6, kMidMaxN = 640;   // left-looking kernel: block rows per wave at most; the host's limit on n

// LDS-resident score: [lower blocks, row-major][yv NP][zv NP][ldv NP][broadcast lines][scaled features nF x NP]; the gradient
// adds [alpha NP][raw features nF x NP][lengthscale partials nF x NB][lengthscales nF].  A kernel builds it from its node's nF,
// the host sizes the launch from the widest node's.
struct SmallLayout {
    int NB, NP, yv, zv, ldv, bcl, fs, al, rw, lsp, lsl, total;
    SML_HD SmallLayout(int n, int nF, bool with_grad) {
        NB = (n + kSmB - 1) / kSmB; NP = NB * kSmB;
        yv = NB * (NB + 1) / 2 * 256; zv = yv + NP; ldv = zv + NP; bcl = ldv + NP; fs = bcl + kSmWaves * kSmB;
        al = fs + nF * NP; rw = al + NP; lsp = rw + nF * NP; lsl = lsp + nF * NB;
        total = with_grad ? lsl + nF : al;
    }
    SML_HD size_t bytes() const { return (size_t)total * 8; }
};

// Left-looking kernel.  LDS: [column image(s), NB + 1 blocks each][ldv NP][broadcast lines][operand row NB blocks, if xrow]
// [features: resident (nF + 1) x NP with the target last, else the current block column's nF x 16].  Scratch per node:
// [lower blocks of rows 0..NB, the right-hand side as row NB][features nF x NP][target NP].
struct MidLayout {
    bool resident, two, xrow;                    // the variant: features in LDS, two column images, shared operand row
    int NB, NP, image, ldv, bcl, orow, feat, tgt, lds_total;
    long long s_feat, s_tgt, s_total;
    SML_HD MidLayout(int n, int nF, bool resident_, bool two_, bool xrow_) : resident(resident_), two(two_), xrow(xrow_) {
        NB = (n + kSmB - 1) / kSmB; NP = NB * kSmB;
        image = (NB + 1) * 256;                                      // doubles per column image; the second one follows the first
        ldv = (two ? 2 : 1) * image; bcl = ldv + NP; orow = bcl + kSmWaves * kSmB; feat = orow + (xrow ? NB * 256 : 0);
        tgt = feat + nF * NP;                                        // resident only: the target's LDS copy
        lds_total = resident ? tgt + NP : feat + nF * kSmB;
        s_feat = (long long)(NB + 1) * (NB + 2) / 2 * 256; s_tgt = s_feat + (long long)nF * NP; s_total = s_tgt + NP;
    }
    // the richest variant that fits: operand row (with two images and the features), else two images, else the features, else none
    SML_HD static MidLayout choose(int n, int nF) {
        for (int v = 3; v > 0; --v) {
            const MidLayout l(n, nF, true, v >= 2, v == 3);
            if (l.lds_bytes() <= kLdsCapBytes) return l;
        }
        return MidLayout(n, nF, false, false, false);
    }
    SML_HD size_t lds_bytes() const { return (size_t)lds_total * 8; }
    SML_HD static bool fits(int n) { return (n + kSmB - 1) / kSmB + 1 <= kSmWaves * kMidMaxRows && n <= kMidMaxN; }
};

// A node in the pinned buffer.  Input: [scaled features n x nF][target n], with a gradient [raw features n x nF][ls nF].
// Gradient result: [dF n x nF][dls nF][dscale][dnoise][dtarget n].
struct NodeStage {
    size_t target, raw, ls, in_total, dls, dscale, dnoise, dtarget, out_total;
    SML_HD NodeStage(size_t n, size_t nF, bool with_grad) {
        target = n * nF; raw = target + n; ls = raw + n * nF; in_total = with_grad ? ls + nF : raw;
        dls = n * nF; dscale = dls + nF; dnoise = dscale + 1; dtarget = dnoise + 1; out_total = with_grad ? dtarget + n : 0;
    }
    // the launch's result header: [logdet quad info reserved] per node, then (measurement build) 8 stamps per node, 8 x 8 per wave
    static constexpr size_t kResult = 4, kStamps = 8, kWaveStamps = 64;
    SML_HD static size_t header(size_t count) { return count * (kResult + kStamps) + kWaveStamps; }
};
