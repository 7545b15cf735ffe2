// The launches of the tile-product kernels (k_tilegemm.hip), described in one place: the makers of the tile-matrix references, one
// builder per kind of GemmArgs, and the profiler's flop count of a launch.  Plain host C++ (tests/c/tile_launch_test.cpp compiles
// it with g++).  A builder returns a complete GemmArgs and owns the invariants between its fields; no caller sets a field of the
// launches it passes to gemm() itself ("Where a tile-product launch is described").
#pragma once
#include <algorithm>
#include <vector>
#include "gpslc_internal.h"

inline TRef lower_ref(double* base, long long bstride) { return TRef{base, bstride, 0, 0, 0, 0}; }
inline TRef rect_ref(double* base, long long bstride, int ld) { return TRef{base, bstride, 1, 0, 0, ld}; }
// the nt inverted diagonal blocks of a factor, one tile row per matrix: tile (j, kk) -> inv[kk]
inline TRef inv_ref(double* inv, int nt) { return TRef{inv, (long long)nt * GP_TSQ, 1, 0, 0, 0}; }

// GemmArgs::sym of a symmetric launch of the factorisation of A: with a single short augmented tile row, its off-diagonal tiles
// ride with the diagonal items (3).  Up to 32 live rows (31 levels): beyond that the diagonal kernel runs out of registers and
// the augmented tiles carry enough real work to stay ordinary items
inline int aug_sym(int short_rows) { return (short_rows > 0 && short_rows <= 32) ? 3 : 2; }

// Kind: RECTANGLE.  C(i, j) -= sum_{kk in [k0, k1)} A(i, kk) B(j, kk)^T on the mi x mj tiles from (i0, j0), item t = tile
// (i0 + t / mj, j0 + t % mj): ntiles = mi mj
inline GemmArgs tile_rect(const TRef& A, const TRef& B, const TRef& C, int i0, int j0, int mi, int mj, int k0, int k1, int nb) {
    GemmArgs g{};
    g.A = A; g.B = B; g.C = C;
    g.shape = 1; g.i0 = i0; g.j0 = j0; g.mi = mi; g.mj = mj;
    g.k0 = k0; g.k1 = k1; g.nbatch = nb; g.ntiles = mi * mj;
    return g;
}

// Kind: ONE TILE COLUMN j0, tile rows [i0, i0 + mi): ntiles = mi.  sym: A, B and C are one tile matrix and (i0, j0) is its
// diagonal tile, which this launch leaves to the diagonal-tile kernels (GemmArgs::sym = 2)
inline GemmArgs tile_column(const TRef& A, const TRef& B, const TRef& C, int i0, int j0, int mi, int k0, int k1, int nb, bool sym) {
    GemmArgs g = tile_rect(A, B, C, i0, j0, mi, 1, k0, k1, nb); g.sym = sym ? 2 : 0; return g;
}
// ... whose items also apply the panel product with tile (0, fk) of F, the inverted diagonal blocks (strip_item; an empty K range
// is then the panel product alone).  F and fk are set here and nowhere else
inline GemmArgs fused(GemmArgs column, const TRef& F, int fk) { column.fuse = 1; column.F = F; column.fk = fk; return column; }

// Visiting order of the m(m+1)/2 lower-triangular output tiles as (ii, jj) pairs: G x G super-blocks in row-major order,
// row-major inside.  The kernel hands XCD x the x-th contiguous run of work items, so the ~64
// workgroups an XCD runs concurrently cover about one super-block: they walk the K slabs of the same
// G + G operand tile rows together and share them in that XCD's L2 instead of each streaming its own
// copy from HBM (operand traffic / ~G).
constexpr int kOrderBlock = 8;     // super-block edge (tiles)
inline std::vector<unsigned short> tri_order_pairs(int m) {
    constexpr int G = kOrderBlock;
    std::vector<unsigned short> h;
    h.reserve((size_t)m * (m + 1));
    for (int I = 0; I < m; I += G)
        for (int J = 0; J <= I; J += G)
            for (int i = I; i < std::min(I + G, m); ++i)
                for (int j = J; j < std::min(J + G, m) && j <= i; ++j) h.insert(h.end(), {(unsigned short)i, (unsigned short)j});
    return h;
}

// Kind: LOWER TRIANGLE (diagonal included) of the m x m tile square from (i0, i0), symmetric (A == B by contract): ntiles =
// m (m + 1) / 2, visited in `order` = tri_order(c, m), the device copy of tri_order_pairs(m) (or null: tri_decode's order)
inline GemmArgs tile_triangle(const TRef& A, const TRef& B, const TRef& C, int i0, int m, int k0, int k1, int nb, const unsigned short* order) {
    GemmArgs g = tile_rect(A, B, C, i0, i0, m, m, k0, k1, nb);
    g.shape = 0; g.sym = 2; g.order = order;
    g.ntiles = (int)((long long)m * (m + 1) / 2);
    return g;
}

// Modifier: the output tile rows from row0 on (augmented right-hand-side rows) carry only `rows` live rows (0 = all of them).  A
// symmetric launch takes its sym from aug_sym: 3 only with a short row of at most 32 live rows.  skip_diag (triangles): the short
// augmented diagonal tile (row0, row0) is not an item, nobody reads -R R^T (EpiArgs::from_rows)
inline GemmArgs short_aug_row(GemmArgs g, int row0, int rows, bool skip_diag = false) {
    g.short_row0 = row0; g.short_rows = rows;
    if (g.sym) g.sym = aug_sym(rows);
    g.skip_gdiag = (skip_diag && rows > 0 && g.shape == 0) ? 1 : 0;
    return g;
}

// Kind: THE MATRIX OF A TASK LAUNCH (PotrfTaskArgs::g): the tasks come from the launch's list, not from (i0, mi, ntiles); the
// strips are fused ones of the lower-packed M with its inverted diagonal blocks F, K ranges from column 0, and the one augmented
// tile row nt rides with the diagonal tasks (sym = 3) or, beyond 32 live rows, as tasks of the list (build_task_list's aug_full)
inline GemmArgs task_matrix(const TRef& M, const TRef& F, int nt, int short_rows, int nb, int* info, int info_base) {
    GemmArgs g = short_aug_row(fused(tile_rect(M, M, M, 0, 0, 0, 0, 0, 0, nb), F, 0), nt, short_rows);
    g.sym = 3; g.info = info; g.info_base = info_base;
    return g;
}

// The profiler's algorithmic flop count of launch_tile_gemm(g) (gemm(), factor.hip); diag_skip: the measurement build's
// GPSLC_GEMM_DIAG variant, 0 otherwise
inline double tile_launch_flop(const GemmArgs& g, int diag_skip) {
    // algorithmic flop: full tiles count 2*128^3 per K tile, items in the (single) augmented row only
    // their live right-hand-side rows
    double short_items = 0;
    if (g.short_rows > 0) {
        const int last = g.i0 + g.mi - 1;                       // last output tile row of the launch
        if (last >= g.short_row0) short_items = (g.shape == 0) ? (double)g.mi : (double)g.mj;
    }
    // diagonal tiles of a symmetric launch need only their lower triangle: half a tile product, as in the
    // textbook N^3/3 count (the kernel runs 36 of the 64 sub-tile products, GemmArgs::sym); the short
    // augmented diagonal tile is already counted by its live rows
    double diag_items = 0.0;
    if (g.sym && g.i0 == g.j0) diag_items = (g.shape == 0) ? (double)g.mi : 1.0;
    if (short_items > 0 && g.shape == 0) diag_items -= 1.0;
    // this kernel does not run the full-size diagonal tiles at all (launch_syrk_diag does, outside the timed bracket, so
    // that the HIP-event average equals rocprofv3's average for the dominant kernel); the timing-only variants
    // (GPSLC_GEMM_DIAG = 1 / 2) keep them as half a tile product each
    const double diag_out = (diag_skip == 0 || diag_skip == 3) ? 1.0 : 0.5;
    // sym == 3: the off-diagonal augmented-row tiles are not this kernel's either (they ride with the diagonal items)
    double short_exec = short_items;
    if (g.sym == 3 && short_items > 0) short_exec = (g.shape == 0) ? 1.0 : 0.0;
    if (g.skip_gdiag && g.shape == 0 && short_exec >= 1.0) short_exec -= 1.0;     // the augmented diagonal tile is not run
    const double rows = GP_TS * ((double)g.ntiles - short_items - diag_out * diag_items)
                      + (double)g.short_rows * short_exec;
    double flop = 2.0 * GP_TS * GP_TS * rows * (double)(g.k1 - g.k0) * (double)g.nbatch;
    // fused panel product: one triangular solve per tile row = 128^2 * 128 multiply-adds... counted as the
    // textbook n^2 b flop of a TRSM (the kernel runs 56 % of the dense 2*128^3 product)
    if (g.fuse) flop += (double)GP_TS * GP_TS * rows * (double)g.nbatch;
    return flop;
}
