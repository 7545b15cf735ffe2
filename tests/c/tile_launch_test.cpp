// Host-side check of the launch builders of causalgpslc.jl_amd/csrc/tile_launch.h (plain C++ against tests/c/hip_stub).  Every
// launch site of api.hip is walked over a sweep of shapes; at each, the GemmArgs the site's builder call returns is compared FIELD
// BY FIELD with the field assignments api.hip made by hand before the builders existed (the parent_* functions restate them
// literally), and checked against the invariants the builders own: ntiles is the number of tiles the kernel's decode visits
// (tri_decode, t / mj, or the order array), each visited once and inside [i0, i0 + mi) x [j0, j0 + mj); F / fk go with fuse;
// short_row0 / short_rows go together; sym == 3 needs one short augmented row of at most 32 live rows; skip_gdiag needs a
// triangle.  tile_launch_flop is compared with the arithmetic gemm() carried (restated below) bit for bit, and with counts worked
// out by hand.
//
// Three fields differ from the hand-written assignments on purpose, none of them read by the kernel that receives them:
//   * an unfused column update (factor_panels' last column alone) no longer carries F / fk, which only fused() sets;
//   * the diagonal-tile launch of an in-panel column (launch_diag_update_potrf) is the fused strip's description, fuse included;
//   * a block diagonal of loo() says mi = ntiles as every column does (mi was left 0: loo_diagonal_kernel decodes its own tiles).
#include <cstdio>
#include <cstring>
#include <set>
#include <utility>
#include "../../causalgpslc.jl_amd/csrc/tile_launch.h"

static long long fails = 0, checked = 0;
static void fail(const char* site, const char* what, long long a, long long b) {
    if (fails++ < 30) printf("FAIL %s: %s %lld != %lld\n", site, what, a, b);
}
#define CMP(f) do { if ((long long)(a.f) != (long long)(b.f)) fail(site, #f, (long long)(a.f), (long long)(b.f)); } while (0)
#define CMPP(f) do { if ((const void*)(a.f) != (const void*)(b.f)) fail(site, #f, 0, 1); } while (0)
static void same_ref(const char* site, const TRef& a, const TRef& b) {
    CMPP(base); CMP(bstride); CMP(kind); CMP(ro); CMP(co); CMP(ld); CMP(bdiv);
}
static void same(const char* site, const GemmArgs& a, const GemmArgs& b) {      // a: the builder's, b: the parent's
    ++checked;
    same_ref(site, a.A, b.A); same_ref(site, a.B, b.B); same_ref(site, a.C, b.C); same_ref(site, a.F, b.F);
    CMP(shape); CMP(i0); CMP(j0); CMP(mi); CMP(mj); CMP(k0); CMP(k1); CMP(diag_skip); CMP(nbatch); CMP(ntiles);
    CMP(short_row0); CMP(short_rows); CMP(sym); CMP(fuse); CMP(fk); CMP(skip_gdiag); CMPP(info); CMP(info_base);
    CMPP(queue); CMPP(order); CMPP(dbg);
}

// what tile_gemm_nt_kernel / tile_fused_strip_kernel decode from an item (k_tilegemm.hip); host_order = the order array's content
static void invariants(const char* site, const GemmArgs& g, const std::vector<unsigned short>* host_order) {
    std::set<std::pair<int, int>> seen;
    for (int t = 0; t < g.ntiles; ++t) {
        int ii, jj;
        if (g.order) { ii = (*host_order)[2 * t]; jj = (*host_order)[2 * t + 1]; }
        else if (g.shape == 0) tri_decode(t, ii, jj);
        else { ii = t / g.mj; jj = t - ii * g.mj; }
        const int ti = g.i0 + ii, tj = g.j0 + jj;
        if (ti < g.i0 || ti >= g.i0 + g.mi || tj < g.j0 || tj >= g.j0 + g.mj) fail(site, "tile outside the launch's rectangle", ti, tj);
        if (g.shape == 0 && tj > ti) fail(site, "tile above the diagonal", ti, tj);
        seen.insert({ti, tj});
    }
    const long long want = g.shape == 0 ? (long long)g.mi * (g.mi + 1) / 2 : (long long)g.mi * g.mj;
    if ((long long)seen.size() != want || g.ntiles != want) fail(site, "tiles visited", (long long)seen.size(), want);
    if (g.shape == 0 && (g.mi != g.mj || g.i0 != g.j0 || !g.sym)) fail(site, "triangle is not a symmetric square", g.mi, g.mj);
    if (g.order && host_order->size() != 2 * (size_t)g.ntiles) fail(site, "order length", (long long)host_order->size(), 2 * g.ntiles);
    if ((g.fuse != 0) != (g.F.base != nullptr)) fail(site, "F without fuse or fuse without F", g.fuse, g.F.base != nullptr);
    if (g.fuse && g.mj != 1) fail(site, "fused launch wider than a column", g.mj, 1);
    if (!g.fuse && g.fk) fail(site, "fk without fuse", g.fk, 0);
    if (g.sym == 3 && !(g.short_rows > 0 && g.short_rows <= 32 && g.i0 + g.mi - 1 == g.short_row0))
        fail(site, "sym 3 without one short augmented row of <= 32 live rows", g.short_rows, g.short_row0);
    if (g.skip_gdiag && !(g.shape == 0 && g.short_rows > 0)) fail(site, "skip_gdiag outside a triangle with a short row", g.shape, g.short_rows);
    if (g.short_rows == 0 && g.sym == 3) fail(site, "sym 3 with no short row", g.sym, 0);
}

// ---- the arithmetic gemm() carried for the profiler before tile_launch_flop existed, in its order ----
static double parent_flop(const GemmArgs& g) {
    double short_items = 0;
    if (g.short_rows > 0) {
        const int last = g.i0 + g.mi - 1;
        if (last >= g.short_row0) short_items = (g.shape == 0) ? (double)g.mi : (double)g.mj;
    }
    double diag_items = 0.0;
    if (g.sym && g.i0 == g.j0) diag_items = (g.shape == 0) ? (double)g.mi : 1.0;
    if (short_items > 0 && g.shape == 0) diag_items -= 1.0;
    const double diag_out = (g.diag_skip == 0 || g.diag_skip == 3) ? 1.0 : 0.5;
    double short_exec = short_items;
    if (g.sym == 3 && short_items > 0) short_exec = (g.shape == 0) ? 1.0 : 0.0;
    if (g.skip_gdiag && g.shape == 0 && short_exec >= 1.0) short_exec -= 1.0;
    const double rows = GP_TS * ((double)g.ntiles - short_items - diag_out * diag_items)
                      + (double)g.short_rows * short_exec;
    double flop = 2.0 * GP_TS * GP_TS * rows * (double)(g.k1 - g.k0) * (double)g.nbatch;
    if (g.fuse) flop += (double)GP_TS * GP_TS * rows * (double)g.nbatch;
    return flop;
}
static void flop_as_parent(const char* site, const GemmArgs& g) {
    for (int ds = 0; ds <= 3; ++ds) {
        GemmArgs p = g;
        p.diag_skip = ds;
        const double a = tile_launch_flop(g, ds), b = parent_flop(p);
        if (std::memcmp(&a, &b, sizeof a) != 0) fail(site, "flop bits (diag_skip)", ds, -1);
    }
}
static void launch(const char* site, const GemmArgs& built, const GemmArgs& parent, const std::vector<unsigned short>* order = nullptr) {
    same(site, built, parent);
    invariants(site, built, order);
    flop_as_parent(site, built);
}

// ---- api.hip's hand-written assignments, site by site, as they stood ----
static int parent_aug_sym(int short_rows) { return (short_rows > 0 && short_rows <= 32) ? 3 : 2; }
static GemmArgs parent_robust_column(const TRef& M, int nt, int k, int ka, int nb) {
    GemmArgs g{};
    g.A = M; g.B = M; g.C = M;
    g.shape = 1; g.i0 = k; g.j0 = k; g.mi = nt - k; g.mj = 1; g.sym = 2;
    g.k0 = ka; g.k1 = k; g.nbatch = nb; g.ntiles = g.mi;
    return g;
}
static GemmArgs parent_robust_trailing(const TRef& M, int nt, int ka, int kend, int nb, const unsigned short* order) {
    GemmArgs g{};
    g.A = M; g.B = M; g.C = M;
    const int m = nt - kend;
    g.shape = 0; g.i0 = kend; g.j0 = kend; g.mi = m; g.mj = m; g.sym = 2;
    g.k0 = ka; g.k1 = kend; g.nbatch = nb; g.ntiles = m * (m + 1) / 2;
    g.order = order;
    return g;
}
static GemmArgs parent_strip_base(const TRef& M, const TRef& invref, int nt, int k, int nb, int short_rows) {
    GemmArgs g{};
    g.A = M; g.B = M; g.C = M; g.F = invref; g.fk = k;
    g.shape = 1; g.j0 = k; g.mj = 1; g.k1 = k; g.nbatch = nb;
    g.short_row0 = nt; g.short_rows = short_rows;
    return g;
}
static GemmArgs parent_trailing(const TRef& M, int nt, int ntot, int ka, int kend, int nb, int short_rows, bool skip_gd,
                                const unsigned short* order) {
    GemmArgs t{};
    t.A = M; t.B = M; t.C = M;
    const int m = ntot - kend;
    t.skip_gdiag = skip_gd ? 1 : 0;
    t.shape = 0; t.i0 = kend; t.j0 = kend; t.mi = m; t.mj = m; t.sym = parent_aug_sym(short_rows);
    t.k0 = ka; t.k1 = kend; t.nbatch = nb; t.ntiles = m * (m + 1) / 2;
    t.order = order;
    t.short_row0 = nt; t.short_rows = short_rows;
    return t;
}
static GemmArgs parent_w_solve(const TRef& W, const TRef& Ls, const TRef& invref, int k, int ub, int rows) {
    GemmArgs g{};
    g.A = W; g.B = Ls; g.C = W; g.F = invref; g.fk = k;
    g.shape = 1; g.i0 = 0; g.j0 = k; g.mi = rows; g.mj = 1; g.nbatch = ub; g.ntiles = rows;
    g.k0 = 0; g.k1 = k; g.fuse = 1;
    return g;
}
static GemmArgs parent_loo(const TRef& W, const TRef& M, double* inv, long long inv_bstride, int nt, int d, int nb) {
    GemmArgs g{};
    g.A = g.C = W;
    g.B = M;
    g.F = TRef{inv, inv_bstride, 1, 0, 0, 0};
    g.shape = 1; g.mj = 1; g.fuse = 1; g.nbatch = nb; g.ntiles = nt - d;
    return g;
}
static GemmArgs parent_minus_w_wt(const TRef& W, const TRef& C, int nt, int ub, int rows, const unsigned short* order) {
    GemmArgs g{};
    g.A = W; g.B = W; g.C = C;
    g.shape = 0; g.i0 = 0; g.j0 = 0; g.mi = rows; g.mj = rows; g.sym = 2;
    g.k0 = 0; g.k1 = nt; g.nbatch = ub; g.ntiles = (int)((long long)rows * (rows + 1) / 2);
    g.order = order;
    return g;
}
static GemmArgs parent_tasks(const TRef& M, double* inv, long long inv_bstride, int nt, int nb, int short_rows, int* info, int info_base) {
    GemmArgs g{};
    g.A = M; g.B = M; g.C = M;
    g.F = TRef{inv, inv_bstride, 1, 0, 0, 0};
    g.shape = 1; g.k0 = 0; g.fuse = 1; g.nbatch = nb;
    g.short_row0 = nt; g.short_rows = short_rows; g.sym = 3;
    g.info = info; g.info_base = info_base;
    return g;
}
static GemmArgs parent_mvn_update(const TRef& W, const TRef& Ls, int nt, int naug, int k, int short_rows) {
    GemmArgs u{};
    u.A = W; u.B = Ls; u.C = W;
    u.shape = 1; u.i0 = 0; u.j0 = k + 1; u.mi = naug; u.mj = nt - k - 1;
    u.k0 = k; u.k1 = k + 1; u.nbatch = 1; u.ntiles = naug * (nt - k - 1);
    u.short_row0 = 0; u.short_rows = short_rows;
    return u;
}
static GemmArgs parent_ld_block(const TRef& Wa, const TRef& Wb, const TRef& Cm, int nt) {
    GemmArgs g{};
    g.A = Wa; g.B = Wb; g.C = Cm;
    g.shape = 1; g.i0 = 0; g.j0 = 0; g.mi = nt; g.mj = nt;
    g.k0 = 0; g.k1 = nt; g.nbatch = 1; g.ntiles = nt * nt;
    return g;
}

// the order array of a triangle of m tile rows as api.hip's tri_order hands it to the builder: null up to m = 2
struct Order {
    std::vector<unsigned short> h;
    const unsigned short* p;
    explicit Order(int m) : h(m > 2 ? tri_order_pairs(m) : std::vector<unsigned short>()), p(m > 2 ? h.data() : nullptr) {}
};

static double buf[8];      // stand-ins for device memory: only the addresses matter
static int info_words[4];

static void walk_factor_robust(int nt, int pw, int nb) {
    const TRef M = lower_ref(buf, 7);
    for (int k = 0; k < nt; ++k) {
        const int ka = (k / pw) * pw, kend = std::min(ka + pw, nt);
        if (k > ka) launch("factor_robust column", tile_column(M, M, M, k, k, nt - k, ka, k, nb, true), parent_robust_column(M, nt, k, ka, nb));
        if (k == kend - 1 && nt - kend > 0) {
            const Order o(nt - kend);
            launch("factor_robust trailing", tile_triangle(M, M, M, kend, nt - kend, ka, kend, nb, o.p),
                   parent_robust_trailing(M, nt, ka, kend, nb, o.p), &o.h);
        }
    }
}

static void walk_factor_panels(int nt, int ntot, int pw, int nb, int aug_rows, bool skip_aug_diag) {
    const TRef M = lower_ref(buf, 7);
    const int short_rows = (aug_rows > 0 && ntot == nt + 1) ? aug_rows : 0;
    const long long inv_bstride = (long long)nt * GP_TSQ;
    const TRef invref = inv_ref(buf + 1, nt), parent_invref = TRef{buf + 1, inv_bstride, 1, 0, 0, 0};
    same_ref("inv_ref", invref, parent_invref);
    for (int k = 0; k < nt; ++k) {
        const int ka = (k / pw) * pw, kend = std::min(ka + pw, nt), below = ntot - k - 1;
        auto column = [&](int i0, int k0, bool sym) {
            return short_aug_row(tile_column(M, M, M, i0, k, ntot - i0, k0, k, nb, sym), nt, short_rows);
        };
        GemmArgs g = parent_strip_base(M, parent_invref, nt, k, nb, short_rows);
        if (k > ka && below > 0) {
            g.i0 = k; g.mi = ntot - k; g.ntiles = g.mi; g.k0 = ka; g.sym = parent_aug_sym(short_rows);
            GemmArgs d = g;
            d.info = info_words; d.info_base = 5;
            g.fuse = 1;
            const GemmArgs built = fused(column(k, ka, true), invref, k);
            launch("factor_panels in-panel strip", built, g);
            GemmArgs bd = built;
            bd.info = info_words; bd.info_base = 5;
            d.fuse = 1;      // on purpose (see the top): the diagonal-tile kernel does not read it
            same("factor_panels diagonal-tile launch", bd, d);
        } else {
            if (k > ka) {
                g.i0 = k; g.mi = 1; g.ntiles = 1; g.k0 = ka; g.sym = 2;
                GemmArgs p = g;
                p.F = TRef{}; p.fk = 0;      // on purpose (see the top): an unfused launch reads neither
                launch("factor_panels last column alone", column(k, ka, true), p);
            }
            if (below > 0) {
                g.i0 = k + 1; g.mi = below; g.ntiles = below; g.k0 = k; g.sym = 0; g.fuse = 1;
                launch("factor_panels first column of a panel", fused(column(k + 1, k, false), invref, k), g);
            }
        }
        const bool skip_gd = skip_aug_diag && short_rows > 0;
        if (k == kend - 1 && ntot - kend > (skip_gd ? 1 : 0)) {
            const Order o(ntot - kend);
            launch("factor_panels trailing",
                   short_aug_row(tile_triangle(M, M, M, kend, ntot - kend, ka, kend, nb, o.p), nt, short_rows, skip_gd),
                   parent_trailing(M, nt, ntot, ka, kend, nb, short_rows, skip_gd, o.p), &o.h);
        }
    }
}

static void walk_pairs(int nt, int rows, int ub) {      // w_solve, minus_w_wt: rows = nt (unit B) or the new individuals' mt
    const TRef W = rect_ref(buf + 2, 11, nt), C = lower_ref(buf + 3, 13);
    TRef Ls = lower_ref(buf, 7), invref = inv_ref(buf + 1, nt);
    Ls.bdiv = invref.bdiv = 3;                            // as for_pair_batches sets it on the makers' results
    for (int k = 0; k < nt; ++k)
        launch("w_solve", fused(tile_column(W, Ls, W, 0, k, rows, 0, k, ub, false), invref, k), parent_w_solve(W, Ls, invref, k, ub, rows));
    const Order o(rows);
    launch("minus_w_wt", tile_triangle(W, W, C, 0, rows, 0, nt, ub, o.p), parent_minus_w_wt(W, C, nt, ub, rows, o.p), &o.h);
}

static void walk_loo(int nt, int nb) {
    const TRef W = lower_ref(buf + 4, 17), M = lower_ref(buf, 7);
    for (int d = 1; d < nt; ++d) {
        GemmArgs p = parent_loo(W, M, buf + 1, (long long)nt * GP_TSQ, nt, d, nb);
        p.mi = nt - d;       // on purpose (see the top)
        const GemmArgs g = fused(tile_column(W, M, W, 0, 0, nt - d, 0, 0, nb, false), inv_ref(buf + 1, nt), 0);
        same("loo block diagonal", g, p);
        // loo_diagonal_kernel's own decode: item i is tile (i, i + d), i < ntiles, K range [i, i + d)
        if (g.ntiles != g.mi || g.mj != 1 || !g.fuse) fail("loo block diagonal", "not a fused column", g.ntiles, g.mi);
        for (int i = 0; i < g.ntiles; ++i)
            if (i < g.i0 || i >= g.i0 + g.mi || i + d >= nt) fail("loo block diagonal", "tile outside the matrix", i, i + d);
    }
}

static void walk_tasks(int nt, int nb, int short_rows) {
    const TRef M = lower_ref(buf, 7);
    same("potrf_tasks", task_matrix(M, inv_ref(buf + 1, nt), nt, short_rows, nb, info_words, 9),
         parent_tasks(M, buf + 1, (long long)nt * GP_TSQ, nt, nb, short_rows, info_words, 9));
}

static void walk_mvn(int nt, int naug, int S) {
    const TRef W = rect_ref(buf + 2, (long long)naug * nt * GP_TSQ, nt), Ls = lower_ref(buf, 7);
    const int short_rows = naug == 1 ? S : 0;
    for (int k = 0; k + 1 < nt; ++k)
        launch("mvn update", short_aug_row(tile_rect(W, Ls, W, 0, k + 1, naug, nt - k - 1, k, k + 1, 1), 0, short_rows),
               parent_mvn_update(W, Ls, nt, naug, k, short_rows));
}

static void walk_likelihood(int nt) {
    const TRef Wa = rect_ref(buf + 2, 19, nt), Wb = rect_ref(buf + 3, 19, nt), Cm = rect_ref(buf + 4, 19, nt);
    launch("likelihood block", tile_rect(Wa, Wb, Cm, 0, 0, nt, nt, 0, nt, 1), parent_ld_block(Wa, Wb, Cm, nt));
}

static void expect(const char* what, double got, double want) {
    ++checked;
    if (got != want) { if (fails++ < 30) printf("FAIL flop by hand, %s: %.17g != %.17g\n", what, got, want); }
}
static void flops_by_hand() {
    const TRef M = lower_ref(buf, 7), F = inv_ref(buf + 1, 9);
    const double T3 = 128.0 * 128.0 * 128.0;
    // a plain rectangle: 2 128^3 per tile and K tile
    expect("rectangle", tile_launch_flop(tile_rect(M, M, M, 1, 2, 3, 5, 4, 11, 6), 0), 2.0 * T3 * 3 * 5 * (11 - 4) * 6);
    // a fused column with an empty K range: the panel product alone, 128^3 per tile
    expect("fused column, empty K", tile_launch_flop(fused(tile_column(M, M, M, 4, 3, 5, 3, 3, 7, false), F, 3), 0), T3 * 5 * 7);
    // a fused column with a K range: both
    expect("fused column", tile_launch_flop(fused(tile_column(M, M, M, 4, 3, 5, 1, 3, 7, false), F, 3), 0), 2.0 * T3 * 5 * 2 * 7 + T3 * 5 * 7);
    // a symmetric triangle of m = 6 tile rows, K = 4 tiles: the kernel runs the m (m - 1) / 2 tiles below the diagonal
    const GemmArgs tri = tile_triangle(M, M, M, 3, 6, 0, 4, 2, nullptr);
    expect("triangle", tile_launch_flop(tri, 0), 2.0 * T3 * 15 * 4 * 2);
    // the timing-only variants keep the diagonal tiles as half a tile each
    expect("triangle, diag_skip 1", tile_launch_flop(tri, 1), 2.0 * T3 * (15 + 3) * 4 * 2);
    // its last row (tile row 8) short with r live rows: the 5 x 4 / 2 = 10 full tiles of the rows above, below the diagonal, and
    // r <= 32: the short diagonal tile alone, r rows (the other short tiles ride with the diagonal kernel) — or not even that;
    // r > 32: all 6 short tiles, r rows each — or 5 without the diagonal one
    expect("triangle, short 17", tile_launch_flop(short_aug_row(tri, 8, 17), 0), 2.0 * 128 * 128 * (128.0 * 10 + 17) * 4 * 2);
    expect("triangle, short 17, skip", tile_launch_flop(short_aug_row(tri, 8, 17, true), 0), 2.0 * 128 * 128 * (128.0 * 10) * 4 * 2);
    expect("triangle, short 33", tile_launch_flop(short_aug_row(tri, 8, 33), 0), 2.0 * 128 * 128 * (128.0 * 10 + 33 * 6) * 4 * 2);
    expect("triangle, short 33, skip", tile_launch_flop(short_aug_row(tri, 8, 33, true), 0), 2.0 * 128 * 128 * (128.0 * 10 + 33 * 5) * 4 * 2);
    // a rectangle whose single tile row is short (the MVN update with S <= 128 vectors): S rows per tile
    expect("rectangle, short row", tile_launch_flop(short_aug_row(tile_rect(M, M, M, 0, 3, 1, 4, 2, 3, 1), 0, 100), 0), 2.0 * 128 * 128 * (100.0 * 4) * 1 * 1);
}

int main() {
    const int nts[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 17, 34}, pws[] = {1, 4, 8}, lives[] = {0, 1, 16, 17, 32, 33, 128};
    for (int nt : nts) {
        for (int pw : pws) {
            walk_factor_robust(nt, pw, 3);
            for (int extra = 0; extra <= 2; ++extra)
                for (int live : lives)
                    for (int skip = 0; skip <= 1; ++skip) walk_factor_panels(nt, nt + extra, pw, 2, live, skip != 0);
        }
        for (int rows : {1, 2, nt, nt + 3}) walk_pairs(nt, rows, 6);
        walk_loo(nt, 5);
        for (int live : lives) if (live > 0) walk_tasks(nt, 4, live);
        for (int naug = 1; naug <= 2; ++naug) walk_mvn(nt, naug, naug == 1 ? 100 : 130);
        walk_likelihood(nt);
    }
    flops_by_hand();
    if (aug_sym(0) != 2 || aug_sym(1) != 3 || aug_sym(32) != 3 || aug_sym(33) != 2) fail("aug_sym", "rule", 0, 1);
    printf("%s %lld\n", fails ? "FAILED" : "OK", checked);
    return fails ? 1 : 0;
}
