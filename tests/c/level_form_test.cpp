// Host-side check of the level-form table (causalgpslc.jl_amd/csrc/level_form.h) that every prediction kernel takes its per-form
// factors from.  Exact statements only, over a grid of T_j, a, b and tyLS that includes values off the unit scale; built with
// -ffp-contract=off, so every expression below is evaluated operation by operation as written:
//   - cross / prior / joint equal, bit for bit, the literal expressions the kernels held before the table was folded into the
//     header (the recorded GPU bits, tests/test_gpu_level_form_parent_bits.py, pin the same on the device);
//   - a contrast with a == b gives cross == 0.0, prior == 0.0 and joint == 0.0 against every other level, on either side;
//   - joint of a level with itself equals prior for the contrast, the slope and the outcome: the diagonal of covW is varW;
//   - exactly one form has `factual`, exactly one has `paired`; dispatch_form hands every form its own constant.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <hip/hip_runtime.h>
#include "../../causalgpslc.jl_amd/csrc/level_form.h"

static long long fails = 0, checked = 0;
static void same(double got, double want, const char* what) {
    ++checked;
    if (std::memcmp(&got, &want, sizeof got) == 0) return;
    if (fails++ < 20) printf("FAIL %s: %.17g != %.17g\n", what, got, want);
}
static double rho(double x, double y, double wt) { return std::exp(-((x - y) * (x - y)) * wt); }

using Ord = LevelForm<FORM_ORDINARY>;
using Con = LevelForm<FORM_CONTRAST>;
using Slp = LevelForm<FORM_SLOPE>;
using Out = LevelForm<FORM_OUTCOME>;
static_assert(Ord::factual + Con::factual + Slp::factual + Out::factual == 1 && Ord::factual, "one factual form");
static_assert(Ord::paired + Con::paired + Slp::paired + Out::paired == 1 && Con::paired, "one paired form");

int main() {
    const double Ts[] = {-1.3, 0.0, 0.7, 2.5e-3, 1985.25, -3.0e4};
    const double As[] = {-0.6, 0.3, 0.7, 2001.0, -2.9e4};
    const double Bs[] = {0.5, -0.6, 0.7, 1999.5, 1.0e-3};
    const double LSs[] = {0.25, 1.0, 3.7, 40.0, 1.0e3};
    for (double tl : LSs) {
        const double wt = 1.0 / (tl * tl);
        for (double a : As)
            for (double b : Bs) {
                const double rab = rho(a, b, wt);
                same(Con::prior(rab, wt), (1.0 - rab) + (1.0 - rab), "contrast prior");
                same(Slp::prior(rab, wt), 2.0 * wt, "slope prior");
                same(Out::prior(rab, wt), 1.0, "outcome prior");
                for (double t : Ts) {
                    const double dt = t - a, ra = rho(t, a, wt), rb = rho(t, b, wt);
                    same(Ord::cross(dt, ra, rb, wt), ra, "ordinary cross");
                    same(Out::cross(dt, ra, rb, wt), ra, "outcome cross");
                    same(Con::cross(dt, ra, rb, wt), ra - rb, "contrast cross");
                    same(Slp::cross(dt, ra, rb, wt), (2.0 * dt) * wt * ra, "slope cross");
                    same(gp_slope_q(dt, ra, wt), (2.0 * dt) * wt * ra, "gp_slope_q");
                    same(Con::cross(dt, ra, rho(t, a, wt), wt), 0.0, "contrast cross, a == b");
                }
                same(Con::prior(rho(a, a, wt), wt), 0.0, "contrast prior, a == b");
                // the level against itself: the diagonal of covW is varW
                same(Con::joint(rho(a, a, wt), rho(a, b, wt), rho(b, a, wt), rho(b, b, wt), a - a, wt), Con::prior(rab, wt), "contrast joint(l, l)");
                same(Slp::joint(rho(a, a, wt), 0.0, 0.0, 0.0, a - a, wt), Slp::prior(0.0, wt), "slope joint(l, l)");
                same(Out::joint(rho(a, a, wt), 0.0, 0.0, 0.0, a - a, wt), Out::prior(0.0, wt), "outcome joint(l, l)");
                if (Con::zero_level(a, b) != (a == b) || Ord::zero_level(a, a) || Slp::zero_level(a, a) || Out::zero_level(a, a)) {
                    ++fails; printf("FAIL zero_level\n");
                }
                // against another level (a', b')
                for (double ap : As)
                    for (double bp : Bs) {
                        const double raa = rho(a, ap, wt), rabp = rho(a, bp, wt), rba = rho(b, ap, wt), rbb = rho(b, bp, wt), d = a - ap;
                        same(Ord::joint(raa, rabp, rba, rbb, d, wt), raa, "ordinary joint");
                        same(Out::joint(raa, rabp, rba, rbb, d, wt), raa, "outcome joint");
                        same(Con::joint(raa, rabp, rba, rbb, d, wt), (raa - rabp) - (rba - rbb), "contrast joint");
                        same(Slp::joint(raa, rabp, rba, rbb, d, wt), (2.0 * wt - 4.0 * (d * d) * (wt * wt)) * raa, "slope joint");
                        // the contrast (a, a) against (a', b'), on either side
                        same(Con::joint(raa, rabp, rho(a, ap, wt), rho(a, bp, wt), d, wt), 0.0, "contrast joint, a == b");
                        same(Con::joint(rho(ap, a, wt), rho(ap, a, wt), rho(bp, a, wt), rho(bp, a, wt), ap - a, wt), 0.0, "contrast joint, a' == b'");
                    }
            }
    }
    int seen[4] = {0, 0, 0, 0};
    for (int form = 0; form < 4; ++form)
        dispatch_form(form, [&](auto k) { seen[decltype(k)::value] += (decltype(k)::value == form); });
    for (int form = 0; form < 4; ++form)
        if (seen[form] != 1) { ++fails; printf("FAIL dispatch_form %d\n", form); }
    printf("%s %lld\n", fails ? "FAILED" : "OK", checked);
    return fails ? 1 : 0;
}
