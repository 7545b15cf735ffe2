// Host-side check of tri_decode (causalgpslc.jl_amd/csrc/gpslc_internal.h), the inverse of the lower-packed tile index
// t = ii (ii + 1) / 2 + jj, 0 <= jj <= ii, that gram_kernel, dense_load_kernel, gather_cov_kernel and the tile-product kernels
// use to find their tile: every t < 2^21 (2,047 tiles per side and more) and the 1,000 values below INT_MAX, where the
// square root's rounding and the width of the products matter.
#include <climits>
#include <cstdio>
#include "../../causalgpslc.jl_amd/csrc/gpslc_internal.h"

static long long fails = 0, checked = 0;
static void check(int t) {
    int ii = -1, jj = -1;
    tri_decode(t, ii, jj);
    ++checked;
    if ((long long)ii * (ii + 1) / 2 + jj == t && 0 <= jj && jj <= ii) return;
    if (fails++ < 20) printf("FAIL t = %d: ii = %d, jj = %d\n", t, ii, jj);
}

int main() {
    for (int t = 0; t < (1 << 21); ++t) check(t);
    for (int t = INT_MAX - 1000; t < INT_MAX; ++t) check(t);
    check(INT_MAX);
    printf("%s %lld\n", fails ? "FAILED" : "OK", checked);
    return fails ? 1 : 0;
}
