// Prints the layouts of causalgpslc.jl_amd/csrc/sm_layout.h for every n in 1..640 and nF in 0..32, one line per struct and shape;
// tests/test_sm_layout.py checks them against the formulas they replaced.  Regions are printed as name:offset:length in doubles.
#include <cstdio>
#include "../../causalgpslc.jl_amd/csrc/sm_layout.h"

int main() {
    printf("cap %zu waves %d block %d header1 %zu header7 %zu fits640 %d fits641 %d\n", kLdsCapBytes, kSmWaves, kSmB,
           NodeStage::header(1), NodeStage::header(7), (int)MidLayout::fits(640), (int)MidLayout::fits(641));
    for (int n = 1; n <= 640; ++n)
        for (int nF = 0; nF <= 32; ++nF) {
            for (int g = 0; g < 2; ++g) {
                const SmallLayout s(n, nF, g);
                const int blocks = s.NB * (s.NB + 1) / 2 * 256;
                printf("small %d %d %d bytes %zu blocks:0:%d yv:%d:%d zv:%d:%d ldv:%d:%d bcl:%d:%d fs:%d:%d", n, nF, g, s.bytes(), blocks,
                       s.yv, s.NP, s.zv, s.NP, s.ldv, s.NP, s.bcl, kSmWaves * kSmB, s.fs, nF * s.NP);
                if (g) printf(" al:%d:%d rw:%d:%d lsp:%d:%d lsl:%d:%d", s.al, s.NP, s.rw, nF * s.NP, s.lsp, nF * s.NB, s.lsl, nF);
                printf("\n");
                const NodeStage t((size_t)n, (size_t)nF, g);
                printf("stage %d %d %d in %zu out %zu scaled:0:%d target:%zu:%d", n, nF, g, t.in_total, t.out_total, n * nF, t.target, n);
                if (g) printf(" raw:%zu:%d ls:%zu:%d | dF:0:%d dls:%zu:%d dscale:%zu:1 dnoise:%zu:1 dtarget:%zu:%d", t.raw, n * nF, t.ls, nF,
                              n * nF, t.dls, nF, t.dscale, t.dnoise, t.dtarget, n);
                printf("\n");
            }
            const MidLayout m = MidLayout::choose(n, nF);
            printf("mid %d %d variant %d %d %d bytes %zu scratch %lld images:0:%d ldv:%d:%d bcl:%d:%d orow:%d:%d feat:%d:%d", n, nF,
                   (int)m.resident, (int)m.two, (int)m.xrow, m.lds_bytes(), m.s_total, (m.two ? 2 : 1) * m.image, m.ldv, m.NP, m.bcl,
                   kSmWaves * kSmB, m.orow, m.xrow ? m.NB * 256 : 0, m.feat, m.resident ? nF * m.NP : nF * kSmB);
            if (m.resident) printf(" tgt:%d:%d", m.tgt, m.NP);
            printf(" | blocks:0:%lld feat:%lld:%d tgt:%lld:%d\n", (long long)(m.NB + 1) * (m.NB + 2) / 2 * 256, m.s_feat, nF * m.NP, m.s_tgt, m.NP);
        }
    return 0;
}
