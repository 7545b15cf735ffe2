"""The layouts of the single-workgroup node kernels (causalgpslc.jl_amd/csrc/sm_layout.h: the LDS images of the LDS-resident score,
its gradient and the left-looking kernel, that kernel's scratch, a node's pinned staging), compiled with g++ and printed by
tests/c/sm_layout_test.cpp for every n in 1..640 and nF in 0..32: the totals equal the formulas the kernels' host functions used
before the header existed (restated here), the regions ascend without overlap and fill the total, the multiplier broadcast lines
are 16-byte aligned, and the sizes at which a call changes path are where those formulas put them."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 160 * 1024
TABLE_NF = (0, 3, 16, 32)


def _nb(n):
    return (n + 15) // 16


def score_bytes(n, nF):
    NB, NP = _nb(n), 16 * _nb(n)
    return (NB * (NB + 1) // 2 * 256 + 3 * NP + 128 + nF * NP) * 8


def grad_bytes(n, nF):
    NB, NP = _nb(n), 16 * _nb(n)
    return score_bytes(n, nF) + (NP + nF * NP + nF * NB + nF) * 8


def mid_bytes(n, nF, resident, two, xrow):
    NB = _nb(n)
    return ((2 if two else 1) * (NB + 1) * 256 + NB * 16 + 128 + (NB * 256 if xrow else 0)
            + ((nF + 1) * NB * 16 if resident else nF * 16)) * 8


def mid_variant(n, nF):
    """(resident, two, xrow) by the rule of the host function this header replaced"""
    xrow = mid_bytes(n, nF, True, True, True) <= CAP
    two = xrow or mid_bytes(n, nF, True, True, False) <= CAP
    resident = two or mid_bytes(n, nF, True, False, False) <= CAP
    return resident, two, xrow


def mid_scratch(n, nF):
    NB = _nb(n)
    return (NB + 1) * (NB + 2) // 2 * 256 + (nF + 1) * NB * 16


def _regions(words):
    return [(w.split(":")[0], int(w.split(":")[1]), int(w.split(":")[2])) for w in words]


def _check_regions(regs, total, where):
    end = 0
    for name, off, length in regs:
        assert off >= end and length >= 0, (where, name, "overlaps the region before it or descends")
        end = off + length
    assert end <= total, (where, "runs past the total")
    return end


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sm_layout") / "sm_layout_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "c", "sm_layout_test.cpp")])
    out = {"small": {}, "stage": {}, "mid": {}}
    lines = subprocess.check_output([exe], text=True).splitlines()
    out["head"] = lines[0].split()
    for line in lines[1:]:
        w = line.split()
        if w[0] == "mid":
            out["mid"][(int(w[1]), int(w[2]))] = w[3:]
        else:
            out[w[0]][(int(w[1]), int(w[2]), int(w[3]))] = w[4:]
    return out


def test_every_shape_is_there_and_the_constants(layouts):
    assert len(layouts["mid"]) == 640 * 33 and len(layouts["small"]) == len(layouts["stage"]) == 2 * 640 * 33
    h = dict(zip(layouts["head"][::2], map(int, layouts["head"][1::2])))
    assert h == {"cap": CAP, "waves": 8, "block": 16, "header1": 12 + 64, "header7": 7 * 12 + 64, "fits640": 1, "fits641": 0}


def test_small_layout_totals_and_structure(layouts):
    for (n, nF, g), w in layouts["small"].items():
        total = int(w[1])
        assert total == (grad_bytes(n, nF) if g else score_bytes(n, nF)), (n, nF, g)
        regs = _regions(w[2:])
        assert [r[0] for r in regs] == ["blocks", "yv", "zv", "ldv", "bcl", "fs"] + (["al", "rw", "lsp", "lsl"] if g else [])
        assert _check_regions(regs, total // 8, (n, nF, g)) == total // 8          # no gap: the regions fill the image
        assert dict((r[0], r[1]) for r in regs)["bcl"] % 2 == 0, (n, nF, g)        # 16-byte aligned lines
        if g:       # the gradient's image starts with the score's
            assert w[2:8] == layouts["small"][(n, nF, 0)][2:8]


def test_mid_layout_totals_and_structure(layouts):
    for (n, nF), w in layouts["mid"].items():
        variant = tuple(bool(int(x)) for x in w[1:4])
        assert variant == mid_variant(n, nF), (n, nF)
        lds, scratch = int(w[5]), int(w[7])
        assert lds == mid_bytes(n, nF, *variant) and scratch == mid_scratch(n, nF), (n, nF)
        bar = w.index("|")
        regs = _regions(w[8:bar])
        assert _check_regions(regs, lds // 8, (n, nF)) == lds // 8
        assert dict((r[0], r[1]) for r in regs)["bcl"] % 2 == 0, (n, nF)
        assert _check_regions(_regions(w[bar + 1:]), scratch, (n, nF)) == scratch


def test_node_stage_totals_and_structure(layouts):
    for (n, nF, g), w in layouts["stage"].items():
        tin, tout = int(w[1]), int(w[3])
        assert tin == n * nF + n + (n * nF + nF if g else 0) and tout == (n * nF + nF + 2 + n if g else 0), (n, nF, g)
        rest = w[4:]
        bar = rest.index("|") if g else len(rest)
        assert _check_regions(_regions(rest[:bar]), tin, (n, nF, g)) == tin
        if g:
            assert _check_regions(_regions(rest[bar + 1:]), tout, (n, nF, g)) == tout


# nF: (LDS-resident score up to n, operand row from n, two images from n, resident from n, none from n); None = not reached
SWITCH = {0: (176, 177, 385, 577, None), 3: (176, 177, 369, 529, None), 16: (176, 177, 289, 385, 577), 32: (160, 161, 241, 289, 401)}
GRAD_FITS = ((7, 176), (17, 160), (27, 144), (32, 128))         # nF up to ...: the gradient fits up to n


def test_path_switch_points(layouts):
    for nF, (score_to, *starts) in SWITCH.items():
        small = lambda n: int(layouts["small"][(n, nF, 0)][1]) <= CAP     # noqa: E731
        assert all(small(n) for n in range(1, score_to + 1)) and not any(small(n) for n in range(score_to + 1, 641)), nF
        kinds = ((1, 1, 1), (1, 1, 0), (1, 0, 0), (0, 0, 0))
        first = {}
        for n in range(score_to + 1, 641):
            first.setdefault(tuple(int(x) for x in layouts["mid"][(n, nF)][1:4]), n)
        assert [first.get(k) for k in kinds] == starts, nF
        seq = [tuple(int(x) for x in layouts["mid"][(n, nF)][1:4]) for n in range(score_to + 1, 641)]
        assert seq == sorted(seq, reverse=True), nF        # a larger n never takes a richer variant
    lo = 0
    for nF_to, n_to in GRAD_FITS:
        for nF in range(lo, nF_to + 1):
            fits = [n for n in range(1, 641) if int(layouts["small"][(n, nF, 1)][1]) <= CAP]
            assert fits == list(range(1, n_to + 1)), nF
        lo = nF_to + 1
