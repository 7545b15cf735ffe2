"""The level-form table (causalgpslc.jl_amd/csrc/level_form.h) on the CPU: cross / prior / joint of every form against the literal
expressions of the kernels they were folded out of, bit for bit, and the exact identities the outputs rest on (a contrast of a
level with itself is 0.0 everywhere; joint of a level with itself is prior, so the diagonal of covW is varW; one factual and one
paired form).  The header compiles as plain C++ against tests/c/hip_stub; -ffp-contract=off keeps every operation as written."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_level_form_table_is_exact(tmp_path):
    exe = str(tmp_path / "level_form_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-attributes",
                           "-I", os.path.join(ROOT, "tests", "c", "hip_stub"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "level_form_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    verdict, n = r.stdout.strip().splitlines()[-1].split()
    # 5 lengthscales x 25 (a, b) pairs x (3 priors + 6 T x 6 + 1 + 3 + 25 pairs x 6)
    assert verdict == "OK" and int(n) == 5 * 25 * (3 + 36 + 1 + 3 + 150)
