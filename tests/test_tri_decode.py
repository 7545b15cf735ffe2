"""tri_decode (causalgpslc.jl_amd/csrc/gpslc_internal.h), the lower-packed tile index t -> (ii, jj) of every kernel that walks the
lower triangle of a tile matrix, on the CPU: ii (ii + 1) / 2 + jj == t and 0 <= jj <= ii for every t < 2^21 and for the 1,000
values below INT_MAX (and INT_MAX itself).  The header compiles as plain C++ against tests/c/hip_stub, which declares the few
HIP names it mentions."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tri_decode_inverts_the_lower_packed_index(tmp_path):
    exe = str(tmp_path / "tri_decode_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-attributes", "-I", os.path.join(ROOT, "tests", "c", "hip_stub"),
                           "-o", exe, os.path.join(ROOT, "tests", "c", "tri_decode_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    verdict, n = r.stdout.strip().splitlines()[-1].split()
    assert verdict == "OK" and int(n) == (1 << 21) + 1001
