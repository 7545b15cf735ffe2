"""The owners of a context's device and pinned memory (causalgpslc.jl_amd/csrc/dev_mem.h), compiled with g++ and driven by
tests/c/dev_mem_test.cpp against a memory policy that counts: reserve() allocates only to grow, and grows in the order quiesce,
release, allocate; a failed growth leaves the buffer empty — null and capacity 0, nothing live — and the next reserve allocates
again (the progress words of the persistent launch); moves hand a block over exactly once, and a vector of buffer-holding structs
can be grown and erased from in the middle (the task-list cache) with one live block per entry throughout; Arena hands out
256-byte-aligned pieces, refuses what does not fit without moving, and repeats its addresses after reset(); PoolArena chains
blocks of at least 1 MiB without moving earlier pieces, merges the chain in reset() into one block of the total size, then serves
the same sequence of takes without allocating, survives a failing merge empty and usable, and release() frees everything."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owners_free_once_grow_in_order_and_survive_failed_allocations(tmp_path):
    exe = str(tmp_path / "dev_mem_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "c", "dev_mem_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    verdict, n = r.stdout.strip().splitlines()[-1].split()
    assert verdict == "OK" and int(n) >= 190, r.stdout[-2000:]
