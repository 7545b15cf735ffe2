"""The host-built task order of the persistent factorisation launch (causalgpslc.jl_amd/csrc/task_list.h) replayed on the CPU through
task_needs / task_products, the two functions potrf_tasks_kernel itself waits and publishes through: every task sits behind its
producers in its own queue (tickets go out in list order to running workgroups, so this is the launch's no-deadlock argument), every
progress word moves exactly once per column and column by column, a matrix never leaves its queue, and every tile a task reads by the
left-looking algorithm (the test's own statement, in tiles) is final through the task's needs — for every tile count 2 .. 32,
1 .. 1,000 matrices, group sizes 1 .. 4,096, 1 .. 4 tile rows per strip task, with and without the back-substitution task, both forms
of the augmented row.  Lists broken on purpose (a diagonal task in front of a strip it needs, a descriptor dropped, a matrix split
over two queues) must be flagged.
The work the launch replaces: src/likelihood.jl:42-43, src/estimation.jl:46."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_task_order_follows_the_kernels_wait_rules(tmp_path):
    exe = str(tmp_path / "task_list_test")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "c", "task_list_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:]
    verdict, n = r.stdout.strip().splitlines()[-1].split()
    assert verdict == "OK" and int(n) > 10000
