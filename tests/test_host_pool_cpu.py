"""The worker pool of librfxhost.so (csrc/host_pool.h) through its stand-alone program tests/host/pool_resize.cpp: every index of a
parallel region is visited exactly once by the time run() returns, on a used pool resized 1 -> 3 -> 8 -> 2 -> 8 threads and while
another thread resizes it.  The program counts; this test builds it, runs it and asks for exit status 0.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_index_is_visited_once_across_resizes(tmp_path):
    exe = str(tmp_path / "pool_resize")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "pool_resize.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert run.returncode == 0, run.stdout
