"""CPU: the launch plan of k_expand_mm that expand_mm_region and a host check share (csrc/expand_plan.hpp: expand_plan(n, logq, nrows[, periods]) -> {ppc, gx, gy}).

tests/expand_plan_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a program: nothing
is loaded into Python.  At n = 1470 and both logq, for every row count from 1 to 2^21 + 1, it checks the bounds the kernel relies on (2 <= ppc <= 10, 23 ppc + 1 <= 256 for
the two sets of span constants, chunks that cover the periods with no empty one, row blocks that cover the rows), that ppc never decreases with the row count, the plans of
the default instance's regions (2) and of 2^20 rows (10), and the first row count that takes 3 periods per chunk (33 793 / 16 385), recomputed from the 4096-workgroup rule by
loops that count workgroups.  The kernel under those plans: tests/test_gpu_expand_mm.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANS = 2 * ((1 << 21) + 1 + 9 * len(range(1, 4097, 37)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("expand_plan_host") / "expand_plan_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "expand_plan_host_check.cpp")], check=True)
    return path


def test_the_plan_keeps_the_kernels_bounds_at_every_row_count(exe):
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert out.stderr == ""  # (a sanitizer report goes there)
    assert out.stdout == f"ok {PLANS}\n"


def test_a_wrong_rule_is_reported(exe):
    out = subprocess.run([exe, "spoil"], capture_output=True, text=True)
    assert out.returncode == 1 and "the plan differs from the rule" in out.stderr
