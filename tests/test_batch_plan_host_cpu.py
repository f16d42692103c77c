"""CPU: the plan header of the batch prover and the row GEMM's host side (csrc/batch_plan.hpp: row_chunks, row_share, CtGeom, smudge_term, batch_route).

tests/batch_plan_host_check.cpp (a program with its own main that includes only the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a program:
nothing is loaded into Python.  It checks the row-chunk rule at every row count from 1 to 2^18 + 1 (and 2 x 131 071, 2^20, 2^21 + 1), both row units, the chunk limits the
GPU tests set and both minimum chunk counts -- the invariants the kernels rely on, equality with the rule written out step by step, and four values pinned by hand --;
that the row shares of 1 .. 16 ranks tile a region in order and differ by at most one row; the ciphertext geometry at both logq; the smudging term u p against 128-bit
products; and the route of a batch call at the default instance: regenerate / stream, super-groups, the streamed witness pass and each switch that turns it off, forced
slabs, slabs by memory, sub-calls, and a row length that cannot stream.  The kernels under those plans: tests/test_gpu_batch_sizes.py, tests/test_gpu_evalmm.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = 2 * 8 * 2 * ((1 << 18) + 1 + 3) + 4
SHARES = 6 * sum(range(1, 17))
ROUTE = 1 + (2041 - 32 + 1) + 5 + 1 + 3 + 5 + 1 + 3 + 3
CHECKS = CHUNKS + SHARES + 2 + 2 * 7 * 4 + ROUTE


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("batch_plan_host") / "batch_plan_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "batch_plan_host_check.cpp")], check=True)
    return path


def test_the_plan_holds_at_every_row_count_share_and_route(exe):
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert out.stderr == ""  # (a sanitizer report goes there)
    assert out.stdout == f"ok {CHECKS}\n"


def test_a_wrong_chunk_rule_is_reported(exe):
    out = subprocess.run([exe, "spoil"], capture_output=True, text=True)
    assert out.returncode == 1 and "row_chunks differs from the rule" in out.stderr
