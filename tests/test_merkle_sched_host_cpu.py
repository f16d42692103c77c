"""CPU: the update schedule of csrc/merkle_sched.hpp (mf::merkle_schedule, the host half of mfh_merkle_update_rows) against a brute-force search.

tests/merkle_sched_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as
a program: nothing is loaded into Python.  For n = 0, 1, 2, 257 and 1 000 updates at depth 1, 3, 9 and 24, with every update at one leaf, two sibling
leaves strictly alternating, and random draws with heavy repeats, it compares "the last earlier update at my leaf", "the last earlier update at my
sibling" of every level and "I am the last at this node" of every level with an O(n^2) search, on heap arrays of exactly their sizes.  The sanitizer's
clean exit is the bound on what the schedule reads and writes.  The kernels that consume the tables: tests/test_gpu_merkle_update.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 257, 1000]
DEPTHS = [1, 3, 9, 24]
PATTERNS = ["same", "alt", "random"]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_sched_host") / "merkle_sched_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_sched_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_schedule_equals_brute_force(check):
    cases = [(p, d, n) for p in PATTERNS for d in DEPTHS for n in SIZES]
    got = check([f"{p} {d} {n} {7 * d + n}" for p, d, n in cases] + ["random 3 1000 99", "random 9 1000 98"])
    assert got == [f"ok {p} {d} {n}" for p, d, n in cases] + ["ok random 3 1000", "ok random 9 1000"]


def test_a_wrong_schedule_is_reported(check):
    for line in ("same 3 2 5 1", "alt 9 257 6 1", "random 24 1000 7 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 1 and "the schedule differs" in e.value.stderr, line


def test_program_refuses_malformed_input(check):
    for line in ("same 0 4 1", "same 32 4 1", "sideways 3 4 1", "same 3"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
