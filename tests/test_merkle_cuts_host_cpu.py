"""CPU: same_cut of csrc/merkle_sched.hpp (mf::merkle_schedule with cuts, the host half of the mfh_merkle_*_cut calls) against a brute-force search.

tests/merkle_cuts_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For n = 0, 1, 2, 257 and 1 000 updates, at depth 2 (cut 1), 3 (cuts 1 | 2 | 1 2), 12 (3 7 10 | 2) and 24 (4 12 |
1 .. 23, every level), with every update at one leaf, two sibling leaves alternating and random draws with heavy repeats, it compares "the last earlier
update at my node of level c_g" with an O(n^2) search on heap arrays of exactly their sizes, and the three outputs without cuts with a call that passes no
cuts.  The sanitizer's clean exit is the bound on what the schedule reads and writes.  The kernel that consumes the table: tests/test_gpu_merkle_segments.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 2, 257, 1000]
PATTERNS = ["same", "alt", "random"]
CUTS = [(2, [1]), (3, [1]), (3, [2]), (3, [1, 2]), (12, [3, 7, 10]), (12, [2]), (24, [4, 12]), (24, list(range(1, 24)))]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_cuts_host") / "merkle_cuts_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_cuts_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_same_cut_equals_brute_force(check):
    cases = [(p, d, n, c) for p in PATTERNS for d, c in CUTS for n in SIZES]
    got = check([f"{p} {d} {n} {11 * d + n} 0 {' '.join(map(str, c))}" for p, d, n, c in cases])
    assert got == [f"ok {p} {d} {n} {len(c)}" for p, d, n, c in cases]


def test_a_wrong_schedule_is_reported(check):
    for line in ("same 3 2 5 1 1", "alt 12 257 6 1 3 7 10", "random 24 1000 7 1 4 12"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 1 and "the schedule differs" in e.value.stderr, line


def test_program_refuses_malformed_input(check):
    for line in ("same 1 4 1 0 1", "same 3 4 1 0", "same 3 4 1 0 0", "same 3 4 1 0 3", "same 3 4 1 0 2 1", "sideways 3 4 1 0 1", "same 3"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
