"""CPU: the host-compiled half of mfh_merkle_grow in csrc/merkle_grow.hpp -- mf::grow_node, mf::grow_units and mf::grow_inert_roots, the text the kernels
k_grow_nodes / k_grow_spine and the driver of merkle.hip compile too -- against counts computed in this file and the Python model (words.inert_roots).

tests/merkle_grow_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  The two trees, the counters and the constants are heap allocations of exactly their sizes, so the sanitizer's clean
exit is the bound on what the placement names.  The kernels that run on it: tests/test_gpu_merkle_grow.py.

1. every (d, D) with 1 <= d < D <= 12: every position of the new tree is classified exactly once and as its level and index call for, the copies map onto
   every old position exactly once, the spine is D - d positions, the constants carry their level, every unit of the memory is written exactly once.
2. (23, 24) and the other depth-24 growths, (19, 20) and (20, 21) by arithmetic on the boundaries alone.
3. grow_inert_roots against words.inert_roots at the padding edges of SHA-256 -- lengths 0, 55, 56, 64, 119 -- and in leaf mode, up to depth 24.
4. the program refuses malformed input."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c_lwe_snarks_amd.words import inert_roots  # noqa: E402


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_grow_host") / "merkle_grow_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_grow_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _counts(d, D):
    """(copies, inert, spine): the old tree's 2^(d + 1) - 1 nodes, D - d spine nodes, the rest of the new tree's 2^(D + 1) - 1"""
    copies, spine = (2 << d) - 1, D - d
    return copies, (2 << D) - 1 - copies - spine, spine


def test_every_position(check):
    pairs = [(d, D) for d in range(1, 12) for D in range(d + 1, 13)]
    got = check([f"place {d} {D}" for d, D in pairs])
    for (d, D), line in zip(pairs, got):
        copies, inert, spine = _counts(d, D)
        assert line == f"place {copies} {inert} {spine} 1 {copies} {4 << D}", (d, D)
    assert len(got) == len(pairs) == 66


def test_boundaries(check):
    pairs = [(23, 24), (1, 24), (12, 24), (19, 20), (20, 21), (1, 2)]
    got = check([f"edge {d} {D}" for d, D in pairs])
    for (d, D), line in zip(pairs, got):
        copies, inert, spine = _counts(d, D)
        asked = 2 * (d + 1) + (D - d) + 2 * D + 2  # two a copied level, one a spine node, two a level with constants (all but the root's), 0 and the last
        assert line == f"edge {copies} {inert} {spine} {asked}", (d, D)


@pytest.mark.parametrize("length", [None, 0, 55, 56, 64, 119])
def test_inert_roots(check, length):
    for depth in (0, 1, 7, 24):
        want = "roots " + " ".join(e.hex() for e in inert_roots(depth, length))
        assert check([f"roots {0 if length is None else 1} {0 if length is None else length} {depth}"]) == [want], (length, depth)


def test_program_refuses_malformed_input(check):
    for line in ("place 0 1", "place 3 3", "place 4 3", "place 3 17", "place 3", "place 3 x", "place -1 3", "edge 0 1", "edge 24 25", "edge 5 5", "edge 5",
                 "roots 2 55 3", "roots 1 1048577 3", "roots 1 55 25", "roots 1 55", "roots 1 55 3 4", "grow 1 2", "roots"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
