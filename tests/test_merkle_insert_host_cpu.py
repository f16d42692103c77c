"""CPU: the host side of mfh_merkle_insert_keys -- csrc/merkle_insert.hpp (predecessor, successor and the 2 nk update indices of a batch of sequential key
inserts) and csrc/merkle_rows.hpp (the insert row's size, its splice, the chunk of whole inserts).

tests/merkle_insert_host_check.cpp (a program with its own main that includes the headers) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For key_bytes 1, 3, 4, 5, 8 and 32 and nk 0, 1, 2 and 257 (key_bytes 1 has 254 keys: 100 there) it checks the plan
against a brute-force sequential model -- a list of (lo, hi), one key at a time -- with every key of the batch in ONE range in ascending, descending and
shuffled order, one key per range, and a random mix; the row splice out of heap arrays of exactly their sizes at depths where 2 depth is and is not a
multiple of 8; and that a chunk always holds whole inserts.  The sanitizer's clean exit is the bound on what the headers read and write.  The kernels that
produce what the plan takes: tests/test_gpu_merkle_insert.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BYTES = [1, 3, 4, 5, 8, 32]
NK = [0, 1, 2, 257]
MODES = [0, 1, 2, 3, 4]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_insert_host") / "merkle_insert_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_insert_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_plan_splice_and_chunk(check):
    cases = [(kb, 100 if kb == 1 and nk == 257 else nk, mode, extra, seed) for kb in KEY_BYTES for nk in NK for mode in MODES
             for extra, seed in ((0, 3 * kb + nk + mode), (5, 3 * kb + nk + mode + 1))]
    got = check([" ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases)
    for (kb, nk, mode, extra, seed), line in zip(cases, got):
        ok, g_kb, g_nk, g_mode, g_groups, g_rowb = line.split()
        depth, length = 1 + seed % 24, 2 * kb + extra
        assert ok == "ok" and (int(g_kb), int(g_nk), int(g_mode)) == (kb, nk, mode), line
        assert int(g_rowb) == 64 + kb + 3 * length + 64 * depth + (2 * depth + 7) // 8, line
        groups = int(g_groups)
        if mode <= 2:
            assert groups == min(nk, 1), line  # every key in one range
        elif mode == 3:
            assert groups == nk, line  # one key per range
        elif nk > 2:
            assert 1 < groups < nk, line  # mixed: shared and single ranges


def test_program_refuses_malformed_input(check):
    for line in ("0 1 1 0 1", "33 1 1 0 1", "4 4097 1 0 1", "4 1 5 0 1", "4 1 1 65 1", "1 126 0 0 1", "4 1 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
