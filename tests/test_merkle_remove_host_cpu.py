"""CPU: the host side of mfh_merkle_remove_keys -- csrc/merkle_remove.hpp (the slot whose hi changes, the hi it receives and the 2 nk update indices of a
batch of sequential key removes) and csrc/merkle_rows.hpp (the remove row's size and its splice).

tests/merkle_remove_host_check.cpp (a program with its own main that includes the headers) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For key_bytes 1, 3, 4, 5, 8 and 32 it checks the plan's union-find against the quadratic walk the header states and
against a sequential model -- a list of (lo, hi), one key at a time -- on runs of 1 .. 6 adjacent members removed in every order, at the smallest members, the
largest and in between; random batches; every member, down to the empty set; many interleaved runs; and the row splice out of heap arrays of exactly their
sizes, with 64 and 128 zero bytes, at depths where 2 depth is and is not a multiple of 8.  The sanitizer's clean exit is the bound on what the headers read
and write.  The kernels that produce what the plan takes: tests/test_gpu_merkle_remove.py."""
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BYTES = [1, 3, 4, 5, 8, 32]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_remove_host") / "merkle_remove_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_remove_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _run(check, cases):
    got = check([" ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases)
    for (kb, nk, mode, extra, seed), line in zip(cases, got):
        ok, g_kb, g_nk, g_mode, batches, removes, rowb = line.split()
        depth, length = 1 + seed % 24, 2 * kb + extra
        assert ok == "ok" and (int(g_kb), int(g_nk), int(g_mode)) == (kb, nk, mode), line
        assert int(rowb) == 64 + kb + 2 * length + 64 * depth + (2 * depth + 7) // 8, line
        yield (kb, nk, mode), int(batches), int(removes)


def test_runs_of_adjacent_members_in_every_order(check):
    cases = [(kb, run, 0, extra, 7 * kb + run + extra) for kb in KEY_BYTES for run in range(1, 7) for extra in (0, 5)]
    for (kb, run, mode), batches, removes in _run(check, cases):
        assert batches == 3 * math.factorial(run) and removes == run * batches  # the smallest members, the largest, in between


def test_random_batches_and_the_empty_set(check):
    cases = [(kb, 100 if kb == 1 and nk == 257 else nk, mode, extra, 3 * kb + nk + mode + extra) for kb in KEY_BYTES for nk in (0, 1, 2, 257) for mode in (1, 2, 3)
             for extra in (0, 5)]
    for (kb, nk, mode), batches, removes in _run(check, cases):
        assert batches == 1
        if mode != 3:
            assert removes == nk
        elif nk > 2:
            assert nk < removes < 2 * nk + 3  # about three quarters of the members: runs of several lengths


def test_program_refuses_malformed_input(check):
    for line in ("0 1 1 0 1", "33 1 1 0 1", "4 4097 1 0 1", "4 1 4 0 1", "4 1 1 65 1", "1 126 1 0 1", "4 0 0 0 1", "4 7 0 0 1", "4 1 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
