"""CPU: the host side of mfh_merkle_absent_rows -- csrc/merkle_keys.hpp (the queries sorted with their permutation, de-duplicated, turned into big-endian
words; the results scattered back) and csrc/merkle_rows.hpp (the row's size and splice).

tests/merkle_keys_host_check.cpp (a program with its own main that includes the two headers) is compiled with g++ -O1 -fsanitize=address,undefined and
run as a program: nothing is loaded into Python.  For key_bytes 1, 3, 4, 5, 8, 20 and 32 and nq 0, 1 and 257 -- drawn from pools of 1, 40 and 4 096 keys,
so with every query the same, with heavy duplicates and with few, keys that differ in the last byte only among them -- it checks the plan against a
brute-force memcmp model, the scatter on made-up result words, and the splice of found and not-found rows out of heap arrays of exactly their sizes; the
key array is exactly (nq - 1) * key_stride + key_bytes bytes.  The sanitizer's clean exit is the bound on what the header reads and writes.  The kernels
that produce the result words: tests/test_gpu_merkle_absent.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_BYTES = [1, 3, 4, 5, 8, 20, 32]
NQ = [0, 1, 257]
POOLS = [1, 40, 4096]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_keys_host") / "merkle_keys_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_keys_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_plan_scatter_and_splice(check):
    cases = [(kb, nq, pool, extra, seed) for kb in KEY_BYTES for nq in NQ for pool in POOLS for extra, seed in ((0, 2 * kb + nq), (5, 2 * kb + nq + 1))]
    got = check([" ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases)
    for (kb, nq, pool, extra, seed), line in zip(cases, got):
        ok, g_kb, g_nq, g_nu, g_kw, g_rowb = line.split()
        depth, length = 1 + seed % 24, 2 * kb + extra
        assert ok == "ok" and (int(g_kb), int(g_nq), int(g_kw)) == (kb, nq, (kb + 3) // 4), line
        assert int(g_rowb) == 32 + kb + length + 32 * depth + (depth + 7) // 8, line
        nu = int(g_nu)
        assert (nu == 0) == (nq == 0) and nu <= min(nq, pool), line
        if nq == 257 and pool == 4096 and kb >= 4 and not seed & 1:
            assert nu > 240, line  # few duplicates among random keys
        if nq == 257 and pool == 40:
            assert 20 < nu <= 40, line  # heavy duplicates


def test_program_refuses_malformed_input(check):
    for line in ("0 1 1 0 1", "33 1 1 0 1", "4 4097 1 0 1", "4 1 0 0 1", "4 1 1 65 1", "4 1 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
