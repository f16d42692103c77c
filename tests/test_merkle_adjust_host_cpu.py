"""CPU: the host side of mfh_merkle_adjust_keys -- csrc/merkle_adjust.hpp (the running balance of every account through a batch of sequential deposits and
withdrawals: the update index, the new balance and the status of every step, the first overdraft, the first overflow and the count of failed steps) and
csrc/merkle_rows.hpp (the adjust row's size and its splice, uncut and cut).

tests/merkle_adjust_host_check.cpp (a program with its own main that includes the headers) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For amount_bytes 1, 2, 3, 5 and 8 it checks the plan against a sequential model that works on the table's bytes, one
step at a time: random batches of many steps among a few accounts and keys that are no members, in which keys repeat and statuses 0, 1, 3 and 4 occur; an
account next to the limit 2^(8 A) - 1 -- for A = 8 next to 2^64 - 1, where balance + amount does not fit 64 bits --, with the sides given and with side = null;
the first overdraft and the first overflow at each position of a batch; every array the plan reads a heap allocation of exactly its bytes; and the row splice
out of exact-size heap arrays.  The sanitizer's clean exit is the bound on what the headers read and write.  The kernels that produce what the plan takes:
tests/test_gpu_merkle_adjust.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMOUNT_BYTES = [1, 2, 3, 5, 8]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_adjust_host") / "merkle_adjust_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_adjust_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _run(check, cases):
    got = check([" ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases)
    for (ab, acc, nk, mode, seed), line in zip(cases, got):
        ok, g_ab, g_acc, g_nk, g_mode, batches, steps, failed, rowb = line.split()
        depth, length = 1 + seed % 24, 10 + ab + seed % 7
        assert ok == "ok" and (int(g_ab), int(g_acc), int(g_nk), int(g_mode)) == (ab, acc, nk, mode), line
        assert int(rowb) == 64 + 5 + ab + 1 + length + 32 * depth + (depth + 7) // 8, line
        yield (ab, acc, nk, mode), int(batches), int(steps), int(failed)


def test_random_batches_with_repeated_keys(check):
    cases = [(ab, acc, nk, 0, 23 * ab + acc + nk) for ab in AMOUNT_BYTES for acc in (3, 7, 40) for nk in (1, 50, 1500)]
    total = fine = 0
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 1 and steps == nk
        total, fine = total + steps, fine + steps - failed
    assert 0 < fine < total


def test_an_account_next_to_the_limit(check):
    cases = [(ab, 3, nk, 1, 19 * ab + nk) for ab in AMOUNT_BYTES for nk in (1, 2, 100)]
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 9 and steps == 2 * (nk + 6) + 3
        assert failed == 2 * 4 + 1  # per pass: the last deposit of one, the limit onto 1, the two in the batch of four; then the withdrawal of one too many


def test_the_first_failure_at_each_position(check):
    cases = [(ab, acc, nk, 2, 17 * ab + acc + nk) for ab in AMOUNT_BYTES for acc in (3, 6) for nk in (1, 2, 7)]
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == nk and steps == nk * nk and failed == nk  # one failure a batch, and no step behind it fails for it


def test_program_refuses_malformed_input(check):
    for line in ("0 3 1 0 1", "9 3 1 0 1", "8 2 1 0 1", "8 65 1 0 1", "8 3 0 0 1", "8 3 4097 0 1", "8 3 1 3 1", "8 3 201 1 1", "8 3 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
