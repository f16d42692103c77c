"""CPU: the host side of mfh_merkle_transfer_keys -- csrc/merkle_transfer.hpp (the running balance of every account through a batch of sequential transfers:
the 2 nk update indices, the two new balances and the status of every step, the first overdraft and the first overflow) and csrc/merkle_rows.hpp (the transfer
row's size and its splice).

tests/merkle_transfer_host_check.cpp (a program with its own main that includes the headers) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For amount_bytes 1, 2, 3, 5 and 8 it checks the plan against a sequential model that works on the table's bytes, one
step at a time: an account sending three (and more) times; a chain a -> b -> c in which b spends what it has just received, and the same chain backwards, which
overdraws; the first overdraft at each position of a batch; a receiver at the limit 2^(8 A) - 1 -- the limits of A < 8 and of A = 8, where the sum does not fit
64 bits; random batches of many steps among a few accounts and keys that are no members, in which all four statuses occur; and the row splice out of heap arrays
of exactly their sizes, with 64 and 128 zero bytes, at depths where 2 depth is and is not a multiple of 8.  The sanitizer's clean exit is the bound on what the
headers read and write.  The kernels that produce what the plan takes: tests/test_gpu_merkle_transfer.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMOUNT_BYTES = [1, 2, 3, 5, 8]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_transfer_host") / "merkle_transfer_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_transfer_host_check.cpp")], check=True)

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
        assert int(rowb) == 64 + 10 + ab + 2 * length + 64 * depth + (2 * depth + 7) // 8, line
        yield (ab, acc, nk, mode), int(batches), int(steps), int(failed)


def test_an_account_sending_many_times(check):
    cases = [(ab, acc, nk, 0, 11 * ab + acc + nk) for ab in AMOUNT_BYTES for acc in (3, 5) for nk in (3, 1, 32)]
    for _, batches, steps, failed in _run(check, cases):
        assert batches == 2 and failed == 1  # the one step more than the balance allows


def test_a_chain_spends_what_it_has_just_received(check):
    cases = [(ab, acc, nk, 1, 13 * ab + acc + nk) for ab in AMOUNT_BYTES for acc, nk in ((3, 2), (3, 3), (4, 1), (12, 9))]  # (nk <= acc: once round at most)
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 2 and steps == 2 * nk
        assert failed == nk - 1  # backwards nobody but the first account has anything: every step but the last overdraws


def test_the_first_overdraft_at_each_position(check):
    cases = [(ab, acc, nk, 2, 17 * ab + acc + nk) for ab in AMOUNT_BYTES for acc in (3, 6) for nk in (1, 2, 7)]
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == nk and steps == nk * nk and failed == nk  # one overdraft a batch, and no step behind it fails for it


def test_a_receiver_at_the_limit(check):
    cases = [(ab, 3, nk, 3, 19 * ab + nk) for ab in AMOUNT_BYTES for nk in (1, 2, 100)]
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 4 and steps == nk + 5 and failed == 3


def test_random_batches_of_many_steps_among_few_accounts(check):
    cases = [(ab, acc, nk, 4, 23 * ab + acc + nk) for ab in AMOUNT_BYTES for acc in (3, 7, 40) for nk in (1, 50, 1500)]
    total = fine = 0
    for (ab, acc, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 1 and steps == nk
        total, fine = total + steps, fine + steps - failed
    assert 0 < fine < total


def test_program_refuses_malformed_input(check):
    for line in ("0 3 1 0 1", "9 3 1 0 1", "8 2 1 0 1", "8 65 1 0 1", "8 3 0 0 1", "8 3 4097 4 1", "8 3 1 5 1", "8 3 201 3 1", "8 3 33 0 1", "8 3 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
