"""CPU: the host side of mfh_merkle_write_keys -- csrc/merkle_write.hpp (the running field value of every unique key through a batch of sequential writes,
plain and compare-and-set: the update index and the status of every step, the first failed step and the count of failed steps) and csrc/merkle_rows.hpp (the
write row's size and its splice, with and without the expected piece, uncut and cut).

tests/merkle_write_host_check.cpp (a program with its own main that includes the headers) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  For fields of 1, 5, 16, 17 and 39 bytes -- below, at and above one and two 16-byte units of the gather's slot -- it
checks the plan against a sequential model that works on the table's bytes, one step at a time: random batches of many steps among a few members and keys
that are no members, in which keys repeat and statuses 0, 1 and 5 occur, with expectations that only an earlier step satisfies and expectations that an
earlier step breaks, and the same steps without expectations; one key written nk times with e_j = v_j-1; an expectation the table met before the batch and a
step has since overwritten; the first failure at each position of a batch, the step behind it judged without it; every array the plan reads a heap allocation
of exactly its bytes; and the row splice out of exact-size heap arrays.  The sanitizer's clean exit is the bound on what the headers read and write.  The
kernels that produce what the plan takes: tests/test_gpu_merkle_write.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_BYTES = [1, 5, 16, 17, 39]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_write_host") / "merkle_write_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_write_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _run(check, cases):
    got = check([" ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases)
    for (fb, mem, nk, mode, seed), line in zip(cases, got):
        ok, g_fb, g_mem, g_nk, g_mode, batches, steps, failed, rowb = line.split()
        depth, length = 1 + seed % 24, 12 + fb + 1 + seed % 7
        assert ok == "ok" and (int(g_fb), int(g_mem), int(g_nk), int(g_mode)) == (fb, mem, nk, mode), line
        assert int(rowb) == 64 + 5 + 2 * fb + length + 32 * depth + (depth + 7) // 8, line
        yield (fb, mem, nk, mode), int(batches), int(steps), int(failed)


def test_random_batches_with_repeated_keys(check):
    cases = [(fb, mem, nk, 0, 23 * fb + mem + nk) for fb in FIELD_BYTES for mem in (3, 7, 40) for nk in (1, 50, 1500)]
    total = fine = 0
    for (fb, mem, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 2 and steps == 2 * nk
        total, fine = total + steps, fine + steps - failed
    assert 0 < fine < total


def test_expectations_only_the_batch_satisfies_and_ones_it_breaks(check):
    cases = [(fb, 3, nk, 1, 19 * fb + nk) for fb in FIELD_BYTES for nk in (1, 2, 5, 100)]
    for (fb, mem, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == 3 and steps == 2 * nk + 3
        assert failed == 1  # the stale expectation alone: every link of the chain and the no-op are fine


def test_the_first_failure_at_each_position(check):
    cases = [(fb, mem, nk, 2, 17 * fb + mem + nk) for fb in FIELD_BYTES for mem in (3, 6) for nk in (1, 2, 7)]
    for (fb, mem, nk, _), batches, steps, failed in _run(check, cases):
        assert batches == nk and steps == nk * nk and failed == nk  # one failure a batch, and no step behind it fails for it


def test_program_refuses_malformed_input(check):
    for line in ("0 3 1 0 1", "257 3 1 0 1", "8 2 1 0 1", "8 65 1 0 1", "8 3 0 0 1", "8 3 4097 0 1", "8 3 1 3 1", "8 3 201 1 1", "8 3 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
