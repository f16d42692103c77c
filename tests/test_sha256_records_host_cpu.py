"""CPU: the block assembly of csrc/sha256_dev.hpp (sha256_blocks, sha256_block_word, sha256_pad_word), the host pass, against hashlib.

tests/sha256_records_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run
as a program: nothing is loaded into Python.  For every length in 0 .. 130 and 191, 192, 247 .. 257 (the block boundaries at 55 / 56, 119 / 120, 183 / 184
and 247 / 248 bytes, and whole and part words on both sides of them) it hashes a random message from a heap allocation of exactly `length` bytes and at
byte offsets 0 .. 3 at the end of an exact-fit copy, with sha256_block_word for every word of every padded block and sha256_compress; the digest must be
hashlib's.  The sanitizer's clean exit is the bound on what sha256_block_word reads: no byte outside [msg, msg + length).
The kernel k_sha256_records takes its padding from the same sha256_pad_word and its words from an LDS image; tests/test_gpu_sha256_records.py pins it."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(131)) + [191, 192] + list(range(247, 258))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sha256_records_host") / "sha256_records_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sha256_records_host_check.cpp")], check=True)

    def run(pairs):
        """[(message, digest)] -> the program's output lines"""
        text = "".join(f"{bytes(m).hex() or '-'} {bytes(d).hex()}\n" for m, d in pairs)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_block_assembly_equals_hashlib_at_every_length(check):
    rng = np.random.default_rng(2701)
    messages = [rng.bytes(n) for n in LENGTHS]
    messages += [b"\xff" * n for n in (55, 56, 64, 119, 120)] + [b"abc"]
    got = check([(m, hashlib.sha256(m).digest()) for m in messages])
    assert got == [f"ok {len(m)}" for m in messages]


def test_a_wrong_digest_is_reported(check):
    with pytest.raises(subprocess.CalledProcessError) as e:
        check([(b"abc", hashlib.sha256(b"abd").digest())])
    assert e.value.returncode == 1 and "the digest differs" in e.value.stderr


def test_program_refuses_malformed_input(check):
    with pytest.raises(subprocess.CalledProcessError) as e:
        check([(b"abc", bytes(31))])
    assert e.value.returncode == 2
