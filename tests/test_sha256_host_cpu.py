"""CPU: the host pass of csrc/sha256_dev.hpp against the pure-Python reference, and words.MerklePath.statement.

1. tests/sha256_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
   program: nothing is loaded into Python.  Its compressions equal tests/sha256_ref.py on the all-zero block, the all-ones block and 64 random blocks,
   each from the initial hash value and from a random chaining value, and hashlib.sha256(b"abc") for the one padded block.
   This pins the rounds, the message schedule and the 64 constants of sha256_compress.  It does NOT pin the device pass's three v_bitop3 truth tables
   (0x96 XOR3, 0xCA Ch, 0xE8 Maj) nor its v_alignbit rotations: those are compiled for the GPU alone, and tests/test_gpu_merkle.py pins them (every node
   of a tree the kernel built against this same reference).
2. MerklePath.statement(root) is the inverse of root_of: the statement bytes of an assigned row; a wrong length raises CircuitError."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sha256_host") / "sha256_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sha256_host_check.cpp")], check=True)

    def run(pairs):
        """[(chaining value: 8 words, block: 64 bytes)] -> the compressions as bytes"""
        text = "".join(f"{ref.words_bytes(h).hex()} {bytes(b).hex()}\n" for h, b in pairs)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        lines = out.stdout.split()
        assert len(lines) == len(pairs)
        return [bytes.fromhex(x) for x in lines]

    return run


def test_host_compression_equals_reference(check):
    rng = np.random.default_rng(2601)
    blocks = [bytes(64), b"\xff" * 64] + [rng.bytes(64) for _ in range(64)]
    pairs = [(ref.IV, b) for b in blocks]
    pairs += [(tuple(int(x) for x in rng.integers(0, 1 << 32, size=8, dtype=np.uint64)), b) for b in blocks]
    pairs += [((0xFFFFFFFF,) * 8, b"\xff" * 64), ((0,) * 8, bytes(64))]
    got = check(pairs)
    for (h, b), g in zip(pairs, got):
        assert g == ref.words_bytes(ref.compress(h, b)), (h, b.hex())


def test_host_compression_abc(check):
    assert check([(ref.IV, ref.pad(b"abc"))]) == [hashlib.sha256(b"abc").digest()]


def test_host_program_refuses_malformed_input(check):
    with pytest.raises(subprocess.CalledProcessError):
        check([(ref.IV, bytes(63))])


def test_merkle_statement_is_the_inverse_of_root_of():
    p = mf.Params(d=1 << 17, m=87381)
    st = W.MerklePath(1)
    rng = np.random.default_rng(2602)
    leaf, sib = rng.bytes(32), rng.bytes(32)
    bits = st.bits(leaf, [sib], 1)
    row = st.circuit.assign(bits[:256], bits[256:], p)
    root = st.root_of(row)
    assert root == ref.merkle_parent(sib, leaf)
    assert W.MerklePath.statement(root) == bytes(row[:32])
    assert st.statement(bytearray(root)) == bytes(row[:32])
    assert W.MerklePath.statement(bytes(range(32)))[:8] == bytes([3, 2, 1, 0, 7, 6, 5, 4])
    for bad in (b"", root[:31], root + b"\0"):
        with pytest.raises(C.CircuitError):
            W.MerklePath.statement(bad)
