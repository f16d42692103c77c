"""CPU: the host arithmetic of mfh_merkle_update_records in csrc/merkle_rows.hpp -- the row's size, the chunk size, and the splice of the staged
record heads and level rows into the packed input row of words.MerkleRecordUpdate.

tests/merkle_record_row_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and
run as a program: nothing is loaded into Python.  For lengths 0, 1, 55 and 65 521 at depths 1 and 24, with an in_stride that is exact and one that is 13
bytes wider, it splices 3 rows out of heap arrays of exactly their sizes and compares them, the untouched tail bytes of a wider row included, with rows
put together byte by byte.  The sanitizer's clean exit is the bound on what the splice reads and writes.  The row bytes and the chunk sizes it prints are
compared with the issue's arithmetic here (a row of (65 521, 1) is 131 139 bytes: 511 a chunk).  The kernels that fill the staged pieces:
tests/test_gpu_merkle_record_update.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [0, 1, 55, 65521]
DEPTHS = [1, 24]
EXTRAS = [0, 13]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_record_row_host") / "merkle_record_row_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_record_row_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_rows_and_sizes(check):
    cases = [(length, depth, extra) for length in LENGTHS for depth in DEPTHS for extra in EXTRAS]
    got = check([f"{length} {depth} {extra} 3 {length + depth + extra}" for length, depth, extra in cases])
    want = []
    for length, depth, extra in cases:
        rowb = 64 + 2 * length + 32 * depth + (depth + 7) // 8
        want.append(f"ok {length} {depth} {extra} 3 {rowb} {min(1000000, max(1, (64 << 20) // rowb))}")
    assert got == want
    assert "ok 65521 1 0 3 131139 511" in got and "ok 0 1 0 3 97 691843" in got


def test_program_refuses_malformed_input(check):
    for line in ("8 0 0 1 1", "8 25 0 1 1", "1048577 1 0 1 1", "8 1 0 0 1", "8 1 0"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
