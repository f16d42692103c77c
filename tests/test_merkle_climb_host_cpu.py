"""CPU: the host half of the cut reads in csrc/merkle_rows.hpp -- mf::climb_chunk, mf::climb_staged_units, mf::climb_rows_bytes, mf::climb_plan and the
splice of staged rows into the caller's (mf::splice_climb_row, mf::splice_row at tail 64) -- against sizes and rows computed in this file.

tests/merkle_climb_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  The staged buffer and every caller's row are heap allocations of exactly their sizes, so the sanitizer's clean
exit is the bound on what the splice reads and writes.  The kernel that fills the staged rows: tests/test_gpu_merkle_climb.py.

1. chunk and plan at depth 2 (cut 1), 3 (1 | 2 | 1 2), 12 (2 | 3 11), 20 (10 | 1) and 24 (every level), for a call of paths and an absent call of (4, 8) and
   (8, 55) records, with stages of 64 MiB, of exactly k rows, of one byte less and of less than one row (a chunk is at least one statement).
2. the two-chunk recipe of the GPU test: depth 2, cut 1, length 65 521 -- 1 021 statements a chunk.
3. the spliced rows of a small chunk, byte for byte: paths rows whole, absent rows under key and record, a status 2 statement's key alone and zero rows above.
4. the program refuses malformed input."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = 64 << 20
SHAPES = [(2, [1]), (3, [1]), (3, [2]), (3, [1, 2]), (12, [2]), (12, [3, 11]), (20, [10]), (20, [1]), (24, list(range(1, 24)))]
HEADS = [(0, 0), (4, 8), (8, 55)]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_climb_host") / "merkle_climb_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_climb_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _levels(depth, cuts):
    edges = [0] + list(cuts) + [depth]
    return [(lo, hi - lo) for lo, hi in zip(edges, edges[1:])]


def _row_bytes(g, levels, K, length):
    """a caller's row: segment 0 of an absent call has key and record where the others have zeros and a node"""
    head = 32 + K + length if g == 0 and K else 64
    return head + 32 * levels + (levels + 7) // 8


def _want(depth, cuts, n, K, length, stage):
    """the lines the program prints without a dump, from the issue's layout: 5 + 2 levels units a staged row, the segments one behind the other"""
    segs = _levels(depth, cuts)
    all_rows = sum(_row_bytes(g, lv, K, length) for g, (_, lv) in enumerate(segs))
    chunk = max(1, min(n, stage // all_rows))
    units = [5 + 2 * lv for _, lv in segs]
    lines = [f"chunk {chunk} {sum(units)} {all_rows - _row_bytes(0, segs[0][1], K, length)} {max(units)} {len(segs)}"]
    base = 0
    for g, (lo, lv) in enumerate(segs):
        head = 0 if g else 4 if K else 2  # the unit of the stored node: none (the first unit behind the head) under a head of records
        lines.append(f"seg {lo} {lv} {base} {head}")
        base += chunk * units[g]
    return lines, chunk, all_rows


def test_chunk_and_plan(check):
    lines, want = [], []
    for depth, cuts in SHAPES:
        for K, length in HEADS:
            _, _, all_rows = _want(depth, cuts, 1, K, length, STAGE)
            for n, stage in [(1, STAGE), (255, STAGE), (1020, STAGE), (1000, 7 * all_rows), (1000, 7 * all_rows - 1), (5, all_rows - 1), (3, 1), (6, 6 * all_rows)]:
                lines.append(f"{depth} {n} {K} {length} {stage} 0 {' '.join(map(str, cuts))}")
                w, chunk, _ = _want(depth, cuts, n, K, length, stage)
                assert chunk == {(1000, 7 * all_rows): 7, (1000, 7 * all_rows - 1): 6, (5, all_rows - 1): 1, (3, 1): 1, (6, 6 * all_rows): 6}.get((n, stage), n)
                want += w
    assert check(lines) == want


def test_the_two_chunk_recipe(check):
    # a MerkleAbsent(4, 65521, 1) row is 65 590 bytes and a MerkleClimb(1) row 97: 1 021 statements a chunk, so 1 030 queries are two chunks
    got = check(["2 1030 4 65521 %d 0 1" % STAGE])
    assert got == ["chunk 1021 14 97 7 2", "seg 0 1 0 4", "seg 1 1 7147 0"]
    assert (64 << 20) // (65590 + 97) == 1021
    # ... and a call of paths at the benchmark's depth with the cut in the middle: a chunk is far more than 1 020 statements
    assert check(["20 1020 0 0 %d 0 10" % STAGE])[0] == "chunk 1020 50 386 25 2"


def _staged(g, b, u):
    return bytes((131 * g + 31 * b + 7 * u + j) & 0xFF for j in range(16))


@pytest.mark.parametrize("K,length", HEADS)
@pytest.mark.parametrize("depth,cuts", [(3, [1]), (3, [1, 2]), (12, [3, 11]), (12, [2])])
def test_spliced_rows(check, depth, cuts, K, length):
    n = 4
    got = check([f"{depth} {n} {K} {length} {STAGE} 1 {' '.join(map(str, cuts))}"])
    head, chunk, _ = _want(depth, cuts, n, K, length, STAGE)
    assert chunk == n and got[: len(head)] == head
    want = []
    for g, (lo, lv) in enumerate(_levels(depth, cuts)):
        for b in range(n):
            found = not K or b % 3 != 2
            row = b"".join(_staged(g, b, u) for u in range(5 + 2 * lv))
            tail = row[64: 64 + 32 * lv + (lv + 7) // 8]
            if g == 0 and K:
                record = bytes(0x40 + j % 64 for j in range(length))
                out = bytes(32) + bytes([0xC0 + b]) * K + (record + tail if found else b"")
            else:
                out = row[:64] + tail if found else bytes(64 + len(tail))
            assert len(out) == (_row_bytes(g, lv, K, length) if found or g else 32 + K)
            want.append(f"row {g} {b} {out.hex()}")
    assert got[len(head):] == want


def test_program_refuses_malformed_input(check):
    for line in ("1 4 0 0 100 0 1", "25 4 0 0 100 0 1", "3 0 0 0 100 0 1", "3 4 0 0 100 0", "3 4 0 0 100 0 0", "3 4 0 0 100 0 3", "3 4 0 0 100 0 2 1", "3 4 4 0 100 0 1",
                 "3 4 0 8 100 0 1", "3 4 0 0 0 0 1", "3 4 0 0 100 2 1", "3"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
