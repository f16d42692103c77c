"""CPU: the host half of the range reads in csrc/merkle_range.hpp -- mf::range_scratch, mf::range_result_bytes, mf::range_status and mf::words_to_key --
against sizes and verdicts computed in this file.

tests/merkle_range_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  The links' words, the bounds' words and the bytes written back are heap allocations of exactly their sizes, so the
sanitizer's clean exit is the bound on what the chain check reads.  The kernels that fill those words: tests/test_gpu_merkle_range.py.

1. the scratch layout for depths 1 .. 24, max_links 0 .. 2^16 and key widths 1, 4, 5, 8, 32: mask | count | slots | dense | total | order | okeys.
2. range_status at key widths 1, 4, 5, 8 and 32 on chains that are good (1, 2 and 7 links), have a gap, overlap, are empty, have the first lo >= a (equal and
   above) or the last hi <= b (equal and below) -- with the first failing link -- and the keys round-trip through their words.
3. the program refuses malformed input."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 4, 5, 8, 32]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_range_host") / "merkle_range_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_range_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def _scratch(depth, max_links, K):
    nb = ((1 << depth) + 255) // 256
    kw = (K + 3) // 4
    sizes = [nb * 4 * 8, nb * 4, max_links * 4, max_links * 2 * kw * 4, 4, max_links * 4, max_links * 2 * kw * 4]  # mask count slots dense total order okeys
    at = [sum(sizes[:i]) for i in range(8)]
    return f"scratch {nb} " + " ".join(map(str, at)) + f" {4 + sizes[5] + sizes[6]}"


def test_scratch_layout(check):
    lines, want = [], []
    for depth in (1, 3, 8, 9, 12, 19, 20, 24):
        for max_links in (0, 1, 255, 1020, 4096, 1 << 16):
            for K in WIDTHS:
                lines.append(f"scratch {depth} {max_links} {K}")
                want.append(_scratch(depth, max_links, K))
    assert check(lines) == want
    # the benchmark table: 2^20 records of 8-byte keys, 1 020 links -- 128 KiB of masks, 16 KiB of counts, 16 B a link's keys
    assert check(["scratch 20 1020 8"]) == [f"scratch 4096 0 131072 147456 151536 167856 167860 171940 188260 {4 + 4080 + 16320}"]


def _chain(rng, K, n):
    """n + 1 ascending keys, none a sentinel, with room between neighbours where the width allows"""
    top = (1 << (8 * K)) - 1
    if K == 1:
        values = sorted(int(v) for v in rng.choice(np.arange(2, top - 1, 3), size=n + 1, replace=False))
    else:
        values = sorted({int.from_bytes(rng.bytes(K), "big") | 4 for _ in range(4 * (n + 1))} - {top})[: n + 1]
    assert len(values) == n + 1
    return values


def _line(K, a, b, links):
    hexed = lambda v: v.to_bytes(K, "big").hex()
    return f"status {K} {hexed(a)} {hexed(b)} {len(links)} " + " ".join(hexed(lo) + " " + hexed(hi) for lo, hi in links)


@pytest.mark.parametrize("K", WIDTHS)
def test_range_status(check, K):
    rng = np.random.default_rng(12000 + K)
    cases = []  # (a, b, links, status, first)
    for n in (1, 2, 7):
        v = _chain(rng, K, n)
        links = list(zip(v, v[1:]))
        a, b = v[0] + 1, v[-1] - 1
        cases.append((a, b, links, 0, 0))
        cases.append((a, a, links, 0, 0))
        cases.append((v[0], b, links, 2, 0))           # the first lo == a
        cases.append((v[0] - 1, b, links, 2, 0))       # the first lo > a
        cases.append((a, v[-1], links, 2, n - 1))      # the last hi == b
        cases.append((a, v[-1] + 1, links, 2, n - 1))  # the last hi < b
        if n >= 2:
            for at in sorted({1, n - 1}):
                gap = [list(x) for x in links]
                gap[at][0] += 1                          # a gap in front of link `at`
                cases.append((a, b, [tuple(x) for x in gap], 2, at))
                over = [list(x) for x in links]
                over[at][0] -= 1                         # link `at` overlaps the one before
                cases.append((a, b, [tuple(x) for x in over], 2, at))
    cases.append((5, 9, [], 2, 0))                      # no link at all
    lines = [_line(K, a, b, links) for a, b, links, _, _ in cases]
    got = check(lines)
    assert len(got) == 2 * len(cases)
    for i, (a, b, links, status, first) in enumerate(cases):
        assert got[2 * i] == f"status {status} {first}", (i, lines[i])
        assert got[2 * i + 1] == ("keys " + "".join(lo.to_bytes(K, "big").hex() + hi.to_bytes(K, "big").hex() for lo, hi in links)), i
    # keys that differ in their LAST byte alone: a partial last word is compared, and no byte behind it
    if K > 1:
        base = int.from_bytes(bytes([0x80] * (K - 1)) + b"\x00", "big")
        assert check([_line(K, base + 2, base + 2, [(base + 1, base + 3)])])[0] == "status 0 0"
        assert check([_line(K, base + 1, base + 2, [(base + 1, base + 3)])])[0] == "status 2 0"
        assert check([_line(K, base + 2, base + 3, [(base + 1, base + 3)])])[0] == "status 2 0"


def test_program_refuses_malformed_input(check):
    for line in ("scratch 0 4 4", "scratch 25 4 4", "scratch 3 65537 4", "scratch 3 4 0", "scratch 3 4 33", "scratch 3 4", "status 4 00000001 00000002 1 00000000",
                 "status 4 000001 00000002 0", "status 4 00000001 00000002 1 00000000 000000", "status 0 00 00 0", "order 1 2 3", "status"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
