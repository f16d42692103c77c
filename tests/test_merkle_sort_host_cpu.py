"""CPU: the host-compiled half of the device key sort in csrc/merkle_sort.hpp -- mf::kSortTile, mf::load_scratch, mf::check_scratch, mf::merge_slice and
mf::merge_path, the text the kernels k_sort_tiles / k_sort_merge of merkle.hip compile too -- against sizes and merges computed in this file.

tests/merkle_sort_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  The runs, every slice and every output are heap allocations of exactly their sizes, so the sanitizer's clean exit is
the bound on what the partition and a slice's merge read.  The kernels that run on it: tests/test_gpu_merkle_load.py.

1. the scratch layouts for depths 1 .. 24, n in 0, 1, tile - 1, tile, tile + 1 and 2^depth - 1 (and 2^depth, the check's) and key widths 1, 4, 5, 8, 32.
2. the slice of every workgroup of every merge pass over a few n: the slices tile [0, n), lie in one pair of runs, and are the ones computed here.
3. merge_path on every diagonal of two runs of lengths (0, n), (n, 0), (1, 1), (tile, 1), (tile, tile - 1), (7, 300) at KW = 1, 2 and 8 -- random keys with
   many ties in every word, all-equal keys (the tag alone decides), keys that differ in the last word alone -- against a sequential merge (in the program), and
   the merged order against sorted() of the same entries (here).
4. the program refuses malformed input."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [1, 4, 5, 8, 32]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_sort_host") / "merkle_sort_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_sort_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


@pytest.fixture(scope="module")
def tile(check):
    (line,) = check(["tile"])
    t = int(line.split()[1])
    assert line == f"tile {t}" and t >= 64 and t & (t - 1) == 0
    assert 9 * 4 * t <= 64 << 10  # a tile of KW = 8 entries fits the static LDS limit
    return t


def _scratch(tile, depth, n, K):
    kw = (K + 3) // 4
    tiles = (n + tile - 1) // tile
    passes = (tiles - 1).bit_length() if tiles > 1 else 0
    buf = n * (kw + 1) * 4
    load = [0, buf, 2 * buf, 2 * buf + 16]
    nb = ((1 << depth) + 255) // 256
    sizes = [nb * 32, nb * 4, n * 4, n * 2 * kw * 4, 4, buf, buf]  # mask count slots dense total ent0 ent1
    at = [sum(sizes[:i]) for i in range(8)]
    result = (at[7] + 7) // 8 * 8
    digests = (result + 32 + 15) // 16 * 16
    return (f"scratch {tiles} {passes} | " + " ".join(map(str, load)) + f" | {nb} " + " ".join(map(str, at[:7])) + f" {result} {digests} {digests + (32 << depth)}")


def test_scratch_layout(check, tile):
    lines, want = [], []
    for depth in range(1, 25):
        for n in sorted({0, 1, tile - 1, tile, tile + 1, (1 << depth) - 1, 1 << depth}):
            if n > 1 << depth:
                continue
            for K in WIDTHS:
                lines.append(f"scratch {depth} {n} {K}")
                want.append(_scratch(tile, depth, n, K))
    assert check(lines) == want
    # the benchmark shape: 2^20 - 1 keys of 8 bytes -- 1 024 tiles, 10 passes, two buffers of 12 bytes an entry
    if tile == 1024:
        assert check(["scratch 20 1048575 8"])[0].startswith("scratch 1024 10 | 0 12582900 25165800 25165816 | 4096 ")


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5123, 8191, (1 << 20) - 1])
def test_merge_slices(check, tile, n):
    tiles = (n + tile - 1) // tile
    run = tile
    while True:  # every pass that a sort of n entries makes, and one beyond (a single run: the pass copies)
        lines = [f"slice {n} {run} {g}" for g in range(tiles)]
        got = [tuple(int(x) for x in line.split()[1:]) for line in check(lines)]
        at = 0
        for g, (out0, count, a_at, na, nb, d0) in enumerate(got):
            base = g * tile // (2 * run) * 2 * run
            mid, end = min(base + run, n), min(base + 2 * run, n)
            assert (out0, a_at, na, nb, d0) == (g * tile, base, mid - base, end - mid, g * tile - base), (n, run, g)
            assert out0 == at and 1 <= count <= tile and out0 + count <= end
            at += count
        assert at == n
        if run >= n:
            break
        run *= 2


def _lcg(state):
    state[0] = (state[0] * 1103515245 + 12345) & 0x7FFFFFFF
    return state[0] >> 16


def _merged_hash(kw, na, nb, mode, seed):
    """the program's two runs made again here; their merge is sorted() of all entries (the tags differ: a total order); FNV-1a over the tags"""
    total, state, entries = na + nb, [seed], []
    for i in range(total):
        key = tuple(_lcg(state) % 3 if mode == 0 else 0x01020304 if mode == 1 else (_lcg(state) % 5 if j == kw - 1 else 0xAAAAAAAA) for j in range(kw))
        entries.append(key + (total - 1 - i,))
    h = 2166136261
    for e in sorted(entries):
        h = ((h ^ e[-1]) * 16777619) & 0xFFFFFFFF
    return h


@pytest.mark.parametrize("kw", [1, 2, 8])
def test_merge_path(check, tile, kw):
    lines, want = [], []
    for na, nb in ((0, 5), (0, tile), (5, 0), (tile, 0), (1, 1), (tile, 1), (tile, tile - 1), (7, 300)):
        for mode in (0, 1, 2):
            for step in sorted({1 if na + nb < 400 else 97, tile}):
                seed = 1000 * kw + 10 * mode + na % 7
                lines.append(f"merge {kw} {na} {nb} {mode} {seed} {step}")
                want.append(f"merge {na + nb} {max(1, (na + nb + step - 1) // step)} {_merged_hash(kw, na, nb, mode, seed)}")
    assert check(lines) == want


def test_program_refuses_malformed_input(check):
    for line in ("scratch 0 4 4", "scratch 25 4 4", "scratch 3 9 4", "scratch 3 4 0", "scratch 3 4 33", "scratch 3 4", "scratch 3 -1 4", "tile 1", "slice 5 1000 0",
                 "slice 5 1024 1", "slice 0 1024 0", "merge 0 1 1 0 1 1", "merge 9 1 1 0 1 1", "merge 1 1 1 3 1 1", "merge 1 1 1 0 1 0", "merge 1 1 1 0 1", "merge 1 x 1 0 1 1",
                 "order 1 2 3", "merge"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
