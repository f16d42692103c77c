"""CPU: the host side of mfh_merkle_block_keys -- csrc/merkle_block.hpp: the windows of a block's unique keys (block_windows), the walk of the steps over the
running window bytes under both policies (block_plan: statuses, indices, first_update, the update list and the source bytes) and the front of the scratch
(block_layout).

tests/merkle_block_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  It checks the plan against a sequential model that works on the table's bytes, one step at a time: random blocks of
all three kinds in which keys repeat across kinds and every status occurs, with writes of 1, 16, 17 and 39 bytes over the balance, behind it and at the
record's end and expectations that hold, that only the block satisfies and that are stale; crafted blocks -- every status alone and together, a write over the
balance and a transfer that spends it, a compare-and-set that only an earlier adjust satisfies and one an earlier transfer has broken, keys whose windows
have different unit counts side by side in slot order, steps of 0, 1 and 2 updates; the layout against formulas written out literally.  Every array the plan
reads is a heap allocation of exactly its bytes: the sanitizer's clean exit is the bound on what the header reads and writes.  The kernels that produce and
consume what the plan takes and gives: tests/test_gpu_merkle_block.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WRITE_BYTES = [1, 16, 17, 39]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("merkle_block_host") / "merkle_block_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "merkle_block_host_check.cpp")], check=True)

    def run(lines):
        out = subprocess.run([exe], input="".join(line + "\n" for line in lines), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        return out.stdout.split("\n")[:-1]

    return run


def test_random_blocks_of_all_kinds_under_both_policies(check):
    cases = [(wb, mem, nk, 29 * wb + mem + nk) for wb in WRITE_BYTES for mem in (2, 5, 40) for nk in (1, 40, 1200)]
    got = check([f"r {wb} {mem} {nk} {seed}" for wb, mem, nk, seed in cases])
    assert len(got) == len(cases)
    total = fine = 0
    for (wb, mem, nk, _), line in zip(cases, got):
        ok, kind, g_wb, g_mem, g_nk, batches, steps, failed = line.split()
        assert (ok, kind) == ("ok", "r") and (int(g_wb), int(g_mem), int(g_nk)) == (wb, mem, nk), line
        assert int(batches) == 2 and int(steps) == 2 * nk
        total, fine = total + int(steps), fine + int(steps) - int(failed)
    assert 0 < fine < total


def test_crafted_blocks(check):
    for seed in (1, 2, 3):
        assert check([f"c {seed}"]) == ["ok c 18"]


def test_layout_against_literal_formulas(check):
    stage = 64 << 20
    cases = [(1, 1, 16, 100, 1, 0, stage), (24, 500, 19, 300, 3, 2, stage), (257, 4000, 55, 700, 10, 0, stage), (2040, 16320, 55, 1000, 20, 1, stage),
             (300, 300 << 19, 1 << 19, (1 << 19) + 200, 2, 0, stage), (300, 300 << 19, 1 << 19, (1 << 19) + 200, 2, 1, stage), (5, 80, 17, 1 << 27, 4, 3, stage)]
    got = check(["l " + " ".join(str(x) for x in case) for case in cases])
    assert len(got) == len(cases) and all(line.startswith("ok l ") for line in got)
    chunks = [int(line.split()[2]) for line in got]
    assert chunks[0] == 1 and chunks[1] == 24 and chunks[4] == 127 and chunks[6] == 1  # all fit; 127 half-MiB rows fit 64 MiB; one row above the stage


def test_program_refuses_malformed_input(check):
    for line in ("r 0 3 1 1", "r 300 3 1 1", "r 8 1 1 1", "r 8 3 0 1", "r 8 3 5000 1", "c", "l 0 1 16 100 1 0 100", "l 1 1 16 100 1 1 100", "x 1", "r 8 3 1"):
        with pytest.raises(subprocess.CalledProcessError) as e:
            check([line])
        assert e.value.returncode == 2, line
