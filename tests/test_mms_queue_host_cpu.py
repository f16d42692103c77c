"""CPU: the slot arithmetic the host and the persistent streaming kernels share (csrc/mms_slots.hpp: mms_item, mms_slots, mms_nblk, mms_slot_valid, mms_flat).

tests/mms_queue_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a program: nothing
is loaded into Python.  For 1 .. 130 tile groups, 2 | 4 | 8 | 16 groups per region with one and two regions, both slot maps and 1 .. 3 row chunks it checks that the valid
indices of the eight per-XCD queues enumerate every (group, tile group, chunk) exactly once and that the order inside a 32-slot block is the static walk's, against the map
written out as nested loops; the count tables are heap arrays of exactly their sizes, so the sanitizer's clean exit bounds every index.  The kernels that draw from the
queues: tests/test_gpu_mmstream_queue.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = 130 * 4 * 2 * 2 * 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("mms_queue_host") / "mms_queue_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", path, os.path.join(ROOT, "tests", "mms_queue_host_check.cpp")], check=True)
    return path


def test_queues_enumerate_every_item_once_in_the_static_order(exe):
    out = subprocess.run([exe], capture_output=True, text=True, check=True)
    assert out.stderr == ""  # (a sanitizer report goes there)
    assert out.stdout == f"ok {CASES}\n"


def test_a_wrong_map_is_reported(exe):
    out = subprocess.run([exe, "spoil"], capture_output=True, text=True)
    assert out.returncode == 1 and "the map differs: tgs 77" in out.stderr
