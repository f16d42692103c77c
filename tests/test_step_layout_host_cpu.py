"""CPU: mf::step_layout (csrc/merkle_rows.hpp), the one function that lays out the front of the device scratch and sizes the chunk of every batch of key
steps -- two record updates a step (insert, remove, transfer) or one (adjust, write).

tests/step_layout_host_check.cpp (a program with its own main that includes the header) is compiled with g++ -O1 -fsanitize=address,undefined and run as a
program: nothing is loaded into Python.  It compares every field of the layout with the formulas the two-record driver and the two one-record calls each
used to write out by hand, restated literally in the program, over nk in {1, 2, 1020, 4097}, lengths 9 .. 64, key sizes 1, 4 and 32, payloads of 0, 1, 8 and
39 bytes, uncut and cut paths at depths 1, 10 and 24, and stages that hold many rows, a few, and less than one.  The kernels that run inside that layout:
tests/test_gpu_merkle_insert.py, _remove.py, _transfer.py, _adjust.py, _write.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_step_layout_is_the_two_drivers_formulas(tmp_path):
    exe = str(tmp_path / "step_layout_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "step_layout_host_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.stderr == ""  # (a sanitizer report goes there)
    assert out.returncode == 0, out.stdout
    # 7 (depth, cuts) pairs x 4 nk x 11 (length, K) pairs x 4 payloads x 3 stages
    assert out.stdout == "ok 3696\n"
