"""CPU: the reference's UNMODIFIED driver sources, compiled with the reference's own headers and linked against libmfuoco_gpu*.so by build()
(oracle/Makefile `drivers`, into oracle/_ref/drivers/) -- the drop-in claim of INTEGRATION.md.  build() fails when one of them does not compile or link;
this checks what it produced: each binary needs the shim library of its size and nothing of the reference's, and every function it imports is defined by
the shim (or libgmp).  Nothing is run (no GPU here).  Skipped where the drivers were not built (no reference sources or gmp.h at build time).
<flint/nmod_poly.h> resolves to the shim's layout-compatible header because FLINT is not installed in this image."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "c-lwe-snarks_amd")
DRV = os.path.join(ROOT, "oracle", "_ref", "drivers")
GMP = "/usr/lib/x86_64-linux-gnu/libgmp.so.10"


def _symbols(args, path):
    out = subprocess.run(["nm", *args, path], capture_output=True, text=True, check=True).stdout
    return [ln.split() for ln in out.splitlines() if ln.strip()]


@pytest.mark.parametrize("prog,ndebug", [("benchmark_snark", True), ("benchmark_lwe", True), ("benchmark_eval", True), ("test_snark", False), ("test_lwe", False),
                                         ("test_entropy", False), ("test_ssp", False), ("test_aes", False)])
def test_reference_driver_links_unchanged(prog, ndebug):
    lib = "mfuoco_gpu" if ndebug else "mfuoco_gpu_debug"
    if not os.path.exists(os.path.join(PKG, f"lib{lib}.so")):
        pytest.skip("shim not built")
    exe = os.path.join(DRV, prog)
    if not os.path.exists(exe):
        pytest.skip(f"oracle/_ref/drivers/{prog} was not built (build() needs the reference sources for it)")
    assert shutil.which("nm") and shutil.which("readelf")
    dyn = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True, check=True).stdout
    needed = [ln.split("[", 1)[1].rstrip("]") for ln in dyn.splitlines() if "(NEEDED)" in ln]
    assert f"lib{lib}.so" in needed, needed
    assert not any("mfuoco_gpu" in n and n != f"lib{lib}.so" for n in needed), needed
    # every reference-library symbol the driver needs is provided by the shim (none by the reference's .c files)
    undefined = {s[-1] for s in _symbols(["-u"], exe) if s[0] == "U" and "@" not in s[-1]}
    defined = {s[-1] for p in (os.path.join(PKG, f"lib{lib}.so"), os.path.join(PKG, "libmfhip.so"), GMP)
               for s in _symbols(["-D", "--defined-only"], p)}
    assert undefined and undefined <= defined, sorted(undefined - defined)
    assert "prover" in undefined or "regev_encrypt2" in undefined or "aesctr_prg" in undefined or "random_ssp" in undefined or "aesctr_init" in undefined
    if prog == "benchmark_eval":  # src/benchmark_eval.c:30-86: D encryptions, then ONE eval_poly over the mapped ./coeffs -- all three from the shim
        assert {"eval_poly", "regev_encrypt2", "ct_export"} <= undefined
