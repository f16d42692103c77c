"""CPU: public inputs (include/mfhip.h, mfh_*_public).  The new entry points are declared, exported and bound; and in the Python-integer restatement alone
(tests/test_oracle_python_mirror.py's Mirror, extended in tests/test_gpu_public_inputs.py) at tiny parameters, the composition identity the GPU tests rest on
holds, and the forgery that setup_public's zeroed rows exist to stop behaves as stated."""
import os
import re

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import oracle_lib as ol
from public_mirror import _mirror_public

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mfh_setup_public", "mfh_prove_public", "mfh_prove_batch_public", "mfh_vk_derive", "mfh_verify_public"]
PP = ol.P


def test_public_entry_points_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "mfhip.h")).read()
    declared = set(re.findall(r"\b(mfh_[a-z0-9_]+)\s*\(", hdr))
    lib = mf.load_library()
    for name in NEW:
        assert name in declared, name
        assert name in mf.EXPORTS, name
        assert getattr(lib, name).argtypes, name  # load_library gave it a signature
    for meth in ("setup_public", "prove_public", "prove_batch_public", "derive_vk", "verify_public"):
        assert callable(getattr(mf.Context, meth))


SHIM_NEW = ["mfuoco_setup_public", "mfuoco_prover_public", "mfuoco_prover_batch_public", "mfuoco_verifier_public", "mfuoco_verifier_batch_public"]


def test_shim_public_entry_points_declared_and_exported():
    """the reference-signature shim declares the five _public calls and both of its builds export them"""
    import subprocess

    hdr = open(os.path.join(ROOT, "c-lwe-snarks_amd", "host", "include", "mfuoco", "mangiafuoco_api.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # declarations only
    declared = set(re.findall(r"\b(mfuoco_[a-z0-9_]+)\s*\(", hdr))
    for name in SHIM_NEW:
        assert name in declared, name
    for so in ("libmfuoco_gpu.so", "libmfuoco_gpu_debug.so"):
        path = os.path.join(ROOT, "c-lwe-snarks_amd", so)
        if not os.path.exists(path):
            pytest.fail(f"{so} has not been built (make -C c-lwe-snarks_amd shim)")
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.split()
        for name in SHIM_NEW:
            assert name in syms, (so, name)


def _clear_low(bits, lu):
    b = bytearray(bits)
    for i in range(lu):
        b[i >> 3] &= ~(1 << (i & 7)) & 0xFF
    return bytes(b)


@pytest.mark.parametrize("n,d,m,lu", [(33, 64, 9, 3), (33, 64, 9, 8), (40, 32, 20, 10)])
def test_restatement_composition_identity_and_forgery(oracle, n, d, m, lu):
    p = mf.Params(n=n, d=d, m=m)
    mi = _mirror_public()(oracle, p)
    rng = np.random.default_rng(n + d + m + lu)
    seed = rng.bytes(40)
    bits = bytearray(rng.bytes((m + 7) // 8))
    bits[0] |= 1  # u != 0
    bits = bytes(bits)
    tape = rng.integers(0, 1 << 63, size=m * d, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=m * d, dtype=np.uint64)
    t, v = mi.random_ssp(tape, bits)
    alpha, beta, s = (int(x) for x in rng.integers(1, PP, size=3, dtype=np.uint64))
    sk = [ol.limbs_to_int(r) for r in ol.rand_values(rng, n, p.L, p.logq)]
    errs = [ol.limbs_to_int(r) for r in ol.rand_values(rng, 2 * d + m, p.L, 559)]
    delta = int(rng.integers(0, PP, dtype=np.uint64))
    smudges = [(rng.bytes(80), int(rng.integers(0, 2))) for _ in range(5)]
    plain = mi.setup(seed, t, v, alpha, beta, s, sk, errs)
    public = mi.setup_public(seed, t, v, alpha, beta, s, sk, errs, lu)
    # only rows v[0..lu) differ, and they decrypt to 0
    assert (plain["s"], plain["as_"], plain["t"]) == (public["s"], public["as_"], public["t"])
    assert plain["v"][lu * p.ctb:] == public["v"][lu * p.ctb:]
    off = p.ctr_bv
    for i in range(lu):
        ct, off = mi.ct_import(seed, off, public["v"][i * p.ctb:(i + 1) * p.ctb])
        assert mi.decrypt(sk, ct) == 0
    u = bits[:(lu + 7) // 8]
    for crs in (public, plain):
        full = mi.prover(seed, crs, t, v, bits, delta, smudges)["proof"]
        zero = mi.prover(seed, crs, t, v, _clear_low(bits, lu), delta, smudges)["proof"]
        pub = mi.prover_public(seed, crs, t, v, bits, lu, delta, smudges)
        assert pub == full[:3] + zero[3:]
        assert mi.verifier_public(t, v, alpha, beta, s, sk, lu, u, pub)
        flipped = bytes([u[0] ^ 1]) + u[1:]
        assert not mi.verifier_public(t, v, alpha, beta, s, sk, lu, flipped, pub)
    # the forgery: today's prover on (u || w), checked against the all-zero statement
    zero_stmt = bytes(len(u))
    assert mi.verifier_public(t, v, alpha, beta, s, sk, lu, zero_stmt, mi.prover(seed, plain, t, v, bits, delta, smudges)["proof"])
    assert not mi.verifier_public(t, v, alpha, beta, s, sk, lu, zero_stmt, mi.prover(seed, public, t, v, bits, delta, smudges)["proof"])
