"""GPU: the public-input entry points of the reference-signature shim (mfuoco_setup_public, mfuoco_prover_public, mfuoco_prover_batch_public,
mfuoco_verifier_public, mfuoco_verifier_batch_public) driven by c-lwe-snarks_amd/host/test_shim_public.c on one entropy tape: setup_public differs from setup() only
in rows v[0..lu); prover_public is the composition of two prover() calls; the batch is the composition of two mfuoco_prover_batch calls; the verifiers accept
honest proofs and reject a wrong statement and the forgery."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_shim_public_inputs():
    exe = os.path.join(ROOT, "c-lwe-snarks_amd", "host", "test_shim_public")
    if not os.path.exists(exe):
        pytest.fail("host/test_shim_public has not been built (make -C c-lwe-snarks_amd shim); the shim needs gmp.h at build time")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "test_shim_public: ok" in r.stdout
    assert "public verifier checks ok" in r.stdout  # both _public verifiers on constructed proofs: every subset of failing checks
