"""bench.py's plain run on one GPU: the headline alone.  It times its steps, writes --dump-outputs and prints ONE line in which every leg and check
that only --full runs is null (the N > 1 --full run is tests/test_gpu_rccl.py's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("setup_s", "setup_enc_per_s", "lwe_enc_per_s", "lwe", "lwe_decrypt", "lwe_dec_per_s", "single_proof", "cpu_baseline", "reference_typed_api",
             "regenerate_per_group_batch", "resident_crs_batch", "call_of_twice_the_statements", "mixed_witnesses", "device_verifier_proofs_per_s",
             "row_sharded_batch", "single_proof_row_sharded")


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(tmp_path):
    import c_lwe_snarks_amd as mf

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "62",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout[-2000:]
    js = json.loads(lines[0])
    assert js["metric"] == "snark_proofs_per_sec" and js["unit"] == "proofs/s" and js["higher_is_better"] is True
    assert js["full"] is False and js["mode"] == "batch" and js["steps"] == 2 and js["warmup"] == 1
    assert js["value"] > 0 and abs(js["value"] * js["ms_per_step"] / 1e3 - 62) < 1e-6 * 62
    assert js["proof_accepted"] is None
    assert [k for k in FULL_ONLY if js[k] is not None] == []
    sums = np.load(out / "proof_ct_word_sums.npy")
    proofs = np.load(out / "proofs.npy")
    assert sums.shape == (62, 5) and proofs.shape == (32, 5, 2 * mf.DEFAULT.ct_limbs)
    assert np.array_equal(proofs.sum(axis=2), sums[np.load(out / "proof_statements.npy").astype(np.int64)])
