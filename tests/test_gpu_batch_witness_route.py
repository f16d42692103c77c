"""GPU: mfh_prove_batch with the witness pass of the whole call as one streaming launch over the SSP image (mfh_set_batch_witness, the default) against the same call
with k_witness_mm8q per super-group: the proofs bit for bit, 300 statements (two super-groups, 255 + 45) and 810 (four, 3 x 255 + 45), item queues and static walk.
The route is a tuning choice, so the timing kind of its launch ("mmstream_witness") is what shows that it was taken -- once per call with the route on, never with it off.
Instance as in tests/test_gpu_mmstream_queue.py: d = 512, m = 341 (b_w and the witness pass over 341 rows: two 256-row stages)."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes((29 * i + 3) & 0xFF for i in range(40))
D, M = 512, 341


@pytest.fixture(scope="module")
def inst(gpu_ctx_factory):
    """context, SSP, CRS and 810 statements (every third one a random, unsatisfying assignment): made once, read-only"""
    import torch

    import c_lwe_snarks_amd as mf

    sys.path.insert(0, ROOT)
    import bench

    p = mf.Params(d=D, m=M)
    c = gpu_ctx_factory(p)
    c.set_seed(SEED)
    i = bench.build_instance(mf, c, torch, p, 7 * D + M)
    c.ssp_prepare(i["d_ssp"])
    d_crs = c.setup(i["d_ssp"], i["alpha"], i["beta"], i["s"], i["sk"], i["err"])
    rng = np.random.default_rng(810)
    n, nbytes = 810, (p.m + 7) // 8
    bits = [i["bits"] if b % 3 != 2 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for b in range(n)]
    deltas = [int(x) for x in rng.integers(0, ol.P, size=n, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(n)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(n)]
    return c, i["d_ssp"], d_crs, (bits, deltas, mags, signs), torch


def prove(inst, nb, streamed, queue):
    c, d_ssp, d_crs, stmts, torch = inst
    c.set_batch_witness(streamed)
    c.set_mm_queue(queue, 0, -8)
    c.set_timing(True)
    try:
        c.timing_drain("mmstream_witness")
        got = c.prove_batch(d_crs, d_ssp, *(x[:nb] for x in stmts)).clone()
        torch.cuda.synchronize()
        launches = c.timing_drain("mmstream_witness")[0]
    finally:
        c.set_timing(False)
        c.set_mm_queue(1, 0, -8)
        c.set_batch_witness(True)
    return got, launches


@pytest.mark.parametrize("nb", [300, 810])
def test_route_on_equals_route_off(inst, nb):
    torch = inst[4]
    want, n_off = prove(inst, nb, False, 1)
    assert n_off == 0
    for queue in (1, 0):
        got, n_on = prove(inst, nb, True, queue)
        assert n_on == 1, "the streamed witness pass was not taken"
        assert torch.equal(got, want), f"{nb} statements, queue mode {queue}: the proofs differ"
    # and the route off again after it was on (the W areas and the SSP image stay behind: nothing of them may leak into the other route)
    again, n_off = prove(inst, nb, False, 0)
    assert n_off == 0 and torch.equal(again, want)
