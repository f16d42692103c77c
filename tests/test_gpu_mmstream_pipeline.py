"""The streaming GEMM's stage pipeline (csrc/evalmm.hip: mmstream_body under k_mmstream1, k_mmstream_p and k_mmstream_pb) at the stage counts where it can go wrong.

The ring of digit-fragment reads runs on from one 256-row stage into the next (LDS buffer X -> Y -> X) and the stage's one barrier sits in the middle of the stage, so what
has to be shown is that no wave ever reads a fragment before every wave has written it, nor overwrites one that is still to be read, at every number of stages an item can
have: 1 (the item is prologue, one stage and the trailing barrier), 2 and 3 (X -> Y, Y -> X), 4, 5, with a ragged last stage (the `ulast` clamp re-reads it) and with several
row chunks (consecutive items of a persistent workgroup, and a clamp per chunk).  The digit dimension K is the region's row count, so small `d` / `m` give few stages.

Every comparison is for EQUALITY OF BYTES against a path that does not stream: set_batch_image(False) (every group regenerates the keystream: k_evalmm16) for the batch
prover, eval_rows (the VALU kernel k_eval) for a single evaluation."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = bytes((11 * i + 3) & 0xFF for i in range(40))


def _statements(rng, p, n, valid_bits):
    nbytes = (p.m + 7) // 8
    bits = [valid_bits if b % 3 != 2 else rng.integers(0, 256, size=nbytes, dtype=np.uint8).tobytes() for b in range(n)]
    deltas = [int(x) for x in rng.integers(0, ol.P, size=n, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(n)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(n)]
    return bits, deltas, mags, signs


class _Batch:
    """an instance of (d, m), `nb` statements, and their proofs from the regenerating path: computed once per module, never changed"""

    def __init__(self, make_ctx, d, m, nb):
        import torch

        import c_lwe_snarks_amd as mf

        sys.path.insert(0, ROOT)
        import bench

        self.torch = torch
        self.p = p = mf.Params(d=d, m=m)
        self.ctx = c = make_ctx(p)
        c.set_seed(SEED)
        inst = bench.build_instance(mf, c, torch, p, 7 * d + m)
        c.ssp_prepare(inst["d_ssp"])
        self.d_ssp = inst["d_ssp"]
        self.d_crs = c.setup(inst["d_ssp"], inst["alpha"], inst["beta"], inst["s"], inst["sk"], inst["err"])
        self.stmts = _statements(np.random.default_rng(d + nb), p, nb, inst["bits"])
        c.set_batch_image(False)
        try:
            self.want = self.prove().clone()
        finally:
            c.set_batch_image(True)

    def prove(self):
        return self.ctx.prove_batch(self.d_crs, self.d_ssp, *self.stmts)


@pytest.fixture(scope="module")
def batches(gpu_ctx_factory):
    made = {}

    def get(d, m, nb):
        if (d, m, nb) not in made:
            made[d, m, nb] = _Batch(gpu_ctx_factory, d, m, nb)
        return made[d, m, nb]

    return get


@pytest.mark.parametrize("d", [256, 512, 1024])
@pytest.mark.parametrize("pack", [True, False])
def test_persistent_grid_items_of_one_two_and_four_stages(batches, d, pack):
    """70 statements = more than one group per region, so the S / AS launch is the persistent grid (k_mmstream_p: 506 tile groups x 4 - 6 groups over 256 workgroups, several
    items per workgroup); d rows = d / 256 stages per item; m = 300: b_w's items have a full and a ragged stage.  Both partial-product forms."""
    b = batches(d, 300, 70)
    b.ctx.set_mm_pack(pack)
    try:
        got = b.prove()
    finally:
        b.ctx.set_mm_pack(True)
    assert b.torch.equal(got, b.want)


@pytest.mark.parametrize("chunk_rows", [256, 500])
def test_persistent_grid_items_that_change_the_chunk(batches, chunk_rows):
    """d = 1024 in chunks of 256 rows (500 is rounded down to whole stages): four one-stage items per (group, tile group), walked chunk by chunk"""
    b = batches(1024, 300, 70)
    b.ctx.set_mm_chunk_rows(chunk_rows)
    try:
        got = b.prove()
    finally:
        b.ctx.set_mm_chunk_rows(0)
    assert b.torch.equal(got, b.want)


@pytest.mark.parametrize("option", ["width16", "rendezvous_sharers", "rendezvous_xcd", "one_workgroup_per_item"])
def test_grid_options(batches, option):
    """the same 70 statements (two stages per item) on 16 workgroups per XCD, with the speed-only rendezvous in front of every item, and as k_mmstream (one workgroup per item)"""
    b = batches(512, 300, 70)
    c = b.ctx
    try:
        if option == "width16":
            c.set_mm_width(16, False)
        elif option == "rendezvous_sharers":
            c.set_mm_stream(1, True, 1, 16)
        elif option == "rendezvous_xcd":
            c.set_mm_stream(1, True, 2, 16)
        else:
            c.set_mm_stream(1, False, 0, 0)
        got = b.prove()
    finally:
        c.set_mm_width(32, False)
        c.set_mm_stream(1, True, 0, 64)
    assert b.torch.equal(got, b.want)


@pytest.mark.parametrize("pack", [True, False])
def test_bw_launch_of_two_super_groups(batches, pack):
    """300 statements = two super-groups, whose b_w runs as ONE launch of one-byte groups (k_mmstream_pb) over the BT+BV region: m = 341 rows, one full and one ragged stage"""
    b = batches(512, 341, 300)
    b.ctx.set_mm_pack(pack)
    try:
        got = b.prove()
    finally:
        b.ctx.set_mm_pack(True)
    assert b.torch.equal(got, b.want)


class _Image:
    """random CRS bytes of a (d, 70) instance, their matrix-core image, coefficient vectors and the VALU path's evaluations over the S region: once per module"""

    NVEC = 5

    def __init__(self, make_ctx, d):
        import c_lwe_snarks_amd as mf

        self.p = p = mf.Params(d=d, m=70)
        self.ctx = c = make_ctx(p)
        c.set_seed(SEED)
        rng = np.random.default_rng(d)
        self.d_crs = c.to_device(rng.integers(0, 256, size=(2 * p.d + p.m) * p.ctb, dtype=np.uint8))
        self.c8 = self.d_crs[: p.d * p.ctb]
        co = rng.integers(0, ol.P, size=(self.NVEC, p.d), dtype=np.uint64).astype(np.uint32)
        co[0, :] = 0xFFFFFFFA  # p - 1 everywhere: the largest digits
        co[1, p.d - 1] = 0xFFFFFFFF  # the last row of the ragged stage counts
        self.d_co = c.to_device(co)
        self.cb = c.to_device(rng.integers(0, 256, size=(7, p.d), dtype=np.uint32))
        self.image = c.crs_expand_mm(self.d_crs)
        self.want = []
        for v in range(self.NVEC):
            ref, _ = c.eval_rows(p.ctr_s, p.d, self.c8, c.to_device(co[v]))
            self.want.append(c.to_host(ref, np.uint64).reshape(p.n + 1, p.L).copy())
        self.want_b = []
        cb = c.to_host(self.cb, np.uint32).reshape(7, p.d)
        for v in (0, 6):
            ref, _ = c.eval_rows(p.ctr_s, p.d, self.c8, c.to_device(cb[v].copy()))
            self.want_b.append(c.to_host(ref, np.uint64).reshape(p.n + 1, p.L).copy())


@pytest.fixture(scope="module")
def images(gpu_ctx_factory):
    made = {}

    def get(d):
        if d not in made:
            made[d] = _Image(gpu_ctx_factory, d)
        return made[d]

    return get


@pytest.mark.parametrize("nrows,chunk_rows", [(700, 0), (1100, 0), (1100, 256), (1100, 500)])
@pytest.mark.parametrize("pack", [True, False])
def test_evaluation_from_a_registered_image(images, nrows, chunk_rows, pack):
    """k_mmstream1 over a registered image: 700 rows = 3 stages, 1100 = 5, the last one ragged (188 / 76 rows: the clamp re-reads it for the prefetches past it); chunks of
    256 rows (500 is rounded down to whole stages) = five one-stage items, the last ragged.  Four-byte vectors and one-byte columns, both partial-product forms."""
    im = images(nrows)
    c, p = im.ctx, im.p
    c.set_resident_mm(im.image)
    c.set_mm_chunk_rows(chunk_rows)
    c.set_mm_pack(pack)
    try:
        got = c.to_host(c.eval_rows_multi(p.ctr_s, nrows, im.c8, im.d_co, im.NVEC), np.uint64).reshape(im.NVEC, p.n + 1, p.L).copy()
        got_b = c.to_host(c.eval_rows_multi(p.ctr_s, nrows, im.c8, im.cb, 7, coeff_bytes=1), np.uint64).reshape(7, p.n + 1, p.L).copy()
    finally:
        c.set_mm_pack(True)
        c.set_mm_chunk_rows(0)
        c.set_resident_mm(None)
    for v in range(im.NVEC):
        assert np.array_equal(got[v], im.want[v]), f"vector {v}"
    for k, v in enumerate((0, 6)):
        assert np.array_equal(got_b[v], im.want_b[k]), f"one-byte column {v}"
