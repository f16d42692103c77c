"""GPU: the witness pass as the batch prover's streaming GEMM over the SSP image (csrc/witness.hip: k_ssp_image, mfh_witness_poly_stream; csrc/evalmm.hip:
mms_plan_ssp, k_witness_stream_finish) against exact integers.

    w_b[k] = delta_b t[k] + sum_{i = 1 .. m - 1} bit_b[i - 1] v_i[k]  mod p

Every case compares all nstmt x d coefficients with tests/witness_ref.py (the exact-integer reference of tests/test_gpu_witness_exact.py, at that file's reduced
parameters) and, where mfh_witness_poly_mm takes the shape (d % 128 == 0), with its result as well.  The SSP is the A operand here: rows 0 .. m - 1 of the K dimension
are slots 1 .. m, padded to 256-row stages, and the witness bits are digit columns in groups of 255 statements:
  statements  1 and 255 are one group (k_mmstream1), 256 and 300 two and 1020 four (the persistent grid: the claim log must show the launch and every item once);
  m - 1       1, 255, 256, 257: one row beside v_0, the last row of a stage, the first of the next one, and one more;
  d           64 and 128: one and two tile groups of 16 row tiles;
  row chunks  forced with mfh_set_mm_chunk_rows(ctx, 256): the epilogue sums the records of 1 .. 2 chunks.
Statement 0 is all-zero, statement 1 all 0xFF bytes (padding bits set), delta_0 = 0, delta_1 = p - 1."""
import functools

import numpy as np
import pytest

import witness_ref as wr

pytestmark = pytest.mark.gpu
P = wr.P

NSTMT = [1, 255, 256, 300, 1020]
ROWS = [1, 255, 256, 257]  # m - 1


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@functools.lru_cache(maxsize=None)
def random_ssp(m, d, seed=0):
    a = np.random.default_rng([m, d, seed]).integers(0, P, size=(m + 3, d), dtype=np.uint64).astype(np.uint32)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def case(m, d, nstmt):
    """(bits, deltas, expected w) of a shape: computed once, shared by the tests that need it, never changed"""
    rng = np.random.default_rng([d, m, nstmt])
    nbytes = (m + 6) // 8
    bits = [bytes(nbytes), b"\xff" * nbytes][:nstmt] + [rng.bytes(nbytes) for _ in range(nstmt - 2)]
    deltas = [0, P - 1][:nstmt] + [int(x) for x in rng.integers(0, P, size=max(0, nstmt - 2), dtype=np.uint64)]
    want = wr.w_polys(random_ssp(m, d), bits, deltas, m)
    want.flags.writeable = False
    return bits, deltas, want


def assert_exact(got, want, what):
    got = np.asarray(got).view(np.uint32).reshape(want.shape).astype(np.uint64)
    if np.array_equal(got, want):
        return
    bad = got != want
    b, k = (int(x) for x in np.argwhere(bad)[0])
    raise AssertionError(f"{what}: first difference at statement {b}, k = {k}: got {int(got[b, k]):#010x}, want {int(want[b, k]):#010x} "
                         f"({int(bad.sum())} of {want.size} coefficients differ, in {int(bad.any(axis=1).sum())} of {want.shape[0]} statements)")


def stream(c, d_ssp, bits, deltas):
    return c.to_host(c.witness_poly_many(d_ssp, bits, deltas, mm="stream"), np.uint32)


def logged(c, d_ssp, bits, deltas):
    """the streamed pass with the claim log on -> (w, the logged persistent launches, the log's words)"""
    import torch

    log = torch.zeros(1 << 16, dtype=torch.int32, device=c.device)
    c.set_mm_claim_log(log)
    try:
        got = stream(c, d_ssp, bits, deltas)
        torch.cuda.synchronize()
        descs = c.mm_claim_log_launches()
    finally:
        c.set_mm_claim_log(None)
    return got, descs, log.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("nstmt", NSTMT)
def test_streamed_pass_is_exact(gpu_ctx_factory, mf, nstmt, rows, d):
    m = rows + 1
    bits, deltas, want = case(m, d, nstmt)
    ngroups = (nstmt + 254) // 255
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = c.ssp_upload(random_ssp(m, d).astype(np.uint64).reshape(-1))
        got, descs, words = logged(c, d_ssp, bits, deltas)
        assert_exact(got, want, f"streamed pass, {ngroups} group(s)")
        if ngroups == 1:
            assert descs == []  # one group: k_mmstream1, one workgroup per item
        else:
            # 2 and 4 groups divide 32: the persistent grid, one launch of one-byte columns whose every item (d / 64 tile groups x groups) was taken once
            assert [(l["ngt"], l["coeff_bytes"], l["tgs"], l["nchunks"]) for l in descs] == [(ngroups, 1, d // 64, 1)]
            l = descs[0]
            counts = words[l["offset"]:l["offset"] + 2 * l["nchunks"] * 8 * l["nblk"] * 32].reshape(-1, 2)[:, 0]
            assert int(counts.sum()) == ngroups * (d // 64) and int(counts.max()) == 1
        if d % 128 == 0:
            for b0 in range(0, nstmt, 256):
                mm = c.to_host(c.witness_poly_many(d_ssp, bits[b0:b0 + 256], deltas[b0:b0 + 256], mm=True), np.uint32)
                assert_exact(mm, want[b0:b0 + 256], f"mfh_witness_poly_mm, statements from {b0}")
        # several row chunks: 256 rows each, so m = 257 and 258 take two
        c.set_mm_chunk_rows(256)
        try:
            got, descs, _ = logged(c, d_ssp, bits, deltas)
        finally:
            c.set_mm_chunk_rows(0)
        assert_exact(got, want, f"streamed pass in chunks of 256 rows, {ngroups} group(s)")
        assert ngroups == 1 or [l["nchunks"] for l in descs] == [(m + 255) // 256]
    finally:
        c.close()


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("nstmt", [255, 300])
def test_largest_sum(gpu_ctx_factory, mf, nstmt, d):
    """every coefficient of t and of every v_i is p - 1 and every delta p - 1; the all-ones statement then sums (m - 1)(p - 1) per coefficient, the largest
    value the epilogue reduces; the closed form cnt_b (p - 1) + (p - 1)^2 mod p stands beside the reference"""
    m = 258
    ssp = np.full((m + 3, d), P - 1, dtype=np.uint32)
    rng = np.random.default_rng([d, nstmt, 1])
    nbytes = (m + 6) // 8
    bits = [b"\xff" * nbytes, bytes(nbytes)] + [rng.bytes(nbytes) for _ in range(nstmt - 2)]
    deltas = [P - 1] * nstmt
    want = wr.w_polys(ssp, bits, deltas, m)
    cnt = wr.bit_matrix(bits, m).sum(axis=1)
    assert int(cnt[0]) == m - 1 and int(cnt[1]) == 0
    for b in (0, 1, nstmt - 1):
        assert {int(x) for x in want[b]} == {(int(cnt[b]) * (P - 1) + (P - 1) * (P - 1)) % P}
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp = c.ssp_upload(ssp.astype(np.uint64).reshape(-1))
        assert_exact(stream(c, d_ssp, bits, deltas), want, "streamed pass, every coefficient p - 1")
        c.set_mm_chunk_rows(256)
        try:
            assert_exact(stream(c, d_ssp, bits, deltas), want, "streamed pass, every coefficient p - 1, two row chunks")
        finally:
            c.set_mm_chunk_rows(0)
    finally:
        c.close()


def test_a_second_ssp_in_the_same_context(gpu_ctx_factory, mf):
    """the image is a function of the SSP: after a second upload -- into a new buffer, and over the first one in place -- the pass must see the new rows"""
    d, m, nstmt = 128, 258, 300
    bits, deltas, want0 = case(m, d, nstmt)
    ssp1 = random_ssp(m, d, seed=1)
    want1 = wr.w_polys(ssp1, bits, deltas, m)
    assert not np.array_equal(want0, want1)
    c = gpu_ctx_factory(mf.Params(d=d, m=m))
    try:
        d_ssp0 = c.ssp_upload(random_ssp(m, d).astype(np.uint64).reshape(-1))
        assert_exact(stream(c, d_ssp0, bits, deltas), want0, "first SSP")
        d_ssp1 = c.ssp_upload(ssp1.astype(np.uint64).reshape(-1))
        assert_exact(stream(c, d_ssp1, bits, deltas), want1, "second SSP, its own buffer")
        assert_exact(stream(c, d_ssp0, bits, deltas), want0, "first SSP again")
        c.ssp_upload(ssp1.astype(np.uint64).reshape(-1), d_ssp=d_ssp0)  # same address, new contents: only the upload can tell
        assert_exact(stream(c, d_ssp0, bits, deltas), want1, "second SSP uploaded over the first one's buffer")
    finally:
        c.close()
