"""GPU: public inputs -- proofs bound to a statement of lu public wires (include/mfhip.h, mfh_*_public; the reference defines GAMMA_LU 10 in src/lwe.h:26
but fixes l_u = 0, src/snark.c:160).

The pin every test rests on is the composition identity: with the same delta and smudging draws, a public-input proof of (u || w) is
    h, hat_h, hat_v  of mfh_prove on the full bits (u || w)   and   v_w, b_w  of mfh_prove on (0^lu || w),
under either CRS (neither piece reads rows v[0..lu)).  mfh_prove is pinned to the oracle, the Python-integer restatement and the default-size goldens, so the
new entry points are pinned through it.  Independently, a Python-integer restatement of the public-input scheme (Mirror, extended here) must give the same bytes."""
import numpy as np
import pytest

import oracle_lib as ol
from public_mirror import _mirror_public

pytestmark = pytest.mark.gpu

SEED = bytes((29 * i + 3) & 0xFF for i in range(40))
PRG_SEED = 0x5EED0F1A2B3C4D5E


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


def _clear_low(bits, lu):
    b = bytearray(bits)
    for i in range(lu):
        b[i >> 3] &= ~(1 << (i & 7)) & 0xFF
    return bytes(b)


def _instance(ctx, oracle, p, prg, rng):
    """a random_ssp instance (src/ssp.c:37-77): the input bits satisfy it; dense (oracle.ssp_from_tape) or generator-defined"""
    bits = rng.bytes((p.m + 7) // 8)
    if prg:
        d_t = ctx.ssp_prg_make_t(PRG_SEED, bits)
        ctx.ssp_set_prg(PRG_SEED, d_t)
        d_ssp = None
    else:
        tape = rng.integers(0, 256, size=p.m * 8 * p.d, dtype=np.uint8)
        d_ssp = ctx.ssp_upload(oracle.ssp_from_tape(p, tape, bits))
    ctx.ssp_prepare(d_ssp)
    alpha, beta, s = (int(x) for x in rng.integers(1, ol.P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    err = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    return dict(p=p, bits=bits, d_ssp=d_ssp, alpha=alpha, beta=beta, s=s, sk=sk, d_sk=ctx.to_device(sk), d_err=ctx.to_device(err))


def _draws(rng, nb):
    deltas = [int(x) for x in rng.integers(0, ol.P, size=nb, dtype=np.uint64)]
    mags = [rng.integers(0, 256, size=400, dtype=np.uint8).tobytes() for _ in range(nb)]
    signs = [bytes(rng.integers(0, 2, size=5, dtype=np.uint8).tolist()) for _ in range(nb)]
    return deltas, mags, signs


def _composed(ctx, d_crs, d_ssp, lu, bits, delta, mag, sign):
    """the composition identity: (h, hat_h, hat_v) of prove(u || w), (v_w, b_w) of prove(0^lu || w)"""
    import torch

    full = ctx.prove(d_crs, d_ssp, bits, delta, mag, sign).clone().view(5, -1)
    zero = ctx.prove(d_crs, d_ssp, _clear_low(bits, lu), delta, mag, sign).clone().view(5, -1)
    return torch.cat([full[:3], zero[3:]]).reshape(-1)


def _crs_pair(ctx, I, lu):
    plain = ctx.setup(I["d_ssp"], I["alpha"], I["beta"], I["s"], I["d_sk"], I["d_err"]).clone()
    public = ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], lu, I["d_sk"], I["d_err"]).clone()
    return plain, public


# ------------------------------------------------------------------ 1. lu = 0 is the existing API
@pytest.mark.parametrize("prg", [False, True])
def test_lu0_is_the_existing_api(gpu_ctx_factory, oracle, mf, prg):
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(100 + prg)
    I = _instance(ctx, oracle, p, prg, rng)
    d_crs, rows = ctx.setup_image(I["d_ssp"], I["alpha"], I["beta"], I["s"], I["d_sk"], I["d_err"])
    d_crs0, rows0 = ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], 0, I["d_sk"], I["d_err"], image=True)
    assert torch.equal(d_crs, d_crs0) and torch.equal(rows, rows0)
    assert torch.equal(ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], 0, I["d_sk"], I["d_err"]), d_crs)
    nb = 40
    stmts = [I["bits"] if b % 3 else rng.bytes((p.m + 7) // 8) for b in range(nb)]
    deltas, mags, signs = _draws(rng, nb)
    one = ctx.prove(d_crs, I["d_ssp"], stmts[0], deltas[0], mags[0], signs[0]).clone()
    assert torch.equal(ctx.prove_public(d_crs, I["d_ssp"], 0, stmts[0], deltas[0], mags[0], signs[0]), one)
    batch = ctx.prove_batch(d_crs, I["d_ssp"], stmts, deltas, mags, signs).clone()
    assert torch.equal(ctx.prove_batch_public(d_crs, I["d_ssp"], 0, stmts, deltas, mags, signs), batch)
    ok = ctx.verify(I["d_ssp"], I["alpha"], I["beta"], I["s"], I["d_sk"], batch, nb).clone()
    vk = ctx.derive_vk(I["d_ssp"], I["s"], 0)
    assert torch.equal(ctx.verify_public(vk, 0, I["alpha"], I["beta"], I["d_sk"], batch, [b""] * nb), ok)
    assert int(ok.sum()) == sum(1 for b in range(nb) if b % 3)


def test_lu_out_of_range_is_einval(gpu_ctx_factory, oracle, mf):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    I = _instance(ctx, oracle, p, False, np.random.default_rng(7))
    with pytest.raises(mf.MfhError):
        ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], p.m, I["d_sk"], I["d_err"])
    with pytest.raises(mf.MfhError):
        ctx.derive_vk(I["d_ssp"], I["s"], p.m)
    d_crs = ctx.setup(I["d_ssp"], I["alpha"], I["beta"], I["s"], I["d_sk"], I["d_err"])
    with pytest.raises(mf.MfhError):
        ctx.prove_public(d_crs, I["d_ssp"], p.m, I["bits"], 1, bytes(400), bytes(5))
    with pytest.raises(mf.MfhError):
        ctx.prove_batch_public(d_crs, I["d_ssp"], p.m, [I["bits"]], [1], [bytes(400)], [bytes(5)])


# ------------------------------------------------------------------ 2. composition identity, single proof
@pytest.mark.parametrize("d,m,logq,prg", [
    (256, 64, 736, False),    # the reference's debug parameters (src/lwe.h:18-21)
    (256, 64, 736, True),     # ... generator-defined SSP
    (2176, 321, 736, False),  # odd shapes of test_gpu_batch_sizes.py: m - 1 not a multiple of 8
    (64, 16, 1472, False),    # the doubled modulus at reduced D (d % 128 != 0: the VALU witness pass)
    (128, 24, 1472, True),
])
def test_composition_identity_single(gpu_ctx_factory, oracle, mf, d, m, logq, prg):
    import torch

    p = mf.Params(logq=logq, d=d, m=m)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(d * 7 + m + logq + prg)
    I = _instance(ctx, oracle, p, prg, rng)
    for lu in sorted({1, 7, 8, 9, 10, 64, m - 1} & set(range(1, m))):
        plain, public = _crs_pair(ctx, I, lu)
        deltas, mags, signs = _draws(rng, 2)
        for d_crs in (public, plain):
            for b, bits in enumerate((I["bits"], rng.bytes((m + 7) // 8))):  # a satisfying statement and a random one
                got = ctx.prove_public(d_crs, I["d_ssp"], lu, bits, deltas[b], mags[b], signs[b]).clone()
                exp = _composed(ctx, d_crs, I["d_ssp"], lu, bits, deltas[b], mags[b], signs[b])
                assert torch.equal(got, exp), (lu, b)


# ------------------------------------------------------------------ 3. composition identity, batch: every regime of mfh_prove_batch
@pytest.mark.parametrize("regime", ["transient", "resident", "regenerate", "slabs"])
def test_batch_equals_single(gpu_ctx_factory, oracle, mf, regime):
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(300 + ["transient", "resident", "regenerate", "slabs"].index(regime))
    I = _instance(ctx, oracle, p, regime == "regenerate", rng)
    lu = 10
    plain, d_crs = _crs_pair(ctx, I, lu)
    nb = 300  # two super-groups, the second one short
    stmts = []
    for b in range(nb):  # own statement each; every fourth a random input that does not satisfy the SSP (the Euclidean fallback)
        x = bytearray(I["bits"] if b % 4 else rng.bytes((p.m + 7) // 8))
        if b % 4:
            x[0] ^= (b * 37) & 0xFF  # another statement u -- the input then no longer satisfies the SSP either, unless the flip is empty
        stmts.append(bytes(x))
    deltas, mags, signs = _draws(rng, nb)
    image = None
    if regime == "resident":
        image = ctx.crs_expand_mm(d_crs)
        ctx.set_resident_mm(image)
    elif regime == "regenerate":
        ctx.set_batch_image(False)
    elif regime == "slabs":
        ctx.set_batch_slabs(3)
    try:
        got = ctx.prove_batch_public(d_crs, I["d_ssp"], lu, stmts, deltas, mags, signs).clone().view(nb, -1)
    finally:
        ctx.set_resident_mm(None)
        ctx.set_batch_image(True)
        ctx.set_batch_slabs(0)
    for b in range(nb):
        one = ctx.prove_public(d_crs, I["d_ssp"], lu, stmts[b], deltas[b], mags[b], signs[b])
        assert torch.equal(got[b], one), b
    for b in (0, 1, 299):
        assert torch.equal(got[b], _composed(ctx, d_crs, I["d_ssp"], lu, stmts[b], deltas[b], mags[b], signs[b]))


@pytest.mark.parametrize("d,m,logq,lu", [
    (256, 200, 736, 63), (256, 200, 736, 64), (256, 200, 736, 65), (256, 200, 736, 150), (256, 200, 736, 199),
    (192, 150, 736, 10), (192, 150, 736, 100), (192, 150, 736, 149),  # d % 128 != 0: the VALU witness pass, on both sides of the switch
    (64, 16, 1472, 10), (128, 100, 1472, 90),                          # the doubled modulus at reduced D (VALU and matrix-core witness pass)
])
def test_batch_many_public_wires(gpu_ctx_factory, oracle, mf, d, m, logq, lu):
    """above 64 public wires the V step takes their sum from a second witness pass (delta 0); both sides of the switch, up to lu = m - 1, both witness-pass
    forms, and logq 1472"""
    import torch

    p = mf.Params(logq=logq, d=d, m=m)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(lu + d + logq)
    I = _instance(ctx, oracle, p, lu % 2 == 1, rng)
    d_crs = ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], lu, I["d_sk"], I["d_err"])
    nb = 45
    stmts = [I["bits"] if b % 2 else rng.bytes((p.m + 7) // 8) for b in range(nb)]
    deltas, mags, signs = _draws(rng, nb)
    got = ctx.prove_batch_public(d_crs, I["d_ssp"], lu, stmts, deltas, mags, signs).clone().view(nb, -1)
    for b in range(nb):
        assert torch.equal(got[b], _composed(ctx, d_crs, I["d_ssp"], lu, stmts[b], deltas[b], mags[b], signs[b])), b
    vk = ctx.derive_vk(I["d_ssp"], I["s"], lu)
    ok = ctx.to_host(ctx.verify_public(vk, lu, I["alpha"], I["beta"], I["d_sk"], got.reshape(-1), stmts))
    assert [bool(x) for x in ok] == [b % 2 == 1 for b in range(nb)]


# ------------------------------------------------------------------ 4. setup
@pytest.mark.parametrize("prg", [False, True])
def test_setup_public_zeroes_the_public_rows(gpu_ctx_factory, oracle, mf, prg):
    import torch

    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    I = _instance(ctx, oracle, p, prg, np.random.default_rng(400 + prg))
    lu = 10
    plain, public = _crs_pair(ctx, I, lu)
    r0 = 2 * p.d + 1  # row v[0] in stream order
    a, b = ctx.to_host(plain).reshape(-1, p.ctb), ctx.to_host(public).reshape(-1, p.ctb)
    assert np.array_equal(a[:r0], b[:r0]) and np.array_equal(a[r0 + lu:], b[r0 + lu:])
    vk = ctx.to_host(ctx.derive_vk(I["d_ssp"], I["s"], lu), np.uint32)
    q = 1 << (64 * (p.logq // 64))  # modq (src/lwe.h:107-118)
    for i in range(lu):
        diff = (int.from_bytes(a[r0 + i].tobytes(), "little") - int.from_bytes(b[r0 + i].tobytes(), "little")) % q
        assert diff == I["beta"] * int(vk[i + 2]) % ol.P
    dec = ctx.to_host(ctx.decrypt_rows(r0 * p.ctr_ct, lu, I["d_sk"], public[r0 * p.ctb:]), np.uint32)
    assert dec.tolist() == [0] * lu
    crs_img, rows = ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], lu, I["d_sk"], I["d_err"], image=True)
    assert torch.equal(crs_img, public)
    assert torch.equal(rows, ctx.crs_expand(0, 2 * p.d + p.m, public))


# ------------------------------------------------------------------ 5. verifier
def _py_verify(p, vk, alpha, beta, lu, u, dec):
    h_s, hath_s, hatv_s, w_s, b_s = dec
    v_s = (vk[1] + w_s + sum(vk[i + 2] for i in range(lu) if (u[i >> 3] >> (i & 7)) & 1)) % ol.P
    return (h_s * alpha % ol.P == hath_s and v_s * alpha % ol.P == hatv_s and (v_s * v_s - 1 - h_s * vk[0]) % ol.P == 0
            and w_s * beta % ol.P == b_s)


@pytest.mark.parametrize("prg", [False, True])
def test_verifier(gpu_ctx_factory, oracle, mf, prg):
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(500 + prg)
    I = _instance(ctx, oracle, p, prg, rng)
    lu = 10
    d_crs = ctx.setup_public(I["d_ssp"], I["alpha"], I["beta"], I["s"], lu, I["d_sk"], I["d_err"])
    vk = ctx.derive_vk(I["d_ssp"], I["s"], lu)
    # the key against Horner in Python integers, over the materialised SSP
    import torch

    dense = I["d_ssp"] if not prg else torch.cat([ctx.ssp_prg_make_t(PRG_SEED, I["bits"]), ctx.ssp_prg_fill(PRG_SEED, 1, p.m + 2)])
    ssp = ctx.to_host(dense, np.uint32).astype(np.uint64).reshape(p.m + 3, p.d)
    exp = [oracle.poly_eval(ssp[0], I["s"])] + [oracle.poly_eval(ssp[i + 1], I["s"]) for i in range(lu + 1)]
    assert ctx.to_host(vk, np.uint32).tolist() == [int(x) for x in exp]
    u = I["bits"][:2]
    nb = 6
    deltas, mags, signs = _draws(rng, nb)
    proofs = ctx.prove_batch_public(d_crs, I["d_ssp"], lu, [I["bits"]] * nb, deltas, mags, signs).clone()
    stmts = [u, u, bytes([u[0] ^ 1, u[1]]), bytes([u[0], u[1] ^ 2]), u, bytes([u[0], u[1] ^ 0xFC])]  # bits >= lu = 10 of byte 1 are not read
    ok = [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, I["alpha"], I["beta"], I["d_sk"], proofs, stmts))]
    pr = ctx.to_host(proofs, np.uint64).reshape(nb, 5, p.n + 1, p.L)
    pr[4, 1, p.n, 0] ^= np.uint64(1 << 40)  # a tampered proof
    proofs2 = ctx.to_device(pr)
    ok2 = [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, I["alpha"], I["beta"], I["d_sk"], proofs2, stmts))]
    assert ok == [True, True, False, False, True, True]
    assert ok2 == [True, True, False, False, False, True]
    vkh = [int(x) for x in ctx.to_host(vk, np.uint32)]
    for b in range(nb):
        dec = [int(x) for x in ctx.to_host(ctx.decrypt(I["d_sk"], proofs2[b * 5 * p.ct_limbs * 8:], 5), np.uint32)]
        assert _py_verify(p, vkh, I["alpha"], I["beta"], lu, stmts[b], dec) == ok2[b]


# ------------------------------------------------------------------ 6. forgery: why setup zeroes the public rows
def test_forgery_needs_the_public_rows(gpu_ctx_factory, oracle, mf):
    """prove (u || w) with today's prover and claim the all-zero statement: the v_i of the public wires then ride in w.  The plain CRS accepts that;
    the setup_public CRS does not (b_w carries Enc(0) for those rows, eq-lin fails)."""
    p = mf.DEBUG
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(600)
    I = _instance(ctx, oracle, p, False, rng)
    lu = 10
    assert any(_clear_low(I["bits"], lu) != I["bits"] for _ in [0])  # u != 0
    plain, public = _crs_pair(ctx, I, lu)
    vk = ctx.derive_vk(I["d_ssp"], I["s"], lu)
    zero = [bytes((lu + 7) // 8)]
    u = [I["bits"][:2]]
    deltas, mags, signs = _draws(rng, 1)
    verdict = {}
    for name, d_crs in (("plain", plain), ("public", public)):
        forged = ctx.prove(d_crs, I["d_ssp"], I["bits"], deltas[0], mags[0], signs[0])
        verdict[name] = int(ctx.to_host(ctx.verify_public(vk, lu, I["alpha"], I["beta"], I["d_sk"], forged, zero))[0])
        honest = ctx.prove_public(d_crs, I["d_ssp"], lu, I["bits"], deltas[0], mags[0], signs[0])
        assert int(ctx.to_host(ctx.verify_public(vk, lu, I["alpha"], I["beta"], I["d_sk"], honest, u))[0]) == 1
    assert verdict == {"plain": 1, "public": 0}


# ------------------------------------------------------------------ 7. independent restatement in Python integers
PP = ol.P


def test_python_integer_restatement(gpu_ctx_factory, oracle, mf):
    p = mf.DEBUG
    lu = 10
    mi = _mirror_public()(oracle, p)
    rng = np.random.default_rng(700)
    bits = rng.bytes((p.m + 7) // 8)
    tape = rng.integers(0, 1 << 63, size=p.m * p.d, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=p.m * p.d, dtype=np.uint64)
    ssp = oracle.ssp_from_tape(p, tape.view(np.uint8), bits)
    t, v = mi.random_ssp(tape, bits)
    alpha, beta, s = (int(x) for x in rng.integers(1, PP, size=3, dtype=np.uint64))
    sk_l = ol.rand_values(rng, p.n, p.L, p.logq)
    err_l = ol.rand_values(rng, 2 * p.d + p.m, p.L, 559)
    sk, errs = [ol.limbs_to_int(r) for r in sk_l], [ol.limbs_to_int(r) for r in err_l]
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    d_ssp = ctx.ssp_upload(ssp)
    ctx.ssp_prepare(d_ssp)
    d_sk = ctx.to_device(sk_l)
    d_crs = ctx.setup_public(d_ssp, alpha, beta, s, lu, d_sk, ctx.to_device(err_l))
    crs = mi.setup_public(SEED, t, v, alpha, beta, s, sk, errs, lu)
    assert ctx.to_host(d_crs).tobytes() == crs["s"] + crs["as_"] + crs["t"] + crs["v"]
    nb = 6
    stmts = [bits if b % 2 else bytes([bits[0] ^ (b + 1)]) + bits[1:] for b in range(nb)]
    deltas = [int(x) for x in rng.integers(0, PP, size=nb, dtype=np.uint64)]
    sm = [[(rng.bytes(80), int(rng.integers(0, 2))) for _ in range(5)] for _ in range(nb)]
    mags = [b"".join(x[0] for x in smb) for smb in sm]
    signs = [bytes(x[1] for x in smb) for smb in sm]
    one = ctx.to_host(ctx.prove_public(d_crs, d_ssp, lu, stmts[1], deltas[1], mags[1], signs[1]), np.uint64).reshape(5, p.n + 1, p.L)
    batch = ctx.to_host(ctx.prove_batch_public(d_crs, d_ssp, lu, stmts, deltas, mags, signs), np.uint64).reshape(nb, 5, p.n + 1, p.L)
    vk = ctx.derive_vk(d_ssp, s, lu)
    ok = [bool(x) for x in ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, ctx.to_device(batch), [x[:2] for x in stmts]))]
    for b in range(nb):
        exp = mi.prover_public(SEED, crs, t, v, stmts[b], lu, deltas[b], sm[b])
        assert [[ol.limbs_to_int(r) for r in ct] for ct in batch[b]] == exp, b
        if b == 1:
            assert [[ol.limbs_to_int(r) for r in ct] for ct in one] == exp
        assert mi.verifier_public(t, v, alpha, beta, s, sk, lu, stmts[b][:2], exp) == ok[b] == (b % 2 == 1)


# ------------------------------------------------------------------ 8. one full-shape run
def test_full_config4_shape_one_public_proof(gpu_ctx_factory, mf):
    """config 4 (D = 2^20, M = 699 050, generator-defined SSP, as tests/test_gpu_prg_ssp.py builds it): one public proof at lu = 10, accepted, and
    rejected with one statement bit flipped"""
    import torch

    p = mf.Params(d=1 << 20, m=699050)
    ctx = gpu_ctx_factory(p)
    ctx.set_seed(SEED)
    rng = np.random.default_rng(4)
    bits = rng.bytes((p.m + 7) // 8)
    d_t = ctx.ssp_prg_make_t(PRG_SEED, bits)
    ctx.ssp_set_prg(PRG_SEED, d_t)
    ctx.ssp_prepare(None)
    alpha, beta, s = (int(x) for x in rng.integers(1, ol.P, size=3, dtype=np.uint64))
    g = torch.Generator(device=ctx.device)
    g.manual_seed(4)
    sk = torch.randint(-(2 ** 63), 2 ** 63 - 1, (p.n, p.L), dtype=torch.int64, device=ctx.device, generator=g)
    sk[:, p.L - 1] &= (1 << (p.logq - 64 * (p.L - 1))) - 1
    rows = 2 * p.d + p.m
    err = torch.randint(-(2 ** 63), 2 ** 63 - 1, (rows, p.L), dtype=torch.int64, device=ctx.device, generator=g)
    err[:, 8] &= (1 << 47) - 1
    err[:, 9:] = 0
    d_sk = sk.view(torch.uint8).reshape(-1)
    lu = 10
    d_crs = ctx.setup_public(None, alpha, beta, s, lu, d_sk, err.view(torch.uint8).reshape(-1))
    del err
    delta = int(rng.integers(0, ol.P, dtype=np.uint64))
    mags = rng.integers(0, 256, size=400, dtype=np.uint8).tobytes()
    signs = bytes([1, 0, 1, 1, 0])
    proof = ctx.prove_public(d_crs, None, lu, bits, delta, mags, signs)
    vk = ctx.derive_vk(None, s, lu)
    u = bits[:2]
    flipped = bytes([u[0] ^ 0x10, u[1]])
    ok = ctx.to_host(ctx.verify_public(vk, lu, alpha, beta, d_sk, torch.cat([proof, proof]), [u, flipped]))
    assert [int(x) for x in ok] == [1, 0]
    ctx.close()
