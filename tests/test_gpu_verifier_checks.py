"""GPU: the device verifier (csrc/snark.hip: verify_checks under k_verify / mfh_verify and k_verify_public / mfh_verify_public) pinned by proofs built by
construction, not by the prover: ciphertexts whose decryptions the test chooses (tests/verifier_ref.py), so that each of the four checks of verifier()
(src/snark.c:219-235) fails alone and in every combination, at the edges of the field (v_s = 0, +-1, v_0(s) + w_s wrapping past p, t(s) = 0, alpha / beta / s in
{0, 1, p - 1}), at known positions of a batch, and on both sides of the 819 / 820 proofs at which the automatic decrypt path changes kernels.  Every verdict is
compared exactly with verifier_ref.checks, which tests/test_verifier_ref_cpu.py pins against the oracle's verifier()."""
import ctypes
import types

import numpy as np
import pytest

import oracle_lib as ol
import verifier_ref as vr

pytestmark = pytest.mark.gpu

P = ol.P
SEED = bytes((37 * i + 11) & 0xFF for i in range(40))
PRG_SEED = 0x0F1E2D3C4B5A6978
EINVAL = -1


@pytest.fixture(scope="module")
def mf():
    import c_lwe_snarks_amd as m

    return m


@pytest.fixture(scope="module")
def env(gpu_ctx_factory, mf):
    """env(logq): one context, key and shared a (with its dot product, formed once) per modulus at d = 256, m = 64 (mf.DEBUG at logq 736)"""
    cache = {}

    def get(logq=736):
        if logq not in cache:
            p = mf.Params(logq=logq, d=256, m=64)
            ctx = gpu_ctx_factory(p)
            ctx.set_seed(SEED)
            rng = np.random.default_rng(logq)
            sk = ol.rand_values(rng, p.n, p.L, p.logq)
            cache[logq] = types.SimpleNamespace(p=p, ctx=ctx, rng=rng, sk=sk, d_sk=ctx.to_device(sk), shared=vr.shared_a(p, sk, rng))
        return cache[logq]

    return get


def _bits(ctx, t):
    return [int(x) for x in ctx.to_host(t, np.uint8)]


def _same(got, want, rows, what):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f"{what}: {len(bad)} verdicts differ; first at proof {bad[0]}: got {got[bad[0]]}, values {rows[bad[0]]}"


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _on_both_paths(ctx, fn):
    """fn(path) with the VALU k_decrypt (1), then with k_decrypt_mm (2); the context goes back to choosing by batch size"""
    for path in (1, 2):
        ctx.set_decrypt_path(path)
        try:
            fn(path)
        finally:
            ctx.set_decrypt_path(0)


def _run_matrix(E, d_ssp, s, alpha, beta, t_s, v0_s):
    """the matrix of failing checks at (t_s, v0_s) through mfh_verify and mfh_verify_public(lu = 0) on both decrypt kernels"""
    ctx = E.ctx
    rows = list(vr.matrix(t_s, v0_s, alpha, beta, vr.w_list(v0_s)))
    want = [int(vr.accept(*v, t_s, (v0_s + v[3]) % P, alpha, beta)) for v, _ in rows]
    assert want == [int(not f) for _, f in rows] and len(rows) == (112 if t_s else 56)
    d_proofs = ctx.to_device(vr.craft_batch(E.p, E.sk, [v for v, _ in rows], E.rng, E.shared))
    vk = ctx.derive_vk(d_ssp, s, 0)
    assert [int(x) for x in ctx.to_host(vk, np.uint32)] == [t_s, v0_s], "t(s), v_0(s) differ from Horner in Python integers"

    def both(path):
        got = _bits(ctx, ctx.verify(d_ssp, alpha, beta, s, E.d_sk, d_proofs, len(rows)))
        _same(got, want, rows, f"mfh_verify, decrypt path {path}")
        pub = _bits(ctx, ctx.verify_public(vk, 0, alpha, beta, E.d_sk, d_proofs, [b""] * len(rows)))
        _same(pub, want, rows, f"mfh_verify_public, decrypt path {path}")
        assert got == pub

    _on_both_paths(ctx, both)


# ------------------------------------------------------------------ a. the matrix through both kernels
@pytest.mark.parametrize("logq,name", [(736, n) for n in sorted(vr.PARAM_SETS)] + [(1472, "random")])
def test_matrix_through_both_kernels(env, logq, name):
    """all 16 subsets of failing checks x 7 w_s at the field's edges = 112 proofs in one call (56 with t(s) = 0, where v_s alone decides eq-div), ciphertexts of
    the four crafted kinds spread over the five positions; k_decrypt and k_decrypt_mm under k_verify and k_verify_public"""
    E = env(logq)
    s, alpha, beta, t, v0 = vr.instance(E.p, name, E.rng)
    d_ssp = E.ctx.ssp_upload(vr.ssp_with(E.p, t, v0))
    _run_matrix(E, d_ssp, s, alpha, beta, vr.horner(t, s), vr.horner(v0, s))


# ------------------------------------------------------------------ b. SSP sources
def test_matrix_under_the_generator_ssp(env, gpu_ctx_factory):
    """mfh_verify(d_ssp = NULL) with a generator-defined SSP: k_eval_slots01 reads slot 0 from the registered t and generates slot 1"""
    E = env(736)
    ctx = gpu_ctx_factory(E.p)
    ctx.set_seed(SEED)
    t = E.rng.integers(0, P, size=E.p.d, dtype=np.uint64)
    d_t = ctx.to_device(t.astype(np.uint32))
    ctx.ssp_set_prg(PRG_SEED, d_t)
    v0 = ctx.to_host(ctx.ssp_prg_fill(PRG_SEED, 1, 1), np.uint32)
    s, alpha, beta = vr.PARAM_SETS["random"]
    F = types.SimpleNamespace(**{**vars(E), "ctx": ctx, "d_sk": ctx.to_device(E.sk)})
    try:
        _run_matrix(F, None, s, alpha, beta, vr.horner(t, s), vr.horner(v0, s))
    finally:
        ctx.close()  # (a context of its own, so that the registration cannot reach another test: freed here, not at the end of the session)


def test_matrix_under_a_row_ssp(env, gpu_ctx_factory):
    """mfh_verify(d_ssp = NULL) with a registered row SSP: slots 0 and 1 come from its dense prefix (ssp_rows_fill materialises the same slots)"""
    E = env(736)
    ctx = gpu_ctx_factory(E.p)
    ctx.set_seed(SEED)
    # 200 rows of one to four random (wire, coefficient) entries, each with a constant term as well (wire 0: v_0 is no trivial polynomial)
    rows = [[(int(w), int(c)) for w, c in zip(E.rng.integers(0, E.p.m, size=k), E.rng.integers(0, P, size=k))] + [(0, int(E.rng.integers(0, P)))]
            for k in E.rng.integers(1, 5, size=200)]
    ctx.ssp_set_rows(rows, lu_max=0)
    try:
        slots = ctx.to_host(ctx.ssp_rows_fill(0, 2), np.uint32).reshape(2, E.p.d)
        s, alpha, beta = vr.PARAM_SETS["random"]
        F = types.SimpleNamespace(**{**vars(E), "ctx": ctx, "d_sk": ctx.to_device(E.sk)})
        _run_matrix(F, None, s, alpha, beta, vr.horner(slots[0], s), vr.horner(slots[1], s))
    finally:
        ctx.ssp_set_rows(None)
        ctx.close()


# ------------------------------------------------------------------ c. public statements
def _statements(lu, rng):
    ub = max(1, (lu + 7) // 8)

    def of(bits):
        return sum(1 << i for i in bits).to_bytes(ub, "little")

    out = [of([]), of(range(lu))] + [of([i]) for i in sorted({0, 7, 8, lu - 1}) if 0 <= i < lu]
    return out + [(int.from_bytes(rng.bytes(ub), "little") & ((1 << lu) - 1)).to_bytes(ub, "little")]


def _xor(u, mask):
    return (int.from_bytes(u, "little") ^ mask).to_bytes(len(u), "little")


@pytest.mark.parametrize("lu", [0, 1, 8, 9, 63])
def test_public_statements(env, lu):
    """k_verify_public's sum over the statement bits, from verification keys written to the device directly: every v_i(s) = p - 1 (each selected bit wraps the
    running sum), and random entries with v_8(s) = 0 (bit 7: the one flip that must NOT reject).  Per statement one proof crafted to be accepted under it, then
    presented under it, under it with every bit at lu and above set (lu = 0: a byte 0xFF where the kernel reads nothing), and under statements that differ in one
    bit below lu; the same through the raw call with stmt_stride > (lu + 7) / 8 and three random bytes behind every statement, which is where the bits at lu
    and above lie when lu is a multiple of 8.  verifier_ref decides every verdict."""
    E = env(736)
    ctx, rng = E.ctx, np.random.default_rng(900 + lu)
    alpha, beta = 7, P - 1
    ub = max(1, (lu + 7) // 8)
    t_s, v0_s = int(rng.integers(1, P)), int(rng.integers(0, P))
    vks = {"pm1": [t_s, v0_s] + [P - 1] * lu, "random": [t_s, v0_s] + [int(x) for x in rng.integers(1, P, size=lu)]}
    if lu > 7:
        vks["random"][2 + 7] = 0
    for kind, vk in vks.items():
        rows, claimed, own, flipped = [], [], [], []
        for k, u in enumerate(_statements(lu, rng)):
            base = vr.v_s(vk, lu, u, 0)
            values = vr.row(t_s, base, alpha, beta, vr.w_list(base)[k % 7])  # accepted under u: w_s chosen against v_0(s) + the statement's sum
            variants = [(u, None)]
            if lu % 8 or lu == 0:  # (lu = 0: the one byte per proof that the wrapper sends; lu = 8 has no spare bit in its byte: the raw call below)
                variants.append((_xor(u, ((1 << (8 * ub)) - 1) & ~((1 << lu) - 1)), None))
            variants += [(_xor(u, 1 << i), i) for i in sorted({0, 7, 8, lu - 1}) if 0 <= i < lu]
            for c, bit in variants:
                rows.append(values)
                claimed.append(c)
                (own if bit is None else flipped).append((len(rows) - 1, bit))
        want = [int(vr.accept(*v, t_s, vr.v_s(vk, lu, c, v[3]), alpha, beta)) for v, c in zip(rows, claimed)]
        assert all(want[i] == 1 for i, _ in own)
        assert all(want[i] == int(vk[2 + bit] == 0) for i, bit in flipped)
        if lu > 7 and kind == "random":
            assert any(want[i] for i, _ in flipped)
        d_vk = ctx.to_device(np.array(vk, dtype=np.uint32))
        d_proofs = ctx.to_device(vr.craft_batch(E.p, E.sk, rows, E.rng, E.shared))
        got = _bits(ctx, ctx.verify_public(d_vk, lu, alpha, beta, E.d_sk, d_proofs, claimed))
        _same(got, want, list(zip(rows, claimed)), f"lu {lu}, {kind} key")
        stride = ub + 3
        st = b"".join(c + rng.bytes(3) for c in claimed)
        ok = ctx.empty(len(rows))
        ctx._chk(ctx.lib.mfh_verify_public(ctx._h, _ptr(d_vk), lu, alpha, beta, _ptr(E.d_sk), _ptr(d_proofs), st, stride, len(rows), _ptr(ok)))
        _same(_bits(ctx, ok), want, list(zip(rows, claimed)), f"lu {lu}, {kind} key, stmt_stride {stride}")


# ------------------------------------------------------------------ d., e. verdicts land where they belong; the 819 / 820 seam
def _zero_a_batch(E, rows):
    """proofs with a = 0 built on the device: zeros plus the (count, 5, L) b limbs written into coordinate n; nothing but the b limbs is staged on the host"""
    import torch

    p = E.p
    b = np.stack([ol.int_to_limbs(vr.craft_b(p, "zero", v, E.rng), p.L) for values in rows for v in values])
    d = torch.zeros((5 * len(rows), p.n + 1, p.L), dtype=torch.int64, device=E.ctx.device)
    d[:, p.n, :] = torch.from_numpy(b.view(np.int64)).to(E.ctx.device)
    return d


def _placed(E, count, reject_at, t_s, v0_s, alpha, beta):
    """count accepted proofs at varying w_s, except at reject_at: the k-th of those fails check k mod 4 alone"""
    wl = vr.w_list(v0_s)
    ws = [wl[i] if i < 7 else int(x) for i, x in enumerate(E.rng.integers(0, P, size=count))]
    failing = {i: frozenset([k % 4]) for k, i in enumerate(reject_at)}
    rows = [vr.row(t_s, v0_s, alpha, beta, ws[i], failing.get(i, frozenset())) for i in range(count)]
    want = [int(vr.accept(*v, t_s, (v0_s + v[3]) % P, alpha, beta)) for v in rows]
    assert want == [int(i not in failing) for i in range(count)]
    return rows, want


@pytest.fixture(scope="module")
def placed_ssp(env):
    E = env(736)
    s, alpha, beta, t, v0 = vr.instance(E.p, "random", np.random.default_rng(4))
    d_ssp = E.ctx.ssp_upload(vr.ssp_with(E.p, t, v0))
    return d_ssp, s, alpha, beta, vr.horner(t, s), vr.horner(v0, s)


@pytest.mark.parametrize("count", [1, 255, 256, 257])
def test_verdicts_land_at_their_index(env, placed_ssp, count):
    """one, just under, exactly and just over one 256-thread block of k_verify / k_verify_public: rejections at 0, 63, 64, 255, 256 (those below count), each
    failing a different single check, everything else accepted"""
    E = env(736)
    ctx = E.ctx
    d_ssp, s, alpha, beta, t_s, v0_s = placed_ssp
    rows, want = _placed(E, count, [i for i in (0, 63, 64, 255, 256) if i < count], t_s, v0_s, alpha, beta)
    d_proofs = _zero_a_batch(E, rows)
    vk = ctx.derive_vk(d_ssp, s, 0)

    def both(path):
        _same(_bits(ctx, ctx.verify(d_ssp, alpha, beta, s, E.d_sk, d_proofs, count)), want, rows, f"mfh_verify, path {path}")
        _same(_bits(ctx, ctx.verify_public(vk, 0, alpha, beta, E.d_sk, d_proofs, [b""] * count)), want, rows, f"mfh_verify_public, path {path}")

    _on_both_paths(ctx, both)


@pytest.mark.parametrize("count,launches", [(819, 0), (820, 1)])
def test_automatic_decrypt_path_seam(env, placed_ssp, count, launches):
    """mfh_verify decrypts 5 count ciphertexts and mfh_decrypt changes kernels at 4096: 819 proofs (4095) run the VALU k_decrypt, 820 (4100) k_decrypt_mm --
    the timing records count the k_decrypt_mm launches -- with the same rejection pattern, and the last index, on both sides"""
    import torch

    E = env(736)
    ctx = E.ctx
    d_ssp, s, alpha, beta, t_s, v0_s = placed_ssp
    rows, want = _placed(E, count, [0, 63, 64, 255, 256, count - 1], t_s, v0_s, alpha, beta)
    d_proofs = _zero_a_batch(E, rows)
    vk = ctx.derive_vk(d_ssp, s, 0)
    ctx.set_decrypt_path(0)
    ctx.set_timing(True)
    try:
        ctx.timing_drain("decrypt")
        got = _bits(ctx, ctx.verify(d_ssp, alpha, beta, s, E.d_sk, d_proofs, count))
        assert ctx.timing_drain("decrypt")[0] == launches
        pub = _bits(ctx, ctx.verify_public(vk, 0, alpha, beta, E.d_sk, d_proofs, [b""] * count))
        assert ctx.timing_drain("decrypt")[0] == launches
    finally:
        ctx.set_timing(False)
    _same(got, want, rows, "mfh_verify")
    _same(pub, want, rows, "mfh_verify_public")
    del d_proofs
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ f. arguments
def test_arguments(env, placed_ssp):
    """mfh_verify / mfh_verify_public through the raw calls: count = 0 returns 0 and writes nothing; alpha, beta or s equal to p, or lu = m, is MFH_EINVAL with
    its message and d_ok untouched"""
    E = env(736)
    ctx, lib, h = E.ctx, E.ctx.lib, E.ctx._h
    d_ssp, s, alpha, beta, t_s, v0_s = placed_ssp
    rows = [vr.row(t_s, v0_s, alpha, beta, 777)] * 2
    d_proofs = _zero_a_batch(E, rows)
    vk = ctx.derive_vk(d_ssp, s, 0)
    ok = ctx.empty(2).fill_(0xA5)
    pr, sk, vkp, okp, sp = _ptr(d_proofs), _ptr(E.d_sk), _ptr(vk), _ptr(ok), _ptr(d_ssp)

    def untouched():
        return _bits(ctx, ok) == [0xA5, 0xA5]

    assert lib.mfh_verify(h, sp, alpha, beta, s, sk, pr, 0, okp) == 0 and untouched()
    assert lib.mfh_verify(h, sp, alpha, beta, s, sk, None, 0, None) == 0
    assert lib.mfh_verify_public(h, vkp, 0, alpha, beta, sk, pr, b"", 0, 0, okp) == 0 and untouched()
    for a, b, x in ((P, beta, s), (alpha, P, s), (alpha, beta, P)):
        assert lib.mfh_verify(h, sp, a, b, x, sk, pr, 2, okp) == EINVAL
        assert lib.mfh_last_error(h).decode() == "alpha, beta, s must be < p" and untouched()
    for a, b in ((P, beta), (alpha, P)):
        assert lib.mfh_verify_public(h, vkp, 0, a, b, sk, pr, b"", 0, 2, okp) == EINVAL
        assert lib.mfh_last_error(h).decode() == "alpha, beta must be < p" and untouched()
    big = ctx.zeros((E.p.m + 2) * 4)
    assert lib.mfh_verify_public(h, _ptr(big), E.p.m, alpha, beta, sk, pr, bytes(16), 8, 2, okp) == EINVAL
    assert "lu must be < m" in lib.mfh_last_error(h).decode() and untouched()
    assert lib.mfh_verify_public(h, _ptr(big), E.p.m - 1, alpha, beta, sk, pr, bytes(14), 7, 2, okp) == EINVAL  # stmt_stride shorter than the 63 bits
    assert "stmt_stride" in lib.mfh_last_error(h).decode() and untouched()
    # and the same arguments in range: both proofs accepted
    assert lib.mfh_verify(h, sp, alpha, beta, s, sk, pr, 2, okp) == 0 and _bits(ctx, ok) == [1, 1]
