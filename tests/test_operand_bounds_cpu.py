"""The expected-value helpers of test_gpu_operand_bounds.py against plain Python integers (no GPU)."""
import numpy as np

import oracle_lib as ol
from test_gpu_operand_bounds import _byte_sums, _limbs, _rep


def test_byte_sums_are_exact_at_their_limit():
    """3 x 131 071 rows (the most test_gpu_operand_bounds.py uses) of the largest coefficients and bytes: every float64 partial sum must
    stay exact"""
    rows = 3 * 131071
    rng = np.random.default_rng(0)
    A = np.full((rows, 3), 255, np.uint8)
    A[:, 2] = rng.integers(0, 256, size=rows, dtype=np.uint8)
    co = np.stack([np.full(rows, 0xFFFFFFFF, np.uint32), np.full(rows, ol.P - 1, np.uint32),
                   rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)])
    S = _byte_sums(co, A)
    assert int(S[0, 0]) == rows * 0xFFFFFFFF * 255  # > 2^53: a single float64 product sum would round
    for v in range(3):
        for u in range(3):
            assert int(S[v, u]) == sum(int(x) for x in (co[v].astype(object) * A[:, u].astype(object)))


def test_constant_values_and_limbs():
    import c_lwe_snarks_amd as mf

    p = mf.Params(logq=736)
    assert _rep(0xFF, 88) == (1 << 704) - 1
    assert _rep(0x80, 2) == 0x8080
    x = _limbs(-1, p)
    assert x.shape == (p.L,) and ol.limbs_to_int(x) == (1 << 704) - 1 and x[p.K:].sum() == 0
    assert ol.limbs_to_int(_limbs(-128 * _rep(1, 88), p)) == (1 << 704) - 128 * _rep(1, 88)
