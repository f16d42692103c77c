"""CPU: the judges of tests/test_gpu_seed_compressed.py, checked before they judge a kernel.

(i) seed_compressed_ref's regev_decrypt in Python integers against the oracle's in C limbs (oracle.decrypt of oracle.ct_import), on honest and crafted b at both moduli;
(ii) its dot product against the oracle's encryption (b = dot + e p + m mod 2^(64 K));
(iii) its restatement of enc_plan against the table the GPU tests were planned from (n = 1470)."""
import numpy as np
import pytest

import oracle_lib as ol
import seed_compressed_ref as scr

SEED = bytes((11 * i + 5) & 0xFF for i in range(40))


def _params(logq):
    import c_lwe_snarks_amd as mf

    return mf.Params(logq=logq, d=64, m=16)


@pytest.mark.parametrize("logq", [736, 1472])
@pytest.mark.parametrize("off", [0, 8, (1 << 36) - 1608])
def test_python_decrypt_equals_the_oracle(oracle, logq, off):
    p = _params(logq)
    rng = np.random.default_rng(logq + off % 1000)
    sk = scr.extreme_key(rng, p)
    ski = scr.key_ints(sk)
    nrows = 3
    dots = scr.row_dots(oracle, p, SEED, off, nrows, ski)
    top = 1 << (8 * p.ctb)
    for i, dot in enumerate(dots):
        off_i = off + i * p.ctr_ct
        cases = [dot, (dot - 1) % top, dot + ol.P - 1, dot + ol.P, 0, top - 1, 1 << (64 * p.K), (1 << (64 * p.K)) - 1, 0xFFFFFFFF << (8 * p.ctb - 32),
                 int.from_bytes(rng.bytes(p.ctb), "little")]
        for v in cases:
            b = (v % top).to_bytes(p.ctb, "little")
            want = oracle.decrypt(p, sk, oracle.ct_import(p, oracle.rng(SEED, off_i), b))
            assert scr.decrypt_b(b, dot) == want, (i, hex(v))
        assert scr.decrypt_b(dot.to_bytes(p.ctb, "little"), dot) == 0
        # the same dot product is what an encryption adds e p + m to
        m, e = int(rng.integers(0, ol.P)), ol.rand_values(rng, 1, p.L, 559)[0]
        ct = oracle.encrypt(p, oracle.rng(SEED, off_i), sk, m, e)
        assert int.from_bytes(oracle.ct_export(p, ct), "little") == (dot + ol.limbs_to_int(e) * ol.P + m) % (1 << (64 * p.K))


def test_enc_plan_restatement():
    """chunks x k-steps per chunk of k_encrypt_mm at n = 1470: by batch size, and under the forced chunk counts the GPU tests use"""
    p7, p14 = _params(736), _params(1472)
    by_rows = {1: ((705, 3), (470, 9)), 70: ((705, 3), (470, 9)), 4200: ((112, 19), (125, 34)), 8192: ((63, 34), (32, 133)), 16384: ((32, 67), (16, 265)),
               65536: ((8, 265), (4, 1057))}
    for nrows, (w7, w14) in by_rows.items():
        assert scr.enc_plan(p7, nrows)[1:] == w7, nrows
        assert scr.enc_plan(p14, nrows)[1:] == w14, nrows
    for nrows in (1, 70, 513):
        assert [scr.enc_plan(p7, nrows, f)[2] for f in (1, 2, 32, 33, 64)] == [2114, 1057, 67, 65, 34]
        assert [scr.enc_plan(p14, nrows, f)[2] for f in (1, 16, 32, 64)] == [1409, 265, 133, 67]
    assert scr.enc_plan(p14, 513, 1)[1] == 3  # the int32 floor: no accumulator sees more than 131 071 products
    assert scr.enc_plan(p14, 513, 1, honour_kc_min=False)[1:] == (1, 4227)
    # the refresh runs exactly once, on the chunk's last k-step, with 33 chunks at logq 736; never under the default plan of a small batch
    assert scr.refreshes(65) == 1 and scr.refreshes(64) == 0 and scr.refreshes(2114) == 33
    assert scr.refreshes(scr.enc_plan(p7, 513)[2]) == 0 and scr.refreshes(scr.enc_plan(p14, 513)[2]) == 0
