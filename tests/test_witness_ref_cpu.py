"""CPU: the reference of the witness pass (tests/witness_ref.py) against what it restates.

The generator: tests/ssp_prg_host_check.cpp (a program with its own main that includes csrc/ssp_prg.hpp) is compiled with g++ -O1
-fsanitize=address,undefined and run as a program: nothing is loaded into Python.  Its row key, raw hash and coefficient equal the numpy restatement on
random triples, at the edges of k and of the slot, and at seeds crafted so that the raw hash is one of the five values in [p, 2^32), where the
coefficient is raw - p; both equal tests/golden/ssp_prg.json, 64 (seed, slot, k, coeff) records written once by the compiled header (the crafted seeds
among them), so a changed constant of the hash -- which would silently invalidate every CRS made under the old generator -- fails against recorded
numbers and not against itself.  The witness polynomials: w_polys (float64 BLAS on 16-bit halves) equals the definition looped in Python integers, and
the w that the oracle's prover returns at the DEBUG size.  The kernels held against this reference: tests/test_gpu_witness_exact.py."""
import json
import os
import subprocess

import numpy as np
import pytest

import witness_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ssp_prg.json")
PRG_SEED = 0x0123456789ABCDEF  # (the seed of tests/test_gpu_prg_ssp.py)
CRAFT_SLOTS = (1, 2, 3, 5)     # v_0, the two public rows of lu = 2, and v_4


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ssp_prg_host") / "ssp_prg_host_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "c-lwe-snarks_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "ssp_prg_host_check.cpp")], check=True)

    def run(triples):
        """[(seed, slot, k)] -> [(rowkey, raw, coeff)] by the compiled header"""
        out = subprocess.run([exe], input="".join(f"{s:#x} {slot} {k}\n" for s, slot, k in triples), capture_output=True, text=True, check=True)
        assert out.stderr == ""  # (a sanitizer report goes there)
        rows = [tuple(int(x) for x in line.split()) for line in out.stdout.split("\n")[:-1]]
        assert len(rows) == len(triples)
        return rows

    return run


def restated(triples):
    out = []
    for seed, slot, k in triples:
        rk = wr.prg_rowkey(seed, slot)
        out.append((int(rk), int(wr.prg_raw(rk, k)), int(wr.prg_coeff(rk, k))))
    return out


def crafted():
    return [c for slot in CRAFT_SLOTS for c in wr.crafted_seeds(slot)]


def test_crafting_reproduces_the_seeds_worked_out_by_hand():
    """slot 5, k = 70, low word 0x89abcdef: the seeds for raw = p, p + 2, p + 3 as first computed in plain Python integers"""
    got = {raw: seed for seed, _, _, raw in wr.crafted_seeds(5)}
    assert got[wr.P] == 0xC242941589ABCDEF and got[wr.P + 2] == 0xFB83E2E789ABCDEF and got[wr.P + 3] == 0xAA9014D789ABCDEF
    assert sorted(got) == list(wr.RAW_AT_OR_ABOVE_P)  # all five are reached (p + 1 at k = 3 mod 4, 2^32 - 1 at k = 1 mod 8)
    with pytest.raises(ValueError):
        wr.prg_craft_seed(5, 70, wr.P + 1, wr.CRAFT_LO32)  # an even preimage has no odd row key at an odd k + K0


def test_restatement_equals_the_header(header):
    rng = np.random.default_rng(11)
    d = 1 << 20
    triples = [(int(rng.integers(0, 1 << 64, dtype=np.uint64)), int(rng.integers(0, (1 << 20) + 3)), int(rng.integers(0, 1 << 32))) for _ in range(2000)]
    for seed in (0, (1 << 64) - 1, PRG_SEED, int(rng.integers(0, 1 << 64, dtype=np.uint64))):
        for slot in (0, 1, 2, (1 << 20) + 2, (1 << 32) - 1):
            triples += [(seed, slot, k) for k in (0, 1, d - 1, d, (1 << 32) - 1)]
    triples += [(seed, slot, k) for seed, slot, k, _ in crafted()]
    got, want = header(triples), restated(triples)
    for t, g, w in zip(triples, got, want):
        assert g == w, f"(seed, slot, k) = ({t[0]:#x}, {t[1]}, {t[2]}): header (rowkey, raw, coeff) = {g}, restatement {w}"
        assert g[0] & 1 and g[2] < wr.P and g[2] == g[1] % wr.P
    # arrays of k and of slots give what the scalars give
    seed = PRG_SEED
    ks = np.array([t[2] for t in triples[:500]], dtype=np.uint64)
    rk = wr.prg_rowkey(seed, 7)
    assert [int(x) for x in wr.prg_coeff(rk, ks)] == [int(wr.prg_coeff(rk, int(k))) for k in ks]
    assert np.array_equal(wr.prg_image(seed, 3, 4, 9), np.array([[int(wr.prg_coeff(wr.prg_rowkey(seed, s), k)) for k in range(9)] for s in range(3, 7)]))


def test_crafted_seeds_reach_the_raw_values_at_and_above_p(header):
    cs = crafted()
    assert len(cs) == 5 * len(CRAFT_SLOTS)
    rows = header([(seed, slot, k) for seed, slot, k, _ in cs])
    for (seed, slot, k, raw), (rk, hraw, coeff) in zip(cs, rows):
        assert hraw == raw and raw >= wr.P and coeff == raw - wr.P, f"seed {seed:#x} slot {slot} k {k}: raw {hraw:#x}, coefficient {coeff}"
        assert seed & 0xFFFFFFFF == wr.CRAFT_LO32 and k < 128


def test_unmix_inverts_mix():
    rng = np.random.default_rng(12)
    x = rng.integers(0, 1 << 32, size=100000, dtype=np.uint64)
    x = np.concatenate([x, np.array(wr.RAW_AT_OR_ABOVE_P + (0, 1, 0x80000000), dtype=np.uint64)])
    assert np.array_equal(wr.prg_unmix(wr.prg_mix(x)).astype(np.uint64), x)
    assert np.array_equal(wr.prg_mix(wr.prg_unmix(x)).astype(np.uint64), x)


def test_golden_records(header):
    """the recorded coefficients: by the header as it is compiled today, and by the restatement"""
    with open(GOLDEN) as f:
        recs = json.load(f)
    assert len(recs) == 64
    triples = [(int(r["seed"], 16), r["slot"], r["k"]) for r in recs]
    want = [r["coeff"] for r in recs]
    assert [row[2] for row in header(triples)] == want
    assert [row[2] for row in restated(triples)] == want
    for seed, slot, k, raw in crafted():  # the crafted ones are among them
        assert (seed, slot, k) in triples and want[triples.index((seed, slot, k))] == raw - wr.P


@pytest.mark.parametrize("d,m,nstmt", [(4, 2, 3), (7, 34, 5), (12, 21, 4)])
def test_w_polys_equals_the_definition(d, m, nstmt):
    """m - 1 = 1 (one row), 33 (a byte of padding bits beyond the last row's) and 20; values at the top of the range, all-ones / all-zero statements"""
    rng = np.random.default_rng(d + m)
    ssp = rng.integers(0, wr.P, size=(m + 3, d), dtype=np.uint64).astype(np.uint32)
    ssp[2, 0] = wr.P - 1
    ssp[0, d - 1] = wr.P - 1
    nbytes = (m + 6) // 8
    bits = [bytes(nbytes), b"\xff" * nbytes] + [rng.bytes(nbytes) for _ in range(nstmt - 2)]
    deltas = [0, wr.P - 1] + [int(x) for x in rng.integers(0, wr.P, size=nstmt - 2)]
    got = wr.w_polys(ssp, bits, deltas, m)
    assert got.dtype == np.uint64 and got.shape == (nstmt, d)
    assert got.tolist() == wr.w_polys_plain(ssp.tolist(), bits, deltas, m)
    assert wr.w_polys(ssp, bits, deltas, m, col_block=5).tolist() == got.tolist()  # (column blocks that do not divide d)
    pad = (0xFF << ((m - 1) % 8)) & 0xFF if (m - 1) % 8 else 0  # the last byte's bits at and above m - 1
    assert pad
    flipped = [x[:-1] + bytes([x[-1] ^ pad]) for x in bits]
    assert wr.w_polys(ssp, flipped, deltas, m).tolist() == got.tolist()  # bits at and above m - 1 in the last byte are ignored


def test_w_polys_equals_the_oracle_prover(oracle):
    import c_lwe_snarks_amd as mf
    import oracle_lib as ol

    p = mf.DEBUG
    seed = bytes((17 * i + 9) & 0xFF for i in range(40))
    rng = np.random.default_rng(13)
    nbytes = (p.m + 7) // 8
    wit = rng.bytes(nbytes)
    ssp = oracle.ssp_from_tape(p, rng.integers(0, 256, size=p.m * 8 * p.d, dtype=np.uint8), wit)
    alpha, beta, s = (int(x) for x in rng.integers(1, ol.P, size=3, dtype=np.uint64))
    sk = ol.rand_values(rng, p.n, p.L, p.logq)
    crs = oracle.setup(p, seed, ssp, alpha, beta, s, sk, ol.rand_values(rng, 2 * p.d + p.m, p.L, 559))
    stmts = [wit, bytes(nbytes), b"\xff" * nbytes, rng.bytes(nbytes)]
    deltas = [31337, wr.P - 1, 0, int(rng.integers(0, ol.P))]
    want = wr.w_polys(ssp.reshape(p.m + 3, p.d), stmts, deltas, p.m)
    for b, (bits, delta) in enumerate(zip(stmts, deltas)):
        tape = b"".join(rng.bytes(80) + bytes([int(rng.integers(0, 2))]) for _ in range(5))  # five smudging terms: magnitude | sign
        ref = oracle.prover(p, crs, ssp, bits, delta, tape, 80, want_pre=False)
        assert np.array_equal(ref["w"], want[b]), f"statement {b}"
