"""CPU: the SHA-256 compression statement of words.py (Sha256Compress) against hashlib.

1. sha256_pad / be_words / the constants against FIPS 180-4 (the padded "abc" block, K and IV from the primes);
2. chaining="iv": one-block messages of 0, 1, 3 ("abc", the NIST vector) and 55 bytes: digest_of(assign(...)) = hashlib, holds with garbage at the
   result's positions, and the statement read back from the witness is the digest;
3. chaining="public": two-block messages of 56, 64 and 119 bytes chained statement to statement from SHA256_IV;
4. the sizes the builder documents, inside Params(d=1 << 17, m=87381), and the shape of the compiled program (256 outputs, no other equality)."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

PARAMS = mf.Params(d=1 << 17, m=87381)
ABC_DIGEST = "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"  # FIPS 180-4 / NIST example, SHA-256("abc")


@pytest.fixture(scope="module")
def iv():
    st = W.Sha256Compress("iv")
    return st, st.circuit.compile(PARAMS)


@pytest.fixture(scope="module")
def pub():
    st = W.Sha256Compress("public")
    return st, st.circuit.compile(PARAMS)


def _primes(n):
    out, k = [], 2
    while len(out) < n:
        if all(k % q for q in out):
            out.append(k)
        k += 1
    return out


def _frac_root(prime, root):
    """the first 32 bits of the fractional part of prime^(1/root), by integer arithmetic"""
    target = prime << (32 * root)
    lo, hi = 0, 1 << 40
    while lo < hi:  # the largest x with x^root <= prime * 2^(32 root)
        mid = (lo + hi + 1) // 2
        if mid ** root <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo & 0xFFFFFFFF


def test_constants_and_padding():
    assert list(W.SHA256_IV) == [_frac_root(q, 2) for q in _primes(8)]
    assert list(W.SHA256_K) == [_frac_root(q, 3) for q in _primes(64)]
    blk = W.sha256_pad(b"abc")
    assert blk == b"abc\x80" + bytes(52) + (24).to_bytes(8, "big")
    assert W.be_words(blk)[0] == 0x61626380 and W.be_words(blk)[15] == 24
    for n in (0, 1, 55, 56, 63, 64, 119, 120):
        padded = W.sha256_pad(bytes(n))
        assert len(padded) == 64 * ((n + 8) // 64 + 1) and padded[n] == 0x80 and int.from_bytes(padded[-8:], "big") == 8 * n
    with pytest.raises(C.CircuitError):
        W.be_words(b"abc")


@pytest.mark.parametrize("n", [0, 1, 3, 55])
def test_one_block_messages_against_hashlib(iv, n):
    st, cc = iv
    msg = b"abc" if n == 3 else bytes(np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8).tolist())
    blk = W.sha256_pad(msg)
    assert len(blk) == 64
    bits = st.bits(blk)
    assert bits.shape == (768,) and not bits[:256].any()
    wit = st.circuit.assign(bits[:256], bits[256:], PARAMS)
    assert len(wit) == (PARAMS.m + 7) // 8
    digest = hashlib.sha256(msg).digest()
    assert st.digest_of(wit) == digest
    if n == 3:
        assert digest.hex() == ABC_DIGEST
    assert st.digest_of(np.frombuffer(wit, dtype=np.uint8)) == digest
    # the statement: the digest's big-endian words, each LSB first
    assert st.circuit.outputs_of(wit) == np.packbits(W.pack(W.be_words(digest)), bitorder="little").tobytes()
    garbage = np.random.default_rng(100 + n).integers(0, 2, size=256, dtype=np.uint8)
    assert st.circuit.holds(garbage, bits[256:])
    assert st.circuit.assign(garbage, bits[256:], PARAMS) == wit


@pytest.mark.parametrize("n", [56, 64, 119])
def test_two_block_messages_chained_through_the_public_variant(pub, n):
    st, cc = pub
    msg = bytes(np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8).tolist())
    padded = W.sha256_pad(msg)
    assert len(padded) == 128
    h = b"".join(v.to_bytes(4, "big") for v in W.SHA256_IV)
    for k in range(2):
        bits = st.bits(padded[64 * k: 64 * k + 64], h)
        assert bits.shape == (1024,) and not bits[256:512].any()
        wit = st.circuit.assign(bits[:512], bits[512:], PARAMS)
        stmt = st.circuit.outputs_of(wit)
        assert stmt[:32] == np.packbits(W.pack(W.be_words(h)), bitorder="little").tobytes()  # the incoming chaining value stays where it was given
        h = st.digest_of(wit)
    assert h == hashlib.sha256(msg).digest()


def test_sizes(iv, pub):
    for (st, cc), lu, nwires, nrows in ((iv, 256, 61698, 122884), (pub, 512, 61954, 123140)):
        assert (cc.lu, st.lu, cc.nwires, cc.nrows) == (lu, lu, nwires, nrows)
        assert len(cc.program) == 60930 and len(cc.asserts) == 0 and len(cc.equal) == 256 and len(cc.outputs) == 256
        assert np.array_equal(cc.equal, cc.outputs)
        assert cc.outputs[:, 0].tolist() == list(range(st.digest_at + 1, st.digest_at + 257))
        assert cc.nwires <= PARAMS.m - 1 and cc.nrows <= PARAMS.d - 1
        assert cc.nwires > mf.CIRCUIT_MAX_WIRES  # the device-memory kernel's circuit
        ops = cc.program[:, 0]
        assert int((ops == C.GATE_MAJ).sum()) == 600 * 31 + 64 * 32 and int((ops == C.GATE_SUM3).sum()) == 600 * 31
        assert int((ops == C.GATE_CONST0).sum()) == 1 and int((ops == C.GATE_CONST1).sum()) == 1
    with pytest.raises(C.CircuitError):
        W.Sha256Compress("iv").circuit.compile(mf.Params(d=1 << 16, m=43690))
    with pytest.raises(C.CircuitError):
        W.Sha256Compress("merkle")
    st = iv[0]
    with pytest.raises(C.CircuitError):
        st.bits(bytes(64), bytes(32))
    with pytest.raises(C.CircuitError):
        pub[0].bits(bytes(64))
    with pytest.raises(C.CircuitError):
        st.bits(bytes(63))
