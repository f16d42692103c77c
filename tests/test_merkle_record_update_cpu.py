"""CPU: the record transition statement words.MerkleRecordUpdate(length, depth, frozen): one record changed, and that change alone takes the tree of
record hashes from old_root to new_root.

1. sizes: compile at (8, 1), (55, 1), (56, 1) and (55, 2) gives the tabled (wires, rows) and MERKLE_RECORD_UPDATE_SIZES; where the tables have the
   length, the identity MERKLE_UPDATE_SIZES[depth] + 2 x SHA256_MESSAGE_SIZES[length] - (1 028, 1 544); the input count is 512 + 16 length + 257 depth;
   lu, the outputs and the equalities are 512; frozen adds 8 (hi - lo) rows (equalities) and no wire; what fits d = 2^18 and d = 2^20.
2. roots at (8, 2), every index: holds, and roots_of(assign(bits(...))) equals the roots from hashlib.sha256 and tests/sha256_ref.py's merkle_parent; one
   bit flipped in the old record changes the old root alone, in the new record the new root alone.
3. frozen=(0, 4): a new record that changes byte 3 does not hold while both roots are computed as before; changing byte 4 holds.
4. refusals: record lengths, the sibling count and sizes, the index range, frozen out of [0, length] or reversed, bad lengths and depths.
5. statement: statement() equals MerkleUpdate.statement() and bytes [0, 64) of the assigned row."""
import hashlib

import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P18 = mf.Params(d=1 << 18, m=174762)
P19 = mf.Params(d=1 << 19, m=349525)
P20 = mf.Params(d=1 << 20, m=699050)

# the issue's table: (length, depth) -> (wires, rows)
TABLE = {(8, 1): (112309, 199735), (55, 1): (113075, 200501), (56, 1): (167755, 297613), (55, 2): (170068, 301974)}


def _identity(length, depth):
    (uw, ur), (sw, sr) = W.MERKLE_UPDATE_SIZES[depth], W.SHA256_MESSAGE_SIZES[length]
    return uw + 2 * sw - 1028, ur + 2 * sr - 1544


def _fits(size, p):  # Circuit.compile's two limits
    return size[0] <= p.m - 1 and size[1] <= p.d - 1


@pytest.fixture(scope="module")
def st82():
    st = W.MerkleRecordUpdate(8, 2)
    return st, st.circuit.compile(P19)  # (8, 2) is 301 208 rows: above d = 2^18


@pytest.fixture(scope="module")
def frozen82():
    st = W.MerkleRecordUpdate(8, 2, frozen=(0, 4))
    return st, st.circuit.compile(P19)  # (8, 2) is 301 208 rows: above d = 2^18


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("length,depth", sorted(TABLE))
def test_compiled_sizes(length, depth):
    st = W.MerkleRecordUpdate(length, depth)
    cc = st.circuit.compile(P19)
    assert (cc.nwires, cc.nrows) == TABLE[(length, depth)] == W.MERKLE_RECORD_UPDATE_SIZES[(length, depth)]
    if length in W.SHA256_MESSAGE_SIZES:
        assert (cc.nwires, cc.nrows) == _identity(length, depth)
    assert st.lu == cc.lu == 512 and len(cc.outputs) == 512 and len(cc.equal) == 512 and len(cc.asserts) == 0
    assert cc.nwires - len(cc.program) == 512 + 16 * length + 257 * depth
    assert st.blocks == (1 if length <= 55 else 2)


def test_frozen_adds_rows_and_no_wire():
    plain = W.MerkleRecordUpdate(8, 1).circuit.compile(P18)
    for lo, hi in [(0, 4), (3, 8), (0, 8), (5, 5), (0, 0), (8, 8)]:
        st = W.MerkleRecordUpdate(8, 1, frozen=(lo, hi))
        cc = st.circuit.compile(P18)
        assert (cc.nwires, cc.nrows) == (plain.nwires, plain.nrows + 8 * (hi - lo)), (lo, hi)
        assert len(cc.equal) == 512 + 8 * (hi - lo) and len(cc.outputs) == 512 and cc.lu == 512
        assert cc.nwires - len(cc.program) == 512 + 16 * 8 + 257
        assert st.frozen == (lo, hi)
    assert W.MerkleRecordUpdate(8, 1).frozen is None
    assert (plain.nrows + 32, plain.nwires) == (199767, 112309)  # the issue's frozen=(0, 4) on (8, 1)


def test_table_identity_and_capacity():
    assert {k: W.MERKLE_RECORD_UPDATE_SIZES[k] for k in TABLE} == TABLE
    for length, depth in [(55, 1), (56, 1), (55, 2)]:
        assert TABLE[(length, depth)] == _identity(length, depth)
    assert _fits(TABLE[(55, 1)], P18) and not _fits(TABLE[(55, 1)], mf.Params(d=1 << 17, m=87381))
    # d = 2^20: one-block records reach depth 9, two-block records depth 8 (a level more is MerkleUpdate's 56 993 wires and 101 473 rows)
    assert W.MERKLE_RECORD_UPDATE_SIZES[(55, 9)] == (569019, 1012285) and _fits((569019, 1012285), P20)
    assert 1012285 + 101473 == 1113758 and not _fits((569019 + 56993, 1113758), P20)
    w8, r8 = W.MERKLE_RECORD_UPDATE_SIZES[(119, 8)]
    assert _fits((w8, r8), P20) and not _fits((w8 + 56993, r8 + 101473), P20)
    # both follow from the small table by the per-level increment
    assert (569019, 1012285) == (TABLE[(55, 1)][0] + 8 * 56993, TABLE[(55, 1)][1] + 8 * 101473)
    sw, sr = W.SHA256_MESSAGE_SIZES[119]
    assert (w8, r8) == (1026 + 8 * 56993 + 2 * sw - 1028, 1540 + 8 * 101473 + 2 * sr - 1544)


def test_bad_shapes_refused():
    for length, depth in [(-1, 1), (1.0, 1), (None, 1), (8, 0), (8, -1), (8, 1.0), (8, None)]:
        with pytest.raises(C.CircuitError):
            W.MerkleRecordUpdate(length, depth)
    for frozen in [(-1, 2), (3, 2), (0, 9), (9, 9), (0.0, 2), (0, None)]:
        with pytest.raises(C.CircuitError):
            W.MerkleRecordUpdate(8, 1, frozen=frozen)


# ------------------------------------------------------------------ 2. roots
def _root(record, sibs, index):
    cur = hashlib.sha256(record).digest()
    for l, s in enumerate(sibs):
        cur = ref.merkle_parent(s, cur) if (index >> l) & 1 else ref.merkle_parent(cur, s)
    return cur


def _roots(stcc, old, new, sibs, index, holds=True):
    st, _ = stcc
    bits = st.bits(old, new, sibs, index)
    assert bits.shape == (512 + 16 * st.length + 257 * st.depth,) and bits.dtype == np.uint8 and not bits[:512].any()
    assert st.circuit.holds(bits[:512], bits[512:]) is holds
    row = st.circuit.assign(bits[:512], bits[512:], P19)
    return st.roots_of(row), row


def _flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def test_roots_equal_reference_at_every_index(st82):
    rng = np.random.default_rng(8600)
    old, new = rng.bytes(8), rng.bytes(8)
    sibs = [rng.bytes(32) for _ in range(2)]
    seen = set()
    for index in range(4):
        (r_old, r_new), _ = _roots(st82, old, new, sibs, index)
        assert (r_old, r_new) == (_root(old, sibs, index), _root(new, sibs, index)), index
        seen |= {r_old, r_new}
        (a_old, a_new), _ = _roots(st82, _flip(old, 13), new, sibs, index)
        assert a_old != r_old and a_new == r_new and a_old == _root(_flip(old, 13), sibs, index), index
        (b_old, b_new), _ = _roots(st82, old, _flip(new, 62), sibs, index)
        assert b_old == r_old and b_new != r_new and b_new == _root(_flip(new, 62), sibs, index), index
    assert len(seen) == 8  # the direction bits matter, to both roots
    # the layout of the private bits: byte k's bit b at 8 k + b, old then new; the siblings as big-endian words; the index bits
    bits = st82[0].bits(old, new, sibs, 2)
    assert np.array_equal(bits[512: 512 + 128], np.unpackbits(np.frombuffer(old + new, dtype=np.uint8), bitorder="little"))
    assert np.array_equal(bits[640: 640 + 512], W.pack(W.be_words(b"".join(sibs))))
    assert bits[-2:].tolist() == [0, 1]
    # an unchanged record is a statement like any other: both roots the same
    (s_old, s_new), _ = _roots(st82, old, old, sibs, 3)
    assert s_old == s_new == _root(old, sibs, 3)


# ------------------------------------------------------------------ 3. frozen
def test_frozen_bytes(st82, frozen82):
    rng = np.random.default_rng(8700)
    old = rng.bytes(8)
    sibs = [rng.bytes(32) for _ in range(2)]
    free = old[:4] + bytes(x ^ 0x5A for x in old[4:])
    for index in (0, 3):
        (r_old, r_new), _ = _roots(frozen82, old, free, sibs, index)
        assert (r_old, r_new) == (_root(old, sibs, index), _root(free, sibs, index))
        byte3 = _flip(free, 8 * 3 + 6)
        (a_old, a_new), _ = _roots(frozen82, old, byte3, sibs, index, holds=False)  # both roots still computed
        assert (a_old, a_new) == (_root(old, sibs, index), _root(byte3, sibs, index))
        assert _roots(st82, old, byte3, sibs, index)[0] == (a_old, a_new)  # the statement without the relation holds on it
        byte4 = _flip(free, 8 * 4)
        (b_old, b_new), _ = _roots(frozen82, old, byte4, sibs, index)
        assert (b_old, b_new) == (_root(old, sibs, index), _root(byte4, sibs, index))
    for bit in (0, 31):  # the edges of the frozen range
        _roots(frozen82, old, _flip(free, bit), sibs, 1, holds=False)
    _roots(frozen82, old, _flip(free, 32), sibs, 1)


# ------------------------------------------------------------------ 4. refusals
def test_bits_refusals(st82):
    st, _ = st82
    rec, sibs = bytes(8), [bytes(32), bytes(32)]
    for old, new, s, index in [(rec[:7], rec, sibs, 0), (rec, rec + b"x", sibs, 0), (b"", rec, sibs, 0), (rec, rec, sibs[:1], 0), (rec, rec, sibs + [bytes(32)], 0),
                               (rec, rec, [sibs[0], sibs[1][:31]], 0), (rec, rec, sibs, 4), (rec, rec, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(old, new, s, index)
    assert st.bits(rec, rec, sibs, 3).shape == (512 + 128 + 514,)


# ------------------------------------------------------------------ 5. statement
def test_statement_bytes(st82):
    st, _ = st82
    rng = np.random.default_rng(8800)
    old, new = rng.bytes(8), rng.bytes(8)
    sibs = [rng.bytes(32) for _ in range(2)]
    (r_old, r_new), row = _roots(st82, old, new, sibs, 1)
    assert st.statement(r_old, r_new) == bytes(row[:64]) == W.MerkleUpdate.statement(r_old, r_new)
    assert len(st.statement(r_old, r_new)) == 64 and st.statement(r_new, r_old) != st.statement(r_old, r_new)
    assert W.MerkleRecordUpdate.statement(bytearray(r_old), bytearray(r_new)) == W.MerklePath.statement(r_old) + W.MerklePath.statement(r_new)
    for bad in (b"", r_old[:31], r_old + b"\0"):
        with pytest.raises(C.CircuitError):
            W.MerkleRecordUpdate.statement(bad, r_new)
        with pytest.raises(C.CircuitError):
            W.MerkleRecordUpdate.statement(r_old, bad)
