"""CPU: the transition statement words.MerkleUpdate(depth): one leaf changed, and that change alone takes the tree from old_root to new_root.

1. sizes: depths 1 and 2 are compiled and equal MERKLE_UPDATE_SIZES and the formula 56 993 depth + 1 026 wires, 101 473 depth + 1 540 rows (twice
   MerklePath's less the shared sibling and direction wires); the input count is 1024 + 257 depth; lu, the outputs and the equalities are 512; at
   d = 2^20, m = 699 050 depth 10 fits and depth 11 does not.
2. roots: roots_of(assign(bits(...))) equals tests/sha256_ref.py's merkle_root of the old and of the new leaf at depth 1 (both indices) and depth 2 (every
   index).
3. sensitivity: one bit flipped in the old leaf changes the old root alone, in the new leaf the new root alone, in a sibling both.
4. statement: statement(old, new) equals bits [0, 512) of the assigned row, and its halves are MerklePath.statement's bytes.
5. refusals: what MerklePath.bits refuses (leaf and sibling sizes, the sibling count, the index range), and bad depths."""
import numpy as np
import pytest

import c_lwe_snarks_amd as mf
import sha256_ref as ref
from c_lwe_snarks_amd import circuit as C
from c_lwe_snarks_amd import words as W

P18 = mf.Params(d=1 << 18, m=174762)
P20 = mf.Params(d=1 << 20, m=699050)

# the issue's table: depth -> (wires, rows)
TABLE = {1: (58019, 103013), 2: (115012, 204486), 3: (172005, 305959), 10: (570956, 1016270)}


def _formula(depth):
    return 56993 * depth + 1026, 101473 * depth + 1540


@pytest.fixture(scope="module")
def statements():
    out = {}
    for depth in (1, 2):
        st = W.MerkleUpdate(depth)
        out[depth] = (st, st.circuit.compile(P18))
    return out


# ------------------------------------------------------------------ 1. sizes
@pytest.mark.parametrize("depth", [1, 2])
def test_compiled_sizes(statements, depth):
    st, cc = statements[depth]
    assert (cc.nwires, cc.nrows) == TABLE[depth] == W.MERKLE_UPDATE_SIZES[depth] == _formula(depth)
    assert st.lu == cc.lu == 512 and len(cc.outputs) == 512 and len(cc.equal) == 512 and len(cc.asserts) == 0
    assert cc.nwires - len(cc.program) == 1024 + 257 * depth
    # twice MerklePath's, less what the two passes share: 257 input wires (and their bit rows) a level and the two constant wires
    pw, pr = W.MERKLE_PATH_SIZES[depth]
    assert (cc.nwires, cc.nrows) == (2 * pw - 257 * depth - 2, 2 * pr - 257 * depth - 4)


def test_table_by_formula_and_capacity():
    assert W.MERKLE_UPDATE_SIZES == TABLE
    for depth, size in TABLE.items():
        assert size == _formula(depth), depth
    fits = lambda size, p: size[0] <= p.m - 1 and size[1] <= p.d - 1  # noqa: E731  (Circuit.compile's two limits)
    assert fits(_formula(10), P20) and _formula(10) == (570956, 1016270)
    assert _formula(11)[1] == 1117743 and not fits(_formula(11), P20)
    assert fits(_formula(1), mf.Params(d=1 << 17, m=87381)) and fits(_formula(2), P18) and not fits(_formula(2), mf.Params(d=1 << 17, m=87381))


def test_bad_depths_refused():
    for depth in (0, -1, 1.0, None):
        with pytest.raises(C.CircuitError):
            W.MerkleUpdate(depth)


# ------------------------------------------------------------------ 2. roots
def _roots(statements, depth, old, new, sibs, index):
    st, _ = statements[depth]
    bits = st.bits(old, new, sibs, index)
    assert bits.shape == (1024 + 257 * depth,) and bits.dtype == np.uint8 and not bits[:512].any()
    row = st.circuit.assign(bits[:512], bits[512:], P18)
    assert st.circuit.holds(bits[:512], bits[512:])
    return st.roots_of(row), row


@pytest.mark.parametrize("depth", [1, 2])
def test_roots_equal_reference_at_every_index(statements, depth):
    rng = np.random.default_rng(8100 + depth)
    old, new = rng.bytes(32), rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(depth)]
    seen = set()
    for index in range(1 << depth):
        (r_old, r_new), _ = _roots(statements, depth, old, new, sibs, index)
        assert r_old == ref.merkle_root(old, sibs, index), index
        assert r_new == ref.merkle_root(new, sibs, index), index
        seen |= {r_old, r_new}
    assert len(seen) == 2 << depth  # the direction bits matter, to both roots
    # the layout of the private bits
    st, _ = statements[depth]
    bits = st.bits(old, new, sibs, (1 << depth) - 2)
    assert np.array_equal(bits[512: 512 + 512 + 256 * depth], W.pack(W.be_words(old + new + b"".join(sibs))))
    assert bits[-depth:].tolist() == [0] + [1] * (depth - 1)


# ------------------------------------------------------------------ 3. sensitivity
def _flip(b: bytes, bit: int) -> bytes:
    out = bytearray(b)
    out[bit >> 3] ^= 1 << (bit & 7)
    return bytes(out)


def test_one_flipped_bit_changes_the_right_roots(statements):
    depth, index = 2, 1
    rng = np.random.default_rng(8200)
    old, new = rng.bytes(32), rng.bytes(32)
    sibs = [rng.bytes(32) for _ in range(depth)]
    (r_old, r_new), _ = _roots(statements, depth, old, new, sibs, index)
    (a_old, a_new), _ = _roots(statements, depth, _flip(old, 77), new, sibs, index)
    assert a_old != r_old and a_new == r_new and a_old == ref.merkle_root(_flip(old, 77), sibs, index)
    (b_old, b_new), _ = _roots(statements, depth, old, _flip(new, 200), sibs, index)
    assert b_old == r_old and b_new != r_new and b_new == ref.merkle_root(_flip(new, 200), sibs, index)
    for level in range(depth):
        other = list(sibs)
        other[level] = _flip(sibs[level], 5 + level)
        (c_old, c_new), _ = _roots(statements, depth, old, new, other, index)
        assert c_old != r_old and c_new != r_new, level
        assert (c_old, c_new) == (ref.merkle_root(old, other, index), ref.merkle_root(new, other, index))


# ------------------------------------------------------------------ 4. statement
def test_statement_is_the_inverse_of_roots_of(statements):
    st, _ = statements[1]
    rng = np.random.default_rng(8300)
    old, new, sib = rng.bytes(32), rng.bytes(32), rng.bytes(32)
    (r_old, r_new), row = _roots(statements, 1, old, new, [sib], 1)
    assert st.statement(r_old, r_new) == bytes(row[:64]) == W.MerkleUpdate.statement(bytearray(r_old), bytearray(r_new))
    assert st.statement(r_old, r_new) == W.MerklePath.statement(r_old) + W.MerklePath.statement(r_new)
    assert st.statement(r_new, r_old) != st.statement(r_old, r_new)
    for bad in (b"", r_old[:31], r_old + b"\0"):
        with pytest.raises(C.CircuitError):
            W.MerkleUpdate.statement(bad, r_new)
        with pytest.raises(C.CircuitError):
            W.MerkleUpdate.statement(r_old, bad)


# ------------------------------------------------------------------ 5. refusals
def test_bits_refusals(statements):
    st, _ = statements[2]
    leaf, sibs = bytes(32), [bytes(32), bytes(32)]
    for old, new, s, index in [(leaf[:31], leaf, sibs, 0), (leaf, leaf + b"x", sibs, 0), (leaf, leaf, sibs[:1], 0), (leaf, leaf, sibs + [leaf], 0),
                               (leaf, leaf, [sibs[0], sibs[1][:31]], 0), (leaf, leaf, sibs, 4), (leaf, leaf, sibs, -1)]:
        with pytest.raises(C.CircuitError):
            st.bits(old, new, s, index)
    assert st.bits(leaf, leaf, sibs, 3).shape == (1024 + 514,)
