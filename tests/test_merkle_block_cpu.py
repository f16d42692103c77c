"""CPU: words.Block, the builder of a block of transfers, adjusts and writes (MerkleTree.apply_block), and tests/merkle_block_model.py, the model the GPU tests
compare the device with.

1. Block's argument checks, the steps it records and len.
2. Block.statements: every step's statement key and bytes are what the existing classes' .statement gives for (R_j, R_j+1); a skipped step gives None.
3. The model against the three existing models run once per maximal run of one kind: the same rows, roots and records; both policies; first_update.
4. Every row of a model block satisfies its own statement's circuit at the smallest compiled size of each kind, (4, 16, 1): MerkleTransfer, MerkleAdjust,
   MerkleWrite plain and with an expectation, and bits [0, lu) of the assigned row are Block.statements' bytes."""
import numpy as np
import pytest

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import words as W
from merkle_adjust_model import AdjustModel
from merkle_block_model import NONE, BlockModel, row_bytes
from merkle_transfer_model import TransferModel, ledger
from merkle_write_model import WriteModel

P20 = mf.Params(d=1 << 20, m=699050)
K, A, LENGTH = 4, 8, 16
A_KEY, B_KEY, C_KEY, GONE = bytes.fromhex("40aa5580"), bytes.fromhex("40aa5585"), bytes.fromhex("c1aa557f"), bytes.fromhex("77000001")


def _ring(b_a, b_b):
    """depth 1 has no room for the sentinel record: the two records close the ring by hand, (A, B) and (B, FF..FF)"""
    pay = lambda b: b.to_bytes(A, "big")  # noqa: E731
    return [A_KEY + B_KEY + pay(b_a), B_KEY + b"\xff" * K + pay(b_b)]


def test_block_records_steps_and_refuses_bad_arguments():
    b = W.Block(K, A)
    assert len(b) == 0 and b.steps == []
    assert b.transfer(A_KEY, B_KEY, 5) is b and b.adjust(A_KEY, 7) is b and b.adjust(B_KEY, 1, side=1) is b
    b.write(A_KEY, (8, 11), b"abc").write(B_KEY, (15, 16), b"x", expect=b"y")
    assert len(b) == 5
    assert b.steps == [(0, A_KEY, B_KEY, 5), (1, A_KEY, 7, 0), (1, B_KEY, 1, 1), (2, A_KEY, (8, 11), b"abc", None), (2, B_KEY, (15, 16), b"x", b"y")]
    assert (W.Block.TRANSFER, W.Block.ADJUST, W.Block.WRITE) == (0, 1, 2)
    for bad in [(0,), (33,), (4, 0), (4, 9), ("4",), (4, 2.0)]:
        with pytest.raises(W.CircuitError, match="Block"):
            W.Block(*bad)
    small = W.Block(K, 2)
    for call in [lambda: b.transfer(A_KEY, A_KEY, 1), lambda: b.transfer(A_KEY, b"\0" * K, 1), lambda: b.transfer(b"\xff" * K, A_KEY, 1), lambda: b.transfer(A_KEY, B_KEY[:3], 1),
                 lambda: b.transfer(A_KEY, B_KEY, -1), lambda: b.transfer(A_KEY, B_KEY, 1 << 64), lambda: small.adjust(A_KEY, 1 << 16), lambda: b.adjust(A_KEY, 1.5),
                 lambda: b.adjust(A_KEY, 1, side=2), lambda: b.adjust(b"\0" * K, 1), lambda: b.write(A_KEY, (7, 9), b"ab"), lambda: b.write(A_KEY, (9, 9), b""),
                 lambda: b.write(A_KEY, (8, 10), b"abc"), lambda: b.write(A_KEY, (8, 10), b"ab", expect=b"a"), lambda: b.write(A_KEY, 8, b"a"),
                 lambda: b.write(b"\xff" * K, (8, 9), b"a")]:
        with pytest.raises(W.CircuitError, match="Block"):
            call()
    assert len(b) == 5 and len(small) == 0  # a refused step is not recorded


def test_columns_follow_the_steps():
    b = W.Block(K, A).transfer(A_KEY, B_KEY, 5).adjust(B_KEY, 7, 1).write(A_KEY, (9, 12), b"abc", expect=b"xyz")
    col = b.columns()
    assert b.columns() is col  # kept
    assert col["kinds"].tolist() == [0, 1, 2] and col["keys"].tobytes() == A_KEY + B_KEY + A_KEY and col["keys_to"].tobytes() == B_KEY + bytes(2 * K)
    assert col["amounts"].tolist() == [5, 7, 0] and col["sides"].tolist() == [0, 1, 0] and col["fields"].tolist() == [[0, 0], [0, 0], [9, 12]]
    assert col["value_at"].tolist() == [0, 0, 0] and col["expect_at"].tolist() == [2**64 - 1, 2**64 - 1, 0]
    assert col["values"].tobytes() == b"abc" and col["expect"].tobytes() == b"xyz" and (col["values_bytes"], col["expect_bytes"], col["updates"], col["field_hi"]) == (3, 3, 4, 12)
    b.steps[1] = (W.Block.ADJUST, B_KEY, 9, 0)  # a step replaced in place: same list, same length
    assert b.columns() is not col and b.columns()["amounts"].tolist() == [5, 9, 0] and b.columns()["sides"].tolist() == [0, 0, 0]
    col = b.columns()
    b.adjust(A_KEY, 1)  # appended
    assert b.columns()["kinds"].tolist() == [0, 1, 2, 1]
    b.steps = b.steps[:1]  # assigned
    assert b.columns()["kinds"].tolist() == [0] and b.columns()["updates"] == 2
    del b.steps[0]
    assert b.columns()["kinds"].tolist() == [] and b.columns()["values"].size == 1 and b.columns()["values_bytes"] == 0


def test_statements_are_the_existing_classes():
    b = W.Block(K, A).transfer(A_KEY, B_KEY, 5).adjust(A_KEY, 7, 1).write(B_KEY, (9, 12), b"abc").write(B_KEY, (9, 12), b"xyz", expect=b"abc").adjust(GONE, 1)
    roots = [bytes([j]) * 32 for j in range(6)]
    got = b.statements(LENGTH, 3, roots, status=[0, 0, 0, 0, 1])
    upd = W.MerkleUpdate.statement
    assert got[0] == (("MerkleTransfer", K, LENGTH, 3, A), upd(roots[0], roots[1]) + A_KEY + B_KEY + (5).to_bytes(A, "big"))
    assert got[1] == (("MerkleAdjust", K, LENGTH, 3, A), upd(roots[1], roots[2]) + A_KEY + (7).to_bytes(A, "big") + b"\x01")
    assert got[2] == (("MerkleWrite", K, LENGTH, 3, (9, 12), False), upd(roots[2], roots[3]) + B_KEY + b"abc")
    assert got[3] == (("MerkleWrite", K, LENGTH, 3, (9, 12), True), upd(roots[3], roots[4]) + B_KEY + b"abc" + b"xyz")
    assert got[4] is None and b.statements(LENGTH, 3, roots)[4] is not None
    assert [b.statement_key(j, LENGTH, 3) for j in range(4)] == [g[0] for g in got[:4]]
    for bad in [lambda: b.statements(LENGTH, 3, roots[:5]), lambda: b.statements(LENGTH, 3, roots, status=[0]), lambda: b.statements(LENGTH, 3, [b"x"] * 6)]:
        with pytest.raises(W.CircuitError):
            bad()


def _mixed(rng):
    """a table at depth 3 and a block of interleaved kinds in which every status occurs and most steps apply"""
    keys = [bytes([0x10 + 7 * i, 1, 2, i]) for i in range(5)]
    records = ledger(W, {k: 100 * (i + 1) for i, k in enumerate(keys)}, K, 3, 19, A, rng)
    b = W.Block(K, A)
    b.adjust(keys[0], 50).transfer(keys[0], keys[1], 150).write(keys[2], (16, 19), b"abc").write(keys[2], (16, 19), b"xyz", expect=b"abc")
    b.transfer(GONE, keys[0], 1).transfer(keys[0], GONE, 1).adjust(keys[3], 401, 1).adjust(keys[3], 400, 1).adjust(keys[4], (1 << 64) - 500)
    b.write(keys[2], (16, 19), b"...", expect=b"abc").write(keys[1], (8, 16), (7).to_bytes(8, "big")).transfer(keys[1], keys[4], 7).transfer(keys[1], keys[4], 1)
    b.write(GONE, (8, 9), b"z").adjust(keys[4], 1)
    return keys, records, b, [0, 0, 0, 0, 1, 2, 3, 0, 4, 5, 0, 0, 3, 1, 0]


def test_model_against_the_per_kind_models_and_both_policies():
    keys, records, b, want = _mixed(np.random.default_rng(3))
    m = BlockModel(W, records, K, A)
    out = m.apply(b, skip_failed=True)
    assert list(out["status"]) == want
    assert list(out["first_update"]) == [0, 1, 3, 4, 5, 5, 5, 5, 6, 6, 6, 7, 9, 9, 9, 10]
    assert [r is None for r in out["rows"]] == [bool(s) for s in want]
    assert all(len(r) == row_bytes(W, s, K, A, 19, 3) for r, s in zip(out["rows"], b.steps) if r is not None)
    assert out["index"][4, 0] == NONE and out["index"][5, 1] == NONE and out["index"][2, 1] == NONE and out["index"][1, 1] != NONE
    for j, s in enumerate(want):
        assert s == 0 or np.array_equal(out["roots"][j], out["roots"][j + 1])
    assert np.array_equal(out["update_roots"][out["first_update"]], out["roots"])
    # the same steps through the three existing models, one step a call on one shared table
    records_now, roots = list(records), [out["roots"][0].tobytes()]
    for j, step in enumerate(b.steps):
        if want[j]:
            continue
        if step[0] == W.Block.TRANSFER:
            sub = TransferModel(records_now, K, A)
            idx, rows, r = sub.transfer_batch([step[1:]])
        elif step[0] == W.Block.ADJUST:
            sub = AdjustModel(records_now, K, A)
            idx, rows, r = sub.adjust_batch([step[1:]])
        else:
            sub = WriteModel(records_now, K, step[2])
            idx, rows, r = sub.write_batch([(step[1], step[3], step[4])])
        assert np.array_equal(rows[0], out["rows"][j]), j
        assert list(np.atleast_1d(idx[0])) == [int(x) for x in out["index"][j] if x != NONE]
        assert r[0] == out["roots"][j].tobytes() and r[1] == out["roots"][j + 1].tobytes()
        records_now = sub.records
    assert records_now == m.records
    # fail-fast: the statuses and the index all the same, nothing applied
    m2 = BlockModel(W, records, K, A)
    out2 = m2.apply(b, skip_failed=False)
    assert np.array_equal(out2["status"], out["status"]) and np.array_equal(out2["index"], out["index"])
    assert m2.records == [bytes(r) for r in records] and not out2["first_update"].any() and all(r is None for r in out2["rows"])
    # the block without its failed steps gives what skipping gave
    clean = W.Block(K, A)
    clean.steps = [s for s, st in zip(b.steps, want) if not st]
    m3 = BlockModel(W, records, K, A)
    out3 = m3.apply(clean, skip_failed=False)
    assert m3.records == m.records and np.array_equal(out3["update_roots"], out["update_roots"])
    assert all(np.array_equal(x, y) for x, y in zip(out3["rows"], [r for r in out["rows"] if r is not None]))


@pytest.fixture(scope="module")
def programs():
    return {}


def _statement(programs, key):
    if key not in programs:
        programs[key] = getattr(W, key[0])(*key[1:])
    return programs[key]


def test_every_model_row_satisfies_its_statement(programs):
    records = _ring(1000, 5)
    b = W.Block(K, A).adjust(A_KEY, 24).transfer(A_KEY, B_KEY, 1024).write(B_KEY, (8, 16), (3).to_bytes(8, "big")).write(A_KEY, (9, 16), b"MEMO-01", expect=bytes(7))
    b.adjust(B_KEY, 3, 1)
    m = BlockModel(W, records, K, A)
    out = m.apply(b)
    assert not out["status"].any() and m.balance(0) == int.from_bytes(b"\0MEMO-01", "big") and m.balance(1) == 0
    stmts = b.statements(LENGTH, 1, out["roots"], out["status"])
    assert {s[0][0] for s in stmts} == {"MerkleTransfer", "MerkleAdjust", "MerkleWrite"}
    for j, (key, statement) in enumerate(stmts):
        st = _statement(programs, key)
        bits = np.unpackbits(out["rows"][j], bitorder="little")[: st.nin]
        assert len(out["rows"][j]) == st.row_bytes and not bits[:512].any()
        assert st.circuit.holds(bits[: st.lu], bits[st.lu:]), (j, key)
        row = st.circuit.assign(bits[: st.lu], bits[st.lu:], P20)
        assert st.roots_of(row) == (out["roots"][j].tobytes(), out["roots"][j + 1].tobytes())
        assert st.lu == 8 * len(statement) and bytes(row[: st.lu // 8]) == statement
        flipped = bits.copy()
        flipped[512 + 8 * K] ^= 1  # a bit of the amount, the expectation or the value: another statement, which this witness does not satisfy
        assert not st.circuit.holds(flipped[: st.lu], flipped[st.lu:]) or st.roots_of(st.circuit.assign(flipped[: st.lu], flipped[st.lu:], P20))[1] != out["roots"][j + 1].tobytes()
