"""GPU: the ONE build kernel of the steps that change one field of a record (k_refield_records) gives its three callers the same record.

mfh_merkle_adjust_keys, mfh_merkle_write_keys and mfh_merkle_transfer_keys each build their new records with that kernel -- the field at [2K, 2K + A) or at
the caller's (lo, hi), one plan word a step or two of three -- so the same change asked for through two of them must leave the same bytes.  Shape: depth 3,
K = 6, A = 5, so the balance [12, 17) straddles a 16-byte unit; length 23, no multiple of 16; the table 3 bytes into its tensor at a stride of 29; nk = 5
with one key in three steps, and balances whose sums carry through all five bytes.
1. a batch of deposits through adjust_keys, and on a second copy of the table write_keys on the field (12, 17) with the big-endian new balances as values:
   the same table allocation byte for byte, the same roots R_0 .. R_nk, the same index -- and the records W.indexed_adjust makes one step at a time.
2. a batch of transfers through transfer_keys, and on a second copy two adjust_keys calls, the withdrawals and then the deposits: the same table allocation
   and the same final root.
Each call's rows, launch counts and work rows are pinned against the Python models in test_gpu_merkle_adjust.py, _write.py and _transfer.py."""
import numpy as np
import pytest

from merkle_adjust_model import ledger
from test_gpu_merkle_absent import _key, _keys
from test_gpu_merkle_record_update import Placed

pytestmark = pytest.mark.gpu

K, A, LENGTH, DEPTH, STRIDE, OFF = 6, 5, 23, 3, 29, 3


@pytest.fixture(scope="module")
def W():
    from c_lwe_snarks_amd import words

    return words


@pytest.fixture(scope="module")
def ctx(gpu_ctx_factory):
    return gpu_ctx_factory()  # (the tree does not depend on the parameters)


@pytest.fixture(scope="module")
def bank(W):
    """(the seven accounts' keys, the records of a full depth-3 ledger): balances just below a carry out of the low byte, of three bytes and of four"""
    top = 0x10 << (8 * (K - 1))
    keys = [_key(x, K) for x in (top, top + 1, 3 * top, 5 * top + 7, 5 * top + 8, 9 * top, 0xF0 << (8 * (K - 1)))]
    balances = [0xFD, 0xFFFFFE, 0xFFFFFFFA, 0x1234567890, 1000, 0, 0x7FFFFFFFFF]
    return keys, ledger(W, dict(zip(keys, balances)), K, DEPTH, LENGTH, A, np.random.default_rng(52000))


def _placed(ctx, records):
    tree = ctx.merkle_tree(DEPTH)
    table = Placed(ctx, records, stride=STRIDE, off=OFF)
    tree.set_records(0, table.view)
    return tree, table


def test_deposits_as_adjusts_and_as_writes(ctx, W, bank):
    keys, records = bank
    steps = [(keys[2], 7), (keys[0], 0x300), (keys[2], (1 << 32) + 5), (keys[4], 1), (keys[2], 0xFFFFFFF0)]  # keys[2] three times
    want, values = list(records), []
    for key, v in steps:  # the model, one step at a time: the record of `key` is slot keys.index(key) + 1 of a full ledger
        i = keys.index(key) + 1
        want[i] = W.indexed_adjust(want[i], v, 0, K, amount_bytes=A).tobytes()
        values.append(want[i][2 * K: 2 * K + A])
    assert int.from_bytes(values[-1], "big") == 0xFFFFFFFA + 7 + (1 << 32) + 5 + 0xFFFFFFF0  # carries through every byte of the field
    k = _keys([s[0] for s in steps], K)
    tree_a, table_a = _placed(ctx, records)
    tree_w, table_w = _placed(ctx, records)
    try:
        _, index_a, roots_a = tree_a.adjust_keys(table_a.view, k, [s[1] for s in steps], amount_bytes=A, roots=True)
        _, index_w, roots_w = tree_w.write_keys(table_w.view, k, values, (2 * K, 2 * K + A), roots=True)
        assert np.array_equal(table_a.whole.cpu().numpy(), table_w.whole.cpu().numpy())
        assert roots_a.shape == (len(steps) + 1, 32) and np.array_equal(roots_a, roots_w)
        assert index_a.tolist() == index_w.tolist() == [keys.index(s[0]) + 1 for s in steps]
        table_a.holds(want, "adjust_keys")
        table_w.holds(want, "write_keys")
        assert tree_a.root() == tree_w.root() == roots_a[-1].tobytes() != roots_a[0].tobytes()
    finally:
        tree_a.close()
        tree_w.close()


def test_transfers_as_a_withdrawal_and_a_deposit_batch(ctx, W, bank):
    keys, records = bank
    steps = [(keys[3], keys[0], 0x90), (keys[6], keys[3], 0xFFFFFFFF), (keys[3], keys[4], 0x34567890), (keys[2], keys[5], 0xFFFFFFFA), (keys[1], keys[0], 3)]  # keys[3] in three
    want = list(records)
    for k_from, k_to, v in steps:
        p, s = keys.index(k_from) + 1, keys.index(k_to) + 1
        _, new = W.indexed_transfer(want[p], p, want[s], s, v, K, amount_bytes=A)
        want[p], want[s] = new[0].tobytes(), new[1].tobytes()
    k_from, k_to, amounts = _keys([s[0] for s in steps], K), _keys([s[1] for s in steps], K), [s[2] for s in steps]
    tree_t, table_t = _placed(ctx, records)
    tree_a, table_a = _placed(ctx, records)
    try:
        tree_t.transfer_keys(table_t.view, k_from, k_to, amounts, amount_bytes=A)
        tree_a.adjust_keys(table_a.view, k_from, amounts, sides=[1] * len(steps), amount_bytes=A)
        tree_a.adjust_keys(table_a.view, k_to, amounts, sides=[0] * len(steps), amount_bytes=A)
        assert np.array_equal(table_t.whole.cpu().numpy(), table_a.whole.cpu().numpy())
        table_t.holds(want, "transfer_keys")
        assert tree_t.root() == tree_a.root()
    finally:
        tree_t.close()
        tree_a.close()
