"""CPU: the compiled programs of the Merkle statements and of Sha256Message are the recorded ones.  A compiled program is part of every CRS made for it, so
a change of words.py that moves one wire breaks every key in use: tests/golden/merkle_programs.json holds, per statement, a SHA-256 over every array of
Circuit.compile's result (the rows in CSR form, gates, asserts, program, equal, outputs, terms, the node-to-wire map) with nrows, nwires and lu;
tests/golden/make_golden.py regenerates it from program_digests() below."""
import hashlib
import json
import os

import numpy as np

import c_lwe_snarks_amd as mf
from c_lwe_snarks_amd import words as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merkle_programs.json")
P18 = mf.Params(d=1 << 18, m=174762)  # the largest of the older statements, MerkleRecordUpdate(8, 1), is 199 735 rows
P19 = mf.Params(d=1 << 19, m=349525)  # the key steps and MerkleSegment: MerkleInsert(4, 8, 1, joined=False) is 399 885 rows

STATEMENTS = {
    "MerklePath(1)": lambda: W.MerklePath(1),
    "MerklePath(2)": lambda: W.MerklePath(2),
    "MerkleRecord(3, 2)": lambda: W.MerkleRecord(3, 2),
    "MerkleRecord(56, 1)": lambda: W.MerkleRecord(56, 1),
    "MerkleUpdate(1)": lambda: W.MerkleUpdate(1),
    "MerkleRecordUpdate(8, 1)": lambda: W.MerkleRecordUpdate(8, 1),
    "MerkleRecordUpdate(8, 1, frozen=(0, 4))": lambda: W.MerkleRecordUpdate(8, 1, frozen=(0, 4)),
    "MerkleAbsent(4, 8, 1)": lambda: W.MerkleAbsent(4, 8, 1),
    "MerkleAbsent(8, 16, 1)": lambda: W.MerkleAbsent(8, 16, 1),
    "Sha256Message(0)": lambda: W.Sha256Message(0),
    "Sha256Message(56)": lambda: W.Sha256Message(56),
    "MerkleAdjust(4, 16, 1, 8)": lambda: W.MerkleAdjust(4, 16, 1, 8),
    "MerkleAdjust(4, 16, 1, 3)": lambda: W.MerkleAdjust(4, 16, 1, 3),
    "MerkleWrite(4, 16, 1, (8, 16))": lambda: W.MerkleWrite(4, 16, 1, (8, 16)),
    "MerkleWrite(4, 16, 1, (8, 16), True)": lambda: W.MerkleWrite(4, 16, 1, (8, 16), True),
    "MerkleWrite(4, 16, 1, (9, 10), True)": lambda: W.MerkleWrite(4, 16, 1, (9, 10), True),
}
# compiled against P19; the entries above stay on P18, so their digests do not move
STATEMENTS_P19 = {
    "MerkleInsert(4, 8, 1)": lambda: W.MerkleInsert(4, 8, 1),
    "MerkleInsert(4, 8, 1, joined=False)": lambda: W.MerkleInsert(4, 8, 1, joined=False),
    "MerkleRemove(4, 8, 1)": lambda: W.MerkleRemove(4, 8, 1),
    "MerkleRemove(5, 11, 1, joined=False)": lambda: W.MerkleRemove(5, 11, 1, joined=False),
    "MerkleSegment(2)": lambda: W.MerkleSegment(2),
    "MerkleTransfer(4, 16, 1, 8)": lambda: W.MerkleTransfer(4, 16, 1, 8),
}
STATEMENTS.update(STATEMENTS_P19)


def program_digest(statement, params=P18) -> str:
    cc = statement.circuit.compile(params)
    h = hashlib.sha256(f"nrows {cc.nrows} nwires {cc.nwires} lu {cc.lu} statement lu {statement.lu}".encode())
    arrays = dict(zip(("row_ptr", "wire", "coef"), cc.rows), gates=cc.gates, asserts=cc.asserts, program=cc.program, equal=cc.equal, outputs=cc.outputs,
                  terms=cc.terms, wires=np.array(cc.wires, dtype=np.uint32))
    for name, a in arrays.items():
        h.update(f"{name} {a.dtype.str} {a.shape}".encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def program_digests():
    return {name: program_digest(make(), P19 if name in STATEMENTS_P19 else P18) for name, make in STATEMENTS.items()}


def test_compiled_programs_are_the_recorded_ones():
    want = json.load(open(GOLDEN))
    assert set(want) == set(STATEMENTS)
    got = program_digests()
    assert got == want
