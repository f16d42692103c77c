"""numpy reference of the row check (mfh_ssp_rows_violations): the CSR entries times the selected bits, summed per row in uint64, mod p."""
import numpy as np

P = 0xFFFFFFFB
NONE = 0xFFFFFFFF


def csr(rows):
    """(row_ptr, wire, coef) uint32 arrays of a list of rows of (wire, coef) pairs"""
    rp = np.zeros(len(rows) + 1, dtype=np.uint32)
    np.cumsum([len(r) for r in rows], out=rp[1:])
    w = np.array([x for r in rows for x, _ in r], dtype=np.uint32)
    c = np.array([a for r in rows for _, a in r], dtype=np.uint32)
    return rp, w, c


def row_sums(rows, witness_row):
    """E_j mod p of every row for one statement: witness_row = its packed bits (bit i - 1 = wire i); wire 0 is always selected"""
    rp, wire, coef = (np.asarray(x) for x in rows)
    nrows = len(rp) - 1
    if nrows == 0:
        return np.zeros(0, dtype=np.uint64)
    bits = np.unpackbits(np.frombuffer(bytes(witness_row), dtype=np.uint8), bitorder="little")
    sel = np.ones(len(wire), dtype=np.uint64)
    nz = wire > 0
    sel[nz] = bits[wire[nz].astype(np.int64) - 1]
    terms = coef.astype(np.uint64) * sel  # each < 2^32: a row of fewer than 2^32 entries sums in uint64
    lens = np.diff(rp.astype(np.int64))
    out = np.zeros(nrows, dtype=np.uint64)
    if len(terms):
        # reduceat over the non-empty rows only: for an empty row it would return the next row's first term
        ne = lens > 0
        out[ne] = np.add.reduceat(terms, rp[:-1][ne].astype(np.int64))
    return out % np.uint64(P)


def violations(rows, witness_rows):
    """(count, first) as mfh_ssp_rows_violations defines them, uint32 arrays over the statements"""
    count = np.zeros(len(witness_rows), dtype=np.uint32)
    first = np.full(len(witness_rows), NONE, dtype=np.uint32)
    for b, wr in enumerate(witness_rows):
        e = row_sums(rows, wr)
        bad = np.flatnonzero((e != 1) & (e != P - 1))
        count[b] = len(bad)
        if len(bad):
            first[b] = bad[0]
    return count, first
