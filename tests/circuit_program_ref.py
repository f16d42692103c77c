"""Helpers of the circuit-program tests: random circuits and a numpy restatement of the bitsliced evaluation of mfh_circuit_assign (include/mfhip.h)."""
import numpy as np

from c_lwe_snarks_amd import circuit as C


def random_circuit(rng, npub, npriv, ngates, nasserts=0, interleave=False):
    """inputs, then ngates random gates on earlier wires, then nasserts random assertions; interleave: private inputs declared between the gates"""
    c = C.Circuit()
    ws = c.public(npub)
    priv = c.private(min(npriv, 1) if interleave else npriv)
    ws += priv
    for g in range(ngates):
        if interleave and len(priv) < npriv and rng.integers(0, 3) == 0:  # inputs declared between gates still take the low wires
            w = c.private()
            priv.append(w)
            ws.append(w)
        kind = ("XOR", "AND", "OR", "NOT")[int(rng.integers(0, 4))]
        a, b = (ws[int(rng.integers(0, len(ws)))] for _ in range(2))
        ws.append(c.NOT(a) if kind == "NOT" else getattr(c, kind)(a, b))
    while len(priv) < npriv:
        priv.append(c.private())
    for _ in range(nasserts):
        c.assert_equal(ws[int(rng.integers(0, len(ws)))], int(rng.integers(0, 2)))
    return c


def bitsliced(cc, bits, m):
    """witness bytes [nb, (m + 7) // 8] and holds [nb] from the gate program alone, 32 statements per word"""
    nb, nin = bits.shape
    ng = len(cc.gates)
    nw = nin + ng
    out_bits = np.zeros((nb, nw), dtype=np.uint8)
    holds = np.zeros(nb, dtype=bool)
    for s0 in range(0, nb, 32):
        blk = bits[s0: s0 + 32] & 1
        n = len(blk)
        weights = (np.uint32(1) << np.arange(n, dtype=np.uint32))[:, None]
        st = np.zeros(nw + 1, dtype=np.uint32)
        st[1: nin + 1] = (blk.astype(np.uint32) * weights).sum(axis=0, dtype=np.uint32)
        for g, (op, a, b) in enumerate(cc.gates):
            x, y = st[a], st[b]
            st[nin + 1 + g] = (x ^ y, x & y, x | y, ~x)[op]
        ok = np.uint32(0xFFFFFFFF)
        for w, v in cc.asserts:
            ok &= st[w] if v else ~st[w]
        mask = np.uint32((1 << n) - 1) if n < 32 else np.uint32(0xFFFFFFFF)
        holds[s0: s0 + n] = [(int(ok & mask) >> j) & 1 for j in range(n)]
        out_bits[s0: s0 + n] = ((st[1:][None, :] >> np.arange(n, dtype=np.uint32)[:, None]) & 1).astype(np.uint8)
    packed = np.packbits(out_bits, axis=1, bitorder="little")
    wit = np.zeros((nb, (m + 7) // 8), dtype=np.uint8)
    wit[:, : packed.shape[1]] = packed
    return wit, holds
