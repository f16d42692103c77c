"""32-bit words over one circuit.Circuit, and the ChaCha20 block function (RFC 8439) and the SHA-256 compression function (FIPS 180-4) written with them.

A word is a tuple of 32 wires, least significant bit first.  Costs, in gate wires (each also one SSP row besides the wire's bit row):
    add          64   bit 0 a half adder (XOR, AND), bits 1 .. 31 a full adder each (MAJ + SUM3; the last carry is unused)
    sum          34 .. 38 wires and 4 more rows than wires, for k words at once: two weighted-sum gates (Circuit.wsum) on 16-bit limbs.
                      k = 2: 34 wires / 38 rows; k = 3, 4: 36 / 40; k = 5 .. 8: 38 / 42 (an add is 64 wires / 128 rows for every two words)
    xor / and_ / or_ / not_   32
    ch           96   z ^ (x & (y ^ z))
    maj          32   one MAJ per bit
    less_than     2 n   for two n-bit operands: a NOT and a MAJ a bit (the borrow chain of a - b); 4 n rows
    ripple        2 n   for two n-bit operands of any width: a full adder a bit, the carry out returned; subtract=True 3 n + 1 (a NOT a bit, the borrow out)
    rotl / rotr   0   rewiring only
    shr           0   the vacated bits are the circuit's shared zero wire (1 wire for the whole circuit)
    const         0   the shared zero and one wires (at most 2 for the whole circuit)
    assert_u32        32 value assertions (rows, no wires)
    assert_same_u32   32 equalities (rows, no wires)
    output            32 computed public outputs (Circuit.output): 32 public wires and 32 equality rows

    w = Words()
    x, y = w.public(), w.private()
    w.assert_u32(w.add(w.rotl(x, 7), y), 0xDEADBEEF)
    cc = w.c.compile(mf.DEFAULT)
    bits = np.concatenate([pack([x_value]), pack([y_value])], axis=1)   # public words, then private words, as Context.circuit_assign takes them

The ChaCha20 block statement (ChaCha20Block) takes 32 642 wires and 64 900 rows: it fits d = 2^16 (m = 43 690) and the LDS kernel.
The SHA-256 compression statement (Sha256Compress) takes 61 698 wires and 122 884 rows (61 954 and 123 140 with a public chaining value): it fits
d = 2^17 (m = 87 381), above the LDS kernel's wire limit, so its witnesses come from the device-memory kernel and its SSP is the row SSP.
Written with sums (Sha256Compress(adds="sum")) it takes 28 114 wires and 49 588 rows (28 370 and 49 844 with a public chaining value): it fits
d = 2^16 (m = 43 690) and the LDS kernel.

Whole statements built from that compression, the result 256 computed public outputs (lu = 256; MerkleUpdate has two results, lu = 512):
    Sha256Message(length)   "I know a `length`-byte message with this digest": the padding of FIPS 180-4 5.1.1 is constant wires, part of the statement.
                            length -> (wires, rows): 0 -> (27 588, 49 062), 55 -> (28 042, 49 516): one block, d = 2^16 and the LDS kernel;
                            56 -> (55 382, 98 072), 100 -> (55 746, 98 436), 119 -> (55 898, 98 588): two blocks, d = 2^17 (m = 87 381);
                            120 -> (83 238, 147 144): three blocks.
    MerklePath(depth)       "I know a leaf and a path of `depth` siblings to this root", parent = compress(IV, left || right) (one compression, no
                            padding block).  28 625 depth + 514 wires, 50 865 depth + 772 rows: depth 1 -> (29 139, 51 637), 2 -> (57 764, 102 502),
                            3 -> (86 389, 153 367); depth 20 -> (573 014, 1 018 072) fits d = 2^20 (m = 699 050) and the device-memory kernel.
    MerkleRecord(length, depth)   "I know a `length`-byte record and a path of `depth` siblings, such that SHA-256(record) is a leaf of the tree with this
                            root": Sha256Message's chain into MerklePath's levels.  Sha256Message(length)'s sizes plus 28 625 depth wires and 50 865 depth
                            rows: (55, 1) -> (56 667, 100 381); at d = 2^20 (m = 699 050) records up to 55 bytes reach depth 19, up to 119 bytes depth 18.
    MerkleUpdate(depth)     "I know an old leaf, a new leaf and a path of `depth` siblings that takes the old leaf to old_root and the new leaf to
                            new_root" (lu = 512): MerklePath's levels twice over shared siblings and directions.  56 993 depth + 1 026 wires, 101 473
                            depth + 1 540 rows: depth 1 -> (58 019, 103 013), 2 -> (115 012, 204 486); depth 10 -> (570 956, 1 016 270) fits d = 2^20.
    MerkleRecordUpdate(length, depth, frozen=None)   "I know an old and a new `length`-byte record and a path of `depth` siblings that takes SHA-256(old
                            record) to old_root and SHA-256(new record) to new_root" (lu = 512); frozen=(lo, hi) adds "bytes [lo, hi) did not change".
                            MerkleUpdate(depth)'s sizes plus twice Sha256Message(length)'s less (1 028, 1 544): (55, 1) -> (113 075, 200 501) fits
                            d = 2^18; at d = 2^20 records up to 55 bytes reach depth 9, up to 119 bytes depth 8.
    MerkleAbsent(key_bytes, length, depth)   "the key q is not in the set behind this root" for an indexed table of records (lo | hi | payload): MerkleRecord's
                            body plus "lo < q < hi" (two Words.less_than), q public (lu = 256 + 8 key_bytes).  MerkleRecord(length, depth)'s sizes plus 40
                            key_bytes wires and 72 key_bytes + 2 rows: (4, 8, 1) -> (56 444, 100 288) fits d = 2^17; (8, 55, 19) fits d = 2^20.  Sound
                            relative to the table's invariant (the class has it); indexed_records / indexed_insert make and extend such tables.
    MerkleInsert(key_bytes, length, depth, joined=True)   "key k was inserted into the indexed table, and that alone takes the tree from R to R'"; joined=False
                            outputs all four chain tops (lu = 1024 + 8 key_bytes): segment 0 of an insert into a tree deeper than one circuit.
    MerkleRemove(key_bytes, length, depth, joined=True)   "key k was removed from the indexed table, and that alone takes the tree from R to R'": the
                            inverse step, three record chains and a constant inert leaf; the same public wires and joined=False form as MerkleInsert.
    MerkleTransfer(key_bytes, length, depth, amount_bytes=8, joined=True)   "v moved from the account k_from to the account k_to, and that alone takes the
                            tree from R to R'": two live records whose balances (bytes [2K, 2K + A), big-endian) become b_p - v and b_s + v with no borrow
                            and no carry; lu = 512 + 16 key_bytes + 8 amount_bytes; the same joined=False form.
    MerkleAdjust(key_bytes, length, depth, amount_bytes=8)   "the balance of the account k went up by v (side 0, a deposit) or down by v (side 1, a
                            withdrawal), and that alone takes the tree from R to R'": ONE live record whose balance becomes b + v or b - v through one ripple
                            with the side as carry in, the carry out tied to the side; lu = 512 + 8 (key_bytes + amount_bytes + 1); MerkleRecordUpdate's
                            depth range, (8, 55, 9, 8) fits d = 2^20.
    MerkleWrite(key_bytes, length, depth, field, expect=False)   "bytes [lo, hi) of the record of key k were set to v [, having been e], and that alone takes
                            the tree from R to R'": the put, plain or compare-and-set; ONE live record whose field's wires are replaced by v's; lu = 512 +
                            8 (key_bytes + F), 8 F more with expect=True; (8, 55, 9, (16, 55), True) fits d = 2^20.
    MerkleSegment(levels)   "one node changed from X to X', and that alone takes its ancestor `levels` levels up from Y to Y'" (lu = 1024, the two nodes
                            given, the two tops computed): one level range of a path cut by segment_levels(depth, cuts); MerkleUpdate's sizes, 10 levels
                            fit d = 2^20.  chain(nodes) turns the published node pairs of a transition into the upper segments' statements.
Context.ssp_rows_violations(witness) tells which rows of the registered statement a witness violates, Compiled.row_source(j) what row j constrains.
"""
from __future__ import annotations

import hashlib

import numpy as np

from .circuit import Circuit, CircuitError

MASK = 0xFFFFFFFF


def pack(values):
    """input bits of words: uint8 [len(values) * 32], word i's bit j at 32 i + j (Circuit.evaluate / Context.circuit_assign order); values may also be a
    2-D array [nb, nwords], giving [nb, nwords * 32]"""
    v = np.asarray(values, dtype=np.uint64)
    bits = ((v[..., None] >> np.arange(32, dtype=np.uint64)) & 1).astype(np.uint8)
    return bits.reshape(v.shape[:-1] + (v.shape[-1] * 32,)) if v.ndim else bits


def unpack(bits):
    """the words of 32 bits each, LSB first: a list of ints from a 1-D array, else an array [..., nwords] of uint32"""
    b = np.asarray(bits, dtype=np.uint64)
    if b.shape[-1] % 32:
        raise CircuitError("unpack: the bit count must be a multiple of 32")
    w = (b.reshape(b.shape[:-1] + (b.shape[-1] // 32, 32)) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)
    return [int(x) for x in w] if w.ndim == 1 else w


class Words:
    """32-bit word operations on one Circuit (self.c)"""

    def __init__(self, circuit: Circuit | None = None):
        self.c = circuit if circuit is not None else Circuit()

    # -- inputs and constants -------------------------------------------------------------------------------------------
    def public(self, count=None):
        """one public input word, or a list of `count` of them"""
        if count is not None:
            return [self.public() for _ in range(count)]
        return tuple(self.c.public(32))

    def private(self, count=None):
        """one private input word, or a list of `count` of them"""
        if count is not None:
            return [self.private() for _ in range(count)]
        return tuple(self.c.private(32))

    def output(self, x):
        """a public word whose value is defined as that of x (32 computed public outputs, Circuit.output): the statement's position of x"""
        return tuple(self.c.output(a) for a in x)

    def const(self, value: int):
        """the word `value`: the circuit's shared constant wires, no new wire beyond them"""
        return tuple(self.c.const((value >> i) & 1) for i in range(32))

    # -- arithmetic and logic -------------------------------------------------------------------------------------------
    def add(self, x, y):
        """x + y mod 2^32: 64 wires"""
        out = [self.c.XOR(x[0], y[0])]
        carry = self.c.AND(x[0], y[0])
        for i in range(1, 32):
            s, carry = self.c.full_add(x[i], y[i], carry)
            out.append(s)
        return tuple(out)

    def sum(self, xs):
        """the sum of the k >= 1 words xs mod 2^32 through two weighted-sum gates on 16-bit limbs (a single 32-bit limb would be unsound: p is about
        2^32).  lo sums the low halves at shifts 0 .. 15; its output bits 16 and up are the carry count.  hi sums the high halves at shifts 0 .. 15 and
        lo's carry bits at shifts 0, 1, ..; its output bits 16 and up are discarded wires.  A constant operand (const) costs nothing: its zero bits are
        left out and its one bits are terms on the shared one wire.  CircuitError when k is so large that a gate would need more than 24 bits."""
        xs = [tuple(x) for x in xs]
        if not xs or any(len(x) != 32 for x in xs):
            raise CircuitError("sum: one or more words of 32 wires")
        if (len(xs) * 0xFFFF + len(xs)).bit_length() > 24:  # hi's largest sum: k limbs and a carry count below k
            raise CircuitError(f"sum: {len(xs)} words need a gate of more than 24 bits")

        def limb(bits, carries):
            terms = [(x[i], i % 16) for x in xs for i in bits if self.c.const_value(x[i]) != 0] + [(k, i) for i, k in enumerate(carries)]
            out = self.c.wsum(terms) if terms else []
            return [out[i] if i < len(out) else self.c.const(0) for i in range(16)], out[16:]

        lo, carries = limb(range(16), [])
        hi, _ = limb(range(16, 32), carries)
        return tuple(lo + hi)

    def xor(self, x, y):
        return tuple(self.c.XOR(a, b) for a, b in zip(x, y))

    def and_(self, x, y):
        return tuple(self.c.AND(a, b) for a, b in zip(x, y))

    def or_(self, x, y):
        return tuple(self.c.OR(a, b) for a, b in zip(x, y))

    def not_(self, x):
        return tuple(self.c.NOT(a) for a in x)

    def ch(self, x, y, z):
        """bitwise x ? y : z (SHA-2's Ch)"""
        return self.xor(z, self.and_(x, self.xor(y, z)))

    def maj(self, x, y, z):
        """bitwise majority (SHA-2's Maj)"""
        return tuple(self.c.MAJ(a, b, d) for a, b, d in zip(x, y, z))

    def less_than(self, a_bits, b_bits):
        """the wire "a < b" for two equal-length lists of wires, least significant first, read as unsigned integers: the final borrow of a - b,
        borrow' = MAJ(NOT a_i, b_i, borrow) from const(0).  Two wires (a NOT and a MAJ) and four rows a bit."""
        a_bits, b_bits = list(a_bits), list(b_bits)
        if not a_bits or len(a_bits) != len(b_bits):
            raise CircuitError("less_than: two lists of wires of one length, at least 1")
        borrow = self.c.const(0)
        for a, b in zip(a_bits, b_bits):
            borrow = self.c.MAJ(self.c.NOT(a), b, borrow)
        return borrow

    def ripple(self, a_bits, b_bits, subtract=False):
        """(the n wires of a + b mod 2^n, the carry out) for two equal-length lists of wires of ANY width n >= 1, least significant first, read as unsigned
        integers: one full adder a bit (Circuit.full_add: MAJ + SUM3) from the carry const(0) -- 2 n wires, 4 n rows.  subtract=True: (the n wires of
        a - b mod 2^n, the BORROW out, 1 when a < b) as a + NOT b + 1, the carry from const(1), the borrow the NOT of the last carry -- 3 n + 1 wires, 6 n + 2
        rows.  (add stays the 32-bit modular word addition.)"""
        a_bits, b_bits = list(a_bits), list(b_bits)
        if not a_bits or len(a_bits) != len(b_bits):
            raise CircuitError("ripple: two lists of wires of one length, at least 1")
        out, carry = [], self.c.const(1 if subtract else 0)
        for a, b in zip(a_bits, b_bits):
            s, carry = self.c.full_add(a, self.c.NOT(b) if subtract else b, carry)
            out.append(s)
        return out, self.c.NOT(carry) if subtract else carry

    # -- rewiring -------------------------------------------------------------------------------------------------------
    @staticmethod
    def rotl(x, n: int):
        n %= 32
        return tuple(x[(i - n) % 32] for i in range(32))

    @staticmethod
    def rotr(x, n: int):
        return Words.rotl(x, -n)

    def shr(self, x, n: int):
        """x >> n for n in [0, 32]: the top n bits are the shared zero wire"""
        if not 0 <= n <= 32:
            raise CircuitError("shr: the shift must be in [0, 32]")
        return tuple(x[i + n] if i + n < 32 else self.c.const(0) for i in range(32))

    # -- assertions -----------------------------------------------------------------------------------------------------
    def assert_u32(self, x, value: int):
        """x = value: 32 value assertions"""
        for i in range(32):
            self.c.assert_equal(x[i], (value >> i) & 1)

    def assert_same_u32(self, x, y):
        """x = y: 32 equalities"""
        for a, b in zip(x, y):
            self.c.assert_same(a, b)


# ---------------------------------------------------------------------------------------------------------------------- ChaCha20 (RFC 8439)
CHACHA_CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"


def quarter_round(w: Words, a, b, c, d):
    """RFC 8439 2.1 on four words: 4 adds, 4 xors, 4 rotations"""
    a = w.add(a, b); d = w.rotl(w.xor(d, a), 16)
    c = w.add(c, d); b = w.rotl(w.xor(b, c), 12)
    a = w.add(a, b); d = w.rotl(w.xor(d, a), 8)
    c = w.add(c, d); b = w.rotl(w.xor(b, c), 7)
    return a, b, c, d


def double_round(w: Words, x):
    """a column round and a diagonal round (RFC 8439 2.3) on the 16-word state x: 32 adds, 32 xors"""
    x = list(x)
    for i in (0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14):
        x[i[0]], x[i[1]], x[i[2]], x[i[3]] = quarter_round(w, *(x[j] for j in i))
    return x


def chacha20_block(w: Words, key, counter, nonce):
    """the 16 output words of the ChaCha20 block function (RFC 8439 2.3): key = 8 words, counter = 1 word, nonce = 3 words -- 336 adds, 320 xors"""
    state = [w.const(v) for v in CHACHA_CONSTANTS] + list(key) + [counter] + list(nonce)
    x = state
    for _ in range(10):
        x = double_round(w, x)
    return [w.add(a, b) for a, b in zip(x, state)]


def le_words(data: bytes):
    """little-endian 32-bit words of a byte string (RFC 8439's serialisation)"""
    if len(data) % 4:
        raise CircuitError("le_words: the length must be a multiple of 4")
    return [int.from_bytes(data[i: i + 4], "little") for i in range(0, len(data), 4)]


class ChaCha20Block:
    """The statement "I know a 256-bit key whose ChaCha20 block, at this public counter and nonce, is this public 64-byte block".

    Public inputs (lu = 640): the counter word, the 3 nonce words, the 16 block words; private: the 8 key words.  The computed block is tied to the
    public one by 512 equalities.  32 642 wires (896 inputs, 2 constants, 336 adds x 64, 320 xors x 32) and 64 900 rows."""

    def __init__(self):
        self.w = w = Words()
        self.counter = w.public()
        self.nonce = w.public(3)
        self.block = w.public(16)
        self.key = w.private(8)
        self.out = chacha20_block(w, self.key, self.counter, self.nonce)
        for o, b in zip(self.out, self.block):
            w.assert_same_u32(o, b)

    @property
    def circuit(self) -> Circuit:
        return self.w.c

    @staticmethod
    def public_bits(counter: int, nonce: bytes, block: bytes):
        """the 640 public bits: counter, nonce (12 bytes), block (64 bytes)"""
        if len(nonce) != 12 or len(block) != 64:
            raise CircuitError("ChaCha20Block: the nonce is 12 bytes and the block 64")
        return pack([counter & MASK] + le_words(nonce) + le_words(block))

    @staticmethod
    def private_bits(key: bytes):
        """the 256 private bits of a 32-byte key"""
        if len(key) != 32:
            raise CircuitError("ChaCha20Block: the key is 32 bytes")
        return pack(le_words(key))

    def bits(self, key: bytes, counter: int, nonce: bytes, block: bytes):
        """one statement's 896 input bits, public then private (a row of Context.circuit_assign's input)"""
        return np.concatenate([self.public_bits(counter, nonce, block), self.private_bits(key)])


# ---------------------------------------------------------------------------------------------------------------------- SHA-256 (FIPS 180-4)
SHA256_IV = (0x6A09E667, 0xBB67AE85, 0x3C6EF372, 0xA54FF53A, 0x510E527F, 0x9B05688C, 0x1F83D9AB, 0x5BE0CD19)
SHA256_K = (
    0x428A2F98, 0x71374491, 0xB5C0FBCF, 0xE9B5DBA5, 0x3956C25B, 0x59F111F1, 0x923F82A4, 0xAB1C5ED5, 0xD807AA98, 0x12835B01, 0x243185BE, 0x550C7DC3,
    0x72BE5D74, 0x80DEB1FE, 0x9BDC06A7, 0xC19BF174, 0xE49B69C1, 0xEFBE4786, 0x0FC19DC6, 0x240CA1CC, 0x2DE92C6F, 0x4A7484AA, 0x5CB0A9DC, 0x76F988DA,
    0x983E5152, 0xA831C66D, 0xB00327C8, 0xBF597FC7, 0xC6E00BF3, 0xD5A79147, 0x06CA6351, 0x14292967, 0x27B70A85, 0x2E1B2138, 0x4D2C6DFC, 0x53380D13,
    0x650A7354, 0x766A0ABB, 0x81C2C92E, 0x92722C85, 0xA2BFE8A1, 0xA81A664B, 0xC24B8B70, 0xC76C51A3, 0xD192E819, 0xD6990624, 0xF40E3585, 0x106AA070,
    0x19A4C116, 0x1E376C08, 0x2748774C, 0x34B0BCB5, 0x391C0CB3, 0x4ED8AA4A, 0x5B9CCA4F, 0x682E6FF3, 0x748F82EE, 0x78A5636F, 0x84C87814, 0x8CC70208,
    0x90BEFFFA, 0xA4506CEB, 0xBEF9A3F7, 0xC67178F2,
)


def _xor3(w: Words, x, y, z):
    return w.xor(w.xor(x, y), z)


def sha256_compress(w: Words, H, M):
    """the 8 words of the SHA-256 compression function (FIPS 180-4 6.2.2): H = the 8 words of the incoming hash value, M = the 16 words of one block
    (big-endian words of the bytes, be_words).  48 schedule words of 2 x 2 xors and 3 adds, 64 rounds of 4 xors, Ch, Maj and 7 adds, 8 final adds:
    600 adds, 448 xors, 64 Ch, 64 Maj -- 60 928 gate wires, and the circuit's two constant wires.  The adds of a round are ordered so that the words
    that are ready early (h, K_t, W_t, then Ch and Sigma_1) are summed first and the ripple carries of consecutive adds overlap."""
    H, W = list(H), list(M)
    if len(H) != 8 or len(W) != 16:
        raise CircuitError("sha256_compress: H is 8 words and M 16")
    for t in range(16, 64):
        s0 = _xor3(w, w.rotr(W[t - 15], 7), w.rotr(W[t - 15], 18), w.shr(W[t - 15], 3))
        s1 = _xor3(w, w.rotr(W[t - 2], 17), w.rotr(W[t - 2], 19), w.shr(W[t - 2], 10))
        W.append(w.add(w.add(W[t - 16], s0), w.add(W[t - 7], s1)))
    a, b, c, d, e, f, g, h = H
    for t in range(64):
        S1 = _xor3(w, w.rotr(e, 6), w.rotr(e, 11), w.rotr(e, 25))
        S0 = _xor3(w, w.rotr(a, 2), w.rotr(a, 13), w.rotr(a, 22))
        t1 = w.add(w.add(w.add(h, w.add(w.const(SHA256_K[t]), W[t])), w.ch(e, f, g)), S1)
        t2 = w.add(S0, w.maj(a, b, c))
        a, b, c, d, e, f, g, h = w.add(t1, t2), a, b, c, w.add(d, t1), e, f, g
    return [w.add(x, y) for x, y in zip(H, (a, b, c, d, e, f, g, h))]


def sha256_compress_sum(w: Words, H, M):
    """sha256_compress with every addition a Words.sum: per round a' = sum(h, K_t, W_t, e & f, ~e & g, Sigma_1, Sigma_0, Maj) and
    e' = sum(d, h, K_t, W_t, e & f, ~e & g, Sigma_1) -- Ch = (e & f) + (~e & g), the two addends being disjoint, one AND and one ANDN per bit -- the
    schedule word sum(W[t - 16], sigma_0, W[t - 7], sigma_1) and the eight final sum(H_i, x_i).  184 sums, 448 xors, 64 x (AND, ANDN, MAJ):
    27 344 gate wires, and the circuit's two constant wires; about 4 levels per round."""
    H, W = list(H), list(M)
    if len(H) != 8 or len(W) != 16:
        raise CircuitError("sha256_compress_sum: H is 8 words and M 16")
    for t in range(16, 64):
        s0 = _xor3(w, w.rotr(W[t - 15], 7), w.rotr(W[t - 15], 18), w.shr(W[t - 15], 3))
        s1 = _xor3(w, w.rotr(W[t - 2], 17), w.rotr(W[t - 2], 19), w.shr(W[t - 2], 10))
        W.append(w.sum([W[t - 16], s0, W[t - 7], s1]))
    a, b, c, d, e, f, g, h = H
    for t in range(64):
        S1 = _xor3(w, w.rotr(e, 6), w.rotr(e, 11), w.rotr(e, 25))
        S0 = _xor3(w, w.rotr(a, 2), w.rotr(a, 13), w.rotr(a, 22))
        ef = w.and_(e, f)
        neg = tuple(w.c.ANDN(y, x) for x, y in zip(e, g))  # ~e & g
        t1 = [h, w.const(SHA256_K[t]), W[t], ef, neg, S1]
        a, b, c, d, e, f, g, h = w.sum(t1 + [S0, w.maj(a, b, c)]), a, b, c, w.sum([d] + t1), e, f, g
    return [w.sum([x, y]) for x, y in zip(H, (a, b, c, d, e, f, g, h))]


def be_words(data: bytes):
    """big-endian 32-bit words of a byte string (FIPS 180-4's convention)"""
    if len(data) % 4:
        raise CircuitError("be_words: the length must be a multiple of 4")
    return [int.from_bytes(data[i: i + 4], "big") for i in range(0, len(data), 4)]


def sha256_pad(message: bytes) -> bytes:
    """the message padded to whole 64-byte blocks (FIPS 180-4 5.1.1): 0x80, zeros, the bit length as 8 big-endian bytes"""
    message = bytes(message)
    return message + b"\x80" + bytes((55 - len(message)) % 64) + (8 * len(message)).to_bytes(8, "big")


class Sha256Compress:
    """The statement "I know a 64-byte block whose SHA-256 compression, from this chaining value, is this value".

    chaining="iv": the chaining value is the constant SHA256_IV, so the statement is the digest of a one-block padded message: lu = 256, the eight result
    words as computed public outputs; 61 698 wires (768 inputs, 2 constants, 60 928 gates) and 122 884 rows.
    chaining="public": the incoming chaining value is public too, ahead of the result (lu = 512: bits [0, 256) the chaining value, [256, 512) the
    result) -- what a caller hashing several blocks, or a Merkle path, chains from statement to statement; 61 954 wires and 123 140 rows.
    The block is private (512 bits).  Both fit Params(d=1 << 17, m=87381).  The result is computed, not given: bits() leaves its positions zero,
    Circuit.assign / Context.circuit_assign write it into the witness row, and digest_of reads the 32 bytes back.
    adds="ripple" (the default) is the circuit above, every addition a Words.add.  adds="sum" writes the additions as Words.sum
    (sha256_compress_sum): the same statement in 28 114 wires and 49 588 rows ("iv"; 28 370 and 49 844 for "public"), which fits
    Params(d=1 << 16, m=43690) and the LDS witness kernel."""

    def __init__(self, chaining="iv", adds="ripple"):
        if chaining not in ("iv", "public"):
            raise CircuitError("Sha256Compress: chaining is 'iv' or 'public'")
        if adds not in ("ripple", "sum"):
            raise CircuitError("Sha256Compress: adds is 'ripple' or 'sum'")
        self.chaining = chaining
        self.adds = adds
        self.w = w = Words()
        self.h_in = w.public(8) if chaining == "public" else [w.const(v) for v in SHA256_IV]
        self.block = w.private(16)
        self.out = (sha256_compress_sum if adds == "sum" else sha256_compress)(w, self.h_in, self.block)
        self.digest = [w.output(x) for x in self.out]
        self.digest_at = 256 if chaining == "public" else 0  # the result's first bit in the statement

    @property
    def circuit(self) -> Circuit:
        return self.w.c

    @property
    def lu(self) -> int:
        return self.digest_at + 256

    def public_bits(self, chaining: bytes | None = None):
        """the lu public bits: the 32-byte chaining value (chaining="public" only), then 256 zeros where the result is computed"""
        if (chaining is not None) != (self.chaining == "public"):
            raise CircuitError("Sha256Compress: a chaining value goes with chaining='public', and only with it")
        if chaining is not None and len(chaining) != 32:
            raise CircuitError("Sha256Compress: the chaining value is 32 bytes")
        head = pack(be_words(chaining)) if chaining is not None else np.zeros(0, dtype=np.uint8)
        return np.concatenate([head, np.zeros(256, dtype=np.uint8)])

    @staticmethod
    def private_bits(block: bytes):
        """the 512 private bits of a 64-byte block"""
        if len(block) != 64:
            raise CircuitError("Sha256Compress: the block is 64 bytes")
        return pack(be_words(block))

    def bits(self, block: bytes, chaining: bytes | None = None):
        """one statement's input bits, public then private (a row of Context.circuit_assign's input), the result's positions zero"""
        return np.concatenate([self.public_bits(chaining), self.private_bits(block)])

    def digest_of(self, witness_row) -> bytes:
        """the 32 bytes of the computed result, from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        row = np.frombuffer(bytes(bytearray(witness_row)[: self.lu // 8]), dtype=np.uint8)
        bits = np.unpackbits(row, bitorder="little")[self.digest_at: self.digest_at + 256]
        return b"".join(v.to_bytes(4, "big") for v in unpack(bits))


def _digest_from_row(witness_row, at: int) -> bytes:
    """the 32 bytes of the eight computed words at statement bits [at, at + 256) of a witness row"""
    row = np.frombuffer(bytes(bytearray(witness_row)[: (at + 256) // 8]), dtype=np.uint8)
    bits = np.unpackbits(row, bitorder="little")[at: at + 256]
    return b"".join(v.to_bytes(4, "big") for v in unpack(bits))


def _message_chain(w: Words, message, length: int):
    """(the eight words of SHA-256 of the `length`-byte message whose 8 * length bit wires are `message`, the number of blocks): the padding of FIPS 180-4
    5.1.1 as constant wires, the compressions (sha256_compress_sum) chained from the constant SHA256_IV -- the body of Sha256Message and MerkleRecord"""
    tail = sha256_pad(bytes(length))[length:]  # the padding depends on the length alone
    blocks = (length + len(tail)) // 64

    def byte(k):  # the 8 wires of padded byte k, LSB first
        if k < length:
            return message[8 * k: 8 * k + 8]
        return [w.c.const((tail[k - length] >> b) & 1) for b in range(8)]

    h = [w.const(v) for v in SHA256_IV]
    for blk in range(blocks):
        # big-endian words: bit i of word t is bit i % 8 of byte 4 t + 3 - i // 8
        M = [tuple(byte(64 * blk + 4 * t + 3 - i // 8)[i % 8] for i in range(32)) for t in range(16)]
        h = sha256_compress_sum(w, h, M)
    return h, blocks


def _merkle_levels(w: Words, cur, siblings, dirs):
    """the eight words of the root above the node `cur` (8 words): per level a conditional swap, four gates a bit -- t = AND(dir, XOR(cur, sib)),
    L = XOR(cur, t), R = XOR(sib, t) -- then parent = sha256_compress_sum(IV, L || R) -- the body of MerklePath and MerkleRecord"""
    iv = [w.const(v) for v in SHA256_IV]
    for sib, d in zip(siblings, dirs):
        left, right = [], []
        for x, y in zip(cur, sib):
            t = tuple(w.c.AND(d, a) for a in w.xor(x, y))
            left.append(w.xor(x, t))
            right.append(w.xor(y, t))
        cur = sha256_compress_sum(w, iv, left + right)
    return cur


def _statement_of(digest: bytes, who: str) -> bytes:
    """the 32 statement bytes (bits [0, 256) of a witness row) of eight computed words whose big-endian bytes are `digest`: each word's 4 bytes reversed"""
    digest = bytes(digest)
    if len(digest) != 32:
        raise CircuitError(f"{who} is 32 bytes")
    return b"".join(digest[i: i + 4][::-1] for i in range(0, 32, 4))


class _Statement:
    """Private base of Sha256Message and the Merkle statements: the argument checks and the pieces of bits() they share, every refusal under the public
    class's own name.  A statement's nin input bits, public then private, packed eight to a byte (least significant first) are its packed input row, one
    layout for all of them (MerkleTree's *_rows write it on the device; csrc/merkle_rows.hpp): 32 or 64 zero bytes where the root(s) are computed
    (MerkleAbsent: and the key) | the head (leaves as words, records as bytes) | depth siblings of 32 bytes as words | ceil(depth / 8) index bytes.
    MerkleInsert's row has two paths: 64 zero bytes | the key | old_p | old_s | new_s | depth siblings of p | depth siblings of s | ceil(2 depth / 8) index
    bytes, bit l < depth = bit l of p, bit depth + l = bit l of s: 64 + key_bytes + 3 length + 64 depth + ceil(2 depth / 8) bytes.  MerkleRemove's row is
    that without new_s: 64 + key_bytes + 2 length + 64 depth + ceil(2 depth / 8) bytes."""

    def _arg(self, value, lo, hi, what):
        if not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
            raise CircuitError(f"{type(self).__name__}: {what}")
        return int(value)

    def _length_arg(self, length):
        return self._arg(length, 0, None, "the length is a non-negative number of bytes")

    def _depth_arg(self, depth):
        return self._arg(depth, 1, None, "the depth is at least 1")

    def _tail_wires(self):
        """the private wires behind the head: `depth` siblings of 8 words from the leaf's level up, then `depth` direction bits"""
        self.siblings = [self.w.private(8) for _ in range(self.depth)]
        self.dirs = self.w.c.private(self.depth)

    @property
    def circuit(self) -> Circuit:
        return self.w.c

    @property
    def nin(self) -> int:
        """the input bits, public then private: len(bits(...)), and nwires - len(program) of the compiled circuit"""
        return self.w.c.lu + len(self.w.c._priv)

    @property
    def row_bytes(self) -> int:
        """the bytes of the packed input row: ceil(nin / 8)"""
        return (self.nin + 7) // 8


# The pieces of the statements' bits().  Functions of the sizes, not methods: bits() reads self.depth and self.length alone, so it also serves a stand-in that
# has only those (a model of a statement too deep to build); `who` is the public class's name, for the refusals.
def _input_bits(computed: int, *parts):
    """`computed` zeros where the public outputs are computed, then the given bits"""
    return np.concatenate([np.zeros(computed, dtype=np.uint8), *parts])


def _record_bits(who: str, length: int, *records, what="the record is"):
    """the bits of byte strings of `length` bytes each, byte k's bit b (LSB first) at 8 k + b"""
    records = [bytes(r) for r in records]
    if any(len(r) != length for r in records):
        raise CircuitError(f"{who}: {what} {length} bytes")
    return np.unpackbits(np.frombuffer(b"".join(records), dtype=np.uint8), bitorder="little")


def _tail_bits(who: str, depth: int, siblings, index: int, leaves=(), what=""):
    """the bits of `leaves` (32-byte heads, refused together with the siblings: `what` names them) and of the `depth` siblings, as big-endian words, then the
    direction bits = the bits of the leaf's index, least significant first"""
    leaves, siblings = [bytes(x) for x in leaves], [bytes(s) for s in siblings]
    if len(siblings) != depth or any(len(x) != 32 for x in leaves + siblings):
        raise CircuitError(f"{who}: {what}{depth} siblings of 32 bytes")
    if not 0 <= index < 1 << depth:
        raise CircuitError(f"{who}: the index is in [0, 2^{depth})")
    dirs = np.array([(index >> l) & 1 for l in range(depth)], dtype=np.uint8)
    return np.concatenate([pack(be_words(b"".join(leaves + siblings))), dirs])


class _OneRoot(_Statement):
    """a statement whose public outputs are one root, at statement bits [0, 256)"""

    @property
    def lu(self) -> int:
        return 256

    def root_of(self, witness_row) -> bytes:
        """the 32 bytes of the computed root, from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return _digest_from_row(witness_row, 0)

    @classmethod
    def statement(cls, root: bytes) -> bytes:
        """the 32 statement bytes (what verify_public takes, bits [0, lu) of a witness row) that say "the root is `root`": each word's 4 bytes reversed, the
        inverse of root_of -- a verifier checks a proof against a root it knows without a witness row"""
        return _statement_of(root, f"{cls.__name__}: the root")


class _TwoRoots(_Statement):
    """a statement whose public outputs are the old root at statement bits [0, 256) and the new root at [256, 512)"""

    @property
    def lu(self) -> int:
        return 512

    def _root_outputs(self, old_leaf, new_leaf):
        """MerklePath's levels twice over the shared sibling and direction wires, then the two roots' outputs"""
        self.out_old = _merkle_levels(self.w, old_leaf, self.siblings, self.dirs)
        self.out_new = _merkle_levels(self.w, new_leaf, self.siblings, self.dirs)
        self.old_root = [self.w.output(x) for x in self.out_old]
        self.new_root = [self.w.output(x) for x in self.out_new]

    def roots_of(self, witness_row):
        """(old_root, new_root), 32 bytes each, as computed: from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return _digest_from_row(witness_row, 0), _digest_from_row(witness_row, 256)

    @classmethod
    def statement(cls, old_root: bytes, new_root: bytes) -> bytes:
        """the 64 statement bytes (what verify_public takes, bits [0, 512) of a witness row) that say "old_root became new_root": the inverse of
        roots_of, each half MerklePath.statement's bytes"""
        return _statement_of(old_root, f"{cls.__name__}: the old root") + _statement_of(new_root, f"{cls.__name__}: the new root")


class Sha256Message(_Statement):
    """The statement "I know a `length`-byte message whose SHA-256 digest is this value".

    Private inputs: the 8 * length message bits, byte k's bit b (LSB first) at private index 8 k + b -- np.unpackbits(message, bitorder="little").  The
    padding of FIPS 180-4 5.1.1 (sha256_pad: 0x80, zeros, the bit length) is constant wires: it costs nothing and it is part of the statement, so a proof
    says the digest is that of a message of exactly `length` bytes (Sha256Compress leaves the padding to the caller).  len(sha256_pad) / 64 compressions
    (sha256_compress_sum) are chained from the constant SHA256_IV; the digest is 256 computed public outputs (lu = 256).  bits() leaves the digest's
    positions zero, Circuit.assign / Context.circuit_assign write them, digest_of reads the 32 bytes back.  Sizes: SHA256_MESSAGE_SIZES."""

    def __init__(self, length: int):
        self.length = length = self._length_arg(length)
        self.w = w = Words()
        self.message = w.c.private(8 * length)
        h, self.blocks = _message_chain(w, self.message, length)
        self.out = h
        self.digest = [w.output(x) for x in h]

    @property
    def lu(self) -> int:
        return 256

    def bits(self, message: bytes):
        """one statement's input bits, public then private (a row of Context.circuit_assign's input): 256 zeros where the digest is computed, then the message"""
        return _input_bits(256, _record_bits("Sha256Message", self.length, message, what="the message is"))

    def digest_of(self, witness_row) -> bytes:
        """the 32 bytes of the computed digest, from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return _digest_from_row(witness_row, 0)

    @staticmethod
    def statement(digest: bytes) -> bytes:
        """the 32 statement bytes (what verify_public takes, bits [0, lu) of a witness row) that say "the digest is `digest`": each word's 4 bytes reversed,
        the inverse of digest_of, as MerklePath.statement -- a verifier checks a proof against a digest it knows (one of Context.sha256_records, say)
        without a witness row"""
        return _statement_of(digest, "Sha256Message: the digest")


class MerklePath(_OneRoot):
    """The statement "I know a leaf and an authentication path of `depth` siblings to this root".

    The node function is parent = compress(IV, left || right): ONE SHA-256 compression of the 64-byte concatenation from the constant SHA256_IV, with no
    padding block -- the usual 2-to-1 compression tree, not SHA-256 of a 64-byte message (which would be two compressions).
    Private inputs, in this order: the leaf (8 words, big-endian words of its 32 bytes), then per level its sibling (8 words), then `depth` direction
    bits, bit l = 1 meaning the current node is the RIGHT child at level l (level 0 is the leaf's: bit l of the leaf's index).  Per level a conditional
    swap, four gates a bit -- t = AND(dir, XOR(cur, sib)), L = XOR(cur, t), R = XOR(sib, t) -- then sha256_compress_sum.  The root is 256 computed
    public outputs (lu = 256).  28 625 depth + 514 wires and 50 865 depth + 772 rows (MERKLE_PATH_SIZES): depth 20 is 573 014 wires and 1 018 072 rows,
    which fits Params(d=1 << 20, m=699050)."""

    def __init__(self, depth: int):
        self.depth = self._depth_arg(depth)
        self.w = w = Words()
        self.leaf = w.private(8)
        self._tail_wires()
        self.out = cur = _merkle_levels(w, self.leaf, self.siblings, self.dirs)
        self.root = [w.output(x) for x in cur]

    def bits(self, leaf: bytes, siblings, index: int):
        """one statement's input bits, public then private: 256 zeros where the root is computed, the leaf, the siblings from the leaf's level up, then
        the direction bits = the bits of the leaf's index, least significant first"""
        return _input_bits(256, _tail_bits("MerklePath", self.depth, siblings, index, (leaf,), "a 32-byte leaf and "))


class MerkleRecord(_OneRoot):
    """The statement "I know a `length`-byte record and an authentication path of `depth` siblings, such that SHA-256(record) is a leaf of the tree with
    this root": Sha256Message's block chain over the private record bits (the padding constant wires, part of the statement), its eight output words
    fed, in place of MerklePath's private leaf, into MerklePath's levels (the same conditional swap and parent = compress(IV, left || right)).  It ties a
    membership proof to the data: the tree is the one Context.merkle_tree keeps, its leaves made by MerkleTree.set_records.
    Private inputs, in this order: the 8 * length record bits, byte k's bit b (LSB first) at 8 k + b; `depth` siblings of 8 words each (big-endian words
    of their 32 bytes), from the leaf's level up; `depth` direction bits, bit l of the leaf's index.  The root is 256 computed public outputs (lu = 256),
    and statement(root) is MerklePath.statement's bytes.  MerkleTree.record_rows / record_bits give the input rows for records of a device tree.
    Sizes (MERKLE_RECORD_SIZES): exactly those of Sha256Message(length) plus 28 625 depth wires and 50 865 depth rows.  At Params(d=1 << 20, m=699050)
    records of up to 55 bytes (one block) reach depth 19 (571 917 wires, 1 015 951 rows) and records of up to 119 bytes (two blocks) depth 18 (571 148
    wires, 1 014 158 rows); (55, 20) does not fit: 1 066 816 rows.  A deeper tree is read with the path cut (segment_levels): MerkleRecord(length, c_0) over
    the leaf's subtree, MerkleClimb above it (MerkleTree.record_segments)."""

    def __init__(self, length: int, depth: int):
        self.length, self.depth = length, depth = self._length_arg(length), self._depth_arg(depth)
        self.w = w = Words()
        self.record = w.c.private(8 * length)
        self._tail_wires()
        self.leaf, self.blocks = _message_chain(w, self.record, length)
        self.out = cur = _merkle_levels(w, self.leaf, self.siblings, self.dirs)
        self.root = [w.output(x) for x in cur]

    def bits(self, record: bytes, siblings, index: int):
        """one statement's input bits, public then private: 256 zeros where the root is computed, the record's bits, the siblings from the leaf's level
        up, then the direction bits = the bits of the leaf's index, least significant first"""
        return _input_bits(256, _record_bits("MerkleRecord", self.length, record), _tail_bits("MerkleRecord", self.depth, siblings, index))


class MerkleUpdate(_TwoRoots):
    """The statement "I know an old leaf, a new leaf, `depth` siblings and an index such that the path from the old leaf gives old_root and the SAME
    siblings and directions from the new leaf give new_root": one leaf changed, and that change alone takes the tree from old_root to new_root.

    Private inputs, in this order: the old leaf (8 words, big-endian words of its 32 bytes, as MerklePath), the new leaf (8 words), `depth` siblings of 8
    words from the leaf's level up, `depth` direction bits (bit l of the index).  The body is MerklePath's levels (_merkle_levels) twice over the shared
    sibling and direction wires.  Public outputs (lu = 512): the old root's 8 words at statement bits [0, 256), the new root's at [256, 512), all computed.
    MerkleTree.update_rows / update_bits give the input rows of a batch of sequential updates of a device tree, and statement k is (R_k, R_k+1).
    Sizes (MERKLE_UPDATE_SIZES): 56 993 depth + 1 026 wires and 101 473 depth + 1 540 rows, i.e. twice MerklePath's less the 257 wires and bit rows a level
    that are shared (and the two shared constant wires); nwires - len(program) = 1024 + 257 depth inputs.  Depth 10 is 570 956 wires and 1 016 270 rows,
    which fits Params(d=1 << 20, m=699050); depth 11 (1 117 743 rows) does not.  Depth 1 fits Params(d=1 << 17, m=87381), depth 2
    Params(d=1 << 18, m=174762)."""

    def __init__(self, depth: int):
        self.depth = self._depth_arg(depth)
        self.w = w = Words()
        self.old_leaf = w.private(8)
        self.new_leaf = w.private(8)
        self._tail_wires()
        self._root_outputs(self.old_leaf, self.new_leaf)

    def bits(self, old_leaf: bytes, new_leaf: bytes, siblings, index: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed, the old leaf, the new leaf, the siblings from the
        leaf's level up, then the direction bits = the bits of the leaf's index, least significant first"""
        return _input_bits(512, _tail_bits("MerkleUpdate", self.depth, siblings, index, (old_leaf, new_leaf), "two 32-byte leaves and "))


class MerkleSegment(_Statement):
    """The statement "one node changed from X to X', and that change alone takes its ancestor `levels` levels up from Y to Y'": MerkleUpdate's body with the
    two leaves made PUBLIC -- one level range of a path that is too deep for one circuit (segment_levels cuts it).

    A deep transition R -> R' is proved per level range.  With cuts c_0 < .. < c_G-1 segment 0 is an existing statement (MerkleUpdate, MerkleRecordUpdate,
    MerkleInsert(joined=False)) over the subtree of height c_0 that holds the leaf, its "roots" the old and new value of the level-c_0 node on the path, and
    segment g >= 1 is MerkleSegment(c_g - c_g-1) (c_G = the depth).  The prover publishes the node pairs (X_g, X_g'), g = 0 .. G, (X_G, X_G') = (R, R'); the
    verifier builds every segment's statement bytes from that ONE list (chain), so adjacent segments agree by construction, and checks one proof a segment.
    Soundness is MerkleUpdate's applied G + 1 times: within a segment the old and the new pass share siblings and directions, so nothing but the lower node
    changed below its top.  A segment's private index bits need not be consistent with its neighbours'.
    WHAT BECOMES PUBLIC: the intermediate nodes (X_g, X_g'), 0 <= g < G.  They are hashes; nothing else is revealed.
    Public wires, in this order (public wires are laid out in declaration order, so the given ones come first): the old node as 8 given words at statement bits
    [0, 256), the new node at [256, 512), the old top as 256 computed outputs at [512, 768), the new top at [768, 1024); lu = 1024.  Private inputs: `levels`
    siblings of 8 words from the node's level up, then `levels` direction bits.  The packed row (csrc/merkle_rows.hpp): old node as words | new node as words
    | 64 zero bytes | the siblings as words | ceil(levels / 8) index bytes -- the tail starts at byte 128, as in MerkleUpdate's row.
    MerkleTree.update_segments / update_record_segments / insert_key_segments give every segment's rows and the published nodes for a device tree.
    Sizes (MERKLE_SEGMENT_SIZES): exactly MerkleUpdate's, 56 993 levels + 1 026 wires and 101 473 levels + 1 540 rows; levels = 10 is the most that fits
    Params(d=1 << 20, m=699050), levels = 1 fits Params(d=1 << 17, m=87381)."""

    def __init__(self, levels: int):
        self.levels = self.depth = self._arg(levels, 1, None, "levels is at least 1")
        self.w = w = Words()
        self.old_node = w.public(8)
        self.new_node = w.public(8)
        self._tail_wires()
        self.out_old = _merkle_levels(w, self.old_node, self.siblings, self.dirs)
        self.out_new = _merkle_levels(w, self.new_node, self.siblings, self.dirs)
        self.old_top = [w.output(x) for x in self.out_old]
        self.new_top = [w.output(x) for x in self.out_new]

    @property
    def lu(self) -> int:
        return 1024

    def bits(self, old_node: bytes, new_node: bytes, siblings, index: int):
        """one statement's input bits, public then private: the old node, the new node, 512 zeros where the two tops are computed, the siblings from the node's
        level up, then the direction bits = the bits of the node's index inside the segment's subtree, least significant first"""
        tail = _tail_bits("MerkleSegment", self.levels, siblings, index, (old_node, new_node), "two 32-byte nodes and ")
        return np.concatenate([tail[:512], np.zeros(512, dtype=np.uint8), tail[512:]])

    def tops_of(self, witness_row):
        """(old_top, new_top), 32 bytes each, as computed: from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return _digest_from_row(witness_row, 512), _digest_from_row(witness_row, 768)

    @staticmethod
    def statement(old_node: bytes, new_node: bytes, old_top: bytes, new_top: bytes) -> bytes:
        """the 128 statement bytes (what verify_public takes, bits [0, 1024) of a witness row) that say "old_node -> new_node takes old_top to new_top": each
        quarter MerklePath.statement's bytes"""
        return b"".join(_statement_of(x, f"MerkleSegment: {what}") for x, what in ((old_node, "the old node"), (new_node, "the new node"),
                                                                                  (old_top, "the old top"), (new_top, "the new top")))

    @classmethod
    def chain(cls, nodes):
        """the G upper statements of one transition from its published list [(X_0, X_0'), .., (X_G, X_G')], (X_G, X_G') = (R, R'): statement g - 1 of the result
        is segment g's, statement(X_g-1, X_g-1', X_g, X_g').  Segment 0's statement is its own class's, over (X_0, X_0')."""
        nodes = [(bytes(a), bytes(b)) for a, b in nodes]
        if len(nodes) < 2:
            raise CircuitError("MerkleSegment: a chain is at least two node pairs")
        return [cls.statement(*nodes[g - 1], *nodes[g]) for g in range(1, len(nodes))]


def segment_levels(depth: int, cuts):
    """[(0, c_0), (c_0, c_1), .., (c_G-1, depth)]: the level ranges of a path of `depth` levels cut at `cuts`; CircuitError unless 1 <= c_0 < .. < c_G-1 < depth"""
    cuts = list(cuts)
    if (not isinstance(depth, (int, np.integer)) or not cuts or not all(isinstance(c, (int, np.integer)) for c in cuts) or cuts[0] < 1 or cuts[-1] >= depth
            or any(a >= b for a, b in zip(cuts, cuts[1:]))):
        raise CircuitError("segment_levels: cuts are 1 <= c_0 < .. < c_G-1 < depth, at least one")
    edges = [0] + [int(c) for c in cuts] + [int(depth)]
    return list(zip(edges, edges[1:]))


class MerkleClimb(_Statement):
    """The statement "the node X lies `levels` levels below the node Y": MerklePath's body with the leaf made PUBLIC -- one level range of a READ path that is
    too deep for one circuit (segment_levels cuts it), at half of MerkleSegment's cost a level.

    A deep read -- "this leaf / record is in the tree with root R", "this key is not in the table under R" -- is proved per level range.  With cuts c_0 < ..
    < c_G-1 segment 0 is an existing statement (MerklePath(c_0), MerkleRecord(length, c_0), MerkleAbsent(key_bytes, length, c_0)) over the subtree of height
    c_0 that holds the leaf, its computed "root" X_0 the level-c_0 node on the path, and segment g >= 1 is MerkleClimb(c_g - c_g-1) (c_G = the depth).  The
    prover publishes the nodes X_0 .. X_G, X_G = R; the verifier builds every upper statement's bytes from that ONE list (chain), so adjacent statements share
    a node by construction, and checks one proof a segment.
    Soundness is MerklePath's applied G + 1 times: each proof says its lower node hashes up to its top through SOME siblings and directions, and the shared
    nodes tie the tops to the next segment's lower node, so the leaf's subtree top X_0 lies depth - c_0 levels below R.  A segment's private index bits need
    not agree with its neighbours'.
    WHAT BECOMES PUBLIC: the intermediate nodes X_g, g < G.  They are hashes; to someone who holds the tree they reveal which level-c_g subtree the leaf lies
    in, that is the high bits of the index.  That matters for MerklePath and MerkleRecord, which hide the leaf; for MerkleAbsent the key is public already.
    Public wires, in this order (public wires are laid out in declaration order, so the given ones come first): X as 8 given words at statement bits [0, 256),
    Y as 256 computed outputs at [256, 512); lu = 512.  Private inputs: `levels` siblings of 8 words from X's level up, then `levels` direction bits; nin =
    512 + 257 levels.  The packed row (csrc/merkle_rows.hpp): X as words | 32 zero bytes | the siblings as words | ceil(levels / 8) index bytes -- the tail
    starts at byte 64, as in MerklePath's row.
    MerkleTree.path_segments / record_segments / absent_segments give every segment's rows and the published nodes for a device tree.
    Sizes (MERKLE_CLIMB_SIZES): exactly MerklePath's, 28 625 levels + 514 wires and 50 865 levels + 772 rows; levels = 20 is the most that fits
    Params(d=1 << 20, m=699050), levels = 10 fits d = 2^19 and levels = 2 is the most that fits Params(d=1 << 17, m=87381)."""

    def __init__(self, levels: int):
        self.levels = self.depth = self._arg(levels, 1, None, "levels is at least 1")
        self.w = w = Words()
        self.node = w.public(8)
        self._tail_wires()
        self.out = _merkle_levels(w, self.node, self.siblings, self.dirs)
        self.top = [w.output(x) for x in self.out]

    @property
    def lu(self) -> int:
        return 512

    def bits(self, node: bytes, siblings, index: int):
        """one statement's input bits, public then private: the node, 256 zeros where the top is computed, the siblings from the node's level up, then the
        direction bits = the bits of the node's index inside the segment's subtree, least significant first"""
        tail = _tail_bits("MerkleClimb", self.levels, siblings, index, (node,), "a 32-byte node and ")
        return np.concatenate([tail[:256], np.zeros(256, dtype=np.uint8), tail[256:]])

    def top_of(self, witness_row) -> bytes:
        """the 32 bytes of the computed top: from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return _digest_from_row(witness_row, 256)

    @staticmethod
    def statement(node: bytes, top: bytes) -> bytes:
        """the 64 statement bytes (what verify_public takes, bits [0, 512) of a witness row) that say "node lies below top": each half
        MerklePath.statement's bytes"""
        return _statement_of(node, "MerkleClimb: the node") + _statement_of(top, "MerkleClimb: the top")

    @classmethod
    def chain(cls, nodes):
        """the G upper statements of one read from its published list [X_0, .., X_G], X_G = R: statement g - 1 of the result is segment g's,
        statement(X_g-1, X_g).  Segment 0's statement is its own class's, over X_0."""
        nodes = [bytes(x) for x in nodes]
        if len(nodes) < 2:
            raise CircuitError("MerkleClimb: a chain is at least two nodes")
        if any(len(x) != 32 for x in nodes):
            raise CircuitError("MerkleClimb: a node of a chain is 32 bytes")
        return [cls.statement(nodes[g - 1], nodes[g]) for g in range(1, len(nodes))]


class MerkleRecordUpdate(_TwoRoots):
    """The statement "I know an old record and a new record of `length` bytes, `depth` siblings and an index such that the path from SHA-256(old record)
    gives old_root and the SAME siblings and directions from SHA-256(new record) give new_root": MerkleUpdate about the data behind the leaf.

    Private inputs, in this order: the 8 * length bits of the old record, byte k's bit b (LSB first) at 8 k + b, as MerkleRecord; the 8 * length bits of
    the new record; `depth` siblings of 8 words from the leaf's level up; `depth` direction bits (bit l of the index).  The body is Sha256Message's block
    chain (_message_chain) once per record and MerklePath's levels (_merkle_levels) twice over the shared sibling and direction wires, as MerkleUpdate
    shares them.  Public outputs (lu = 512): the old root at statement bits [0, 256), the new root at [256, 512), both computed; statement(R, R') is
    MerkleUpdate.statement's 64 bytes.
    frozen=(lo, hi), 0 <= lo <= hi <= length: bytes [lo, hi) of the new record equal the old record's (assert_same on the 8 (hi - lo) bit pairs: that
    many rows, no wire) -- "the key did not change, only the value did".  It is part of the circuit, and therefore of the CRS.
    MerkleTree.update_records / update_record_bits give the input rows of a batch of sequential record updates of a device table and its tree.
    Sizes (MERKLE_RECORD_UPDATE_SIZES): those of MerkleUpdate(depth) plus twice Sha256Message(length)'s, less 1 028 wires and 1 544 rows (the 512 leaf
    inputs and their bit rows, the chains' outputs and constants counted once); nwires - len(program) = 512 + 16 length + 257 depth inputs.  (55, 1)
    fits Params(d=1 << 18, m=174762).  At Params(d=1 << 20, m=699050) one-block records (up to 55 bytes) reach depth 9 (569 019 wires, 1 012 285
    rows; depth 10 would be 1 113 758 rows) and two-block records (up to 119 bytes) depth 8."""

    def __init__(self, length: int, depth: int, frozen=None):
        self.length, self.depth = length, depth = self._length_arg(length), self._depth_arg(depth)
        if frozen is not None:
            lo, hi = frozen
            if not all(isinstance(x, (int, np.integer)) for x in (lo, hi)) or not 0 <= lo <= hi <= length:
                raise CircuitError("MerkleRecordUpdate: frozen is (lo, hi) with 0 <= lo <= hi <= length")
            frozen = (int(lo), int(hi))
        self.frozen = frozen
        self.w = w = Words()
        self.old_record = w.c.private(8 * length)
        self.new_record = w.c.private(8 * length)
        self._tail_wires()
        self.old_leaf, self.blocks = _message_chain(w, self.old_record, length)
        self.new_leaf, _ = _message_chain(w, self.new_record, length)
        self._root_outputs(self.old_leaf, self.new_leaf)
        if frozen:
            for a, b in zip(self.old_record[8 * frozen[0]: 8 * frozen[1]], self.new_record[8 * frozen[0]: 8 * frozen[1]]):
                w.c.assert_same(a, b)

    def bits(self, old_record: bytes, new_record: bytes, siblings, index: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed, the old record's bits, the new record's, the
        siblings from the leaf's level up, then the direction bits = the bits of the leaf's index, least significant first.  (A new record that breaks
        `frozen` is not refused here: Circuit.holds / circuit_assign say so.)"""
        who = "MerkleRecordUpdate"
        return _input_bits(512, _record_bits(who, self.length, old_record, new_record, what="the records are"), _tail_bits(who, self.depth, siblings, index))


def _key_bits_lsb_first(bits, key_bytes: int):
    """the 8 * key_bytes wires of a key (byte k's bit b at 8 k + b) as an unsigned big-endian integer, least significant wire first: byte 0 is the most
    significant byte, and bit 7 of a byte stands above its bit 0"""
    return [bits[8 * k + b] for k in range(key_bytes - 1, -1, -1) for b in range(8)]


def _is_sentinel(key: bytes) -> bool:
    return key == bytes(len(key)) or key == b"\xff" * len(key)


def _checked_key(who: str, key_bytes: int, key, never: str) -> bytes:
    """the key as bytes; refused when it is not key_bytes bytes or a sentinel, which is `never` ("queries", "members") what the statement takes"""
    key = bytes(key)
    if len(key) != key_bytes:
        raise CircuitError(f"{who}: the key is {key_bytes} bytes")
    if _is_sentinel(key):
        raise CircuitError(f"{who}: the all-zero and the all-0xFF key are sentinels, never {never}")
    return key


class MerkleAbsent(_OneRoot):
    """The statement "the key q is NOT in the set behind this root", for a set kept as an indexed Merkle tree: I know a `length`-byte record (lo | hi |
    payload) and an authentication path of `depth` siblings, such that SHA-256(record) is a leaf of the tree with this root and lo < q < hi.

    The data model.  A key is key_bytes bytes, 1 <= key_bytes <= 32, compared as a big-endian unsigned integer (memcmp order); the all-zero and the
    all-0xFF key are sentinels, never members and never queries.  A record is length >= 2 key_bytes bytes: its own key lo at [0, K), the next larger key
    of the set hi at [K, 2K), an opaque payload behind them.  A well-formed table of 2^depth records holds, in any positions, the sentinel record
    (0...0, k_1), one record (k_i, k_i+1) per member, the last with hi = FF...FF, and in every other slot lo >= hi: the open ranges (lo, hi) of the live
    records then partition the keys that are neither members nor sentinels, so exactly one record shows a key absent and none does for a member.
    SOUNDNESS IS RELATIVE TO THAT INVARIANT: whoever accepts a root accepts that the table behind it is well formed; the circuit proves membership of
    ONE record with lo < q < hi and nothing about the other records (indexed_records makes such a table, indexed_insert the two updates of an insert).
    Public wires, in this order: the root as 256 computed outputs (statement bits [0, 256), as MerkleRecord), then the 8 key_bytes given bits of q,
    byte k's bit b (LSB first) at 256 + 8 k + b; lu = 256 + 8 key_bytes.  Private inputs, in MerkleRecord's order: the 8 * length record bits, `depth`
    siblings of 8 words, `depth` direction bits.  The body is MerkleRecord's (_message_chain, _merkle_levels) and two comparators (Words.less_than)
    asserted to 1.  MerkleTree.absent_rows / absent_bits find the record and give the input rows for queries against a device table.
    Sizes (MERKLE_ABSENT_SIZES): those of MerkleRecord(length, depth) plus 40 key_bytes wires and 72 key_bytes + 2 rows -- the 8 key_bytes public wires of
    q and their bit rows, and per comparison 16 key_bytes wires (a NOT and a MAJ a bit), 32 key_bytes rows and the assertion's row.  It keeps
    MerkleRecord's depth range: (8, 55, 19) fits Params(d=1 << 20, m=699050).  A deeper table is read with the path cut (segment_levels):
    MerkleAbsent(key_bytes, length, c_0) over the record's subtree, MerkleClimb above it (MerkleTree.absent_segments)."""

    def __init__(self, key_bytes: int, length: int, depth: int):
        self.key_bytes = K = self._arg(key_bytes, 1, 32, "key_bytes is in [1, 32]")
        self.length = length = self._arg(length, 2 * K, None, "the length is at least 2 key_bytes bytes")
        self.depth = self._depth_arg(depth)
        self.w = w = Words()
        self.record = w.c.private(8 * length)
        self._tail_wires()
        self.leaf, self.blocks = _message_chain(w, self.record, length)
        self.out = cur = _merkle_levels(w, self.leaf, self.siblings, self.dirs)
        self.root = [w.output(x) for x in cur]
        self.key = w.c.public(8 * K)
        lo, hi, q = (_key_bits_lsb_first(bits, K) for bits in (self.record[: 8 * K], self.record[8 * K: 16 * K], self.key))
        w.c.assert_equal(w.less_than(lo, q), 1)
        w.c.assert_equal(w.less_than(q, hi), 1)

    @property
    def lu(self) -> int:
        return 256 + 8 * self.key_bytes

    def _query(self, key) -> bytes:
        return _checked_key("MerkleAbsent", self.key_bytes, key, "queries")

    def bits(self, key: bytes, record: bytes, siblings, index: int):
        """one statement's input bits, public then private: 256 zeros where the root is computed, the query's bits, the record's bits, the siblings from
        the leaf's level up, then the direction bits = the bits of the leaf's index, least significant first.  (A record whose range does not hold the
        key is not refused here: Circuit.holds / circuit_assign say so.)"""
        key = np.unpackbits(np.frombuffer(self._query(key), dtype=np.uint8), bitorder="little")
        return _input_bits(256, key, _record_bits("MerkleAbsent", self.length, record), _tail_bits("MerkleAbsent", self.depth, siblings, index))

    def statement(self, root: bytes, key: bytes) -> bytes:
        """the 32 + key_bytes statement bytes (what verify_public takes, bits [0, lu) of a witness row) that say "`key` is not in the set with root
        `root`": MerklePath.statement's bytes, then the key"""
        return _statement_of(root, "MerkleAbsent: the root") + self._query(key)


class MerkleLink(_OneRoot):
    """The statement "the set behind this root has a record whose first P = 2 key_bytes + reveal bytes are these", for a set kept as an indexed Merkle
    tree (MerkleAbsent has the data model).  Read as (k | k' | the first `reveal` payload bytes) it says: k and k' are ADJACENT in the set -- no member lies
    strictly between them -- and k's payload begins with these bytes.  With reveal = amount_bytes it publishes a MerkleTransfer balance.

    One statement gives the two reads that MerkleRecord (which hides the record) and MerkleAbsent cannot: "k IS a member, and its payload begins with v" is
    one link (k, successor); "the members inside [a, b] are exactly k_1 < .. < k_n" is the n + 1 links (p, k_1), (k_1, k_2), .., (k_n, s) with p < a and
    b < s, which `chain` checks in the clear -- completeness of a range scan, n + 1 proofs of ONE circuit under one CRS (Context.prove_batch_public).
    SOUNDNESS IS RELATIVE TO THE TABLE INVARIANT, as MerkleAbsent's: whoever accepts a root accepts that the table behind it is well formed; the circuit
    proves membership of ONE record with this prefix and nothing about the other records.  In a well-formed table a live record (k, k') exists exactly
    when k is a member or the lower sentinel and k' is the next larger member or the upper sentinel.
    The circuit is MerkleRecord's body unchanged (_message_chain, _merkle_levels); the first 8 P record bits are PUBLIC GIVEN wires instead of private ones,
    declared before the leaf and moved behind the root (Circuit.public_last).  No comparator and no equality row: the verifier checks k < k' in the clear
    (statement refuses anything else).
    Public wires: the root as 256 computed outputs at statement bits [0, 256), then the 8 P prefix bits, byte j's bit b (LSB first) at 256 + 8 j + b; lu =
    256 + 8 P.  Private inputs: the remaining 8 (length - P) record bits, `depth` siblings of 8 words, `depth` direction bits.  The input bits, and so the
    packed row, are MerkleRecord's: 32 zero bytes | record | siblings as words | index bytes.  MerkleTree.range_rows / range_segments find the records of a
    key range and give the rows for a device table.
    Sizes (MERKLE_LINK_SIZES): MerkleRecord(length, depth)'s, wire for wire and row for row -- a public input costs what a private one does -- and its depth
    range: (8, 55, 19) fits Params(d=1 << 20, m=699050), depth 20 needs a cut (MerkleClimb above MerkleLink(.., c_0), chain_cut)."""

    def __init__(self, key_bytes: int, length: int, depth: int, reveal=0):
        self.key_bytes = K = self._arg(key_bytes, 1, 32, "key_bytes is in [1, 32]")
        self.reveal = reveal = self._arg(reveal, 0, None, "reveal is a non-negative number of payload bytes")
        self.length = length = self._arg(length, 2 * K + reveal, None, "the length is at least 2 key_bytes + reveal bytes")
        self.depth = self._depth_arg(depth)
        self.shown_bytes = P = 2 * K + reveal
        self.w = w = Words()
        # the public prefix is read by the leaf's gates, so it is declared here and moved behind the root below
        self.shown = w.c.public(8 * P)
        self.hidden = w.c.private(8 * (length - P))
        self.record = list(self.shown) + list(self.hidden)
        self._tail_wires()
        self.leaf, self.blocks = _message_chain(w, self.record, length)
        self.out = cur = _merkle_levels(w, self.leaf, self.siblings, self.dirs)
        self.root = [w.output(x) for x in cur]
        w.c.public_last(self.shown)

    @property
    def lu(self) -> int:
        return 256 + 8 * self.shown_bytes

    def bits(self, record: bytes, siblings, index: int):
        """one statement's input bits, public then private: MerkleRecord.bits(record, siblings, index) unchanged -- 256 zeros where the root is computed, the
        record's bits (the first 8 P of them public), the siblings from the leaf's level up, then the direction bits"""
        return _input_bits(256, _record_bits("MerkleLink", self.length, record), _tail_bits("MerkleLink", self.depth, siblings, index))

    def shown_of(self, witness_row) -> bytes:
        """the P public prefix bytes, from a witness row (Circuit.assign's bytes or a row of Context.circuit_assign)"""
        return bytes(bytearray(witness_row)[32: 32 + self.shown_bytes])

    def _shown(self, shown) -> bytes:
        shown, K = bytes(shown), self.key_bytes
        if len(shown) != self.shown_bytes:
            raise CircuitError(f"MerkleLink: the shown prefix is 2 key_bytes + reveal = {self.shown_bytes} bytes")
        if shown[:K] >= shown[K: 2 * K]:
            raise CircuitError("MerkleLink: not a live record (lo < hi)")
        return shown

    def statement(self, root: bytes, shown: bytes) -> bytes:
        """the 32 + P statement bytes (what verify_public takes, bits [0, lu) of a witness row) that say "a record of the set with root `root` begins with
        `shown`" = (k | k' | reveal payload bytes): MerklePath.statement's bytes, then the prefix.  Refused unless k < k': an inert slot is no link."""
        return _statement_of(root, "MerkleLink: the root") + self._shown(shown)

    def _links(self, lo, hi, keys, shown):
        """the n + 1 prefixes of a range read, after the checks on which the claim "exactly these members" rests"""
        K = self.key_bytes
        lo, hi, keys = bytes(lo), bytes(hi), [bytes(k) for k in keys]
        if len(lo) != K or len(hi) != K or any(len(k) != K for k in keys):
            raise CircuitError(f"MerkleLink: the bounds and the keys are {K} bytes")
        if len(keys) < 2:
            raise CircuitError("MerkleLink: a chain is at least the two keys p and s around the range")
        if self.reveal:
            if shown is None or len(shown) != len(keys) - 1:
                raise CircuitError("MerkleLink: with reveal > 0 a chain takes one shown payload prefix per link: those of p, k_1, .., k_n")
            shown = [bytes(v) for v in shown]
            if any(len(v) != self.reveal for v in shown):
                raise CircuitError(f"MerkleLink: a shown payload prefix is reveal = {self.reveal} bytes")
        else:
            if shown is not None and len(shown):
                raise CircuitError("MerkleLink: with reveal = 0 a chain takes no shown bytes")
            shown = [b""] * (len(keys) - 1)
        p, members, s = keys[0], keys[1:-1], keys[-1]
        if not lo <= hi:
            raise CircuitError("MerkleLink: the range is lo <= hi")
        if not p < lo:
            raise CircuitError("MerkleLink: the first key is not below lo (p < lo)")
        if not hi < s:
            raise CircuitError("MerkleLink: the last key is not above hi (hi < s)")
        if members and not lo <= members[0]:
            raise CircuitError("MerkleLink: a member below lo (lo <= k_1)")
        if members and not members[-1] <= hi:
            raise CircuitError("MerkleLink: a member above hi (k_n <= hi)")
        if any(not a < b for a, b in zip(members, members[1:])):
            raise CircuitError("MerkleLink: the members are strictly ascending (k_1 < .. < k_n)")
        return [keys[i] + keys[i + 1] + shown[i] for i in range(len(keys) - 1)]

    def chain(self, root: bytes, lo: bytes, hi: bytes, keys, shown=None):
        """the verifier's side of a range read: the n + 1 statements statement(root, keys[i] | keys[i + 1] | shown[i]) of the claim "the members of the set
        inside [lo, hi] are exactly k_1 < .. < k_n", keys = [p, k_1, .., k_n, s] (n + 2 keys) and shown the n + 1 payload prefixes of `reveal` bytes of p,
        k_1, .., k_n (required exactly when reveal > 0).  CircuitError unless p < lo <= k_1 < .. < k_n <= hi < s; with n = 0 that is p < lo <= hi < s, the
        absence of a whole interval.
        THE CLAIM "EXACTLY THESE MEMBERS" RESTS ON THIS CHECK together with the n + 1 proofs: every link shares a key with the next, so the links tile
        (p, s) without a gap, and (p, s) covers [lo, hi].  A list that omits a member passes the check -- it is consistent on its face -- but then one of its
        links is not a record of the table, and no proof verifies against that statement."""
        return [self.statement(root, link) for link in self._links(lo, hi, keys, shown)]

    def chain_cut(self, nodes_0, lo: bytes, hi: bytes, keys, shown=None):
        """chain for a path cut at c_0 (this statement being MerkleLink(.., depth = c_0)): nodes_0 is one published level-c_0 node per link, statement i is
        statement(nodes_0[i], ..) over the subtree that holds link i's record.  The upper statements of link i come from MerkleClimb.chain(nodes[i]) over its
        whole published list (MerkleTree.range_segments' nodes)."""
        links = self._links(lo, hi, keys, shown)
        nodes_0 = [bytes(x) for x in nodes_0]
        if len(nodes_0) != len(links):
            raise CircuitError("MerkleLink: one level-c_0 node per link")
        return [self.statement(node, link) for node, link in zip(nodes_0, links)]


class _KeyStep(_TwoRoots):
    """Private base of MerkleInsert and MerkleRemove: a key step, the two record updates of slots p and s under ONE pair of roots, with the key as public
    wires behind the roots.  It holds what the two share -- the argument checks, the two tails' wires, the four level chains over (p, p, s, s), the wiring of
    their tops (joined or not), the key's wires, lu, statement, tops_of and the tail half of bits.  A subclass states its private records, how new_p is
    composed, its four leaves, its assert_same and comparator lines and the record arguments of bits: its __init__ is _open, its own records and leaves,
    _close, its own assertions -- in that order, which is the order of the wires and gates of the compiled program."""

    joined = True  # (on the class too: bits() reads the sizes and this alone, so it still serves a stand-in that has only the sizes)

    def _open(self, key_bytes, length, depth, nrec: int, field=0):
        """the argument checks, then the private wires in their order: nrec records of 8 * length bits (returned), `depth` siblings of p, `depth` siblings of
        s, the direction bits of p, those of s.  field: the bytes of a field the statement reads behind the two keys (MerkleTransfer's balance)"""
        self.key_bytes = K = self._arg(key_bytes, 1, 32, "key_bytes is in [1, 32]")
        self.length = length = self._arg(length, 2 * K + field, None, "the length is at least 2 key_bytes" + (f" + {field}" if field else "") + " bytes")
        self.depth = depth = self._depth_arg(depth)
        self.w = w = Words()
        records = [w.c.private(8 * length) for _ in range(nrec)]
        self.siblings_p = [w.private(8) for _ in range(depth)]
        self.siblings_s = [w.private(8) for _ in range(depth)]
        self.dirs_p = w.c.private(depth)
        self.dirs_s = w.c.private(depth)
        return records

    def _close(self, leaves, joined, pieces=None):
        """the level chains of the four leaves (old p, new p, old s, new s), the first two over p's tail and the last two over s's; the old root's outputs,
        with joined=False the two middle tops', the new root's; the key's public wires; joined: the 256 assert_same that tie the middle tops, the private
        intermediate root.  pieces: the statement's public pieces behind the tops where the key is not the only one (self._piece_bytes says their bytes) --
        lists of public wires that the subclass declared BEFORE its leaves, because its leaves depend on them; they are moved behind the tops here
        (Circuit.public_last), the key first"""
        w = self.w
        tails = ((self.siblings_p, self.dirs_p), (self.siblings_p, self.dirs_p), (self.siblings_s, self.dirs_s), (self.siblings_s, self.dirs_s))
        self.out_old, self.mid_p, self.mid_s, self.out_new = (_merkle_levels(w, leaf, sibs, dirs) for leaf, (sibs, dirs) in zip(leaves, tails))
        self.joined = bool(joined)
        self.old_root = [w.output(x) for x in self.out_old]
        if not self.joined:  # every chain top is public: X_p, X_p', X_s, X_s'
            self.top_mid_p = [w.output(x) for x in self.mid_p]
            self.top_mid_s = [w.output(x) for x in self.mid_s]
        self.new_root = [w.output(x) for x in self.out_new]
        if pieces is None:
            self.key = w.c.public(8 * self.key_bytes)
        else:
            self.key = pieces[0]
            w.c.public_last([x for piece in pieces for x in piece])
        if self.joined:
            for x, y in zip(self.mid_p, self.mid_s):
                w.assert_same_u32(x, y)

    def _piece_bytes(self):
        """the bytes of the public pieces behind the tops, in their order: the key's, then whatever else the step's statement names"""
        return (self.key_bytes,)

    @property
    def lu(self) -> int:
        return (512 if self.joined else 1024) + 8 * sum(self._piece_bytes())

    def _query(self, key) -> bytes:
        return _checked_key(type(self).__name__, self.key_bytes, key, "members")

    def _public(self, *pieces) -> bytes:
        """the checked bytes of the public pieces behind the tops, as the statement has them: one value per entry of _piece_bytes"""
        return self._query(*pieces)

    def _step_bits(self, pieces, records, siblings_p, index_p, siblings_s, index_s):
        """512 zeros where the two roots are computed (1024 with joined=False: the four tops), the bits of the public pieces (the key: one value, or a tuple
        of one value a piece), the records' bits, p's siblings and s's as big-endian words, then the direction bits of p and of s"""
        who = type(self).__name__
        key = np.unpackbits(np.frombuffer(self._public(*(pieces if isinstance(pieces, tuple) else (pieces,))), dtype=np.uint8), bitorder="little")
        tail_p, tail_s = (_tail_bits(who, self.depth, sibs, index) for sibs, index in ((siblings_p, index_p), (siblings_s, index_s)))
        nsib = 256 * self.depth
        return _input_bits(512 if self.joined else 1024, key, _record_bits(who, self.length, *records, what="the records are"), tail_p[:nsib], tail_s[:nsib],
                           tail_p[nsib:], tail_s[nsib:])

    def statement(self, *tops_and_key) -> bytes:
        """statement(old_root, new_root, key): the 64 + key_bytes statement bytes (what verify_public takes, bits [0, lu) of a witness row) that say "the step
        with `key` took old_root to new_root": MerkleUpdate.statement's bytes, then the key.  With joined=False statement(X_p, X_p', X_s, X_s', key), 128 +
        key_bytes bytes: "the step with `key` took p's top from X_p to X_p' and then s's top from X_s to X_s'"."""
        who = type(self).__name__
        npieces = len(self._piece_bytes())
        tops, pieces = tops_and_key[: -npieces], tops_and_key[-npieces:]
        if len(tops_and_key) != (2 if self.joined else 4) + npieces:
            what = "key" if npieces == 1 else f"the {npieces} public pieces"
            raise CircuitError(f"{who}: statement takes (old_root, new_root, {what}), or with joined=False (X_p, X_p', X_s, X_s', {what})")
        return b"".join(_statement_of(x, f"{who}: a top") for x in tops) + self._public(*pieces)

    def tops_of(self, witness_row):
        """joined=False: (X_p, X_p', X_s, X_s'), 32 bytes each, as computed, from a witness row"""
        if self.joined:
            raise CircuitError(f"{type(self).__name__}: tops_of is for joined=False (roots_of reads the two roots)")
        return tuple(_digest_from_row(witness_row, at) for at in (0, 256, 512, 768))


class MerkleInsert(_KeyStep):
    """The statement "the key k was inserted into the indexed table (MerkleAbsent has the data model), and that alone takes the tree from root R to root
    R'": the two record updates of an insert (indexed_insert) under ONE pair of roots.  Record p, whose range held k (lo_p < k < hi_p), gets hi <- k; the
    record (k, the old hi_p, a payload) goes into a slot s that was inert (lo_s >= hi_s).  A chain of such steps from the root of an indexed_records table
    keeps the invariant MerkleAbsent's soundness rests on, so a verifier who has seen every step's proof accepts absence proofs against the last root.

    Public wires, in this order: R as 256 computed outputs at statement bits [0, 256), R' at [256, 512), then the 8 key_bytes given bits of k, byte j's
    bit b (LSB first) at 512 + 8 j + b, as MerkleAbsent places q; lu = 512 + 8 key_bytes.  statement(R, R', k) is MerkleUpdate.statement's 64 bytes, then k.
    Private inputs, in this order: the old record of slot p (8 * length bits, byte j's bit b at 8 j + b), the old record of slot s, the new record of slot
    s; `depth` siblings of 8 words for p, from the leaf's level up; `depth` siblings for s, taken from the tree AFTER p's update; `depth` direction bits
    of p; `depth` direction bits of s.
    The body.  The new record of p is no input: it is old_p's wires with those of bytes [K, 2K) replaced by new_s's bytes [0, K), so lo and payload of p
    cannot change.  Four record chains (_message_chain: old_p, new_p, old_s, new_s) and four level chains (_merkle_levels: old_p and new_p over p's siblings
    and directions, old_s and new_s over s's).  R is the root of the first chain, R' that of the last; the two middle roots -- the private intermediate
    root, the tree after p's update -- are tied by 256 assert_same.  Further assert_same: k = new_s[0, K); old_p[K, 2K) = new_s[K, 2K) (the new record
    inherits the old hi).  Comparators (Words.less_than): lo_p < k and k < hi_p asserted to 1, lo_s < hi_s asserted to 0 (the slot was inert).
    p != s needs no constraint of its own: the siblings of s open the tree AFTER p's update, in which slot p holds the live record (lo_p, k), lo_p < k,
    so with s = p the record old_s would have to be that live record and could not pass the inert check.
    What it does not cover: the payload of the new record is free (bytes [2K, length) of new_s are unconstrained; constrain them in a wrapping circuit if
    they matter), and, like MerkleAbsent, it says nothing about the records it does not open.
    MerkleTree.insert_keys / insert_bits perform a batch of inserts on a device table and give the input rows; statement j is (R_j, R_j+1, key_j).
    Sizes (MERKLE_INSERT_SIZES): four level chains cost about 203 000 rows a level, so (8, 55, 4) is the deepest one-block statement that fits
    Params(d=1 << 20, m=699050); depth 5 (about 1 212 000 rows) does not.  Depth 1 fits Params(d=1 << 19, m=349525).
    joined=False is segment 0 of an insert into a deeper tree (MerkleSegment): the 256 assert_same on the middle roots are dropped and all four chain tops are
    outputs, so p and s may lie in different height-`depth` subtrees.  Public wires then: X_p at [0, 256), X_p' at [256, 512), X_s at [512, 768), X_s' at
    [768, 1024), the key's bits from 1024; lu = 1024 + 8 key_bytes; statement(X_p, X_p', X_s, X_s', key); tops_of(row) reads the four back; the packed row is
    the joined one with 128 zero bytes in front in place of 64.  X_s is opened in the tree after p's update, so the p != s argument above still holds; the upper
    chain of s starts from the root after p's update, which thereby becomes public.  Sizes (MERKLE_INSERT_SPLIT_SIZES): the joined ones plus 512 wires and 768
    rows; (8, 55, 4) still fits Params(d=1 << 20, m=699050)."""

    def __init__(self, key_bytes: int, length: int, depth: int, joined=True):
        self.old_p, self.old_s, self.new_s = self._open(key_bytes, length, depth, 3)
        w, K = self.w, self.key_bytes
        self.new_p = self.old_p[: 8 * K] + self.new_s[: 8 * K] + self.old_p[16 * K:]
        chains = [_message_chain(w, rec, self.length) for rec in (self.old_p, self.new_p, self.old_s, self.new_s)]
        self.blocks = chains[0][1]
        self._close([leaf for leaf, _ in chains], joined)
        for a, b in zip(self.key, self.new_s[: 8 * K]):
            w.c.assert_same(a, b)
        for a, b in zip(self.old_p[8 * K: 16 * K], self.new_s[8 * K: 16 * K]):
            w.c.assert_same(a, b)
        lo_p, hi_p, lo_s, hi_s, k = (_key_bits_lsb_first(bits, K) for bits in (self.old_p[: 8 * K], self.old_p[8 * K: 16 * K], self.old_s[: 8 * K],
                                                                              self.old_s[8 * K: 16 * K], self.key))
        w.c.assert_equal(w.less_than(lo_p, k), 1)
        w.c.assert_equal(w.less_than(k, hi_p), 1)
        w.c.assert_equal(w.less_than(lo_s, hi_s), 0)

    def bits(self, key: bytes, old_p: bytes, old_s: bytes, new_s: bytes, siblings_p, index_p: int, siblings_s, index_s: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed (1024 with joined=False: the four tops), the key's bits,
        the three records' bits, p's siblings and s's (those from the tree after p's update) as big-endian words, then the direction bits of p and of s.  (A
        witness that breaks a constraint is not refused here: Circuit.holds / circuit_assign say so.)"""
        return self._step_bits(key, (old_p, old_s, new_s), siblings_p, index_p, siblings_s, index_s)


class MerkleRemove(_KeyStep):
    """The statement "the key k was removed from the indexed table (MerkleAbsent has the data model), and that alone takes the tree from root R to root
    R'": the two record updates of a removal (indexed_remove) under ONE pair of roots.  Record s is the one whose own key is k (lo_s = k): it becomes the
    all-zero record, which is inert and is what indexed_records leaves in unused slots.  Record p is the live record whose hi is k: it gets hi <- hi_s, its
    lo and payload kept.  The inverse of MerkleInsert's step: a chain of inserts and removes from the root of an indexed_records table keeps the invariant
    MerkleAbsent's soundness rests on.

    Public wires, in this order: R as 256 computed outputs at statement bits [0, 256), R' at [256, 512), then the 8 key_bytes given bits of k, byte j's
    bit b (LSB first) at 512 + 8 j + b, as MerkleInsert places it; lu = 512 + 8 key_bytes.  statement(R, R', k) is MerkleUpdate.statement's 64 bytes, then k.
    Private inputs, in this order: the old record of slot p (8 * length bits, byte j's bit b at 8 j + b), the old record of slot s; `depth` siblings of 8
    words for p, from the leaf's level up; `depth` siblings for s, taken from the tree AFTER p's update; `depth` direction bits of p; `depth` direction
    bits of s.  nin = 512 + 8 key_bytes + 16 length + 514 depth.
    The body.  Neither new record is an input: new_p is old_p's wires with those of bytes [K, 2K) replaced by old_s's bytes [K, 2K), so lo and payload of p
    cannot change, and the new leaf of s is the CONSTANT digest SHA-256(bytes(length)) as eight Words.const words.  Three record chains (_message_chain:
    old_p, new_p, old_s; MerkleInsert has four) and four level chains (_merkle_levels: old_p and new_p over p's siblings and directions, old_s and the
    constant leaf over s's).  R is the root of the first chain, R' that of the last; the two middle roots -- the private intermediate root, the tree after
    p's update -- are tied by 256 assert_same.  Further assert_same: k = old_p[K, 2K) and k = old_s[0, K).  Comparators (Words.less_than): lo_p < k and
    k < hi_s asserted to 1.
    Soundness.  p and s are records under R (s under the root after p's update, which differs from R in slot p alone).  After the step p's range is
    (lo_p, hi_s) with lo_p < k < hi_s and s is inert: the live ranges partition the keys again, and k is the lo of none of them.  p != s needs no
    constraint of its own: the siblings of s open the tree AFTER p's update, in which slot p holds a record with lo = lo_p < k, so it cannot be a record
    with lo = k.
    What it does not cover: the removed record's payload is discarded unseen, and, like MerkleInsert, it says nothing about the records it does not open.
    MerkleTree.remove_keys / remove_bits perform a batch of removes on a device table and give the input rows; statement j is (R_j, R_j+1, key_j).
    Sizes (MERKLE_REMOVE_SIZES): a level costs what MerkleInsert's does, so (8, 55, 4) is the deepest one-block statement that fits Params(d=1 << 20,
    m=699050); depth 5 does not.  Depth 1 fits Params(d=1 << 19, m=349525).
    joined=False is segment 0 of a removal from a deeper tree (MerkleSegment), exactly as MerkleInsert's: the 256 assert_same on the middle roots are
    dropped and all four chain tops are outputs, so p and s may lie in different height-`depth` subtrees.  Public wires then: X_p at [0, 256), X_p' at
    [256, 512), X_s at [512, 768), X_s' at [768, 1024), the key's bits from 1024; lu = 1024 + 8 key_bytes; statement(X_p, X_p', X_s, X_s', key);
    tops_of(row) reads the four back; the packed row is the joined one with 128 zero bytes in front in place of 64 (MERKLE_REMOVE_SPLIT_SIZES)."""

    def __init__(self, key_bytes: int, length: int, depth: int, joined=True):
        self.old_p, self.old_s = self._open(key_bytes, length, depth, 2)
        w, K = self.w, self.key_bytes
        self.new_p = self.old_p[: 8 * K] + self.old_s[8 * K: 16 * K] + self.old_p[16 * K:]
        chains = [_message_chain(w, rec, self.length) for rec in (self.old_p, self.new_p, self.old_s)]
        self.blocks = chains[0][1]
        self.inert_leaf = [w.const(v) for v in be_words(hashlib.sha256(bytes(self.length)).digest())]  # the all-zero record's leaf
        self._close([leaf for leaf, _ in chains] + [self.inert_leaf], joined)
        for a, b in zip(self.key, self.old_p[8 * K: 16 * K]):
            w.c.assert_same(a, b)
        for a, b in zip(self.key, self.old_s[: 8 * K]):
            w.c.assert_same(a, b)
        lo_p, hi_s, k = (_key_bits_lsb_first(bits, K) for bits in (self.old_p[: 8 * K], self.old_s[8 * K: 16 * K], self.key))
        w.c.assert_equal(w.less_than(lo_p, k), 1)
        w.c.assert_equal(w.less_than(k, hi_s), 1)

    def bits(self, key: bytes, old_p: bytes, old_s: bytes, siblings_p, index_p: int, siblings_s, index_s: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed (1024 with joined=False: the four tops), the key's bits,
        the two records' bits, p's siblings and s's (those from the tree after p's update) as big-endian words, then the direction bits of p and of s.  (A
        witness that breaks a constraint is not refused here: Circuit.holds / circuit_assign say so.)"""
        return self._step_bits(key, (old_p, old_s), siblings_p, index_p, siblings_s, index_s)


class MerkleTransfer(_KeyStep):
    """The statement "the amount v moved from the account with key k_from to the account with key k_to, and that alone takes the tree from root R to root
    R'": the two record updates of a transfer (indexed_transfer) under ONE pair of roots -- the first statement over the indexed table (MerkleAbsent has
    the data model) that does arithmetic on the payload.

    The data model.  amount_bytes = A, 1 <= A <= 8.  A record's BALANCE is its bytes [2K, 2K + A), an unsigned big-endian integer, so length >= 2K + A;
    a transfer touches nothing else of a record (lo, hi and the payload bytes from 2K + A on).  Record p is the live record whose own key is k_from: its
    balance becomes b_p - v.  Record s is the live record whose own key is k_to, opened in the tree AFTER p's update: its balance becomes b_s + v.
    Public wires, in this order: R as 256 computed outputs at statement bits [0, 256), R' at [256, 512), the 8K given bits of k_from, the 8K of k_to, the 8A
    of v -- v as A big-endian bytes, byte j's bit b (LSB first) at 8 j + b, as the keys are placed; lu = 512 + 16K + 8A.  statement(R, R', k_from, k_to, v)
    is MerkleUpdate.statement's 64 bytes, then the two keys, then v as A bytes.
    Private inputs, in this order: the old record of p (8 * length bits, byte j's bit b at 8 j + b), the old record of s; `depth` siblings of 8 words for p,
    from the leaf's level up; `depth` siblings for s, taken from the tree AFTER p's update; `depth` direction bits of p; `depth` direction bits of s.
    nin = 512 + 16K + 8A + 16 length + 514 depth.
    The body.  Neither new record is an input: new_p is old_p's wires with the 8A balance wires replaced by the difference b_p - v, new_s is old_s's wires
    with them replaced by the sum b_s + v (Words.ripple, a full adder a bit), so keys and the rest of the payload cannot change.  The final BORROW of the
    subtraction is asserted 0 (no overdraft) and the final CARRY of the addition is asserted 0 (no overflow past 2^(8A) - 1).  Four record chains
    (_message_chain: old_p, new_p, old_s, new_s) and four level chains (_merkle_levels) as MerkleInsert's; the two middle roots tied by 256 assert_same.
    Further assert_same: k_from = old_p[0, K), k_to = old_s[0, K).  Comparators: less_than(lo_p, hi_p) = 1 and less_than(lo_s, hi_s) = 1 -- both records
    are live.  The sentinel keys are refused as for members.
    Soundness.  A transfer CONSERVES b_p + b_s: with no borrow and no carry the two new balances are the integers b_p - v and b_s + v.  It keeps the
    table's invariant, because no key changes: every record's lo and hi are the wires they were.  By the invariant a key is the lo of at most one live
    record, so p and s are the accounts of k_from and k_to and no others.
    k_from = k_to.  The statement needs no constraint against it.  With k_from = k_to the invariant makes s the slot p, and s is opened in the tree after
    p's update, so old_s is new_p, balance b_p - v; the step then leaves the slot at (b_p - v) + v = b_p: R' = R and the sum of all balances is what it
    was.  A transfer to oneself is a no-op that still demands v <= b_p, nothing is created -- so the circuit allows it, and MerkleTree.transfer_keys,
    which has nothing to do for it, refuses it.
    What it does not cover: like MerkleInsert, the records it does not open.
    MerkleTree.transfer_keys / transfer_bits perform a batch of transfers on a device table and give the input rows; statement j is (R_j, R_j+1,
    from_j, to_j, v_j).  An account may occur in many steps of a batch, and may spend what an earlier step delivered.
    Sizes (MERKLE_TRANSFER_SIZES): MerkleInsert's four chains and four level chains, so a level costs 113 986 wires and 202 946 rows; (8, 55, 4, 8) fits
    Params(d=1 << 20, m=699050), depth 5 does not; (4, 16, 1, 8) fits Params(d=1 << 19, m=349525).
    joined=False is segment 0 of a cut transfer (MerkleSegment), exactly as MerkleInsert's: the 256 assert_same on the middle roots are dropped and all four
    chain tops are outputs, X_p at [0, 256), X_p' at [256, 512), X_s at [512, 768), X_s' at [768, 1024); the keys and the amount follow from bit 1024;
    lu = 1024 + 16K + 8A; statement(X_p, X_p', X_s, X_s', k_from, k_to, v); tops_of(row) reads the four back; the packed row is the joined one with 128
    zero bytes in front in place of 64 (MERKLE_TRANSFER_SPLIT_SIZES)."""

    amount_bytes = 8

    def __init__(self, key_bytes: int, length: int, depth: int, amount_bytes=8, joined=True):
        self.amount_bytes = A = self._arg(amount_bytes, 1, 8, "amount_bytes is in [1, 8]")
        self.old_p, self.old_s = self._open(key_bytes, length, depth, 2, field=A)
        w, K = self.w, self.key_bytes
        # the public pieces are read by the two balances' gates, so they are declared here; _close moves them behind the tops
        self.key, self.key_to, self.amount = w.c.public(8 * K), w.c.public(8 * K), w.c.public(8 * A)
        field = slice(16 * K, 16 * K + 8 * A)
        v, b_p, b_s = (_key_bits_lsb_first(bits, A) for bits in (self.amount, self.old_p[field], self.old_s[field]))
        diff, self.borrow = w.ripple(b_p, v, subtract=True)
        total, self.carry = w.ripple(b_s, v)

        def with_balance(record, bits):  # `bits` least significant first, back into the record's byte order
            return record[: field.start] + [bits[8 * (A - 1 - j) + b] for j in range(A) for b in range(8)] + record[field.stop:]

        self.new_p, self.new_s = with_balance(self.old_p, diff), with_balance(self.old_s, total)
        chains = [_message_chain(w, rec, self.length) for rec in (self.old_p, self.new_p, self.old_s, self.new_s)]
        self.blocks = chains[0][1]
        self._close([leaf for leaf, _ in chains], joined, pieces=(self.key, self.key_to, self.amount))
        w.c.assert_equal(self.borrow, 0)
        w.c.assert_equal(self.carry, 0)
        for a, b in zip(self.key, self.old_p[: 8 * K]):
            w.c.assert_same(a, b)
        for a, b in zip(self.key_to, self.old_s[: 8 * K]):
            w.c.assert_same(a, b)
        lo_p, hi_p, lo_s, hi_s = (_key_bits_lsb_first(bits, K) for bits in (self.old_p[: 8 * K], self.old_p[8 * K: 16 * K], self.old_s[: 8 * K],
                                                                           self.old_s[8 * K: 16 * K]))
        w.c.assert_equal(w.less_than(lo_p, hi_p), 1)
        w.c.assert_equal(w.less_than(lo_s, hi_s), 1)

    def _piece_bytes(self):
        return (self.key_bytes, self.key_bytes, self.amount_bytes)

    def _public(self, *pieces) -> bytes:
        if len(pieces) != 3:
            raise CircuitError("MerkleTransfer: the public pieces are (k_from, k_to, v)")
        k_from, k_to, v = pieces
        if not isinstance(v, (int, np.integer)) or not 0 <= v < 1 << (8 * self.amount_bytes):
            raise CircuitError(f"MerkleTransfer: the amount is an integer in [0, 2^{8 * self.amount_bytes})")
        return self._query(k_from) + self._query(k_to) + int(v).to_bytes(self.amount_bytes, "big")

    def bits(self, k_from: bytes, k_to: bytes, amount: int, old_p: bytes, old_s: bytes, siblings_p, index_p: int, siblings_s, index_s: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed (1024 with joined=False: the four tops), the bits of
        k_from, of k_to and of the amount's A big-endian bytes, the two records' bits, p's siblings and s's (those from the tree after p's update) as
        big-endian words, then the direction bits of p and of s.  (A witness that breaks a constraint is not refused here: Circuit.holds / circuit_assign
        say so.)"""
        return self._step_bits((k_from, k_to, amount), (old_p, old_s), siblings_p, index_p, siblings_s, index_s)


class _RecordStep(_TwoRoots):
    """Private base of MerkleAdjust and MerkleWrite: ONE record update by key under a pair of roots, the new record the old one's wires with one field
    replaced, the key and the step's other public pieces (self.public; _public) behind the roots.  A subclass's __init__ is _open, its further public pieces
    and its new record, _close, then its own assertions with _assert_key and _assert_live among them in ITS order: that of the compiled program's."""

    def _open(self, key_bytes, length, depth, least: int):
        """the checks of key_bytes, length (the two keys and `least` bytes) and depth; the private wires (the old record, _tail_wires); the key's public wires.
        The public pieces are read by the new record's gates: the subclass declares its others next, and _close moves them all behind the roots"""
        self.key_bytes = K = self._arg(key_bytes, 1, 32, "key_bytes is in [1, 32]")
        self.length = self._arg(length, 2 * K + least, None, f"the length is at least 2 key_bytes + {least} bytes")
        self.depth = self._depth_arg(depth)
        self.w = w = Words()
        self.old_record = w.c.private(8 * self.length)
        self._tail_wires()
        self.key = w.c.public(8 * K)
        return w

    def _close(self, new_record, *pieces):
        """the two record chains, MerkleUpdate's two level chains over the shared tail and the roots' outputs; the key and then `pieces` go behind the roots"""
        self.new_record = new_record
        self.old_leaf, self.blocks = _message_chain(self.w, self.old_record, self.length)
        self.new_leaf, _ = _message_chain(self.w, self.new_record, self.length)
        self._root_outputs(self.old_leaf, self.new_leaf)
        self.public = [x for piece in (self.key,) + pieces for x in piece]
        self.w.c.public_last(self.public)

    def _assert_key(self):  # k = old[0, K)
        for x, y in zip(self.key, self.old_record[: 8 * self.key_bytes]):
            self.w.c.assert_same(x, y)

    def _assert_live(self):  # less_than(lo, hi) = 1: the record is live
        K = self.key_bytes
        lo, hi = (_key_bits_lsb_first(part, K) for part in (self.old_record[: 8 * K], self.old_record[8 * K: 16 * K]))
        self.w.c.assert_equal(self.w.less_than(lo, hi), 1)

    @property
    def lu(self) -> int:
        return 512 + len(self.public)

    def _step_bits(self, public: bytes, old_record, siblings, index):  # the bits of: 64 zero bytes | the checked public bytes | the old record | the tail
        who = type(self).__name__
        return _input_bits(512, np.unpackbits(np.frombuffer(public, dtype=np.uint8), bitorder="little"), _record_bits(who, self.length, old_record),
                           _tail_bits(who, self.depth, siblings, index))

    def statement(self, old_root: bytes, new_root: bytes, *pieces) -> bytes:
        """the lu / 8 statement bytes (what verify_public takes, bits [0, lu) of a witness row): MerkleUpdate.statement's, then the pieces' checked bytes"""
        return super().statement(old_root, new_root) + self._public(*pieces)


class MerkleAdjust(_RecordStep):
    """The statement "the balance of the account with key k went up by v (side 0, a deposit) or down by v (side 1, a withdrawal), and that alone takes the
    tree from root R to root R'": ONE record update of the indexed table with balances -- what funds and drains the ledger that MerkleTransfer moves
    value within.

    The data model is MerkleTransfer's.  amount_bytes = A, 1 <= A <= 8; the BALANCE of a record is its bytes [2K, 2K + A), an unsigned big-endian
    integer, so length >= 2K + A; an adjust touches nothing else of the record.
    Public wires, in this order: R as 256 computed outputs at statement bits [0, 256), R' at [256, 512), the 8K given bits of k, the 8A of v -- v as A
    big-endian bytes, byte j's bit b (LSB first) at 8 j + b, as MerkleTransfer places its amount -- and one byte `side`: its bit 0 is the direction, its
    bits 1 .. 7 are asserted 0.  lu = 512 + 8 (K + A + 1).  statement(R, R', k, v, side) is MerkleUpdate.statement's 64 bytes, then k, v as A bytes and
    the side byte.
    Private inputs, in this order: the old record (8 * length bits, byte j's bit b at 8 j + b); `depth` siblings of 8 words from the leaf's level up;
    `depth` direction bits -- _tail_wires, as MerkleRecordUpdate has them.  nin = 512 + 8 (K + A + 1) + 8 length + 257 depth.  The packed row: 64 zero
    bytes | k | v | side | old record | depth siblings as words | ceil(depth / 8) index bytes.
    The body.  The new record is not an input: it is the old record's wires with the 8A balance wires replaced by b + (v XOR side) + side -- ONE ripple of
    full adders whose carry in is the side wire and whose second operand is v_i XOR side (an XOR a bit): b + v for side 0, b + NOT v + 1 = b - v mod
    2^(8A) for side 1.  The carry out is tied to the side wire (assert_same).  Two record chains (_message_chain) and MerkleUpdate's two level chains over
    the shared tail (_root_outputs).  Further assert_same: k = old[0, K).  One comparator: less_than(lo, hi) = 1, the record is live.  The sentinel keys
    are refused as for members.
    Soundness.  Keys and the rest of the payload are the old record's wires, so every record's lo and hi are what they were: the table's invariant
    (MerkleAbsent) is kept.  By the invariant k is the lo of at most one live record, so the record opened is the account of k and no other.  With
    carry = side the new balance is the INTEGER b + v or b - v: a deposit's carry out must be 0, so b + v <= 2^(8A) - 1, no overflow; a withdrawal's
    carry out of b + (2^(8A) - 1 - v) + 1 must be 1, which is b >= v, no borrow, so no overdraft.  v = 0 is a no-op with R' = R in either direction
    (b + 0 carries 0; b + (2^(8A) - 1) + 1 = b + 2^(8A) carries 1).  The sum of all live balances therefore changes by exactly +v or -v.
    What it does not cover: like MerkleInsert, the records it does not open.
    MerkleTree.adjust_keys / adjust_bits perform a batch of adjusts on a device table and give the input rows; statement j is (R_j, R_j+1, k_j, v_j,
    side_j).  An account may occur in many steps of a batch, and a withdrawal may spend what an earlier deposit delivered.
    Sizes (MERKLE_ADJUST_SIZES): MerkleRecordUpdate(length, depth)'s two record chains and two level chains with one input record fewer; (8, 55, 9, 8)
    fits Params(d=1 << 20, m=699050), depth 10 does not; (4, 16, 1, 8) fits Params(d=1 << 18, m=174762).
    Cut form.  There is no `joined` parameter: the statement has one pair of tops, so segment 0 of a cut adjust (segment_levels) is MerkleAdjust(K,
    length, c_0, A) itself over the record's subtree of height c_0, and the upper ranges are MerkleSegment rows, exactly as
    MerkleTree.update_record_segments has them (MerkleTree.adjust_key_segments)."""

    def __init__(self, key_bytes: int, length: int, depth: int, amount_bytes=8):
        self.amount_bytes = A = self._arg(amount_bytes, 1, 8, "amount_bytes is in [1, 8]")
        w, K = self._open(key_bytes, length, depth, A), self.key_bytes
        self.amount, self.side = w.c.public(8 * A), w.c.public(8)
        field = slice(16 * K, 16 * K + 8 * A)
        v, b = _key_bits_lsb_first(self.amount, A), _key_bits_lsb_first(self.old_record[field], A)
        side = self.side[0]
        bits, carry = [], side
        for x, y in zip(b, v):  # b + (v XOR side) + side: Words.ripple's full adders with the side as carry in
            s, carry = w.c.full_add(x, w.c.XOR(y, side), carry)
            bits.append(s)
        self.carry = carry
        # `bits` least significant first, back into the record's byte order
        self._close(self.old_record[: field.start] + [bits[8 * (A - 1 - j) + i] for j in range(A) for i in range(8)] + self.old_record[field.stop:],
                    self.amount, self.side)
        w.c.assert_same(self.carry, side)
        for x in self.side[1:]:
            w.c.assert_equal(x, 0)
        self._assert_key()
        self._assert_live()

    def _public(self, key, amount, side) -> bytes:
        """the checked K + A + 1 bytes of the public pieces behind the roots"""
        A = self.amount_bytes
        if not isinstance(amount, (int, np.integer)) or not 0 <= amount < 1 << (8 * A):
            raise CircuitError(f"MerkleAdjust: the amount is an integer in [0, 2^{8 * A})")
        if not isinstance(side, (int, np.integer)) or side not in (0, 1):
            raise CircuitError("MerkleAdjust: the side is 0 (a deposit) or 1 (a withdrawal)")
        return _checked_key("MerkleAdjust", self.key_bytes, key, "members") + int(amount).to_bytes(A, "big") + bytes([int(side)])

    def bits(self, key: bytes, amount: int, side: int, old_record: bytes, siblings, index: int):
        """one statement's input bits, public then private: 512 zeros where the two roots are computed, the bits of k, of the amount's A big-endian bytes
        and of the side byte, the old record's bits, the siblings from the leaf's level up, then the direction bits.  (A witness that breaks a constraint
        is not refused here: Circuit.holds / circuit_assign say so.)"""
        return self._step_bits(self._public(key, amount, side), old_record, siblings, index)


def _field_arg(who: str, field, key_bytes: int, length: int):
    """(lo, hi) of a written field, checked: two integers with 2 key_bytes <= lo < hi <= length"""
    try:
        lo, hi = field
    except (TypeError, ValueError):
        lo = hi = None
    if not all(isinstance(x, (int, np.integer)) for x in (lo, hi)) or not 2 * key_bytes <= lo < hi <= length:
        raise CircuitError(f"{who}: the field is (lo, hi) with 2 key_bytes <= lo < hi <= length -- the keys are never writable")
    return int(lo), int(hi)


class MerkleWrite(_RecordStep):
    """The statement "bytes [lo, hi) of the record of key k were set to v, and that alone takes the tree from root R to root R'" -- with expect=True "... were
    set to v, having been e": the PUT of the indexed table as a keyed store, plain or compare-and-set.  ONE record update, beside MerkleAdjust.

    field = (lo, hi) with 2K <= lo < hi <= length, F = hi - lo: the keys are never writable, the whole payload is.
    Public wires, in this order: R as 256 computed outputs at statement bits [0, 256), R' at [256, 512), the 8K given bits of k, with expect=True the 8F bits
    of e, the field's old bytes, then the 8F bits of v.  The values are bytes, not integers: byte j's bit b (LSB first) at 8 j + b, the record's own bit
    order.  lu = 512 + 8 (K + F), with expect=True 512 + 8 (K + 2F).  statement(R, R', k, v) or statement(R, R', k, e, v) is MerkleUpdate.statement's 64
    bytes, then k, [e,] v.
    Private inputs, in this order: the old record (8 * length bits, byte j's bit b at 8 j + b); `depth` siblings of 8 words from the leaf's level up;
    `depth` direction bits -- _tail_wires, as MerkleAdjust has them.  nin = lu + 8 length + 257 depth.  The packed row: 64 zero bytes | k | [e |] v | old
    record | depth siblings as words | ceil(depth / 8) index bytes.
    The body.  The new record is not an input: it is the old record's wires with the field's 8F wires replaced by v's.  Two record chains (_message_chain)
    and MerkleUpdate's two level chains over the shared tail (_root_outputs).  assert_same: k = old[0, K); with expect=True e = old[lo, hi).  One comparator:
    less_than(lo_key, hi_key) = 1, the record is live.  The sentinel keys are refused as for members.
    Soundness.  Keys and the rest of the payload are the old record's wires, so every record's lo and hi are what they were: the table's invariant
    (MerkleAbsent) is kept.  By the invariant k is the lo of at most one live record, so the record opened is the record of k and no other.  v equal to the
    field's old bytes is a no-op with R' = R.  What it does not cover: like MerkleInsert, the records it does not open.
    MerkleTree.write_keys / write_bits perform a batch of writes on a device table and give the input rows; statement j is (R_j, R_j+1, k_j, [e_j,] v_j).  A
    key may occur in many steps of a batch, and an expectation may be one that only an earlier step of the batch satisfies.
    Sizes (MERKLE_WRITE_SIZES): MerkleAdjust's without the ripple; (8, 55, 9, (16, 55), True), the whole payload, fits Params(d=1 << 20, m=699050), depth 10
    does not.
    Cut form.  There is no `joined` parameter: the statement has one pair of tops, so segment 0 of a cut write (segment_levels) is MerkleWrite(K, length,
    c_0, field, expect) itself over the record's subtree of height c_0, and the upper ranges are MerkleSegment rows (MerkleTree.write_key_segments)."""

    def __init__(self, key_bytes: int, length: int, depth: int, field, expect=False):
        w = self._open(key_bytes, length, depth, 1)
        self.field = lo, hi = _field_arg("MerkleWrite", field, self.key_bytes, self.length)
        if not isinstance(expect, (bool, np.bool_)):
            raise CircuitError("MerkleWrite: expect is True or False")
        self.expect = bool(expect)
        self.field_bytes = F = hi - lo
        self.expected = w.c.public(8 * F) if self.expect else []
        self.value = w.c.public(8 * F)
        self._close(self.old_record[: 8 * lo] + self.value + self.old_record[8 * hi:], self.expected, self.value)
        self._assert_key()
        for x, y in zip(self.expected, self.old_record[8 * lo: 8 * hi]):
            w.c.assert_same(x, y)
        self._assert_live()

    def _public(self, key, *values) -> bytes:
        """the checked K + F [+ F] bytes of the public pieces behind the roots; values = (v,) or (e, v)"""
        if len(values) != (2 if self.expect else 1):
            raise CircuitError("MerkleWrite: the public values are (e, v) with expect=True and v alone without")
        values = [bytes(x) for x in values]
        if any(len(x) != self.field_bytes for x in values):
            raise CircuitError(f"MerkleWrite: a value is the field's {self.field_bytes} bytes")
        return _checked_key("MerkleWrite", self.key_bytes, key, "members") + b"".join(values)

    def bits(self, key: bytes, *values_record_siblings_index):
        """bits(key, [expected,] value, old_record, siblings, index): one statement's input bits, public then private -- 512 zeros where the two roots are
        computed, the bits of k, of e with expect=True and of v, the old record's bits, the siblings from the leaf's level up, then the direction bits.  (A
        witness that breaks a constraint is not refused here: Circuit.holds / circuit_assign say so.)"""
        if len(values_record_siblings_index) != (5 if self.expect else 4):
            raise CircuitError(f"MerkleWrite: bits(key, {'expected, ' if self.expect else ''}value, old_record, siblings, index)")
        *values, old_record, siblings, index = values_record_siblings_index
        return self._step_bits(self._public(key, *values), old_record, siblings, index)


class Block:
    """A BLOCK of a keyed ledger: transfers, adjusts and writes in any order, built step by step and applied in that order by MerkleTree.apply_block /
    apply_block_segments in one device call.  key_bytes = K and amount_bytes = A hold for the whole block; a write's field is per step.  A step's statement is
    an existing one -- MerkleTransfer, MerkleAdjust or MerkleWrite over (R_j, R_j+1) -- and a step may spend what the step before it delivered; a write may
    cover balance bytes.  Inserts and removes are no steps of a block: they change membership.

    .transfer(k_from, k_to, v), .adjust(k, v, side=0), .write(k, (lo, hi), value, expect=None) append one step and return the block; len(block) is the
    number of steps; .steps is the list of (kind, ...) tuples: (Block.TRANSFER, k_from, k_to, v), (Block.ADJUST, k, v, side), (Block.WRITE, k, (lo, hi),
    value, expect or None).  What needs the record's length (a field's upper end, the balance's room) is judged where the block is applied."""

    TRANSFER, ADJUST, WRITE = 0, 1, 2

    def __init__(self, key_bytes: int, amount_bytes=8):
        if not isinstance(key_bytes, (int, np.integer)) or not 1 <= key_bytes <= 32:
            raise CircuitError("Block: key_bytes is in [1, 32]")
        if not isinstance(amount_bytes, (int, np.integer)) or not 1 <= amount_bytes <= 8:
            raise CircuitError("Block: amount_bytes is in [1, 8]")
        self.key_bytes, self.amount_bytes = int(key_bytes), int(amount_bytes)
        self.steps = []

    def __len__(self):
        return len(self.steps)

    def _key(self, key) -> bytes:
        return _checked_key("Block", self.key_bytes, key, "members")

    def _amount(self, v) -> int:
        if not isinstance(v, (int, np.integer)) or not 0 <= v < 1 << (8 * self.amount_bytes):
            raise CircuitError(f"Block: the amount is an integer in [0, 2^{8 * self.amount_bytes})")
        return int(v)

    def transfer(self, k_from, k_to, v):
        k_from, k_to = self._key(k_from), self._key(k_to)
        if k_from == k_to:
            raise CircuitError("Block: a transfer from an account to itself")
        self.steps.append((self.TRANSFER, k_from, k_to, self._amount(v)))
        return self

    def adjust(self, k, v, side=0):
        if not isinstance(side, (int, np.integer)) or side not in (0, 1):
            raise CircuitError("Block: the side is 0 (a deposit) or 1 (a withdrawal)")
        self.steps.append((self.ADJUST, self._key(k), self._amount(v), int(side)))
        return self

    def write(self, k, field, value, expect=None):
        lo, hi = _field_arg("Block", field, self.key_bytes, 1 << 20)
        value = bytes(value)
        expect = None if expect is None else bytes(expect)
        if len(value) != hi - lo or (expect is not None and len(expect) != hi - lo):
            raise CircuitError(f"Block: a value is the field's {hi - lo} bytes")
        self.steps.append((self.WRITE, self._key(k), (lo, hi), value, expect))
        return self

    def columns(self):
        """the steps as the arrays mfh_merkle_block_keys takes, made in one pass and kept for as long as `steps` holds the same steps (compared step by step at every call, so an appended, assigned or replaced step makes them anew): a dict of kinds np.uint8 [nk], keys and keys_to
        np.uint8 [nk, K] (keys_to: zero for a step that is no transfer), amounts np.uint64 [nk], sides np.uint8 [nk], fields np.uint32 [nk, 2], value_at and
        expect_at np.uint64 [nk] (offsets into values and expect; 2^64 - 1: no expectation), values and expect np.uint8 (at least one byte each), updates
        (the record updates of all steps) and field_hi, the largest hi of a written field (0: no write)"""
        now = tuple(self.steps)  # (a step is an immutable tuple, so the steps are what they were exactly when this tuple is: appended to, assigned, or edited in place)
        cached = getattr(self, "_columns", None)
        if cached is not None and cached[0] == now:
            return cached[1]
        K, nk = self.key_bytes, len(self.steps)
        kinds, keys, keys_to, amounts, sides, fields, value_at, expect_at = [], bytearray(), bytearray(), [], [], [], [], []
        values, expect, none, field_hi = bytearray(), bytearray(), bytes(K), 0
        for s in self.steps:
            kinds.append(s[0])
            keys += s[1]
            if s[0] == self.WRITE:
                keys_to += none
                amounts.append(0)
                sides.append(0)
                fields += s[2]
                field_hi = max(field_hi, s[2][1])
                value_at.append(len(values))
                values += s[3]
                expect_at.append(0xFFFFFFFFFFFFFFFF if s[4] is None else len(expect))
                if s[4] is not None:
                    expect += s[4]
            else:
                transfer = s[0] == self.TRANSFER
                keys_to += s[2] if transfer else none
                amounts.append(s[3] if transfer else s[2])
                sides.append(0 if transfer else s[3])
                fields += (0, 0)
                value_at.append(0)
                expect_at.append(0xFFFFFFFFFFFFFFFF)
        cols = {"kinds": np.array(kinds, dtype=np.uint8).reshape(nk), "keys": np.frombuffer(bytes(keys), dtype=np.uint8).reshape(nk, K),
                "keys_to": np.frombuffer(bytes(keys_to), dtype=np.uint8).reshape(nk, K), "amounts": np.array(amounts, dtype=np.uint64).reshape(nk),
                "sides": np.array(sides, dtype=np.uint8).reshape(nk), "fields": np.array(fields, dtype=np.uint32).reshape(nk, 2),
                "value_at": np.array(value_at, dtype=np.uint64).reshape(nk), "expect_at": np.array(expect_at, dtype=np.uint64).reshape(nk),
                "values": np.frombuffer(bytes(values) or b"\0", dtype=np.uint8), "expect": np.frombuffer(bytes(expect) or b"\0", dtype=np.uint8),
                "values_bytes": len(values), "expect_bytes": len(expect), "updates": nk + kinds.count(self.TRANSFER), "field_hi": field_hi}
        self._columns = (now, cols)
        return cols

    def statement_key(self, j: int, length: int, depth: int):
        """what names step j's statement object, the class and its arguments: ("MerkleTransfer", K, length, depth, A), ("MerkleAdjust", K, length, depth, A)
        or ("MerkleWrite", K, length, depth, (lo, hi), expect) -- getattr(words, key[0])(*key[1:]) builds it"""
        step = self.steps[j]
        if step[0] == self.WRITE:
            return ("MerkleWrite", self.key_bytes, int(length), int(depth), step[2], step[4] is not None)
        return ("MerkleTransfer" if step[0] == self.TRANSFER else "MerkleAdjust", self.key_bytes, int(length), int(depth), self.amount_bytes)

    def statements(self, length: int, depth: int, roots, status=None):
        """one entry a step: (statement_key(j, length, depth), the statement bytes for (R_j, R_j+1) = roots[j], roots[j + 1]) -- the existing classes'
        .statement(..) on a stand-in that has the sizes and no circuit, so nothing is compiled here.  roots: the nk + 1 roots of 32 bytes.  status (nk values,
        as apply_block gives them): a step with a status other than 0 was skipped and gives None"""
        if len(roots) != len(self.steps) + 1:
            raise CircuitError("Block: statements takes the nk + 1 roots R_0 .. R_nk")
        if status is not None and len(status) != len(self.steps):
            raise CircuitError("Block: status has one value a step")
        out = []
        for j, step in enumerate(self.steps):
            if status is not None and int(status[j]):
                out.append(None)
                continue
            key = self.statement_key(j, length, depth)
            st = object.__new__(globals()[key[0]])
            st.key_bytes, st.length, st.depth = key[1:4]
            old, new = bytes(roots[j]), bytes(roots[j + 1])
            if step[0] == self.WRITE:
                st.field, st.field_bytes, st.expect = step[2], step[2][1] - step[2][0], step[4] is not None
                pieces = (step[1],) + ((step[4],) if st.expect else ()) + (step[3],)
            else:
                st.amount_bytes = self.amount_bytes
                pieces = step[1:]
            out.append((key, st.statement(old, new, *pieces)))
        return out


def _keys_array(keys, who: str):
    """keys as np.uint8 [n, K]: an array of that shape, or n bytes-likes of one length K >= 1"""
    if isinstance(keys, np.ndarray):
        a = keys
    else:
        keys = [bytes(k) for k in keys]
        if not keys:
            raise CircuitError(f"{who}: an empty set of keys is a uint8 array [0, key_bytes] (a list does not say key_bytes)")
        if len({len(k) for k in keys}) > 1:
            raise CircuitError(f"{who}: the keys are of one length")
        a = np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), len(keys[0]))
    if a.dtype != np.uint8 or a.ndim != 2 or not 1 <= a.shape[1] <= 32:
        raise CircuitError(f"{who}: keys are uint8 [n, key_bytes], key_bytes in [1, 32]")
    return a


def indexed_records(keys, depth: int, length=None, payloads=None):
    """np.uint8 [2^depth, length]: a well-formed indexed table (MerkleAbsent) of the set `keys` -- record 0 the sentinel record (0...0, smallest key),
    then one record (key, next larger key) per member in ascending order, the last with hi = FF...FF, the unused slots all zero (lo >= hi: inert).
    keys: n bytes-likes of one length K, or a uint8 array [n, K] (the only way to say K for the empty set), in any order.  length defaults to 2 K.
    payloads: one bytes-like per key, in the order of `keys`, at most length - 2 K bytes each, zero-padded; the sentinel record's payload is zero.
    CircuitError for duplicates, sentinel keys, or more than 2^depth - 1 members."""
    a = _keys_array(keys, "indexed_records")
    n, K = a.shape
    length = 2 * K if length is None else int(length)
    if length < 2 * K:
        raise CircuitError("indexed_records: the length is at least 2 key_bytes bytes")
    if not isinstance(depth, (int, np.integer)) or depth < 1 or n > (1 << depth) - 1:
        raise CircuitError("indexed_records: a depth >= 1 and at most 2^depth - 1 members")
    members = [k.tobytes() for k in a]
    if any(_is_sentinel(k) for k in members):
        raise CircuitError("indexed_records: the all-zero and the all-0xFF key are sentinels, never members")
    if len(set(members)) != n:
        raise CircuitError("indexed_records: a key is given twice")
    if payloads is None:
        payloads = [b""] * n
    payloads = [bytes(p) for p in payloads]
    if len(payloads) != n or any(len(p) > length - 2 * K for p in payloads):
        raise CircuitError("indexed_records: one payload of at most length - 2 key_bytes bytes per key")
    order = sorted(range(n), key=lambda i: members[i])
    los = [bytes(K)] + [members[i] for i in order]
    pay = [b""] + [payloads[i] for i in order]
    table = np.zeros((1 << depth, length), dtype=np.uint8)
    for r, (lo, p) in enumerate(zip(los, pay)):
        hi = los[r + 1] if r + 1 < len(los) else b"\xff" * K
        table[r, : 2 * K + len(p)] = np.frombuffer(lo + hi + p, dtype=np.uint8)
    return table


def indexed_insert(record_p, p: int, key: bytes, free_slot: int, payload: bytes = b""):
    """(indices, new_records): the two updates that insert `key` into an indexed table, in the order MerkleTree.update_records takes them.  record_p is
    record p of the table, the one whose range holds the key (lo < key < hi: what MerkleTree.locate_keys reports with status 0); free_slot is any inert
    slot.  Update 0 is record p with hi <- key (lo and payload kept), update 1 the record (key, the old hi, payload zero-padded) into free_slot.
    key_bytes is len(key).  CircuitError when the key is not inside record p's range."""
    record_p, key, payload = bytes(record_p), bytes(key), bytes(payload)
    K, length = len(key), len(record_p)
    if not 1 <= K <= 32 or length < 2 * K or len(payload) > length - 2 * K:
        raise CircuitError("indexed_insert: a key of 1 .. 32 bytes, a record of at least 2 key_bytes bytes, a payload that fits behind the keys")
    lo, hi = record_p[:K], record_p[K: 2 * K]
    if not lo < key < hi:
        raise CircuitError("indexed_insert: the key is not inside record p's range (lo < key < hi)")
    if p == free_slot or p < 0 or free_slot < 0:
        raise CircuitError("indexed_insert: p and free_slot are two different slots")
    new = np.zeros((2, length), dtype=np.uint8)
    new[0] = np.frombuffer(lo + key + record_p[2 * K:], dtype=np.uint8)
    new[1, : 2 * K + len(payload)] = np.frombuffer(key + hi + payload, dtype=np.uint8)
    return [int(p), int(free_slot)], new


def indexed_remove(record_p, p: int, record_s, s: int, key_bytes=None):
    """(indices, new_records): the two updates that remove a key from an indexed table, in the order MerkleTree.update_records takes them, p first.
    record_s is record s of the table, the live record whose own key (lo) is the key to remove; record_p is record p, the live record whose hi is that
    key.  Update 0 is record p with hi <- record s's hi (lo and payload kept), update 1 the all-zero record into slot s (inert, as indexed_records
    leaves unused slots).  key_bytes defaults to half the records' length, indexed_records' default layout; say it for records with payloads.
    CircuitError when record_p[K:2K] != record_s[:K], when either record is not live (lo < hi), or when p == s."""
    record_p, record_s = bytes(record_p), bytes(record_s)
    length = len(record_p)
    K = length // 2 if key_bytes is None else key_bytes
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= 32 or length < 2 * K or len(record_s) != length:
        raise CircuitError("indexed_remove: two records of one length, at least 2 key_bytes bytes, key_bytes in [1, 32]")
    if record_p[K: 2 * K] != record_s[:K]:
        raise CircuitError("indexed_remove: record p's hi is not record s's key (record_p[K:2K] != record_s[:K])")
    if not record_p[:K] < record_p[K: 2 * K] or not record_s[:K] < record_s[K: 2 * K]:
        raise CircuitError("indexed_remove: a record is not live (lo < hi)")
    if p == s or p < 0 or s < 0:
        raise CircuitError("indexed_remove: p and s are two different slots")
    new = np.zeros((2, length), dtype=np.uint8)
    new[0] = np.frombuffer(record_p[:K] + record_s[K: 2 * K] + record_p[2 * K:], dtype=np.uint8)
    return [int(p), int(s)], new


def indexed_transfer(record_p, p: int, record_s, s: int, amount: int, key_bytes: int, amount_bytes=8):
    """(indices, new_records): the two updates that move `amount` from the account in slot p to the account in slot s of an indexed table whose records
    carry a balance (MerkleTransfer has the data model), in the order MerkleTree.update_records takes them, p first.  record_p and record_s are the two
    live records as they stand; update 0 is record p with its balance, bytes [2K, 2K + A) big-endian, less the amount, update 1 record s with its
    balance plus the amount; nothing else of either changes.  CircuitError on an overdraft (amount > p's balance), an overflow (s's balance + amount
    >= 2^(8A)), p == s, or a record that is not live (lo < hi)."""
    record_p, record_s = bytes(record_p), bytes(record_s)
    K, A, length = key_bytes, amount_bytes, len(record_p)
    if (not all(isinstance(x, (int, np.integer)) for x in (K, A)) or not 1 <= K <= 32 or not 1 <= A <= 8 or length < 2 * K + A or len(record_s) != length):
        raise CircuitError("indexed_transfer: two records of one length, at least 2 key_bytes + amount_bytes bytes, key_bytes in [1, 32], amount_bytes in [1, 8]")
    if not isinstance(amount, (int, np.integer)) or not 0 <= amount < 1 << (8 * A):
        raise CircuitError(f"indexed_transfer: the amount is an integer in [0, 2^{8 * A})")
    if not record_p[:K] < record_p[K: 2 * K] or not record_s[:K] < record_s[K: 2 * K]:
        raise CircuitError("indexed_transfer: a record is not live (lo < hi)")
    if p == s or p < 0 or s < 0:
        raise CircuitError("indexed_transfer: p and s are two different slots")
    b_p, b_s = (int.from_bytes(r[2 * K: 2 * K + A], "big") for r in (record_p, record_s))
    if amount > b_p:
        raise CircuitError(f"indexed_transfer: an overdraft, the sender has {b_p}")
    if b_s + amount >= 1 << (8 * A):
        raise CircuitError(f"indexed_transfer: the receiver's balance would exceed 2^{8 * A} - 1")
    new = np.zeros((2, length), dtype=np.uint8)
    new[0] = np.frombuffer(record_p[: 2 * K] + (b_p - int(amount)).to_bytes(A, "big") + record_p[2 * K + A:], dtype=np.uint8)
    new[1] = np.frombuffer(record_s[: 2 * K] + (b_s + int(amount)).to_bytes(A, "big") + record_s[2 * K + A:], dtype=np.uint8)
    return [int(p), int(s)], new


def indexed_adjust(record, amount: int, side: int, key_bytes: int, amount_bytes=8):
    """the new record, np.uint8 [length]: `record`, a live record of an indexed table whose records carry a balance (MerkleTransfer has the data model),
    with its balance, bytes [2K, 2K + A) big-endian, plus the amount (side 0, a deposit) or less the amount (side 1, a withdrawal); nothing else of it
    changes.  CircuitError on a record that is not live (lo < hi), an overdraft (amount > the balance) or an overflow (balance + amount >= 2^(8A))."""
    record = bytes(record)
    K, A, length = key_bytes, amount_bytes, len(record)
    if not all(isinstance(x, (int, np.integer)) for x in (K, A)) or not 1 <= K <= 32 or not 1 <= A <= 8 or length < 2 * K + A:
        raise CircuitError("indexed_adjust: a record of at least 2 key_bytes + amount_bytes bytes, key_bytes in [1, 32], amount_bytes in [1, 8]")
    if not isinstance(amount, (int, np.integer)) or not 0 <= amount < 1 << (8 * A):
        raise CircuitError(f"indexed_adjust: the amount is an integer in [0, 2^{8 * A})")
    if not isinstance(side, (int, np.integer)) or side not in (0, 1):
        raise CircuitError("indexed_adjust: the side is 0 (a deposit) or 1 (a withdrawal)")
    if not record[:K] < record[K: 2 * K]:
        raise CircuitError("indexed_adjust: the record is not live (lo < hi)")
    b = int.from_bytes(record[2 * K: 2 * K + A], "big")
    if side and amount > b:
        raise CircuitError(f"indexed_adjust: an overdraft, the account has {b}")
    if not side and b + amount >= 1 << (8 * A):
        raise CircuitError(f"indexed_adjust: the balance would exceed 2^{8 * A} - 1")
    fresh = b - int(amount) if side else b + int(amount)
    return np.frombuffer(record[: 2 * K] + fresh.to_bytes(A, "big") + record[2 * K + A:], dtype=np.uint8).copy()


def indexed_write(record, field, value, key_bytes: int, expect=None):
    """the new record, np.uint8 [length]: `record`, a live record of an indexed table, with its bytes [lo, hi) = field set to `value` (MerkleWrite has the
    statement); nothing else of it changes.  expect: the hi - lo bytes the field must hold now (None: a plain write).  CircuitError on a record that is not
    live (lo < hi), a field outside [2 key_bytes, length], a value that is not hi - lo bytes, or an expectation the record does not meet."""
    record = bytes(record)
    K, length = key_bytes, len(record)
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= 32 or length < 2 * K + 1:
        raise CircuitError("indexed_write: a record of at least 2 key_bytes + 1 bytes, key_bytes in [1, 32]")
    lo, hi = _field_arg("indexed_write", field, K, length)
    value = bytes(value)
    if len(value) != hi - lo:
        raise CircuitError(f"indexed_write: the value is the field's {hi - lo} bytes")
    if not record[:K] < record[K: 2 * K]:
        raise CircuitError("indexed_write: the record is not live (lo < hi)")
    if expect is not None:
        expect = bytes(expect)
        if len(expect) != hi - lo:
            raise CircuitError(f"indexed_write: the expected value is the field's {hi - lo} bytes")
        if record[lo:hi] != expect:
            raise CircuitError("indexed_write: the field is not what was expected")
    return np.frombuffer(record[:lo] + value + record[hi:], dtype=np.uint8).copy()


def indexed_range(table, key_bytes: int, lo: bytes, hi: bytes):
    """the ordered slots of the links of the key range [lo, hi] in an indexed table (a uint8 array [n, length]; MerkleLink has the read): the live records
    with record.hi >= lo and record.lo <= hi, sorted by (record.lo, slot) -- in a well-formed table the records (p, k_1), (k_1, k_2), .., (k_n, s) around
    and between the members k_1 .. k_n of [lo, hi].  The host reference of MerkleTree.range_rows.  CircuitError for bounds that are not key_bytes bytes,
    a sentinel bound, or lo > hi."""
    table = np.asarray(table)
    K = key_bytes
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= 32 or table.dtype != np.uint8 or table.ndim != 2 or table.shape[1] < 2 * K:
        raise CircuitError("indexed_range: a uint8 table [n, length], length at least 2 key_bytes, key_bytes in [1, 32]")
    lo, hi = _checked_key("indexed_range", K, lo, "bounds"), _checked_key("indexed_range", K, hi, "bounds")
    if lo > hi:
        raise CircuitError("indexed_range: the range is lo <= hi")
    def less(a, b):  # a < b per row, big-endian: the first byte that differs decides
        res, open_ = np.zeros(len(table), dtype=bool), np.ones(len(table), dtype=bool)
        for j in range(K):
            res |= open_ & (a[:, j] < b[:, j])
            open_ &= a[:, j] == b[:, j]
        return res

    rlo, rhi = table[:, :K], table[:, K: 2 * K]
    a, b = (np.broadcast_to(np.frombuffer(x, dtype=np.uint8), rlo.shape) for x in (lo, hi))
    slots = np.flatnonzero(less(rlo, rhi) & ~less(rhi, a) & ~less(b, rlo))
    return [int(s) for _, s in sorted((rlo[s].tobytes(), int(s)) for s in slots)]


def indexed_check(table, key_bytes: int):
    """(status, live, where): the CHAIN part of the invariant of an indexed table (a uint8 array [n, length]) -- the live records (lo < hi), sorted by (lo,
    slot), tile the key space from 00..00 to FF..FF.  live is their number.  Status 0 (where = None): they do.  Status 1: where is the slot of the first
    record in sorted order at which the chain breaks -- sorted record 0 when its lo is not 00..00, sorted record i + 1 at the lowest i with hi_i != lo_i+1,
    the last record when its hi is not FF..FF --, 0xFFFFFFFF when no record is live.  The host reference of MerkleTree.check_table's status 1.
    CircuitError for a table that is not uint8 [n, length >= 2 key_bytes] or a key_bytes outside [1, 32]."""
    K = key_bytes
    if not isinstance(K, (int, np.integer)) or not 1 <= K <= 32 or not isinstance(table, np.ndarray) or table.dtype != np.uint8 or table.ndim != 2 \
            or table.shape[1] < 2 * K:
        raise CircuitError("indexed_check: a uint8 table [n, length], length at least 2 key_bytes, key_bytes in [1, 32]")
    rlo, rhi = table[:, :K], table[:, K: 2 * K]
    live, open_ = np.zeros(len(table), dtype=bool), np.ones(len(table), dtype=bool)
    for j in range(K):  # lo < hi per row, big-endian: the first byte that differs decides
        live |= open_ & (rlo[:, j] < rhi[:, j])
        open_ &= rlo[:, j] == rhi[:, j]
    slots = np.flatnonzero(live)
    n = len(slots)
    if not n:
        return 1, 0, 0xFFFFFFFF
    order = np.lexsort((slots,) + tuple(rlo[slots, j] for j in range(K - 1, -1, -1)))  # (lexsort: the LAST key is the primary one)
    s = slots[order]
    lo, hi = rlo[s], rhi[s]
    if lo[0].any():
        return 1, n, int(s[0])
    breaks = np.flatnonzero((hi[:-1] != lo[1:]).any(axis=1))
    if len(breaks):
        return 1, n, int(s[breaks[0] + 1])
    if (hi[-1] != 0xFF).any():
        return 1, n, int(s[-1])
    return 0, n, None


def merkle_node(left: bytes, right: bytes) -> bytes:
    """MerklePath's node function on the host: compress(IV, left || right), ONE SHA-256 compression of the 64 bytes with no padding block (FIPS 180-4 6.2.2;
    hashlib does not expose it).  What a verifier needs to evaluate grown_root."""
    left, right = bytes(left), bytes(right)
    if len(left) != 32 or len(right) != 32:
        raise CircuitError("merkle_node: two nodes of 32 bytes")
    rotr = lambda x, n: (x >> n | x << (32 - n)) & MASK
    w = [int.from_bytes((left + right)[4 * t: 4 * t + 4], "big") for t in range(16)]
    for t in range(16, 64):
        s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ w[t - 15] >> 3
        s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ w[t - 2] >> 10
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & MASK)
    a, b, c, d, e, f, g, h = SHA256_IV
    for t in range(64):
        t1 = (h + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + (e & f ^ ~e & g & MASK) + SHA256_K[t] + w[t]) & MASK
        t2 = ((rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + (a & b ^ a & c ^ b & c)) & MASK
        a, b, c, d, e, f, g, h = (t1 + t2) & MASK, a, b, c, (d + t1) & MASK, e, f, g
    return b"".join(((x + y) & MASK).to_bytes(4, "big") for x, y in zip(SHA256_IV, (a, b, c, d, e, f, g, h)))


GROW_MAX_DEPTH = 24  # the deepest tree (mfh_merkle_create)


def inert_roots(depth: int, length=None):
    """[E_0 .. E_depth], 32 bytes each: the root E_l of a subtree of height l whose leaves are all inert, E_l+1 = merkle_node(E_l, E_l).  With a `length`
    E_0 = SHA-256 of `length` zero bytes, the leaf of an all-zero record (lo >= hi: an inert slot of an indexed table); with length=None E_0 is 32 zero
    bytes, the leaf of a fresh tree of leaves, whose root at depth D is inert_roots(D)[-1].  CircuitError unless 0 <= depth <= 24 and 0 <= length <= 2^20."""
    if not isinstance(depth, (int, np.integer)) or not 0 <= depth <= GROW_MAX_DEPTH:
        raise CircuitError("inert_roots: a depth in [0, 24]")
    if length is not None and (not isinstance(length, (int, np.integer)) or not 0 <= length <= 1 << 20):
        raise CircuitError("inert_roots: a length in [0, 2^20], or None for a tree of leaves")
    e = [bytes(32) if length is None else hashlib.sha256(bytes(int(length))).digest()]
    for _ in range(int(depth)):
        e.append(merkle_node(e[-1], e[-1]))
    return e


def grown_root(root: bytes, depth: int, new_depth: int, length=None) -> bytes:
    """the root R' of the tree of `new_depth` whose leftmost subtree of height `depth` has the root R = `root` and whose other leaves are all inert (what
    MerkleTree.grow makes): S_depth = R, S_l+1 = merkle_node(S_l, E_l) with E = inert_roots(.., length), R' = S_new_depth.  new_depth - depth compressions of
    public values: a verifier who follows a chain of roots evaluates this to accept the jump R -> R'; there is nothing to prove.  Growing depth -> m -> new_depth
    gives what depth -> new_depth gives.  CircuitError unless 1 <= depth < new_depth <= 24 and the root is 32 bytes."""
    if not all(isinstance(x, (int, np.integer)) for x in (depth, new_depth)) or not 1 <= depth < new_depth <= GROW_MAX_DEPTH:
        raise CircuitError("grown_root: 1 <= depth < new_depth <= 24")
    if not isinstance(root, (bytes, bytearray, memoryview, np.ndarray)) or len(bytes(root)) != 32:
        raise CircuitError("grown_root: the root is 32 bytes")
    e = inert_roots(int(new_depth) - 1, length)
    s = bytes(root)
    for l in range(int(depth), int(new_depth)):
        s = merkle_node(s, e[l])
    return s


def indexed_grow(table, new_depth: int):
    """np.uint8 [2^new_depth, length]: the host table (a uint8 array [2^depth, length]) with all-zero rows appended -- inert slots (lo >= hi), so
    indexed_check gives the grown table the answer it gave the original.  The model of the table MerkleTree.grow writes.  CircuitError unless the table has
    2^depth rows, depth >= 1, and depth < new_depth <= 24."""
    if not isinstance(table, np.ndarray) or table.dtype != np.uint8 or table.ndim != 2 or len(table) < 2 or len(table) & (len(table) - 1):
        raise CircuitError("indexed_grow: a uint8 table [2^depth, length], depth >= 1")
    depth = len(table).bit_length() - 1
    if not isinstance(new_depth, (int, np.integer)) or not depth < new_depth <= GROW_MAX_DEPTH:
        raise CircuitError("indexed_grow: depth < new_depth <= 24")
    return np.concatenate([table, np.zeros(((1 << int(new_depth)) - len(table), table.shape[1]), dtype=np.uint8)])


# (wires, rows) of Sha256Message by length in bytes, as compile counts them; 0 .. 55 bytes are one block and fit Params(d=1 << 16, m=43690) and the LDS
# witness kernel, 56 .. 119 are two blocks and fit Params(d=1 << 17, m=87381).  A constant zero bit of the padding is left out of the sums it would enter
# (Words.sum), which can shorten a weighted-sum gate: an all-padding block costs a few wires less than a block of message bits.
SHA256_MESSAGE_SIZES = {0: (27588, 49062), 55: (28042, 49516), 56: (55382, 98072), 100: (55746, 98436), 119: (55898, 98588), 120: (83238, 147144)}
# ... and of MerklePath by depth: 28 625 depth + 514 wires, 50 865 depth + 772 rows
MERKLE_PATH_SIZES = {1: (29139, 51637), 2: (57764, 102502), 3: (86389, 153367), 20: (573014, 1018072)}
# ... and of MerkleRecord by (length, depth): those of Sha256Message(length) plus 28 625 depth wires and 50 865 depth rows
MERKLE_RECORD_SIZES = {(0, 1): (56213, 99927), (55, 1): (56667, 100381), (56, 1): (84007, 148937), (119, 1): (84523, 149453), (120, 1): (111863, 198009),
                       (3, 2): (84865, 150819), (55, 2): (85292, 151246), (56, 2): (112632, 199802), (55, 19): (571917, 1015951), (119, 18): (571148, 1014158)}
# ... and of MerkleLink by (key_bytes, length, depth, reveal): MerkleRecord(length, depth)'s, wire for wire and row for row (the shown prefix is 8 P public
# inputs where MerkleRecord's record bits are private ones), every entry compiled; it keeps MerkleRecord's depth range
MERKLE_LINK_SIZES = {(4, 8, 1, 0): (56284, 99998), (8, 55, 1, 8): (56667, 100381), (4, 9, 1, 1): (56292, 100006), (4, 8, 2, 0): (84909, 150863)}
# ... and of MerkleUpdate by depth: 56 993 depth + 1 026 wires, 101 473 depth + 1 540 rows
MERKLE_UPDATE_SIZES = {1: (58019, 103013), 2: (115012, 204486), 3: (172005, 305959), 10: (570956, 1016270)}
# ... and of MerkleRecordUpdate by (length, depth): MERKLE_UPDATE_SIZES[depth] + 2 x SHA256_MESSAGE_SIZES[length] - (1 028, 1 544); frozen=(lo, hi) adds
# 8 (hi - lo) rows and no wire.  (55, 9) and (119, 8) are the deepest that fit Params(d=1 << 20, m=699050): (55, 10) would be 1 113 758 rows, (119, 9) 1 110 429
MERKLE_RECORD_UPDATE_SIZES = {(8, 1): (112309, 199735), (55, 1): (113075, 200501), (56, 1): (167755, 297613), (55, 2): (170068, 301974),
                              (55, 9): (569019, 1012285), (119, 8): (567738, 1008956)}
# ... and of MerkleAbsent by (key_bytes, length, depth): those of MerkleRecord(length, depth) plus 40 key_bytes wires and 72 key_bytes + 2 rows (a comparison
# is 16 key_bytes wires and 32 key_bytes + 1 rows; q is 8 key_bytes public wires and their bit rows).  (4, 8, 1) and (8, 16, 1) fit Params(d=1 << 17,
# m=87381), (32, 64, 1) (two blocks) Params(d=1 << 18, m=174762); (8, 55, 19) is the deepest one-block statement that fits Params(d=1 << 20, m=699050):
# (8, 55, 20) would be 1 067 394 rows
MERKLE_ABSENT_SIZES = {(4, 8, 1): (56444, 100288), (8, 16, 1): (56672, 100644), (32, 64, 1): (85352, 151308), (8, 55, 19): (572237, 1016529)}
# ... and of MerkleInsert by (key_bytes, length, depth): twice MerkleRecordUpdate(length, depth)'s, less 8 length - 56 key_bytes + 514 wires and 8 length - 120
# key_bytes + 769 rows -- the new record of p is no input (8 length wires and bit rows), the roots are output once, not twice (512 wires, 1 024 rows), the two
# constant wires are shared; k is 8 key_bytes public wires and bit rows, three comparisons are 16 key_bytes wires and 32 key_bytes + 1 rows each, and 256 + 16
# key_bytes equalities tie the middle roots, k and the inherited hi.  A level costs 113 986 wires and 202 946 rows (twice MerkleUpdate's).  Depth 1 fits
# Params(d=1 << 19, m=349525); (8, 55, 4) is the deepest one-block statement that fits Params(d=1 << 20, m=699050): (8, 55, 5) would be 1 212 537 rows
MERKLE_INSERT_SIZES = {(4, 8, 1): (224264, 399117), (8, 55, 1): (225644, 400753), (8, 16, 4): (566654, 1008643), (8, 55, 4): (567602, 1009591)}
# ... and of MerkleInsert(joined=False): the joined sizes plus 512 wires (two more tops are outputs) and 768 rows (their 512 bit rows and 512 equality rows, less
# the 256 equalities on the middle roots); (8, 55, 4) still fits Params(d=1 << 20, m=699050)
MERKLE_INSERT_SPLIT_SIZES = {(4, 8, 1): (224776, 399885), (8, 55, 1): (226156, 401521), (8, 55, 4): (568114, 1010359)}
# ... and of MerkleSegment by levels: MerkleUpdate's, 56 993 levels + 1 026 wires and 101 473 levels + 1 540 rows (the two nodes are public inputs where
# MerkleUpdate's leaves are private ones); 10 levels fit Params(d=1 << 20, m=699050), 11 (1 117 743 rows) do not
MERKLE_SEGMENT_SIZES = {1: (58019, 103013), 2: (115012, 204486), 10: (570956, 1016270)}
# ... and of MerkleClimb by levels: MerklePath's, 28 625 levels + 514 wires and 50 865 levels + 772 rows (the node is 256 public inputs where MerklePath's leaf is
# 256 private ones), every entry compiled; 20 levels (573 014 wires, 1 018 072 rows) fit Params(d=1 << 20, m=699050) and 21 (1 068 937 rows) do not, 10 fit
# d = 2^19, and 2 fit Params(d=1 << 17, m=87381) where 3 do not
MERKLE_CLIMB_SIZES = {1: (29139, 51637), 2: (57764, 102502), 3: (86389, 153367)}
# ... and of MerkleRemove by (key_bytes, length, depth): MerkleInsert's less one record chain (the new leaf of s is a constant), 8 length input wires and their
# bit rows (no new record of s) and one comparison (no inert check), with 16 key_bytes equalities on k as the insert has on k and the inherited hi.  A level
# costs 113 986 wires and 202 946 rows, MerkleInsert's.  (4, 8, 1) fits Params(d=1 << 19, m=349525) and not d = 2^18; (8, 55, 4) is the deepest one-block
# statement that fits Params(d=1 << 20, m=699050): (8, 55, 5) would be 1 163 280 rows
MERKLE_REMOVE_SIZES = {(4, 8, 1): (196799, 350371), (4, 8, 2): (310785, 553317), (8, 55, 1): (197732, 351496), (8, 55, 4): (539690, 960334)}
# ... and of MerkleRemove(joined=False): the joined sizes plus 512 wires and 768 rows, as MERKLE_INSERT_SPLIT_SIZES
MERKLE_REMOVE_SPLIT_SIZES = {(4, 8, 1): (197311, 351139), (8, 55, 1): (198244, 352264), (8, 55, 4): (540202, 961102)}
# ... and of MerkleTransfer by (key_bytes, length, depth, amount_bytes): MerkleInsert's four record chains and four level chains, one input record fewer (neither
# new record is an input), 16 key_bytes + 8 amount_bytes public wires, two comparisons, 16 key_bytes equalities on the keys, and the two ripples: 5 amount_bytes
# x 8 + 1 wires and 10 amount_bytes x 8 + 4 rows with their two assertions (an amount byte costs 48 wires and 88 rows: (4, 16, 1, 3) less (4, 16, 1, 1) is twice
# that).  A level costs 113 986 wires and 202 946 rows, MerkleInsert's.  (4, 16, 1, 8) fits Params(d=1 << 19, m=349525), (4, 16, 2, 8) does not; (8, 55, 4, 8)
# is the deepest one-block statement that fits Params(d=1 << 20, m=699050): (8, 55, 5, 8) would be 1 212 612 rows
MERKLE_TRANSFER_SIZES = {(4, 16, 1, 8): (224697, 399808), (4, 16, 2, 8): (338683, 602754), (4, 16, 1, 1): (224361, 399192), (4, 16, 1, 3): (224457, 399368),
                         (8, 55, 1, 8): (225525, 400828), (8, 55, 4, 8): (567483, 1009666)}
# ... and of MerkleTransfer(joined=False): the joined sizes plus 512 wires and 768 rows, as MERKLE_INSERT_SPLIT_SIZES
MERKLE_TRANSFER_SPLIT_SIZES = {(4, 16, 1, 8): (225209, 400576), (8, 55, 1, 8): (226037, 401596), (8, 55, 4, 8): (567995, 1010434)}
# ... and of MerkleAdjust by (key_bytes, length, depth, amount_bytes): MerkleRecordUpdate(length, depth)'s two record chains and two level chains with ONE input
# record (the new record is not an input), 8 (key_bytes + amount_bytes + 1) public wires, one comparison, 8 key_bytes equalities on the key, the carry's
# equality, the side byte's seven assertions, and the ripple: 4 wires and 7 rows an amount bit (an XOR and a full adder; (4, 16, 1, 3) less (4, 16, 1, 1) is
# (64, 112)).  A level costs 56 993 wires and 101 473 rows, MerkleUpdate's.  (8, 55, 1, 8) is 16 wires and 409 rows above MerkleRecordUpdate(55, 1); (4, 16, 1, 8)
# fits Params(d=1 << 18, m=174762); (8, 55, 9, 8) is the deepest one-block statement that fits Params(d=1 << 20, m=699050): (8, 55, 10, 8) would be 1 114 167 rows
MERKLE_ADJUST_SIZES = {(4, 16, 1, 8): (112677, 200400), (4, 16, 1, 1): (112453, 200008), (4, 16, 1, 3): (112517, 200120), (8, 55, 1, 8): (113091, 200910),
                       (4, 16, 2, 8): (169670, 301873), (8, 55, 9, 8): (569035, 1012694)}
# ... and of MerkleWrite by (key_bytes, length, depth, field, expect), F = hi - lo: MerkleAdjust(key_bytes, length, depth, F)'s two record chains and two level
# chains with ONE input record, without the side byte, the carry's equality and the ripple, the field's wires of the new record being v's own public wires: plain
# it is 8 + 24 F wires and 16 + 48 F rows BELOW MerkleAdjust with amount_bytes = F ((4, 16, 1, (8, 16)) is (200, 400) below (4, 16, 1, 8), (8, 55, 1, (16, 24))
# the same below (8, 55, 1, 8)).  A field byte costs 8 wires and 8 rows; expect=True adds 8 F wires and 16 F rows (e's public wires and its equalities:
# (4, 16, 1, (8, 16), True) less (4, 16, 1, (9, 10), True) is 7 x (16, 24)).  A level costs 56 993 wires and 101 473 rows, MerkleUpdate's.  (4, 16, 1, ..) fits
# Params(d=1 << 18, m=174762); (8, 55, 9, (16, 55), True), the whole payload under compare-and-set, is the deepest that fits Params(d=1 << 20, m=699050):
# (8, 55, 10, (16, 55), True) would be 1 114 639 rows
MERKLE_WRITE_SIZES = {(4, 16, 1, (8, 16), False): (112477, 200000), (4, 16, 1, (8, 16), True): (112541, 200128), (4, 16, 1, (9, 10), True): (112429, 199960),
                      (4, 16, 2, (8, 16), True): (169534, 301601), (8, 55, 1, (16, 24), False): (112891, 200510), (8, 55, 1, (16, 24), True): (112955, 200638),
                      (8, 55, 9, (16, 55), True): (569395, 1013166)}
