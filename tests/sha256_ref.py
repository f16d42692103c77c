"""A pure-Python SHA-256 compression function (FIPS 180-4 6.2.2), written from the standard and independent of words.py: the reference of the Merkle
node function parent = compress(IV, left || right), which hashlib does not expose.  The constants are derived here from the primes, not imported."""
MASK = 0xFFFFFFFF


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
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if mid ** root <= target:
            lo = mid
        else:
            hi = mid - 1
    return lo & MASK


IV = tuple(_frac_root(q, 2) for q in _primes(8))
K = tuple(_frac_root(q, 3) for q in _primes(64))


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & MASK


def compress(h, block: bytes):
    """the eight words after one 64-byte block, from the eight words h"""
    assert len(h) == 8 and len(block) == 64
    w = [int.from_bytes(block[4 * t: 4 * t + 4], "big") for t in range(16)]
    for t in range(16, 64):
        s0 = _rotr(w[t - 15], 7) ^ _rotr(w[t - 15], 18) ^ (w[t - 15] >> 3)
        s1 = _rotr(w[t - 2], 17) ^ _rotr(w[t - 2], 19) ^ (w[t - 2] >> 10)
        w.append((w[t - 16] + s0 + w[t - 7] + s1) & MASK)
    a, b, c, d, e, f, g, hh = h
    for t in range(64):
        t1 = (hh + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & g & MASK)) + K[t] + w[t]) & MASK
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & MASK
        a, b, c, d, e, f, g, hh = (t1 + t2) & MASK, a, b, c, (d + t1) & MASK, e, f, g
    return tuple((x + y) & MASK for x, y in zip(h, (a, b, c, d, e, f, g, hh)))


def words_bytes(h) -> bytes:
    return b"".join(x.to_bytes(4, "big") for x in h)


def digest_of_padded(padded: bytes) -> bytes:
    """SHA-256 of a message already padded to whole blocks"""
    assert len(padded) % 64 == 0
    h = IV
    for i in range(0, len(padded), 64):
        h = compress(h, padded[i: i + 64])
    return words_bytes(h)


def merkle_parent(left: bytes, right: bytes) -> bytes:
    """the 2-to-1 node function: one compression of left || right from the IV, no padding block"""
    assert len(left) == 32 and len(right) == 32
    return words_bytes(compress(IV, left + right))


def merkle_root(leaf: bytes, siblings, index: int) -> bytes:
    """the root above `leaf` at position `index`: bit l of index = 1 means the current node is the right child at level l"""
    cur = leaf
    for l, sib in enumerate(siblings):
        cur = merkle_parent(sib, cur) if (index >> l) & 1 else merkle_parent(cur, sib)
    return cur


def pad(message: bytes) -> bytes:
    """FIPS 180-4 5.1.1"""
    n = len(message)
    return message + b"\x80" + bytes((55 - n) % 64) + (8 * n).to_bytes(8, "big")
