"""The matrix-core CRS image ("MFMA A-fragments"; header comment of csrc/expandmm.hip) stated in numpy, independently of the kernels that write it.

A REGION is nrows consecutive rows of the public stream.  Row i of a region is n keystream values (CT_BYTES = logq / 8 stream bytes each) followed by the b coordinate,
the row's CT_BYTES-byte entry of the compressed CRS.  Only the bytes that survive modq enter the image -- the row's SIGNIFICANT BYTE STREAM:

  logq  736: bytes 0..87 of a coordinate's 92, coordinate j at positions 88 j .. 88 j + 87 (no gaps); 88 (n + 1) positions, the rest of the last row tile(s) is padding;
  logq 1472: all 184 bytes, coordinate j at positions 192 j .. 192 j + 183; positions 192 j + 184 .. 192 j + 191 are padding (11.5 -> 12 row tiles per coordinate).

A ROW TILE is 16 consecutive positions; mtiles = ceil((n + 1) / 2) * 11 (logq 736) or (n + 1) * 12 (1472).  A K-STEP is 64 consecutive rows; the region is padded to
whole 256-row stages, KS = ceil(nrows / 256) * 4 k-steps.  The image is one 1 KiB fragment per (row tile P, k-step ks), P outermost:

  image[P][ks][g4][c16][e] = (position 16 P + c16 of row 64 ks + 16 g4 + e) XOR 0x80          (uint8 [mtiles][KS][4][16][16]; lane = 16 g4 + c16 holds 16 bytes e)

Every byte of the image has one CLASS:
  DATA       a significant byte of a row < nrows: must equal the stream;
  PAD        a padding position of a row < nrows: k_expand_mm stores 0x80 (A = 0) there, k_evalmm16<1> is not held to that;
  SPILL      any position of a row >= nrows inside a k-step the writer touches (k-steps < ceil(nrows / 64)): content is free;
  UNWRITTEN  k-steps ceil(nrows / 64) .. KS - 1: the writer must leave what the buffer held.
No consumer's result may depend on a byte that is not DATA (tests/test_gpu_expand_mm.py, part d)."""
import numpy as np

DATA, PAD, SPILL, UNWRITTEN = 0, 1, 2, 3


def geometry(p):
    """(sig, stride, mtiles): significant bytes of a coordinate, positions from one coordinate to the next, row tiles"""
    if p.logq == 736:
        return 88, 88, (p.n + 2) // 2 * 11
    if p.logq == 1472:
        return 184, 192, (p.n + 1) * 12
    raise ValueError("logq is 736 or 1472")


def ksteps(nrows):
    """(KS, written): k-steps of the region's image, and how many of them hold a row"""
    return (nrows + 255) // 256 * 4, (nrows + 63) // 64


def class_counts(p, nrows):
    """closed forms: bytes of each class in the image of a region of nrows rows"""
    sig, _, mtiles = geometry(p)
    KS, written = ksteps(nrows)
    npos = 16 * mtiles
    return {DATA: nrows * (p.n + 1) * sig, PAD: nrows * (npos - (p.n + 1) * sig), SPILL: (64 * written - nrows) * npos, UNWRITTEN: (KS - written) * 64 * npos}


def significant_rows(p, keystream, c8, nrows):
    """uint8 [nrows][n + 1][sig]: the significant bytes of every row, coordinate by coordinate (keystream coordinates, then b), as the stream has them"""
    sig, _, _ = geometry(p)
    ks = np.frombuffer(keystream, dtype=np.uint8) if isinstance(keystream, (bytes, bytearray, memoryview)) else np.asarray(keystream, dtype=np.uint8)
    b = np.frombuffer(c8, dtype=np.uint8) if isinstance(c8, (bytes, bytearray, memoryview)) else np.asarray(c8, dtype=np.uint8)
    assert ks.size == nrows * p.n * p.ctb and b.size == nrows * p.ctb
    out = np.empty((nrows, p.n + 1, sig), dtype=np.uint8)
    out[:, : p.n] = ks.reshape(nrows, p.n, p.ctb)[:, :, :sig]
    out[:, p.n] = b.reshape(nrows, p.ctb)[:, :sig]
    return out


def image_ref(p, keystream, c8, nrows):
    """(image, classes): both uint8 [mtiles][KS][4 (g4)][16 (c16)][16 (e)].  keystream: the nrows * n * CT_BYTES stream bytes from the region's offset on;
    c8: the nrows compressed ciphertexts.  Bytes of class PAD are 0x80 in `image`, SPILL and UNWRITTEN bytes are 0 (compare them through `classes` only)."""
    sig, stride, mtiles = geometry(p)
    KS, written = ksteps(nrows)
    npos = 16 * mtiles
    rows = np.zeros((64 * KS, npos), dtype=np.uint8)      # [row][position], already offset by 128
    rows[:nrows] = 0x80
    live = np.full((nrows, p.n + 1, stride), 0x80, dtype=np.uint8)  # coordinate by coordinate, then laid along the row
    live[:, :, :sig] = significant_rows(p, keystream, c8, nrows) ^ 0x80
    rows[:nrows, : stride * (p.n + 1)] = live.reshape(nrows, stride * (p.n + 1))
    # [64 ks + 16 g4 + e][16 P + c16] -> [P][ks][g4][c16][e]
    image = np.ascontiguousarray(rows.reshape(KS, 4, 16, mtiles, 16).transpose(3, 0, 1, 4, 2))
    # the classes, from the row and the position alone
    pos = np.arange(npos)
    significant = ((pos % stride < sig) & (pos // stride <= p.n)).reshape(mtiles, 1, 1, 16, 1)
    cls = np.empty(image.shape, dtype=np.uint8)
    cls[...] = np.where(significant, DATA, PAD).astype(np.uint8)
    cls[:, written:] = UNWRITTEN
    if nrows < 64 * written:  # the last k-step that holds a row: local row 16 g4 + e
        local = (16 * np.arange(4)[:, None, None] + np.arange(16)[None, None, :]) >= nrows - 64 * (written - 1)
        np.copyto(cls[:, written - 1], np.uint8(SPILL), where=local[None])
    return image, cls


def read_row(p, image, row):
    """the inverse, for one row: uint8 [n + 1][sig], its significant bytes as the stream has them, read out of the image element by element"""
    sig, stride, _ = geometry(p)
    pos = (stride * np.arange(p.n + 1)[:, None] + np.arange(sig)[None, :])
    return image[pos // 16, row // 64, (row % 64) // 16, pos % 16, row % 16] ^ 0x80
