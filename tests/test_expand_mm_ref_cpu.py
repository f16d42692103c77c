"""CPU: the layout reference of the matrix-core CRS image (tests/expand_mm_ref.py) is consistent with itself and with the constants the suite already holds.

* the byte classes of every region shape tests/test_gpu_expand_mm.py runs are counted and equal their closed forms (data = nrows (n + 1) 88 | 184: the masks can hide no
  more than that allows), and the figures of the 256-row regions are the ones written down for them;
* image_ref inverts: every row's significant bytes are read back out of the image through the index formula alone (expand_mm_ref.read_row, element by element);
* single bytes, addressed by hand;
* the tile that holds b's last bytes is the one test_gpu_evalmm.py::test_expansion_kernels_write_the_same_image masks by: row tile 8090, positions 0..7, at n = 1470, logq 736.
"""
import numpy as np
import pytest

import expand_mm_ref as xr
from c_lwe_snarks_amd import Params

ROWS = (1, 21, 64, 85, 107, 256, 320, 321)  # the regions and shares of (d, m) = (256, 64) and (320, 321) at world 1, 3 and 256


def _region(p, nrows, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=nrows * p.n * p.ctb, dtype=np.uint8), rng.integers(0, 256, size=nrows * p.ctb, dtype=np.uint8)


@pytest.mark.parametrize("logq", [736, 1472])
@pytest.mark.parametrize("nrows", ROWS)
def test_class_counts_equal_their_closed_forms_and_the_image_inverts(logq, nrows):
    p = Params(logq=logq, d=nrows, m=1)
    ks, c8 = _region(p, nrows, nrows + logq)
    image, cls = xr.image_ref(p, ks, c8, nrows)
    sig, stride, mtiles = xr.geometry(p)
    KS, written = xr.ksteps(nrows)
    assert image.shape == cls.shape == (mtiles, KS, 4, 16, 16)
    assert mtiles == (8096 if logq == 736 else 17652) and KS == (nrows + 255) // 256 * 4
    got = np.bincount(cls.reshape(-1), minlength=4)
    want = xr.class_counts(p, nrows)
    assert [int(x) for x in got] == [want[k] for k in (xr.DATA, xr.PAD, xr.SPILL, xr.UNWRITTEN)]
    assert want[xr.DATA] == nrows * 1471 * (88 if logq == 736 else 184)
    assert sum(want.values()) == image.size == mtiles * KS * 1024
    # whole k-steps are written or not: rows >= 64 * written are UNWRITTEN in every tile, rows in [nrows, 64 * written) SPILL in every tile
    assert (cls[:, written:] == xr.UNWRITTEN).all() and not (cls[:, :written] == xr.UNWRITTEN).any()
    assert (image[cls == xr.PAD] == 0x80).all()
    # inversion: the first and last row of every 16-row group and k-step that exists, and a few inside
    sigrows = xr.significant_rows(p, ks, c8, nrows)
    for row in sorted({r for r in (0, 1, 7, 15, 16, 31, 47, 48, 63, 64, 84, 106, 127, 128, 255, 256, 257, 319, 320, nrows - 1) if r < nrows}):
        assert np.array_equal(xr.read_row(p, image, row), sigrows[row]), row


def test_the_256_row_figures():
    for logq, data, total in ((736, 33_138_688, 33_161_216), (1472, 69_289_984, 72_302_592)):
        p = Params(logq=logq, d=256, m=64)
        c = xr.class_counts(p, 256)
        assert c[xr.DATA] == data and sum(c.values()) == total and c[xr.SPILL] == 0 and c[xr.UNWRITTEN] == 0


@pytest.mark.parametrize("logq", [736, 1472])
def test_single_bytes_by_hand(logq):
    p = Params(logq=logq, d=70, m=1)
    nrows = 70
    ks, c8 = _region(p, nrows, 5)
    image, cls = xr.image_ref(p, ks, c8, nrows)
    flat = image.reshape(-1)
    KS = 4
    stream = ks.reshape(nrows, p.n, p.ctb)
    sig, stride, _ = xr.geometry(p)
    for row, j, k in ((0, 0, 0), (69, 0, 0), (17, 3, 87), (65, 1469, 5), (33, 700, sig - 1), (64, 1, 16)):
        pos = stride * j + k
        P, c16, ksx, lane, e = pos // 16, pos % 16, row // 64, 16 * ((row % 64) // 16) + pos % 16, row % 16
        # header comment of expandmm.hip: image[((P * KS + ks) * 64 + lane) * 16 + e], lane & 15 = byte position, lane >> 4 = row group
        assert flat[((P * KS + ksx) * 64 + lane) * 16 + e] == stream[row, j, k] ^ 0x80
        assert cls.reshape(-1)[((P * KS + ksx) * 64 + lane) * 16 + e] == xr.DATA and c16 == lane & 15
    # the insignificant bytes of a value never appear: at logq 736 position 88 is byte 0 of coordinate 1, not byte 88 of coordinate 0
    if logq == 736:
        assert image[88 // 16, 0, 0, 88 % 16, 0] == stream[0, 1, 0] ^ 0x80
    else:
        assert (cls[11, 0, 0, 8:, 0] == xr.PAD).all() and image[12, 0, 0, 0, 0] == stream[0, 1, 0] ^ 0x80
    # rows 70 .. 127 of k-step 1 spill, k-steps 2 and 3 are unwritten
    assert (cls[:, 1, 0, :, 6:] == xr.SPILL).all() and (cls[:, 1, 0, :, :6] != xr.SPILL).all() and (cls[:, 1, 1:] == xr.SPILL).all()
    assert (cls[:, 2:] == xr.UNWRITTEN).all()


def test_the_tile_of_the_last_bytes_of_b():
    """logq 736, n = 1470: 1471 coordinates x 88 bytes = 129 448 = 16 x 8090 + 8"""
    p = Params(logq=736, d=3, m=1)
    ks, c8 = _region(p, 3, 9)
    c8 = c8.copy()
    c8.reshape(3, 92)[1] = 0x00   # stored as 0x80
    c8.reshape(3, 92)[2] = 0xFF   # stored as 0x7F
    image, cls = xr.image_ref(p, ks, c8, 3)
    last = 11 * ((p.n + 1) // 2) + 5  # (the expression of test_expansion_kernels_write_the_same_image)
    assert last == 8090
    assert (cls[8090, 0, 0, :8, :3] == xr.DATA).all() and (cls[8090, 0, 0, 8:, :3] == xr.PAD).all() and (cls[8091:, 0, 0, :, :3] == xr.PAD).all()
    assert (cls[:8090, 0, 0, :, :3] == xr.DATA).all()
    assert np.array_equal(image[8090, 0, 0, :8, 0], c8.reshape(3, 92)[0, 80:88] ^ 0x80)
    # b occupies positions 88 * 1470 .. + 87 = tile 8085 position 0 .. tile 8090 position 7
    assert 88 * 1470 == 16 * 8085
    assert (image[8085:8090, 0, 0, :, 1] == 0x80).all() and (image[8090, 0, 0, :8, 1] == 0x80).all()
    assert (image[8085:8090, 0, 0, :, 2] == 0x7F).all() and (image[8090, 0, 0, :8, 2] == 0x7F).all()
    assert (image[8090, 0, 0, 8:, :3] == 0x80).all() and (image[8091:, 0, 0, :, :3] == 0x80).all()
