"""CPU: the host half of ctvae_amd/imagegrid.py (the PNG writer) and the self-checks of the restatement the GPU tests compare
against (tests/grid_checks.py)."""
import struct
import zlib

import numpy as np
import pytest
import torch

from tests import grid_checks as G


def _stream(h, w, seed=3):
    rows = np.random.default_rng(seed).integers(0, 256, size=(h, 1 + 3 * w), dtype=np.uint8)
    rows[:, 0] = 0
    return rows


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (134, 794)])
def test_png_writer_round_trips(h, w, tmp_path):
    from ctvae_amd import imagegrid
    rows = _stream(h, w)
    data = imagegrid.png_bytes(rows.tobytes(), w, h)
    img, kinds = G.read_png(data)                         # signature, chunk CRCs, filter bytes
    assert kinds == ["IHDR", "IDAT", "IEND"]
    assert np.array_equal(img, rows[:, 1:].reshape(h, w, 3))
    try:                                                  # an independent decoder, where there is one
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        p = tmp_path / "a.png"
        p.write_bytes(data)
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), img)


def test_png_header_fields_and_crcs():
    from ctvae_amd import imagegrid
    rows = _stream(6, 11)
    data = imagegrid.png_bytes(rows.tobytes(), 11, 6)
    assert data[:8] == bytes([137, 80, 78, 71, 13, 10, 26, 10])
    assert struct.unpack(">I", data[8:12])[0] == 13 and data[12:16] == b"IHDR"
    assert struct.unpack(">IIBBBBB", data[16:29]) == (11, 6, 8, 2, 0, 0, 0)     # width, height, 8 bit, RGB, deflate, filter 0, no interlace
    assert struct.unpack(">I", data[29:33])[0] == zlib.crc32(data[12:29])
    assert data[-12:] == b"\x00\x00\x00\x00IEND\xaeB`\x82"                       # the fixed IEND chunk
    broken = bytearray(data)
    broken[45] ^= 1                                                             # inside IDAT: its CRC no longer holds
    with pytest.raises(AssertionError, match="CRC"):
        G.read_png(bytes(broken))
    with pytest.raises(ValueError, match="scanlines"):
        imagegrid.png_bytes(rows.tobytes()[:-1], 11, 6)


@pytest.mark.parametrize("n,want", [(1, (1, 1, 12, 13)), (12, (12, 1, 12, 134)), (13, (12, 2, 22, 134))])
def test_restatement_geometry_and_last_image(n, want):
    """8 x 9 images, nrow 12, padding 2, white padding, image k flat at byte k + 1: Hg / Wg, where the last image sits, what surrounds it."""
    from ctvae_amd import imagegrid
    H, W, pad = 8, 9, 2
    assert G.geometry(n, H, W, 12, pad) == want == imagegrid.grid_geometry(n, H, W, 12, pad)
    xmaps, ymaps, Hg, Wg = want
    x = np.empty((n, 3, H, W), dtype=np.float32)
    for k in range(n):
        x[k] = (k + 1 + 0.25) / 255.0
    flat = G.ref_grid_bytes(x, nrow=12, padding=pad, pad_value=1.0)
    assert flat.shape == (Hg, 3 * Wg)
    g = flat.reshape(Hg, Wg, 3)
    k = n - 1
    r0, c0 = (k // xmaps) * (H + pad) + pad, (k % xmaps) * (W + pad) + pad
    assert (g[r0:r0 + H, c0:c0 + W] == n).all()
    assert (g[r0 - 1, :] == 255).all() and (g[:, c0 - 1] == 255).all() and (g[r0 + H:, :] == 255).all()
    assert (g[r0:, c0 + W:] == 255).all()                                    # the border and every empty cell after it
    assert int((g != 255).sum()) == n * H * W * 3
    scan = G.ref_grid_bytes(x, nrow=12, padding=pad, pad_value=1.0, scanlines=True)
    assert scan.shape == (Hg, 1 + 3 * Wg) and (scan[:, 0] == 0).all() and np.array_equal(scan[:, 1:], flat)


def test_restatement_arithmetic():
    x = G.grid_inputs(5, (3, 1, 4, 5))
    b = G.ref_grid_bytes(x, nrow=8, padding=0, normalize=True).reshape(4, 3, 5, 3)
    assert b.min() == 0 and b.max() == 255                                      # the pinned elements
    assert (b[..., 0] == b[..., 1]).all() and (b[..., 0] == b[..., 2]).all()    # one channel, replicated
    want = np.floor((x.astype(np.float64) + 1.25) / 3.75 * 255 + 0.5).clip(0, 255)
    assert np.array_equal(b[..., 0].transpose(1, 0, 2), want[:, 0].astype(np.uint8))
    with pytest.raises(AssertionError, match="rounding boundary"):
        G.ref_grid_bytes(np.full((1, 1, 2, 2), 0.5 / 255.0, dtype=np.float32))   # v*255 + 0.5 = 1.0
    y = np.array([[[[np.nan, np.inf, -np.inf, 0.301, 7.01]]]], dtype=np.float32)
    assert G.ref_grid_bytes(y, padding=0).reshape(5, 3)[:, 0].tolist() == [0, 255, 0, 77, 255]
    assert G.ref_grid_bytes(y, padding=0, normalize=True, value_range=(0.0, 10.0)).reshape(5, 3)[:, 0].tolist() == [0, 255, 0, 8, 179]


def test_grids_have_no_cpu_path():
    from ctvae_amd import imagegrid
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imagegrid.make_grid_u8(torch.zeros(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        imagegrid.save_image(torch.zeros(2, 3, 4, 4), "never_written.png")
