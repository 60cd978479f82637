"""Shared by the image-grid tests (no GPU): a float64 numpy restatement of the arithmetic of csrc/imggrid.hip (make_grid +
save_image's byte conversion, include/ctvae_hip.h), a minimal PNG reader, and a seeded input builder whose values keep the
byte conversion away from every rounding boundary -- so that the comparison with the kernel's float32 result is EXACT byte
equality over the whole output, padding and empty cells included."""
import struct
import zlib

import numpy as np

MARGIN = 0.05          # least distance of v*255 + 0.5 from an integer (float64) that ref_grid_bytes accepts


def geometry(n, h, w, nrow, padding):
    xmaps = min(nrow, n)
    ymaps = (n + xmaps - 1) // xmaps
    return xmaps, ymaps, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def _to_byte(t):
    """(uint8) clamp(t, 0, 255) with NaN -> 0 (truncation)."""
    t = np.where(np.isnan(t), 0.0, t)
    return np.floor(np.clip(t, 0.0, 255.0)).astype(np.uint8)


def ref_grid_bytes(x, nrow=8, padding=2, normalize=False, value_range=None, pad_value=0.0, scanlines=False, margin=MARGIN):
    """x [N,C,H,W] float32 (C = 1 or 3) -> uint8 [Hg, 3*Wg] or, with scanlines, [Hg, 1 + 3*Wg] (a zero first in every row).
    Asserts that no finite element's v*255 + 0.5 inside (-1, 256) lies within `margin` of an integer: float32 evaluation order,
    a fused multiply-add or a reciprocal instead of a division then cannot move a byte."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4 and x.shape[1] in (1, 3)
    N, C, H, W = x.shape
    v = x.astype(np.float64)
    if normalize:
        if value_range is not None:
            lo, hi = float(np.float32(value_range[0])), float(np.float32(value_range[1]))
        else:
            lo, hi = float(np.nanmin(v)), float(np.nanmax(v))          # NaN does not enter the range
        v = np.where(np.isnan(v), lo, np.clip(v, lo, hi))              # ... and lands on lo: byte 0
        with np.errstate(invalid="ignore"):                            # an infinite range: inf / inf = NaN -> byte 0
            v = (v - lo) / max(hi - lo, 1e-5)
    t = v * 255.0 + 0.5
    live = np.isfinite(t) & (t > -1.0) & (t < 256.0)
    dist = np.abs(t[live] - np.round(t[live]))
    assert dist.size == 0 or dist.min() >= margin, f"an input sits {dist.min():.3g} from a rounding boundary"
    img = _to_byte(t)
    if C == 1:
        img = np.repeat(img, 3, axis=1)
    xmaps, ymaps, Hg, Wg = geometry(N, H, W, nrow, padding)
    grid = np.full((Hg, Wg, 3), _to_byte(np.float64(np.float32(pad_value)) * 255.0 + 0.5), dtype=np.uint8)
    for k in range(N):
        r0, c0 = (k // xmaps) * (H + padding) + padding, (k % xmaps) * (W + padding) + padding
        grid[r0:r0 + H, c0:c0 + W, :] = img[k].transpose(1, 2, 0)
    flat = grid.reshape(Hg, 3 * Wg)
    if scanlines:
        flat = np.concatenate([np.zeros((Hg, 1), dtype=np.uint8), flat], axis=1)
    return flat


def grid_inputs(seed, shape, lo=-1.25, hi=2.5, kmin=0, kmax=256, pin=True):
    """float32 [N,C,H,W]: every element aims at a byte k in [kmin, kmax) with an offset f in [0.1, 0.9] inside it:
    x = lo + (k + f - 0.5) / 255 * (hi - lo), i.e. (x - lo) / (hi - lo) * 255 + 0.5 = k + f.  pin: all values lie inside
    [lo, hi] (f >= 0.55 at k = 0, f <= 0.45 at k = 255) and exactly one element is lo, one is hi -- the batch's range."""
    rng = np.random.default_rng(seed)
    k = rng.integers(kmin, kmax, size=shape).astype(np.float64)
    f = rng.uniform(0.1, 0.9, size=shape)
    if pin:
        assert kmin == 0 and kmax == 256
        f = np.where(k == 0, rng.uniform(0.55, 0.9, size=shape), f)
        f = np.where(k == 255, rng.uniform(0.1, 0.45, size=shape), f)
    x = lo + (k + f - 0.5) / 255.0 * (hi - lo)
    if pin:
        a, b = rng.choice(x.size, size=2, replace=False)
        x.reshape(-1)[a], x.reshape(-1)[b] = lo, hi
    x = x.astype(np.float32)
    if pin:
        assert (x == np.float32(lo)).sum() == 1 and (x == np.float32(hi)).sum() == 1 and x.min() == np.float32(lo) and x.max() == np.float32(hi)
    return x


def read_png(data: bytes):
    """8-bit RGB, non-interlaced, filter-0 PNG -> (uint8 [H,W,3], [chunk types]).  Checks the signature and every chunk's CRC."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "PNG signature"
    pos, kinds, idat, ihdr = 8, [], b"", None
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(kind + body) & 0xffffffff), f"CRC of {kind!r}"
        kinds.append(kind.decode())
        if kind == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert pos == len(data) and kinds[0] == "IHDR" and kinds[-1] == "IEND"
    w, h, depth, colour, comp, filt, interlace = ihdr
    assert (depth, colour, comp, filt, interlace) == (8, 2, 0, 0, 0), ihdr
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 0).all(), "every scanline has filter type 0"
    return rows[:, 1:].reshape(h, w, 3).copy(), kinds
