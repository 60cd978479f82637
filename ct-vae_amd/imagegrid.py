"""Image grids and PNG files without torchvision or Pillow: ``make_grid_u8`` / ``save_image`` over csrc/imggrid.hip.

``torchvision.utils.save_image(x, path, normalize=True, nrow=12)`` -- what the reference's ``sample_images`` calls
(experiment.py:114-150) -- is ``make_grid`` (tile the batch, ``padding`` pixels of ``pad_value`` around every image, optionally
scale the whole batch from [min, max] or ``value_range`` to [0, 1]) followed by ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)``
and an image encoder.  Here the tiling, the scaling and the byte conversion are ONE kernel pass over the batch where it lies
(channels_last decoder outputs and contiguous batches alike, no ``.contiguous()`` copy), which leaves the bytes already laid out
as the scanlines of a PNG; the host side is one device -> host copy, ``zlib.compress`` and four chunks.

The arithmetic is restated from torchvision's published source, not compared against it (the package is absent).  Known
differences: a batch of ONE image is framed by the padding like any other (``make_grid`` returns it bare); NaN does not enter the
batch's minimum / maximum and is written as byte 0 (torch propagates it and blanks the picture); only float32 batches of 1 or 3
channels.  ``scale_each=True`` (every image scaled by its own minimum / maximum, what a rollout sheet needs: rollout.py) is a
second entry point with the same two passes, segmented by image, and is unpinned against torchvision in the same way.
There is no CPU path: a tensor that is not on the GPU is an error.
"""
import struct
import zlib

import torch

from . import native

PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def grid_geometry(n: int, h: int, w: int, nrow: int = 8, padding: int = 2):
    """(xmaps, ymaps, Hg, Wg) of a grid of n images of h x w pixels."""
    xmaps = min(int(nrow), int(n))
    ymaps = -(-int(n) // xmaps)
    return xmaps, ymaps, ymaps * (h + padding) + padding, xmaps * (w + padding) + padding


def _as_batch(x: torch.Tensor) -> torch.Tensor:
    if not torch.is_tensor(x):
        raise TypeError("make_grid_u8 takes one tensor [N,C,H,W]")
    if not x.is_cuda:
        raise RuntimeError("make_grid_u8 runs on the GPU only: there is no CPU fallback")
    if x.dim() != 4 or x.size(1) not in (1, 3):
        raise ValueError(f"make_grid_u8 takes [N,C,H,W] with C = 1 or 3, got {tuple(x.shape)}")
    return x.detach() if x.dtype == torch.float32 else x.detach().float()


def make_grid_u8(x: torch.Tensor, nrow: int = 8, padding: int = 2, normalize: bool = False, value_range=None,
                 pad_value: float = 0.0, scanlines: bool = False, *, scale_each: bool = False,
                 out: torch.Tensor = None) -> torch.Tensor:
    """The grid of batch x as bytes on x's device: [Hg, Wg, 3], or with ``scanlines`` [Hg, 1 + 3*Wg] (a zero in front of every
    row: PNG filter type 0).  Defaults are torchvision's.  ``scale_each``: with ``normalize`` and no ``value_range`` every image
    is scaled by its own minimum and maximum instead of the batch's (otherwise it changes nothing).  ``out``: a flat uint8 buffer
    to write into (16-byte aligned, the stream's length rounded up to a multiple of 4 at least); the result is a view of it."""
    with torch.no_grad():
        x = _as_batch(x)
        N, C, H, W = x.shape
        _, _, Hg, Wg = grid_geometry(N, H, W, nrow, padding) if nrow >= 1 else (0, 0, 0, 0)
        pitch = (1 if scanlines else 0) + 3 * Wg
        total = max(Hg * pitch, 0)
        if out is None:
            out = torch.empty((total + 3) // 4 * 4, dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or out.device != x.device or out.dim() != 1 or not out.is_contiguous():
            raise ValueError("out must be a flat contiguous uint8 tensor on the batch's device")
        has_range = value_range is not None
        lo, hi = (float(value_range[0]), float(value_range[1])) if has_range else (0.0, 1.0)
        entry = "ctvae_image_grid_each_u8" if (scale_each and normalize and not has_range) else "ctvae_image_grid_u8"
        with torch.cuda.device(x.device):
            ws = native.workspace(x.device)
            native.call(entry, x.data_ptr(), x.stride(0), x.stride(1), x.stride(2), x.stride(3), N, C, H, W,
                        int(nrow), int(padding), int(bool(normalize)), int(has_range), lo, hi, float(pad_value), int(bool(scanlines)),
                        out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel() * 4)
        return out[:total].view(Hg, pitch) if scanlines else out[:total].view(Hg, Wg, 3)


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def png_bytes(scanline_stream: bytes, width: int, height: int) -> bytes:
    """An 8-bit RGB PNG from ``height`` scanlines of 1 + 3*width bytes (filter type 0 first): signature, IHDR, one IDAT, IEND."""
    if len(scanline_stream) != height * (1 + 3 * width):
        raise ValueError(f"{len(scanline_stream)} bytes are not {height} scanlines of 1 + 3*{width}")
    ihdr = struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0)       # bit depth 8, colour type 2 (RGB), deflate, filter 0, no interlace
    return PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(scanline_stream)) + _chunk(b"IEND", b"")


def save_image(x: torch.Tensor, path, nrow: int = 8, padding: int = 2, normalize: bool = False, value_range=None,
               pad_value: float = 0.0, scale_each: bool = False) -> None:
    """``torchvision.utils.save_image`` for PNG files: the grid's scanlines come from the GPU in one copy."""
    grid = make_grid_u8(x, nrow=nrow, padding=padding, normalize=normalize, value_range=value_range, pad_value=pad_value,
                        scanlines=True, scale_each=scale_each)
    height, pitch = grid.shape
    data = png_bytes(grid.cpu().numpy().tobytes(), (pitch - 1) // 3, height)
    with open(path, "wb") as f:
        f.write(data)
