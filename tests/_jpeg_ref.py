"""Reference for the JPEG-compression augmentation tests: the pixels of a baseline JPEG round trip in numpy.

`roundtrip(arr, quality)` restates, in signed 32-bit integer arithmetic, what `Image.save(buf, "JPEG", quality=q)` followed by
`Image.open(buf)` does to an RGB picture once the lossless entropy coding is left out (libjpeg's defaults as Pillow uses them:
4:2:0 chroma, the Annex K tables with baseline clamping, the "islow" integer DCT both ways, the "fancy" triangle upsampling).
csrc/dfd_jpeg.hip is the same arithmetic on the device.  tests/test_jpeg_cpu.py pins this file against Pillow byte for byte,
which pins the kernel's arithmetic without a GPU; tests/test_jpeg_gpu.py compares the kernel with this file.

Pictures narrower than 5 pixels are outside it: libjpeg upsamples a chroma plane of width 1 or 2 by plain replication.
"""

from __future__ import annotations

import io

import numpy as np
from PIL import Image

LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
        72, 92, 95, 98, 112, 100, 103, 99)
CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32

F0298, F0390, F0541, F0765, F0899, F1175 = 2446, 3196, 4433, 6270, 7373, 9633
F1501, F1847, F1961, F2053, F2562, F3072 = 12299, 15137, 16069, 16819, 20995, 25172
CONST_BITS, PASS1_BITS = 13, 2


def fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def quant_table(base, quality: int) -> np.ndarray:
    """int32 [8, 8]: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    t = (np.asarray(base, dtype=np.int64) * scale + 50) // 100
    return np.clip(t, 1, 255).astype(np.int32).reshape(8, 8)


def descale(x: np.ndarray, n: int) -> np.ndarray:
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d: np.ndarray, first: bool) -> np.ndarray:
    """jfdctint's one-dimensional pass over the LAST axis (8 long) of an int32 array."""
    x = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = x[0] + x[7], x[0] - x[7], x[1] + x[6], x[1] - x[6]
    t2, t5, t3, t4 = x[2] + x[5], x[2] - x[5], x[3] + x[4], x[3] - x[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        out[0], out[4] = descale(t10 + t11, PASS1_BITS), descale(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * F0541
    out[2] = descale(z1 + t13 * F0765, n)
    out[6] = descale(z1 + t12 * (-F1847), n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F1175
    t4, t5, t6, t7 = t4 * F0298, t5 * F2053, t6 * F3072, t7 * F1501
    z1, z2, z3, z4 = z1 * (-F0899), z2 * (-F2562), z3 * (-F1961) + z5, z4 * (-F0390) + z5
    out[7], out[5], out[3], out[1] = descale(t4 + z1 + z3, n), descale(t5 + z2 + z4, n), descale(t6 + z2 + z3, n), descale(t7 + z1 + z4, n)
    return np.stack(out, axis=-1).astype(np.int32)


def _idct_pass(d: np.ndarray, n: int) -> np.ndarray:
    """jidctint's one-dimensional pass over the LAST axis, descaled by `n` bits."""
    x = [d[..., k] for k in range(8)]
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * F0541
    t2, t3 = z1 + z3 * (-F1847), z1 + z2 * F0765
    t0, t1 = (x[0] + x[4]) << CONST_BITS, (x[0] - x[4]) << CONST_BITS
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F1175
    t0, t1, t2, t3 = t0 * F0298, t1 * F2053, t2 * F3072, t3 * F1501
    z1, z2, z3, z4 = z1 * (-F0899), z2 * (-F2562), z3 * (-F1961) + z5, z4 * (-F0390) + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    return descale(np.stack(out, axis=-1), n).astype(np.int32)


def code_plane(plane: np.ndarray, table: np.ndarray) -> np.ndarray:
    """A sample plane whose sides are multiples of 8 (int32, 0..255) through forward DCT, quantiser, dequantiser and inverse DCT."""
    h, w = plane.shape
    b = (plane.astype(np.int32) - 128).reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)          # [by, bx, row, col]
    c = _fdct_pass(b, True)                                                                         # rows
    c = _fdct_pass(c.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)                            # columns
    div = table.astype(np.int32) * 8
    k = np.sign(c) * ((np.abs(c) + (div >> 1)) // div)
    c = (k * table).astype(np.int32)
    c = _idct_pass(c.transpose(0, 1, 3, 2), CONST_BITS - PASS1_BITS).transpose(0, 1, 3, 2)          # columns
    c = _idct_pass(c, CONST_BITS + PASS1_BITS + 3)                                                  # rows
    return np.clip(c + 128, 0, 255).transpose(0, 2, 1, 3).reshape(h, w)


def _pad_edge(plane: np.ndarray, h: int, w: int) -> np.ndarray:
    return np.pad(plane, ((0, h - plane.shape[0]), (0, w - plane.shape[1])), mode="edge")


def _up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def roundtrip(arr: np.ndarray, quality: int) -> np.ndarray:
    """uint8 [H, W, 3] (W >= 5) -> the picture after a baseline JPEG encode at `quality` (1..100) and decode."""
    h, w = arr.shape[:2]
    if w < 5 or not 1 <= quality <= 100:
        raise ValueError("roundtrip: W >= 5 and 1 <= quality <= 100")
    r, g, b = (arr[..., k].astype(np.int32) for k in range(3))
    y = (fix(.299) * r + fix(.587) * g + fix(.114) * b + 32768) >> 16
    cb = (-fix(.16874) * r - fix(.33126) * g + fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (fix(.5) * r - fix(.41869) * g - fix(.08131) * b + (128 << 16) + 32767) >> 16
    tl, tc = quant_table(LUMA, quality), quant_table(CHROMA, quality)

    y2 = code_plane(_pad_edge(y, _up(h, 8), _up(w, 8)), tl)[:h, :w]
    ch, cw = (h + 1) // 2, (w + 1) // 2
    bias = np.where(np.arange(_up(w, 16) // 2) % 2 == 0, 1, 2).astype(np.int32)
    small = []
    for c in (cb, cr):
        p = _pad_edge(c, _up(h, 2), _up(w, 16))
        d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        d = _pad_edge(d, _up(ch, 8), d.shape[1])                   # the last DOWNSAMPLED row fills the block rows
        small.append(code_plane(d, tc)[:ch, :cw])

    rows = np.arange(h)
    near = rows >> 1
    far = np.clip(np.where(rows % 2 == 0, near - 1, near + 1), 0, ch - 1)
    full = []
    for c in small:
        s = 3 * c[near] + c[far]                                    # [h, cw]
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        up = np.empty((h, 2 * cw), dtype=np.int32)
        up[:, 0::2] = (3 * s + left + 8) >> 4                       # column 0: left is s[0], so (4 * s[0] + 8) >> 4
        up[:, 1::2] = (3 * s + right + 7) >> 4                      # last column: right is s[last]
        full.append(up[:, :w] - 128)
    cb2, cr2 = full
    out = np.stack([y2 + ((fix(1.402) * cr2 + 32768) >> 16),
                    y2 + ((-fix(.34414) * cb2 + 32768 - fix(.71414) * cr2) >> 16),
                    y2 + ((fix(1.772) * cb2 + 32768) >> 16)], axis=-1)
    return np.clip(out, 0, 255).astype(np.uint8)


def device_jpeg(arr: np.ndarray, quality: int, flip: int) -> np.ndarray:
    """One picture as dfd_jpeg_u8 treats it: mirrored in x first when `flip`, copied through at quality 0."""
    src = arr[:, ::-1] if flip else arr
    return src.copy() if quality == 0 else roundtrip(np.ascontiguousarray(src), quality)


def pil_roundtrip(arr: np.ndarray, quality: int) -> np.ndarray:
    buf = io.BytesIO()
    Image.fromarray(arr, "RGB").save(buf, "JPEG", quality=quality)
    buf.seek(0)
    return np.array(Image.open(buf).convert("RGB"), dtype=np.uint8)


def pictures(h: int, w: int, rng) -> dict[str, np.ndarray]:
    """Noise, smoothed noise, 0/255 binary noise, a constant picture, and one whose only detail is its last row and column."""
    noise = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    f = np.pad(noise.astype(np.float32), ((1, 1), (1, 1), (0, 0)), mode="edge")
    smooth = sum(f[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0
    edge = np.full((h, w, 3), 128, dtype=np.uint8)
    edge[-1] = rng.integers(0, 256, (w, 3), dtype=np.uint8)
    edge[:, -1] = rng.integers(0, 256, (h, 3), dtype=np.uint8)
    return {"noise": noise, "smooth": smooth.astype(np.uint8), "binary": (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255),
            "constant": np.full((h, w, 3), 93, dtype=np.uint8), "edge": edge}
