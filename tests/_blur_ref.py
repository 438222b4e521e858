"""Reference for the Gaussian-blur augmentation tests: Pillow's `ImageFilter.GaussianBlur(radius=sigma)` in numpy integers.

Pillow approximates the Gaussian by three extended box blurs along x and then three along y.  One box radius `fr` is derived from
sigma in float32; everything after that is unsigned 32-bit integer arithmetic with edge replication, rounded to a byte after
every pass.  `plan(sigma)` is that float32 step (the same as data.blur_plan, restated here so that the tests compare two
independent writings), `box_pass` one pass along the last axis, `blur(arr, sigma)` the six passes on an [H, W, C] picture.
csrc/dfd_blur.hip is the same arithmetic on the device.  tests/test_blur_cpu.py pins this file against Pillow byte for byte, which
pins the kernel's arithmetic without a GPU; tests/test_blur_gpu.py compares the kernel with this file.
"""

from __future__ import annotations

import numpy as np

PASSES = 3


def plan(sigma: float) -> tuple[int, int, int]:
    """(r, ww, fw): the whole taps' radius, their 8.24 weight and the weight of the two fractional taps at distance r + 1."""
    f = np.float32
    sigma = f(sigma)
    s2 = f(sigma * sigma) / f(PASSES)
    big = f(np.sqrt(f(f(12.0) * s2) + f(1.0)))
    whole = f(np.floor(f(big - f(1.0)) / f(2.0)))
    num = f(f(f(2) * whole + f(1)) * f(f(whole * f(whole + f(1))) - f(f(3) * s2)))
    den = f(f(6) * f(s2 - f(f(whole + f(1)) * f(whole + f(1)))))
    fr = f(whole + f(num / den))
    r = int(fr)
    ww = int(f(1 << 24) / f(f(2) * fr + f(1)))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def box_pass(a: np.ndarray, r: int, ww: int, fw: int) -> np.ndarray:
    """One extended box blur along the last axis of a uint8 array, edges replicated."""
    n = a.shape[-1]
    wide = a.astype(np.uint64)
    x = np.arange(n)
    acc = np.zeros(a.shape, dtype=np.uint64)
    for d in range(-r, r + 1):
        acc += wide[..., np.clip(x + d, 0, n - 1)]
    edge = wide[..., np.clip(x - r - 1, 0, n - 1)] + wide[..., np.clip(x + r + 1, 0, n - 1)]
    total = acc * np.uint64(ww) + edge * np.uint64(fw) + np.uint64(1 << 23)
    assert int(total.max(initial=0)) < 1 << 32
    return (total >> np.uint64(24)).astype(np.uint8)


def blur_planned(arr: np.ndarray, r: int, ww: int, fw: int) -> np.ndarray:
    """The six passes on a uint8 [H, W, C] picture with the constants given."""
    a = np.ascontiguousarray(arr.transpose(2, 0, 1))            # [C, H, W]: x is the last axis
    for _ in range(PASSES):
        a = box_pass(a, r, ww, fw)
    a = np.ascontiguousarray(a.transpose(0, 2, 1))              # [C, W, H]: y is the last axis
    for _ in range(PASSES):
        a = box_pass(a, r, ww, fw)
    return np.ascontiguousarray(a.transpose(2, 1, 0))


def blur(arr: np.ndarray, sigma: float) -> np.ndarray:
    return blur_planned(arr, *plan(sigma))
