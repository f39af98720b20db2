"""The definition of the ignore masks' keep planes (include/dvo_amd.h, "ignore masks"), restated in numpy from the text of the
definition -- dense index arrays, one cumulative sum for the footprints, one shifted OR per offset for the dilation; nothing of
the C++ builder's loops.

A mask is (rows, cols), non-zero = ignore.  Level l (s = first_shift + l) is rows_l x cols_l (level_size: cvRound, half to even).
Level pixel (y, x) stands for camera pixels Y in [y 2^s, (y+1) 2^s), X in [x 2^s, (x+1) 2^s) clipped to the image; an empty range is
the clamped pixel rows - 1 / cols - 1.  drop0 = any mask byte of the footprint; drop = any drop0 within `margin` level pixels
(Chebyshev) inside the level; keep = 0 where drop, else 255.

TEST INFRASTRUCTURE ONLY.  All planes are (rows_l, cols_l) arrays (the library stores them column-major)."""
import numpy as np

MAX_MARGIN = 8
MAX_LEVELS = 8


def level_size(n, shift):
    """cvRound(n * 2^-shift), half to even, in exact integers"""
    q, r = divmod(n, 1 << shift)
    twice = 2 * r
    return q + (1 if (twice > (1 << shift) or (twice == (1 << shift) and q % 2 == 1)) else 0)


def footprint_ranges(n, n_level, shift):
    """lo, hi (exclusive) of the camera pixels along one axis of length n for each of the n_level level coordinates"""
    v = np.arange(n_level, dtype=np.int64)
    lo, hi = v << shift, np.minimum((v + 1) << shift, n)
    empty = lo >= n
    return np.where(empty, n - 1, lo), np.where(empty, n, hi)


def drop0_plane(mask, shift):
    m = (np.asarray(mask) != 0).astype(np.int64)
    rows, cols = m.shape
    R, C = level_size(rows, shift), level_size(cols, shift)
    y0, y1 = footprint_ranges(rows, R, shift)
    x0, x1 = footprint_ranges(cols, C, shift)
    S = np.zeros((rows + 1, cols + 1), np.int64)             # summed-area table: S[a, b] = sum of m[:a, :b]
    S[1:, 1:] = m.cumsum(0).cumsum(1)
    count = S[y1][:, x1] - S[y0][:, x1] - S[y1][:, x0] + S[y0][:, x0]
    return count > 0


def dilate(drop0, margin):
    R, C = drop0.shape
    out = np.zeros((R, C), bool)
    padded = np.zeros((R + 2 * margin, C + 2 * margin), bool)
    padded[margin:margin + R, margin:margin + C] = drop0
    for dy in range(2 * margin + 1):
        for dx in range(2 * margin + 1):
            out |= padded[dy:dy + R, dx:dx + C]
    return out


def keep_levels(mask, n_levels, first_shift, margin):
    """list over levels of (rows_l, cols_l) uint8 planes: 0 dropped, 255 kept"""
    return [np.where(dilate(drop0_plane(mask, first_shift + l), margin), 0, 255).astype(np.uint8) for l in range(n_levels)]


def scene_mask(rows, cols, seed=0):
    """the masks of the GPU tests: a rectangle over the lower third plus one interior blob (a disc), placed by the seed"""
    rng = np.random.default_rng(1000 + seed)
    i, j = np.mgrid[0:rows, 0:cols]
    m = i >= rows - rows // 3
    cy, cx = rng.integers(rows // 6, rows // 2), rng.integers(cols // 5, cols - cols // 5)
    rad = max(3, min(rows, cols) // 8)
    m |= (i - cy) ** 2 + (j - cx) ** 2 <= rad * rad
    return m.astype(np.uint8) * 255
