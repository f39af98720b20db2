"""Shift search on place descriptors and the pose guess from a shift (include/dvo_amd.h: dvo_tracker_place_shifts,
dvo_tracker_place_guess), restated in numpy.  The search is integer arithmetic, so the device's records are compared with these for
equality; the guess is a few dozen double operations.

Also here, because the CPU file asserts their properties on this reference and the GPU file feeds them to the device: the constructed
mono8 frames whose SAD tables have ties (tie_frames)."""
import numpy as np

import frame_reference as fr
import places_reference as pr

FIELDS = ("dy", "dx", "sad", "sad_zero", "sad_second", "area")
NONE = 0xFFFFFFFF
MAX_RADIUS = 8


def view2d(desc, rows, cols):
    """the (rows, cols) image of an unpadded descriptor: b(y, x) = byte x * rows + y"""
    d = np.asarray(desc, np.uint8).ravel()
    assert d.size == rows * cols
    return d.reshape(cols, rows).T


def sad_table(key, query, rows, cols, radius):
    """(2 r + 1, 2 r + 1) int64: table[dy + r, dx + r] = sum over the window of |k(y, x) - q(y + dy, x + dx)|"""
    r = radius
    assert 0 <= r and rows - 2 * r >= 1 and cols - 2 * r >= 1
    k = view2d(key, rows, cols).astype(np.int64)[r:rows - r, r:cols - r]
    q = view2d(query, rows, cols).astype(np.int64)
    t = np.zeros((2 * r + 1, 2 * r + 1), np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            t[dy + r, dx + r] = np.abs(k - q[r + dy:rows - r + dy, r + dx:cols - r + dx]).sum()
    return t


def record_of_table(t, rows, cols):
    """the record of a SAD table, and the number of shifts that share the smallest SAD"""
    r = t.shape[0] // 2
    order = sorted((int(t[dy + r, dx + r]), abs(dy) + abs(dx), dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    sad, _, by, bx = order[0]
    far = [s for s, _, dy, dx in order if max(abs(dy - by), abs(dx - bx)) >= 2]
    rec = dict(dy=by, dx=bx, sad=sad, sad_zero=int(t[r, r]), sad_second=min(far) if far else NONE, area=(rows - 2 * r) * (cols - 2 * r))
    return rec, int((t == sad).sum())


def record(key, query, rows, cols, radius):
    return record_of_table(sad_table(key, query, rows, cols, radius), rows, cols)[0]


def guess(K, level, first_shift, dy, dx):
    """(R0, t0): the smallest rotation with R0 d = e3 for the ray d of the level's pixel (cx_L + dx, cy_L + dy); K as float32"""
    sc = 2.0 ** -(first_shift + level)
    fx, fy = float(np.float32(K[0])) * sc, float(np.float32(K[1])) * sc
    a = np.array([dx / fx, dy / fy, 1.0])
    d = a / np.sqrt(a @ a)
    V = np.array([[0.0, 0.0, -d[0]], [0.0, 0.0, -d[1]], [d[0], d[1], 0.0]])      # [v]x of v = d x e3 = (d_y, -d_x, 0)
    return np.eye(3) + V + (V @ V) / (1.0 + d[2]), np.zeros(3)


def level_descriptor(image, level_shift):
    """the descriptor of a camera image (BGR8 or mono8) at decimation 2^level_shift, from the numpy restatement of the frame stage"""
    img = fr.resize_nn(np.asarray(image), level_shift)
    grey = fr.bgr2gray(img) if img.ndim == 3 else img
    return pr.descriptor(pr.column_major(grey))


def tie_frames(rows, cols, level_shift):
    """name -> (key image, query image, radius, expected (dy, dx)): mono8 camera frames of rows x cols whose level at decimation
    2^level_shift (pixel (i, j) of the level is pixel (i << s, j << s) of the frame) has a SAD table with more than one minimum, one for
    each tier of the order (SAD, |dy| + |dx|, dy, dx) below the first.  `flat`: against a query of one grey value every SAD is the same
    number (the key is not flat too: an image without an edge cannot become a key frame)"""
    s = level_shift
    y, x = np.meshgrid(np.arange(rows) >> s, np.arange(cols) >> s, indexing="ij")
    u8 = lambda a: a.astype(np.uint8)      # noqa: E731
    flat = np.full((rows, cols), 77, np.uint8)
    stripes = u8(90 + 40 * (x & 1) + y)                                 # period 2 across, a ramp down: dx in {-2, 0, 2} tie at 0
    bars, bars_next = u8(60 + 40 * (y & 1) + x), u8(60 + 40 * ((y + 1) & 1) + x)      # the query is the key moved by one row, up or down
    return dict(flat=(bars, flat, 3, (0, 0)),
                stripes=(stripes, stripes, 2, (0, 0)),
                rows_tie=(bars, bars_next, 1, (-1, 0)),
                cols_tie=(u8(60 + 40 * (x & 1) + y), u8(60 + 40 * ((x + 1) & 1) + y), 1, (0, -1)))      # rows_tie transposed
