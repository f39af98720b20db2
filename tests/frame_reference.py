"""An independent plain reference of the camera-frame front end (numpy, int64 / float64, no ctypes): metres -> 16-bit millimetres,
BGR -> grey, nearest-neighbour decimation, and cv::undistort's fixed-point map and remaps.

Written from the DEFINITIONS stated in the header comments of oracle/dvo_oracle_frames.cpp and include/dvo_amd.h, not from either
C++ implementation.  In particular the undistortion map is evaluated in closed form per pixel -- no stripes, no inverted camera
matrix, no running sums -- and the 16-bit remap is evaluated as an exact rational number instead of a float sum, so that what the
engine and the oracle share (one author's loop, one float evaluation order) is checked against something that shares neither.

TEST INFRASTRUCTURE ONLY.  All images are row-major (rows, cols[, 3]) arrays."""
import numpy as np

INT_MIN = -(1 << 31)


def rint_half_even_i64(num, den_log2):
    """round-half-to-even of num / 2^den_log2 for int64 num >= 0; returns (rounded, remainder num mod 2^den_log2)"""
    num = np.asarray(num, np.int64)
    q, r = num >> den_log2, num & ((1 << den_log2) - 1)
    half = 1 << (den_log2 - 1)
    return q + ((r > half) | ((r == half) & ((q & 1) == 1))), r


def cv_round(v):
    """cvRound of OpenCV 2.4 on x86 (cvtsd2si): round half to even; NaN and everything that does not fit an int -> INT_MIN"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        ok = (v > -2147483648.5) & (v < 2147483647.5)
        return np.where(ok, np.rint(np.where(ok, v, 0.0)), float(INT_MIN)).astype(np.int64)


def depth_m_to_mm16(depth_m):
    """1000.0f * depth in float32 -> convertTo(CV_16U) = saturate(cvRound) -> 0 becomes 1.  NaN and |mm| >= 2^31 -> 1"""
    d = np.asarray(depth_m, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        mm = (d * np.float32(1000)).astype(np.float64)                  # the float32 product, held exactly
        out_of_int = ~(np.abs(mm) < 2.0 ** 31)                            # NaN, inf, beyond int
        r = np.rint(np.where(out_of_int, 0.0, mm))                        # half to even
    v = np.clip(r, 0, 65535).astype(np.int64)
    v[out_of_int] = 1
    v[v == 0] = 1
    return v.astype(np.uint16)


def bgr2gray(bgr):
    b = np.asarray(bgr).astype(np.int64)
    return ((1868 * b[..., 0] + 9617 * b[..., 1] + 4899 * b[..., 2] + (1 << 13)) >> 14).astype(np.uint8)


def level_size(n, shift):
    """cv::resize(Size(), 2^-shift): dsize = cvRound(n * 2^-shift), half to even"""
    q, r = n >> shift, n & ((1 << shift) - 1)
    if shift == 0:
        return n
    half = 1 << (shift - 1)
    return q + (1 if (r > half or (r == half and (q & 1))) else 0)


def resize_nn(img, shift):
    """INTER_NEAREST at scale 2^-shift: dst(i, j) = src(min(i << shift, rows-1), min(j << shift, cols-1))"""
    img = np.asarray(img)
    rows, cols = img.shape[:2]
    iy = np.minimum(np.arange(level_size(rows, shift), dtype=np.int64) << shift, rows - 1)
    ix = np.minimum(np.arange(level_size(cols, shift), dtype=np.int64) << shift, cols - 1)
    return img[iy][:, ix]


TIE_EPS = 1e-6


def undistort_map(rows, cols, K4, D5):
    """cv::undistort's CV_16SC2 map in closed form, float64: x = (j-cx)/fx, y = (i-cy)/fy, the radial / tangential model
    u = fx*(x*kr + p1*2xy + p2*(r2 + 2x^2)) + cx (v alike), iu = cvRound(u*32), source pixel (short)(iu >> 5), fraction iu & 31.
    Returns sx, sy (int16), fx5, fy5 (0..31) and the mask of TIE-BAND pixels: u*32 or v*32 within 1e-6 of a half-integer, where
    another derivation of the same real number may legitimately round the other way."""
    fx, fy, cx, cy = (float(k) for k in K4)
    k1, k2, p1, p2, k3 = (float(d) for d in D5)
    i, j = np.mgrid[0:rows, 0:cols].astype(np.float64)
    x, y = (j - cx) / fx, (i - cy) / fy
    r2 = x * x + y * y
    kr = 1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    tu = (fx * (x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)) + cx) * 32.0
    tv = (fy * (y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y) + cy) * 32.0
    iu, iv = cv_round(tu), cv_round(tv)
    band = (np.abs(tu - np.floor(tu) - 0.5) <= TIE_EPS) | (np.abs(tv - np.floor(tv) - 0.5) <= TIE_EPS)
    return (iu >> 5).astype(np.int16), (iv >> 5).astype(np.int16), (iu & 31).astype(np.int64), (iv & 31).astype(np.int64), band


def _taps(src_shape, sx, sy):
    """indices (clipped) and inside masks of the four taps (0,0) (0,1) (1,0) (1,1) = (dy, dx)"""
    rows, cols = src_shape[:2]
    out = []
    for a in (0, 1):
        for b in (0, 1):
            yy, xx = sy.astype(np.int64) + a, sx.astype(np.int64) + b
            inside = (yy >= 0) & (yy < rows) & (xx >= 0) & (xx < cols)
            out.append((np.clip(yy, 0, rows - 1), np.clip(xx, 0, cols - 1), inside))
    return out


def outside_counts(src_shape, sx, sy):
    """per output pixel the number of its four taps that fall outside the source"""
    return sum((~inside).astype(np.int64) for _, _, inside in _taps(src_shape, sx, sy))


def remap_bgr8(src, sx, sy, fx5, fy5):
    """remap INTER_LINEAR, BORDER_CONSTANT 0, 8-bit: integer weights BilinearTab_i = saturate_cast<short>(w * 32768) -- the weights
    are (32-fy | fy) * (32-fx | fx) * 32 exactly, except that 1.0 is stored as 32767 and the missing 1 goes to tap (1,1) --;
    pixel = saturate_cast<uchar>((sum + 2^14) >> 15)"""
    src = np.asarray(src).astype(np.int64)
    wy, wx = (32 - fy5, fy5), (32 - fx5, fx5)
    w = [wy[a] * wx[b] * 32 for a in (0, 1) for b in (0, 1)]
    one = (fx5 == 0) & (fy5 == 0)
    w[0] = np.where(one, 32767, w[0])
    w[3] = np.where(one, 1, w[3])
    acc = np.zeros(sx.shape + src.shape[2:], np.int64)
    for (yy, xx, inside), wk in zip(_taps(src.shape, sx, sy), w):
        v = src[yy, xx] * (inside if src.ndim == 2 else inside[..., None])
        acc += v * (wk if src.ndim == 2 else wk[..., None])
    return np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)


def remap_u16_exact(src, sx, sy, fx5, fy5):
    """remap INTER_LINEAR, BORDER_CONSTANT 0, 16-bit, as the EXACT rational E = sum v_k * wy_k * wx_k / 1024 (weights in 1/32 units,
    border taps 0).  Returns rint_half_even(E), frac(E) and E itself (float64: exact, E * 1024 < 2^26)"""
    src = np.asarray(src).astype(np.int64)
    wy, wx = (32 - fy5, fy5), (32 - fx5, fx5)
    num = np.zeros(sx.shape, np.int64)
    k = 0
    for a in (0, 1):
        for b in (0, 1):
            yy, xx, inside = _taps(src.shape, sx, sy)[k]
            num += src[yy, xx] * inside * wy[a] * wx[b]
            k += 1
    r, rem = rint_half_even_i64(num, 10)
    return r, rem / 1024.0, num / 1024.0


ORDER_MARGIN = 7 * 2.0 ** -8       # seven float roundings (4 products, 3 sums) of at most 2^-8 each above 2^14


def check_remap_u16(got, r, frac, E, where=None):
    """the rule for a float evaluation of the 16-bit remap against the exact value: E < 2^14 -> every product and partial sum is a
    multiple of 2^-10 below 2^24 units, the float sum is exact and the result is rint_half_even(E), ties included; otherwise the
    result may differ from rint(E) by 1, and only where frac(E) is within 7 * 2^-8 of one half.  Returns the counts
    (pixels with E >= 2^14, of those inside the margin, of those differing from rint(E))"""
    got = np.asarray(got).astype(np.int64)
    sel = np.ones(got.shape, bool) if where is None else where
    low = sel & (E < 2 ** 14)
    assert np.array_equal(got[low], r[low]), "16-bit remap below 2^14 must be exact: %d pixels differ" % int((got[low] != r[low]).sum())
    high = sel & ~(E < 2 ** 14)
    margin = high & (np.abs(frac - 0.5) <= ORDER_MARGIN)
    strict = high & ~margin
    assert np.array_equal(got[strict], r[strict]), "16-bit remap outside the rounding margin differs in %d pixels" % int((got[strict] != r[strict]).sum())
    assert np.all(np.abs(got[margin] - r[margin]) <= 1)
    return int(high.sum()), int(margin.sum()), int((got[margin] != r[margin]).sum())


def camera_levels(bgr, depth16, n_levels, first_shift, calib=None):
    """the publisher's pyramid of one frame: (undistort both images,) decimate by 2^(first_shift + l), BGR -> grey.  depth16: the
    16-bit image (after depth_m_to_mm16, or a raw sensor image) or None.  Per level a dict: grey, and with depth r / frac / E of
    remap_u16_exact (without a map: r = the value, frac = 0, E = the value); band = tie-band mask of the pixels kept (all False
    without a map)"""
    rows, cols = bgr.shape[:2]
    band = np.zeros((rows, cols), bool)
    r = frac = E = None
    if calib is not None:
        sx, sy, fx5, fy5, band = undistort_map(rows, cols, *calib)
        bgr = remap_bgr8(bgr, sx, sy, fx5, fy5)
        if depth16 is not None:
            r, frac, E = remap_u16_exact(depth16, sx, sy, fx5, fy5)
    elif depth16 is not None:
        r = np.asarray(depth16).astype(np.int64)
        frac, E = np.zeros(r.shape), r.astype(np.float64)
    out = []
    for l in range(n_levels):
        s = first_shift + l
        lv = dict(grey=bgr2gray(resize_nn(bgr, s)), band=resize_nn(band, s))
        if r is not None:
            lv.update(r=resize_nn(r, s), frac=resize_nn(frac, s), E=resize_nn(E, s))
        out.append(lv)
    return out


# ---- the input domain the tests run: built here once, used by the CPU file (oracle <-> this reference) and the GPU file -------------
def _f32_neighbours(x):
    """the float32 nearest each x (float64) and its +-1, +-2 ulp neighbours"""
    c = np.asarray(x, np.float64).astype(np.float32).view(np.int32).astype(np.int64)
    return np.concatenate([(c + k) for k in (-2, -1, 0, 1, 2)]).astype(np.int32).view(np.float32)


def depth_domain_values(n_random=1 << 21, seed=20240607):
    """every 16-bit millimetre value approached from both sides of its rounding boundaries, the special values, the cvRound range
    boundary, and seeded random bit patterns.  float32 metres, 1-D"""
    k = np.arange(0, 65537, dtype=np.float64)
    parts = [_f32_neighbours(k / 1000.0), _f32_neighbours((k + 0.5) / 1000.0)]
    tiny = np.finfo(np.float32).tiny
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, float(np.finfo(np.float32).max), -float(np.finfo(np.float32).max),
               tiny, -tiny, tiny / 2, -tiny / 2, 1e-45, -1e-45, -1.0, -0.0004, -0.0005, -0.0006, -65.535, -70.0, 65.5354, 65.5355, 70.0, 1e9, -1e9]
    parts.append(np.array(special, np.float32))
    parts.append(np.array([0x7fc00001, 0xffc00000, 0x7f800001, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff], np.uint32).view(np.float32))
    for b in (2.0 ** 31 / 1000.0, -2.0 ** 31 / 1000.0, (2.0 ** 31 - 128) / 1000.0, 2.0 ** 32 / 1000.0, 2.0 ** 63 / 1000.0):
        parts.append(_f32_neighbours(np.array([b])))
    rng = np.random.default_rng(seed)
    parts.append(rng.integers(0, 1 << 32, n_random, dtype=np.uint64).astype(np.uint32).view(np.float32))
    return np.concatenate(parts)


def depth_domain_image(values, rows, cols, seed=7):
    """the values as a rows x cols image (row-major); what is left over is filled with more random bit patterns"""
    assert rows * cols >= values.size
    pad = np.random.default_rng(seed).integers(0, 1 << 32, rows * cols - values.size, dtype=np.uint64).astype(np.uint32).view(np.float32)
    return np.concatenate([values, pad]).reshape(rows, cols)


# undistortion edge cases: name -> (rows, cols, K4, D5).  Chosen so that this reference's tie band stays below 1e-4 of the pixels
# (checked in tests/test_frame_reference_cpu.py) and so that the expectations below hold
CALIBRATIONS = {
    "pincushion": (240, 320, (260.0, 262.0, 159.3, 119.2), (5.0, 1.0, 0.0, 0.0, 0.0)),            # corners and whole tiles outside
    "barrel": (241, 323, (260.0, 262.0, 160.2, 119.1), (-0.45, 0.12, 0.0, 0.0, -0.01)),
    "pp_outside": (200, 264, (300.0, 300.0, -40.25, -30.75), (0.1, -0.02, 0.001, 0.001, 0.0)),     # principal point outside the image
    "tangential": (240, 320, (255.0, 250.0, 161.7, 118.3), (0.02, 0.0, 0.15, -0.12, 0.0)),
    "far": (240, 320, (260.0, 262.0, 159.3, 119.2), (40.0, 20.0, 0.0, 0.0, 0.0)),                 # thousands of pixels beyond the image
    "short_wrap": (240, 320, (260.0, 262.0, 159.3, 119.2), (0.0, 0.0, 0.0, 0.0, 3000.0)),          # beyond 32767 pixels: (short) wraps
    "identity_int": (97, 131, (100.0, 101.0, 65.0, 48.0), (0.0, 0.0, 0.0, 0.0, 0.0)),              # fi == 0 everywhere
    "identity_half": (129, 33, (90.0, 91.0, 16.5, 64.5), (0.0, 0.0, 0.0, 0.0, 0.0)),
    "full_hd": (1080, 1920, (1050.0, 1050.0, 959.5, 539.5), (0.12, -0.25, 0.0012, -0.0009, 0.11)),  # stripes of 2 rows
}
BAND_EMPTY = ("identity_int", "identity_half")
# least share of output pixels with >= 1 tap outside the source / with all four outside
OUTSIDE_SHARE = {"pincushion": (0.5, 0.5), "far": (0.8, 0.8), "short_wrap": (0.3, 0.3), "pp_outside": (0.0, 0.0), "tangential": (0.02, 0.01)}


def edge_frame(rows, cols, seed):
    """BGR8 + depth in metres that reach what generated scenes never do: 0/255 checkerboards (periods 1, 2, 3), depth planes from
    1 to 65 535 mm with sharp steps on both sides of 16 384 mm, holes (0.0, NaN) inside far surfaces"""
    rng = np.random.default_rng(seed)
    i, j = np.mgrid[0:rows, 0:cols]
    bgr = np.stack([(((i // p) + (j // p) + ph) & 1) * 255 for p, ph in ((1, 0), (2, 1), (3, 0))], -1).astype(np.uint8)
    blk = rng.integers(0, 256, (rows // 8 + 1, cols // 8 + 1, 3))[i // 8, j // 8]
    noisy = rng.integers(0, 256, (rows, cols, 3))
    bgr = np.where((i > rows * 2 // 3)[..., None], np.where((j > cols // 2)[..., None], noisy, blk), bgr).astype(np.uint8)
    mm = np.linspace(1, 65535, cols)[None, :].repeat(rows, 0)                                     # a ramp over the whole range
    steps = np.array([1, 65535, 16383, 16385, 32767, 40001, 2, 65534, 20000, 16384, 50001, 1000, 65535, 30003])
    band = (i >= rows // 4) & (i < rows // 2)
    mm = np.where(band, steps[(j // 5) % steps.size], mm)
    far = rng.integers(16384, 65536, (rows // 4 + 1, cols // 4 + 1))[i // 4, j // 4]
    mm = np.where(i >= rows // 2, far + rng.integers(0, 2, (rows, cols)) * 0.5, mm)               # .5: rounding ties of the conversion
    depth = (mm / 1000.0).astype(np.float32)
    holes = rng.random((rows, cols))
    depth[holes < 0.02] = 0.0
    depth[(holes >= 0.02) & (holes < 0.04)] = np.nan
    return bgr, depth
