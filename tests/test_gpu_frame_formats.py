"""Camera frames in sensor formats (dvo_frames_upload_cameras_fmt: mono8 / RGB8 images, 16-bit millimetre depth) on the GPU.

include/dvo_amd.h DEFINES each format by the (BGR8, float depth) input it stands for, so every case uploads a frame twice -- in the new
format, and converted on the host through the existing entry point into a second context with the same parameters -- and asks for every
level's grey, depth and edge map to be bit-equal.  Each case is also held against the independent plain reference
(tests/frame_reference.py, which takes the 16-bit image directly) under the rules tests/test_gpu_frame_inputs.py applies: grey equal
outside the map's tie band, the 16-bit remap through check_remap_u16."""
import ctypes as C

import numpy as np
import pytest

import frame_reference as fr

pytestmark = pytest.mark.gpu

MONO, RGB, BGR = "mono8", "rgb8", "bgr8"


def _ctx(n_pairs=1, **kw):
    from rgbd_odometry_amd import DvoContext
    return DvoContext(n_pairs, **kw)


def _dev(arr, off):
    """the array's bytes in device memory at an address `off` bytes past an allocation's start; (tensor to keep, address)"""
    import torch
    arr = np.ascontiguousarray(arr)
    raw = torch.zeros(arr.nbytes + 64, dtype=torch.uint8, device="cuda")
    raw[off:off + arr.nbytes] = torch.from_numpy(np.frombuffer(arr.tobytes(), np.uint8).copy()).cuda()
    return raw, raw.data_ptr() + off


# ---- the definitions of include/dvo_amd.h, on the host --------------------------------------------------------------------------------
def as_bgr(img, fmt):
    """the BGR8 image a frame in `fmt` stands for"""
    if fmt == MONO:
        return np.repeat(img[..., None], 3, 2)
    return np.ascontiguousarray(img[..., ::-1]) if fmt == RGB else img


def effective_u16(d16, raw):
    """the 16-bit image the engine works on: as it is under DVO_UPLOAD_DEPTH_RAW, else after the publisher's setTo(1, depth16 == 0)"""
    return d16 if raw else np.where(d16 == 0, 1, d16).astype(np.uint16)


def _image(bgr, fmt):
    """a frame in `fmt` whose BGR8 equivalent is `bgr` (mono8: its green channel)"""
    if fmt == MONO:
        return np.ascontiguousarray(bgr[..., 1])
    return np.ascontiguousarray(bgr[..., ::-1]) if fmt == RGB else bgr


def _upload(ctx, imgs, d16s, fmt, **kw):
    ctx.frames_upload_cameras(imgs, d16s, rgb=(fmt == RGB), **kw)


def _upload_converted(ctx, imgs, d16s, fmt, flags=0, **kw):
    """the existing entry point fed the input the formats stand for"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    dl = None if d16s is None else [effective_u16(d, flags & DVO_UPLOAD_DEPTH_RAW).astype(np.float32) for d in d16s]
    ctx.frames_upload_cameras([as_bgr(i, fmt) for i in imgs], dl, flags=flags | DVO_UPLOAD_DEPTH_RAW, **kw)


def _stored(ctx, slot, nl, depth=True):
    return [ctx.frame_level(slot, l, want_depth=depth) for l in range(nl)]


def _assert_same(got, want, what):
    for l, (a, b) in enumerate(zip(got, want)):
        assert a[0].shape == b[0].shape, (what, l)
        assert np.array_equal(a[0], b[0]), (what, l, "grey")
        if b[1] is not None:
            assert np.array_equal(a[1], b[1]), (what, l, "depth", int((a[1] != b[1]).sum()))
        assert np.array_equal(a[2], b[2]) and a[3] == b[3], (what, l, "edge map")


def _assert_reference(got, img, d16, fmt, raw, nl, shift, calib, what):
    """the stored levels against tests/frame_reference.py (test_gpu_frame_inputs._check_levels' rules)"""
    ref = fr.camera_levels(as_bgr(img, fmt), None if d16 is None else effective_u16(d16, raw), nl, shift, calib)
    for l, lv in enumerate(ref):
        grey, dep = got[l][0], got[l][1]
        ok = ~lv["band"]
        assert grey.shape == lv["grey"].shape and np.array_equal(grey[ok], lv["grey"][ok]), (what, l, "grey vs reference")
        if d16 is not None:
            fr.check_remap_u16(dep, lv["r"], lv["frac"], lv["E"], where=ok)


def _both(imgs, d16s, fmt, nl, shift, flags=0, calib=None, what=None):
    """upload in the new format and converted, compare every level of every frame; returns the new-format levels of frame 0"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    n = len(imgs)
    with _ctx() as a, _ctx() as b:
        for c in (a, b):
            c.frames_reserve(n)
            if calib:
                c.frames_set_undistort(imgs[0].shape[0], imgs[0].shape[1], *calib)
        _upload(a, imgs, d16s, fmt, n_levels=nl, first_shift=shift, flags=flags)
        _upload_converted(b, imgs, d16s, fmt, n_levels=nl, first_shift=shift, flags=flags)
        first = None
        for s in range(n):
            got = _stored(a, s, nl, d16s is not None)
            _assert_same(got, _stored(b, s, nl, d16s is not None), (what, s))
            _assert_reference(got, imgs[s], None if d16s is None else d16s[s], fmt, flags & DVO_UPLOAD_DEPTH_RAW, nl, shift, calib, (what, s))
            first = first or got
    return first


def _frame(rows, cols, seed):
    """a seeded random BGR8 frame and a 16-bit depth image over the whole range with holes"""
    rng = np.random.default_rng(seed)
    bgr = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    d16 = rng.integers(0, 65536, (rows, cols)).astype(np.uint16)
    d16[rng.random((rows, cols)) < 0.05] = 0
    d16.flat[:4] = (0, 1, 65535, 16384)
    return bgr, d16


# ---- the whole 16-bit depth domain ---------------------------------------------------------------------------------------------------
def _depth_domain(shape):
    """vector: all 65 536 values in one 256 x 256 frame (rows, cols multiples of four: the four-pixels-per-lane kernel at shift 0).
    generic: 255 x 257 has 65 535 pixels, one short of the domain, so two such frames go up in one call: 0 .. 65 534 ascending and
    65 535 .. 1 descending -- every value occurs, 0 and 65 535 included, and every value but those two at two different places."""
    v = np.arange(65536, dtype=np.uint16)
    if shape == "vector":
        return [v.reshape(256, 256)]
    return [v[:65535].reshape(255, 257), v[:0:-1].reshape(255, 257).copy()]


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("first_shift", [0, 1])
@pytest.mark.parametrize("shape", ["vector", "generic"])
def test_u16_depth_whole_domain(shape, first_shift, raw):
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    kept = _depth_domain(shape)
    if first_shift:                                  # every value at an even row and column; the pixels the level drops hold other values
        full = []
        for k in kept:
            f = np.repeat(np.repeat(~k, 2, 0), 2, 1)
            f[::2, ::2] = k
            full.append(f)
    else:
        full = kept
    rows, cols = full[0].shape
    assert fr.level_size(rows, first_shift) == kept[0].shape[0] and fr.level_size(cols, first_shift) == kept[0].shape[1]
    assert np.array_equal(np.unique(np.concatenate([k.ravel() for k in kept])), np.arange(65536))
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8) for _ in full]
    flags = DVO_UPLOAD_DEPTH_RAW if raw else 0
    n = len(full)
    with _ctx() as a, _ctx() as b:
        a.frames_reserve(n)
        b.frames_reserve(n)
        _upload(a, imgs, full, BGR, n_levels=1, first_shift=first_shift, flags=flags)
        _upload_converted(b, imgs, full, BGR, n_levels=1, first_shift=first_shift, flags=flags)
        for s in range(n):
            got = _stored(a, s, 1)
            _assert_same(got, _stored(b, s, 1), (shape, first_shift, raw, s))
            _assert_reference(got, imgs[s], full[s], BGR, raw, 1, first_shift, None, (shape, first_shift, raw, s))
            dep = got[0][1]
            want = kept[s].astype(np.float32)
            if not raw:
                want[kept[s] == 0] = 1.0                                  # 0 -> 1 only without DVO_UPLOAD_DEPTH_RAW
            assert np.array_equal(dep, want)
            assert dep[kept[s] == 65535].tolist() == [65535.0] * int((kept[s] == 65535).sum())
            assert dep[kept[s] == 0].tolist() == [0.0 if raw else 1.0] * int((kept[s] == 0).sum())


# ---- mono8 and RGB8 ------------------------------------------------------------------------------------------------------------------
def _triples_256():
    """rows and columns 0 .. 255 of the frame that holds every (b, g, r) triple at pixel v = row * 4096 + col (test_gpu_frame_inputs._all_triples)"""
    i, j = np.mgrid[0:256, 0:256].astype(np.uint32)
    v = i * 4096 + j
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8)


@pytest.fixture(scope="module")
def colour_sources():
    return {"random": _frame(256, 256, 17), "triples": (_triples_256(), _frame(256, 256, 18)[1])}


@pytest.mark.parametrize("n_levels", [1, 3])
@pytest.mark.parametrize("fmt,size", [(MONO, (68, 132)), (MONO, (67, 131)), (RGB, (68, 132)), (RGB, (67, 131)), (RGB, (256, 256))])
def test_mono8_and_rgb8(colour_sources, fmt, size, n_levels):
    """68 x 132: partial 64 x 64 tiles of the four-pixels-per-lane kernel; 67 x 131: the generic kernel; 256 x 256: the RGB8 sources whole
    (the smaller sizes are their top left corners)"""
    rows, cols = size
    for name, (bgr, d16) in colour_sources.items():
        if fmt == MONO:
            if name == "triples":
                continue
            g = np.random.default_rng(5).permutation(np.arange(rows * cols) % 256).astype(np.uint8).reshape(rows, cols)
            assert np.unique(g).size == 256                               # all 256 values
            img = g
        else:
            img = _image(np.ascontiguousarray(bgr[:rows, :cols]), RGB)
        d = np.ascontiguousarray(d16[:rows, :cols])
        got = _both([img], [d], fmt, n_levels, 0, what=(fmt, size, name))
        if fmt == MONO:
            assert np.array_equal(got[0][0], img)                         # the grey value of (g, g, g) is g
        _both([img], None, fmt, n_levels, 1, what=(fmt, size, name, "no depth, shift 1"))


# ---- under an undistortion map -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("fmt", [BGR, RGB, MONO])
def test_formats_under_a_map(fmt, raw):
    """96 x 128 under the barrel calibration: taps outside the source, depth above 2^14 (the order of the four taps and the unfused
    products are part of the result there), all image formats with 16-bit depth"""
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    rows, cols = 96, 128
    K, D = fr.CALIBRATIONS["barrel"][2:]
    sx, sy, _, _, band = fr.undistort_map(rows, cols, K, D)
    out = fr.outside_counts((rows, cols), sx, sy)
    assert band.mean() <= 1e-4 and (out > 0).mean() > 0.02 and (out == 4).mean() > 0.01 and ((out > 0) & (out < 4)).any()
    bgr, d16 = _frame(rows, cols, 23)
    i, j = np.mgrid[0:rows, 0:cols]
    steps = np.array([16383, 16385, 65535, 1, 40001, 0, 32767, 50001], np.uint16)
    d16[rows // 3:rows // 2] = steps[(j[rows // 3:rows // 2] // 3) % steps.size]          # sharp steps on both sides of 2^14
    assert (d16 > 1 << 14).mean() > 0.5
    img = _image(bgr, fmt)
    for shift in (0, 1):
        _both([img], [d16], fmt, 3, shift, flags=DVO_UPLOAD_DEPTH_RAW if raw else 0, calib=(K, D), what=(fmt, raw, shift))


# ---- every source mode ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["direct", "mapped", "device", "device+off"])
@pytest.mark.parametrize("fmt", [BGR, RGB, MONO])
def test_every_source_mode(fmt, where):
    """pageable host memory is what every other case uses; here DVO_UPLOAD_DIRECT, mapped pinned memory (pulled by the gather kernel),
    device pointers aligned for the vector loads (read in place) and device pointers off that alignment -- the image by one byte, the
    depth by two -- which take the landing copy.  68 x 132: the four-pixels-per-lane kernel reads the 8-byte depth quads"""
    from rgbd_odometry_amd import capi
    rows, cols, nl = 68, 132, 2
    frames = [_frame(rows, cols, 31 + s) for s in range(2)]
    imgs, d16s = [_image(f[0], fmt) for f in frames], [f[1] for f in frames]
    ifmt = {BGR: capi.DVO_CAM_BGR8, RGB: capi.DVO_CAM_RGB8, MONO: capi.DVO_CAM_MONO8}[fmt]
    with _ctx() as a, _ctx() as b:
        _upload_converted(b, imgs, d16s, fmt, n_levels=nl, first_shift=0)
        if where == "direct":
            _upload(a, imgs, d16s, fmt, n_levels=nl, first_shift=0, flags=capi.DVO_UPLOAD_DIRECT)
        elif where == "mapped":
            keep = []
            for src in imgs + d16s:
                m = capi.MappedHostArray(src.shape, src.dtype)
                m.array[...] = src
                keep.append(m)
            _upload(a, [m.array for m in keep[:2]], [m.array for m in keep[2:]], fmt, n_levels=nl, first_shift=0, flags=capi.DVO_UPLOAD_MAPPED)
        else:
            off = where.endswith("+off")
            ti = [_dev(i, 1 if off else 0) for i in imgs]
            td = [_dev(d, 2 if off else 0) for d in d16s]
            assert all((p % 4 != 0) == off for _, p in ti) and all((p % 8 != 0) == off for _, p in td)
            a.frames_upload_cameras_device([p for _, p in ti], [p for _, p in td], rows, cols, n_levels=nl, first_shift=0,
                                           image_format=ifmt, depth_format=capi.DVO_DEPTH_U16)
        for s in range(2):
            got = _stored(a, s, nl)
            _assert_same(got, _stored(b, s, nl), (fmt, where, s))
            _assert_reference(got, imgs[s], d16s[s], fmt, False, nl, 0, None, (fmt, where, s))


# ---- a batch -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "mapped", "device+off"])
def test_batch_of_33_as_now_frames(where):
    """33 frames of distinct content in one call, one more than a gather launch carries, installed as the now frames of 33 pairs"""
    from rgbd_odometry_amd import capi
    n, rows, cols, nl = 33, 68, 132, 2
    frames = [_frame(rows, cols, 100 + s) for s in range(n)]
    imgs, d16s = [_image(f[0], MONO) for f in frames], [f[1] for f in frames]
    assert len({i.tobytes() for i in imgs}) == n
    with _ctx(n) as a, _ctx(n) as b:
        _upload_converted(b, imgs, d16s, MONO, n_levels=nl, first_shift=0, now_first_pair=0)
        if where == "host":
            _upload(a, imgs, d16s, MONO, n_levels=nl, first_shift=0, now_first_pair=0)
        elif where == "mapped":
            mi, md = capi.MappedHostArray((n, rows, cols), np.uint8), capi.MappedHostArray((n, rows, cols), np.uint16)
            mi.array[...] = np.stack(imgs)
            md.array[...] = np.stack(d16s)
            _upload(a, list(mi.array), list(md.array), MONO, n_levels=nl, first_shift=0, now_first_pair=0, flags=capi.DVO_UPLOAD_MAPPED)
        else:
            ti, td = [_dev(i, 1) for i in imgs], [_dev(d, 2) for d in d16s]
            a.frames_upload_cameras_device([p for _, p in ti], [p for _, p in td], rows, cols, n_levels=nl, first_shift=0, now_first_pair=0,
                                           image_format=capi.DVO_CAM_MONO8, depth_format=capi.DVO_DEPTH_U16)
        for s in range(n):
            _assert_same(_stored(a, s, nl), _stored(b, s, nl), (where, s))
            assert np.array_equal(a.frame_level(s, 0)[0], imgs[s]), s
            for l in range(nl):
                for x, y in zip(a.get_now_level(l, s), b.get_now_level(l, s)):
                    assert np.array_equal(x, y), (where, s, l, "now level")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_frame_store_unchanged():
    from rgbd_odometry_amd import capi
    rows, cols, nl = 96, 128, 2
    bgr, d16 = _frame(rows, cols, 41)
    other, o16 = _frame(rows, cols, 42)
    K, D = fr.CALIBRATIONS["barrel"][2:]
    with _ctx() as ctx:
        ctx.frames_set_undistort(rows, cols, K, D)
        _upload(ctx, [_image(bgr, MONO)], [d16], MONO, n_levels=nl, first_shift=0)
        before = _stored(ctx, 0, nl)
        img = _image(other, MONO)
        table = lambda *addr: (C.c_void_p * len(addr))(*addr)

        def call(images, ifmt, depths, dfmt, r=rows, c=cols):
            return ctx.lib.dvo_frames_upload_cameras_fmt(ctx._h, 0, len(images), images, ifmt, depths, dfmt, r, c, nl, 0, -1, 0)

        I, Dp = table(img.ctypes.data), table(o16.ctypes.data)
        for ifmt, dfmt in ((3, capi.DVO_DEPTH_U16), (-1, capi.DVO_DEPTH_U16), (capi.DVO_CAM_MONO8, 2), (capi.DVO_CAM_MONO8, -1), (7, 7)):
            assert call(I, ifmt, Dp, dfmt) == capi.DVO_ERR_INVALID, (ifmt, dfmt)
        assert call(I, capi.DVO_CAM_MONO8, table(None), capi.DVO_DEPTH_U16) == capi.DVO_ERR_INVALID           # a NULL depth entry
        assert call(table(None), capi.DVO_CAM_MONO8, Dp, capi.DVO_DEPTH_U16) == capi.DVO_ERR_INVALID          # a NULL image entry
        assert call(I, capi.DVO_CAM_MONO8, Dp, capi.DVO_DEPTH_U16, rows // 2, cols * 2) == capi.DVO_ERR_INVALID   # not the map's geometry
        with pytest.raises(capi.DvoError) as e:
            _upload(ctx, [img[:, :cols - 4]], [o16[:, :cols - 4]], MONO, n_levels=nl, first_shift=0)
        assert e.value.code == capi.DVO_ERR_INVALID
        _assert_same(_stored(ctx, 0, nl), before, "after the refused calls")
        assert call(I, capi.DVO_CAM_MONO8, Dp, capi.DVO_DEPTH_U16) == capi.DVO_OK                             # and the handle still works
        assert not np.array_equal(ctx.frame_level(0, 0)[0], before[0][0])
