"""The camera-frame front end on its whole input domain, GPU side: dvo_frames_upload_cameras (camera_level_kernel, the four-pixels-
per-lane full-resolution kernel, camera_decimate_levels_kernel) and the per-image map table of the tracker against the CPU oracle
BIT FOR BIT, and against the independent plain reference (tests/frame_reference.py) under the rules of
tests/test_frame_reference_cpu.py: equal outside the map's tie band; the 16-bit remap exact below 2^14 and within one unit inside the
rounding margin above.  That CPU file proves that these very inputs change under a reordered or a fused float sum, so bit-equality
with the oracle here is the guard for -ffp-contract=off and for the order of the four taps."""
import numpy as np
import pytest

import frame_reference as fr

pytestmark = pytest.mark.gpu

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


# ---- metres -> 16-bit millimetres on the whole float domain ------------------------------------------------------------------------
DEPTH_SHAPES = {"vector": (1400, 1972), "generic": (1399, 1970)}     # rows, cols multiples of four: the four-pixels-per-lane kernel


@pytest.fixture(scope="module")
def depth_values():
    return fr.depth_domain_values()


@pytest.mark.parametrize("shape,first_shift,where", [("vector", 0, "host"), ("generic", 0, "host"), ("generic", 1, "host"),
                                                    ("vector", 0, "device"), ("vector", 0, "device+4"), ("generic", 1, "device+4")])
def test_depth_conversion_whole_domain(oracle, depth_values, shape, first_shift, where):
    """every value of fr.depth_domain_values() through the upload: rounding ties, negatives, denormals, +-inf, NaN, the saturation, the
    |mm| >= 2^31 branch.  first_shift 1: every value sits at an even row and column of a frame of odd width, so level 0 holds them all"""
    rows, cols = DEPTH_SHAPES[shape]
    img = fr.depth_domain_image(depth_values, rows, cols)
    if first_shift:
        img = np.repeat(np.repeat(img, 2, 0), 2, 1)[:, :2 * cols - 1]
    assert img.shape[1] % 4 != 0 or shape == "vector"
    bgr = np.full(img.shape + (3,), 90, np.uint8)
    with _ctx() as ctx:
        if where == "host":
            ctx.frames_upload_cameras([bgr], [img], n_levels=1, first_shift=first_shift)
        else:
            off = 4 if where.endswith("+4") else 0                      # +4: not aligned for 16-byte loads, takes the landing copy
            tb, pb = _dev(bgr, 0)
            td, pd = _dev(img, off)
            assert (pd % 16 != 0) == bool(off)
            ctx.frames_upload_cameras_device([pb], [pd], img.shape[0], img.shape[1], n_levels=1, first_shift=first_shift)
        got = ctx.frame_level(0, 0)[1]
    assert got.shape == (rows, cols)
    want = depth_values if not first_shift else None
    src = fr.resize_nn(img, first_shift)
    if want is not None:
        assert np.array_equal(src.ravel()[:depth_values.size], depth_values, equal_nan=True)
    else:
        assert np.array_equal(src, fr.depth_domain_image(depth_values, rows, cols), equal_nan=True)
    assert np.array_equal(got, oracle.depth_m_to_mm16(src).astype(np.float32))
    assert np.array_equal(got, fr.depth_m_to_mm16(src).astype(np.float32))


# ---- BGR -> grey on every triple ---------------------------------------------------------------------------------------------------
def _all_triples():
    v = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)


def test_bgr2gray_every_triple_in_one_frame(oracle):
    bgr = _all_triples()
    with _ctx() as ctx:
        ctx.frames_upload_cameras([bgr], None, n_levels=1, first_shift=0)                # 4096 x 4096: the four-pixels-per-lane kernel
        grey = ctx.frame_level(0, 0, want_depth=False)[0]
        assert np.array_equal(grey, oracle.bgr2gray(bgr)) and np.array_equal(grey, fr.bgr2gray(bgr))
        odd = bgr[:4095, :4093]                                                          # odd size, shift 1 and 2: the rounded level sizes
        ctx.frames_upload_cameras([odd], None, n_levels=2, first_shift=1)
        for l in range(2):
            grey = ctx.frame_level(0, l, want_depth=False)[0]
            want = fr.bgr2gray(fr.resize_nn(odd, 1 + l))
            assert grey.shape == want.shape == (fr.level_size(4095, 1 + l), fr.level_size(4093, 1 + l))
            assert np.array_equal(grey, want) and np.array_equal(grey, oracle.bgr2gray(oracle.resize_nn(odd, 0.5 ** (1 + l))))


def test_bgr2gray_every_triple_in_a_batch_of_sixteen(oracle):
    """sixteen 1024 x 1024 frames in one call (blockIdx.y), all triples between them; also through the generic kernel (1023 columns)"""
    bgr = _all_triples().reshape(16, 1024, 1024, 3)
    with _ctx() as ctx:
        ctx.frames_reserve(16)
        ctx.frames_upload_cameras(list(bgr), None, n_levels=1, first_shift=0)
        for s in range(16):
            assert np.array_equal(ctx.frame_level(s, 0, want_depth=False)[0], fr.bgr2gray(bgr[s])), s
        cut = [np.ascontiguousarray(b[:, :1023]) for b in bgr]
        ctx.frames_upload_cameras(cut, None, n_levels=2, first_shift=0)
        for s in range(16):
            for l in range(2):
                assert np.array_equal(ctx.frame_level(s, l, want_depth=False)[0], fr.bgr2gray(fr.resize_nn(cut[s], l))), (s, l)


# ---- tile edges --------------------------------------------------------------------------------------------------------------------
def _check_levels(ctx, slot, ref_levels, oracle_pyr, what):
    """a stored frame against the oracle (bit for bit) and the reference (frame_reference rules); returns per level the counts of
    check_remap_u16"""
    counts = []
    for l, (lv, (og, od)) in enumerate(zip(ref_levels, oracle_pyr)):
        grey, dep, _, _ = ctx.frame_level(slot, l)
        assert grey.shape == og.shape == lv["grey"].shape, (what, l)
        assert np.array_equal(grey, og), (what, l, "grey vs oracle")
        assert np.array_equal(dep, od.astype(np.float32)), (what, l, "depth vs oracle", int((dep != od).sum()))
        ok = ~lv["band"]
        assert np.array_equal(grey[ok], lv["grey"][ok]), (what, l, "grey vs reference")
        counts.append(fr.check_remap_u16(dep, lv["r"], lv["frac"], lv["E"], where=ok))
    return counts


@pytest.mark.parametrize("with_map", [False, True])
def test_tile_edges(oracle, with_map):
    """sizes around the 64 x 16 tile of camera_level_kernel and the 64 x 64 tile of the full-resolution kernel, all levels that are not
    empty (at most DVO_MAX_LEVELS = 8)"""
    for rows in (1, 63, 64, 65, 129):
        for cols in (1, 3, 15, 16, 17, 33):
            nl = 1
            while nl < 8 and min(fr.level_size(rows, nl), fr.level_size(cols, nl)) >= 1:
                nl += 1
            bgr, depth = fr.edge_frame(rows, cols, 100 * rows + cols)
            calib = ((0.9 * cols + 3, 0.9 * cols + 4, cols / 2 - 0.3, rows / 2 + 0.2), (0.2, -0.1, 0.01, -0.01, 0.02)) if with_map else None
            if calib is not None:
                assert fr.undistort_map(rows, cols, *calib)[4].mean() <= 1e-4
            with _ctx() as ctx:
                if calib:
                    ctx.frames_set_undistort(rows, cols, *calib)
                ctx.frames_upload_cameras([bgr], [depth], n_levels=nl, first_shift=0)
                _check_levels(ctx, 0, fr.camera_levels(bgr, fr.depth_m_to_mm16(depth), nl, 0, calib),
                              oracle.build_pyramid(bgr, depth, nl, 0, undistort=calib), (rows, cols, with_map))


# ---- undistortion edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.CALIBRATIONS))
def test_undistortion_edges(oracle, name):
    rows, cols, K, D = fr.CALIBRATIONS[name]
    sx, sy, fx5, fy5, band = fr.undistort_map(rows, cols, K, D)
    assert band.mean() <= 1e-4
    bgr, depth = fr.edge_frame(rows, cols, 11)
    d16 = fr.depth_m_to_mm16(depth)
    assert d16.min() == 1 and d16.max() == 65535 and np.isnan(depth).any() and (depth == 0).any()
    nl = 3
    with _ctx() as ctx:
        ctx.frames_set_undistort(rows, cols, K, D)
        for shift in (0, 1):
            ctx.frames_upload_cameras([bgr], [depth], n_levels=nl, first_shift=shift)
            counts = _check_levels(ctx, 0, fr.camera_levels(bgr, d16, nl, shift, (K, D)),
                                   oracle.build_pyramid(bgr, depth, nl, shift, undistort=(K, D)), (name, shift))
            print("\n%-14s shift %d: per level (E >= 2^14, in margin, != rint(E)) %s" % (name, shift, counts), end="")
        # the coverage this case is here for (the same figures as the CPU file asserts on the map)
        out = fr.outside_counts((rows, cols), sx, sy)
        if name in fr.OUTSIDE_SHARE:
            assert (out > 0).mean() >= fr.OUTSIDE_SHARE[name][0] and (out == 4).mean() >= fr.OUTSIDE_SHARE[name][1]
        if name == "identity_int":                                       # fi == 0 everywhere: weights 32767 + 1, the result is the input
            ctx.frames_upload_cameras([bgr], [depth], n_levels=1, first_shift=0)
            grey, dep, _, _ = ctx.frame_level(0, 0)
            assert np.array_equal(grey, fr.bgr2gray(bgr)) and np.array_equal(dep, d16.astype(np.float32))
        # raw sensor units (DVO_UPLOAD_DEPTH_RAW): the same planes as floats, with and without the map; NaN / inf / 3e9 in a tap -> 0
        from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
        raw = d16.astype(np.float32)
        raw[::7, ::5] = np.nan
        raw[3::11, 2::9] = np.inf
        raw[5::13, 1::6] = 3e9
        ctx.frames_upload_cameras([bgr], [raw], n_levels=nl, first_shift=0, flags=DVO_UPLOAD_DEPTH_RAW)
        want = oracle.undistort_u16_from_f32(raw, K, D)
        nan_tap = np.zeros((rows, cols), bool)
        for yy, xx, inside in fr._taps((rows, cols), sx, sy):
            nan_tap |= inside & np.isnan(raw)[yy, xx]
        assert nan_tap.any() or (out == 4).mean() > 0.7
        assert (want[nan_tap] == 0).all()
        for l in range(nl):
            assert np.array_equal(ctx.frame_level(0, l)[1], fr.resize_nn(want, l).astype(np.float32)), (name, l, "raw depth under the map")
        ctx.frames_set_undistort(0, 0, None, None)                       # without a map a raw frame is stored as it is, NaN included
        ctx.frames_upload_cameras([bgr], [raw], n_levels=nl, first_shift=0, flags=DVO_UPLOAD_DEPTH_RAW)
        for l in range(nl):
            assert np.array_equal(ctx.frame_level(0, l)[1], fr.resize_nn(raw, l), equal_nan=True), (name, l, "raw depth as is")


# ---- the per-image map table ---------------------------------------------------------------------------------------------------------
def test_tracker_tick_with_three_maps_and_one_stream_without(oracle):
    """one tick of the multi-stream tracker: streams 0, 1, 3 carry three different maps, stream 2 none -- one launch per stage reads the
    map of each image out of the table (NULL entry: no map).  Each stream's stored levels equal the single-context result for its own
    calibration (itself compared with oracle and reference in test_undistortion_edges)"""
    from rgbd_odometry_amd import DvoTracker, capi
    rows, cols, nl = 240, 320, 3
    cal = dict(fr.CALIBRATIONS, barrel320=(rows, cols, (255.0, 250.0, 161.7, 118.3), (-0.3, 0.1, 0.002, 0.001, -0.02)))
    rig = ["pincushion", "tangential", None, "barrel320"]
    assert all(cal[n][:2] == (rows, cols) for n in rig if n)
    frames = [fr.edge_frame(rows, cols, 40 + s) for s in range(len(rig))]
    with DvoTracker(len(rig), iters=[2, 2, 2], rows=rows, cols=cols, n_levels=nl, first_shift=0) as tr:
        tr.set_intrinsics(262.5, 262.5, 159.75, 119.75)
        for s, n in enumerate(rig):
            if n:
                tr.set_stream_undistort(s, np.array(cal[n][2]), np.array(cal[n][3]))
        try:
            tr.step(list(range(len(rig))), [f[0] for f in frames], [f[1] for f in frames])
        except capi.DvoError:
            pass              # a first frame whose far corner holds no reference point is refused AFTER the levels were written
        h = tr.context_handle()
        lib = capi.load_library()
        stored = {}
        for slot in range(2 * len(rig) + 2):
            for l in range(nl):
                r, c = fr.level_size(rows, l), fr.level_size(cols, l)
                g, d = np.zeros(r * c, np.uint8), np.zeros(r * c, np.float32)
                if lib.dvo_frame_get_level(h, slot, l, None, None, capi._ptr(g), capi._ptr(d), None, None) == 0:
                    stored[(slot, l)] = (g.reshape(c, r).T.copy(), d.reshape(c, r).T.copy())
    for s, n in enumerate(rig):
        with _ctx() as ctx:
            if n:
                ctx.frames_set_undistort(rows, cols, cal[n][2], cal[n][3])
            ctx.frames_upload_cameras([frames[s][0]], [frames[s][1]], n_levels=nl, first_shift=0)
            want = [ctx.frame_level(0, l)[:2] for l in range(nl)]
        hits = [slot for slot in range(2 * len(rig) + 2) if all((slot, l) in stored and np.array_equal(stored[(slot, l)][0], want[l][0]) and
                                                                 np.array_equal(stored[(slot, l)][1], want[l][1]) for l in range(nl))]
        assert len(hits) >= 1, "stream %d (%s): no stored frame equals the single-context result" % (s, n)


# ---- calibrations that are not numbers -----------------------------------------------------------------------------------------------
def test_calibrations_that_are_not_numbers(oracle):
    from rgbd_odometry_amd import DvoError, DvoTracker
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    rows, cols, K, D = fr.CALIBRATIONS["barrel"]
    bgr, depth = fr.edge_frame(rows, cols, 5)
    want = oracle.build_pyramid(bgr, depth, 2, 0, undistort=(K, D))
    with _ctx() as ctx:
        ctx.frames_set_undistort(rows, cols, K, D)
        for k in range(9):
            for bad in (np.nan, np.inf, -np.inf):
                v = np.array(K + D, np.float64); v[k] = bad
                with pytest.raises(DvoError) as e:
                    ctx.frames_set_undistort(rows, cols, v[:4], v[4:])
                assert e.value.code == DVO_ERR_INVALID
        with pytest.raises(DvoError):
            ctx.frames_set_undistort(rows, cols, (0.0,) + K[1:], D)
        ctx.frames_upload_cameras([bgr], [depth], n_levels=2, first_shift=0)           # the refused calls changed nothing
        for l, (g, d16) in enumerate(want):
            grey, dep, _, _ = ctx.frame_level(0, l)
            assert np.array_equal(grey, g) and np.array_equal(dep, d16.astype(np.float32))
        # finite, but u*32 leaves the int range: accepted, and equal to the oracle's saturating cvRound (INT_MIN -> pixel (0, 0))
        for Dx in ((1e9, 0.0, 0.0, 0.0, 0.0), (0.0, 0.0, 1e11, -1e11, 0.0), (-1e12, 0.0, 0.0, 0.0, 1e15)):
            ctx.frames_set_undistort(rows, cols, K, Dx)
            ctx.frames_upload_cameras([bgr], [depth], n_levels=2, first_shift=0)
            for l, (g, d16) in enumerate(oracle.build_pyramid(bgr, depth, 2, 0, undistort=(K, Dx))):
                grey, dep, _, _ = ctx.frame_level(0, l)
                assert np.array_equal(grey, g) and np.array_equal(dep, d16.astype(np.float32)), (Dx, l)
    with DvoTracker(2, iters=[2, 2], rows=rows, cols=cols, n_levels=2, first_shift=0) as tr:
        tr.set_intrinsics(*K)
        for k in range(9):
            v = np.array(K + D, np.float64); v[k] = np.nan if k % 2 else np.inf
            with pytest.raises(DvoError) as e:
                tr.set_stream_undistort(1, v[:4], v[4:])
            assert e.value.code == DVO_ERR_INVALID
