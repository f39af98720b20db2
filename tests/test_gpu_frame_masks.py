"""Per-pair ignore masks of the frame stage on the GPU (include/dvo_amd.h, "ignore masks").  The feature is defined in bytes, so every
check is an equality: the device planes against dvo_mask_levels_host and the numpy restatement (tests/mask_reference.py); the stored
edge maps against `unmasked edges & keep` and against the oracle's Canny & keep; the now level and the reference list against the
oracle run on the masked edge map.

Frames: rgbd_odometry_amd.frame_gen.camera_frame.  Masks: mask_reference.scene_mask -- a rectangle over the lower third plus one interior
disc.  Every tested frame is checked to have, at every level, at least one oracle edge pixel the mask drops and one it keeps (the seeds
were chosen for that on the CPU).  Launch counts are read through dvo_tracker_get_stats, the library's launch counter: a tracker's
first step is one upload (dvo_frames_upload_cameras_fmt with now_first_pair >= 0) plus the reference extraction."""
import functools

import numpy as np
import pytest

from rgbd_odometry_amd import frame_gen
import mask_reference as mr
import oracle_lib

pytestmark = pytest.mark.gpu

NL, SHIFT, MARGIN = 3, 1, 2
GEOMETRIES = [(96, 128), (75, 101)]          # 75 x 101: levels 38x50, 19x25, 9x13 -- store strides that are no multiples of 16 (nor of 4)
FRAME_SEEDS = (21, 23, 24)                   # pairs 0, 1, 2
MASK_SEED = {0: 1, 2: 2}                     # pair -> scene_mask seed; pair 1 has no mask
K = (131.25, 131.25, 63.75, 47.75)           # of the first stored level


def cm(a_rm):
    """row-major 2-D array -> flat column-major buffer"""
    return np.ascontiguousarray(np.asarray(a_rm).T).ravel()


@functools.lru_cache(maxsize=None)
def scene(rows, cols):
    """the three frames, the masks of pairs 0 and 2, the keep planes and the oracle's pyramids and edge maps: computed once"""
    o = oracle_lib.load()
    frames = [frame_gen.camera_frame(s, rows, cols) for s in FRAME_SEEDS]
    masks = {p: mr.scene_mask(rows, cols, k) for p, k in MASK_SEED.items()}
    keep = {p: mr.keep_levels(m, NL, SHIFT, MARGIN) for p, m in masks.items()}
    pyr = [o.build_pyramid(b, d, NL, SHIFT) for b, d in frames]
    canny = [[o.canny(g) for g, _ in p] for p in pyr]
    for p in masks:                          # the condition that keeps the tests honest
        for l in range(NL):
            e = canny[p][l] != 0
            assert (e & (keep[p][l] == 0)).any() and (e & (keep[p][l] != 0)).any(), (rows, cols, p, l)
    return dict(frames=frames, masks=masks, keep=keep, pyr=pyr, canny=canny)


def masked_context(S, n_pairs=3):
    from rgbd_odometry_amd import DvoContext
    ctx = DvoContext(n_pairs)
    for p, m in S["masks"].items():
        ctx.frames_set_pair_mask(p, m, NL, SHIFT, MARGIN)
    return ctx


def _dev(arr):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    return t, t.data_ptr()


def upload(ctx, S, path, rows, cols, **kw):
    """the three frames as the now frames of pairs 0..2 through one of the upload paths; returns the grey pyramids the path stores"""
    from rgbd_odometry_amd import capi
    bgr = [f[0] for f in S["frames"]]
    dep = [f[1] for f in S["frames"]]
    if path == "cameras":
        ctx.frames_upload_cameras(bgr, dep, n_levels=NL, first_shift=SHIFT, now_first_pair=0, **kw)
    elif path == "fmt":                      # mono8 + 16-bit millimetres
        conv = [frame_gen.as_format(b, d, "mono8", "u16") for b, d in S["frames"]]
        ctx.frames_upload_cameras([c[0] for c in conv], [c[1] for c in conv], n_levels=NL, first_shift=SHIFT, now_first_pair=0, **kw)
    elif path == "pyramids":
        ctx.frames_upload_pyramids(S["pyr"], now_first_pair=0, **kw)
    elif path == "device":
        tb, td = [_dev(b) for b in bgr], [_dev(d) for d in dep]
        ctx.frames_upload_cameras_device([p for _, p in tb], [p for _, p in td], rows, cols, n_levels=NL, first_shift=SHIFT,
                                         now_first_pair=0, flags=capi.DVO_UPLOAD_DEVICE, **kw)
        ctx.synchronize()
        del tb, td
    else:
        raise AssertionError(path)


PLANE_GEOMETRIES = [(96, 128, 1, 3), (75, 101, 1, 3), (100, 100, 3, 1)]


def test_device_planes_equal_the_host_builder_and_the_restatement():
    from rgbd_odometry_amd import DvoContext, DvoError, capi
    with DvoContext(2) as ctx:
        for rows, cols, shift, nl in PLANE_GEOMETRIES:
            for margin in (0, 2):
                for name, mask in (("scene", mr.scene_mask(rows, cols, 1)), ("set", np.ones((rows, cols), np.uint8)),
                                   ("corner", np.pad(np.ones((1, 1), np.uint8), ((rows - 1, 0), (cols - 1, 0))))):
                    ctx.frames_set_pair_mask(0, mask, nl, shift, margin)
                    host = capi.mask_levels_host(mask, nl, shift, margin)
                    want = mr.keep_levels(mask, nl, shift, margin)
                    for l in range(nl):
                        got = ctx.frames_get_pair_mask_level(0, l)
                        assert got.shape == want[l].shape, (rows, cols, margin, name, l)
                        assert np.array_equal(got, host[l]) and np.array_equal(got, want[l]), (rows, cols, margin, name, l)
                    with pytest.raises(DvoError) as ei:
                        ctx.frames_get_pair_mask_level(0, nl)
                    assert ei.value.code == capi.DVO_ERR_INVALID
        with pytest.raises(DvoError) as ei:                  # pair 1 never got one
            ctx.frames_get_pair_mask_level(1, 0)
        assert ei.value.code == capi.DVO_ERR_STATE
        m = mr.scene_mask(96, 128, 2)
        ctx.frames_set_pair_mask(-1, m, 3, 1, 8)             # every pair, the largest margin
        want = mr.keep_levels(m, 3, 1, 8)
        for p in range(2):
            for l in range(3):
                assert np.array_equal(ctx.frames_get_pair_mask_level(p, l), want[l])
        ctx.frames_set_pair_mask(0, None)
        with pytest.raises(DvoError) as ei:
            ctx.frames_get_pair_mask_level(0, 0)
        assert ei.value.code == capi.DVO_ERR_STATE
        assert np.array_equal(ctx.frames_get_pair_mask_level(1, 2), want[2])      # pair 1 keeps the shared planes


@pytest.mark.parametrize("path", ["cameras", "fmt", "pyramids", "device"])
@pytest.mark.parametrize("rows,cols", GEOMETRIES)
def test_edges_are_the_unmasked_edges_and_keep(oracle, rows, cols, path):
    """pairs 0 and 2 have different masks, pair 1 has none, one batch"""
    from rgbd_odometry_amd import DvoContext
    S = scene(rows, cols)
    with masked_context(S) as a, DvoContext(3) as b:
        upload(a, S, path, rows, cols)
        upload(b, S, path, rows, cols)
        for p in range(3):
            for l in range(NL):
                grey_a, _, edge_a, n_a = a.frame_level(p, l, want_depth=False)
                grey_b, _, edge_b, n_b = b.frame_level(p, l, want_depth=False)
                assert np.array_equal(grey_a, grey_b) and np.array_equal(grey_a, S["pyr"][p][l][0])      # the grey plane is untouched
                assert np.array_equal(edge_b, S["canny"][p][l]) and n_b == int((edge_b != 0).sum())
                keep = S["keep"][p][l] if p in S["keep"] else np.full(edge_b.shape, 255, np.uint8)
                assert np.array_equal(edge_a, edge_b & keep), (p, l, int((edge_a != (edge_b & keep)).sum()))
                assert np.array_equal(edge_a, S["canny"][p][l] & keep)
                assert n_a == int(((edge_b & keep) != 0).sum())
                if p in S["keep"]:
                    assert 0 < n_a < n_b
        for p in range(3):                                    # the depth plane is untouched, too
            for l in range(NL):
                da, db = a.frame_level(p, l)[1], b.frame_level(p, l)[1]
                assert np.array_equal(da, db, equal_nan=True)


@pytest.mark.parametrize("rows,cols", GEOMETRIES)
def test_now_level_is_the_oracles_on_the_masked_edges(oracle, rows, cols):
    from rgbd_odometry_amd import DvoContext
    S = scene(rows, cols)
    with masked_context(S) as a, DvoContext(1) as c:
        upload(a, S, "cameras", rows, cols)
        for p in S["keep"]:
            for l in range(NL):
                masked = S["canny"][p][l] & S["keep"][p][l]
                r, k = masked.shape
                want = oracle.now_level_from_edges(cm(masked), r, k)
                got = a.get_now_level(l, pair=p)
                c.set_now_level_from_edges(l, cm(masked), r, k)
                twin = c.get_now_level(l)
                plain = oracle.now_level_from_edges(cm(S["canny"][p][l]), r, k)
                for g, w, t, u in zip(got, want, twin, plain):
                    assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (p, l)
                    assert np.array_equal(g.view(np.uint32), t.view(np.uint32)), (p, l)
                assert not np.array_equal(want[0], plain[0]), "the mask must change this distance transform"


@pytest.mark.parametrize("rows,cols", GEOMETRIES)
def test_reference_list_is_the_oracles_on_the_masked_edges(oracle, rows, cols):
    from rgbd_odometry_amd import DvoContext
    S = scene(rows, cols)
    Kf = tuple(np.float32(k) for k in K)
    with masked_context(S) as a, DvoContext(3) as b:
        for ctx in (a, b):
            ctx.set_intrinsics(*K)
            upload(ctx, S, "cameras", rows, cols)
        Na, Nb = a.frames_as_ref(0, 0, 3), b.frames_as_ref(0, 0, 3)
        for p in range(3):
            for l in range(NL):
                g, d16 = S["pyr"][p][l]
                keep = S["keep"][p][l] if p in S["keep"] else np.full(g.shape, 255, np.uint8)
                d = d16.astype(np.uint16).copy()
                d[d == 0] = 1
                xyz, _ = oracle.enlist_ref_points(l, cm(S["canny"][p][l] & keep).astype(np.int32), cm(d).astype(np.float32), g.shape[0], g.shape[1], Kf)
                got = a.get_ref_level(l, pair=p)
                assert Na[p, l] == len(xyz) == len(got)
                assert np.array_equal(got.view(np.uint32), np.asarray(xyz, np.float32).reshape(-1, 3).view(np.uint32)), (p, l)
                if p in S["keep"]:
                    assert 0 < Na[p, l] < Nb[p, l], (p, l, Na[p, l], Nb[p, l])
                else:
                    assert Na[p, l] == Nb[p, l] and np.array_equal(got, b.get_ref_level(l, pair=p))


def test_all_set_mask_leaves_no_edges():
    from rgbd_odometry_amd import DvoContext, DvoError, capi
    rows, cols = 96, 128
    S = scene(rows, cols)
    with DvoContext(3) as a, DvoContext(1) as c:
        a.set_intrinsics(*K)
        a.frames_set_pair_mask(-1, np.full((rows, cols), 255, np.uint8), NL, SHIFT, 0)
        upload(a, S, "cameras", rows, cols)
        # dvo_set_now_level_from_edges refuses a map without an edge pixel (DVO_ERR_INVALID: "the distance transform is undefined"), so
        # the twin is the path an edge-free frame takes today: a uniform grey frame through the same upload, whose now level is all zeros
        with pytest.raises(DvoError) as ei:
            c.set_now_level_from_edges(0, np.zeros(48 * 64, np.uint8), 48, 64)
        assert ei.value.code == capi.DVO_ERR_INVALID
        c.frames_upload_cameras([np.full((rows, cols, 3), 77, np.uint8)], [np.full((rows, cols), 2.0, np.float32)], n_levels=NL,
                                first_shift=SHIFT, now_first_pair=0)
        for p in range(3):
            for l in range(NL):
                _, _, edge, n = a.frame_level(p, l, want_depth=False)
                assert not edge.any() and n == 0
                assert not c.frame_level(0, l, want_depth=False)[2].any()
                for g, w in zip(a.get_now_level(l, pair=p), c.get_now_level(l)):
                    assert g.shape == w.shape and np.array_equal(g.view(np.uint32), w.view(np.uint32))
                    assert not g.view(np.uint32).any()
        with pytest.raises(DvoError) as ei:                   # an empty reference list is refused as it is for a uniform frame
            a.frames_as_ref(0, 0, 3)
        assert ei.value.code == capi.DVO_ERR_INVALID and "no reference point" in str(ei.value)
        a.frames_set_pair_mask(-1, None)                      # and the context goes on: the unmasked bytes on the next upload
        upload(a, S, "cameras", rows, cols)
        N = a.frames_as_ref(0, 0, 3)
        assert (N > 0).all()
        for p in range(3):
            for l in range(NL):
                assert np.array_equal(a.frame_level(p, l, want_depth=False)[2], S["canny"][p][l])


def _first_step_stats(tr, S):
    R, t, ev = tr.step([0, 1, 2], [f[0] for f in S["frames"]], [f[1] for f in S["frames"]])
    assert list(ev) == [1, 1, 1]
    return tr.stats()


def _tracker(rows, cols):
    from rgbd_odometry_amd import DvoTracker
    tr = DvoTracker(3, iters=[4, 4, 4], rows=rows, cols=cols, n_levels=NL, first_shift=SHIFT)
    tr.set_intrinsics(*K)
    return tr


def test_launch_counts():
    from rgbd_odometry_amd import capi
    rows, cols = 96, 128
    S = scene(rows, cols)
    with _tracker(rows, cols) as never, _tracker(rows, cols) as removed, _tracker(rows, cols) as masked:
        base = _first_step_stats(never, S)
        removed.set_stream_mask(1, S["masks"][0])
        removed.set_stream_mask(1, None)
        assert _first_step_stats(removed, S) == base          # launches, synchronisations and runs of a tracker that never had one
        masked.set_stream_mask(2, S["masks"][2])
        st = _first_step_stats(masked, S)
        assert base["runs"] == st["runs"] and st["syncs"] == base["syncs"]
        assert st["launches"] == base["launches"] + capi.DVO_FRAMES_MASK_LAUNCHES      # one run = one chunk = one more launch


def test_refusals_leave_the_mask_in_force():
    from rgbd_odometry_amd import DvoContext, DvoError, capi
    rows, cols = 96, 128
    S = scene(rows, cols)
    m = S["masks"][0]
    with DvoContext(3) as a:
        a.frames_set_pair_mask(0, m, NL, SHIFT, MARGIN)
        planes = [a.frames_get_pair_mask_level(0, l) for l in range(NL)]
        bad = [dict(pair=3), dict(pair=-2), dict(n_levels=0), dict(n_levels=capi.DVO_MAX_LEVELS + 1), dict(first_shift=-1),
               dict(margin=-1), dict(margin=capi.DVO_MASK_MAX_MARGIN + 1), dict(n_levels=8, first_shift=2)]      # the last: an empty level
        for kw in bad:
            args = dict(pair=0, mask=np.ones((rows, cols), np.uint8), n_levels=NL, first_shift=SHIFT, margin=MARGIN)
            args.update(kw)
            with pytest.raises(DvoError) as ei:
                a.frames_set_pair_mask(**args)
            assert ei.value.code == capi.DVO_ERR_INVALID, kw
        for code, (r, c) in ((capi.DVO_ERR_INVALID, (0, cols)), (capi.DVO_ERR_INVALID, (rows, 0))):
            one = np.ones(1, np.uint8)
            assert a.lib.dvo_frames_set_pair_mask(a._h, 0, r, c, one.ctypes.data, NL, SHIFT, MARGIN) == code
        with pytest.raises(DvoError) as ei:
            a.frames_set_pair_mask(3, None)
        assert ei.value.code == capi.DVO_ERR_INVALID
        for l in range(NL):
            assert np.array_equal(a.frames_get_pair_mask_level(0, l), planes[l])
        upload(a, S, "cameras", rows, cols)
        stored = [a.frame_level(0, l, want_depth=False)[2] for l in range(NL)]
        for l in range(NL):
            assert np.array_equal(stored[l], S["canny"][0][l] & S["keep"][0][l])
        # a mask of another level geometry: the upload is refused and the store keeps its frames
        other = frame_gen.camera_frame(5, 64, 80)
        for call in (lambda: a.frames_upload_cameras([other[0]], [other[1]], n_levels=NL, first_shift=SHIFT, now_first_pair=0),
                     lambda: a.frames_upload_cameras([S["frames"][0][0]], [S["frames"][0][1]], n_levels=2, first_shift=SHIFT, now_first_pair=0),
                     lambda: a.frames_upload_pyramids([oracle_lib.load().build_pyramid(other[0], other[1], NL, SHIFT)], now_first_pair=0)):
            with pytest.raises(DvoError) as ei:
                call()
            assert ei.value.code == capi.DVO_ERR_INVALID and "mask" in str(ei.value)
            for l in range(NL):
                assert np.array_equal(a.frame_level(0, l, want_depth=False)[2], stored[l])
        # pair 1 has no mask: the same frame is accepted there (and the geometry change drops the store, as it always did)
        a.frames_upload_cameras([other[0]], [other[1]], n_levels=NL, first_shift=SHIFT, now_first_pair=1)
        # removal restores the unmasked bytes on the next upload
        a.frames_set_pair_mask(0, None)
        upload(a, S, "cameras", rows, cols)
        for l in range(NL):
            assert np.array_equal(a.frame_level(0, l, want_depth=False)[2], S["canny"][0][l])
