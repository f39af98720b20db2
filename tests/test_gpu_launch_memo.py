"""enqueue()'s memo on the device (rgbd_odometry_amd/csrc/dvo_launch_memo.h, dvo_capi.cpp): a repeated request on unchanged host
state goes straight to the launch, and nothing a caller can see tells the difference.

Ground truth is always a context made with DVO_LAUNCH_MEMO=off that is driven through the same calls; after every enqueue the poses,
the level reports of every level, the final outputs and level_texel_mode of every pair are compared byte for byte (a getter that
refuses must refuse on both).  Every case runs with the memo on and under DVO_LAUNCH_MEMO=verify, where each remembered launch is
checked against a full pass inside the library (a difference is DVO_ERR_STATE)."""
import os

import numpy as np
import pytest

import frame_gen
import oracle_lib

ITERS = [3, 3, 3]
MODES = ["on", "verify"]


def _make(mode, n_pairs, **kw):
    from rgbd_odometry_amd import DvoContext
    old = os.environ.get("DVO_LAUNCH_MEMO")
    os.environ["DVO_LAUNCH_MEMO"] = mode          # read when the context is made
    try:
        return DvoContext(n_pairs, **kw)
    finally:
        if old is None:
            del os.environ["DVO_LAUNCH_MEMO"]
        else:
            os.environ["DVO_LAUNCH_MEMO"] = old


@pytest.fixture(scope="module")
def scenes(oracle):
    """four 160x120x3 scenes with their float levels (three are installed, the fourth replaces one), a camera pyramid of the same
    sizes for the frame store, and four 80x60x2 scenes for the batch of more pairs than compute units"""
    from rgbd_odometry_amd import SynthScene
    sc = [SynthScene(160, 120, 3, 40 + i) for i in range(4)]
    lv = [oracle_lib.scene_levels(s, oracle) for s in sc]
    bgr, depth = frame_gen.camera_frame(21, 120, 160)
    pyr = oracle.build_pyramid(bgr, depth, 3, 0)
    small = [SynthScene(80, 60, 2, 60 + i) for i in range(4)]
    return dict(sc=sc, lv=lv, pyr=pyr, small=small)


def _edges(a):
    return (np.asarray(a) != 0).astype(np.uint8) * 255


def _install(ctx, sc_list, n_src, float_now=None):
    """pairs 0 .. n_src-1 from the scenes, the rest replicated; float_now: their float levels instead of the edge maps"""
    ctx.set_intrinsics(*sc_list[0].intrinsics)
    for i in range(n_src):
        for l, L in enumerate(sc_list[i].levels):
            ctx.set_ref_level_from_images(l, L.ref_edge, L.ref_depth, L.rows, L.cols, pair=i)
            if float_now is not None:
                F = float_now[i][l]
                ctx.set_now_level(l, F["dt"], F["gx"], F["gy"], F["rows"], F["cols"], pair=i)
            else:
                ctx.set_now_level_from_edges(l, _edges(L.now_edge), L.rows, L.cols, pair=i)
    if ctx.n_pairs > n_src:
        ctx.replicate_pairs(n_src)


def _snapshot(ctx, iters, cap):
    """everything a caller can read after an enqueue, as bytes; a refusal as its error code"""
    from rgbd_odometry_amd import DvoError
    n = ctx.n_pairs
    R = np.zeros((n, 3, 3)); t = np.zeros((n, 3))
    ctx._chk(ctx.lib.dvo_get_poses(ctx._h, 0, n, R.ctypes.data, t.ctypes.data))
    out = [("poses", R.tobytes(), t.tobytes())]
    for p in range(n):
        for l in range(len(iters)):
            try:
                e, b, r = ctx.level_report(p, l, max(iters[l], 1))
                out.append(("report", p, l, e.tobytes(), b, np.float32(r).tobytes()))
            except DvoError as err:
                out.append(("report", p, l, "refused", err.code))
            out.append(("mode", p, l, ctx.level_texel_mode(p, l)))
        try:
            fe, fr = ctx.final_outputs(p, cap)
            out.append(("final", p, fe.tobytes(), fr.tobytes()))
        except DvoError as err:
            out.append(("final", p, "refused", err.code))
    return out


def _pair(mode, n_pairs, install, **kw):
    """the context under test and its ground truth, installed alike"""
    a, b = _make(mode, n_pairs, **kw), _make("off", n_pairs, **kw)
    for c in (a, b):
        install(c)
    return a, b


def _enqueue_same(a, b, iters, cap, what, **kw):
    """the same enqueue on both; their outputs must be the same bytes; returns the memo context's counts"""
    for c in (a, b):
        c.enqueue(iters, **kw)
    sa, sb = _snapshot(a, iters, cap), _snapshot(b, iters, cap)
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert x == y, (what, x[:3])
    full_off, hits_off = b.enqueue_counts()
    assert hits_off == 0, what                    # DVO_LAUNCH_MEMO=off never remembers
    return a.enqueue_counts()


def _flags():
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS, DVO_FLAG_IDENTITY_START
    return DVO_FLAG_IDENTITY_START | DVO_FLAG_FINAL_OUTPUTS, DVO_FLAG_FINAL_OUTPUTS


CAP = 160 * 120


def _six(scenes):
    return lambda c: _install(c, scenes["sc"], 3)


# ---- 1. repeat ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("batch", ["six", "more_pairs_than_cus"])
def test_repeat(scenes, mode, batch):
    ident, carry = _flags()
    if batch == "six":
        a, b = _pair(mode, 6, _six(scenes))
        iters, cap = ITERS, CAP
    else:                                       # 320 pairs: the launch goes through the resident order
        a, b = _pair(mode, 320, lambda c: _install(c, scenes["small"], 4))
        iters, cap = [3, 3], 80 * 60
    with a, b:
        n = a.n_pairs
        for k in range(3):
            counts = _enqueue_same(a, b, iters, cap, ("identical", k), flags=ident)
            assert counts == (1, k), (k, counts)
        assert a.last_launch_shape() == b.last_launch_shape()
        # device data is not host state: new start poses between the calls, still remembered launches
        rng = np.random.default_rng(5)
        want = [(2, 2), (2, 3), (2, 4)]
        for k in range(3):
            if k < 2:
                w = rng.normal(size=(n, 3)) * 1e-3
                R = np.stack([_rot(v) for v in w])
                t = rng.normal(size=(n, 3)) * 1e-3
                for c in (a, b):
                    c.set_poses(R, t)
            counts = _enqueue_same(a, b, iters, cap, ("set_poses", k), flags=carry)      # k == 2: carries on from its own result
            assert counts == want[k], (k, counts)


def _rot(w):
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


# ---- 2. the key --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_key(scenes, mode):
    ident, _ = _flags()
    from rgbd_odometry_amd.capi import DVO_FLAG_IDENTITY_START
    a, b = _pair(mode, 6, _six(scenes))
    with a, b:
        assert _enqueue_same(a, b, ITERS, CAP, "first", flags=ident) == (1, 0)
        assert _enqueue_same(a, b, ITERS, CAP, "second", flags=ident) == (1, 1)
        others = [("iters", dict(iters=[3, 2, 3], flags=ident)),
                  ("flags", dict(iters=ITERS, flags=DVO_FLAG_IDENTITY_START)),
                  ("first_pair", dict(iters=ITERS, flags=ident, first_pair=1)),
                  ("n_pairs", dict(iters=ITERS, flags=ident, n_pairs=5))]
        for what, kw in others:
            full0, hits0 = a.enqueue_counts()
            it = kw.pop("iters")
            full1, hits1 = _enqueue_same(a, b, it, CAP, what, **kw)
            assert (full1, hits1) == (full0 + 1, hits0), what                   # another request: a full pass
            full2, hits2 = _enqueue_same(a, b, ITERS, CAP, what + ", back", flags=ident)      # correct either way
            assert full2 + hits2 == full1 + hits1 + 1


# ---- 3. mutators -------------------------------------------------------------------------------------------------------------------

def _mut_ref_images(c, S):
    for l, L in enumerate(S["sc"][3].levels):          # another scene: another point count
        c.set_ref_level_from_images(l, L.ref_edge, L.ref_depth, L.rows, L.cols, pair=1)


def _mut_ref_float(c, S):
    for l, F in enumerate(S["lv"][0]):                 # a caller's 3 x N list
        c.set_ref_level(l, np.asarray(F["xyz"])[::2].copy(), pair=0)


def _mut_now_edges(c, S):
    for l, L in enumerate(S["sc"][3].levels):
        c.set_now_level_from_edges(l, _edges(L.now_edge), L.rows, L.cols, pair=2)


def _mut_now_float(c, S):
    for l, F in enumerate(S["lv"][3]):
        c.set_now_level(l, F["dt"], F["gx"], F["gy"], F["rows"], F["cols"], pair=4)


def _mut_frames_now(c, S):
    c.frames_as_now(0, 1, 1)


def _mut_frames_ref(c, S):
    c.frames_as_ref(0, 5, 1)


MUTATORS = {
    "set_ref_level_from_images": _mut_ref_images,
    "set_ref_level": _mut_ref_float,
    "set_now_level_from_edges": _mut_now_edges,
    "set_now_level": _mut_now_float,
    "replicate_pairs": lambda c, S: c.replicate_pairs(2, 3, 3),
    "set_intrinsics": lambda c, S: c.set_intrinsics(*[float(np.float32(k) * np.float32(1.01)) for k in S["sc"][0].intrinsics]),
    "now_prepare": lambda c, S: c.now_prepare(),
    "set_direct_compact": lambda c, S: c.set_direct_compact(True),
    "frames_as_now": _mut_frames_now,
    "frames_as_ref": _mut_frames_ref,
}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mutator", list(MUTATORS))
def test_mutator_forces_a_full_pass(scenes, mode, mutator):
    ident, _ = _flags()

    def install(c):
        _install(c, scenes["sc"], 3)
        c.frames_reserve(1)
        c.frames_upload_pyramids([scenes["pyr"]])

    a, b = _pair(mode, 6, install)
    with a, b:
        assert _enqueue_same(a, b, ITERS, CAP, "first", flags=ident) == (1, 0)
        assert _enqueue_same(a, b, ITERS, CAP, "second", flags=ident) == (1, 1)
        for c in (a, b):
            MUTATORS[mutator](c, scenes)
        assert _enqueue_same(a, b, ITERS, CAP, "after " + mutator, flags=ident) == (2, 1), mutator
        full, hits = _enqueue_same(a, b, ITERS, CAP, "again after " + mutator, flags=ident)
        assert full + hits == 4


# ---- 4. outputs stay valid ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_outputs_between_remembered_calls(scenes, mode):
    ident, _ = _flags()
    a, b = _pair(mode, 6, _six(scenes))
    with a, b:
        assert _enqueue_same(a, b, ITERS, CAP, "first", flags=ident) == (1, 0)
        assert _enqueue_same(a, b, ITERS, CAP, "second", flags=ident) == (1, 1)
        # another schedule on a sub-range: the other pairs' reports sit at other offsets now -- both contexts refuse them alike
        _enqueue_same(a, b, [2, 0, 4], CAP, "sub-range", flags=ident, first_pair=2, n_pairs=3)
        assert _snapshot(a, ITERS, CAP) == _snapshot(b, ITERS, CAP)
        _enqueue_same(a, b, ITERS, CAP, "base after the sub-range", flags=ident)
        _enqueue_same(a, b, ITERS, CAP, "base, repeated", flags=ident)
        wide = [c.align_pyramid_wide(ITERS, np.eye(3), np.zeros(3), pair=1) for c in (a, b)]
        assert all(np.array_equal(x, y) for x, y in zip(wide[0], wide[1]))
        assert _snapshot(a, ITERS, CAP) == _snapshot(b, ITERS, CAP)
        _enqueue_same(a, b, ITERS, CAP, "base after the wide alignment", flags=ident)
        _enqueue_same(a, b, ITERS, CAP, "base, repeated again", flags=ident)
        one = [c.run_iterations(1, 3, np.eye(3), np.zeros(3), pair=0) for c in (a, b)]
        assert np.array_equal(one[0]["energy"], one[1]["energy"]) and np.array_equal(one[0]["R"], one[1]["R"])
        assert _snapshot(a, ITERS, CAP) == _snapshot(b, ITERS, CAP)
        _enqueue_same(a, b, ITERS, CAP, "base after run_iterations", flags=ident)
        full, hits = _enqueue_same(a, b, ITERS, CAP, "base, at the end", flags=ident)
        assert hits >= 2, (full, hits)


# ---- 5. the use count of a form that is not built yet --------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_use_count_still_builds_the_compact_form(scenes, mode):
    import re
    ident, _ = _flags()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dvo_amd.h")).read()
    after = int(re.search(r"#define\s+DVO_COMPACT_NOW_AFTER\s+(\d+)", header).group(1))

    def install(c):
        c.set_direct_compact(False)
        _install(c, scenes["sc"], 3, float_now=scenes["lv"])

    a, b = _pair(mode, 6, install)
    with a, b:
        modes, counts = [], []
        for k in range(after + 2):
            counts.append(_enqueue_same(a, b, ITERS, CAP, ("call", k), flags=ident))      # texel modes compared per call in there
            modes.append(a.level_texel_mode(0, 0))
        switch = modes.index(2)                  # the call that first read the compact form
        assert modes[:switch] == [m for m in modes[:switch] if m != 2] and all(m == 2 for m in modes[switch:])
        assert switch == after, (switch, modes)
        assert counts[switch] == (switch + 1, 0), counts         # no hit up to and including the call that built the form
        assert counts[-1] == (switch + 1, len(modes) - switch - 1), counts
