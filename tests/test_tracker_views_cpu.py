"""CPU checks of the tracker's views (include/dvo_amd.h: dvo_tracker_set_views ...): the jet map's closed form, the numpy composer the
GPU tests compare with (tests/views_reference.py) on a hand-made level, and the agreement of header, binding, C++ mirror and library
on the five calls."""
import os
import re

import numpy as np

import views_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["dvo_tracker_set_views", "dvo_tracker_get_residue_histogram", "dvo_tracker_view_size", "dvo_tracker_get_view",
           "dvo_tracker_view_device"]


def test_jet_closed_form():
    want = {0: (143, 0, 0), 7: (255, 0, 0), 23: (255, 255, 0), 39: (0, 255, 255), 55: (0, 0, 255), 63: (0, 0, 127)}
    for i, c in want.items():
        assert vr.jet(i) == c, (i, vr.jet(i))
    table = [vr.jet(i) for i in range(64)]
    assert len(set(table)) == 64                                          # 64 distinct colours
    assert all(0 <= x <= 255 for c in table for x in c)
    # the shape of a jet map: blue rises then falls, red rises last, every channel moves in steps of 16 (one of 15 at the saturation)
    for ch in range(3):
        steps = {abs(table[i + 1][ch] - table[i][ch]) for i in range(63)}
        assert steps <= {0, 15, 16}, (ch, steps)
    assert vr.JET.shape == (64, 3) and vr.JET.dtype == np.uint8
    from rgbd_odometry_amd import capi
    assert [capi.jet_colour(i) for i in range(64)] == table


def test_composer_on_a_hand_made_level():
    rows, cols = 6, 8
    DT = np.full((rows, cols), 7.0, np.float32)
    DT[0, 0], DT[0, 1], DT[0, 2] = 0.5, 1.5, 2.5                          # half to even: 0, 2, 2
    DT[1, 0], DT[1, 1], DT[1, 2] = 60.0, 60.5, 255.0
    DT[2, 7] = 3.25
    DT[5, 0] = 300.0                                                      # saturates
    dt_cm = np.ascontiguousarray(DT.T).ravel()
    grey = (np.arange(rows * cols, dtype=np.uint8) * 5).reshape(rows, cols)
    below = np.nextafter(np.float32(cols), np.float32(0))                # cols - eps
    pts = [                       # (u, v)
        (below, 2.0),             # the last column, visible
        (np.float32(cols), 2.0),  # u == cols: the reference would write outside its mask; invisible here
        (3.2, 4.9), (3.9, 4.1),   # two points on pixel (4, 3)
        (0.0, 1.0), (1.99, 1.0), (2.5, 1.5),      # d = 60.0, 60.5, 255
        (0.0, 0.0),               # d = 0.5
        (-0.0001, 3.0), (2.0, np.float32(rows)), (np.nan, 1.0),          # invisible
    ]
    u, v = (np.array([p[k] for p in pts], np.float32) for k in (0, 1))
    out = vr.compose_views(u, v, dt_cm, grey, rows, cols)
    assert out["visible"].tolist() == [True, False, True, True, True, True, True, True, False, False, False]
    assert out["eps"].tolist() == [3.25, 0.0, 7.0, 7.0, 60.0, 60.5, 255.0, 0.5, 0.0, 0.0, 0.0]
    hist = np.zeros(260, np.uint32)
    for b, n in {4: 1, 1: 5, 8: 2, 61: 2, 256: 1}.items():               # bin 1: four invisible points and d = 0.5
        hist[b] = n
    assert np.array_equal(out["hist"], hist) and out["hist"].sum() == len(pts) and out["hist"][0] == 0
    marked = [(2, 7), (4, 3), (1, 0), (1, 1), (1, 2), (0, 0)]
    assert sorted(map(tuple, np.argwhere(out["marked"]))) == sorted(marked)
    for y, x in marked:
        assert tuple(out["reproj"][y, x]) == (0, 255, 0)
    assert tuple(out["reproj"][0, 1]) == (2, 2, 2) and tuple(out["reproj"][0, 2]) == (2, 2, 2)      # 1.5 -> 2, 2.5 -> 2
    assert tuple(out["reproj"][5, 0]) == (255, 255, 255) and tuple(out["reproj"][3, 3]) == (7, 7, 7)
    want_heat = {(2, 7): vr.jet(3), (4, 3): vr.jet(7), (1, 0): vr.jet(60), (1, 1): vr.jet(63), (1, 2): vr.jet(63), (0, 0): vr.jet(0)}
    for (y, x), c in want_heat.items():
        assert tuple(out["heat"][y, x]) == c, (y, x)
    free = ~out["marked"]
    assert np.array_equal(out["heat"][free], vr.grey3(grey)[free])
    plain = vr.unmarked(dt_cm, grey, rows, cols)
    assert np.array_equal(out["reproj"][free], plain[0][free]) and plain[0][0, 0].tolist() == [0, 0, 0]       # 0.5 -> 0


def test_header_library_and_binding_have_the_calls():
    from rgbd_odometry_amd import capi
    text = open(os.path.join(ROOT, "include", "dvo_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(dvo_[a-z0-9_]+)\s*\(", src))
    lib = capi.load_library()
    for name in SYMBOLS:
        assert name in declared and name in capi.C_ABI_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for macro, value in (("DVO_VIEW_REPROJ_ON_DT", 0), ("DVO_VIEW_RESIDUE_HEAT", 1), ("DVO_TRACKER_VIEW_LAUNCHES", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), src), macro
        assert getattr(capi, macro) == value
    for name in ("set_views", "residue_histogram", "view", "view_size", "view_device"):
        assert callable(getattr(capi.DvoTracker, name)), name
    hpp = open(os.path.join(ROOT, "include", "dvo_amd.hpp")).read()
    for name in ("void enableViews(bool", "lastResidueHistogram(int", "lastView(int", "jetColour(int"):
        assert name in hpp, name
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in SYMBOLS:
        assert name in integration, name
    # refused before anything is touched
    assert lib.dvo_tracker_set_views(None, 1) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_get_residue_histogram(None, 0, None, None, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_view_size(None, None, None, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_get_view(None, 0, 0, None) == capi.DVO_ERR_INVALID
    assert lib.dvo_tracker_view_device(None, 0, 0, None) == capi.DVO_ERR_INVALID
