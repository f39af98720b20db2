"""Place descriptors and top-k key-frame retrieval of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_places,
dvo_tracker_archive_get_descriptor, dvo_tracker_query_places): what can be checked without a GPU -- the symbols in the header and in
the built library, the ctypes binding's argument types against the header's prototypes, the record's layout, the numpy reference's
own corner cases, and creation without a device."""
import ctypes as C
import os
import re

import numpy as np

import places_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvo_amd.h")
NEW = ["dvo_tracker_set_places", "dvo_tracker_archive_get_descriptor", "dvo_tracker_query_places"]


def prototypes():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert m, "%s is not declared in include/dvo_amd.h" % name
        out[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    return out


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    protos = prototypes()
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.C_ABI_SYMBOLS, name
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(protos[name]), (name, protos[name])
    for method in ("set_places", "archive_descriptor", "places"):
        assert callable(getattr(capi.DvoTracker, method)), method
    text = open(HEADER).read()
    for name, value in (("DVO_TRACKER_PLACE_STORE_LAUNCHES", 1), ("DVO_TRACKER_PLACE_QUERY_LAUNCHES", 2), ("DVO_TRACKER_PLACES_MAX_K", 32)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
        assert getattr(capi, name) == value, name


def ctype_of(decl):
    """the ctypes class a parameter declaration of the header maps to"""
    from rgbd_odometry_amd import capi
    d = decl.replace("const ", "")
    if "*" in d:
        base = d.split("*")[0].strip()
        return {"dvo_tracker": C.c_void_p, "int": C.POINTER(C.c_int), "unsigned char": C.POINTER(C.c_ubyte),
                "dvo_tracker_place": C.POINTER(capi.DvoTrackerPlace)}[base]
    return {"int": C.c_int, "long long": C.c_longlong}[d.rsplit(" ", 1)[0].strip()]


def test_binding_argument_types_follow_the_header():
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    for name, params in prototypes().items():
        want = [ctype_of(p) for p in params]
        got = list(getattr(lib, name).argtypes)
        assert [g.__name__ for g in got] == [w.__name__ for w in want], (name, params, got)
        assert all(C.sizeof(g) == C.sizeof(w) for g, w in zip(got, want)), name


def test_record_layout():
    from rgbd_odometry_amd import capi
    r = capi.DvoTrackerPlace
    assert [f[0] for f in r._fields_] == ["key_id", "frame", "stream", "distance"]
    assert (r.key_id.offset, r.frame.offset, r.stream.offset, r.distance.offset) == (0, 8, 16, 20)
    assert C.sizeof(r) == 24
    text = open(HEADER).read()
    m = re.search(r"typedef struct dvo_tracker_place \{(.*?)\} dvo_tracker_place;", text, re.S)
    assert m, "struct dvo_tracker_place is not in the header"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    assert [" ".join(x.split()) for x in body.split(";") if x.strip()] == ["long long key_id", "long long frame", "int stream", "unsigned distance"]


def test_reference_mean_rounds_half_up():
    # S / D = 100.5 exactly: m = 101, so 100 -> 127 and 101 -> 128;  S / D = 100.25: m = 100
    assert pr.descriptor(np.array([100, 101], np.uint8)).tolist() == [127, 128]
    assert pr.descriptor(np.array([100, 100, 100, 101], np.uint8)).tolist() == [128, 128, 128, 129]
    assert pr.descriptor(np.array([100, 100, 101, 101], np.uint8)).tolist() == [127, 127, 128, 128]
    assert pr.descriptor(np.full(7, 255, np.uint8)).tolist() == [128] * 7 and pr.descriptor(np.zeros(5, np.uint8)).tolist() == [128] * 5


def test_reference_clamps_at_both_ends():
    low = pr.descriptor(np.array([250] * 9 + [0], np.uint8))           # m = 225: 250 -> 153, 0 -> -97 -> 0
    assert low.tolist() == [153] * 9 + [0]
    high = pr.descriptor(np.array([5] * 9 + [255], np.uint8))          # m = 30: 5 -> 103, 255 -> 353 -> 255
    assert high.tolist() == [103] * 9 + [255]
    assert pr.descriptor(np.array([0, 255], np.uint8)).tolist() == [0, 255]      # m = 128: exactly the ends, no clamp needed


def test_reference_distance_and_order():
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, 256, 4941, dtype=np.uint8), rng.integers(0, 256, 4941, dtype=np.uint8)
    assert pr.distance(a, b) == pr.distance(b, a) > 0 and pr.distance(a, a) == 0
    assert pr.distance(np.zeros(19200, np.uint8), np.full(19200, 255, np.uint8)) == 19200 * 255 < 1 << 23
    # ties go to the smaller id, whatever the order of the rows; a row that is not allowed is never returned
    q = np.array([10, 10, 10, 10], np.uint8)
    rows = [np.array(r, np.uint8) for r in ([10, 10, 10, 12], [12, 10, 10, 10], [10, 10, 10, 10], [10, 11, 10, 10], [10, 10, 9, 10])]
    ids = [7, 3, 9, 5, 4]
    assert pr.top_k(q, rows, ids, [True, True, False, True, True], 3) == [(4, 1), (5, 1), (3, 2)]
    assert pr.top_k(q, rows, ids, [True] * 5, 8) == [(9, 0), (4, 1), (5, 1), (3, 2), (7, 2)]
    assert pr.top_k(q, rows[::-1], ids[::-1], [True] * 5, 2) == [(9, 0), (4, 1)]
    assert pr.column_major(np.array([[1, 2, 3], [4, 5, 6]], np.uint8)).tolist() == [1, 4, 2, 5, 3, 6]


def test_creation_without_a_device_fails_as_before():
    """places add nothing to creation: without a device the tracker is refused as it always was, with one it comes up with places off"""
    import torch
    from rgbd_odometry_amd import DvoError, DvoTracker
    from rgbd_odometry_amd.capi import DVO_ERR_NO_DEVICE, DVO_ERR_STATE
    if not torch.cuda.is_available():
        try:
            DvoTracker(4)
        except DvoError as e:
            assert e.code == DVO_ERR_NO_DEVICE and "no CPU fallback" in str(e)
        else:
            raise AssertionError("DvoTracker(4) came up without a device")
        return
    with DvoTracker(2) as tr:
        for call in (lambda: tr.set_places(0), lambda: tr.places([0], 1), lambda: tr.archive_descriptor(0)):
            try:
                call()
            except DvoError as e:
                assert e.code == DVO_ERR_STATE             # the archive is off, hence places are
            else:
                raise AssertionError("places are on by default")
