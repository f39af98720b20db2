"""Key-frame archive of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_archive / _score / _match): what can be checked
without a GPU -- the symbols in the header and in the built library, the ctypes binding's argument types against the header's
prototypes, the record's layout, and creation without a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvo_amd.h")
NEW = ["dvo_tracker_set_archive", "dvo_tracker_key_frame_id", "dvo_tracker_archive_info", "dvo_tracker_archive_get_points",
       "dvo_tracker_archive_stats", "dvo_tracker_score", "dvo_tracker_match"]


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
    for method in ("set_archive", "key_frame_id", "archive_info", "archive_points", "archive_stats", "score", "match"):
        assert callable(getattr(capi.DvoTracker, method)), method


def ctype_of(decl):
    """the ctypes class a parameter declaration of the header maps to"""
    from rgbd_odometry_amd import capi
    d = decl.replace("const ", "")
    if "*" in d:
        base = d.split("*")[0].strip()
        return {"dvo_tracker": C.c_void_p, "int": C.POINTER(C.c_int), "long long": C.POINTER(C.c_longlong), "double": C.c_void_p,
                "float": C.c_void_p, "dvo_tracker_score_record": C.POINTER(capi.DvoTrackerScoreRecord)}[base]
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
    r = capi.DvoTrackerScoreRecord
    assert [f[0] for f in r._fields_] == ["H36", "g6", "sum_eps2", "n_points", "n_visible"]
    assert (r.H36.offset, r.g6.offset, r.sum_eps2.offset, r.n_points.offset, r.n_visible.offset) == (0, 288, 336, 344, 348)
    assert C.sizeof(r) == 352
    text = open(HEADER).read()
    m = re.search(r"typedef struct dvo_tracker_score_record \{(.*?)\} dvo_tracker_score_record;", text, re.S)
    assert m, "struct dvo_tracker_score_record is not in the header"
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    assert [" ".join(x.split()) for x in body.split(";") if x.strip()] == ["double H36[36]", "double g6[6]", "double sum_eps2", "int n_points, n_visible"]
    assert re.search(r"#define DVO_TRACKER_MATCH_LAUNCHES 3\b", text) and re.search(r"#define DVO_TRACKER_ARCHIVE_LAUNCHES 1\b", text)


def test_creation_without_a_device_fails_as_before():
    """the archive adds nothing to creation: without a device the tracker is refused as it always was, with one it comes up with the
    archive off"""
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
        try:
            tr.key_frame_id(0)
        except DvoError as e:
            assert e.code == DVO_ERR_STATE                 # off by default
        else:
            raise AssertionError("the archive is on by default")
        assert tr.archive_stats() == dict(archived=0, refused=0, evicted=0, last_launches=0, last_syncs=0)
