"""Export and import of the key-frame archive (include/dvo_amd.h: dvo_tracker_archive_export, dvo_tracker_archive_import,
dvo_tracker_archive_origin; kernels in dvo_tracker_archive_blob.hip).

Geometry and helpers of tests/test_gpu_tracker_information.py and tests/test_gpu_tracker_archive.py: 240 x 320, 3 levels, 8 iterations
each, one launch shape everywhere, 3 streams and 7 ticks (tick 5 is the forced key-frame switch); stream 0's last frame is generated
with shift (0, 0) again.  Tracker A makes six key frames with descriptors at level 2; tracker B has ONE stream and another ring
capacity and takes them from A's blob.

Expected values are integers and byte strings throughout: the blob against tests/archive_blob_reference.py (numpy, written from the
header's text), an imported key frame against the original in A -- points, descriptor, and every record score, match, verify, the query
and the shift search give for it, bit for bit: the same kernels read the same words -- and B's tracking against a twin that never
imported."""
import ctypes

import numpy as np
import pytest

import archive_blob_reference as br
import frame_gen
import frame_reference as fr
import test_gpu_tracker_archive as TA
import test_gpu_tracker_information as TI
import test_gpu_tracker_places as TP
from test_gpu_tracker_streams import DEMO_IT, DEMO_N, DEMO_NL, demo_args, demo_run  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT, K = TI.ROWS, TI.COLS, TI.NL, TI.SHIFT, TI.K
N_S, N_T, FULL, LEVEL = TA.N_S, TA.N_T, TA.FULL, TP.LEVEL
EXPORT_COST, IMPORT_COST = (1, 1), (2, 1)              # (launches, synchronisations): DVO_TRACKER_EXPORT_LAUNCHES / _IMPORT_LAUNCHES
step, refused, same_bits = TA.step, TA.refused, TA.same_bits
EYE, ZERO = np.eye(3), np.zeros(3)


@pytest.fixture(scope="module")
def seqs():
    out = [TI.sequence(900 + s, N_T, TI.MOTIONS[s]) for s in range(N_S)]
    out[0][N_T - 1] = frame_gen.camera_frame(900, ROWS, COLS, shift=(0, 0), holes=True)       # stream 0 comes back to where it started
    return out


def cost(tr):
    st = tr.archive_stats()
    return st["last_launches"], st["last_syncs"]


def counters(tr):
    st = tr.archive_stats()
    return st["archived"], st["refused"], st["evicted"]


def key_frame(tr, kid, with_desc=True):
    """everything the tracker tells about an archived key frame"""
    return dict(info=tr.archive_info(kid), origin=tr.archive_origin(kid), points=[tr.archive_points(kid, l) for l in range(tr.n_levels)],
                desc=tr.archive_descriptor(kid) if with_desc else None)


def same_key_frame(a, b):
    return (a["info"]["n_points"] == b["info"]["n_points"] and a["origin"] == b["origin"] and
            all(same_bits(p, q) for p, q in zip(a["points"], b["points"])) and
            ((a["desc"] is None and b["desc"] is None) or same_bits(a["desc"], b["desc"])))


@pytest.fixture(scope="module")
def world(seqs):
    """A after the 7-tick run (ids 0..5: the first frames, then the tick-5 switches), its blob, and B: one stream, 16 slots, fed the
    frame A's stream 0 had last, then given the blob"""
    A = TP.make(N_S)
    for entry in FULL:
        step(A, seqs, entry)
    ids = list(range(2 * N_S))
    originals = {i: key_frame(A, i) for i in ids}
    size = A.export_size()
    blob = A.export_archive()
    export_cost = cost(A)
    B = TP.make(1, archive=(16, 4, None))
    step(B, seqs, [(0, N_T - 1)])
    before = counters(B)
    new_ids = B.import_archive(blob)
    import_cost = cost(B)
    yield dict(A=A, B=B, ids=ids, originals=originals, size=size, blob=blob, new_ids=new_ids, export_cost=export_cost, import_cost=import_cost,
               before=before)
    A.close()
    B.close()


def test_export_against_the_reference(world):
    from rgbd_odometry_amd import capi
    A, blob, ids = world["A"], world["blob"], world["ids"]
    assert world["size"] == len(blob) and world["export_cost"] == EXPORT_COST
    info, kfs = br.parse(blob)                             # validates header, table and every payload checksum by recomputation
    assert info == dict(version=1, rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, places_level=LEVEL, D=len(world["originals"][0]["desc"]),
                        n_key_frames=len(ids), total_bytes=len(blob))
    assert capi.archive_blob_info(blob) == info
    records = br.validate(blob)[1]
    for i, (kid, kf, r) in enumerate(zip(ids, kfs, records)):
        want = world["originals"][kid]
        assert (kf["origin_id"], kf["origin_stream"], kf["origin_frame"]) == (kid, want["info"]["stream"], want["info"]["frame"]), kid
        assert want["origin"] == dict(id=kid, stream=want["info"]["stream"], frame=want["info"]["frame"])      # a native key frame is its own origin
        assert kf["K"].tobytes() == np.array(K, np.float32).tobytes()
        assert r["N"][:NL] == want["info"]["n_points"] and r["N"][NL:] == [0] * (br.MAX_LEVELS - NL) and r["has_desc"] == 1
        assert r["payload_checksum"] == br.checksum(blob[r["payload_offset"]:r["payload_offset"] + r["payload_bytes"]])
        assert np.array_equal(kf["desc"], want["desc"])
        for l, L in enumerate(kf["levels"]):
            N = len(want["points"][l])
            assert N > 64 and np.array_equal(np.sort(L["cidx"]), np.arange(N)), (kid, l)      # block order -> list order: a permutation
            assert L["pt4_ok"] in (0, 1) and (L["pt4_ok"] or not (L["cpt4"].any() or L["chdr"].any()))
    assert any(r["N"][l] % 64 for r in records for l in range(NL))                  # ragged last chunks are in play
    # deterministic; a subset comes out in the listed order, with the payloads of the full export
    assert A.export_archive() == blob and cost(A) == EXPORT_COST
    sub = A.export_archive([2, 0])
    assert len(sub) == A.export_size([2, 0])
    sub_records = br.validate(sub)[1]
    assert [r["origin_id"] for r in sub_records] == [2, 0]
    for r, kid in zip(sub_records, (2, 0)):
        full = records[kid]
        assert sub[r["payload_offset"]:r["payload_offset"] + r["payload_bytes"]] == blob[full["payload_offset"]:full["payload_offset"] + full["payload_bytes"]]
        assert r["payload_checksum"] == full["payload_checksum"]
    twice = br.validate(A.export_archive([1, 1]))[1]                                # duplicates are allowed
    assert [r["origin_id"] for r in twice] == [1, 1] and twice[0]["payload_offset"] != twice[1]["payload_offset"]
    assert br.validate(A.export_archive([]))[0]["n_key_frames"] == 0


def test_import_into_another_tracker(world):
    A, B, blob, ids, new_ids = world["A"], world["B"], world["blob"], world["ids"], world["new_ids"]
    assert world["import_cost"] == IMPORT_COST
    assert new_ids == [1 + i for i in ids]                 # fresh ids: B's own first key frame is 0
    assert world["before"] == (1, 0, 0) and counters(B)[0] >= 1 + len(ids)
    for kid, nid in zip(ids, new_ids):
        want, got = world["originals"][kid], key_frame(B, nid)
        assert got["info"]["stream"] == -1 and got["info"]["frame"] == want["info"]["frame"], (kid, got["info"])
        assert got["origin"] == dict(id=kid, stream=want["info"]["stream"], frame=want["info"]["frame"])
        assert same_key_frame(want, got), kid
    assert B.archive_origin(0) == dict(id=0, stream=0, frame=0)
    # the round trip: B's re-export of the imported ids is A's export, byte for byte
    assert B.export_archive(new_ids) == blob
    assert B.export_archive(new_ids[::-1]) == A.export_archive(ids[::-1])


def test_imported_key_frames_serve_like_the_originals(world):
    """B's stream 0 holds the now levels A's stream 0 holds (the same frame through the same frame stage): every record on an imported
    key frame is A's on the original, with the same n and the same launch shape"""
    A, B, ids, new_ids = world["A"], world["B"], world["ids"], world["new_ids"]
    for first in (0, 3):                                   # max_matches = 4: two calls of three candidates
        a_ids, b_ids, s = ids[first:first + 3], new_ids[first:first + 3], [0, 0, 0]
        R, t = np.stack([EYE] * 3), np.zeros((3, 3))
        for level in (0, 2):
            for ra, rb in zip(A.score(s, a_ids, level, R, t), B.score(s, b_ids, level, R, t)):
                assert TA.same_record(ra, rb) and ra["n_visible"] > 6, (first, level)
            va, vb = A.verify(s, a_ids, level, R, t), B.verify(s, b_ids, level, R, t)
            assert va == vb and all(v["n_depth"] > 0 for v in va), (first, level, va, vb)
        # the shift search, and from its shifts the guesses
        sa, sb = A.place_shifts(s, a_ids, 4), B.place_shifts(s, b_ids, 4)
        assert sa == sb, (first, sa, sb)
        guesses = [A.place_guess(0, r["dy"], r["dx"]) for r in sa]
        assert all(same_bits(g[0], h[0]) for g, h in zip(guesses, [B.place_guess(0, r["dy"], r["dx"]) for r in sb]))
        for R0, t0 in ((None, None), (np.stack([g[0] for g in guesses]), np.stack([g[1] for g in guesses]))):
            Ra, ta, reca = A.match(s, a_ids, R0, t0)
            Rb, tb, recb = B.match(s, b_ids, R0, t0)
            assert same_bits(Ra, Rb) and same_bits(ta, tb), (first, R0 is None)
            assert all(TA.same_record(x, y) for x, y in zip(reca, recb))
    # the query: imported key frames are foreign (stream -1), so only B's own current key frame is excluded; A excludes stream 0's
    rows_a = {e["key_id"]: e for e in A.places([0], 8)[0]}
    rows_b = B.places([0], 8)[0]
    assert [e["stream"] for e in rows_b] == [-1] * len(ids) and sorted(e["key_id"] for e in rows_b) == new_ids
    zero_radius = {k: r["sad"] for k, r in zip(ids, A.place_shifts([0] * 3, ids[:3], 0) + A.place_shifts([0] * 3, ids[3:], 0))}
    own = A.key_frame_id(0)
    assert sorted(rows_a) == [k for k in ids if k != own]
    for e in rows_b:
        kid = e["key_id"] - 1
        assert e["frame"] == world["originals"][kid]["info"]["frame"]
        assert e["distance"] == zero_radius[kid] and (kid == own or e["distance"] == rows_a[kid]["distance"]), (kid, e)
    assert [(e["distance"], e["key_id"]) for e in rows_b] == sorted((e["distance"], e["key_id"]) for e in rows_b)
    assert B.places([0], 8, min_frame_gap=1000)[0] == rows_b                        # rule (c) never applies to a foreign key frame


def test_tracking_is_that_of_a_twin_that_never_imported(world, seqs):
    frames = [(0, N_T - 1), (0, 1), (0, 2), (0, 3)]
    with TP.make(1, archive=(16, 4, None)) as B, TP.make(1, archive=(16, 4, None)) as twin:
        for n, f in enumerate(frames):
            if n == 2:
                assert len(B.import_archive(world["blob"])) == len(world["ids"]) and cost(B) == IMPORT_COST
            got, want = step(B, seqs, [f]), step(twin, seqs, [f])
            assert all(same_bits(a, b) for a, b in zip(got, want)), n
            assert B.stats() == twin.stats(), (n, B.stats(), twin.stats())
            assert TI.same_record(B.information(0), twin.information(0)), n
        assert B.key_frame_id(0) == twin.key_frame_id(0) == 0


def test_ring(world, seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    blob, ids = world["blob"], world["ids"]
    # six key frames into four slots: the blob evicts its own first two
    with TP.make(1, archive=(4, 4, None)) as B:
        got = B.import_archive(blob)
        assert got == ids and counters(B) == (6, 0, 2)
        for nid in got[:2]:
            refused(DVO_ERR_STATE, B.archive_info, nid)
            refused(DVO_ERR_STATE, B.archive_origin, nid)
        for nid in got[2:]:
            assert same_key_frame(world["originals"][nid], key_frame(B, nid)), nid
        assert B.export_archive() == world["A"].export_archive(ids[2:])
        # ... and a second import evicts the first one's
        again = B.import_archive(world["A"].export_archive([1, 0]))
        assert again == [6, 7] and counters(B) == (8, 0, 4)
        assert [r["origin_id"] for r in br.validate(B.export_archive())[1]] == [4, 5, 1, 0]
    # a tracker takes its own export: new ids, the same origin
    with TP.make(1) as C:
        step(C, seqs, [(0, 0)])
        own = key_frame(C, 0)
        assert C.import_archive(C.export_archive()) == [1] and counters(C) == (2, 0, 0)
        copy = key_frame(C, 1)
        assert copy["info"]["stream"] == -1 and copy["origin"] == own["origin"] == dict(id=0, stream=0, frame=0) and same_key_frame(own, copy)
        assert C.key_frame_id(0) == 0


def test_partial_refusal(world):
    n0 = [world["originals"][k]["info"]["n_points"][0] for k in world["ids"]]
    cap = max(n0) - 1
    want_refused = [i for i, n in enumerate(n0) if n > cap]
    assert 1 <= len(want_refused) < len(n0), n0
    with TP.make(1, archive=(16, 4, [cap, 0, 0])) as B:
        got = B.import_archive(world["blob"])
        assert [i for i, g in enumerate(got) if g == -1] == want_refused
        assert [g for g in got if g >= 0] == list(range(len(n0) - len(want_refused)))
        assert counters(B) == (len(n0) - len(want_refused), len(want_refused), 0)
        for kid, nid in zip(world["ids"], got):
            if nid >= 0:
                assert same_key_frame(world["originals"][kid], key_frame(B, nid)), kid


def test_whole_blob_refusals_change_nothing(world):
    from rgbd_odometry_amd import DvoTracker, capi
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE
    blob = world["blob"]
    with TP.make(1, archive=(16, 4, None)) as B:
        B.import_archive(world["A"].export_archive([0, 1]))

        def state():
            return B.archive_stats(), [B.archive_info(i) for i in (0, 1)], B.export_archive(), B.stats()

        before = state()
        before = state()                                   # the export's own cost is part of the stats: take it twice
        flipped = bytearray(blob)
        flipped[br.validate(blob)[1][3]["payload_offset"] + 100] ^= 0x04
        assert capi.archive_blob_info(bytes(flipped))["n_key_frames"] == len(world["ids"])      # header and table are fine: only the device sees it
        with pytest.raises(capi.DvoError) as ei:
            B.import_archive(bytes(flipped))
        assert ei.value.code == DVO_ERR_INVALID and "key frame 3" in str(ei.value) and "payload checksum" in str(ei.value), str(ei.value)
        refused(DVO_ERR_INVALID, B.import_archive, blob[:-16])
        refused(DVO_ERR_INVALID, B.import_archive, blob[:100])
        refused(DVO_ERR_INVALID, B.import_archive, b"")
        # a too-small export capacity: the need is reported, nothing is written
        lib, need = capi.load_library(), ctypes.c_size_t()
        buf = np.full(64, 0xAB, np.uint8)
        assert lib.dvo_tracker_archive_export(B._h, 0, None, capi._ptr(buf), buf.size, ctypes.byref(need)) == DVO_ERR_INVALID
        assert need.value == len(before[2]) and (buf == 0xAB).all()
        refused(DVO_ERR_STATE, B.export_archive, [5])      # never given
        refused(DVO_ERR_STATE, B.export_archive, [-1])
        assert lib.dvo_tracker_archive_export_size(B._h, -1, (ctypes.c_longlong * 1)(0), ctypes.byref(need)) == DVO_ERR_INVALID
        after = state()
        assert before == after
    # another geometry
    for kw in (dict(n_levels=2, iters=[8, 8]), dict(rows=ROWS - 8), dict(first_shift=1)):
        args = dict(dict(rows=ROWS, cols=COLS, n_levels=NL, first_shift=SHIFT, iters=TI.ITERS), **kw)
        with DvoTracker(1, **args) as C:
            C.set_intrinsics(*K)
            C.set_archive(8, 1)
            refused(DVO_ERR_INVALID, C.import_archive, blob)
            assert C.archive_stats() == dict(archived=0, refused=0, evicted=0, last_launches=0, last_syncs=0), kw
            assert br.validate(C.export_archive())[0]["n_key_frames"] == 0
    with TA.make(1, archive=None) as C:                    # the archive off
        refused(DVO_ERR_STATE, C.import_archive, blob)
        refused(DVO_ERR_STATE, C.export_archive)
        refused(DVO_ERR_STATE, C.export_size)
        refused(DVO_ERR_STATE, C.archive_origin, 0)


def test_places_must_agree_for_descriptors_to_travel(world, seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    blob, ids = world["blob"], world["ids"]
    for places in (None, 1):                               # off; on at another level
        with TP.make(1, archive=(16, 4, None), places=places) as B:
            step(B, seqs, [(0, N_T - 1)])
            got = B.import_archive(blob)
            assert got == [1 + i for i in ids] and cost(B) == IMPORT_COST
            for kid, nid in zip(ids, got):
                refused(DVO_ERR_STATE, B.archive_descriptor, nid)
                assert same_key_frame(dict(world["originals"][kid], desc=None), key_frame(B, nid, with_desc=False))
            if places is not None:
                assert B.places([0], 8) == [[]]            # its own key frame is excluded, the imported ones have no descriptor
                refused(DVO_ERR_STATE, B.place_shifts, [0], [got[0]], 0)
            again = br.validate(B.export_archive(got))
            assert again[0]["places_level"] == (-1 if places is None else places) and [r["has_desc"] for r in again[1]] == [0] * len(ids)
            assert B.score([0], [got[0]], 0, EYE[None], ZERO[None])[0]["n_visible"] > 6       # they still serve score and match
    # a blob without descriptors into a tracker with places on
    with TP.make(1, places=None) as C:
        step(C, seqs, [(0, 0)])
        bare = C.export_archive()
    info, records = br.validate(bare)
    assert (info["places_level"], info["D"], records[0]["has_desc"]) == (-1, 0, 0)
    with TP.make(1, archive=(2, 4, None)) as B:
        step(B, seqs, [(0, N_T - 1)])
        step(B, seqs, [(0, 1)])
        assert B.import_archive(bare) == [1]
        assert B.import_archive(bare) == [2]               # slot 0 held B's own key frame and its descriptor: the mark goes with it
        for nid in (1, 2):
            refused(DVO_ERR_STATE, B.archive_descriptor, nid)
        assert B.places([0], 8) == [[]]
        assert B.export_archive() == B.export_archive([1, 2]) and [r["has_desc"] for r in br.validate(B.export_archive())[1]] == [0, 0]


def test_descriptor_padding():
    """232 x 312: level 2 is 58 x 78, D = 4524 = 16 * 282 + 12 -- the descriptor section of the payload and the device row are padded"""
    from rgbd_odometry_amd import DvoTracker
    rows, cols = 232, 312
    D = fr.level_size(rows, 2) * fr.level_size(cols, 2)
    assert D == 4524 and D % 16 == 12
    frame = frame_gen.camera_frame(70, rows, cols, shift=(0, 0), holes=True)

    def make():
        tr = DvoTracker(1, iters=[8, 8, 8], rows=rows, cols=cols, n_levels=3, first_shift=0)
        tr.set_intrinsics(*K)
        tr.set_archive(4, 1)
        tr.set_places(2)
        return tr

    with make() as A, make() as B:
        A.step([0], [frame[0]], [frame[1]])
        blob = A.export_archive()
        info, kfs = br.parse(blob)                         # the parser insists on zero padding
        assert info["D"] == D and np.array_equal(kfs[0]["desc"], A.archive_descriptor(0))
        B.step([0], [frame[0]], [frame[1]])
        assert B.import_archive(blob) == [1]
        assert same_key_frame(key_frame(A, 0), key_frame(B, 1))
        assert B.export_archive([1]) == blob
        row = B.places([0], 4)[0]                          # the same frame: distance 0, the row's padding of 128 adds nothing
        assert [(e["key_id"], e["stream"], e["distance"]) for e in row] == [(1, -1, 0)]


def test_demo_saves_an_archive_and_relocalises_against_a_loaded_one(tmp_path, demo_run):  # noqa: F811
    """examples/multi_track_demo --save-archive on three XML sequences, then a second run of three frames with --load-archive and
    --places: on its first frame every stream finds the loaded copy of the key frame the first run made from that very frame -- foreign
    (stream -1), distance 0 -- and aligns against it"""
    import re
    import subprocess
    path = tmp_path / "map.bin"
    save = subprocess.run([demo_run["exe"]] + demo_args(demo_run["dirs"], tmp_path / "save_") + ["--save-archive", str(path)],
                          capture_output=True, text=True, timeout=300)
    assert save.returncode == 0 and "saved the archive to " + str(path) in save.stdout, save.stdout[-1000:] + save.stderr
    for s in range(3):                                     # keeping the archive does not move the poses
        assert (tmp_path / ("save_%d.txt" % s)).read_text() == open(str(demo_run["prefix"]) + "%d.txt" % s).read(), s
    info, records = br.validate(path.read_bytes())
    origins = [(r["origin_stream"], r["origin_frame"]) for r in records]
    assert info["n_key_frames"] >= 3 and info["places_level"] == DEMO_NL - 1 and all((s, 0) in origins for s in range(3)), origins
    args = ["3"] + demo_run["dirs"] + ["0", "2", "1", str(DEMO_NL)] + [repr(float(k)) for k in K] + [str(DEMO_IT), str(tmp_path / "load_")]
    load = subprocess.run([demo_run["exe"]] + args + ["--places", "2", "--load-archive", str(path)], capture_output=True, text=True, timeout=300)
    assert load.returncode == 0, load.stderr
    head = [ln for ln in load.stdout.splitlines() if ln.startswith("loaded ")]
    assert len(head) == 1 and head[0].startswith("loaded %d key frames" % len(records)), load.stdout[:500]
    ids = [int(x) for x in head[0].split(":")[1].split()]
    assert ids == list(range(len(records)))
    for s in range(3):
        ln = [x for x in load.stdout.splitlines() if x.startswith("stream %d frame 0 place " % s)]
        assert len(ln) == 1, load.stdout
        key, stream, frame, distance, visible, points = (int(x) for x in re.findall(r"-?\d+", ln[0])[2:])
        assert (key, stream, frame, distance) == (ids[origins.index((s, 0))], -1, 0, 0) and 6 < visible <= points, ln[0]
