"""Shift search on place descriptors and the pose guess of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_place_shifts,
dvo_tracker_place_guess; kernel place_shift_kernel in dvo_tracker_places.hip).

Geometry, frames and helpers of tests/test_gpu_tracker_places.py: 240 x 320, 3 levels, 3 streams and 7 ticks, descriptor level 2
(60 x 80, D = 4800) unless a test says otherwise.

Expected values: tests/place_shift_reference.py (numpy, integers) on descriptors the reference builds itself from the oracle's pyramid
of the frames fed (the Descs helper of the places tests) or, for mono8 frames, from tests/frame_reference.py's decimation.  All six
fields of every record are compared for equality: integer arithmetic has one value.  The conditions that make these inputs worth
running -- unique deep minima for the shifted revisits, ties for the constructed frames -- are asserted on the reference alone in
tests/test_tracker_place_shift_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import frame_gen
import frame_reference as fr
import place_shift_reference as ps
import test_gpu_tracker_archive as TA
import test_gpu_tracker_places as TP
from test_gpu_tracker_places import descs, seqs  # noqa: F401  (fixtures: the frames of the 7-tick run, the reference descriptors)

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT, K = TP.ROWS, TP.COLS, TP.NL, TP.SHIFT, TP.K
N_S, N_T, FULL, LEVEL = TP.N_S, TP.N_T, TP.FULL, TP.LEVEL
LR, LC = 60, 80
refused, same_bits, step = TA.refused, TA.same_bits, TA.step
_REF = {}


def want_record(key, query, rows, cols, radius):
    """the reference record of two descriptors, computed once per content"""
    k = (key.tobytes(), query.tobytes(), rows, cols, radius)
    if k not in _REF:
        _REF[k] = ps.record(key, query, rows, cols, radius)
    return _REF[k]


def check(tr, cands, radius, key_of, query_of, rows=LR, cols=LC):
    """one call for cands = [(stream, key id)]; every field of every record against the reference.  Returns the raw records"""
    raw = tr.place_shifts_raw([c[0] for c in cands], [c[1] for c in cands], radius)
    st = tr.archive_stats()
    assert (st["last_launches"], st["last_syncs"]) == (1, 1), st
    assert raw.shape == (len(cands),) and raw.dtype.names == ps.FIELDS
    bad = []
    for (s, kid), got in zip(cands, raw):
        want = want_record(key_of(kid), query_of(s), rows, cols, radius)
        g = {f: int(got[f]) for f in ps.FIELDS}
        if g != want:
            bad.append((s, kid, radius, g, want))
    assert not bad, (len(bad), bad[:4])
    return raw


@pytest.fixture(scope="module")
def world(seqs, descs):  # noqa: F811
    """the 7-tick run with places on, left open: (tracker, keys, the streams' current descriptors)"""
    tr = TP.make(N_S)
    keys = {}
    TP.run(tr, FULL, lambda s, i: seqs[s][i], descs, keys)
    yield tr, keys, TP.current(seqs, descs)
    tr.close()


def test_parity_on_the_seven_tick_world(world):
    tr, keys, cur = world
    assert sorted(keys) == list(range(2 * N_S))
    cands = [(s, kid) for s in range(N_S) for kid in sorted(keys)]
    seen = set()
    for radius in (0, 1, 3, 6, 8):
        raw = check(tr, cands, radius, lambda kid: keys[kid]["desc"], lambda s: cur[s])
        assert (raw["area"] == (LR - 2 * radius) * (LC - 2 * radius)).all()
        assert (np.abs(raw["dy"]) <= radius).all() and (np.abs(raw["dx"]) <= radius).all()
        seen |= {(int(r["dy"]), int(r["dx"])) for r in raw}
        dicts = tr.place_shifts([c[0] for c in cands], [c[1] for c in cands], radius)
        assert dicts == [{f: int(r[f]) for f in ps.FIELDS} for r in raw]
    print("best shifts seen:", sorted(seen))
    assert len(seen) > 4                                            # the inputs do not all register at one shift
    # the revisit: stream 0's last frame is its first again
    r = tr.place_shifts([0], [0], 6)[0]
    assert (r["dy"], r["dx"], r["sad"]) == (0, 0, 0) and r["sad_second"] > 20000, r


def test_radius_zero_is_the_distance_of_the_query(world):
    tr, _, _ = world
    rows = tr.places([0, 1, 2], 8)
    cands = [(s, e["key_id"], e["distance"]) for s, row in enumerate(rows) for e in row]
    assert len(cands) == 15
    got = tr.place_shifts([c[0] for c in cands], [c[1] for c in cands], 0)
    for (s, kid, dist), r in zip(cands, got):
        assert r == dict(dy=0, dx=0, sad=dist, sad_zero=dist, sad_second=ps.NONE, area=LR * LC), (s, kid, dist, r)


def test_shifted_revisit_across_streams(descs):  # noqa: F811
    frames = [frame_gen.camera_frame(900, ROWS, COLS, shift=(0, 0), holes=True),
              frame_gen.camera_frame(900, ROWS, COLS, shift=(-16, 16), holes=True),
              frame_gen.camera_frame(901, ROWS, COLS, shift=(0, 0), holes=True)]
    with TP.make(N_S) as tr:
        _, _, ev = tr.step([0, 1, 2], [f[0] for f in frames], [f[1] for f in frames])
        assert ev.tolist() == [1, 1, 1]
        key0 = tr.key_frame_id(0)
        assert np.array_equal(tr.archive_descriptor(key0), descs(frames[0]))
        raw = check(tr, [(1, key0), (2, key0)], 6, lambda kid: descs(frames[0]), lambda s: descs(frames[s]))
        print(raw)
        assert (int(raw[0]["dy"]), int(raw[0]["dx"])) == (4, -4) and raw[0]["sad"] <= raw[0]["area"]
        assert raw[1]["sad"] >= 5 * raw[0]["sad"] and raw[1]["sad"] >= 20000
        # the guess through the C ABI against the reference, over the whole range of shifts: the bound of the CPU file
        for dy in range(-ps.MAX_RADIUS, ps.MAX_RADIUS + 1):
            for dx in range(-ps.MAX_RADIUS, ps.MAX_RADIUS + 1):
                R0, t0 = tr.place_guess(1, dy, dx)
                Rw, tw = ps.guess(K, LEVEL, SHIFT, dy, dx)
                assert np.abs(R0 - Rw).max() <= 1e-14 and np.array_equal(t0, tw), (dy, dx)
        assert np.array_equal(tr.place_guess(1, 0, 0)[0], np.eye(3))
        # the chain: the guess of the best shift is a guess dvo_tracker_match takes
        R0, t0 = tr.place_guess(1, int(raw[0]["dy"]), int(raw[0]["dx"]))
        _, _, recs = tr.match([1], [key0], R0[None], t0[None])
        assert recs[0]["n_points"] > 64


def level_desc(image, level):
    return ps.level_descriptor(image, level)


@pytest.mark.parametrize("geometry", ["61x81", "15x20"])
def test_alignment_and_tails(descs, geometry):  # noqa: F811
    """61 x 81: D = 4941 is no multiple of 4, the odd frame-store slots start at odd addresses, the window heights 51, 49 and 45 leave
    a tail of 3, 1 and 1 bytes in every run.  15 x 20 at radius 7: the window is 1 x 6, every run is one byte at every alignment"""
    from rgbd_odometry_amd import DvoTracker
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    rows, cols, nl, level, radii = (244, 324, 3, 2, (5, 6, 8)) if geometry == "61x81" else (120, 160, 4, 3, (7, 3, 0))
    lr, lc = fr.level_size(rows, level), fr.level_size(cols, level)
    assert (lr, lc) == ((61, 81) if geometry == "61x81" else (15, 20))
    feed = [[frame_gen.camera_frame(70 + s, rows, cols, shift=(i, -2 * i), holes=True) for i in range(4)] for s in range(3)]
    with DvoTracker(3, iters=[8] * nl, rows=rows, cols=cols, n_levels=nl, first_shift=0, key_frame_every=2) as tr:
        tr.set_intrinsics(*K)
        tr.set_archive(8, 1, [fr.level_size(rows, l) * fr.level_size(cols, l) for l in range(nl)])
        tr.set_places(level)
        keys = {}
        dkw = dict(level=level, nl=nl, shift=0)
        TP.run(tr, [[(s, n) for s in range(3)] for n in range(4)], lambda s, i: feed[s][i], descs, keys, **dkw)
        live = sorted(keys)[-8:]
        assert len(live) >= 6 and all(len(keys[i]["desc"]) == lr * lc for i in live)
        cands = [(s, kid) for s in range(3) for kid in live]
        for radius in radii:
            raw = check(tr, cands, radius, lambda kid: keys[kid]["desc"], lambda s: descs(feed[s][3], **dkw), lr, lc)
            assert (raw["area"] == (lr - 2 * radius) * (lc - 2 * radius)).all()
        if geometry == "15x20":
            assert (lr - 14) * (lc - 14) == 6
            refused(DVO_ERR_INVALID, tr.place_shifts, [0], [live[0]], 8)          # 15 - 16 < 1: no window
            assert tr.archive_stats()["last_launches"] == 1


def tie_world(names):
    """the constructed frames of tests/place_shift_reference.py in one tracker: stream 2 i gets key image i as its first frame (it becomes
    a key frame), stream 2 i + 1 gets it too and then query image i as its second frame.  Yields (tracker, [(name, candidate, radius,
    expected shift, key descriptor, query descriptor)])"""
    frames = ps.tie_frames(ROWS, COLS, SHIFT + LEVEL)
    d16 = np.full((ROWS, COLS), 2000, np.uint16)
    full = [fr.level_size(ROWS, SHIFT + l) * fr.level_size(COLS, SHIFT + l) for l in range(NL)]      # the patterns are dense in edges
    tr = TP.make(2 * len(names), archive=(2 * len(names), 1, full))
    first = [frames[n][0] for n in names for _ in range(2)]
    _, _, ev = tr.step(list(range(2 * len(names))), first, [d16] * len(first))
    assert ev.tolist() == [1] * len(first)
    tr.step([2 * i + 1 for i in range(len(names))], [frames[n][1] for n in names], [d16] * len(names))
    cases = []
    for i, n in enumerate(names):
        key, query, radius, want = frames[n]
        kid = tr.key_frame_id(2 * i)
        kd = level_desc(key, SHIFT + LEVEL)
        assert np.array_equal(tr.archive_descriptor(kid), kd), n
        cases.append((n, (2 * i + 1, kid), radius, want, kd, level_desc(query, SHIFT + LEVEL)))
    return tr, cases


@pytest.mark.parametrize("names", [("stripes", "rows_tie", "cols_tie"), ("flat",)], ids=["patterns", "flat_query"])
def test_ties(names):
    """more than one shift at the smallest SAD: the lower tiers of the order decide.  `flat`: the query is an image of one grey value,
    so every SAD is the same number (a flat image has no edge and cannot be a key frame: it is fed as a stream's second frame)"""
    tr, cases = tie_world(names)
    with tr:
        for name, cand, radius, want, kd, qd in cases:
            raw = check(tr, [cand], radius, lambda kid: kd, lambda s: qd)
            print(name, raw[0])
            assert (int(raw[0]["dy"]), int(raw[0]["dx"])) == want, (name, raw[0])
            if name == "flat":
                assert raw[0]["sad"] == raw[0]["sad_zero"] == raw[0]["sad_second"] > 0


def test_clamps(seqs):  # noqa: F811
    """the saturating mono8 frames of the places tests: bytes 0 and 255 in the rows"""
    low = np.full((ROWS, COLS), 250, np.uint8)
    low[60:140, 100:220] = 0
    high = 255 - low
    d16 = np.clip(np.nan_to_num(np.rint(seqs[0][0][1] * 1000.0), nan=0.0), 0, 65535).astype(np.uint16)
    want = [level_desc(img, SHIFT + LEVEL) for img in (low, high)]
    assert want[0].min() == 0 and want[1].max() == 255
    with TP.make(2, archive=(4, 1, None)) as tr:
        tr.step([0, 1], [low, high], [d16, d16])
        ids = [tr.key_frame_id(s) for s in range(2)]
        assert ids == [0, 1]
        for radius in (0, 5, 8):
            raw = check(tr, [(0, 1), (1, 0), (0, 0)], radius, lambda kid: want[kid], lambda s: want[s])
            assert raw[2]["sad"] == 0 and raw[0]["sad"] > 0


def test_a_record_depends_on_its_candidate_alone(world):
    tr, keys, _ = world
    cands = [(s, kid) for s in range(N_S) for kid in sorted(keys)]
    full = tr.place_shifts_raw([c[0] for c in cands], [c[1] for c in cands], 6)
    rev = tr.place_shifts_raw([c[0] for c in cands[::-1]], [c[1] for c in cands[::-1]], 6)
    assert same_bits(rev[::-1], full)
    pick = [7, 2, 16]
    sub = tr.place_shifts_raw([cands[i][0] for i in pick], [cands[i][1] for i in pick], 6)
    assert same_bits(sub, full[pick])
    twice = [cands[5], cands[11], cands[5], cands[5]]
    dup = tr.place_shifts_raw([c[0] for c in twice], [c[1] for c in twice], 6)
    assert same_bits(dup, full[[5, 11, 5, 5]])
    alone = tr.place_shifts_raw([cands[17][0]], [cands[17][1]], 6)
    assert same_bits(alone, full[17:18])


def test_many_candidates(seqs, descs):  # noqa: F811
    """16 streams, 72 slots, 16 x 32 = 512 candidates in one call -- the largest n, more workgroups than the device has compute units"""
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    n_streams, cap = 16, 72
    with TP.make(n_streams, archive=(cap, 1, None), every=2) as tr:
        keys = {}
        TP.run(tr, [[(s, n) for s in range(n_streams)] for n in range(N_T)], lambda s, i: seqs[s % N_S][i], descs, keys)
        live = sorted(keys)[-cap:]
        assert len(keys) > cap
        cands = [(i // 32, live[i % cap]) for i in range(n_streams * 32)]
        assert len(cands) == 512 and len(set(cands)) == 512
        raw = check(tr, cands, 6, lambda kid: keys[kid]["desc"], lambda s: descs(seqs[s % N_S][N_T - 1]))
        assert len({(int(r["dy"]), int(r["dx"])) for r in raw}) > 4
        refused(DVO_ERR_INVALID, tr.place_shifts, [c[0] for c in cands] + [0], [c[1] for c in cands] + [live[0]], 6)


def probe_run(tr, seqs, with_shifts):  # noqa: F811
    """the 7-tick run with score, match, verify and a query between the ticks -- and, with_shifts, shift searches and guesses before them"""
    ticks = []
    for n, entry in enumerate(FULL):
        R, t, ev = step(tr, seqs, entry)
        out = dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), rec={s: tr.information(s) for s in range(N_S)},
                   sig={s: tr.signals(s) for s in range(N_S) if ev[s] != 1}, pts={}, probe=None)
        for s in range(N_S):
            if ev[s] != 0:
                out["pts"][s] = [tr.archive_points(tr.key_frame_id(s), l) for l in range(NL)]
        cand = [(0, tr.key_frame_id(1)), (2, tr.key_frame_id(0))]
        if with_shifts:
            for radius in (6, 0):
                tr.place_shifts([c[0] for c in cand] + [1], [c[1] for c in cand] + [tr.key_frame_id(1)], radius)
                st = tr.archive_stats()
                assert (st["last_launches"], st["last_syncs"]) == (1, 1), (n, st)
            tr.place_guess(0, 3, -2)
        if n >= 1:
            sc = tr.score([c[0] for c in cand], [c[1] for c in cand], 0, R[:2], t[:2])
            Rm, tm, mr = tr.match([c[0] for c in cand], [c[1] for c in cand])
            vf = tr.verify([c[0] for c in cand], [c[1] for c in cand], 0, Rm, tm)
            out["probe"] = (sc, Rm, tm, mr, vf, tr.places_raw([0, 1, 2], 4))
        out["desc"] = [tr.archive_descriptor(tr.key_frame_id(s)).tobytes() for s in range(N_S)]
        out["astats"] = {k: v for k, v in tr.archive_stats().items() if not k.startswith("last_")}
        ticks.append(out)
    return ticks


def test_nothing_else_moves(seqs):  # noqa: F811
    with TP.make(N_S) as tr:
        off = probe_run(tr, seqs, False)
    with TP.make(N_S) as tr:
        on = probe_run(tr, seqs, True)
    for n, (a, b) in enumerate(zip(on, off)):
        assert same_bits(a["R"], b["R"]) and same_bits(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"], n
        assert all(TP.TI.same_record(a["rec"][s], b["rec"][s]) for s in range(N_S)), n
        assert sorted(a["pts"]) == sorted(b["pts"]) and all(same_bits(x, y) for s in a["pts"] for x, y in zip(a["pts"][s], b["pts"][s])), n
        if n >= 1:
            (sa, Ra, ta, ma, va, qa), (sb, Rb, tb, mb, vb, qb) = a["probe"], b["probe"]
            assert all(TA.same_record(x, y) for x, y in zip(sa, sb)) and all(TA.same_record(x, y) for x, y in zip(ma, mb)), n
            assert same_bits(Ra, Rb) and same_bits(ta, tb) and va == vb, n
            assert same_bits(qa[0], qb[0]) and np.array_equal(qa[1], qb[1]), n
        assert a["stats"] == b["stats"], (n, a["stats"], b["stats"])                # launches and synchronisations of the step included
        assert a["desc"] == b["desc"] and a["astats"] == b["astats"], n
    assert [x["stats"]["key_frames"] for x in off] == [0, 0, 0, 0, 0, N_S, 0]


def test_contract(seqs):  # noqa: F811
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE, DVO_TRACKER_PLACES_MAX_K, DvoTrackerPlaceShift
    with TA.make(4, archive=None, every=2) as tr:
        lib, h = tr.lib, tr._h
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [0], 1)                    # places off (and the archive)
        refused(DVO_ERR_STATE, tr.place_guess, 0, 1, 1)
        tr.set_archive(4, 2)
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [0], 1)                    # the archive alone is not enough
        refused(DVO_ERR_STATE, tr.place_guess, 0, 1, 1)
        step(tr, seqs, [(s, 0) for s in range(3)])                              # ids 0, 1, 2: archived while places are off
        tr.set_places(LEVEL)
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [0], 1)                    # no descriptor: archived before set_places
        for n in (1, 2):
            step(tr, seqs, [(s, n) for s in range(3)])                          # tick 2 switches: ids 3, 4, 5 evict 0 and 1
        ids = [tr.key_frame_id(s) for s in range(3)]
        assert ids == [3, 4, 5], ids

        def state():
            return (tr.archive_stats(), tr.stats(), [tr.key_frame_id(s) for s in range(3)], [tr.signals(s) for s in range(3)],
                    [tr.archive_descriptor(i).tobytes() for i in ids])

        ok = tr.place_shifts_raw([0, 1, 2, 0], [3, 4, 5, 4], 6)
        before = state()
        assert (before[0]["last_launches"], before[0]["last_syncs"]) == (1, 1)
        refused(DVO_ERR_INVALID, tr.place_shifts, [], [], 1)                    # n outside [1, max_streams * DVO_TRACKER_PLACES_MAX_K]
        big = 4 * DVO_TRACKER_PLACES_MAX_K + 1
        refused(DVO_ERR_INVALID, tr.place_shifts, [0] * big, [3] * big, 1)
        refused(DVO_ERR_INVALID, tr.place_shifts, [4], [3], 1)                  # stream outside range
        refused(DVO_ERR_INVALID, tr.place_shifts, [-1], [3], 1)
        refused(DVO_ERR_INVALID, tr.place_shifts, [0], [3], -1)                 # radius outside [0, DVO_TRACKER_PLACE_SHIFT_MAX_RADIUS]
        refused(DVO_ERR_INVALID, tr.place_shifts, [0], [3], 9)
        one_s, one_k, one_r = (C.c_int * 1)(0), (C.c_longlong * 1)(3), (DvoTrackerPlaceShift * 1)()
        assert lib.dvo_tracker_place_shifts(h, 1, None, one_k, 1, one_r) == DVO_ERR_INVALID      # a NULL argument
        assert lib.dvo_tracker_place_shifts(h, 1, one_s, None, 1, one_r) == DVO_ERR_INVALID
        assert lib.dvo_tracker_place_shifts(h, 1, one_s, one_k, 1, None) == DVO_ERR_INVALID
        assert lib.dvo_tracker_place_shifts(None, 1, one_s, one_k, 1, one_r) == DVO_ERR_INVALID
        refused(DVO_ERR_STATE, tr.place_shifts, [3], [3], 1)                    # stream 3 has never been stepped
        refused(DVO_ERR_STATE, tr.place_shifts, [0, 1], [3, 0], 1)              # id 0 is evicted
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [2], 1)                    # id 2 lives, archived before set_places: no descriptor
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [99], 1)                   # never given
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [-1], 1)
        refused(DVO_ERR_INVALID, tr.place_guess, 4, 0, 0)                       # the guess: stream outside range
        refused(DVO_ERR_INVALID, tr.place_guess, -1, 0, 0)
        refused(DVO_ERR_INVALID, tr.place_guess, 0, 9, 0)                       # |dy|, |dx| above the maximum radius
        refused(DVO_ERR_INVALID, tr.place_guess, 0, 0, -9)
        R0, t0 = (C.c_double * 9)(), (C.c_double * 3)()
        assert lib.dvo_tracker_place_guess(h, 0, 1, 1, None, t0) == DVO_ERR_INVALID
        assert lib.dvo_tracker_place_guess(h, 0, 1, 1, R0, None) == DVO_ERR_INVALID
        assert lib.dvo_tracker_place_guess(h, 3, 8, -8, R0, t0) == 0            # a stream that has no frame yet has intrinsics
        after = state()
        assert before == after                                                  # last_launches / last_syncs of the archive's statistics included
        assert same_bits(tr.place_shifts_raw([0, 1, 2, 0], [3, 4, 5, 4], 6), ok)
        tr.set_places(-1)                                                       # off again
        refused(DVO_ERR_STATE, tr.place_shifts, [0], [3], 1)
        refused(DVO_ERR_STATE, tr.place_guess, 0, 1, 1)
        step(tr, seqs, [(s, 3) for s in range(3)])
    # a mixed rig: key frames under another camera model are refused, as match and verify refuse them
    with TA.make(N_S) as tr:
        tr.set_stream_intrinsics(1, 250.0, 254.0, 161.0, 118.0)
        tr.set_places(LEVEL)
        step(tr, seqs, [(s, 0) for s in range(N_S)])
        ids = [tr.key_frame_id(s) for s in range(N_S)]
        refused(DVO_ERR_INVALID, tr.place_shifts, [0], [ids[1]], 2)
        refused(DVO_ERR_INVALID, tr.place_shifts, [2, 1], [ids[0], ids[0]], 2)
        got = tr.place_shifts([1, 0, 2], [ids[1], ids[2], ids[0]], 2)
        assert got[0]["sad"] == 0 and (got[0]["dy"], got[0]["dx"]) == (0, 0)
        # the guess uses the stream's own intrinsics
        for s, Ks in ((0, K), (1, (250.0, 254.0, 161.0, 118.0))):
            R0, _ = tr.place_guess(s, -5, 7)
            assert np.abs(R0 - ps.guess(Ks, LEVEL, SHIFT, -5, 7)[0]).max() <= 1e-14, s
        assert not np.array_equal(tr.place_guess(0, -5, 7)[0], tr.place_guess(1, -5, 7)[0])
