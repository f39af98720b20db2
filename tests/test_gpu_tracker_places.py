"""Place descriptors and top-k key-frame retrieval of the multi-stream tracker (include/dvo_amd.h: dvo_tracker_set_places,
dvo_tracker_archive_get_descriptor, dvo_tracker_query_places; kernels in dvo_tracker_places.hip).

Geometry and helpers of tests/test_gpu_tracker_archive.py: 240 x 320, 3 levels, 8 iterations each, one launch shape everywhere,
3 streams and 7 ticks (tick 5 is the forced key-frame switch); stream 0's last frame is generated with shift (0, 0) again.  The
descriptor level is 2: 60 x 80, D = 4800.

Expected values: tests/places_reference.py (numpy, integers) on the grey level of the oracle's pyramid of the frame that became the
key frame -- the tick-0 frame for event 1, the frame of tick n - 1 for a switch at tick n.  Descriptors, distances, ids and their
order are compared for equality: integer arithmetic has one value."""
import numpy as np
import pytest

import frame_gen
import frame_reference as fr
import places_reference as pr
import test_gpu_tracker_archive as TA
import test_gpu_tracker_information as TI

pytestmark = pytest.mark.gpu

ROWS, COLS, NL, SHIFT, K = TI.ROWS, TI.COLS, TI.NL, TI.SHIFT, TI.K
N_S, N_T = TA.N_S, TA.N_T
FULL = TA.FULL
LEVEL = 2
STORE_LAUNCHES, QUERY_LAUNCHES, NONE = 1, 2, 0xFFFFFFFF      # the constants of the header
step, refused, same_bits = TA.step, TA.refused, TA.same_bits


@pytest.fixture(scope="module")
def seqs():
    out = [TI.sequence(900 + s, N_T, TI.MOTIONS[s]) for s in range(N_S)]
    out[0][N_T - 1] = frame_gen.camera_frame(900, ROWS, COLS, shift=(0, 0), holes=True)       # stream 0 comes back to where it started
    return out


class Descs:
    """reference descriptor of a fed frame at a level, computed once per frame"""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def __call__(self, frame, level=LEVEL, nl=NL, shift=SHIFT):
        key = (id(frame[0]), level, nl, shift)
        if key not in self.cache:
            rows, cols = frame[0].shape[:2]
            grey = np.asarray(self.oracle.build_pyramid(frame[0], frame[1], n_levels=nl, first_shift=shift)[level][0], np.uint8)
            grey = grey.reshape(fr.level_size(rows, shift + level), fr.level_size(cols, shift + level))
            self.cache[key] = (frame, pr.descriptor(pr.column_major(grey)))
        return self.cache[key][1]


@pytest.fixture(scope="module")
def descs(oracle):
    return Descs(oracle)


def make(n, archive=(8, 4, None), places=LEVEL, **kw):
    tr = TA.make(n, archive=archive, **kw)
    if places is not None:
        tr.set_places(places)
    return tr


def run(tr, sched, frame_of, descs=None, keys=None, **dkw):
    """sched: per tick [(stream, frame index)]; frame_of(stream, index) -> frame.  Every new key frame is entered in keys as
    id -> dict(stream, frame, desc = the reference descriptor of the frame that became it) and, with descs, its stored descriptor is
    compared with that.  Returns the events per tick"""
    events = []
    last = {}
    for n, entry in enumerate(sched):
        streams = [s for s, _ in entry]
        _, _, ev = tr.step(streams, [frame_of(s, i)[0] for s, i in entry], [frame_of(s, i)[1] for s, i in entry])
        for (s, i), e in zip(entry, ev):
            if e != 0:
                kid = tr.key_frame_id(s)
                src = i if e == 1 else last[s]                     # a switch: the previous frame became the reference
                info = tr.archive_info(kid)
                if keys is not None:
                    keys[kid] = dict(stream=s, frame=info["frame"], desc=descs(frame_of(s, src), **dkw) if descs else None)
                if descs:
                    got = tr.archive_descriptor(kid)
                    assert got.dtype == np.uint8 and np.array_equal(got, keys[kid]["desc"]), (n, s, kid, int((got != keys[kid]["desc"]).sum()))
            last[s] = i
        events.append(ev.copy())
    return events


def expect_rows(tr, keys, queries, k, allowed):
    """reference rows: queries = {stream: descriptor of its current frame}; allowed(stream, id, key) -> bool"""
    ids = sorted(keys)
    return {s: pr.top_k(q, [keys[i]["desc"] for i in ids], ids, [allowed(s, i, keys[i]) for i in ids], k) for s, q in queries.items()}


def check_rows(tr, streams, k, want, keys, gap=0):
    rec, found = tr.places_raw(streams, k, gap)
    got = tr.places(streams, k, gap)
    for r, s in enumerate(streams):
        w = want[s]
        print("stream", s, "got", [(e["key_id"], e["distance"]) for e in got[r]], "want", w)
        assert found[r] == len(w) == len(got[r]), (s, found[r], w)
        assert [(e["key_id"], e["distance"]) for e in got[r]] == w, s
        for e in got[r]:
            assert (e["stream"], e["frame"]) == (keys[e["key_id"]]["stream"], keys[e["key_id"]]["frame"]), (s, e)
        tail = rec[r, found[r]:]
        assert (tail["key_id"] == -1).all() and (tail["frame"] == -1).all() and (tail["stream"] == -1).all() and (tail["distance"] == NONE).all(), s
    return got


@pytest.fixture(scope="module")
def world(seqs, descs):
    """the 7-tick run with places on, every stored descriptor checked on the way, left open for the queries"""
    tr = make(N_S)
    keys = {}
    events = run(tr, FULL, lambda s, i: seqs[s][i], descs, keys)
    yield tr, keys, events
    tr.close()


def current(seqs, descs):
    return {s: descs(seqs[s][N_T - 1]) for s in range(N_S)}


def test_stored_descriptors(world):
    """run() compared the descriptor of every new key frame with the reference on the frame that became it"""
    tr, keys, events = world
    assert [e.tolist() for e in events] == [[1] * N_S] + [[0] * N_S] * 4 + [[5] * N_S] + [[0] * N_S]
    assert sorted(keys) == list(range(2 * N_S))
    assert [keys[i]["frame"] for i in range(2 * N_S)] == [0] * N_S + [4] * N_S
    d = [keys[i]["desc"] for i in sorted(keys)]
    assert all(len(x) == 4800 for x in d)
    assert all(not np.array_equal(d[i], d[j]) for i in range(len(d)) for j in range(i))
    assert len(tr.archive_descriptor(0)) == 4800


def test_query_against_numpy(world, seqs, descs):
    tr, keys, _ = world
    own = {s: tr.key_frame_id(s) for s in range(N_S)}
    want = expect_rows(tr, keys, current(seqs, descs), 8, lambda s, i, key: i != own[s])
    got = check_rows(tr, [0, 1, 2], 8, want, keys)
    assert all(len(r) == 5 for r in got)
    # the revisit: stream 0's last frame is its first one again, byte for byte (frame_gen.camera_frame is deterministic)
    assert np.array_equal(seqs[0][N_T - 1][0], seqs[0][0][0])
    assert (got[0][0]["key_id"], got[0][0]["distance"], got[0][0]["stream"], got[0][0]["frame"]) == (0, 0, 0, 0)
    st = tr.archive_stats()
    assert st["last_launches"] <= QUERY_LAUNCHES and st["last_syncs"] == 1, st
    # the candidates feed dvo_tracker_match as they are
    _, _, recs = tr.match([0, 1, 2], [r[0]["key_id"] for r in got])
    assert all(r["n_points"] > 64 for r in recs), [r["n_points"] for r in recs]


def test_a_row_depends_on_its_stream_alone(world):
    tr, _, _ = world
    alone, _ = tr.places_raw([0], 8)
    mixed, found = tr.places_raw([2, 0, 1], 8)
    assert same_bits(alone[0], mixed[1])
    short, found2 = tr.places_raw([2, 0, 1], 2)
    assert same_bits(short, mixed[:, :2]) and found2.tolist() == [2, 2, 2] and found.tolist() == [5, 5, 5]
    again, found3 = tr.places_raw([2, 0, 1], 8)
    assert same_bits(again, mixed) and np.array_equal(found, found3)
    one, _ = tr.places_raw([1], 1)
    assert same_bits(one[0], mixed[2, :1])


def test_min_frame_gap(world, seqs, descs):
    tr, keys, _ = world
    own = {s: tr.key_frame_id(s) for s in range(N_S)}
    q = current(seqs, descs)
    # current frame 6: a gap of 100 hides every key frame of the stream's own, a gap of 3 only the one of frame 4 (6 - 4 < 3), which
    # is the current key frame anyway, a gap of 7 also the one of frame 0 (6 - 0 < 7) but 6 does not
    for gap in (100, 7, 6, 3):
        want = expect_rows(tr, keys, q, 8, lambda s, i, key: i != own[s] and not (key["stream"] == s and 6 - key["frame"] < gap))
        got = check_rows(tr, [0, 1, 2], 8, want, keys, gap)
        assert all(len(r) == (4 if gap >= 7 else 5) for r in got), gap
        if gap >= 7:
            assert all(e["stream"] != s for s, r in enumerate(got) for e in r)


def test_mixed_rig(seqs, descs):
    """stream 1 under a camera model of its own: its key frames are in no other stream's result, and it sees only its own"""
    with TA.make(N_S) as tr:
        tr.set_stream_intrinsics(1, 250.0, 254.0, 161.0, 118.0)
        tr.set_places()                                                          # default level: the coarsest
        keys = {}
        run(tr, FULL, lambda s, i: seqs[s][i], descs, keys)
        own = {s: tr.key_frame_id(s) for s in range(N_S)}
        want = expect_rows(tr, keys, current(seqs, descs), 8,
                           lambda s, i, key: i != own[s] and (key["stream"] == 1) == (s == 1))
        got = check_rows(tr, [0, 1, 2], 8, want, keys)
        assert [len(r) for r in got] == [3, 1, 3]
        assert all(e["stream"] != 1 for r in (got[0], got[2]) for e in r) and got[1][0]["stream"] == 1


def test_ring_eviction(seqs, descs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    # one stream, a key frame on ticks 0, 2, 3, 4 (key_frame_every = 2), two slots
    with make(1, archive=(2, 1, None), every=2) as tr:
        keys = {}
        run(tr, [[(0, n)] for n in range(5)], lambda s, i: seqs[s][i], descs, keys)
        ids = sorted(keys)
        assert ids == list(range(len(ids))) and len(ids) >= 3, ids
        for kid in ids[:-2]:
            refused(DVO_ERR_STATE, tr.archive_descriptor, kid)
        live = {i: keys[i] for i in ids[-2:]}
        want = expect_rows(tr, live, {0: descs(seqs[0][4])}, 4, lambda s, i, key: i != ids[-1])
        got = check_rows(tr, [0], 4, want, keys)
        assert [e["key_id"] for e in got[0]] == [ids[-2]]


def test_places_switched_on_late(seqs, descs):
    from rgbd_odometry_amd.capi import DVO_ERR_STATE
    with make(N_S, places=None) as tr:
        early = {}
        run(tr, FULL[:1], lambda s, i: seqs[s][i], None, early)
        tr.set_places(LEVEL)
        keys = {}
        run(tr, FULL[1:], lambda s, i: seqs[s][i], descs, keys)
        assert sorted(early) == [0, 1, 2] and sorted(keys) == [3, 4, 5]
        for kid in early:
            refused(DVO_ERR_STATE, tr.archive_descriptor, kid)
            assert tr.archive_info(kid)["frame"] == 0                            # archived all the same
        own = {s: tr.key_frame_id(s) for s in range(N_S)}
        want = expect_rows(tr, keys, current(seqs, descs), 8, lambda s, i, key: i != own[s])
        got = check_rows(tr, [0, 1, 2], 8, want, keys)
        assert all(len(r) == 2 and all(e["key_id"] >= 3 for e in r) for r in got)


def test_ties_go_to_the_smaller_id(seqs, descs):
    """streams 0 and 1 are fed the same sequence: for stream 2 their key frames come in pairs of equal distance"""
    feed = [seqs[0], seqs[0], seqs[2]]
    with make(N_S) as tr:
        keys = {}
        run(tr, FULL, lambda s, i: feed[s][i], descs, keys)
        own = {s: tr.key_frame_id(s) for s in range(N_S)}
        q = {s: descs(feed[s][N_T - 1]) for s in range(N_S)}
        want = expect_rows(tr, keys, q, 8, lambda s, i, key: i != own[s])
        got = check_rows(tr, [0, 1, 2], 8, want, keys)
        row = [(e["key_id"], e["distance"]) for e in got[2]]
        ids = [i for i, _ in row]
        for a, b in ((0, 1), (3, 4)):
            assert ids.index(b) == ids.index(a) + 1 and row[ids.index(a)][1] == row[ids.index(b)][1], row
        # stream 0 is back where it started: its own tick-0 key frame and stream 1's twin of it, both at distance 0
        assert [(e["key_id"], e["distance"]) for e in got[0]][:2] == [(0, 0), (1, 0)]


def test_padding(descs):
    """a descriptor level of 61 x 81: D = 4941 is no multiple of 4 (the row is padded by 11 bytes of 128) and the images of the odd
    frame-store slots start at odd addresses"""
    rows, cols, nl, level = 244, 324, 3, 2
    assert (fr.level_size(rows, level), fr.level_size(cols, level)) == (61, 81)
    from rgbd_odometry_amd import DvoTracker
    feed = [[frame_gen.camera_frame(70 + s, rows, cols, shift=(i, -2 * i), holes=True) for i in range(4)] for s in range(3)]
    with DvoTracker(3, iters=[8, 8, 8], rows=rows, cols=cols, n_levels=nl, first_shift=0, key_frame_every=2) as tr:
        tr.set_intrinsics(*K)
        tr.set_archive(8, 1)
        tr.set_places(level)
        keys = {}
        dkw = dict(level=level, nl=nl, shift=0)
        events = run(tr, [[(s, n) for s in range(3)] for n in range(4)], lambda s, i: feed[s][i], descs, keys, **dkw)
        assert len(keys) >= 6 and all(len(k["desc"]) == 4941 for k in keys.values()), [e.tolist() for e in events]
        live = {i: keys[i] for i in sorted(keys)[-8:]}
        own = {s: tr.key_frame_id(s) for s in range(3)}
        q = {s: descs(feed[s][3], **dkw) for s in range(3)}
        want = expect_rows(tr, live, q, 8, lambda s, i, key: i != own[s])
        got = check_rows(tr, [0, 1, 2], 8, want, keys)
        assert all(len(r) >= 4 for r in got)


def test_clamps_on_the_device(seqs):
    """mono8 first frames: 250 everywhere with a block of 0 (the block saturates at 0), and its inverse (the block saturates at 255)"""
    low = np.full((ROWS, COLS), 250, np.uint8)
    low[60:140, 100:220] = 0
    high = 255 - low
    d16 = np.clip(np.nan_to_num(np.rint(seqs[0][0][1] * 1000.0), nan=0.0), 0, 65535).astype(np.uint16)
    want = [pr.descriptor(pr.column_major(fr.resize_nn(img, SHIFT + LEVEL))) for img in (low, high)]
    assert want[0].min() == 0 and 128 < want[0].max() < 255 and want[1].max() == 255 and 0 < want[1].min() < 128
    with make(2, archive=(4, 1, None)) as tr:
        _, _, ev = tr.step([0, 1], [low, high], [d16, d16])
        assert ev.tolist() == [1, 1]
        ids = [tr.key_frame_id(s) for s in range(2)]
        assert ids == [0, 1], ids
        for s in range(2):
            got = tr.archive_descriptor(ids[s])
            assert np.array_equal(got, want[s]), (s, int((got != want[s]).sum()))
        rows = tr.places([0, 1], 2)
        assert [[(e["key_id"], e["distance"]) for e in r] for r in rows] == [[(1, pr.distance(want[0], want[1]))], [(0, pr.distance(want[0], want[1]))]]


def test_many_slots(seqs, descs):
    """16 streams, a key frame nearly every tick, 72 slots: the ring wraps once, the live slots span two slot chunks of the distance
    kernel (64 slots each) and the queries two query tiles (8 rows each)"""
    n_streams, cap = 16, 72
    with make(n_streams, archive=(cap, 1, None), every=2) as tr:
        keys = {}
        run(tr, [[(s, n) for s in range(n_streams)] for n in range(N_T)], lambda s, i: seqs[s % N_S][i], descs, keys)
        st = tr.archive_stats()
        assert st["archived"] == len(keys) > cap and st["evicted"] == len(keys) - cap and st["refused"] == 0, st
        live = {i: keys[i] for i in sorted(keys)[-cap:]}
        own = {s: tr.key_frame_id(s) for s in range(n_streams)}
        q = {s: descs(seqs[s % N_S][N_T - 1]) for s in range(n_streams)}
        streams = list(range(n_streams))
        for k in (8, 32):
            want = expect_rows(tr, live, q, k, lambda s, i, key: i != own[s])
            got = check_rows(tr, streams, k, want, keys)
            assert all(len(r) == k for r in got)
        sub, _ = tr.places_raw([9, 3], 8)
        full, _ = tr.places_raw(streams, 8)
        assert same_bits(sub[0], full[9]) and same_bits(sub[1], full[3])


def probe_run(tr, seqs, with_places):
    """the 7-tick run with score and match between the ticks, and a query where places are on"""
    ticks = []
    for n, entry in enumerate(FULL):
        R, t, ev = step(tr, seqs, entry)
        out = dict(R=R, t=t, ev=ev.copy(), stats=tr.stats(), rec={s: tr.information(s) for s in range(N_S)},
                   sig={s: tr.signals(s) for s in range(N_S) if ev[s] != 1}, pts={}, probe=None)
        for s in range(N_S):
            if ev[s] != 0:
                out["pts"][s] = [tr.archive_points(tr.key_frame_id(s), l) for l in range(NL)]
        if n >= 1:
            cand = [(0, tr.key_frame_id(1)), (2, tr.key_frame_id(0))]
            sc = tr.score([c[0] for c in cand], [c[1] for c in cand], 0, R[:2], t[:2])
            Rm, tm, mr = tr.match([c[0] for c in cand], [c[1] for c in cand])
            out["probe"] = (sc, Rm, tm, mr)
            if with_places:
                tr.places([0, 1, 2], 4)
                st = tr.archive_stats()
                assert st["last_launches"] <= QUERY_LAUNCHES and st["last_syncs"] == 1, (n, st)
        ticks.append(out)
    return ticks


def test_nothing_else_moves(seqs):
    with make(N_S, places=None) as tr:
        off = probe_run(tr, seqs, False)
    with make(N_S) as tr:
        on = probe_run(tr, seqs, True)
    for n, (a, b) in enumerate(zip(on, off)):
        assert same_bits(a["R"], b["R"]) and same_bits(a["t"], b["t"]) and np.array_equal(a["ev"], b["ev"]), n
        assert a["sig"] == b["sig"], n
        assert all(TI.same_record(a["rec"][s], b["rec"][s]) for s in range(N_S)), n
        assert sorted(a["pts"]) == sorted(b["pts"]) and all(same_bits(x, y) for s in a["pts"] for x, y in zip(a["pts"][s], b["pts"][s])), n
        if n >= 1:
            (sa, Ra, ta, ma), (sb, Rb, tb, mb) = a["probe"], b["probe"]
            assert all(TA.same_record(x, y) for x, y in zip(sa, sb)) and all(TA.same_record(x, y) for x, y in zip(ma, mb)), n
            assert same_bits(Ra, Rb) and same_bits(ta, tb), n
        assert a["stats"]["syncs"] == b["stats"]["syncs"], (n, a["stats"], b["stats"])
        extra = STORE_LAUNCHES if n in (0, 5) else 0              # one store launch on each of these ticks, none on the others
        assert a["stats"]["launches"] == b["stats"]["launches"] + extra, (n, a["stats"], b["stats"])
        assert {k: v for k, v in a["stats"].items() if k != "launches"} == {k: v for k, v in b["stats"].items() if k != "launches"}, n
    assert [x["stats"]["key_frames"] for x in off] == [0, 0, 0, 0, 0, N_S, 0]


def test_contract(seqs):
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID, DVO_ERR_STATE, DVO_TRACKER_PLACES_MAX_K
    with TA.make(4, archive=None) as tr:
        refused(DVO_ERR_STATE, tr.set_places, 2)                                # needs the archive
        refused(DVO_ERR_STATE, tr.places, [0], 1)
        tr.set_archive(4, 2)
        refused(DVO_ERR_STATE, tr.places, [0], 1)                               # places are off by default
        refused(DVO_ERR_STATE, tr.archive_descriptor, 0)
        refused(DVO_ERR_INVALID, tr.set_places, NL)                             # a level outside the tracker's
        refused(DVO_ERR_INVALID, tr.set_places, -2)
        refused(DVO_ERR_INVALID, tr.set_places, 0)                              # 240 x 320: D over the cap
        refused(DVO_ERR_STATE, tr.places, [0], 1)                               # nothing changed: still off
        tr.set_places(1)                                                        # 120 x 160 = 19 200: the largest descriptor
        refused(DVO_ERR_STATE, tr.places, [0], 1)                               # never stepped
        for n in range(2):
            step(tr, seqs, [(s, n) for s in range(3)])                          # stream 3 stays at its start
        assert len(tr.archive_descriptor(0)) == 19200

        def state():
            return (tr.archive_stats(), tr.stats(), [tr.key_frame_id(s) for s in range(3)], [tr.signals(s) for s in range(3)],
                    [tr.archive_descriptor(i).tobytes() for i in range(3)])

        ok = tr.places_raw([0, 1, 2], 3)
        assert ok[1].tolist() == [2, 2, 2]
        before = state()
        refused(DVO_ERR_INVALID, tr.places, [], 1)                              # n outside [1, max_streams]
        refused(DVO_ERR_INVALID, tr.places, [0, 1, 2, 3, 0], 1)
        refused(DVO_ERR_INVALID, tr.places, [0], 0)                             # k outside [1, DVO_TRACKER_PLACES_MAX_K]
        refused(DVO_ERR_INVALID, tr.places, [0], DVO_TRACKER_PLACES_MAX_K + 1)
        refused(DVO_ERR_INVALID, tr.places, [4], 1)                             # stream outside range
        refused(DVO_ERR_INVALID, tr.places, [-1], 1)
        refused(DVO_ERR_INVALID, tr.places, [1, 1], 1)                          # listed twice
        refused(DVO_ERR_INVALID, tr.places, [0], 1, -1)                         # negative min_frame_gap
        refused(DVO_ERR_STATE, tr.places, [0, 3], 1)                            # stream 3 has never been stepped
        refused(DVO_ERR_STATE, tr.archive_descriptor, 7)                        # unknown id
        refused(DVO_ERR_STATE, tr.archive_descriptor, -1)
        refused(DVO_ERR_INVALID, tr.set_places, 0)                              # refused: places stay on as they were
        after = state()
        assert before[:1] + before[2:] == after[:1] + after[2:] and before[1] == after[1]
        again = tr.places_raw([0, 1, 2], 3)
        assert same_bits(ok[0], again[0]) and np.array_equal(ok[1], again[1])
        full = tr.places_raw([0], DVO_TRACKER_PLACES_MAX_K)                     # the largest k
        assert full[1].tolist() == [2] and same_bits(full[0][0, :3], ok[0][0])
        tr.set_places(-1)                                                       # off: the descriptors are gone, the archive stays
        refused(DVO_ERR_STATE, tr.places, [0], 1)
        refused(DVO_ERR_STATE, tr.archive_descriptor, 0)
        assert tr.archive_info(0)["stream"] == 0
        tr.set_places(2)                                                        # on again: without descriptors for what is archived
        refused(DVO_ERR_STATE, tr.archive_descriptor, 0)
        assert tr.places_raw([0], 2)[1].tolist() == [0]
        tr.set_archive(4, 2)                                                    # re-configuring the archive switches places off
        refused(DVO_ERR_STATE, tr.places, [0], 1)
        step(tr, seqs, [(s, 2) for s in range(3)])
