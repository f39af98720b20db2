"""Multi-stream photometric engine on the GPU (include/dvo_amd.h, "many camera streams on the photometric engine"): every stream's T,
|eps| norms, update counts and events must be bit-identical to the single-stream sequence -- a one-stream context driven through
photo_set_ref / photo_align as dvo_amd::RGBDOdometry::processFrame drives it -- run on that stream's frames alone."""
import os
import signal
import subprocess
from contextlib import contextmanager

import numpy as np
import pytest

import frame_gen

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K640 = (525.0, 525.0, 319.5, 239.5)
LEVELS = (3, 2)


@contextmanager
def time_limit(seconds):
    def boom(*_):
        raise TimeoutError("test case exceeded %d s" % seconds)
    old = signal.signal(signal.SIGALRM, boom)
    signal.alarm(seconds)
    try:
        yield
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def _K(rows, cols):
    return (525.0 * cols / 640, 525.0 * cols / 640, (cols - 1) / 2.0, (rows - 1) / 2.0)


def camera(seed, rows=480, cols=640, shift=(0, 0)):
    """bgr8 + depth in u16 millimetres (no zeros), as test_gpu_photo.py builds them"""
    bgr, depth_m = frame_gen.camera_frame(seed, rows, cols, shift=shift)
    d = np.nan_to_num(np.round(depth_m * 1000.0), nan=0.0, posinf=65535, neginf=0)
    return bgr, np.clip(d, 1, 65535).astype(np.uint16)


def sequence(seed, n, motion, rows=480, cols=640):
    dy, dx = motion
    return [camera(seed, rows, cols, (int(round(dy * i)), int(round(dx * i)))) for i in range(n)]


def single_stream(frames, K=K640, fixed=False, ref_every=10000, levels=LEVELS, first_level=1, **over):
    """RGBDOdometry::processFrame's engine calls on a one-stream context: [(T, norms, updates, event)] per frame; a refused reference
    gives event -1 and changes nothing (the streams engine's rule)"""
    from rgbd_odometry_amd import DvoContext, DvoError
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
    it = over.get("iterations", 3)
    out = []
    with DvoContext(1) as ctx:
        ctx.photo_configure(K, fixed=fixed, **over)
        T, n_frame = np.eye(4), 0
        for bgr, d16 in frames:
            up = lambda slot: ctx.frames_upload_cameras([bgr], [d16.astype(np.float32)], n_levels=4, first_shift=0, first_slot=slot,
                                                        flags=DVO_UPLOAD_DEPTH_RAW)
            ev = 0
            if n_frame % ref_every == 0:
                up(0)
                try:
                    ctx.photo_set_ref(0, first_level=first_level)
                except DvoError:
                    out.append((T.copy(), np.full((len(levels), it), -1.0), [0] * len(levels), -1))
                    continue
                T, ev = np.eye(4), 1
            up(1)
            T, norms, upd = ctx.photo_align(1, T, levels=levels)
            out.append((T.copy(), norms, list(upd), ev))
            n_frame += 1
    return out


def assert_same(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for n, ((T, norms, upd, ev), (wT, wn, wu, we)) in enumerate(zip(got, want)):
        assert ev == we, (what, n, ev, we)
        assert np.array_equal(T, wT), (what, n, np.abs(T - wT).max())
        assert np.array_equal(norms, wn), (what, n, norms, wn)
        assert list(upd) == list(wu), (what, n, upd, wu)


def record(res, k):
    return (res["T"][k].copy(), res["norms"][k].copy(), [int(x) for x in res["updates"][k]], int(res["event"][k]))


def streams_engine(n, K=K640, **kw):
    from rgbd_odometry_amd import DvoPhotoStreams
    return DvoPhotoStreams(n, K, **kw)


@pytest.mark.parametrize("fixed", [False, True])
def test_bit_identity_with_single_stream(oracle, fixed):
    with time_limit(900):
        n_s, n_t = 6, 8
        seqs = [sequence(50 + s, n_t, ((s % 3) - 1.0, 2.0 - (s % 5))) for s in range(n_s)]
        got = {s: [] for s in range(n_s)}
        with streams_engine(n_s, fixed=fixed, ref_every=3) as ps:
            for t in range(n_t):
                res = ps.step(list(range(n_s)), [seqs[s][t][0] for s in range(n_s)], [seqs[s][t][1] for s in range(n_s)])
                st = ps.stats()
                assert st["ref_events"] == (n_s if t % 3 == 0 else 0) and st["refused"] == 0 and st["runs"] == 1, (t, st)
                for s in range(n_s):
                    got[s].append(record(res, s))
        for s in range(n_s):
            assert [g[3] for g in got[s]] == [1 if t % 3 == 0 else 0 for t in range(n_t)]
            assert_same(got[s], single_stream(seqs[s], fixed=fixed, ref_every=3), "stream %d" % s)
        # against the CPU oracle's restatement: frame 0 aligned to itself from T = I, frame 1 from frame 0's T
        for s in range(2):
            pyr = [[(oracle.bgr2gray(oracle.resize_nn(b, 0.5 ** l)), oracle.resize_nn(d, 0.5 ** l)) for l in range(4)] for b, d in seqs[s][:2]]
            Tw = np.eye(4)
            for n in range(2):
                Tw, _ = oracle.photo_track(pyr[0], pyr[n], K640, T0=Tw, fixed=fixed)
                T = got[s][n][0]
                assert np.abs(T - Tw).max() <= 1e-9 * max(1.0, np.abs(Tw).max()), (s, n, np.abs(T - Tw).max())
                Tw = T.copy()


def _runs(streams):
    s = sorted(streams)
    return 1 + sum(1 for a, b in zip(s, s[1:]) if b != a + 1)


def test_subsets_late_join_skip_and_reset():
    """steps list streams out of order and non-consecutively; stream 5 joins late, stream 2 skips three ticks, stream 4 is reset"""
    with time_limit(900):
        n_s, n_t, every = 6, 10, 4
        seqs = [sequence(200 + s, n_t, (1.0 - (s % 3), (s % 2) + 0.5)) for s in range(n_s)]
        received = {s: [] for s in range(n_s)}
        got = {s: [] for s in range(n_s)}
        with streams_engine(n_s, ref_every=every) as ps:
            for t in range(n_t):
                streams = [s for s in (4, 0, 3, 1, 5, 2) if not (s == 5 and t < 3) and not (s == 2 and t in (4, 5, 6))]
                if t % 2:
                    streams = [s for s in streams if s != 1]        # stream 1 every other tick: non-consecutive lists
                if t == 6:
                    ps.reset(4)
                    received[4].append("reset")
                idx = {s: len([x for x in received[s] if x != "reset"]) for s in streams}
                res = ps.step(streams, [seqs[s][idx[s]][0] for s in streams], [seqs[s][idx[s]][1] for s in streams])
                assert ps.stats()["runs"] == _runs(streams), (t, streams, ps.stats())
                for k, s in enumerate(streams):
                    received[s].append(idx[s])
                    got[s].append(record(res, k))
        for s in range(n_s):
            parts, cur = [], []
            for x in received[s]:
                if x == "reset":
                    parts.append(cur); cur = []
                else:
                    cur.append(x)
            parts.append(cur)
            want = []
            for part in parts:
                want += single_stream([seqs[s][i] for i in part], ref_every=every)
            assert_same(got[s], want, "stream %d" % s)
        assert got[4][6][3] == 1                                   # the reset stream's next frame is a reference


def _check_refusals(ps, frames_of, n_t, expect_refused, **single_kw):
    """step all streams n_t ticks; refused (stream, tick) pairs must be exactly expect_refused, every stream must equal its single-stream
    sequence with the refused frames removed"""
    n_s = len(frames_of)
    got = {s: [] for s in range(n_s)}
    refused = set()
    for t in range(n_t):
        res = ps.step(list(range(n_s)), [frames_of[s][t][0] for s in range(n_s)], [frames_of[s][t][1] for s in range(n_s)])
        assert ps.stats()["refused"] == sum(1 for s in range(n_s) if (s, t) in expect_refused)
        for s in range(n_s):
            r = record(res, s)
            if r[3] == -1:
                refused.add((s, t))
                prev = got[s][-1][0] if got[s] else np.eye(4)
                assert np.array_equal(r[0], prev) and (r[1] == -1).all() and r[2] == [0] * len(LEVELS)
            else:
                got[s].append(r)
    assert refused == set(expect_refused), refused
    for s in range(n_s):
        kept = [frames_of[s][t] for t in range(n_t) if (s, t) not in refused]
        assert_same(got[s], single_stream(kept, **single_kw), "stream %d" % s)


def test_per_stream_refusal_min_points():
    """a flat frame on a reference tick: too few textured pixels (:500) -- that stream reports -1 and keeps its state, the others go on"""
    with time_limit(900):
        n_t, every = 7, 3
        seqs = [sequence(300 + s, n_t, (1.0, -1.0 + s)) for s in range(3)]
        flat = (np.full((480, 640, 3), 128, np.uint8), seqs[1][3][1])
        seqs[1][3] = flat                                          # tick 3 is a reference tick of every stream
        seqs[2][0] = flat                                          # a stream that has no reference yet retries on its next frame
        with streams_engine(3, ref_every=every) as ps:
            _check_refusals(ps, seqs, n_t, {(1, 3), (2, 0)}, ref_every=every)


def test_per_stream_refusal_capacity():
    """max_jacobian_size = n of level 1 (:464 asserts before every scanned pixel): n == cap is refused unless the last scanned pixel is
    selected, n > cap is refused; the other streams in the same steps are unaffected"""
    with time_limit(900):
        bgr, d16 = camera(3)
        bgr_last = bgr.copy()
        r, c = 2 * (240 - 1), 2 * (320 - np.arange(3, 0, -1))      # level 1 samples the full frame at (2i, 2j) (INTER_NEAREST)
        bgr[r, c] = np.array([0, 90, 200], np.uint8)[:, None]      # last row of level 1 ends 0, 90, 200: last pixel not selected
        bgr_last[r, c] = np.array([0, 200, 90], np.uint8)[:, None]  # 0, 200, 90: last pixel selected, same count
        from rgbd_odometry_amd import DvoContext
        from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
        with DvoContext(1) as ctx:                                 # level-1 counts of the candidate frames
            cands = [bgr, bgr_last] + [camera(s)[0] for s in range(20, 32)]
            ctx.frames_reserve(len(cands))
            ctx.frames_upload_cameras(cands, [d16.astype(np.float32)] * len(cands), n_levels=4, first_shift=0, flags=DVO_UPLOAD_DEPTH_RAW)
            ctx.photo_configure(K640, max_jacobian_size=10 ** 6)
            counts = [ctx.photo_set_ref(i)[1] for i in range(len(cands))]
        n = counts[0]
        assert counts[1] == n
        big = next(cands[i] for i in range(2, len(cands)) if counts[i] > n)
        nows = sequence(3, 4, (1.0, -1.0))
        frames_of = [
            [(bgr, d16), (bgr_last, d16), nows[1], nows[2]],      # refused (n == cap, last not selected), then accepted
            [(bgr_last, d16), nows[1], nows[2], nows[3]],         # accepted at once
            [(big, d16), (bgr_last, d16), nows[2], nows[3]],      # refused (n > cap), then accepted
        ]
        with streams_engine(3, max_jacobian_size=n) as ps:
            _check_refusals(ps, frames_of, 4, {(0, 0), (2, 0)}, max_jacobian_size=n)


def test_jacobians_match_single_stream():
    with time_limit(600):
        from rgbd_odometry_amd import DvoContext
        from rgbd_odometry_amd.capi import DVO_UPLOAD_DEPTH_RAW
        frames = [camera(60 + s, shift=(s, -s)) for s in range(3)]
        for fixed in (False, True):
            with streams_engine(3, fixed=fixed) as ps:
                ps.step([2, 0, 1], [frames[s][0] for s in (2, 0, 1)], [frames[s][1] for s in (2, 0, 1)])
                for s in range(3):
                    with DvoContext(1) as ctx:
                        ctx.frames_upload_cameras([frames[s][0]], [frames[s][1].astype(np.float32)], n_levels=4, first_shift=0,
                                                  flags=DVO_UPLOAD_DEPTH_RAW)
                        ctx.photo_configure(K640, fixed=fixed)
                        ctx.photo_set_ref(0, first_level=1)
                        for l in (1, 2, 3):
                            want, got = ctx.photo_jacobian(l), ps.jacobian(s, l)
                            assert got["n"] == want["n"] > 100
                            for k in ("J", "sel_i", "sel_j", "A"):
                                assert np.array_equal(got[k], want[k]), (fixed, s, l, k)


@pytest.mark.parametrize("rows,cols,cap", [(481, 641, 50000), (1200, 2112, 400000)])
def test_shapes(rows, cols, cap):
    """odd sizes, and a level wider than 1024 columns (level 1 of 1200 x 2112 is 600 x 1056): two columns per scan thread"""
    with time_limit(900):
        K = _K(rows, cols)
        seqs = [sequence(70 + s, 3, (1.0, -1.0 - s), rows, cols) for s in range(2)]
        got = {s: [] for s in range(2)}
        with streams_engine(2, K, rows=rows, cols=cols, ref_every=2, levels=(3, 2, 1), max_jacobian_size=cap) as ps:
            for t in range(3):
                res = ps.step([1, 0], [seqs[s][t][0] for s in (1, 0)], [seqs[s][t][1] for s in (1, 0)])
                got[1].append(record(res, 0))
                got[0].append(record(res, 1))
        for s in range(2):
            assert_same(got[s], single_stream(seqs[s], K, ref_every=2, levels=(3, 2, 1), max_jacobian_size=cap), "stream %d" % s)


def test_scale_256_streams_and_launch_counts():
    """256 streams with frames in HBM: a sample is bit-equal to single-stream; an ordinary tick is the upload launches + 1 Gauss-Newton
    launch and 1 host synchronisation at K = 8 and K = 256 alike; a reference tick adds the same launches at both K and one more sync
    (tick 3; the first step also allocates the frame store)"""
    import torch
    from rgbd_odometry_amd.capi import DVO_UPLOAD_DEVICE
    with time_limit(1500):
        n_seq, n_t, every = 16, 5, 3
        seqs = [sequence(900 + q, n_t, ((q % 5) * 0.5 - 1.0, (q % 3) * 0.5 - 0.5)) for q in range(n_seq)]
        dev = [[(torch.from_numpy(b).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()) for b, d in q] for q in seqs]
        stats, sample = {}, {}
        for k in (8, 256):
            st = []
            with streams_engine(k, ref_every=every) as ps:
                for t in range(n_t):
                    res = ps.step(list(range(k)), [dev[s % n_seq][t][0].data_ptr() for s in range(k)],
                                  [dev[s % n_seq][t][1].data_ptr() for s in range(k)], flags=DVO_UPLOAD_DEVICE)
                    st.append(ps.stats())
                    assert (res["event"] == (1 if t % every == 0 else 0)).all()
                    for s in (0, 5, k - 1):
                        sample.setdefault((k, s), []).append(record(res, s))
            stats[k] = st
        for (k, s), got in sample.items():
            assert_same(got, single_stream(seqs[s % n_seq], ref_every=every), "K %d stream %d" % (k, s))
        print(stats)
        for k in (8, 256):
            assert all(x["runs"] == 1 for x in stats[k])
            assert all(stats[k][t]["syncs"] == 1 and stats[k][t]["ref_events"] == 0 for t in (1, 2, 4)), stats[k]
            assert stats[k][3]["syncs"] == 2 and stats[k][3]["ref_events"] == k, stats[k]
        for t in range(n_t):
            assert stats[8][t]["launches"] == stats[256][t]["launches"], (t, stats[8][t], stats[256][t])
        # ordinary ticks: the same count; a reference tick adds select (count + scan) and fill (J + A) per reference level 1..3
        assert stats[256][1]["launches"] == stats[256][2]["launches"] == stats[256][4]["launches"]
        assert stats[256][3]["launches"] - stats[256][4]["launches"] == 12


def test_refusals_change_nothing():
    from rgbd_odometry_amd import DvoError
    from rgbd_odometry_amd.capi import DVO_ERR_INVALID
    with time_limit(900):
        n_t, every = 4, 2
        seqs = [sequence(400 + s, n_t, (1.0, 1.0 - s)) for s in range(3)]
        for bad in (dict(levels=(3, 0)), dict(first_level=2, levels=(3, 1)), dict(iterations=33), dict(levels=(4,)), dict(ref_every=0)):
            with pytest.raises(DvoError) as ei:
                streams_engine(3, **bad)
            assert ei.value.code == DVO_ERR_INVALID, bad
        got = {s: [] for s in range(3)}
        with streams_engine(3, ref_every=every) as ps:
            for t in range(n_t):
                b, d = seqs[0][t]
                for streams in ([0, 3], [1, 1], [0, 1, 2, 0], [-1], []):
                    with pytest.raises(DvoError) as ei:
                        ps.step(streams, [b] * len(streams), [d] * len(streams))
                    assert ei.value.code == DVO_ERR_INVALID, streams
                with pytest.raises(DvoError) as ei:                # geometry other than the handle's
                    ps.step([0], [b[:240]], [d[:240]])
                assert ei.value.code == DVO_ERR_INVALID
                res = ps.step([0, 1, 2], [q[t][0] for q in seqs], [q[t][1] for q in seqs])
                for s in range(3):
                    got[s].append(record(res, s))
        for s in range(3):
            assert_same(got[s], single_stream(seqs[s], ref_every=every), "stream %d" % s)


MIRROR = r"""
#include "dvo_amd.hpp"
#include <cstdio>
#include <fstream>
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    int hdr[4];
    in.read((char *)hdr, sizeof(hdr));
    const int S = hdr[0], N = hdr[1], rows = hdr[2], cols = hdr[3];
    const size_t npx = (size_t)rows * cols;
    std::vector<std::vector<unsigned char>> bgr((size_t)S * N, std::vector<unsigned char>(npx * 3));
    std::vector<std::vector<unsigned short>> dep((size_t)S * N, std::vector<unsigned short>(npx));
    for (int s = 0; s < S; s++)
        for (int n = 0; n < N; n++) {
            in.read((char *)bgr[(size_t)s * N + n].data(), npx * 3);
            in.read((char *)dep[(size_t)s * N + n].data(), npx * 2);
        }
    if (!in) { std::fprintf(stderr, "cannot read frames\n"); return 1; }
    dvo_amd::RGBDOdometryStreams multi(S, false, rows, cols);
    multi.refEvery = 3;
    multi.setCameraMatrix(525.0, 525.0, 319.5, 239.5);
    std::vector<dvo_amd::RGBDOdometry *> one;
    for (int s = 0; s < S; s++) {
        one.push_back(new dvo_amd::RGBDOdometry(false));
        one[s]->refEvery = 3;
        one[s]->setCameraMatrix(525.0, 525.0, 319.5, 239.5);
    }
    int differ = 0;
    for (int n = 0; n < N; n++) {
        std::vector<int> streams;
        std::vector<const unsigned char *> b;
        std::vector<const unsigned short *> d;
        for (int s = S - 1; s >= 0; s--) { streams.push_back(s); b.push_back(bgr[(size_t)s * N + n].data()); d.push_back(dep[(size_t)s * N + n].data()); }
        std::vector<dvo_amd::Pose> pm = multi.processFrames(streams, b, d);
        for (size_t i = 0; i < streams.size(); i++) {
            const int s = streams[i];
            one[s]->setRcvdFrame(b[i], d[i], rows, cols);
            const dvo_amd::Pose p1 = one[s]->processFrame(), &p2 = pm[i];
            const double a[7] = {p1.px, p1.py, p1.pz, p1.qx, p1.qy, p1.qz, p1.qw}, c[7] = {p2.px, p2.py, p2.pz, p2.qx, p2.qy, p2.qz, p2.qw};
            std::printf("stream %d frame %d event %d", s, n, multi.lastEvents[i]);
            for (int k = 0; k < 7; k++) { std::printf(" %a/%a", a[k], c[k]); differ += a[k] != c[k]; }
            std::printf("\n");
        }
    }
    for (auto *o : one) delete o;
    std::printf("differ %d\n", differ);
    return differ ? 3 : 0;
}
"""


def test_cpp_mirror_matches_rgbd_odometry(tmp_path):
    """dvo_amd::RGBDOdometryStreams for 3 streams and 3 separate dvo_amd::RGBDOdometry objects on the same frames publish identical poses"""
    with time_limit(900):
        S, N = 3, 5
        seqs = [sequence(500 + s, N, (1.0, 0.5 * s - 0.5)) for s in range(S)]
        with open(tmp_path / "frames.bin", "wb") as f:
            f.write(np.array([S, N, 480, 640], np.int32).tobytes())
            for s in range(S):
                for b, d in seqs[s]:
                    f.write(np.ascontiguousarray(b).tobytes())
                    f.write(np.ascontiguousarray(d).tobytes())
        src, exe = tmp_path / "mirror.cpp", tmp_path / "mirror"
        src.write_text(MIRROR)
        lib = os.path.join(ROOT, "rgbd_odometry_amd", "lib")
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", lib,
                            "-ldvo_amd", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        run = subprocess.run([str(exe), str(tmp_path / "frames.bin")], capture_output=True, text=True, timeout=600)
        print(run.stdout[-2000:])
        assert run.returncode == 0 and "differ 0" in run.stdout, (run.returncode, run.stdout[-3000:], run.stderr[-2000:])
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("stream")]
        assert len(lines) == S * N
        assert sum(" event 1 " in ln for ln in lines) == S * 2                # frames 0 and 3 renew the reference
