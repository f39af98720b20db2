"""Depth fusion on the device at every layout of the pool (include/dvo_amd.h, "depth fusion", "from the map back to depth", "triangle
meshes", "colour in the map"): the 23 packed volumes of tests/tsdf_map_reference.py in one handle whose pool is exactly their sum.  A
thread of the integrate kernel owns an aligned group of four POOL words, and the extract, mesh and ray-cast kernels read pool + off at
every alignment with a neighbour right behind the last word: none of that has a counterpart in the host definitions, so it is tested
here by what it must leave alone -- tr.check_packed_pool, which tests/test_tsdf_map_cpu.py shows to fail on three wrong stand-ins of a
handle -- and by byte equality of every read with the host definition, per volume.  All comparisons are byte equality."""
import numpy as np
import pytest

import tsdf_colour_reference as cr
import tsdf_map_reference as tr
import tsdf_raycast_reference as rr

pytestmark = pytest.mark.gpu
VOLS = tr.PACKED_VOLUMES
NV = len(VOLS)
ROWS, COLS = tr.ROWS, tr.COLS
#: three of the fusion poses, every volume seen from each: one ray-cast call of 69 views
VIEW_POSES = list(tr.PACKED_FRAMES)
VIEW_VOLUMES = [v for v in range(NV) for _ in VIEW_POSES]
THIN = [v for v, vol in enumerate(VOLS) if min(vol["dims"]) == 1]


def c_volume(vol):
    from rgbd_odometry_amd import capi
    return capi.DvoTsdfVolume.make(vol["dims"], vol["voxel_size"], vol["origin"], vol["trunc"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def new_handle(vols, colour=False):
    """the volumes, cleared, set in order in a pool that is exactly their sum"""
    from rgbd_odometry_amd import capi
    h = capi.DvoTsdfVolumes(len(vols), sum(tr.voxels_of(v) for v in vols))
    if colour:
        h.enable_colour()
    for i, vol in enumerate(vols):
        h.set_volume(i, c_volume(vol))
    return h


class DeviceImages:
    """a handle whose integrate calls hand over device-resident images"""

    def __init__(self, h):
        self.h = h
        for name in ("set_voxels", "voxels", "set_colours", "get_colours", "stats", "close"):
            setattr(self, name, getattr(h, name))

    @staticmethod
    def _dev(imgs):
        import torch
        dev = [torch.from_numpy(i.view(np.int16) if i.dtype == np.uint16 else i).cuda().contiguous() for i in imgs]
        torch.cuda.synchronize()
        return dev

    def integrate(self, volumes, imgs, K, poses):
        self.h.integrate(volumes, self._dev(imgs), K, poses, device=True)

    def integrate_colour(self, volumes, imgs, images, K, poses, image_format="bgr8"):
        self.h.integrate_colour(volumes, self._dev(imgs), self._dev(images), K, poses, image_format=image_format, device=True)


# ---- the integrate kernels: word ownership ----

def test_packed_pool():
    """the plain kernel (a handle without a colour pool), host-staged images, both depth formats"""
    tr.check_packed_pool(new_handle)


@pytest.mark.parametrize("fmt", ["bgr8", "rgb8", "mono8"])
def test_packed_pool_with_colour(fmt):
    """the colour kernel: the same for the words, and the colour words of an unlisted volume stay too"""
    tr.check_packed_pool(lambda vols: new_handle(vols, colour=True), image_format=fmt)


@pytest.mark.parametrize("fmt", [None, "bgr8"])
def test_packed_pool_with_device_images(fmt):
    tr.check_packed_pool(lambda vols: DeviceImages(new_handle(vols, colour=fmt is not None)), image_format=fmt)


# ---- the kernels that read: extract, mesh, ray cast ----

_state = {}


def fused_state():
    """[(words, colour words)] per volume: tr.PACKED_FRAMES with the random bgr8 images into a cleared pool, by the host definition"""
    from rgbd_odometry_amd import capi
    if "fused" not in _state:
        imgs, poses = tr.frame_list("u16")
        pics = cr.images("random", "bgr8")
        idx = list(tr.PACKED_FRAMES)
        _state["fused"] = [capi.tsdf_integrate_colour_host(c_volume(vol), None, None, [imgs[i] for i in idx], [pics[i] for i in idx], tr.K4, poses[idx],
                                                           image_format="bgr8") for vol in VOLS]
    return _state["fused"]


def random_state():
    """random words with weights 0 .. 3 and random colour words: what lies one word past a volume's end is random bits"""
    return [(rr.random_words(vol, seed=40 + v), cr.random_colours(vol, seed=v)) for v, vol in enumerate(VOLS)]


def host_reads(state):
    """what the host definitions read from the state: dict of (kind, volume, min_weight[, depth format]) -> arrays"""
    from rgbd_odometry_amd import capi
    poses = np.stack(tr.POSES)[VIEW_POSES]
    out = {}
    for v, (vol, (w, c)) in enumerate(zip(VOLS, state)):
        cv = c_volume(vol)
        for mw in (1, 2):
            out["points", v, mw] = capi.tsdf_extract_host(cv, w, mw)
            out["mesh", v, mw] = capi.tsdf_mesh_host(cv, w, mw)
            out["colour mesh", v, mw] = capi.tsdf_mesh_colour_host(cv, w, c, mw)
            p = capi.DvoRaycastParams.default(min_weight=mw)
            for fmt in ("u16", "f32"):
                out["views", v, mw, fmt] = capi.tsdf_raycast_host(cv, w, tr.K4, poses, ROWS, COLS, p, fmt, True)
                out["colour views", v, mw, fmt] = capi.tsdf_raycast_colour_host(cv, w, c, tr.K4, poses, ROWS, COLS, p, fmt, image_format="rgb8", normals=True)
    return out


def check_thin_volumes(want):
    """a volume with a dimension of 1 has no cell of eight voxels: no triangle and no hit, whatever its words"""
    for v in THIN:
        for mw in (1, 2):
            assert len(want["mesh", v, mw][1]) == 0 and len(want["colour mesh", v, mw][1]) == 0, v
            for fmt in ("u16", "f32"):
                assert not want["views", v, mw, fmt][0].any() and not want["views", v, mw, fmt][1].any() and not want["colour views", v, mw, fmt][2].any(), v


def check_reads(h, state, want):
    """every read of every volume against the host's, and the pool unchanged after them"""
    from rgbd_odometry_amd import capi
    poses = np.stack(tr.POSES)[VIEW_POSES]
    for v in range(NV):
        h.set_voxels(v, state[v][0])
        h.set_colours(v, state[v][1])
    for mw in (1, 2):
        for v in range(NV):
            pts, n = h.points(v, mw)
            assert h.stats() == (capi.DVO_TSDF_EXTRACT_LAUNCHES, 1)
            assert n == want["points", v, mw][1] and same_bits(pts, want["points", v, mw][0]), ("points", v, mw, n, want["points", v, mw][1])
            for got, ref in zip(h.extract_mesh(v, mw), want["mesh", v, mw]):
                assert same_bits(got, ref), ("mesh", v, mw, got.shape, ref.shape)
            for got, ref in zip(h.extract_mesh(v, mw, colours=True), want["colour mesh", v, mw]):
                assert same_bits(got, ref), ("colour mesh", v, mw, got.shape, ref.shape)
        p = capi.DvoRaycastParams.default(min_weight=mw)
        for fmt in ("u16", "f32"):
            depth, nrm = h.raycast(VIEW_VOLUMES, tr.K4, np.tile(poses, (NV, 1)), ROWS, COLS, p, fmt, normals=True)
            assert h.stats() == (capi.DVO_RAYCAST_LAUNCHES, 1)
            cdepth, cnrm, img = h.raycast(VIEW_VOLUMES, tr.K4, np.tile(poses, (NV, 1)), ROWS, COLS, p, fmt, normals=True, image_format="rgb8")
            k = len(VIEW_POSES)
            for v in range(NV):
                d, n = want["views", v, mw, fmt]
                assert same_bits(depth[k * v:k * v + k], d) and same_bits(nrm[k * v:k * v + k], n), ("views", v, mw, fmt, int((depth[k * v:k * v + k] != d).sum()))
                d, n, m = want["colour views", v, mw, fmt]
                assert same_bits(cdepth[k * v:k * v + k], d) and same_bits(cnrm[k * v:k * v + k], n) and same_bits(img[k * v:k * v + k], m), ("colour views", v, mw, fmt)
    for v in range(NV):
        assert same_bits(h.voxels(v), state[v][0]) and same_bits(h.get_colours(v), state[v][1]), "a read changed volume %d" % v


@pytest.fixture(scope="module")
def handle():
    h = new_handle(VOLS, colour=True)
    yield h
    h.close()


def test_reads_of_the_fused_pool(handle):
    """points, meshes and ray-cast views of all 23 volumes after the fusion from cleared, min_weight 1 and 2"""
    state = fused_state()
    want = host_reads(state)
    check_thin_volumes(want)
    # a thin volume still has points where its long axis crosses the surface; five volumes and more have triangles; rays hit
    assert sum(want["points", v, 1][1] > 0 for v in THIN) >= 3, [want["points", v, 1][1] for v in THIN]
    assert sum(len(want["mesh", v, 1][1]) > 0 for v in range(NV)) >= 5, [len(want["mesh", v, 1][1]) for v in range(NV)]
    assert sum(int((want["views", v, 1, "f32"][0] > 0).sum()) for v in range(NV)) >= 100
    assert sum(int(want["colour views", v, 1, "f32"][2].any(axis=-1).sum()) for v in range(NV)) >= 100
    check_reads(handle, state, want)


def test_reads_of_random_words(handle):
    """the same reads after dvo_tsdf_set_voxels of random words into every volume: a read one word past a volume's end lands in random
    bits and shows as a point, a triangle or a pixel the host does not have"""
    state = random_state()
    want = host_reads(state)
    check_thin_volumes(want)
    assert sum(want["points", v, 1][1] > 0 for v in THIN) >= 5 and sum(len(want["mesh", v, 2][1]) > 0 for v in range(NV)) >= 5
    check_reads(handle, state, want)
