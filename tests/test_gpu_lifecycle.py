"""Device memory over the life of a multi-stream tracker: everything a tracker allocates -- its own buffers, the views, the key-frame
archive with its match context, the place descriptors -- goes back when it is re-configured, switched off and closed.

Six trackers in a row in one process; the free device memory after the second and after the last must agree to within the smallest
of the large slabs one repetition allocates (computed below from the shapes used), so a repetition that leaks any one of them once
fails.  The first two repetitions absorb what the runtime keeps for itself (code objects, its own pools)."""
import pytest

import test_gpu_tracker_information as TI

pytestmark = pytest.mark.gpu

N_S, N_T, REPS = 4, 3, 6
CAPACITY, CAPACITY_2, MAX_MATCHES = 256, 224, 2


def view_slab_bytes():
    """dvo_tracker_set_views: two planes of N_S BGR images of the finest level, each image rounded up to 256 bytes"""
    rows, cols = TI.level_dims(0)
    return 2 * N_S * ((rows * cols * 3 + 255) // 256 * 256)


def ring_cpts_bytes(capacity):
    """dvo_tracker_set_archive: the level-0 ring of 8-byte points, rows * cols / 8 per slot rounded up to whole chunks of 64"""
    rows, cols = TI.level_dims(0)
    return capacity * ((rows * cols // 8 + 63) // 64 * 64) * 8


def test_six_trackers_return_their_memory():
    import torch
    assert min(ring_cpts_bytes(CAPACITY), ring_cpts_bytes(CAPACITY_2)) >= 16 << 20
    allowed = min(view_slab_bytes(), ring_cpts_bytes(CAPACITY), ring_cpts_bytes(CAPACITY_2))
    seqs = [TI.sequence(900 + s, N_T, TI.MOTIONS[s]) for s in range(N_S)]
    free = {}
    for rep in range(REPS):
        tr = TI.make_tracker(N_S)                               # information on
        tr.set_views(True)
        tr.set_archive(CAPACITY, MAX_MATCHES)
        tr.set_places()
        for n in range(N_T):
            tr.step(list(range(N_S)), [seqs[s][n][0] for s in range(N_S)], [seqs[s][n][1] for s in range(N_S)])
        assert tr.archive_stats()["archived"] >= N_S            # the first frames are key frames: the ring and the descriptors are in use
        tr.set_archive(CAPACITY_2, MAX_MATCHES)
        tr.set_archive(0)
        tr.close()
        free[rep] = torch.cuda.mem_get_info()[0]
    drift = abs(free[1] - free[REPS - 1])
    print("free after each repetition (MB):", [round(free[r] / 1e6, 2) for r in range(REPS)], "drift %d bytes, allowed < %d" % (drift, allowed))
    assert drift < allowed, (free, allowed)
