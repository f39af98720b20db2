"""Place descriptors of the key-frame archive (include/dvo_amd.h: dvo_tracker_set_places / dvo_tracker_query_places), restated in
numpy.  Everything is integer arithmetic, so the device's descriptors and distances are compared with these for equality."""
import numpy as np


def column_major(grey_rows_cols):
    """a (rows, cols) grey level in the frame store's order: column after column"""
    return np.ascontiguousarray(np.asarray(grey_rows_cols, np.uint8).T).ravel()


def descriptor(grey_u8_colmajor):
    """b_i = clamp(a_i - m + 128, 0, 255) with m = (2 S + D) / (2 D): the mean of the D bytes, rounded half up"""
    a = np.asarray(grey_u8_colmajor, np.uint8).ravel().astype(np.int64)
    D = a.size
    m = (2 * int(a.sum()) + D) // (2 * D)
    return np.clip(a - m + 128, 0, 255).astype(np.uint8)


def distance(a, b):
    a, b = np.asarray(a, np.uint8).astype(np.int64), np.asarray(b, np.uint8).astype(np.int64)
    assert a.shape == b.shape
    return int(np.abs(a - b).sum())


def top_k(query, rows, ids, allowed, k):
    """[(id, distance)] of the k allowed rows nearest to `query`, ordered by (distance, id)"""
    cand = sorted((distance(query, r), int(i)) for r, i, ok in zip(rows, ids, allowed) if ok)
    return [(i, d) for d, i in cand[:k]]
