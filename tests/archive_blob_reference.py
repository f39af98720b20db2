"""The key-frame archive blob, format version 1, in numpy: builder, parser, validator and checksum, written from the text of
include/dvo_amd.h ("export and import of the key-frame archive") and from nothing else.

A key frame is a dict:
    origin_id, origin_stream, origin_frame   ints
    K                                        (4,) float32: fx, fy, cx, cy
    levels                                   per level dict(cpts (N, 2) uint32, cidx (N,) uint32, cpt4 (N,) uint32, chdr (ceil(N / 64),) uint32,
                                             pt4_ok 0 / 1); cpt4 and chdr are written as zeros where pt4_ok == 0
    desc                                     (D,) uint8 or None
"""
import struct

import numpy as np

MAGIC = b"DVOKFAR1"
VERSION = 1
MAX_LEVELS = 8
HEADER = struct.Struct("<8sIIQQQiiiiiiiiQ")
RECORD = struct.Struct("<qiiq4f8i8iiiQQQQ")
HEADER_BYTES, RECORD_BYTES = 80, 144
assert HEADER.size == HEADER_BYTES and RECORD.size == RECORD_BYTES
M64 = (1 << 64) - 1


class BlobError(ValueError):
    pass


def pad16(n):
    return (n + 15) & ~15


def checksum(data) -> int:
    """sum_i mix(w_i | (i + 1) << 32) mod 2^64 over the u32 words of `data`, mix = the splitmix64 finaliser"""
    w = np.frombuffer(bytes(data), "<u4").astype(np.uint64)
    if w.size == 0:
        return 0
    with np.errstate(over="ignore"):
        z = w | ((np.arange(w.size, dtype=np.uint64) + np.uint64(1)) << np.uint64(32))
        z ^= z >> np.uint64(30); z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27); z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return int(np.add.reduce(z, dtype=np.uint64))


def checksum_scalar(data) -> int:
    """the same in Python integers, word by word (a check of the vectorised form)"""
    total = 0
    for i, (w,) in enumerate(struct.iter_unpack("<I", bytes(data))):
        z = w | ((i + 1) << 32)
        z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
        z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
        z ^= z >> 31
        total = (total + z) & M64
    return total


def section_sizes(N):
    """unpadded bytes of cpts, cidx, cpt4, chdr of a level with N points"""
    return [8 * N, 4 * N, 4 * N, 4 * ((N + 63) // 64)]


def payload_size(Ns, has_desc, D):
    return sum(pad16(s) for N in Ns for s in section_sizes(N)) + (pad16(D) if has_desc else 0)


def _padded(b):
    return b + bytes(pad16(len(b)) - len(b))


def payload_of(kf, n_levels, D):
    out = b""
    assert len(kf["levels"]) == n_levels
    for L in kf["levels"]:
        N = len(L["cidx"])
        cpts = np.ascontiguousarray(L["cpts"], "<u4").reshape(N, 2)
        cpt4 = np.ascontiguousarray(L["cpt4"], "<u4") if L["pt4_ok"] else np.zeros(N, "<u4")
        chdr = np.ascontiguousarray(L["chdr"], "<u4") if L["pt4_ok"] else np.zeros((N + 63) // 64, "<u4")
        assert len(cpt4) == N and len(chdr) == (N + 63) // 64
        for a in (cpts, np.ascontiguousarray(L["cidx"], "<u4"), cpt4, chdr):
            out += _padded(a.tobytes())
    if kf.get("desc") is not None:
        d = np.ascontiguousarray(kf["desc"], np.uint8)
        assert d.size == D
        out += _padded(d.tobytes())
    return out


def build(key_frames, rows, cols, n_levels, first_shift, places_level=-1, D=0) -> bytes:
    n = len(key_frames)
    payloads = [payload_of(kf, n_levels, D) for kf in key_frames]
    offset = HEADER_BYTES + RECORD_BYTES * n
    table = b""
    for kf, p in zip(key_frames, payloads):
        Ns = [len(L["cidx"]) for L in kf["levels"]] + [0] * (MAX_LEVELS - n_levels)
        ok = [int(bool(L["pt4_ok"])) for L in kf["levels"]] + [0] * (MAX_LEVELS - n_levels)
        table += RECORD.pack(kf["origin_id"], kf["origin_stream"], 0, kf["origin_frame"], *[float(np.float32(k)) for k in kf["K"]], *Ns, *ok,
                             int(kf.get("desc") is not None), 0, offset, len(p), checksum(p), 0)
        offset += len(p)
    header = HEADER.pack(MAGIC, VERSION, 0, HEADER_BYTES, RECORD_BYTES, offset, n, rows, cols, n_levels, first_shift, places_level, D, 0,
                         checksum(table))
    return header + table + b"".join(payloads)


def set_table_checksum(blob: bytearray):
    """after an edit of the table: the header's checksum follows (so that the edit itself is what a validator meets)"""
    n = struct.unpack_from("<i", blob, 40)[0]
    struct.pack_into("<Q", blob, 72, checksum(blob[HEADER_BYTES:HEADER_BYTES + RECORD_BYTES * max(n, 0)]))


def validate(blob, payloads=True):
    """header and table (what dvo_archive_blob_info validates; payloads=True: the payload checksums too).  Returns
    (info dict, list of record dicts); raises BlobError naming the first defect"""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise BlobError("shorter than a header")
    (magic, version, z0, hb, rb, total, n, rows, cols, n_levels, first_shift, places_level, D, z1, table_sum) = HEADER.unpack_from(blob, 0)
    if magic != MAGIC:
        raise BlobError("bad magic")
    if version != VERSION:
        raise BlobError("wrong version")
    if hb != HEADER_BYTES or rb != RECORD_BYTES:
        raise BlobError("header_bytes / record_bytes")
    if z0 or z1:
        raise BlobError("header padding")
    if n < 0:
        raise BlobError("negative n_key_frames")
    if rows < 1 or cols < 1 or not 1 <= n_levels <= MAX_LEVELS or first_shift < 0:
        raise BlobError("geometry")
    if places_level < -1 or places_level >= n_levels or D < 0 or (places_level < 0) != (D == 0):
        raise BlobError("places_level and D")
    table_end = HEADER_BYTES + RECORD_BYTES * n
    if total % 16 or total < table_end:
        raise BlobError("total_bytes does not hold the table")
    if total != len(blob):
        raise BlobError("truncated" if total > len(blob) else "trailing bytes")
    if checksum(blob[HEADER_BYTES:table_end]) != table_sum:
        raise BlobError("table checksum")
    records, spans = [], []
    for i in range(n):
        f = RECORD.unpack_from(blob, HEADER_BYTES + RECORD_BYTES * i)
        r = dict(origin_id=f[0], origin_stream=f[1], origin_frame=f[3], K=np.array(f[4:8], np.float32), N=list(f[8:16]), pt4_ok=list(f[16:24]),
                 has_desc=f[24], payload_offset=f[26], payload_bytes=f[27], payload_checksum=f[28])
        if f[2] or f[25] or f[29]:
            raise BlobError("record padding")
        for l in range(MAX_LEVELS):
            if r["N"][l] < 0:
                raise BlobError("negative N")
            if r["pt4_ok"][l] not in (0, 1):
                raise BlobError("pt4_ok")
            if l >= n_levels and (r["N"][l] or r["pt4_ok"][l]):
                raise BlobError("N / pt4_ok beyond n_levels")
        if r["has_desc"] not in (0, 1) or (r["has_desc"] and D == 0):
            raise BlobError("has_desc")
        if r["payload_bytes"] != payload_size(r["N"][:n_levels], r["has_desc"], D):
            raise BlobError("payload_bytes")
        if r["payload_offset"] % 16 or r["payload_offset"] < table_end or r["payload_offset"] + r["payload_bytes"] > total:
            raise BlobError("payload offset out of range")
        if r["payload_bytes"]:
            spans.append((r["payload_offset"], r["payload_bytes"]))
        records.append(r)
    spans.sort()
    for a, b in zip(spans, spans[1:]):
        if a[0] + a[1] > b[0]:
            raise BlobError("overlapping payloads")
    if payloads:
        for i, r in enumerate(records):
            if checksum(blob[r["payload_offset"]:r["payload_offset"] + r["payload_bytes"]]) != r["payload_checksum"]:
                raise BlobError("payload checksum of key frame %d" % i)
    info = dict(version=version, rows=rows, cols=cols, n_levels=n_levels, first_shift=first_shift, places_level=places_level, D=D,
                n_key_frames=n, total_bytes=total)
    return info, records


def parse(blob):
    """(info, key frames as build() takes them) of a valid blob"""
    blob = bytes(blob)
    info, records = validate(blob)
    out = []
    for r in records:
        o = r["payload_offset"]
        levels = []
        for l in range(info["n_levels"]):
            N = r["N"][l]
            arrays = []
            for size in section_sizes(N):
                arrays.append(np.frombuffer(blob, "<u4", size // 4, o).copy())
                if any(blob[o + size:o + pad16(size)]):
                    raise BlobError("section padding is not zero")
                o += pad16(size)
            levels.append(dict(cpts=arrays[0].reshape(N, 2), cidx=arrays[1], cpt4=arrays[2], chdr=arrays[3], pt4_ok=r["pt4_ok"][l]))
        desc = None
        if r["has_desc"]:
            desc = np.frombuffer(blob, np.uint8, info["D"], o).copy()
            if any(blob[o + info["D"]:o + pad16(info["D"])]):
                raise BlobError("descriptor padding is not zero")
        out.append(dict(origin_id=r["origin_id"], origin_stream=r["origin_stream"], origin_frame=r["origin_frame"], K=r["K"], levels=levels,
                        desc=desc))
    return info, out


def section_boundaries(blob):
    """every offset at which a section of the blob ends or begins: header, each record, each padded section of each payload"""
    info, records = validate(blob)
    cuts = {0, HEADER_BYTES}
    for i in range(info["n_key_frames"]):
        cuts.add(HEADER_BYTES + RECORD_BYTES * (i + 1))
    for r in records:
        o = r["payload_offset"]
        for l in range(info["n_levels"]):
            for size in section_sizes(r["N"][l]):
                o += pad16(size)
                cuts.add(o)
        if r["has_desc"]:
            cuts.add(o + pad16(info["D"]))
    return sorted(c for c in cuts if c < len(blob))


def synthetic_key_frames(seed=7):
    """two small key frames of a 3-level tracker with an 11-byte descriptor: one with N % 64 != 0 on every level, one with a level of
    N = 0 and a level without valid 4-byte twins"""
    rng = np.random.default_rng(seed)

    def level(N, ok=1):
        return dict(cpts=rng.integers(0, 2 ** 32, (N, 2), dtype=np.uint64).astype(np.uint32), cidx=rng.permutation(N).astype(np.uint32),
                    cpt4=rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32),
                    chdr=rng.integers(0, 2 ** 32, (N + 63) // 64, dtype=np.uint64).astype(np.uint32), pt4_ok=ok)
    a = dict(origin_id=3, origin_stream=1, origin_frame=4, K=np.array([262.5, 262.5, 159.75, 119.75], np.float32),
             levels=[level(70), level(65), level(1)], desc=rng.integers(0, 256, 11, dtype=np.uint8))
    b = dict(origin_id=9, origin_stream=0, origin_frame=0, K=np.array([250.0, 254.0, 161.0, 118.0], np.float32),
             levels=[level(128), level(0), level(5, ok=0)], desc=None)
    return [a, b], dict(rows=24, cols=32, n_levels=3, first_shift=0, places_level=2, D=11)
