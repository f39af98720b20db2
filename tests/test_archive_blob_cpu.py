"""The key-frame archive blob, format version 1 (include/dvo_amd.h, "export and import of the key-frame archive"), without a device:
the numpy reference (tests/archive_blob_reference.py, written from the header's text) against itself, against dvo_archive_blob_info
through ctypes, against the same validation compiled into a stand-alone program under -fsanitize=address,undefined
(tests/host/archive_blob_main.cpp), and against the committed fixture tests/golden/archive_blob_v1.bin, which pins version 1.

Every expected value is an integer or a byte string; the verdict on a defective blob is the reference's."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import archive_blob_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "archive_blob_v1.bin")
# what tests/golden/make_archive_blob_golden.py wrote, recorded when the fixture was made
GOLDEN_INFO = dict(version=1, rows=24, cols=32, n_levels=3, first_shift=0, places_level=2, D=11, n_key_frames=2, total_bytes=4880)
GOLDEN_TABLE = [
    dict(origin_id=3, origin_stream=1, origin_frame=4, has_desc=1, payload_offset=368, payload_bytes=2320, N=[70, 65, 1], pt4_ok=[1, 1, 1]),
    dict(origin_id=9, origin_stream=0, origin_frame=0, has_desc=0, payload_offset=2688, payload_bytes=2192, N=[128, 0, 5], pt4_ok=[1, 1, 0]),
]


def valid_blobs():
    kfs, geo = br.synthetic_key_frames()
    no_desc = [dict(k, desc=None) for k in kfs]
    return {
        "two key frames": br.build(kfs, **geo),
        "reordered": br.build(kfs[::-1], **geo),
        "duplicate": br.build([kfs[0], kfs[0]], **geo),
        "no descriptors": br.build(no_desc, **dict(geo, places_level=-1, D=0)),
        "empty": br.build([], **geo),
        "one level": br.build([dict(kfs[0], levels=kfs[0]["levels"][:1])], **dict(geo, n_levels=1, places_level=0)),
    }


def edit_record(blob, index, **fields):
    """a copy with fields of record `index` replaced and the table checksum recomputed: the edit itself is what the validator meets"""
    b = bytearray(blob)
    at = br.HEADER_BYTES + br.RECORD_BYTES * index
    f = list(br.RECORD.unpack_from(b, at))
    names = dict(N0=8, N1=9, ok0=16, ok2=18, has_desc=24, payload_offset=26, payload_bytes=27, payload_checksum=28, zero=29)
    for k, v in fields.items():
        f[names[k]] = v
    br.RECORD.pack_into(b, at, *f)
    br.set_table_checksum(b)
    return bytes(b)


def defective_blobs():
    good = valid_blobs()["two key frames"]
    rec1 = br.validate(good)[1][1]
    out = {}
    for cut in br.section_boundaries(good):
        out["truncated at %d" % cut] = good[:cut]
    out["truncated by one byte"] = good[:-1]
    out["truncated inside the header"] = good[:40]
    out["trailing bytes"] = good + bytes(16)
    out["bad magic"] = b"DVOKFAR2" + good[8:]
    b = bytearray(good); struct.pack_into("<I", b, 8, 2); out["wrong version"] = bytes(b)
    out["offset out of range"] = edit_record(good, 1, payload_offset=len(good))
    out["offset into the table"] = edit_record(good, 0, payload_offset=br.HEADER_BYTES)
    out["offset not a multiple of 16"] = edit_record(good, 1, payload_offset=rec1["payload_offset"] + 8)
    out["overlapping payloads"] = edit_record(good, 1, payload_offset=rec1["payload_offset"] - 16)
    out["negative N"] = edit_record(good, 0, N0=-1)
    out["N that the payload size contradicts"] = edit_record(good, 0, N1=100)
    out["pt4_ok = 2"] = edit_record(good, 0, ok0=2)
    out["has_desc = 2"] = edit_record(good, 0, has_desc=2)
    out["record padding"] = edit_record(good, 0, zero=1)
    b = bytearray(good); b[br.HEADER_BYTES + 3] ^= 0x10; out["wrong table checksum"] = bytes(b)
    b = bytearray(good); struct.pack_into("<Q", b, 72, 0); out["zero table checksum"] = bytes(b)
    b = bytearray(good); struct.pack_into("<i", b, 40, -1); out["negative n_key_frames"] = bytes(b)
    b = bytearray(good); struct.pack_into("<i", b, 40, 3); out["n_key_frames beyond the table"] = bytes(b)
    b = bytearray(good); struct.pack_into("<i", b, 52, 9); out["n_levels = 9"] = bytes(b)
    return out


def reference_verdict(blob, payloads=False):
    try:
        return br.validate(blob, payloads=payloads)[0]
    except br.BlobError:
        return None


def library_verdict(blob):
    from rgbd_odometry_amd import DvoError, capi
    try:
        return capi.archive_blob_info(blob)
    except DvoError as e:
        assert e.code == capi.DVO_ERR_INVALID and "archive blob: " in str(e), str(e)
        return None


def test_checksum_forms_agree_and_depend_on_position():
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, 4 * 257, dtype=np.uint8).tobytes()
    assert br.checksum(data) == br.checksum_scalar(data)
    assert br.checksum(b"") == 0 and br.checksum(bytes(4)) != 0                     # a zero word still counts: truncation shows
    swapped = data[4:8] + data[0:4] + data[8:]
    assert br.checksum(swapped) != br.checksum(data)
    # splitmix64's finaliser of 1 | 1 << 32, worked by hand from the header's text
    z = 1 | (1 << 32)
    z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 % 2 ** 64; z ^= z >> 27; z = z * 0x94D049BB133111EB % 2 ** 64; z ^= z >> 31
    assert br.checksum(struct.pack("<I", 1)) == z


def test_reference_round_trips():
    kfs, geo = br.synthetic_key_frames()
    for name, blob in valid_blobs().items():
        info, got = br.parse(blob)
        assert info["total_bytes"] == len(blob) and len(blob) % 16 == 0, name
        assert br.build(got, info["rows"], info["cols"], info["n_levels"], info["first_shift"], info["places_level"], info["D"]) == blob, name
    info, got = br.parse(valid_blobs()["two key frames"])
    assert {k: info[k] for k in geo} == geo
    for a, b in zip(kfs, got):
        assert (a["origin_id"], a["origin_stream"], a["origin_frame"]) == (b["origin_id"], b["origin_stream"], b["origin_frame"])
        assert a["K"].tobytes() == b["K"].tobytes()
        assert (a["desc"] is None) == (b["desc"] is None) and (a["desc"] is None or np.array_equal(a["desc"], b["desc"]))
        for La, Lb in zip(a["levels"], b["levels"]):
            assert np.array_equal(La["cpts"], Lb["cpts"]) and np.array_equal(La["cidx"], Lb["cidx"]) and La["pt4_ok"] == Lb["pt4_ok"]
            if La["pt4_ok"]:
                assert np.array_equal(La["cpt4"], Lb["cpt4"]) and np.array_equal(La["chdr"], Lb["chdr"])
            else:                                                                   # not defined in the slot: zeros in the blob
                assert not Lb["cpt4"].any() and not Lb["chdr"].any()
    # every defect is one for the reference; a flipped payload byte is one only for the payload checksums
    for name, blob in defective_blobs().items():
        assert reference_verdict(blob) is None, name
    good = bytearray(valid_blobs()["two key frames"])
    good[-20] ^= 1
    assert reference_verdict(bytes(good)) is not None and reference_verdict(bytes(good), payloads=True) is None


def test_library_agrees_with_the_reference():
    for name, blob in valid_blobs().items():
        want = reference_verdict(blob)
        assert want is not None and library_verdict(blob) == want, name
    assert library_verdict(valid_blobs()["empty"])["n_key_frames"] == 0
    for name, blob in defective_blobs().items():
        assert library_verdict(blob) is None, name
    from rgbd_odometry_amd import capi
    lib = capi.load_library()
    info = capi.DvoArchiveBlobInfo()
    blob = valid_blobs()["two key frames"]
    assert lib.dvo_archive_blob_info(None, 100, info) == capi.DVO_ERR_INVALID
    assert lib.dvo_archive_blob_info(blob, len(blob), None) == capi.DVO_ERR_INVALID
    assert lib.dvo_archive_blob_info(blob, 0, info) == capi.DVO_ERR_INVALID


def test_defects_are_named():
    from rgbd_odometry_amd import DvoError, capi
    d = defective_blobs()
    for name, word in (("bad magic", "magic"), ("wrong version", "version"), ("overlapping payloads", "overlapping"), ("negative N", "N is negative"),
                       ("pt4_ok = 2", "pt4_ok"), ("wrong table checksum", "table checksum"), ("offset out of range", "out of range"),
                       ("truncated by one byte", "truncated")):
        with pytest.raises(DvoError) as ei:
            capi.archive_blob_info(d[name])
        assert word in str(ei.value), (name, str(ei.value))


def test_symbols_in_header_library_and_binding():
    from rgbd_odometry_amd import capi
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvo_amd.h")).read(), flags=re.S)
    lib = capi.load_library()
    for name in ("dvo_archive_blob_info", "dvo_tracker_archive_export_size", "dvo_tracker_archive_export", "dvo_tracker_archive_import",
                 "dvo_tracker_archive_origin"):
        assert re.search(r"\b%s\s*\(" % name, text) and hasattr(lib, name) and name in capi.C_ABI_SYMBOLS, name
    for macro, value in (("DVO_TRACKER_EXPORT_LAUNCHES", capi.DVO_TRACKER_EXPORT_LAUNCHES), ("DVO_TRACKER_IMPORT_LAUNCHES", capi.DVO_TRACKER_IMPORT_LAUNCHES)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % macro, text).group(1)) == value
    assert hasattr(capi.DvoTracker, "export_archive") and hasattr(capi.DvoTracker, "import_archive") and hasattr(capi.DvoTracker, "archive_origin")
    # the ctypes mirror has the size the C compiler gives the struct
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "s.c")
        open(src, "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "dvo_amd.h"\nint main(){printf("%zu %zu", '
                             'sizeof(struct dvo_archive_blob_info), offsetof(struct dvo_archive_blob_info, total_bytes));return 0;}')
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", os.path.join(d, "s")])
        size, off = (int(x) for x in subprocess.check_output([os.path.join(d, "s")]).split())
    assert (C_sizeof(capi.DvoArchiveBlobInfo), capi.DvoArchiveBlobInfo.total_bytes.offset) == (size, off)


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    d = tmp_path_factory.mktemp("archive_blob")
    exe = str(d / "archive_blob_main")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I", os.path.join(ROOT, "rgbd_odometry_amd", "csrc"), "-o", exe,
                            os.path.join(ROOT, "tests", "host", "archive_blob_main.cpp")], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, "tests/host/archive_blob_main.cpp did not build (it needs g++ with libasan and libubsan):\n" + build.stderr
    return d, exe


def program_verdict(host_program, blob):
    """(info, table lines) or None; any other exit status -- a sanitizer report among them -- fails"""
    d, exe = host_program
    path = str(d / "blob.bin")
    with open(path, "wb") as f:
        f.write(blob)
    run = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    if run.returncode == 3:
        assert run.stdout.startswith("refused: "), run.stdout
        return None
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    head = lines[0].split()
    assert head[0] == "ok"
    keys = ("version", "rows", "cols", "n_levels", "first_shift", "places_level", "D", "n_key_frames", "total_bytes")
    return dict(zip(keys, (int(x) for x in head[1:]))), [[int(x) for x in l.split()[1:]] for l in lines[1:]]


def test_validation_under_sanitizers(host_program):
    """the same code the library compiles, the blob in an allocation of exactly its size: the verdicts of the reference, payload
    checksums included, and nothing read beyond a truncated blob"""
    for name, blob in valid_blobs().items():
        info, records = br.validate(blob)
        got = program_verdict(host_program, blob)
        assert got is not None and got[0] == info, name
        for r, line in zip(records, got[1]):
            assert line == [r["origin_id"], r["origin_stream"], r["origin_frame"], r["has_desc"], r["payload_offset"], r["payload_bytes"],
                            r["payload_checksum"]] + r["N"] + r["pt4_ok"], name
    for name, blob in defective_blobs().items():
        assert program_verdict(host_program, blob) is None, name
    good = valid_blobs()["two key frames"]
    for at in (br.validate(good)[1][0]["payload_offset"], len(good) - 1):          # first and last payload byte
        flipped = bytearray(good)
        flipped[at] ^= 0x80
        assert program_verdict(host_program, bytes(flipped)) is None, at
    assert program_verdict(host_program, b"") is None


def test_golden_fixture_pins_version_1():
    """tests/golden/archive_blob_v1.bin is what make_archive_blob_golden.py writes today, and library and reference parse it to the
    fields recorded above: an accidental change of the layout shows here"""
    blob = open(GOLDEN, "rb").read()
    kfs, geo = br.synthetic_key_frames()
    assert blob == br.build(kfs, **geo)
    assert library_verdict(blob) == GOLDEN_INFO and reference_verdict(blob, payloads=True) == GOLDEN_INFO
    records = br.validate(blob)[1]
    for want, r in zip(GOLDEN_TABLE, records):
        assert {k: (r[k][:3] if k in ("N", "pt4_ok") else r[k]) for k in want} == want
    assert [r["N"][1] for r in records] == [65, 0] and records[0]["N"][0] % 64 != 0     # a ragged last chunk, an empty level
    assert struct.unpack_from("<Q", blob, 72)[0] == br.checksum(blob[80:80 + 2 * 144])
