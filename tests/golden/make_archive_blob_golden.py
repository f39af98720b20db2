"""Writes tests/golden/archive_blob_v1.bin: two synthetic key frames in the key-frame archive blob's format version 1, built by the
numpy reference (tests/archive_blob_reference.py).  Run from the repository root: python tests/golden/make_archive_blob_golden.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import archive_blob_reference as br  # noqa: E402

if __name__ == "__main__":
    kfs, geo = br.synthetic_key_frames()
    blob = br.build(kfs, **geo)
    info, records = br.validate(blob)
    with open(os.path.join(HERE, "archive_blob_v1.bin"), "wb") as f:
        f.write(blob)
    print(info)
    for r in records:
        print({k: r[k] for k in ("origin_id", "origin_stream", "origin_frame", "has_desc", "payload_offset", "payload_bytes", "N", "pt4_ok")})
