"""The engine's environment variables are exactly the ones INTEGRATION.md section 6 documents (CPU only): every DVO_* name the
library reads through getenv appears in the first column of that table, and the table lists no name the library does not read."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names_read_by_the_library():
    names = set()
    for p in glob.glob(os.path.join(ROOT, "rgbd_odometry_amd", "csrc", "*")):
        if p.endswith((".cpp", ".hip", ".h")):
            names |= set(re.findall(r'getenv\(\s*"(DVO_[A-Z0-9_]+)"', open(p).read()))
    return names


def _names_in_integration_section_6():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = re.search(r"^## 6\..*?(?=^## )", text, re.S | re.M)
    assert section, "INTEGRATION.md has no section 6"
    names = set()
    for line in section.group(0).splitlines():
        if line.startswith("| `"):
            names |= set(re.findall(r"DVO_[A-Z0-9_]+", line.split("|")[1]))
    return names


def test_getenv_names_are_the_integration_table():
    read, documented = _names_read_by_the_library(), _names_in_integration_section_6()
    assert read, "no getenv(\"DVO_...\") found in rgbd_odometry_amd/csrc"
    assert read == documented, ("read but not in INTEGRATION.md section 6: %s; in the table but never read: %s"
                                % (sorted(read - documented), sorted(documented - read)))
