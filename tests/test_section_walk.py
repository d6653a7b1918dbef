"""The walk from a download-order row of a SIFT buffer to its stored row (vulkansift_amd/csrc/hip/records.h: section_counts and
section_row, used by k_gather_sections, k_pack_features, k_gather_corr and k_gather_xy). The header is compiled into a host program
(tests/native/section_probe.cpp) and compared, for every row of every table, with the numpy statement: the stored rows of a buffer in
download order are concatenate(arange(off[o], off[o] + min(found[o], cap[o]))) over its sections. (The kernels themselves are compared
with the numpy restatements of tests/np_records.py, which import stored_rows and TABLES from here, by tests/test_gpu_record_launchers.py.)"""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SECTIONS = 16


def _table(nsec, cap, found, off=None, beyond=(7, 9, 11)):
    """16-entry arrays: the given sections, then entries that a walk of nsec sections must not look at (non-zero on purpose)"""
    cap, found = list(cap), list(found)
    assert len(cap) == len(found) == nsec
    off = list(off) if off is not None else [int(s) for s in np.cumsum([0] + cap[:-1])]   # sections back to back, as the detector lays them out
    pad = MAX_SECTIONS - nsec
    return nsec, off + [beyond[0]] * pad, cap + [beyond[1]] * pad, found + [beyond[2]] * pad


TABLES = {
    "one section": _table(1, [40], [17]),
    "one section, found > cap": _table(1, [40], [1000]),
    "one section, found == cap": _table(1, [40], [40]),
    "three sections": _table(3, [50, 20, 8], [31, 20, 3]),
    "three, found > cap in the middle": _table(3, [50, 20, 8], [31, 77, 3]),
    "three, an empty section between two others": _table(3, [50, 20, 8], [31, 0, 5]),
    "three, first empty, last found == cap": _table(3, [50, 20, 8], [0, 2, 8]),
    "three, gaps between the sections": _table(3, [5, 6, 7], [5, 9, 1], off=[100, 3, 40]),
    "sixteen sections": _table(16, [300 >> (o // 2) for o in range(16)], [(37 * (o + 1)) % 160 for o in range(16)]),
    "sixteen, every one clamped": _table(16, list(range(1, 17)), [99] * 16),
    "sixteen, only the last holds rows": _table(16, [4] * 16, [0] * 15 + [3]),
    "one section, empty": _table(1, [40], [0]),
    "three sections, all empty": _table(3, [50, 20, 8], [0, 0, 0]),
    "sixteen sections, all empty": _table(16, [4] * 16, [0] * 16),
    "a capacity of zero": _table(3, [0, 6, 0], [5, 5, 5]),
}


def stored_rows(nsec, off, cap, found):
    return np.concatenate([np.arange(off[o], off[o] + min(found[o], cap[o]), dtype=np.int64) for o in range(nsec)] + [np.zeros(0, np.int64)])


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("walk") / "section_probe")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vulkansift_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "section_probe.cpp"), "-o", exe], check=True)
    names = list(TABLES)
    text = "".join(" ".join(str(v) for v in [TABLES[k][0]] + TABLES[k][1] + TABLES[k][2] + TABLES[k][3]) + "\n" for k in names)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == 2 * len(names) + 1
    out = {k: (lines[2 * i].split(), lines[2 * i + 1].split()) for i, k in enumerate(names)}
    out["constants"] = lines[-1].split()
    return out


@pytest.mark.parametrize("name", list(TABLES))
def test_counts_and_every_row(probe, name):
    nsec, off, cap, found = TABLES[name]
    counts, rows = probe[name]
    want_cnt = [min(found[o], cap[o]) if o < nsec else 0 for o in range(MAX_SECTIONS)]
    want = stored_rows(nsec, off, cap, found)
    assert counts[0] == "C" and rows[0] == "R"
    assert [int(c) for c in counts[2:]] == want_cnt              # min(found, cap) per section, zero beyond nsec
    assert int(counts[1]) == sum(want_cnt) == len(want)           # the total
    assert np.array_equal(np.array(rows[1:], dtype=np.int64), want)   # every row of [0, total); none when the total is 0


def test_tables_cover_the_cases():
    """the cases the walk can go wrong at are all present in TABLES"""
    ts = list(TABLES.values())
    assert {t[0] for t in ts} == {1, 3, 16}
    assert any(t[3][o] > t[2][o] for t in ts for o in range(t[0]))
    assert any(t[3][o] == t[2][o] > 0 for t in ts for o in range(t[0]))
    assert any(t[0] >= 3 and t[3][o] == 0 and min(t[3][o - 1], t[2][o - 1]) > 0 and min(t[3][o + 1], t[2][o + 1]) > 0 for t in ts for o in range(1, t[0] - 1))
    assert sum(1 for t in ts if len(stored_rows(*t)) == 0) >= 3


def test_constants(probe):
    """a record is 164 bytes = 41 words with the descriptor at byte 36 (vksift_Feature); a section table is {nsec, off[16], cap[16]}"""
    assert [int(v) for v in probe["constants"][1:]] == [164, 41, 36, 33, 17]
