"""The walk over a list of SIFT buffers in runs of one section layout (csrc/host/vksift_runs.c), on the CPU: the translation unit makes no
device call, so it is compiled alone with a small program that prints the runs of hand-built buffer tables (tests/native/layout_runs.c), with
gcc's address and undefined-behaviour sanitizers where their runtimes exist. The expected runs are written down here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vulkansift_amd", "csrc", "host")
FOUND_STRIDE = 16   # VKSIFT_MAX_OCTAVES: the counters of a detected buffer


def sectioned(first, n, nsec, cap, max_rows, last_cap=None):
    caps = [cap] * (nsec - 1) + [cap if last_cap is None else last_cap]
    return dict(first=first, n=n, nsec=nsec, off=[o * cap for o in range(nsec)], cap=caps, fixed=None, stride=FOUND_STRIDE, max_rows=max_rows)


def dense(first, n, stored, max_rows):
    """an uploaded buffer: one section {off 0, cap stored} with a fixed count, no counters on the device"""
    return dict(first=first, n=n, nsec=1, off=[0], cap=[stored], fixed=[stored], stride=0, max_rows=max_rows)


EXPECTED = {
    "one dense buffer": [dense(0, 1, 40, 0)],
    "two dense buffers, equal": [dense(0, 2, 40, 0)],
    "two dense buffers, different": [dense(0, 1, 40, 0), dense(1, 1, 41, 0)],
    # bounds 10 + (37 i mod 200) for ids 4 .. 511, zero for the last four: every residue occurs
    "512 ids, one layout": [sectioned(4, 512, 3, 100, 209)],
    # ids 9, 3 | 200, 201 | 7 with bounds 5, 300 | 11, 12 | 299: the largest of the run, not of the list
    "A B A": [sectioned(9, 2, 3, 100, 300), sectioned(200, 2, 4, 50, 12), sectioned(7, 1, 3, 100, 299)],
    "A B A, no bounds": [sectioned(9, 2, 3, 100, 0), sectioned(200, 2, 4, 50, 0), sectioned(7, 1, 3, 100, 0)],
    "dense between sectioned": [sectioned(10, 1, 3, 100, 1), dense(300, 1, 1000, 1000), sectioned(11, 2, 3, 100, 3)],
    "sixteen sections": [sectioned(400, 2, 16, 8, 47)],
    "the last capacity differs": [sectioned(410, 1, 5, 20, 0), sectioned(411, 1, 5, 20, 0, last_cap=19)],
    "a list of one": [sectioned(17, 1, 3, 100, 39)],
    "an empty list": [],
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("runs") / "layout_runs")
    san = []
    runtimes = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if all(os.path.isabs(p) and os.path.exists(p) for p in runtimes):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    srcs = [os.path.join(ROOT, "tests", "native", "layout_runs.c"), os.path.join(HOST, "vksift_runs.c")]
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Werror"] + san + ["-I" + os.path.join(ROOT, "include"), "-I" + HOST] + srcs + ["-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "BAD" not in r.stdout, r.stdout
    out, name = {}, None
    for line in r.stdout.splitlines():
        kind, _, rest = line.partition(" ")
        if kind == "case":
            name = rest
            out[name] = []
        else:
            assert kind == "run", line
            f = dict(kv.split("=") for kv in rest.split())
            words = lambda v: None if v == "-" else [int(w) for w in v.split(",") if w]
            out[name].append(dict(first=int(f["first"]), n=int(f["n"]), nsec=int(f["nsec"]), off=words(f["off"]), cap=words(f["cap"]), fixed=words(f["fixed"]),
                                  stride=int(f["stride"]), max_rows=int(f["max_rows"])))
    return out


def test_every_case_is_walked(runs):
    assert list(runs) == list(EXPECTED)


@pytest.mark.parametrize("name", list(EXPECTED))
def test_runs(runs, name):
    assert runs[name] == EXPECTED[name]
