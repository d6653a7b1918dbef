"""The arithmetic of the single-pair matcher's stream decomposition (vulkansift_amd/csrc/match_stream.h: stream_span, the piece walk
stream_next of k_match_mfma and k_match_scan32, the piece count stream_pieces of k_match_merge and k_match_fix), restated in Python and
checked over many shapes: every (row block, B tile) pair is visited exactly once, the pieces of a row block are numbered 0..n-1
without gaps in increasing tile order, and no row block needs more partial lists than VKSIFT_HIP_MATCH_CHUNKS. The header itself is
compiled into a host program and compared with the restatement on the same shapes, so the arithmetic checked here is the arithmetic
the kernels execute. (The kernels themselves are compared with the oracle by the -m gpu tests.)"""
import re
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _chunks():
    hdr = open(os.path.join(ROOT, "include", "vksift_hip.h")).read()
    return int(re.search(r"#define VKSIFT_HIP_MATCH_CHUNKS (\d+)", hdr).group(1))


CHUNKS = _chunks()


def stream_span(nblocks, tiles, G):
    even = (nblocks * tiles + G - 1) // G
    floor_ = (tiles + CHUNKS - 3) // (CHUNKS - 2)
    return max(even, floor_, 1)


def pieces(na, nb, G, block_rows=256, tile_rows=128):
    """what each workgroup of the grid does: (workgroup, row block, first tile, tile count, partial-list slot)"""
    nblocks, tiles = (na + block_rows - 1) // block_rows, (nb + tile_rows - 1) // tile_rows
    span = stream_span(nblocks, tiles, G)
    out = []
    for w in range(G):
        pos, end = w * span, min((w + 1) * span, nblocks * tiles)
        while pos < end:
            rb = pos // tiles
            t_first = pos - rb * tiles
            t_cnt = min(tiles - t_first, end - pos)
            out.append((w, rb, t_first, t_cnt, w - (rb * tiles) // span))
            pos += t_cnt
    return out, nblocks, tiles, span


def merge_count(rb, tiles, span):
    return ((rb + 1) * tiles - 1) // span - (rb * tiles) // span + 1


SHAPES = [(1, 2), (300, 33000), (1537, 2), (1537, 4097), (4000, 4000), (9000, 700), (33000, 5000), (50000, 50000),
          (70001, 130), (100000, 100000), (257, 128), (256, 129), (1000000, 300)]


@pytest.mark.parametrize("na,nb", SHAPES)
@pytest.mark.parametrize("G", [512, 608, 64])
def test_every_tile_once_and_slots_dense(na, nb, G):
    ps, nblocks, tiles, span = pieces(na, nb, G)
    seen = np.zeros((nblocks, tiles), np.int32)
    slots = {}
    for w, rb, t0, cnt, slot in ps:
        seen[rb, t0:t0 + cnt] += 1
        slots.setdefault(rb, []).append((t0, slot))
    assert (seen == 1).all()
    for rb, lst in slots.items():
        lst.sort()
        assert [s for _, s in lst] == list(range(len(lst))), (rb, lst)          # slot order == tile order: ties keep arrival order
        assert len(lst) == merge_count(rb, tiles, span) <= CHUNKS, (rb, len(lst))
        assert lst[0][0] == 0                                                    # slot 0 holds tile 0 (the Q7 swap flag lives there)
    assert set(slots) == set(range(nblocks))


def test_random_shapes():
    rng = np.random.default_rng(5)
    for _ in range(300):
        na, nb, G = int(rng.integers(1, 200000)), int(rng.integers(2, 200000)), int(rng.choice([64, 128, 512, 608]))
        nblocks, tiles = (na + 255) // 256, (nb + 127) // 128
        span = stream_span(nblocks, tiles, G)
        assert span * G >= nblocks * tiles                                       # the grid covers the list
        worst = max(merge_count(rb, tiles, span) for rb in {0, nblocks // 2, nblocks - 1})
        assert worst <= CHUNKS


def test_header_agrees_with_the_restatement(tmp_path):
    """csrc/match_stream.h, compiled with the host C++ compiler: stream_span, the full piece list of stream_next and stream_pieces of
    every row block equal the Python restatement, for the parametrised shapes (every grid) and the 300 random shapes"""
    exe = str(tmp_path / "stream_probe")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "vulkansift_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "stream_probe.cpp"), "-o", exe], check=True)
    shapes = [(na, nb, G) for G in (512, 608, 64) for na, nb in SHAPES]
    rng = np.random.default_rng(5)
    shapes += [(int(rng.integers(1, 200000)), int(rng.integers(2, 200000)), int(rng.choice([64, 128, 512, 608]))) for _ in range(300)]
    r = subprocess.run([exe], input="".join("%d %d %d 256 128\n" % s for s in shapes), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = iter(r.stdout.splitlines())
    for na, nb, G in shapes:
        ps, nblocks, tiles, span = pieces(na, nb, G)
        assert next(lines).split() == ["S", str(span), str(nblocks), str(tiles)], (na, nb, G)
        for piece in ps:
            assert next(lines) == "P %d %d %d %d %d" % piece, (na, nb, G, piece)
        counts = next(lines).split()
        assert counts[0] == "M" and [int(c) for c in counts[1:]] == [merge_count(rb, tiles, span) for rb in range(nblocks)], (na, nb, G)
    assert next(lines, None) is None
