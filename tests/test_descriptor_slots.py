"""The pair-slot enumeration of k_descriptor (features.hip desc_row_prefix / desc_run / desc_next_slot), restated in tests/desc_slots.py,
checked on the CPU: over the NW * NPH shares of a pass every sample of every row span is visited exactly once by a live slot half, no dead half
lies inside a span, the row advance never leaves the pass's arrays, and the shares' steps add up to ceil(P / 64). The kernel itself is checked
byte for byte by tests/test_gpu_descriptor_slots.py; this is the identity it relies on (integer adds commute, so any enumeration that visits
every sample once gives the same histogram)."""
import math
import random

import pytest

import desc_slots as DS

SHARES = (1, 2, 4, 8, 16)  # NW * NPH: team of two = 2, solo wave in 4 phases = 4, four-wave form = 4, and what a re-sweep of the phases may pick


def check(spans, what):
    P = DS.slots(spans)
    assert P == sum((c + 1) // 2 for _, c in spans)
    want = sorted((row, lo + i) for row, (lo, c) in enumerate(spans) for i in range(c))
    inside = set(want)
    for nwv in SHARES:
        live, dead, steps = DS.enumerate_pass(spans, nwv)
        assert sorted(live) == want, (what, nwv)                    # exactly once: a sorted list, not a set
        assert not inside.intersection(dead), (what, nwv)
        assert len(dead) == sum(c & 1 for _, c in spans), (what, nwv)  # one per odd span, none elsewhere
        assert sum(steps) == (P + 63) // 64 and max(steps) - min(steps) <= 1, (what, nwv, steps)
        if P < 64 * nwv:
            assert steps.count(0) >= nwv - max((P + 63) // 64, 0), (what, nwv)  # shares with no step at all


def rows_of(counts, lo=-3):
    return [(lo - (c // 2) + (i % 3), c) for i, c in enumerate(counts)]


def test_short_rows_and_empty_runs():
    check(rows_of([0]), "one empty row")
    check(rows_of([1]), "one sample")
    check(rows_of([2]), "one slot")
    check(rows_of([0, 1, 2, 0, 0, 2, 1, 1, 0]), "lengths 0, 1, 2")
    check(rows_of([0, 0, 0, 5, 7, 0, 0, 0, 0, 9, 4, 0, 0]), "empty rows at the start, in the middle and at the end")
    check(rows_of([0] * 70 + [3] + [0] * 70 + [130] + [0] * 60), "long runs of empty rows around two spans")
    check(rows_of([0] * 256), "a whole pass of empty rows")
    check(rows_of([1] * 256), "a whole pass of one-sample rows")


def test_all_odd_and_all_even_rows():
    check(rows_of([1, 3, 5, 7, 9, 11, 13, 11, 9, 7, 5, 3, 1]), "all odd")
    check(rows_of([2, 4, 6, 8, 10, 12, 10, 8, 6, 4, 2]), "all even")
    check(rows_of([63, 65, 127, 129]), "odd around the wave width")
    check(rows_of([64, 128, 2, 62]), "even around the wave width")


@pytest.mark.parametrize("P", [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 64 * 16 - 1, 64 * 16, 64 * 16 + 1])
def test_slot_totals(P):
    """P slots in one row, in rows of one slot, and in odd rows with gaps; P < NW * NPH gives shares (phases) with no step"""
    check([(-P, 2 * P)], f"P = {P}, one even row")
    if P:
        check([(-P, 2 * P - 1)], f"P = {P}, one odd row")
        check(rows_of([1 + (i & 1) for i in range(P)]), f"P = {P}, one slot per row")  # (a pass has at least one row)
    rng = random.Random(P)
    counts, left = [], P
    while left:
        s = min(left, rng.randint(1, 9))
        counts += [2 * s - rng.randint(0, 1)] + [0] * rng.randint(0, 2)
        left -= s
    assert sum((c + 1) // 2 for c in counts) == P
    check(rows_of([0, 0] + counts), f"P = {P}, mixed rows")


def test_spans_of_the_kernel_expression():
    """windows from desc_row_spans: R 1 .. 34 and 64, the angles of the GPU cases, positions inside and 1.2 texels from the borders"""
    w, h = 64, 64
    rng = random.Random(39)
    seen_one, seen_empty = False, False
    for R in list(range(1, 35)) + [64]:
        rel = R / (math.sqrt(2.0) * 7.5)
        for theta in (0.0, math.pi / 4, math.pi / 2, rng.uniform(0, 2 * math.pi)):
            for x, y in ((32.0, 32.0), (rng.uniform(3, 61), rng.uniform(3, 61)), (1.2, 1.2), (62.8, 30.3), (31.7, 62.8)):
                spans = DS.row_spans(x, y, rel, theta, w, h)
                assert spans, (R, theta, x, y)
                for _, rows in DS.passes(spans):
                    check(rows, f"R {R}, theta {theta:.3f}, at ({x:.1f}, {y:.1f})")
                seen_one |= any(c == 1 for _, c in spans)
                seen_empty |= any(c == 0 for _, c in spans)
    assert seen_one and seen_empty
    # a keypoint on a texel centre at pi / 4: every span is symmetric about dx = 0, so every row is odd
    spans = DS.row_spans(32.0, 32.0, 12 / (math.sqrt(2.0) * 7.5), math.pi / 4, w, h)
    assert all(c & 1 for _, c in spans if c) and sum(1 for _, c in spans if c) > 12


def test_window_taller_than_a_pass():
    spans = DS.row_spans(12.0, 150.0, 140 / (math.sqrt(2.0) * 7.5), 0.3, 24, 300)
    ps = DS.passes(spans)
    assert len(spans) > DS.MAX_ROWS and len(ps) == 2 and all(len(r) <= DS.MAX_ROWS for _, r in ps)
    for r0, rows in ps:
        check(rows, f"pass from row {r0}")
