"""The sample enumeration of k_descriptor (vulkansift_amd/csrc/hip/features.hip) restated in Python: the analytic row spans of a keypoint's
window (desc_row_spans), the exclusive scan of their pair slots (desc_row_prefix), the run of a wave and a lane (desc_run) and the walk along it
(desc_next_slot). A slot is two row neighbours (dx, dx + 1); a span of cnt samples is (cnt + 1) // 2 slots, and the second half of the last slot
of an odd span is dead. Used by tests/test_descriptor_slots.py (the enumeration itself, CPU) and tests/test_gpu_descriptor_slots.py (which
cases reach which slot counts).

The spans are float32 arithmetic in the kernel's order; the kernel takes 1 / kcos and 1 / -ksin from v_rcp_f32 (1 ulp) and cos / sin from its own
routine, so a span may differ from the kernel's by a texel where a bound falls within an ulp of an integer + 0.01 — a model of which windows have
which shape, not a bit-exact restatement (the bytes are checked against the oracle, which enumerates the whole window)."""
import math

import numpy as np

f32 = np.float32
MAX_ROWS = 256       # features.hip DESC_MAX_ROWS: window rows per pass


def window(sx, sy, rel_sigma, w, h):
    """R and the window [dx0, dx1] x [dy0, dy1] clipped to the image interior, relative to the rounded position (desc_radius, desc_setup)"""
    lam = f32(f32(3.0) * f32(rel_sigma))
    radius = f32(f32(f32(f32(np.sqrt(f32(2.0))) * lam) * f32(5)) * f32(0.5))
    R = int(np.floor(f32(radius + f32(0.5))))
    rsx, rsy = np.floor(f32(f32(sx) + f32(0.5))), np.floor(f32(f32(sy) + f32(0.5)))  # roundf of a positive value
    cx, cy = int(rsx), int(rsy)
    return R, lam, (max(-R, 1 - cx), min(R, w - 2 - cx), max(-R, 1 - cy), min(R, h - 2 - cy)), (f32(rsx - f32(sx)), f32(rsy - f32(sy)))


def row_spans(sx, sy, rel_sigma, theta, w, h):
    """[(lo, cnt)] of every window row dy0 .. dy1 (desc_row_spans); [] for an empty window"""
    R, lam, (dx0, dx1, dy0, dy1), (offx, offy) = window(sx, sy, rel_sigma, w, h)
    kcos, ksin = f32(f32(math.cos(float(f32(theta)))) / lam), f32(f32(math.sin(float(f32(theta)))) / lam)
    T = f32(f32(2.5) + f32(0.01))
    out = []
    for dy in range(dy0, dy1 + 1):
        fy = f32(f32(dy) + offy)
        lo, hi = f32(f32(dx0) - f32(0.5)), f32(f32(dx1) + f32(0.5))
        for aa, bb in ((kcos, f32(ksin * fy)), (f32(-ksin), f32(kcos * fy))):
            if abs(aa) > f32(1e-12):
                ia = f32(f32(1.0) / aa)
                ctr, half = f32(f32(f32(-bb) * ia) - offx), f32(T * abs(ia))
                lo, hi = max(lo, f32(ctr - half)), min(hi, f32(ctr + half))
            elif not abs(bb) < T:
                hi = f32(lo - f32(2.0))
        ilo, ihi = int(np.ceil(f32(lo - f32(0.01)))), int(np.floor(f32(hi + f32(0.01))))
        xl, xh = max(ilo, dx0), min(ihi, dx1)
        out.append((xl, xh - xl + 1 if xh >= xl else 0))
    return out


def passes(spans, max_rows=MAX_ROWS):
    """the spans of a window in the passes the kernel takes them in: [(first row, spans of the pass)]"""
    return [(r0, spans[r0:r0 + max_rows]) for r0 in range(0, len(spans), max_rows)]


def slot_prefix(spans):
    """desc_row_prefix: pre[row] = slots in front of the row, pre[nrows] = P"""
    pre = [0]
    for _, cnt in spans:
        pre.append(pre[-1] + ((cnt + 1) >> 1))
    return pre


def slots(spans):
    return slot_prefix(spans)[-1]


def search_row(pre, nrows, sidx):
    """desc_run's bisection: the largest row of 0 .. nrows - 1 with pre[row] <= sidx, then past empty rows (reads counted for the caller)"""
    lo_r, hi_r = 0, nrows - 1
    while lo_r < hi_r:
        mid = (lo_r + hi_r + 1) >> 1
        if pre[mid] <= sidx:
            lo_r = mid
        else:
            hi_r = mid - 1
    row = lo_r
    while pre[row + 1] <= sidx:
        row += 1
    return row


def run(spans, pre, nwv, wave, lane):
    """desc_run + the sample loop of one lane of share `wave` of nwv: -> (steps, [(row, dx, live0, live1)] of its `steps` slots).
    Every LDS index the kernel forms is asserted to lie inside the pass's arrays."""
    nrows = len(spans)
    P = pre[nrows]
    T = (P + 63) // 64
    tq, tr = T // nwv, T % nwv
    steps = tq + (1 if wave < tr else 0)
    step0 = wave * tq + min(wave, tr)
    sidx = min(P, step0 * 64 + lane * steps)
    send = min(P, sidx + steps)
    row = search_row(pre, nrows, sidx) if sidx < send else 0
    assert 0 <= row < nrows
    lo, cnt = spans[row]
    cdx, xend = lo + 2 * (sidx - pre[row]), lo + cnt
    out = []
    for _ in range(steps):
        live0 = sidx < send
        if live0 and cdx >= xend:
            while True:
                row += 1
                assert row < nrows, "the row advance walked off the pass"
                if spans[row][1]:
                    break
            cdx = spans[row][0]
            xend = cdx + spans[row][1]
        out.append((row, cdx, live0, live0 and cdx + 1 < xend))
        cdx += 2
        sidx += 1
    return steps, out


def enumerate_pass(spans, nwv):
    """every slot of every lane of the nwv shares of one pass: -> (live samples [(row, dx)], dead halves of live slots [(row, dx)], steps per share)"""
    pre = slot_prefix(spans)
    live, dead, steps = [], [], []
    for wave in range(nwv):
        st = None
        for lane in range(64):
            st, sl = run(spans, pre, nwv, wave, lane)
            for row, dx, l0, l1 in sl:
                if l0:
                    live.append((row, dx))
                    (live if l1 else dead).append((row, dx + 1))
                else:
                    assert not l1
        steps.append(st)
    return live, dead, steps
