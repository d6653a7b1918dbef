"""tests/np_rootsift.py — the specification of the RootSIFT conversion — against independent statements over its WHOLE domain, the 8 323 455 pairs
(d, s) with 0 <= d <= 255 and max(d, 1) <= s <= 32640: big-integer arithmetic (math.isqrt) and the defining inequalities, a float64 computation
wherever that is safe, the stated properties, and the fp32 shortcut, which is NOT the specification: the fact that motivates the integer
correction step of the kernel stays pinned here. CPU only."""
import math

import numpy as np
import pytest

import np_rootsift as RS

N_PAIRS = 8323455


@pytest.fixture(scope="module")
def domain():
    """(d, s, r): every pair of the domain, d-major, and the restatement's unsaturated r"""
    d = np.concatenate([np.full(RS.S_MAX - max(k, 1) + 1, k, np.int64) for k in range(256)])
    s = np.concatenate([np.arange(max(k, 1), RS.S_MAX + 1, dtype=np.int64) for k in range(256)])
    assert len(d) == len(s) == N_PAIRS
    return d, s, RS.root_bins(d, s)


def test_against_big_integers_over_the_whole_domain(domain):
    """512 sqrt(d / s) + 1/2 = (sqrt(2^20 d s) + s) / (2 s), and the floor of a quotient by an integer takes the floor of the numerator first"""
    d, s, r = domain
    isqrt = math.isqrt
    want = [(isqrt((k * t) << 20) + t) // (2 * t) for k in range(256) for t in range(max(k, 1), RS.S_MAX + 1)]
    assert np.array_equal(r, np.array(want, np.int64))
    # the definition itself, in int64 (an arbitrary r against an arbitrary s reaches 1025^2 * 32640, beyond 32 bits)
    n = d << 20
    assert ((2 * r + 1) ** 2 * s > n).all() and ((2 * r - 1) ** 2 * s <= n)[d > 0].all() and (r[d == 0] == 0).all()
    assert 1025 ** 2 * RS.S_MAX > 1 << 32
    # ... but the products a correction step forms from an estimate within 1 of r stay below 2^32: (2r - 1)^2 s <= 2^20 d < 2^28 and r >= 3 for
    # d >= 1, so (2 (r + 1) + 1)^2 s <= (9 / 5)^2 2^28. The kernel's 32-bit arithmetic rests on this
    assert r[d > 0].min() == 3 and int(((2 * (r + 1) + 1) ** 2 * s).max()) < 1 << 32


def test_against_float64_away_from_the_ties(domain):
    d, s, r = domain
    x = 512.0 * np.sqrt(d.astype(np.float64) / s.astype(np.float64))
    safe = np.abs(x - np.floor(x) - 0.5) > 1e-6
    assert safe.mean() > 0.999
    assert np.array_equal(np.floor(x[safe] + 0.5).astype(np.int64), r[safe])


def test_properties(domain):
    d, s, r = domain
    assert ((r == 0) == (d == 0)).all()                       # a non-zero bin stays non-zero
    assert r.max() == 512 and (r[d == s] == 512).all()        # a single bin: 512, saturated to 255 in a row
    # d = 255: 512 sqrt(255 / s) is 255.25 at s = 1026, 255.4995 at s = 1024 and 255.62 at s = 1023, where r = 256 is first cut to 255
    sat = s[(d == 255) & (r > 255)]
    assert r[(d == 255) & (s == 1026)][0] == 255 and r[(d == 255) & (s == 1024)][0] == 255 and sat.max() == 1023
    rows = np.zeros((6, 128), np.uint8)
    rows[1, 7] = 1
    rows[2, 100] = 255
    rows[3] = 255
    rows[4, :4] = 255, 255, 255, 255 - 1          # s = 1019
    rows[5] = 2
    out = RS.root_rows(rows)
    assert not out[0].any()                                   # s == 0
    assert out[1, 7] == 255 and out[1].sum() == 255 and out[2, 100] == 255 and out[2].sum() == 255
    assert (out[3] == 45).all() and (out[5] == 45).all()      # 512 / sqrt(128) = 45.25: the scale of the row does not matter
    assert out[4, 0] == 255 and out[4, 3] == 255 and not out[4, 4:].any()
    assert ((out == 0) == (rows == 0)).all()


def test_only_the_descriptor_bytes_of_a_record_change():
    rng = np.random.default_rng(3)
    recs = rng.integers(0, 256, (50, RS.REC), dtype=np.uint8)
    out = RS.convert_records(recs)
    assert np.array_equal(out[:, :RS.DESC_AT], recs[:, :RS.DESC_AT]) and np.array_equal(out[:, RS.DESC_AT:], RS.root_rows(recs[:, RS.DESC_AT:]))
    assert (out[:, RS.DESC_AT:] != recs[:, RS.DESC_AT:]).any()
    buf = rng.integers(0, 256, (20, RS.REC), dtype=np.uint8)
    rows = np.array([3, 4, 9, 17])
    after = RS.convert_buffer(buf, rows)
    rest = np.setdiff1d(np.arange(20), rows)
    assert np.array_equal(after[rest], buf[rest]) and np.array_equal(after[rows], RS.convert_records(buf[rows]))
    # norms: a converted row has the norm of a SIFT row, about 512 (sum of r^2 ~ 2^18 sum(d) / s)
    norms = np.sqrt((RS.root_rows(rng.integers(0, 60, (200, 128), dtype=np.uint8)).astype(np.int64) ** 2).sum(1))
    assert (np.abs(norms - 512.0) < 4.0).all()


def test_the_fp32_shortcut_is_not_the_specification(domain):
    """floor(512 sqrtf((float)d / (float)s) + 0.5f) with every operation correctly rounded (numpy's float32) is wrong somewhere on the domain:
    an implementation needs the integer correction step"""
    d, s, r = domain
    f = np.float32
    x = np.floor(f(512.0) * np.sqrt(d.astype(f) / s.astype(f)) + f(0.5))
    assert x.dtype == f
    bad = np.flatnonzero(x.astype(np.int64) != r)
    print("fp32 shortcut differs for", len(bad), "pairs; the first (d, s):", [(int(d[i]), int(s[i])) for i in bad[:5]])
    assert 0 < len(bad) < 1000
    assert (np.abs(x[bad].astype(np.int64) - r[bad]) == 1).all()    # by one: a single correction step against the inequalities repairs it
