"""Get2NearestNeighbors.comp (sift_matcher.c:246-279) restated in vectorised numpy, the reference of tests/test_gpu_match_launchers.py
(tests/test_np_match.py pins it against the loop of np_restatement.match_2nn, the C oracle and tests/golden/matches_a_b.npy):

  * d2 = sum (a - b)^2 exactly: |a|^2 + |b|^2 - 2 a.b as a float64 matmul (every product is below 2^16, every sum of 128 of them below
    2^23: exact), then the shader's float: dist = sqrt(float32(d2)) in float32 (correctly rounded, like the GPU's)
  * the shader initialises from b[0], b[1] unconditionally and scans b[2..] in index order with strict '<': best and second are the
    first two columns in (dist, index) order — two argmin passes, numpy's argmin returning the first of equals —
  * except that d[0] == d[1] makes column 1 the earlier of the two (quirk Q7): for those rows the labels 0 and 1 are exchanged
  * quirk Q6, fewer than two reference rows: the caller pads B with zero rows (pad_two)

Records are five uint32 words {idx_a, idx_b1, idx_b2, dist1 bits, dist2 bits}, as the kernels store them."""
import numpy as np

f32 = np.float32
u32 = np.uint32
ROWS_PER_STEP = 256   # query rows per matmul: 256 x 32 768 doubles = 64 MiB


def distances(a, b):
    """(len(a), len(b)) float32 distances of uint8 rows, as the shader computes them"""
    a, b = a.astype(np.float64), b.astype(np.float64)
    d2 = (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2.0 * (a @ b.T)
    return np.sqrt(d2.astype(f32))


def match_2nn(a, b, a_index_base=0):
    """(len(a), 5) uint32 records of a against b (len(b) >= 2)"""
    a, b = np.asarray(a, np.uint8).reshape(-1, 128), np.asarray(b, np.uint8).reshape(-1, 128)
    assert len(b) >= 2
    out = np.empty((len(a), 5), u32)
    out[:, 0] = (np.arange(len(a), dtype=np.uint64) + np.uint64(a_index_base)).astype(u32)   # modulo 2^32, like the kernel's addition
    for r0 in range(0, len(a), ROWS_PER_STEP):
        d = distances(a[r0:r0 + ROWS_PER_STEP], b)
        rows = np.arange(len(d))
        q7 = d[:, 0] == d[:, 1]
        best = d.argmin(1)
        d1 = d[rows, best]
        d[rows, best] = np.inf
        second = d.argmin(1)
        d2 = d[rows, second]
        for idx in (best, second):
            idx[q7 & (idx < 2)] ^= 1
        out[r0:r0 + len(d), 1], out[r0:r0 + len(d), 2] = best, second
        out[r0:r0 + len(d), 3], out[r0:r0 + len(d), 4] = d1.view(u32), d2.view(u32)
    return out


def pad_two(b):
    """quirk Q6: the rows of a reference set of fewer than two rows, zero rows up to two"""
    b = np.asarray(b, np.uint8).reshape(-1, 128)
    return b if len(b) >= 2 else np.vstack([b, np.zeros((2 - len(b), 128), np.uint8)])


def shifted_norms(desc):
    """sum over the 128 bytes of (byte - 128)^2, uint32 (vksift_hip_shifted_norms)"""
    d = np.asarray(desc, np.uint8).reshape(-1, 128).astype(np.int64) - 128
    return (d * d).sum(1).astype(u32)


def expected_async(case):
    """vksift_hip_match_2nn_async on a case of tests/match_cases.py (case["rows"][e]: the rows of cache entry e, case["ids_a"], case["ids_b"]):
    per slot (N_A, N_B, records) — the count words are the entries' own counts, the records those of A against B padded to two rows;
    no records when max_na is 0. Slots that name the same pair share one computation."""
    memo, out = {}, []
    for ea, eb in zip(case["ids_a"], case["ids_b"]):
        a, b = case["rows"][ea], case["rows"][eb]
        if (ea, eb) not in memo:
            memo[ea, eb] = match_2nn(a, pad_two(b)) if case["max_na"] else np.empty((0, 5), u32)
        out.append((len(a), len(b), memo[ea, eb]))
    return out
