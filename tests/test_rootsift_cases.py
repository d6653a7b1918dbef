"""The case table of tests/hip_rootsift.py without a GPU: it reaches the edges it is there for, the large case holds every reachable (d, s) pair
and would fail the fp32 shortcut, and the arenas state the contract — what is expected differs from what goes in only inside the descriptor
bytes of stored records of named buffers and inside their cache entries. CPU only."""
import numpy as np
import pytest

import hip_rootsift as HT
import np_rootsift as RS
from test_section_walk import stored_rows


def test_all_pairs_rows_cover_the_reachable_domain_and_fail_the_fp32_shortcut():
    rows = HT.all_pairs_rows()       # (asserts its own coverage)
    reach = HT.reachable_pairs()
    assert rows.dtype == np.uint8 and rows.shape[1] == 128 and 300000 < len(rows) < 420000
    assert int(reach.sum()) == 256 * (HT.REST_MAX + 1) - 1      # every d with every rest 0 .. 127 * 255, less (0, 0)
    f = np.float32
    s = rows.sum(1, dtype=np.int64)[:, None].astype(f)
    shortcut = np.minimum(np.floor(f(512.0) * np.sqrt(rows.astype(f) / s) + f(0.5)), 255).astype(np.uint8)
    assert (shortcut != RS.root_rows(rows)).any()
    c = HT.all_pairs_case()
    assert c["totals"] == [len(rows)] and c["rows"] == "all pairs"


def test_case_table_reaches_its_edges():
    cs = HT.CASES
    single = {(c["totals"][0], c["max_rows"]) for c in cs if c["table"][0] == 1 and len(c["buf_ids"]) == 1 and c["rows"] == "random"}
    w, b, g = HT.ROWS_PER_WAVE, HT.ROWS_PER_BLOCK, HT.MAX_BLOCKS * HT.ROWS_PER_BLOCK
    assert single >= {(t, "exact") for t in (0, 1, 2, w - 1, w, w + 1, b - 1, b, b + 1, g - 1, g, g + 1)}
    assert single >= {(t, 0) for t in (b - 1, b, b + 1)} | {(t, 2 * b) for t in (2 * b - 1, 2 * b, 2 * b + 1)}
    assert {c["max_rows"] for c in cs} >= {0, 4000000000}
    assert any(c["table"][0] == 16 for c in cs) and any(c["fixed"] and c["table"][0] == 1 for c in cs) and any(c["fixed"] and c["table"][0] == 3 for c in cs)
    assert {(c["totals"][0], c["pad"]) for c in cs if c["cache"] and len(c["buf_ids"]) == 1} >= {(0, 0), (1, 0), (0, 2), (1, 2)}
    assert any(c["desc_extra"] and c["norm_extra"] and c["n_stride"] > 1 for c in cs)
    three = HT.case_named("three slots {5, 0, 3} of 8")
    assert three["buf_ids"] == [5, 0, 3] and all(t > 0 for t in three["totals"])
    big = HT.case_named("512 slots")
    assert len(big["buf_ids"]) == 512 and max(big["totals"]) > HT.MIN_BLOCKS * HT.ROWS_PER_BLOCK
    shapes = HT.shape_rows()
    sums = shapes.sum(1, dtype=np.int64)
    assert (sums == 0).any() and ((sums == 1) & (shapes.max(1) == 1)).any() and ((sums == 255) & (shapes.max(1) == 255)).any() and (shapes.min(1) == 255).any()
    assert set(range(1021, 1035)) <= {int(v) for v in sums[shapes.max(1) == 255]}
    out = RS.root_rows(shapes)
    assert set(np.unique(out[(shapes == 255) & (sums[:, None] > 1000) & (sums[:, None] < 1040)])) == {254, 255}


@pytest.mark.parametrize("case", [c for c in HT.CASES if max(c["totals"]) <= 400 and c["nbuf"] <= 8], ids=lambda c: c["name"])
def test_arena_states_the_contract(case):
    h = HT.Root(case, device="cpu")
    exp, host = h.expected(), h.host
    allowed = np.zeros(len(host), bool)
    nsec, off, cap, _ = case["table"]
    for b in case["buf_ids"]:
        for r in stored_rows(nsec, off, cap, case["counts"][b]):
            lo = h.feats.off + b * h.buf_stride + int(r) * HT.REC
            allowed[lo + RS.DESC_AT:lo + HT.REC] = True
        if case["cache"]:
            rows = max(case["totals"][b], case["pad"])
            allowed[h.desc.off + b * h.desc_stride:][:rows * 128] = True
            allowed[h.norms.off + b * h.norm_stride * 4:][:rows * 4] = True
            allowed[h.n.off + b * case["n_stride"] * 4:][:4] = True
    assert not (exp != host)[~allowed].any()
    if any(case["totals"][b] for b in case["buf_ids"]):
        assert (exp != host).any()
