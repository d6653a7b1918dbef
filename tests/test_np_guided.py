"""The restatement of guided matching (tests/np_guided.py) pinned on the CPU: against a straightforward scalar loop, against the oracle's matcher and
filter under a model that admits everything, the superset property over filtering, what it recovers under repeated structure — and the resource
metadata of the kernels it restates (hipcc cross-compiles)."""
import os
import re
import subprocess

import numpy as np
import pytest

import np_guided as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
ARGS = ("xa", "ya", "desc_a", "xb", "yb", "desc_b")


def _args(s):
    return [s[k] for k in ARGS]


@pytest.mark.parametrize("kind", [G.HOMOGRAPHY, G.FUNDAMENTAL])
@pytest.mark.parametrize("cross_check", [False, True])
def test_vectorised_form_equals_the_scalar_loop(kind, cross_check):
    s = G.slot_case(20, 25, 5, planar=kind == G.HOMOGRAPHY)
    M = s["H"] if kind == G.HOMOGRAPHY else s["F"]
    seen = 0
    for thr in (0.5, 2.5, 1e6):
        for ratio, max_distance in ((0.8, np.inf), (1.01, np.inf), (1.01, 40.0)):
            got = G.guided(kind, M, 1, *_args(s), thr, ratio, max_distance, cross_check)
            want = G.guided_scalar(kind, M, *_args(s), thr, ratio, max_distance, cross_check)
            assert got.tobytes() == want.tobytes(), (thr, ratio, max_distance)
            seen += len(got)
    assert seen > 20                                   # not a comparison of empty lists
    assert len(G.guided(kind, M, 0, *_args(s), 2.5, 0.8, np.inf, cross_check)) == 0


def test_threshold_is_the_square_in_pixels():
    for t in (0.5, 2.5, 3.0, 1e6):
        assert G.threshold2(t) == np.float32(t) * np.float32(t)


ORACLE_SEED = 4242          # the seed of the synthetic descriptors; the share of tied rows it gives is asserted below


def test_everything_admissible_is_the_oracles_filtered_matching(oracle, vk):
    """identity homography, 1e6 px, max_distance = inf: guided matching is cross-check + ratio over plain 2-NN records — the oracle's — on every row whose
    forward and reverse top 2 are free of distance ties (quirk Q7 breaks ties differently by design)"""
    a, b = vk.gen_synthetic_descriptors(ORACLE_SEED, 300), vk.gen_synthetic_descriptors(ORACLE_SEED + 1, 320)
    za, zb = np.zeros(len(a), np.float32), np.zeros(len(b), np.float32)
    d2 = G.distances2(a, b)
    fs, rs = np.sort(d2, axis=1), np.sort(d2.T, axis=1)
    tied_a, tied_b = (fs[:, 0] == fs[:, 1]) | (fs[:, 1] == fs[:, 2]), (rs[:, 0] == rs[:, 1]) | (rs[:, 1] == rs[:, 2])
    tied = tied_a | tied_b[np.argmin(d2, axis=1)]       # a row is left out when its own or its nearest neighbour's top 2 hold a tie
    print(f"{int(tied.sum())} of {len(a)} rows left out for distance ties")
    assert tied.sum() <= 0.05 * len(a)
    m12, m21 = oracle.match_2nn(a, b), oracle.match_2nn(b, a)
    compared = 0
    for ratio in (0.8, 0.97):
        for cc in (False, True):
            oa, ob = oracle.filter_matches(m12, m21, ratio, cc)
            got = G.guided(G.HOMOGRAPHY, IDENTITY, 1, za, za, a, zb, zb, b, 1e6, ratio, np.inf, cc)
            want = {(int(i), int(j)) for i, j in zip(oa, ob) if not tied[i]}
            have = {(int(r["idx_a"]), int(r["idx_b"])) for r in got if not tied[r["idx_a"]]}
            assert have == want, (ratio, cc)
            for r in got:
                if not tied[r["idx_a"]]:
                    assert (r["dist_a_b1"], r["dist_a_b2"]) == (m12["dist_a_b1"][r["idx_a"]], m12["dist_a_b2"][r["idx_a"]])
            compared += len(want)
    assert compared > 50


TIE_FREE_SEED = 3           # slot_case(240, 260, seed, dups=False, amp=12): no distance tie among the three nearest of any row, either direction (asserted)


def _tie_free(s):
    d2 = G.distances2(s["desc_a"], s["desc_b"])
    for d in (d2, d2.T):
        t = np.sort(d, axis=1)[:, :3]
        if (t[:, 0] == t[:, 1]).any() or (t[:, 1] == t[:, 2]).any():
            return False
    return True


@pytest.mark.parametrize("repeat", [1, 4])
def test_guided_matches_hold_every_admissible_filtered_match(repeat):
    s = G.slot_case(240, 260, TIE_FREE_SEED, repeat=repeat, dups=False, amp=12)
    assert _tie_free(s)
    found = 0
    for kind, M in ((G.HOMOGRAPHY, G.fit_affine(np.stack([s["xa"], s["ya"], s["xb"][s["truth"]], s["yb"][s["truth"]]], axis=1)[s["truth"] >= 0])), (G.FUNDAMENTAL, s["F"])):
        for thr in (2.5, 25.0):
            adm = G.admissible(kind, M, s["xa"], s["ya"], s["xb"], s["yb"], G.threshold2(thr))
            for ratio in (0.8, 0.95):
                for cc in (False, True):
                    filt = G.guided(G.HOMOGRAPHY, IDENTITY, 1, *_args(s), 1e6, ratio, np.inf, cc)       # everything admissible: plain filtering
                    got = G.guided(kind, M, 1, *_args(s), thr, ratio, np.inf, cc)
                    have = {(int(r["idx_a"]), int(r["idx_b"])) for r in got}
                    for r in filt:
                        if adm[r["idx_a"], r["idx_b"]]:
                            assert (int(r["idx_a"]), int(r["idx_b"])) in have, (kind, thr, ratio, cc)
                            found += 1
    if repeat == 1:
        assert found > 500                             # the property was exercised


def test_repeated_structure_guided_matching_recovers_what_the_ratio_test_rejected():
    s = G.slot_case(240, 260, TIE_FREE_SEED, repeat=4, dups=False, amp=12)

    def correct(m):
        return int((s["truth"][m["idx_a"]] == m["idx_b"]).sum())

    filt = G.guided(G.HOMOGRAPHY, IDENTITY, 1, *_args(s), 1e6, 0.8, np.inf, True)
    got = G.guided(G.FUNDAMENTAL, s["F"], 1, *_args(s), 2.5, 0.8, np.inf, True)
    print(f"correct matches: filtering {correct(filt)} of {len(filt)}, guided {correct(got)} of {len(got)}, planted {int((s['truth'] >= 0).sum())}")
    assert correct(got) > correct(filt)
    assert 2 * correct(got) > int((s["truth"] >= 0).sum())


def test_kernel_slots_are_not_trivial():
    """what the GPU test relies on: rows with 0, 1, 2 and more admissible candidates, a match decided by the tie rule, both special slots"""
    slots = G.kernel_test_slots()
    assert [(len(s["xa"]), len(s["xb"])) for s in slots] == G.SLOT_SIZES
    assert {n for pair in G.SLOT_SIZES for n in pair} >= {0, 1, 2, 63, 64, 65, 255, 256, 257, 700}
    assert float(slots[G.BIG_SLOT]["xa"].max()) == 16383.0 and slots[G.INVALID_SLOT]["valid"] == 0
    seen, tie_decided = set(), 0
    for s in slots:
        for kind in (G.HOMOGRAPHY, G.FUNDAMENTAL):
            fwd, rev, adm = G.sweep(kind, s["H"] if kind == G.HOMOGRAPHY else s["F"], *_args(s), 2.5)
            seen |= set(np.minimum(adm.sum(axis=1), 3).tolist())
            got = G.decide(fwd, rev, 1.01, np.inf, False)
            tie_decided += int((got["dist_a_b1"] == got["dist_a_b2"]).sum())
    assert seen == {0, 1, 2, 3}
    assert tie_decided > 0


def test_guided_kernel_resources(tmp_path):
    """resource metadata of the code object only: no kernel of guided.hip spills to scratch memory, the sweep keeps four workgroups per CU resident"""
    import vulkansift_amd.build as b  # the flags the shipped kernels are compiled with

    src = os.path.join(ROOT, "vulkansift_amd", "csrc", "hip", "guided.hip")
    out = str(tmp_path / "guided.s")
    cmd = [b.HIPCC] + [f for f in b.HIPFLAGS if f != "-fPIC"] + b._extra_flags("hip/guided.hip") + b.INCLUDES + ["-S", "--cuda-device-only", "-o", out, src]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr
    txt = open(out).read()
    meta = [(name, int(scratch), int(vgpr)) for name, scratch, vgpr in
            re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)]
    for kernel, instances in (("k_gather_xy", 1), ("k_guided_2nn", 4), ("k_guided_keep", 1)):
        hits = [m for m in meta if kernel in m[0]]
        assert len(hits) == instances, (kernel, meta)
        for name, scratch, vgpr in hits:
            assert scratch == 0, (name, scratch)
            assert vgpr <= 128, (name, vgpr)            # 256 lanes per workgroup: four workgroups per CU stay resident at 128 VGPRs
