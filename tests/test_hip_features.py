"""The harness of tests/test_gpu_feature_launchers.py checked on the CPU (arena on the host, no launch): layouts, the expectation built from
the oracle, and that check() sees a byte changed anywhere outside what a launch may write."""
import numpy as np
import pytest

import hip_features as HF

f32 = np.float32


def _case(oracle, image_major, fp16):
    S, w, h, cap, batch = 3, 24, 20, 9, 2
    planes = np.stack([HF.field("periodic", S, h, w, 3 + b, fp16) for b in range(batch)])
    recs = [HF.star_points(w, h, 6, S, 1.3, 5), HF.star_points(w, h, 9, S, 1.3, 6)]
    geom = dict(pitch=w + 5, layer_gap=7, base_offset=2, image_major=True) if image_major else dict(pitch=w + 3, img_gap=11, base_offset=1)
    fa = HF.FeatureArena(planes, recs, [6, 14], cap, fp16=fp16, device="cpu", feat_gap=3, found_img_stride=4, ori_img_stride=cap + 1, sec_index=1,
                         nsec=2, front=[[5, 0], [2, 0]], dense=[7, 9], post=True, tab=HF.fp_table(oracle, 8), **geom)
    cfg = oracle.default_config(math_mode=1, nb_scales_per_octave=S, pyramid_fp16=1 if fp16 else 0)
    return fa, planes, [oracle.Pyramid.from_planes(cfg, p) for p in planes]


@pytest.mark.parametrize("fp16", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("image_major", [False, True], ids=["layer-major", "image-major"])
def test_layout_and_job(oracle, image_major, fp16):
    fa, planes, _ = _case(oracle, image_major, fp16)
    job = fa.job()
    base = fa.arena.dev.data_ptr()
    raw = fa.host
    es = 2 if fp16 else 4
    for b in range(fa.batch):
        for l in range(fa.layers):
            for (y, x) in ((0, 0), (fa.h - 1, fa.w - 1), (7, 5)):
                off = job.gauss - base + es * (b * job.img_stride + l * job.plane_stride + y * job.pitch + x)
                got = raw[off:off + es].view(np.uint16 if fp16 else np.uint32)[0]
                want = planes[b, l, y, x].astype(np.float16).view(np.uint16) if fp16 else planes[b, l, y, x].view(np.uint32)
                assert got == want, (b, l, y, x)
            pad = job.gauss - base + es * (b * job.img_stride + l * job.plane_stride + job.pitch - 1)   # pitch padding: a quiet NaN
            assert raw[pad:pad + es].view(np.uint16 if fp16 else np.uint32)[0] == (HF.HP.POISON_F16 if fp16 else HF.HP.POISON_F32)
        cnt = raw[job.found - base + 4 * b * job.found_img_stride - 4:][:8].view(np.uint32)
        assert cnt.tolist() == [[5, 6], [2, 14]][b]
        rec = raw[job.feats - base + b * job.feat_img_stride:][:HF.REC * fa.cap].view(HF.FEATURE_DTYPE)
        n = min(fa.found0[b], fa.cap)
        assert rec[:n].tobytes() == fa.recs[b].tobytes() and (rec[n:].view(np.uint8) == HF.POISON_BYTE).all()


def test_expectations_and_check(oracle):
    fa, planes, pyr = _case(oracle, False, False)
    exp, free, angles = fa.expected_orientation(pyr, 4)
    fa.check(exp, exp, "self")
    changed = np.flatnonzero(exp != fa.host)
    lo, hi = fa.feats.off, fa.feats.off + len(fa.feats.payload)
    in_feats = changed[(changed >= lo) & (changed < hi)]
    assert len(in_feats) and len(changed) - len(in_feats) <= 8              # records and the two counters, nothing else
    assert fa.found_after(exp, 0) == 6 + sum(max(len(a) - 1, 0) for a in angles[0]) > 9 == fa.cap   # un-clamped, beyond cap
    assert fa.found_after(exp, 1) == 14 + sum(max(len(a) - 1, 0) for a in angles[1])
    assert (fa.records(exp, 0)[6:9]["descriptor"] == HF.POISON_BYTE).all()  # appended copies: 9 header words only
    assert fa.records(exp, 0)[6]["scale_x"] in fa.recs[0]["scale_x"]
    for where in (fa.feats.off - 1, fa.feats.off + fa.cap * HF.REC, fa.ori_cnt.off + 4 * fa.cap, fa.found.off, fa.tab_block.off, fa.layer_refs[0].byte_off - 3,
                  fa.d_desc.off + 5):
        bad = exp.copy()
        bad[where] ^= 0x40
        with pytest.raises(AssertionError):
            fa.check(bad, exp, "tampered", free)
    ok = exp.copy()
    ok[fa.ori_cnt.off] ^= 0x40                                                # the scratch rows of valid records are free
    fa.check(ok, exp, "scratch", free)
    d = fa.expected_descriptor(pyr, dense=True, post=True)
    rows = d[fa.d_desc.off:][:16 * 128].reshape(16, 128)
    assert (rows[:5] == HF.POISON_BYTE).all() and rows[5:11].tobytes() == fa.records(d, 0)[:6]["descriptor"].tobytes() and (rows[11:] == HF.POISON_BYTE).all()
    norms = fa.words(d, fa.d_norm)
    assert norms[5] == ((rows[5].astype(np.int64) - 128) ** 2).sum()
    post = d[fa.d_post.off:][:16 * HF.REC].view(HF.FEATURE_DTYPE)
    assert post[5:11].tobytes() == fa.records(d, 0)[:6].tobytes()
