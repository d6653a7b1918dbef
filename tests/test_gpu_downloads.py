"""The ways results come back to the caller (csrc/host/vksift_buffers.c, vksift_match.c) deliver the same bytes: posted records, the one-buffer packed copy, the
packed copy of a batch staged through pinned memory, and the same read by DMA into a page-locked destination; for the plain matching's records
the packed copy of all pairs and the per-pair DMA. Which strategy serves which download is pinned on the CPU (tests/test_download_plan.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def loaded(vk):
    """vksift_ext_pinHostMemory refuses until vksift_loadVulkan has run, which otherwise only the first instance of a process does (where these
    tests came from, earlier tests of the module had made one)"""
    vk.load()


def test_page_locked_destinations_receive_the_same_records(vk):
    """vksift_ext_pinHostMemory: a page-locked destination gets the records of a batched detection / matching by DMA straight from the
    packed device copy (no pinned staging, no host memcpy) — byte for byte what the pageable path returns, in any interleaving of pinned
    and pageable downloads of the same detection"""
    w, h, n = 320, 240, 16
    imgs = [vk.gen_synthetic_image_family(610 + i, w, h, i % 3) for i in range(n)]
    L = vk.lib()
    cap = 20000
    cfg = vk.default_config(sift_buffer_count=n, input_image_max_size=w * h, max_nb_sift_per_buffer=cap)
    fbuf = np.zeros(cap, vk.FEATURE_DTYPE)
    mbuf = np.zeros(cap, vk.MATCH_DTYPE)
    assert L.vksift_ext_pinHostMemory(fbuf.ctypes.data, fbuf.nbytes) == 0 and L.vksift_ext_pinHostMemory(mbuf.ctypes.data, mbuf.nbytes) == 0
    try:
        with vk.Instance(cfg, batch_capacity=n) as inst:
            ids = list(range(n))
            for order in ("pinned_first", "pageable_first"):
                inst.detectFeaturesBatch(imgs, 0)
                inst.matchFeaturesBatch(ids, ids[::-1])
                ref, got = {}, {}
                seq = ids if order == "pinned_first" else []
                if order == "pageable_first":
                    for i in ids[:3]:
                        ref[i] = inst.downloadFeatures(i)      # builds the staged copy: the pinned downloads below read it
                for i in ids:
                    cnt = inst.getFeaturesNumber(i)
                    fbuf[:] = 0
                    L.vksift_downloadFeatures(inst._h, fbuf.ctypes.data, i)
                    got[i] = fbuf[:cnt].copy()
                for i in ids:
                    if i not in ref:
                        ref[i] = inst.downloadFeatures(i)
                for i in ids:
                    assert len(got[i]) > 50 and got[i].tobytes() == ref[i].tobytes(), (order, i)
                for k in ids:
                    cnt = L.vksift_ext_getMatchesNumberBatch(inst._h, k)
                    mbuf[:] = 0
                    L.vksift_ext_downloadMatchesBatch(inst._h, k, mbuf.ctypes.data)
                    assert mbuf[:cnt].tobytes() == inst.downloadMatchesBatch(k).tobytes(), (order, k)
    finally:
        assert L.vksift_ext_unpinHostMemory(fbuf.ctypes.data) == 0 and L.vksift_ext_unpinHostMemory(mbuf.ctypes.data) == 0


def test_every_download_strategy_delivers_the_same_bytes(vk, monkeypatch):
    """8 images of 160x120 — the smallest batch that reaches the packed copy — detected as one batch and walked with a pageable and with a
    page-locked destination, then detected one by one on instances without and with feature posting (one-buffer packed copy, posted records):
    every buffer's bytes are the same four times. The same for 8 self-pairs of matches, pageable (packed copy) against page-locked (per-pair DMA)."""
    w, h, n = 160, 120, 8
    imgs = [vk.gen_synthetic_image_family(720 + i, w, h, i % 3) for i in range(n)]
    L = vk.lib()
    cap = 4000
    ids = list(range(n))
    fbuf, mbuf = np.zeros(cap, vk.FEATURE_DTYPE), np.zeros(cap, vk.MATCH_DTYPE)
    got = {}
    assert L.vksift_ext_pinHostMemory(fbuf.ctypes.data, fbuf.nbytes) == 0 and L.vksift_ext_pinHostMemory(mbuf.ctypes.data, mbuf.nbytes) == 0
    try:
        with vk.Instance(vk.default_config(sift_buffer_count=n, input_image_max_size=w * h, max_nb_sift_per_buffer=cap), batch_capacity=n) as inst:
            inst.detectFeaturesBatch(imgs, 0)
            got["pageable walk"] = [inst.downloadFeatures(i).tobytes() for i in ids]
            inst.detectFeaturesBatch(imgs, 0)
            got["page-locked walk"] = []
            for i in ids:
                cnt = inst.getFeaturesNumber(i)
                fbuf[:] = 0
                L.vksift_downloadFeatures(inst._h, fbuf.ctypes.data, i)
                got["page-locked walk"].append(fbuf[:cnt].tobytes())
            inst.matchFeaturesBatch(ids, ids)
            pageable = [inst.downloadMatchesBatch(k).tobytes() for k in ids]
            inst.matchFeaturesBatch(ids, ids)
            for k in ids:
                cnt = L.vksift_ext_getMatchesNumberBatch(inst._h, k)
                mbuf[:] = 0
                L.vksift_ext_downloadMatchesBatch(inst._h, k, mbuf.ctypes.data)
                assert cnt > 20 and mbuf[:cnt].tobytes() == pageable[k], k
    finally:
        assert L.vksift_ext_unpinHostMemory(fbuf.ctypes.data) == 0 and L.vksift_ext_unpinHostMemory(mbuf.ctypes.data) == 0
    for name, posting in (("single, not posted", "0"), ("single, posted", "1")):
        monkeypatch.setenv("VKSIFT_POST_FEATURES", posting)
        with vk.Instance(vk.default_config(sift_buffer_count=n, input_image_max_size=w * h, max_nb_sift_per_buffer=cap)) as inst:
            got[name] = []
            for i in ids:
                inst.detectFeatures(imgs[i], i)         # (an accessor between the detections: each is launched on its own)
                got[name].append(inst.downloadFeatures(i).tobytes())
    assert all(len(b) > 20 * vk.FEATURE_DTYPE.itemsize for b in got["pageable walk"])
    for name in got:
        assert got[name] == got["pageable walk"], name
