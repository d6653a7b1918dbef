"""Who owns the instance's memory, events and streams (csrc/host/vksift_mem.c), on the CPU: the module is linked against a counting
stub of the device shims (tests/native/mem_stub.c) that keeps a ledger of every live block and handle, logs the call order and can
fail the k-th allocation or enforce a byte budget. Built with gcc's address and undefined-behaviour sanitizers where their runtimes
exist: a leak of a heap block, or a sanitizer report, fails the run through the exit status.

The expected allocation sequences and sizes below are written down from create_instance() and resize_detect_scratch() as they were
before the module existed: which physical range the scale-space gets depends on what was allocated before it, so the order is pinned.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "vulkansift_amd", "csrc", "host")
MAX_OCTAVES, MAX_ORI, FEAT_BYTES, MATCH_BYTES, DESC_FP_TAB_MAX = 16, 18, 164, 20, 1024

# (batch capacity, input_image_max_size, max_nb_sift_per_buffer, sift_buffer_count, scale-space buffers)
SMALL = (1, 640 * 480, 1000, 2, 1)
PINGPONG = (2, 640 * 480, 1000, 4, 2)
BIG = (8, 4096 * 4096, 5000, 16, 1)  # a batch instance whose scale-space is placed by measurement (>= 8 images, >= 256 MB)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mem") / "mem_harness")
    san = []
    runtimes = [subprocess.run(["gcc", "-print-file-name=" + n], capture_output=True, text=True).stdout.strip() for n in ("libasan.so", "libubsan.so")]
    if all(os.path.isabs(p) and os.path.exists(p) for p in runtimes):
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]
    srcs = [os.path.join(ROOT, "tests", "native", "mem_stub.c")] + [os.path.join(HOST, f) for f in ("vksift_mem.c", "vksift_hostmath.c", "vksift_log.c")]
    subprocess.run(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror"] + san +
                   ["-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-I" + os.path.join(ROOT, "vulkansift_amd", "csrc")] + srcs + ["-lm", "-o", exe], check=True)

    def run(*cmds, env=None):
        e = {k: v for k, v in os.environ.items() if not k.startswith("VKSIFT_")}
        e.update(env or {})
        r = subprocess.run([exe] + [str(c) for c in cmds], capture_output=True, text=True, env=e)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.splitlines()
    return run


def new(cfg):
    return ("new",) + tuple(cfg)


def fields(line):
    return {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", line)}


def last(lines, word):
    return fields([l for l in lines if l.startswith(word + " ")][-1])


def calls(lines):
    """the logged shim calls, as ('D', bytes) / ('freeD', bytes) / ('E', 0) ... ; a failed call is ('D', bytes, 'FAILED')"""
    return [tuple(int(t) if t.isdigit() else t for t in l.split()[1:]) for l in lines if l.startswith("call ")]


def after(lines, word):
    """the output behind the first report of command `word`"""
    return lines[[i for i, l in enumerate(lines) if l.startswith(word + " ")][0] + 1:]


def sizes(lines):
    return {l.split()[1]: int(l.split()[2]) for l in lines if l.startswith("size ")}


def assert_clean(lines):
    led = last(lines, "ledger")
    assert led["live"] == 0 and led["bad_free"] == 0, [l for l in lines if l.startswith("live ") or "BAD" in l]


def reservation(run, cfg, w=None, h=None):
    """per-image strides of the reservation for a w x h image (default: the configured square): layout + 25 % + constant"""
    side = int(-(-(cfg[1] ** 0.5) // 1))
    d = last(run(*new(cfg), "dims", w or side, h or side, "destroy"), "dims")
    return dict(pyr=d["img_floats"] + d["img_floats"] // 4 + 4096, seg=d["seg_total"] + d["seg_total"] // 4 + 1024,
                cand=d["cand_total"] + d["cand_total"] // 4 + 4096, px=d["max_image_size"])


def scratch_sizes(cfg, r, cap, texel=4):
    """bytes of every block of the detection scratch for `cap` images"""
    feats, nbuf = cfg[2], cfg[4]
    s = {"d_pyr_buf[0]": texel * r["pyr"] * cap, "d_pyr_buf[1]": texel * r["pyr"] * cap if nbuf == 2 else -1,
         "d_seg_mask": 8 * r["seg"] * cap, "d_seg_off": 4 * r["seg"] * cap, "d_cand_xy": 4 * r["cand"] * cap, "d_cand_flag": 4 * r["cand"] * cap,
         "d_input": r["px"] * cap, "h_input": r["px"] * cap, "d_cand_n": 4 * cap * MAX_OCTAVES, "d_ori_ang": 4 * MAX_ORI * feats * cap, "d_ori_cnt": 4 * feats * cap}
    return s


STRIDE_BLOCKS = ["d_seg_mask", "d_seg_off", "d_cand_xy", "d_cand_flag"]
CAP_BLOCKS = ["d_input", "h_input", "d_cand_n", "d_ori_ang", "d_ori_cnt"]


def kind(name):
    return "H" if name.startswith("h_") else "D"


def creation_sequence(cfg, r):
    """create_instance(): the staging pair, the SIFT buffers, the extraction scratch, the matcher's slots, the stream, and only then the
    scale-space (the first of the large blocks after the stream); the other streams and the events follow"""
    bc, _, feats, nbuf, pyr_nbuf = cfg
    s = scratch_sizes(cfg, r, bc)
    align = lambda v: (v + 255) & ~255
    seq = [("D", s["d_input"]), ("H", s["h_input"]), ("D", align(feats * FEAT_BYTES) * nbuf), ("D", 4 * MAX_OCTAVES * nbuf), ("H", 4 * MAX_OCTAVES * nbuf),
           ("D", s["d_seg_mask"]), ("D", s["d_seg_off"]), ("D", s["d_cand_xy"]), ("D", s["d_cand_flag"]), ("D", s["d_cand_n"]), ("D", s["d_ori_ang"]),
           ("D", s["d_ori_cnt"]), ("D", 4 * DESC_FP_TAB_MAX), ("D", 4 * nbuf), ("D", align(feats * MATCH_BYTES) * bc), ("D", 4 * (feats + 32) * bc),
           ("D", 16 * bc), ("H", 16 * bc), ("S", 0)]
    seq += [("D", s["d_pyr_buf[0]"])] * pyr_nbuf
    seq += [("S", 0)] * 3 + [("E", 0)] * (3 + 2 + 16 + 2) + [("S", 0)] + [("E", 0)] * (4 + 1 + 1 + 8 + 16 + 6 + 2 + 2)
    return seq


# ------------------------------------------------------------------------------------------------ (a), (f)
@pytest.mark.parametrize("cfg", [SMALL, PINGPONG])
def test_creation_allocates_in_the_recorded_order_and_destruction_returns_everything(harness, cfg):
    lines = harness(*new(cfg), "create", "sizes", "destroy", "ledger")
    assert last(lines, "create")["ok"] == 1 and last(lines, "create")["fork_scales"] == 1
    r = reservation(harness, cfg)
    c = calls(lines)
    made = [x for x in c if not x[0].startswith("free")]
    assert made == creation_sequence(cfg, r)
    assert sizes(lines) == scratch_sizes(cfg, r, cfg[0])
    assert len([x for x in c if x[0].startswith("free")]) == len(made)
    assert_clean(lines)


def test_destruction_returns_every_lazy_block_and_event(harness):
    lines = harness(*new(SMALL), "create", "lazy", "ledger", "destroy", "ledger")
    assert last(lines, "lazy")["ok"] == 1
    # 20 lazy blocks of which 2 on the heap, the staging pair, 8 + 1 + 2 lazy events on top of creation's
    n_created = len(creation_sequence(SMALL, reservation(harness, SMALL)))
    assert fields([l for l in lines if l.startswith("ledger ")][0])["live"] == n_created + 18 + 2 + 11
    assert_clean(lines)


def test_placement_search_keeps_the_fastest_range_and_frees_the_rest(harness):
    lines = harness(*new(BIG), "create", "sizes", "ledger", "destroy", "ledger")
    cr = last(lines, "create")
    # the stub's first range is slow, its second fast: the search stops there, keeps the second and frees the first
    assert cr["ok"] == 1 and cr["place_n"] == 2 and cr["chosen"] == 1
    r = reservation(harness, BIG)
    pyr = 4 * r["pyr"] * 8
    c = calls(lines[:[i for i, l in enumerate(lines) if l.startswith("create ")][0]])
    assert [x for x in c if x[1] == pyr] == [("D", pyr), ("D", pyr), ("freeD", pyr)]
    assert sizes(lines) == scratch_sizes(BIG, r, 8)
    n_created = len(creation_sequence(BIG, r))
    assert fields([l for l in lines if l.startswith("ledger ")][0])["live"] == n_created
    assert_clean(lines)
    # VKSIFT_PYR_PLACEMENT is read at each search: 0 = plain allocation
    lines = harness(*new(BIG), "create", "destroy", "ledger", env={"VKSIFT_PYR_PLACEMENT": "0"})
    assert last(lines, "create")["place_n"] == 0 and [x for x in calls(lines) if x[1] == pyr] == [("D", pyr), ("freeD", pyr)]
    assert_clean(lines)


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("cfg", [SMALL, PINGPONG, BIG])
def test_creation_that_fails_at_any_allocation_leaves_nothing_behind(harness, cfg):
    made = [x for x in calls(harness(*new(cfg), "create", "destroy")) if not x[0].startswith("free")]
    n_alloc = len([x for x in made if x[0] in "DH"])
    n_handle = len(made) - n_alloc
    assert n_alloc >= 19 and n_handle >= 68  # 5 streams and 63 events
    for k in range(1, n_alloc + 1):
        lines = harness(*new(cfg), "fail", k, "create", "destroy", "ledger")
        # (the measured placement survives the loss of a candidate beyond the ones it needs)
        assert last(lines, "create")["ok"] == (1 if cfg is BIG and k == n_alloc else 0), k
        assert_clean(lines)
    for k in range(1, n_handle + 1):
        lines = harness(*new(cfg), "failh", k, "create", "lazy", "destroy", "ledger")
        assert_clean(lines)
    if cfg is not BIG:
        # handles in creation order: the stream, 3 streams, 5 events, ev_fork[16] (10..25), ev_join[2], the side stream (28), det_ring[4], ev_match (33)
        for k, ok, fork in ((1, 0, None), (2, 0, None), (10, 1, 0), (25, 1, 0), (27, 1, 0), (28, 1, 0), (29, 0, None), (32, 0, None), (33, 0, None), (40, 1, 1)):
            cr = last(harness(*new(cfg), "failh", k, "create", "destroy"), "create")
            assert cr["ok"] == ok and (fork is None or cr["fork_scales"] == fork), k


# ------------------------------------------------------------------------------------------------ (c)
def test_capacity_growth_within_budget(harness):
    r = reservation(harness, SMALL)
    lines = harness(*new(SMALL), "create", "resize", 4, 0, 0, "sizes", "destroy", "ledger")
    assert last(lines, "resize") == dict(rc=0, det_cap=4, pyr=r["pyr"], seg=r["seg"], cand=r["cand"], d_pyr=1)
    old, grown = scratch_sizes(SMALL, r, 1), scratch_sizes(SMALL, r, 4)
    assert sizes(lines) == grown
    # the old blocks go first, the pyramid in front; then the new ones in the same order
    order = ["d_pyr_buf[0]"] + STRIDE_BLOCKS + CAP_BLOCKS
    assert calls(after(lines, "create"))[:20] == [("free" + kind(n), old[n]) for n in order] + [(kind(n), grown[n]) for n in order]
    assert_clean(lines)


def test_capacity_growth_over_budget_falls_back_then_gives_up_then_recovers(harness):
    r = reservation(harness, SMALL)
    old = scratch_sizes(SMALL, r, 1)
    live = last(harness(*new(SMALL), "create", "ledger", "destroy"), "ledger")["device_live"]
    side = int(-(-(SMALL[1] ** 0.5) // 1))
    # room for what the instance has, not for four images
    lines = harness(*new(SMALL), "create", "budget", live + 4096, "resize", 4, 0, 0, "sizes", "destroy", "ledger")
    assert last(lines, "resize") == dict(rc=1, det_cap=1, pyr=r["pyr"], seg=r["seg"], cand=r["cand"], d_pyr=1)
    assert sizes(lines) == old
    assert_clean(lines)
    # room for neither: no scratch is held, the capacities are 0; with the budget lifted the next attempt succeeds
    fixed = live - sum(v for k, v in old.items() if kind(k) == "D" and v > 0)
    lines = harness(*new(SMALL), "create", "budget", fixed + 4096, "resize", 4, 0, 0, "sizes", "ledger",
                    "budget", 0, "resize", 0, side, side, "sizes", "destroy", "ledger")
    first = [l for l in lines if l.startswith("resize ")][0]
    assert fields(first) == dict(rc=-1, det_cap=1, pyr=0, seg=0, cand=0, d_pyr=0)
    i_led = [i for i, l in enumerate(lines) if l.startswith("ledger ")][0]
    assert set(sizes(lines[:i_led]).values()) == {-1}
    assert fields(lines[i_led])["device_live"] == fixed
    assert last(lines, "resize") == dict(rc=0, det_cap=1, pyr=r["pyr"], seg=r["seg"], cand=r["cand"], d_pyr=1)
    assert sizes(lines[i_led:]) == old
    assert_clean(lines)


def test_stride_growth_keeps_the_capacity_blocks_and_fails_without_a_fallback(harness):
    r, narrow = reservation(harness, SMALL), reservation(harness, SMALL, 130, 2363)
    assert narrow["pyr"] > r["pyr"]
    big = {k: max(r[k], narrow[k]) for k in ("pyr", "seg", "cand")}
    big["px"] = r["px"]
    lines = harness(*new(SMALL), "create", "resize", 0, 130, 2363, "sizes", "destroy", "ledger")
    assert last(lines, "resize") == dict(rc=0, det_cap=1, pyr=big["pyr"], seg=big["seg"], cand=big["cand"], d_pyr=1)
    assert sizes(lines) == scratch_sizes(SMALL, big, 1)
    old = scratch_sizes(SMALL, r, 1)
    order = ["d_pyr_buf[0]"] + STRIDE_BLOCKS
    assert calls(after(lines, "create"))[:10] == [("freeD", old[n]) for n in order] + [("D", scratch_sizes(SMALL, big, 1)[n]) for n in order]
    assert_clean(lines)
    live = last(harness(*new(SMALL), "create", "ledger", "destroy"), "ledger")["device_live"]
    lines = harness(*new(SMALL), "create", "budget", live + 4096, "resize", 0, 130, 2363, "sizes", "destroy", "ledger")
    assert last(lines, "resize") == dict(rc=-1, det_cap=1, pyr=0, seg=0, cand=0, d_pyr=0)
    s = sizes(lines)
    assert all(s[n] == -1 for n in order) and all(s[n] == old[n] for n in CAP_BLOCKS)
    assert_clean(lines)


def test_only_a_capacity_growth_searches_for_fast_memory(harness):
    r = reservation(harness, BIG)
    grown = harness(*new(BIG), "create", "resize", 16, 0, 0, "sizes", "destroy", "ledger")
    assert last(grown, "resize")["rc"] == 0 and sizes(grown) == scratch_sizes(BIG, r, 16)
    assert ("E", 0) in calls(after(grown, "create")) and calls(after(grown, "create")).count(("D", 4 * r["pyr"] * 16)) == 2
    assert_clean(grown)
    stride = harness(*new(BIG), "create", "resize", 0, 256, 65536, "destroy", "ledger")
    assert last(stride, "resize")["rc"] == 0 and ("E", 0) not in calls(after(stride, "create"))
    assert_clean(stride)
    live = last(harness(*new(BIG), "create", "ledger", "destroy"), "ledger")["device_live"]
    back = harness(*new(BIG), "create", "budget", live + 4096, "resize", 16, 0, 0, "sizes", "destroy", "ledger")
    c = calls(after(back, "create"))
    i_fail = [i for i, x in enumerate(c) if x[-1] == "FAILED"][0]
    assert last(back, "resize")["rc"] == 1 and sizes(back) == scratch_sizes(BIG, r, 8) and ("E", 0) not in c[i_fail:]
    assert_clean(back)


# ------------------------------------------------------------------------------------------------ (d)
def test_ensure_allocates_once_and_a_half_failed_group_only_what_is_missing(harness):
    lines = harness(*new(SMALL), "ensure", "d_corr", 4096, "ensure", "d_corr", 4096, "ensure", "filt_ids", 64, "ensure", "filt_ids", 64, "destroy", "ledger")
    assert [x for x in calls(lines) if x[0] == "D"] == [("D", 4096)]
    assert_clean(lines)
    group = ("ensure", "d_corr", 1000, "ensure", "res[PR_VERIFY_H].d_payload", 2000, "ensure", "res[PR_VERIFY_H].h_words", 3000)
    lines = harness(*new(SMALL), "fail", 2, *group, *group, "destroy", "ledger")
    oks = [fields(l)["ok"] for l in lines if l.startswith("ensure ")]
    assert oks == [1, 0, 1, 1, 1, 1]
    assert [x for x in calls(lines) if not x[0].startswith("free")] == [("D", 1000), ("D", 2000, "FAILED"), ("H", 3000), ("D", 2000)]
    assert_clean(lines)


# ------------------------------------------------------------------------------------------------ (e)
def test_staging_pair_grows_shrinks_only_when_allowed_and_is_empty_after_a_failure(harness):
    cap = lambda b: b + b // 4 + 4096
    big = 100 << 20
    edge = cap(big) // 4 - 4096  # "more than four times what is needed": cap / 4 > bytes + 4096
    lines = harness(*new(SMALL), "fit", 1000, 0, "fit", 500, 1, "fit", big, 0, "fit", 1000, 0, "fit", edge, 1, "fit", edge - 1, 1, "fit", 1000, 0,
                    "fit", 1000, 1, "destroy", "ledger")
    fits = [fields(l) for l in lines if l.startswith("fit ")]
    assert all(f["ok"] == 1 and f["d_dl"] == 1 and f["h_dl"] == 1 for f in fits)
    # grows; a small pair is never oversized; grows; the single-buffer path keeps it; exactly four times what is needed: kept; more:
    # released; grow-only again; a pair of 64 MB and less is kept however little is needed
    assert [f["cap"] for f in fits] == [cap(1000), cap(1000), cap(big), cap(big), cap(big), cap(edge - 1), cap(edge - 1), cap(edge - 1)]
    assert cap(edge - 1) <= (64 << 20) and cap(edge - 1) // 4 > 1000 + 4096
    assert_clean(lines)
    for k in (1, 2):
        lines = harness(*new(SMALL), "fit", 1000, 0, "fail", k, "fit", big, 0, "ledger", "fit", 2000, 0, "destroy", "ledger")
        fits = [fields(l) for l in lines if l.startswith("fit ")]
        assert fits[1] == dict(ok=0, cap=0, d_dl=0, h_dl=0)
        assert fields([l for l in lines if l.startswith("ledger ")][0])["live"] == 0
        assert fits[2] == dict(ok=1, cap=cap(2000), d_dl=1, h_dl=1)
        assert_clean(lines)
