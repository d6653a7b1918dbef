"""Direct access to the keypoint-stage launchers of include/vksift_hip.h (extraction, orientation, descriptor) for tests: plain module, no fixtures.

  * OctaveJob / DenseRows / bind(): the ctypes vksift_hip_OctaveJob and vksift_hip_DenseRows (tests/test_abi_hip.py compares every offset
    with the header) and the argtypes of vksift_hip_orientations(_multi) and vksift_hip_descriptors(_multi)(_dense)
  * FeatureArena: ONE byte tensor on the GPU (a hip_planes.Arena) that holds everything a job of one octave names, for a batch:
      - the S + 3 Gaussian layers as hip_planes.PlaneRef planes: pitch padding, the rows between images and the gaps between layers hold
        quiet NaNs (a kernel that USES such a texel carries the NaN into a histogram and from there into a record)
      - the feature section: image b at + b * feat_img_stride bytes; the first min(found, cap) records of an image are valid, every other
        byte — the rest of the section, the records at and beyond cap, the room between images — holds 0xA5
      - the section counters with sec_index counters in front of `found`, image b at + b * found_img_stride words
      - ori_ang / ori_cnt (poisoned: they are outputs), the fixed-point table, and on request dense rows, norms, n, a posting block, found_post
    Every block lies between two guard zones of its own, and the arena adds its own in front and behind.
  * fp_table(): the descriptor's fixed-point multipliers by R / 2, from the oracle's exported det math by the expression of orc_descriptor;
    tests/test_oracle_from_planes.py compares it with the table the product hands to the kernel (vksift_hm_desc_fp_table) and with
    orc_descriptor's own scale
  * ori_size_records() / thetas() / thirteen_scale_records(), ORI_R, DESC_R: the records that tests/test_gpu_feature_launchers.py launches and
    tests/test_feature_reference.py pins on the CPU
  * expected_orientation() / expected_descriptor(): the arena as the contract of the header says it must look after a launch, computed with
    orc_orientations / orc_descriptor; check(): byte comparison of the whole arena that names the first differing block, image and record

  * scratch=True adds what vksift_hip_extract_keypoints needs: seg_mask, seg_off, cand_xy, cand_flag, cand_n, each a block between guards,
    poisoned with 0xA5 (a launcher that relies on a cleared mask without clearing it reads set bits everywhere); expected_extraction(): the arena
    as the extraction contract says it must look, from orc_extract_keypoints (tests/extract_planes.py builds the planes of those cases)

What a launch may change (include/vksift_hip.h): extraction — words 0..8 of the first min(found, cap) records, found, and its scratch blocks
(seg_mask / seg_off: seg_img_stride * batch elements, cand_xy / cand_flag: cand_cap elements per image, cand_n: batch words); orientation — word 7 of the first min(found, cap) records, 9-word copies appended at found..
(clipped at cap), found, and its scratch rows of those records; descriptor — bytes 36..163 of the first min(found, cap) records and the dense
rows / norms / n / posting when asked for. Every other byte of the arena must come back as it went in.
"""
import ctypes as C

import numpy as np

import hip_planes as HP

MAX_ORI = 18
REC = 164
HIP_ERROR_INVALID_VALUE = 1
POISON_BYTE = 0xA5
GUARD = 1024  # bytes on either side of every block
POISON_WORD = 0xA5A5A5A5
TUNE_MULTI_MAX, TUNE_REFINE_PTR, TUNE_SCAN_BAND = 2, 3, 9  # VKSIFT_TUNE_* of the header
SEG_CHUNK, CAND_CHUNK = 4096, 256  # extrema.hip: segments per scan chunk, candidates per refinement chunk
FEATURE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("scale_x", "<f4"), ("scale_y", "<f4"), ("scale_idx", "<u4"), ("octave_idx", "<i4"),
                          ("sigma", "<f4"), ("orientation", "<f4"), ("intensity", "<f4"), ("descriptor", "u1", (128,))])
assert FEATURE_DTYPE.itemsize == REC


class OctaveJob(C.Structure):
    _fields_ = [
        ("gauss", C.c_void_p), ("fp16", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32), ("pitch", C.c_uint32),
        ("plane_stride", C.c_uint64), ("img_stride", C.c_uint64), ("S", C.c_uint32), ("octave_idx", C.c_int32),
        ("seed_sigma", C.c_float), ("dog_threshold", C.c_float), ("edge_limit", C.c_float),
        ("feats", C.c_void_p), ("feat_img_stride", C.c_uint64), ("cap", C.c_uint32), ("found", C.c_void_p), ("found_img_stride", C.c_uint32),
        ("seg_mask", C.c_void_p), ("seg_off", C.c_void_p), ("seg_img_stride", C.c_uint64),
        ("cand_xy", C.c_void_p), ("cand_flag", C.c_void_p), ("cand_n", C.c_void_p), ("cand_img_stride", C.c_uint64), ("cand_cap", C.c_uint32),
        ("ori_ang", C.c_void_p), ("ori_cnt", C.c_void_p), ("ori_img_stride", C.c_uint64), ("max_ori", C.c_uint32), ("use_vlfeat", C.c_uint32),
        ("desc_fp_tab", C.c_void_p), ("desc_fp_tab_len", C.c_uint32), ("scan_reverse", C.c_uint32), ("masks_cleared", C.c_uint32),
        ("sec_index", C.c_uint32),
    ]


class DenseRows(C.Structure):
    _fields_ = [
        ("desc", C.c_void_p), ("desc_img_stride", C.c_uint64), ("norm", C.c_void_p), ("norm_img_stride", C.c_uint64),
        ("n", C.c_void_p), ("n_img_stride", C.c_uint32), ("nsec", C.c_uint32), ("sec_cap", C.c_uint32 * 16),
        ("post", C.c_void_p), ("post_img_stride", C.c_uint64), ("found_post", C.c_void_p), ("found_post_n", C.c_uint32),
    ]


def bind(L):
    jp, dp, u32, vp = C.POINTER(OctaveJob), C.POINTER(DenseRows), C.c_uint32, C.c_void_p
    sigs = {
        "vksift_hip_orientations": [jp, u32, vp],
        "vksift_hip_descriptors": [jp, u32, vp],
        "vksift_hip_orientations_multi": [jp, u32, u32, vp],
        "vksift_hip_descriptors_multi": [jp, u32, u32, vp],
        "vksift_hip_descriptors_multi_dense": [jp, u32, u32, dp, vp],
        "vksift_hip_extract_keypoints": [jp, u32, vp, vp],
        "vksift_hip_extract_keypoints_multi": [jp, u32, u32, vp, vp],
        "vksift_hip_clear_segment_masks": [jp, u32, u32, vp],
        "vksift_hip_tune": [C.c_int, C.c_int],
        "vksift_hip_tune_get": [C.c_int],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = C.c_int
    L.vksift_hip_error_string.argtypes = [C.c_int]
    L.vksift_hip_error_string.restype = C.c_char_p
    return L


# ---------------------------------------------------------------------------------------------------------------- window sizes (fp32, as the
# kernels and the oracle form them)
f32 = np.float32


def rel_sigma(rec):
    """sigma / 2^octave_idx of a record"""
    return f32(f32(rec["sigma"]) / f32(2.0 ** int(rec["octave_idx"])))


def ori_radius(rec):
    """(r, lambda) of the orientation window (ComputeOrientation.comp:63-65)"""
    lam = f32(f32(1.5) * rel_sigma(rec))
    return int(np.floor(f32(f32(3) * lam))), float(lam)


def desc_radius(rec):
    """R of the descriptor window (ComputeDescriptors.comp:107-109)"""
    lam = f32(f32(3.0) * rel_sigma(rec))
    radius = f32(f32(f32(f32(np.sqrt(f32(2.0))) * lam) * f32(5)) * f32(0.5))
    return int(np.floor(f32(radius + f32(0.5))))


def rel_for_r(r):
    """a relative sigma whose orientation radius is r (the middle of its interval)"""
    return float(f32((r + 0.5) / 4.5))


def rel_for_R(R):
    """a relative sigma whose descriptor radius is R (R >= 1)"""
    return float(f32(R / (np.sqrt(2.0) * 7.5)))


def round_half_away(v):
    v = float(f32(v))
    return int(np.floor(abs(v) + 0.5) * (1 if v >= 0 else -1))


def ori_fast_path(rec, w, h):
    """does k_orientation take its interior form for this record (window and taps inside the image interior)?"""
    r, _ = ori_radius(rec)
    cx, cy = round_half_away(rec["scale_x"]), round_half_away(rec["scale_y"])
    return cx - r >= 1 and cx + r <= w - 2 and cy - r >= 1 and cy + r <= h - 2


def desc_rows(rec, w, h):
    """(bw, bh): extent of the descriptor window clipped to the image interior (<= 0: empty)"""
    R = desc_radius(rec)
    cx, cy = round_half_away(rec["scale_x"]), round_half_away(rec["scale_y"])
    dx0, dx1 = max(-R, 1 - cx), min(R, w - 2 - cx)
    dy0, dy1 = max(-R, 1 - cy), min(R, h - 2 - cy)
    return dx1 - dx0 + 1, dy1 - dy0 + 1


def fp_table(oracle, n):
    """fixed-point multipliers indexed by R / 2, entries 0 .. n - 1: 1 << (16 - ceil_log2(m)) with m summed as orc_descriptor sums it
    (entry 0: the sum is empty and the shift is defined as 16)"""
    L = oracle.lib()
    es = f32(-1.0) / f32(8.0)
    sqrt2 = f32(np.sqrt(f32(2.0)))
    tab = np.empty(n, f32)
    last = None
    for k in range(n):
        if last is not None and k > 24:  # the terms beyond i, j = 24 are below half an ulp of the sum (e^-72): the sum no longer moves
            tab[k] = last
            continue
        m = f32(0)
        for i in range(k):
            m = f32(m + f32(f32(L.orc_dm_expf(float(f32(es * f32(i * i + i * i))))) * sqrt2))
            for j in range(i + 1, k):
                m = f32(m + f32(f32(f32(L.orc_dm_expf(float(f32(es * f32(i * i + j * j))))) * sqrt2) * f32(2)))
        tab[k] = f32(1 << (16 - L.orc_dm_ceil_log2f(float(m)))) if m > 0 else f32(1 << 16)
        last = tab[k]
    return tab


def make_records(rows):
    """rows of (scale_x, scale_y, scale_idx, octave_idx, relative sigma, orientation) -> FEATURE_DTYPE records. x, y and intensity get
    recognisable values (the kernels only carry them), the descriptor bytes are poison."""
    out = np.zeros(len(rows), FEATURE_DTYPE)
    out["descriptor"] = POISON_BYTE
    for i, (sx, sy, si, oi, rel, th) in enumerate(rows):
        out[i]["scale_x"], out[i]["scale_y"] = f32(sx), f32(sy)
        out[i]["scale_idx"], out[i]["octave_idx"] = si, oi
        out[i]["sigma"] = f32(f32(rel) * f32(2.0 ** oi))
        out[i]["orientation"] = f32(th)
        out[i]["x"], out[i]["y"] = f32(f32(sx) * f32(2.0 ** oi)), f32(f32(sy) * f32(2.0 ** oi))
        out[i]["intensity"] = f32(0.001 * (i + 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- the arena
class Block:
    """a run of bytes inside the arena, between two guard zones of its own"""

    def __init__(self, name, payload):
        self.name = name
        self.payload = np.ascontiguousarray(payload).view(np.uint8).reshape(-1).copy()
        self.ref = None

    @property
    def off(self):
        return self.ref.byte_off + GUARD

    @property
    def ptr(self):
        return self.ref.ptr + GUARD


class FeatureArena:
    def __init__(self, planes, recs, found, cap, *, fp16=False, pitch=None, layer_gap=0, img_gap=0, image_major=False, base_offset=0,
                 feat_gap=0, found_img_stride=None, ori_img_stride=None, sec_index=0, front=None, nsec=None, tab=None,
                 dense=None, post=False, dense_strides=(0, 0, 0, 0), device="cuda", scratch=False, cand_cap=None, cand_img_stride=None,
                 seg_extra=0):
        """planes: (batch, S + 3, h, w) float32 (binary16 values when fp16); recs: per image, the valid records (min(found, cap) of them);
        found: per image, the counter on entry; front: per image, the sec_index counters in front of it (and the counters behind it up to
        nsec); dense: None or a list of sec_cap (nsec entries): dense rows, norms and n are laid out; post: a posting block as well.
        scratch: the extraction stage's scratch blocks as well (cand_cap: candidates per image, default the most an octave can have + 64;
        cand_img_stride >= cand_cap; seg_extra: elements behind the batch's seg_mask / seg_off regions, which a launch must leave alone).
        found=None (extraction: the counter is an output): the counter holds poison on entry and the section no record."""
        planes = np.asarray(planes, f32)
        self.batch, self.layers, self.h, self.w = planes.shape
        self.found_is_output = found is None
        if found is None:
            found, recs = [POISON_WORD] * self.batch, [np.zeros(0, FEATURE_DTYPE)] * self.batch
        self.S = self.layers - 3
        self.fp16, self.cap, self.sec_index = bool(fp16), int(cap), int(sec_index)
        self.found0 = [int(v) for v in found]
        self.recs = [np.array(r, FEATURE_DTYPE) for r in recs]
        assert len(self.found0) == self.batch and len(self.recs) == self.batch
        for r, f in zip(self.recs, self.found0):
            assert self.found_is_output or len(r) == min(f, self.cap), (len(r), f, self.cap)
        self.arena = HP.Arena(device)
        kind = "f16" if fp16 else "f32"
        pitch = int(pitch or self.w)
        if image_major:
            # one PlaneRef of batch * (S + 3) planes: layer l of image b is its plane b * (S + 3) + l
            self.plane_stride = pitch * self.h + layer_gap
            assert img_gap == 0, "image-major: the images follow each other a whole number of layers apart"
            self.img_stride = self.plane_stride * self.layers
            ref = self.arena.plane("layers", self.w, self.h, self.batch * self.layers, kind=kind, pitch=pitch, img_stride=self.plane_stride,
                                   offset=base_offset, data=planes.reshape(self.batch * self.layers, self.h, self.w))
            self.layer_refs = [ref]
        else:
            # one PlaneRef per layer, each holding the batch: equal sizes, so the arena lays them out a constant distance apart
            self.img_stride = pitch * self.h + img_gap
            self.layer_refs = [self.arena.plane(f"layer{l}", self.w, self.h, self.batch, kind=kind, pitch=pitch, img_stride=self.img_stride,
                                                offset=base_offset, data=planes[:, l]) for l in range(self.layers)]
        self.pitch = pitch

        # feature section
        self.feat_img_stride = self.cap * REC + 4 * int(feat_gap)
        sec = np.full((self.batch - 1) * self.feat_img_stride + (self.cap + 3) * REC, POISON_BYTE, np.uint8)  # three poisoned records beyond cap
        for b, r in enumerate(self.recs):
            sec[b * self.feat_img_stride:b * self.feat_img_stride + len(r) * REC] = r.view(np.uint8).reshape(-1)
        self.feats = Block("feature section", sec)

        # counters
        self.nsec = int(nsec if nsec is not None else self.sec_index + 1)
        assert self.sec_index < self.nsec or dense is None
        self.found_img_stride = int(found_img_stride or max(self.nsec, 1))
        assert self.found_img_stride >= self.nsec or self.batch == 1
        cnt = np.full((self.batch - 1) * self.found_img_stride + max(self.nsec, self.sec_index + 1), 0xA5A5A5A5, np.uint32)
        self.counters = []  # per image: every section's counter on entry
        for b in range(self.batch):
            c = list(front[b]) if front is not None else [0] * max(self.nsec, self.sec_index + 1)
            c[self.sec_index] = self.found0[b]
            cnt[b * self.found_img_stride:b * self.found_img_stride + len(c)] = c
            self.counters.append(c)
        self.found = Block("section counters", cnt)

        # orientation scratch (outputs: poisoned)
        self.ori_img_stride = int(ori_img_stride or self.cap)
        assert self.ori_img_stride >= self.cap or self.batch == 1
        nk = (self.batch - 1) * self.ori_img_stride + self.cap
        self.ori_ang = Block("ori_ang", np.full(nk * MAX_ORI, 0xA5A5A5A5, np.uint32))
        self.ori_cnt = Block("ori_cnt", np.full(nk, 0xA5A5A5A5, np.uint32))

        self.tab = np.asarray(tab if tab is not None else np.full(1, 65536, f32), f32)  # entry 0 alone: enough for the orientation launcher, which reads none
        self.tab_block = Block("fixed-point table", self.tab)

        self.blocks = [self.feats, self.found, self.ori_ang, self.ori_cnt, self.tab_block]
        self.scratch = bool(scratch)
        if scratch:
            self.nseg = (self.w + 63) // 64
            self.nsegs = self.S * self.h * self.nseg          # seg_img_stride: the contract fixes it
            self.nchunks = -(-self.nsegs // SEG_CHUNK)
            self.seg_extra = int(seg_extra)
            most = self.S * 2 * ((self.w - 1) // 2) * ((self.h - 1) // 2)   # tests/test_extraction_limits.py
            self.cand_cap = int(cand_cap) if cand_cap is not None else max(most + 64, self.nchunks)
            self.cand_img_stride = int(cand_img_stride) if cand_img_stride is not None else self.cand_cap
            nseg_words = self.nsegs * self.batch + self.seg_extra
            ncand = (self.batch - 1) * self.cand_img_stride + self.cand_cap
            self.seg_mask = Block("seg_mask", np.full(nseg_words, 0xA5A5A5A5A5A5A5A5, np.uint64))
            self.seg_off = Block("seg_off", np.full(nseg_words, POISON_WORD, np.uint32))
            self.cand_xy = Block("cand_xy", np.full(ncand, POISON_WORD, np.uint32))
            self.cand_flag = Block("cand_flag", np.full(ncand, POISON_WORD, np.uint32))
            self.cand_n = Block("cand_n", np.full(self.batch, POISON_WORD, np.uint32))
            self.blocks += [self.seg_mask, self.seg_off, self.cand_xy, self.cand_flag, self.cand_n]
        self.dense_caps = None
        self.post = bool(post)
        if dense is not None or post:
            self.dense_caps = [int(v) for v in dense] if dense is not None else [self.cap] * self.nsec
            assert len(self.dense_caps) == self.nsec
            rows = max(sum(self.dense_caps), 2)
            self.max_rows = rows
            self.desc_img_stride = rows * 128 + 128 * dense_strides[0]
            self.norm_img_stride = rows + dense_strides[1]
            self.n_img_stride = 1 + dense_strides[2]
            self.post_img_stride = rows * REC + 4 * dense_strides[3]
            self.rows_on = dense is not None
            if self.rows_on:
                self.d_desc = Block("dense rows", np.full((self.batch - 1) * self.desc_img_stride + rows * 128, POISON_BYTE, np.uint8))
                self.d_norm = Block("dense norms", np.full((self.batch - 1) * self.norm_img_stride + rows, 0xA5A5A5A5, np.uint32))
                self.d_n = Block("dense n", np.full((self.batch - 1) * self.n_img_stride + 1, 0xA5A5A5A5, np.uint32))
                self.blocks += [self.d_desc, self.d_norm, self.d_n]
            if post:
                self.d_post = Block("posting block", np.full((self.batch - 1) * self.post_img_stride + rows * REC, POISON_BYTE, np.uint8))
                self.d_found_post = Block("found_post", np.full(self.batch * self.nsec, 0xA5A5A5A5, np.uint32))
                self.blocks += [self.d_post, self.d_found_post]
        for blk in self.blocks:
            body = np.full(len(blk.payload) + 2 * GUARD, POISON_BYTE, np.uint8)
            body[GUARD:GUARD + len(blk.payload)] = blk.payload
            blk.ref = self.arena.plane(blk.name, len(body), 1, kind="u8", data=body.reshape(1, 1, -1))
        self.arena.build()
        if not image_major:
            step = self.layer_refs[1].byte_off - self.layer_refs[0].byte_off
            assert all(self.layer_refs[l + 1].byte_off - self.layer_refs[l].byte_off == step for l in range(self.layers - 1))
            self.plane_stride = step // self.layer_refs[0].es
        self.host = self.arena.host

    # ------------------------------------------------------------------------------------------------------------ the job
    def job(self, *, max_ori=4, use_vlfeat=0, octave_idx=0, seed_sigma=1.6, dog_threshold=None, edge_limit=12.1, scan_reverse=0, masks_cleared=0,
            cap=None):
        """dog_threshold: default intensity_threshold 0.04 / S; cap: a section capacity below the arena's (the records behind it are poison)"""
        j = OctaveJob()
        j.gauss = self.layer_refs[0].ptr
        j.fp16 = 1 if self.fp16 else 0
        j.w, j.h, j.pitch = self.w, self.h, self.pitch
        j.plane_stride, j.img_stride = self.plane_stride, self.img_stride
        j.S, j.octave_idx = self.S, octave_idx
        j.seed_sigma, j.dog_threshold, j.edge_limit = seed_sigma, (0.04 / self.S if dog_threshold is None else dog_threshold), edge_limit
        j.feats, j.feat_img_stride, j.cap = self.feats.ptr, self.feat_img_stride, (self.cap if cap is None else cap)
        assert j.cap <= self.cap
        j.scan_reverse, j.masks_cleared = scan_reverse, masks_cleared
        if self.scratch:
            j.seg_mask, j.seg_off, j.seg_img_stride = self.seg_mask.ptr, self.seg_off.ptr, self.nsegs
            j.cand_xy, j.cand_flag, j.cand_n = self.cand_xy.ptr, self.cand_flag.ptr, self.cand_n.ptr
            j.cand_img_stride, j.cand_cap = self.cand_img_stride, self.cand_cap
        j.found, j.found_img_stride = self.found.ptr + 4 * self.sec_index, self.found_img_stride
        j.ori_ang, j.ori_cnt, j.ori_img_stride = self.ori_ang.ptr, self.ori_cnt.ptr, self.ori_img_stride
        j.max_ori, j.use_vlfeat = max_ori, use_vlfeat
        j.desc_fp_tab, j.desc_fp_tab_len = self.tab_block.ptr, len(self.tab)
        j.sec_index = self.sec_index
        return j

    def dense_rows(self, nsec=None):
        d = DenseRows()
        if self.rows_on:
            d.desc, d.desc_img_stride = self.d_desc.ptr, self.desc_img_stride
            d.norm, d.norm_img_stride = self.d_norm.ptr, self.norm_img_stride
            d.n, d.n_img_stride = self.d_n.ptr, self.n_img_stride
        d.nsec = self.nsec if nsec is None else nsec
        for i, v in enumerate(self.dense_caps):
            d.sec_cap[i] = v
        if self.post:
            d.post, d.post_img_stride = self.d_post.ptr, self.post_img_stride
            d.found_post, d.found_post_n = self.d_found_post.ptr, self.nsec
        return d

    # ------------------------------------------------------------------------------------------------------------ views into arena bytes
    def records(self, raw, b, n=None):
        n = self.cap if n is None else n
        off = self.feats.off + b * self.feat_img_stride
        return raw[off:off + n * REC].view(FEATURE_DTYPE)

    def words(self, raw, blk):
        return raw[blk.off:blk.off + len(blk.payload)].view(np.uint32)

    def found_after(self, raw, b):
        return int(self.words(raw, self.found)[b * self.found_img_stride + self.sec_index])

    # ------------------------------------------------------------------------------------------------------------ expectations
    def expected_orientation(self, pyramids, max_ori):
        """(arena bytes after vksift_hip_orientations, mask of the scratch bytes the launch may change, per image the kept angle lists)"""
        exp = self.host.copy()
        free = np.zeros(len(exp), bool)
        keep = MAX_ORI if max_ori == 0 else min(max_ori, MAX_ORI)
        angles = []
        for b in range(self.batch):
            recs = self.records(exp, b)
            n0 = min(self.found0[b], self.cap)
            total = self.found0[b]
            per = []
            for k in range(n0):
                ang, _ = pyramids[b].orientations(0, recs[k])
                ang = ang[:keep]
                per.append(ang)
                if len(ang):
                    recs[k]["orientation"] = ang[0]
                for a in ang[1:]:
                    if total < self.cap:
                        dst = recs[total:total + 1].view(np.uint8)
                        dst[:36] = recs[k:k + 1].view(np.uint8)[:36]
                        recs[total]["orientation"] = a
                    total += 1
            self.words(exp, self.found)[b * self.found_img_stride + self.sec_index] = total & 0xFFFFFFFF
            k0 = b * self.ori_img_stride
            free[self.ori_ang.off + 4 * MAX_ORI * k0:self.ori_ang.off + 4 * MAX_ORI * (k0 + n0)] = True
            free[self.ori_cnt.off + 4 * k0:self.ori_cnt.off + 4 * (k0 + n0)] = True
            angles.append(per)
        return exp, free, angles

    def expected_extraction(self, pyramids, *, octave_idx=0, cap=None, keep=None, seg_free=()):
        """(arena bytes after vksift_hip_extract_keypoints, mask of the scratch bytes the launch may change, per image the un-clamped count).
        Records and count: orc_extract_keypoints in det math mode on pyramids[b] (Pyramid.from_planes, octave index 0); for another octave_idx
        the oracle's x, y and sigma are scaled by 2^octave_idx, which is exact in fp32 (tests/test_extract_reference.py compares it with the
        oracle's own octave -1). Words 0..8 of the first min(found, cap) records over the poison, nothing else of the section.
        keep: per image, how many of the oracle's keypoints the candidate list holds (cand_cap below the candidate count: the contract keeps
        the first cand_cap candidates in raster order, so the first `keep` keypoints); seg_free: further (lo, hi) element ranges of the seg
        blocks that belong to other jobs of the call (their regions inside this arena's seg blocks)."""
        assert self.scratch
        cap = self.cap if cap is None else cap
        exp = self.host.copy()
        free = np.zeros(len(exp), bool)
        counts = []
        for b in range(self.batch):
            recs, n = pyramids[b].extract_keypoints(0, cap=max(cap, 1) if keep is None else 1 << 20)
            if keep is not None:
                n = int(keep[b])
                recs = recs[:n]
            recs = recs[:min(n, cap)].copy()
            assert (recs["octave_idx"] == 0).all() and (recs["orientation"] == 0).all()
            sf = f32(2.0 ** octave_idx)
            recs["x"], recs["y"], recs["sigma"] = recs["x"] * sf, recs["y"] * sf, recs["sigma"] * sf
            recs["octave_idx"] = octave_idx
            dst = self.records(exp, b, len(recs)).view(np.uint8).reshape(-1, REC)
            dst[:, :36] = recs.view(np.uint8).reshape(-1, REC)[:, :36]
            self.words(exp, self.found)[b * self.found_img_stride + self.sec_index] = n
            counts.append(n)
            for blk in (self.cand_xy, self.cand_flag):
                lo = blk.off + 4 * b * self.cand_img_stride
                free[lo:lo + 4 * self.cand_cap] = True
        free[self.seg_mask.off:self.seg_mask.off + 8 * self.nsegs * self.batch] = True
        free[self.seg_off.off:self.seg_off.off + 4 * self.nsegs * self.batch] = True
        for lo, hi in seg_free:
            free[self.seg_mask.off + 8 * lo:self.seg_mask.off + 8 * hi] = True
            free[self.seg_off.off + 4 * lo:self.seg_off.off + 4 * hi] = True
        free[self.cand_n.off:self.cand_n.off + 4 * self.batch] = True
        return exp, free, counts

    def expected_descriptor(self, pyramids, dense=False, post=False):
        exp = self.host.copy()
        for b in range(self.batch):
            recs = self.records(exp, b)
            n1 = min(self.found0[b], self.cap)
            for k in range(n1):
                assert desc_radius(recs[k]) // 2 < len(self.tab), "the fixed-point table of the case is too short for this record"
                recs[k]["descriptor"], _ = pyramids[b].descriptor(0, recs[k])
            if not (dense or post):
                continue
            stored = [min(c, cp) for c, cp in zip(self.counters[b][:self.nsec], self.dense_caps)]
            row0, total = sum(stored[:self.sec_index]), sum(stored)
            d = recs[:n1]["descriptor"]
            if dense:
                rows = exp[self.d_desc.off + b * self.desc_img_stride:][:self.max_rows * 128].reshape(-1, 128)
                norms = self.words(exp, self.d_norm)[b * self.norm_img_stride:][:self.max_rows]
                rows[row0:row0 + n1] = d
                norms[row0:row0 + n1] = ((d.astype(np.int64) - 128) ** 2).sum(1)
                if self.sec_index == 0:
                    self.words(exp, self.d_n)[b * self.n_img_stride] = total
                    if total < 2:  # quirk Q6: the rows below 2 of a buffer with fewer features read as zero descriptors
                        rows[total:2] = 0
                        norms[total:2] = 128 ** 3
            if post:
                out = exp[self.d_post.off + b * self.post_img_stride:][:self.max_rows * REC].view(FEATURE_DTYPE)
                out[row0:row0 + n1] = recs[:n1]
                if self.sec_index == 0:
                    self.words(exp, self.d_found_post)[b * self.nsec:(b + 1) * self.nsec] = self.counters[b][:self.nsec]
        return exp

    # ------------------------------------------------------------------------------------------------------------ comparison
    def where(self, byte):
        for blk in self.blocks:
            lo = blk.ref.byte_off
            if lo <= byte < lo + len(blk.payload) + 2 * GUARD:
                o = byte - blk.off
                if o < 0 or o >= len(blk.payload):
                    return f"guard zone of {blk.name!r} ({o} bytes from its start)"
                if blk is self.feats:
                    b = min(o // self.feat_img_stride, self.batch - 1)
                    r = o - b * self.feat_img_stride
                    return f"feature section image {b} record {r // REC} byte {r % REC} (cap {self.cap}, found on entry {self.found0[b]})"
                return f"{blk.name!r} byte {o} (word {o // 4})"
        return self.arena.where(byte)

    def check(self, after, exp, what, free=None):
        bad = after != exp
        if free is not None:
            bad &= ~free
        if bad.any():
            idx = np.flatnonzero(bad)
            b = int(idx[0])
            raise AssertionError(f"{what}: {len(idx)} bytes differ from the contract, first at arena byte {b}: {self.where(b)}: "
                                 f"expected 0x{int(exp[b]):02x}, got 0x{int(after[b]):02x}")

    def read(self):
        return self.arena.read()


# ---------------------------------------------------------------------------------------------------------------- planes of the cases
FAMILIES = ("smooth", "blackhalf", "tiny", "const", "periodic")
STAR_CELL = 16


def field(family, S, h, w, seed, fp16=False):
    """(S + 3, h, w) float32 Gaussian layers of one image; every layer differs from the others, so a wrong layer shows.
    smooth: random cosines + a little noise, amplitudes in [0, 1] · blackhalf: the same with exact zeros on the left half ·
    tiny: the same with the left half times 2^-60 (gradients below 2^-48 send a whole wave step through the kernels' general-form fallback,
    the lanes on the right half with it) · const: no gradient inside the image · periodic: a five- or six-armed star in every 16 x 16 tile —
    a keypoint on a tile centre (star_points) has up to five histogram peaks. fp16: every value rounded to binary16."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = np.empty((S + 3, h, w), f32)
    for l in range(S + 3):
        if family == "const":
            v = np.full((h, w), 0.25 + 0.03125 * l)
        elif family == "periodic":
            # a star in every 16 x 16 tile: N = 5 or 6 lobes of tangential gradients around the tile centre
            dx, dy = xx % STAR_CELL - STAR_CELL / 2 + 0.5, yy % STAR_CELL - STAR_CELL / 2 + 0.5
            lobes = 5 + ((xx // STAR_CELL + yy // STAR_CELL) % 2)
            v = 0.5 + 0.4 * np.cos(lobes * np.arctan2(dy, dx) + 0.2 * l) * np.minimum(np.hypot(dx, dy) / 3, 1)
        else:
            v = np.zeros((h, w))
            for _ in range(6):
                lam = np.exp(rng.uniform(np.log(5), np.log(60)))
                a, ph = rng.uniform(0, 2 * np.pi), rng.uniform(0, 2 * np.pi)
                v += rng.uniform(0.3, 1) * np.cos(2 * np.pi / lam * (xx * np.cos(a) + yy * np.sin(a)) + ph)
            v = (v - v.min()) / max(v.max() - v.min(), 1e-9) * 0.9 + 0.1 * rng.random((h, w))
            if family == "blackhalf":
                v[:, :w // 2] = 0
            if family == "tiny":
                v[:, :w // 2] *= 2.0 ** -60
        out[l] = v.astype(f32)
    if fp16:
        out = out.astype(np.float16).astype(f32)
    return out


def star_points(w, h, n, S, rel, seed, octave_idx=0):
    """n records on (jittered) tile centres of the periodic family"""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        cx = int(rng.integers(0, w // STAR_CELL)) * STAR_CELL + STAR_CELL / 2 - 0.5 + rng.uniform(-0.4, 0.4)
        cy = int(rng.integers(0, h // STAR_CELL)) * STAR_CELL + STAR_CELL / 2 - 0.5 + rng.uniform(-0.4, 0.4)
        rows.append((cx, cy, i % (S + 2), octave_idx, rel, 0.0))
    return make_records(rows)


# ---------------------------------------------------------------------------------------------------------------- records of the cases
ORI_R = [0, 1, 31, 63, 64, 65, 108, 127, 128, 130]   # orientation radii: one, two and three passes of the fixed-point-scale loop
DESC_R = [1, 2, 3, 21, 127, 128, 129, 255, 257]      # descriptor radii
S_MAX = 13                                           # the largest nb_scales_per_octave a configuration may ask for: 16 layers


def ori_size_records(w, h, S):
    """(records, the r each is built for): every r of ORI_R at an interior, a bottom-left and a top-right position, and relative sigmas of
    0.02 and 0.05 (lambda < 0.08: es * d2 can pass dm_expf's clamp at -87.3); scale_idx and octave_idx cycle through their ranges"""
    rows, want_r = [], []
    i = 0
    for r in ORI_R:
        rel = rel_for_r(r) if r else 0.1
        for (x, y) in ((w / 2 + 0.3, h / 2 - 0.2), (7.6, h - 9.25), (w - 3.5, 4.5)):
            rows.append((x, y, i % (S + 2), (i % 8) - 1, rel, 0.0))
            want_r.append(r)
            i += 1
    for rel in (0.02, 0.05):
        for (x, y) in ((w / 2 + 0.49, h / 2 + 0.5), (0.2, 0.4), (w - 0.51, h - 1.0)):
            rows.append((x, y, i % (S + 2), (i % 8) - 1, rel, 0.0))
            want_r.append(0)
            i += 1
    return make_records(rows), want_r


def thetas():
    """orientations fed to the descriptor: 0, the fp32 values nearest pi/2, pi, 3pi/2 and 2pi and their neighbours, all 72 values a
    histogram peak can take, 24 random ones"""
    PI = np.pi
    near = [float(f32(v)) for v in (PI / 2, PI, 3 * PI / 2, 2 * PI)]
    near += [float(np.nextafter(f32(v), f32(0))) for v in (PI / 2, PI, 3 * PI / 2, 2 * PI)] + [float(np.nextafter(f32(PI), f32(4)))]
    bins = [float(f32(f32(f32(f32(k / 2.0) + f32(0.5)) * f32(2 * PI)) / f32(36))) for k in range(72)]  # (k / 2 + 0.5) * 2 pi / 36, as the kernel forms it
    rnd = np.random.default_rng(90).uniform(0, 2 * PI, 24).astype(f32).tolist()
    return [0.0] + near + bins + rnd


def thirteen_scale_records(w, h, seed):
    """S = 13: three records on each scale_idx 0 .. 14, so every layer a record may name is read; windows from a few texels to larger than
    a small plane (r = 1 .. 64, R = 4 .. 152), every octave_idx, orientations incl. 0"""
    rng = np.random.default_rng(seed)
    th = [0.0, float(f32(np.pi))] + rng.uniform(0, 2 * np.pi, 43).astype(f32).tolist()
    rels = (0.4, 1.0, 2.6, 5.0, rel_for_r(64))
    rows = [(rng.uniform(0, w - 0.001), rng.uniform(0, h - 0.001), i % (S_MAX + 2), (i % 8) - 1, rels[(i + i // 15) % 5], th[i]) for i in range(45)]
    recs = make_records(rows)
    assert sorted(set(recs["scale_idx"].tolist())) == list(range(S_MAX + 2)) and set(recs["octave_idx"].tolist()) == set(range(-1, 7))
    return recs
