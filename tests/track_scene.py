"""The multi-view fixture of the track tests (plain module): six overlapping views of one synthetic scene — crops of a blob image
(vksift_ext_genSyntheticImageFamily) at six offsets, three of 192 x 144 and three of 160 x 120 pixels —, and all 15 pairs of them. A scene point seen by
several views is a track over several buffers."""
import itertools

BASE_W, BASE_H, SEED = 256, 208, 77
VIEWS = [(192, 144, 0, 0), (192, 144, 8, 4), (192, 144, 16, 10), (160, 120, 24, 2), (160, 120, 4, 16), (160, 120, 12, 12)]     # width, height, x0, y0
PAIRS = list(itertools.combinations(range(6), 2))
IDS_A, IDS_B = [a for a, _ in PAIRS], [b for _, b in PAIRS]


def images(gen_family):
    """gen_family(seed, width, height, family) -> uint8 [height, width] (vulkansift_amd.api.gen_synthetic_image_family)"""
    base = gen_family(SEED, BASE_W, BASE_H, 0)
    return [base[y0:y0 + h, x0:x0 + w].copy() for w, h, x0, y0 in VIEWS]
