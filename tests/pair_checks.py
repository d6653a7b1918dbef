"""What the tests of the pair stages share: the correspondences of a pair's filtered matches, and the comparison of a result record with its
restatement (tests/np_verify.py, np_verify_f.py, np_refine.py, np_refine_f.py). One definition of each for tests/test_gpu_verify.py,
test_gpu_verify_fundamental.py, test_gpu_refine.py, test_gpu_refine_f.py and the model of tests/api_model.py. No GPU, no library."""
import numpy as np


def corr(fa, fb, fm):
    """float32 [n, 4] {xa, ya, xb, yb} of the filtered matches fm between the downloaded feature sets fa and fb"""
    return np.stack([fa["x"][fm["idx_a"]], fa["y"][fm["idx_a"]], fb["x"][fm["idx_b"]], fb["y"][fm["idx_b"]]], axis=1).astype(np.float32).reshape(-1, 4)


def same_homography(got, want, ctx):
    """a vksift_ext_Homography record against np_verify.ransac's"""
    assert int(got["valid"]) == want["valid"], ctx
    assert int(got["nb_matches"]) == want["nb_matches"], ctx
    assert (int(got["best_hypothesis"]), int(got["nb_inliers"])) == (want["best_hypothesis"], want["nb_inliers"]), ctx
    assert np.asarray(got["H"], np.float32).tobytes() == want["H"].tobytes(), (ctx, got["H"], want["H"])


def same_fundamental(got, want, ctx):
    """a vksift_ext_Fundamental record against np_verify_f.ransac's"""
    assert int(got["valid"]) == want["valid"], ctx
    assert int(got["nb_matches"]) == want["nb_matches"], ctx
    assert (int(got["best_hypothesis"]), int(got["best_root"]), int(got["nb_inliers"])) == (want["best_hypothesis"], want["best_root"], want["nb_inliers"]), ctx
    assert np.asarray(got["F"], np.float32).tobytes() == want["F"].tobytes(), (ctx, got["F"], want["F"])


def _same_refined(got, want, ctx, model):
    assert (int(got["valid"]), int(got["nb_matches"]), int(got["nb_inliers"]), int(got["rounds"])) == (want["valid"], want["nb_matches"], want["nb_inliers"], want["rounds"]), \
        (ctx, got, {k: v for k, v in want.items() if k != "mask"})
    assert np.asarray(got[model], np.float32).tobytes() == np.asarray(want[model], np.float32).tobytes(), (ctx, got[model], want[model])


def same_refined_homography(got, want, ctx):
    """a vksift_ext_RefinedHomography record against np_refine.refit's"""
    _same_refined(got, want, ctx, "H")


def same_refined_fundamental(got, want, ctx):
    """a vksift_ext_RefinedFundamental record against np_refine_f.refit's"""
    _same_refined(got, want, ctx, "F")
