#!/usr/bin/env python3
"""The describe table of tests/api_model.py, recorded on an MI355X: for every profile the records and the placed-keypoint count that a describe
call on a fresh, quiet instance of the profile's configuration returns for every entry of api_model.DESCRIBE.

    python tests/golden/make_api_model_describe.py          (needs the GPU; writes tests/golden/api_model_describe.npz)

tests/test_api_model.py generates its walks from this table on the CPU; tests/test_gpu_api_model.py holds the table to what the instance returns
before it walks, so a stale recording fails there."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import api_model as A                      # noqa: E402
import test_gpu_api_model as T             # noqa: E402
from oracle import oracle as O             # noqa: E402
from vulkansift_amd import api as vk       # noqa: E402

if __name__ == "__main__":
    O.build()
    vk.lib().vksift_setLogLevel(vk.VKSIFT_NO_LOG)
    out = {}
    for profile, p in A.PROFILES.items():
        os.environ.update(p["env"])
        w = T.world(vk, O, profile)
        for d, (recs, placed) in enumerate(w.desc):
            out[f"{profile}_{d}_records"] = recs.view(np.uint8).reshape(-1, 164)
            out[f"{profile}_{d}_placed"] = np.int64(placed)
            print(f"{profile} entry {d}: {len(w.kps[d])} keypoints, {len(recs)} records, {placed} placed")
        for k in p["env"]:
            del os.environ[k]
    np.savez_compressed(A.GOLDEN, **out)
    print(A.GOLDEN, os.path.getsize(A.GOLDEN), "bytes")
