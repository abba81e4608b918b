"""Writes the input of tests/tools/tiled420_host_check.cpp: the oracle arrays of the 100 x 70 image of tests/test_tiled420_host.py in 52 x 50 tiles, in plane order.
u32 [9] = W, H, tile_w, tile_h, quality, n_y, n_c, F_y, F_c; then streams u16, hist u32 [3 n][10][1024], value_params and width_params f32 [3 n][3][6], coefficients
i32 in plane order. No GPU involved."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from tests import test_tiled420_host as t  # noqa: E402

if __name__ == "__main__":
    quality = 60
    per, (streams, n_y, n_c, hist, vp, wp) = t._inputs(quality)
    coefs = t._coefs_in_plane_order(per)
    head = np.array([t.W, t.H, t.TW, t.TH, quality, n_y, n_c, per[0][0]["coefs"].shape[0], per[0][1]["coefs"].shape[0]], np.uint32)
    with open(sys.argv[1], "wb") as f:
        for a, dt in ((head, np.uint32), (streams, np.uint16), (hist, np.uint32), (vp, np.float32), (wp, np.float32), (coefs, np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())
