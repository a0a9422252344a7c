"""TEST INFRASTRUCTURE (not product code).  Records what the depthwise grid queries of a BUILT
libsegmentron_hip.so answer (seg_dwconv_grid_y, seg_dwconv3x3_s2_grid_y,
seg_dwconv3x3_bwd_fused_add_ok; host code, no device needed) into
tests/golden/dw_grid_queries.npz for tests/test_host_api.py, which replays them against the
library under test.  The fixture pins a refactor of the routing, so it must come from the build of
the commit BEFORE that refactor, never from the code under test:
    SEGMENTRON_HIP_LIB=<parent build>/segmentron_amd/libsegmentron_hip.so \
        python oracle/gen_golden_dw_grid.py
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CS = [4, 8, 12, 16, 24, 32, 36, 64, 72, 96, 128, 144, 256, 260, 728, 1024, 1536, 2048]
SHAPES = [(1, 1, 1), (1, 1, 5), (1, 3, 3), (1, 7, 15), (1, 8, 16), (1, 9, 20), (2, 9, 17),
          (1, 10, 68), (2, 33, 65), (2, 65, 129), (1, 129, 257), (2, 257, 513), (2, 513, 1025),
          (16, 256, 512), (128, 2, 128), (129, 2, 128), (1025, 1, 1)]
STRIDES = [1, 2, 3]
DILS = [1, 2, 3, 6, 12, 18, 24, 36, 64, 65, 100]
KINDS = [0, 1, 2]
SKIPPED = -2  # C is not a multiple of the dtype's channel vector (4 fp32 / 8 bf16): not recorded


def main():
    path = os.environ.get("SEGMENTRON_HIP_LIB")
    if not path:
        sys.exit("set SEGMENTRON_HIP_LIB to the library of the commit the fixture is to pin")
    dll = ctypes.CDLL(path)
    grid = np.full((2, len(CS), len(SHAPES), len(STRIDES), len(DILS), len(KINDS)), SKIPPED, np.int32)
    for dt in (0, 1):  # DT_F32, DT_BF16
        for ci, C in enumerate(CS):
            if C % (8 if dt else 4):
                continue
            for si, (N, H, W) in enumerate(SHAPES):
                for ti, stride in enumerate(STRIDES):
                    for di, dil in enumerate(DILS):
                        for kind in KINDS:
                            grid[dt, ci, si, ti, di, kind] = dll.seg_dwconv_grid_y(
                                dt, C, N, H, W, stride, dil, kind)
    s2 = np.array([[dll.seg_dwconv3x3_s2_grid_y(C, N, H, W) for (N, H, W) in SHAPES] for C in CS],
                  np.int32)
    add_ok = np.array([dll.seg_dwconv3x3_bwd_fused_add_ok(d) for d in (1, 2, 3)], np.int32)
    out = os.path.join(ROOT, "tests", "golden", "dw_grid_queries.npz")
    np.savez_compressed(out, grid_y=grid, s2_grid_y=s2, add_ok=add_ok, C=np.array(CS, np.int32),
                        shapes=np.array(SHAPES, np.int32), strides=np.array(STRIDES, np.int32),
                        dils=np.array(DILS, np.int32), kinds=np.array(KINDS, np.int32))
    rec = grid[grid != SKIPPED]
    print("wrote", out, rec.size, "points, values", rec.min(), "..", rec.max())


if __name__ == "__main__":
    main()
