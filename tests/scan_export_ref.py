"""The published scan of pub_localtraj (voxelslam.cpp:37-45) as vba_odom_state_export_scan states it (include/voxelba.h, DESIGN.md
section 22), restated in numpy: world = x.R p + x.p in the order ((R[r][0] x + R[r][1] y) + R[r][2] z) + t[r], every product and sum a
float64 operation of its own (numpy fuses nothing), each coordinate narrowed to float32 once.  tests/test_scan_export_cpu.py pins this
restatement to exact arithmetic; tests/test_gpu_kd_on_state.py holds the device to it bit for bit."""
import numpy as np


def export_restated(state25, pts, intensity=0.0):
    """state25 [25] = t, R (9, row-major), p (3), ...; pts [n][3] float64 -> float32 [n][4] records x y z intensity"""
    state25 = np.asarray(state25, dtype=np.float64)
    R = state25[1:10].reshape(3, 3); t = state25[10:13]
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty((len(pts), 4), dtype=np.float32)
    for r in range(3):
        out[:, r] = (((R[r, 0] * x + R[r, 1] * y) + R[r, 2] * z) + t[r]).astype(np.float32)
    out[:, 3] = np.float32(intensity)
    return out


def checksum(xyzi):
    """the sum of the float bits of the records as integers (the harness prints the same sum)"""
    return int(np.ascontiguousarray(xyzi, dtype=np.float32).view(np.uint32).astype(np.uint64).sum())
