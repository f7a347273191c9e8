"""numpy restatement of the raw-message decode: Features::process (feature_point.hpp:103-366) + pcl_handler (voxelslam.hpp:77-103).

Every per-point operation is done in the number format the reference uses (np.float32 where it computes in float, np.float64 where
it computes in double); the time sort is ``np.argsort(kind="stable")``, which is the contract of vba_scan_decode (ties keep message
order; the reference's std::sort leaves them undefined).  ``layout`` is any object with the fields of vba_scan_layout."""
import numpy as np

TIME_NONE, TIME_F32, TIME_U32_DIV1E9, TIME_F64_REL_FIRST = range(4)
INTENSITY_NONE, INTENSITY_F32, INTENSITY_U8 = range(3)

_TIME_DTYPE = {TIME_F32: "<f4", TIME_U32_DIV1E9: "<u4", TIME_F64_REL_FIRST: "<f8"}
_INT_DTYPE = {INTENSITY_F32: "<f4", INTENSITY_U8: "u1"}


class Unsupported(Exception):
    """A velodyne message whose last time is outside (0.01, 0.12): the reference's yaw-angle branch (FP:176, FP:200-252)."""


def _put(rec, off, values, dtype):
    a = np.ascontiguousarray(values, dtype=dtype)
    rec[:, off:off + a.dtype.itemsize] = a.view(np.uint8).reshape(len(a), a.dtype.itemsize)


def make_message(layout, xyz, intensity=None, time=None):
    """Packs n records of layout.point_step bytes (uint8 array of n * point_step); bytes no field covers hold a filler pattern."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = len(xyz)
    rec = np.full((n, layout.point_step), 0xA5, dtype=np.uint8)
    _put(rec, layout.off_x, xyz[:, 0], "<f4"); _put(rec, layout.off_y, xyz[:, 1], "<f4"); _put(rec, layout.off_z, xyz[:, 2], "<f4")
    if layout.intensity_type != INTENSITY_NONE:
        _put(rec, layout.off_intensity, intensity, _INT_DTYPE[layout.intensity_type])
    if layout.time_type != TIME_NONE:
        _put(rec, layout.off_time, time, _TIME_DTYPE[layout.time_type])
    return rec.reshape(-1)


def _get(rec, off, dtype):
    size = np.dtype(dtype).itemsize
    return np.frombuffer(np.ascontiguousarray(rec[:, off:off + size]).tobytes(), dtype=dtype)


def decode(layout, raw, point_filter_num=1, blind2=0.0, n_raw=None):
    """Returns dict(pnt float32 [n][3], intensity float32 [n], curvature float32 [n], n, last_curvature (float, 0 when n == 0))."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8) if not isinstance(raw, np.ndarray) else raw
    step = layout.point_step
    if n_raw is None:
        n_raw = len(raw) // step
    rec = raw[:n_raw * step].reshape(n_raw, step)
    x = _get(rec, layout.off_x, "<f4"); y = _get(rec, layout.off_y, "<f4"); z = _get(rec, layout.off_z, "<f4")
    if layout.intensity_type == INTENSITY_NONE:
        inten = np.zeros(n_raw, dtype=np.float32)
    else:
        inten = _get(rec, layout.off_intensity, _INT_DTYPE[layout.intensity_type]).astype(np.float32)
    if layout.time_type == TIME_NONE:
        curv = np.zeros(n_raw, dtype=np.float32)
    elif layout.time_type == TIME_F32:
        curv = _get(rec, layout.off_time, "<f4").copy()
        if n_raw > 0 and not (np.float64(curv[-1]) > 0.01 and np.float64(curv[-1]) < 0.12):      # FP:176
            raise Unsupported()
    elif layout.time_type == TIME_U32_DIV1E9:
        curv = _get(rec, layout.off_time, "<u4").astype(np.float32) / np.float32(1e9)            # FP:155, FP:271: one float division
    else:
        t = _get(rec, layout.off_time, "<f8")
        curv = (t - t[0]).astype(np.float32) if n_raw > 0 else np.zeros(0, dtype=np.float32)     # FP:304, FP:335
    assert x.dtype == np.float32 and curv.dtype == np.float32
    if layout.filter:
        r2 = (x * x + y * y) + z * z                                                             # float, FP:159
        assert r2.dtype == np.float32
        keep = (np.arange(n_raw) % point_filter_num == 0) & (r2.astype(np.float64) > blind2)
    else:
        keep = np.ones(n_raw, dtype=bool)
    pnt = np.stack([x, y, z], axis=1)[keep]; inten = inten[keep]; curv = curv[keep]
    if len(curv) == 0:                                                                           # VH:82-90
        pnt = np.zeros((2, 3), dtype=np.float32); inten = np.zeros(2, dtype=np.float32); curv = np.array([0.0, 0.09], dtype=np.float32)
    order = np.argsort(curv, kind="stable")                                                      # VH:92-95
    pnt, inten, curv = pnt[order], inten[order], curv[order]
    n = len(curv)
    while n > 0 and np.float64(curv[n - 1]) > 0.11:                                              # VH:96-97 (n = 0: see vba_scan_decode)
        n -= 1
    return dict(pnt=pnt[:n].astype(np.float32), intensity=inten[:n].astype(np.float32), curvature=curv[:n].astype(np.float32), n=n,
                last_curvature=float(curv[n - 1]) if n > 0 else 0.0)
