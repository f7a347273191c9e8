"""The raw-message decode without a GPU: the numpy restatement (tests/decode_oracle.py) against values written out by hand, and the
host-only vba_scan_layout_check."""
import ctypes as C
import os

import numpy as np
import pytest

import decode_oracle as do


@pytest.fixture(scope="module")
def capi():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


class L:   # a plain stand-in for vba_scan_layout: the restatement needs no library
    def __init__(self, point_step, off_x, off_y, off_z, off_intensity, intensity_type, off_time, time_type, filter):
        self.point_step, self.off_x, self.off_y, self.off_z = point_step, off_x, off_y, off_z
        self.off_intensity, self.intensity_type, self.off_time, self.time_type, self.filter = off_intensity, intensity_type, off_time, time_type, filter


LIVOX = L(20, 4, 8, 12, 16, do.INTENSITY_U8, 0, do.TIME_U32_DIV1E9, 1)
HESAI = L(26, 0, 4, 8, 12, do.INTENSITY_F32, 16, do.TIME_F64_REL_FIRST, 1)
VELODYNE = L(32, 0, 4, 8, 0, do.INTENSITY_NONE, 20, do.TIME_F32, 1)


def _livox7():
    xyz = [(3, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 2), (4, 0, 0), (0.5, 0, 0), (0, 0, 5)]
    #        kept      ON the     tie with   tie with   cut        inside      kept
    #                  sphere     record 3   record 2   (0.12 s)   the sphere
    t = [50_000_000, 10_000_000, 30_000_000, 30_000_000, 120_000_000, 0, 20_000_000]
    refl = [10, 20, 30, 40, 50, 60, 70]
    return do.make_message(LIVOX, xyz, refl, t)


def test_make_message_packs_the_livox_record():
    msg = _livox7()
    assert msg.dtype == np.uint8 and len(msg) == 7 * 20
    r2 = bytes(msg[40:60])
    assert r2[0:4] == np.uint32(30_000_000).tobytes() and r2[4:16] == np.array([0, 2, 0], "<f4").tobytes() and r2[16] == 30


def test_livox_every_record_blind_sphere_tie_and_cut():
    # blind = 1: record 1 has (0 + 1) + 0 = 1.0, not > 1.0, dropped; record 5 is inside; the times 2e7, 3e7, 5e7, 1.2e8 and 1e9 are
    # exact floats, so the one division gives the correctly rounded 0.02, 0.03, 0.05, 0.12; record 4 (0.12 > 0.11) is cut
    d = do.decode(LIVOX, _livox7(), point_filter_num=1, blind2=1.0)
    assert d["n"] == 4
    np.testing.assert_array_equal(d["pnt"], np.array([(0, 0, 5), (0, 2, 0), (0, 0, 2), (3, 0, 0)], np.float32))   # the tie keeps message order
    np.testing.assert_array_equal(d["intensity"], np.array([70, 30, 40, 10], np.float32))
    np.testing.assert_array_equal(d["curvature"], np.array([0.02, 0.03, 0.03, 0.05], np.float32))
    assert d["last_curvature"] == float(np.float32(0.05))


def test_livox_point_filter_num_3():
    d = do.decode(LIVOX, _livox7(), point_filter_num=3, blind2=1.0)   # records 0, 3, 6
    assert d["n"] == 3
    np.testing.assert_array_equal(d["pnt"], np.array([(0, 0, 5), (0, 0, 2), (3, 0, 0)], np.float32))
    np.testing.assert_array_equal(d["intensity"], np.array([70, 40, 10], np.float32))
    np.testing.assert_array_equal(d["curvature"], np.array([0.02, 0.03, 0.05], np.float32))


def test_hesai_record_earlier_than_record_0_sorts_first():
    xyz = [(1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (5, 0, 0)]
    t = np.array([1000.0, 1000.015625, 1000.03125, 1000.0 - 0.0078125, 1000.0625])      # binary fractions: the differences are exact
    msg = do.make_message(HESAI, xyz, [1, 2, 3, 4, 5], t)
    assert len(msg) == 5 * 26
    d = do.decode(HESAI, msg, point_filter_num=1, blind2=0.25)
    assert d["n"] == 5
    np.testing.assert_array_equal(d["pnt"][:, 0], np.array([4, 1, 2, 3, 5], np.float32))
    np.testing.assert_array_equal(d["curvature"], np.array([-0.0078125, 0.0, 0.015625, 0.03125, 0.0625], np.float32))
    np.testing.assert_array_equal(d["intensity"], np.array([4, 1, 2, 3, 5], np.float32))
    assert d["last_curvature"] == 0.0625


def test_empty_message_gives_the_two_points():
    for msg in (np.zeros(0, np.uint8), do.make_message(LIVOX, [(0.1, 0, 0)], [1], [5])):   # nothing at all / nothing kept
        d = do.decode(LIVOX, msg, point_filter_num=1, blind2=1.0)
        assert d["n"] == 2
        np.testing.assert_array_equal(d["pnt"], np.zeros((2, 3), np.float32))
        np.testing.assert_array_equal(d["intensity"], np.zeros(2, np.float32))
        np.testing.assert_array_equal(d["curvature"], np.array([0.0, 0.09], np.float32))
        assert d["last_curvature"] == float(np.float32(0.09))


def test_everything_beyond_the_cut_gives_no_point():
    d = do.decode(LIVOX, do.make_message(LIVOX, [(2, 0, 0), (3, 0, 0)], [1, 2], [120_000_000, 130_000_000]), 1, 1.0)
    assert d["n"] == 0 and d["last_curvature"] == 0.0 and d["pnt"].shape == (0, 3)


def test_velodyne_time_rule():
    xyz = [(2, 0, 0), (3, 0, 0)]
    assert do.decode(VELODYNE, do.make_message(VELODYNE, xyz, None, [0.02, 0.1]), 1, 1.0)["n"] == 2
    for last in (0.5, 0.01, 0.0):
        with pytest.raises(do.Unsupported):
            do.decode(VELODYNE, do.make_message(VELODYNE, xyz, None, [0.02, last]), 1, 1.0)


# ---------------------------------------------------------------- vba_scan_layout_check (host only)

def test_layout_check_accepts_the_shipped_layouts(capi):
    for name in ("livox", "velodyne", "ouster", "hesai", "tartanair"):
        assert capi.scan_layout_check(capi.scan_layout(name)) == capi.OK, name
    lv = capi.scan_layout("livox")
    assert (lv.point_step, lv.off_time, lv.off_x, lv.off_y, lv.off_z, lv.off_intensity) == (20, 0, 4, 8, 12, 16)
    assert (lv.time_type, lv.intensity_type, lv.filter) == (capi.SCAN_TIME_U32_DIV1E9, capi.SCAN_INTENSITY_U8, 1)
    assert capi.scan_layout_check(capi.ScanLayout(1, 0, 0, 0, 0, 0, 0, 0, 1)) == capi.ERR_BAD_ARG     # a float does not fit a 1-byte record
    assert capi.scan_layout_check(capi.ScanLayout(4, 0, 0, 0, -1, 0, -1, 0, 0)) == capi.OK            # offsets of absent fields are not read


def test_layout_check_rejects(capi):
    def bad(**kw):
        l = capi.scan_layout("hesai")
        for k, v in kw.items():
            setattr(l, k, v)
        return capi.scan_layout_check(l)
    assert bad() == capi.OK
    assert bad(off_time=19) == capi.ERR_BAD_ARG          # the f64 would cross point_step (19 + 8 > 26)
    assert bad(off_time=18) == capi.OK
    assert bad(off_z=23) == capi.ERR_BAD_ARG
    assert bad(off_x=-1) == capi.ERR_BAD_ARG
    assert bad(point_step=-26) == capi.ERR_BAD_ARG
    assert bad(point_step=0) == capi.ERR_BAD_ARG
    assert bad(time_type=4) == capi.ERR_BAD_ARG
    assert bad(intensity_type=3) == capi.ERR_BAD_ARG
    assert bad(intensity_type=-1) == capi.ERR_BAD_ARG
    assert bad(filter=2) == capi.ERR_BAD_ARG
    assert capi.load().vba_scan_layout_check(None) == capi.ERR_BAD_ARG


def test_restatement_layout_constants_match_the_binding(capi):
    assert (do.TIME_NONE, do.TIME_F32, do.TIME_U32_DIV1E9, do.TIME_F64_REL_FIRST) == \
        (capi.SCAN_TIME_NONE, capi.SCAN_TIME_F32, capi.SCAN_TIME_U32_DIV1E9, capi.SCAN_TIME_F64_REL_FIRST)
    assert (do.INTENSITY_NONE, do.INTENSITY_F32, do.INTENSITY_U8) == (capi.SCAN_INTENSITY_NONE, capi.SCAN_INTENSITY_F32, capi.SCAN_INTENSITY_U8)
    assert C.sizeof(capi.ScanLayout) == 9 * 4
