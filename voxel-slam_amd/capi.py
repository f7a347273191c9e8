"""ctypes binding of libvoxelba.so (include/voxelba.h) plus thin Python mirrors of the reference classes
``LidarFactor`` / ``Lidar_BA_Optimizer`` / ``LI_BA_Optimizer`` / ``LI_BA_OptimizerGravity`` (voxel_map.hpp:124-976)
and of the voxel-map entry points (``cut_voxel`` / ``multi_recut`` / ``multi_margi``).

The product has no CPU path: ``load()`` raises if the shared library is missing, ``Context()`` raises if no
HIP device is present.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from .abi import KINDS, PROTOTYPES

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VBA_LIB") or os.path.join(_PKG, "libvoxelba.so")   # VBA_LIB: an alternative build (tools/ A/B runs)
_dp = C.POINTER(C.c_double)

OK = 0
ERR_NO_DEVICE, ERR_BAD_ARG, ERR_UNSUPPORTED_WINDOW, ERR_TOO_FEW_VOXELS, ERR_OPT_STATE, ERR_HIP, ERR_CAPACITY, ERR_IO, ERR_UNSUPPORTED, ERR_SINGULAR = range(1, 11)

EXPORTS = list(PROTOTYPES)     # every function of include/voxelba.h, in the header's order


class Options(C.Structure):
    _fields_ = [
        ("win_size", C.c_int), ("voxel_size", C.c_double), ("max_layer", C.c_int), ("max_points", C.c_int),
        ("min_eigen_value", C.c_double), ("plane_eigen_value_thre", C.c_double * 4), ("min_point", C.c_double * 4),
        ("imu_coef", C.c_double), ("thread_num", C.c_int), ("device", C.c_int), ("stream", C.c_void_p),
        ("max_voxels", C.c_size_t), ("max_points_per_scan", C.c_size_t),
        ("lm_spec", C.c_int), ("force_collective", C.c_int), ("hessian_workgroups", C.c_int), ("residual_vpl_from", C.c_int), ("hessian_compact_tiles", C.c_int),
        ("lm_trial_launches", C.c_int),      # (in what was padding in front of max_map_nodes: every other offset is unchanged)
        ("max_map_nodes", C.c_size_t), ("max_fix_points", C.c_size_t), ("hba_workers", C.c_int),
        ("deterministic", C.c_int),
    ]


class BtcConfig(C.Structure):
    """vba_btc_config: the retrieval fields of ConfigSetting (BTC.h:22-57), with the reference's float types."""
    _fields_ = [
        ("skip_near_num", C.c_int), ("candidate_num", C.c_int), ("rough_dis_threshold", C.c_float),
        ("similarity_threshold", C.c_float), ("icp_threshold", C.c_float), ("normal_threshold", C.c_float),
        ("dis_threshold", C.c_float), ("occupy_len", C.c_int),
    ]


class BtcResult(C.Structure):
    _fields_ = [("loop_id", C.c_int), ("score", C.c_double), ("t", C.c_double * 3), ("R", C.c_double * 9)]


class BtcIcpState(C.Structure):
    """vba_btc_icp_state: the state of one icp_normal iteration"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("paras", C.c_double * 4), ("is_conv", C.c_int), ("done", C.c_int),
                ("iters", C.c_int), ("pad", C.c_int), ("mat", C.c_double * 6), ("eig", C.c_double * 3)]

    @classmethod
    def start(cls, t, R, paras=(0.2, 0.2, 0.5, 3.0), is_conv=0, done=0, iters=0):
        """the state vba_btc_icp_normal starts from (loop_refine.hpp:62-63), or a caller's"""
        s = cls()
        s.R[:] = [float(x) for x in np.reshape(R, 9)]; s.t[:] = [float(x) for x in np.reshape(t, 3)]
        s.paras[:] = [float(x) for x in paras]
        s.is_conv, s.done, s.iters = int(is_conv), int(done), int(iters)
        return s


class BtcCandidate(C.Structure):
    _fields_ = [("frame", C.c_int), ("votes", C.c_int), ("match_len", C.c_int), ("max_vote_index", C.c_int),
                ("max_vote", C.c_int), ("score", C.c_double)]


BTC_ROW_LEN = 19


class BtcGenConfig(C.Structure):
    """vba_btc_gen_config: the ConfigSetting fields (BTC.h:22-46) GenerateSTDescs reads, with the reference's float types."""
    _fields_ = [
        ("useful_corner_num", C.c_int), ("plane_merge_normal_thre", C.c_float), ("plane_merge_dis_thre", C.c_float),
        ("plane_detection_thre", C.c_float), ("voxel_size", C.c_float), ("voxel_init_num", C.c_int), ("proj_plane_num", C.c_int),
        ("proj_image_resolution", C.c_float), ("proj_image_high_inc", C.c_float), ("proj_dis_min", C.c_float),
        ("proj_dis_max", C.c_float), ("summary_min_thre", C.c_float), ("line_filter_enable", C.c_int),
        ("touch_filter_enable", C.c_int), ("descriptor_near_num", C.c_float), ("descriptor_min_len", C.c_float),
        ("descriptor_max_len", C.c_float), ("non_max_suppression_radius", C.c_float), ("std_side_resolution", C.c_float),
    ]


def btc_default_gen_config(is_high_fly=0) -> BtcGenConfig:
    """read_parameters (BTC.cpp:3-68), generation fields."""
    f = BtcGenConfig()
    st = load().vba_btc_default_gen_config(int(is_high_fly), C.byref(f))
    if st:
        raise VbaError(st)
    return f


def btc_max_stds(gcfg) -> int:
    """useful_corner_num * C(K - 1, 2), K = (int)descriptor_near_num: the row capacity generate_stds needs"""
    k1 = int(gcfg.descriptor_near_num) - 1
    return int(gcfg.useful_corner_num) * (k1 * (k1 - 1) // 2)


def btc_default_config(is_high_fly=0) -> BtcConfig:
    """read_parameters (BTC.cpp:3-68), retrieval fields only."""
    f = BtcConfig()
    st = load().vba_btc_default_config(int(is_high_fly), C.byref(f))
    if st:
        raise VbaError(st)
    return f


def _btc_query(rows, bits):
    rows = np.ascontiguousarray(np.reshape(rows, (-1, BTC_ROW_LEN)), dtype=np.float64)
    bits = np.ascontiguousarray(np.reshape(bits, (-1, 3)), dtype=np.uint64)
    if len(rows) != len(bits):
        raise ValueError("rows and bits differ in length")
    return rows, bits, bits.ctypes.data_as(C.POINTER(C.c_uint64))


def _btc_result(r):
    return dict(loop_id=r.loop_id, score=r.score, t=np.array(r.t[:]), R=np.array(r.R[:]).reshape(3, 3))


class BtcDb:
    """One vba_btc_db: the database half of STDescManager (descriptors + plane clouds) on a context."""

    def __init__(self, ctx, config):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(self.lib.vba_btc_create(ctx.h, C.byref(config), C.byref(h)))
        self.h = h
        ctx._btc.append(self)

    def close(self):
        if getattr(self, "h", None):
            self.lib.vba_btc_destroy(self.h)
            self.h = None
        btc = getattr(self.ctx, "_btc", None)
        if btc is not None and self in btc:
            btc.remove(self)

    def reserve(self, stds=0, frames=0, cloud_points=0, matches=0):
        """capacity hint: a database sized for these never re-allocates (results do not depend on it)"""
        self.ctx._chk(self.lib.vba_btc_reserve(self.h, stds, frames, cloud_points, matches))

    def set_skip_near_num(self, v):
        self.ctx._chk(self.lib.vba_btc_set_skip_near_num(self.h, int(v)))

    def push_plane_cloud(self, xyz_normal, seq):
        a = np.ascontiguousarray(np.reshape(xyz_normal, (-1, 6)), dtype=np.float32)
        self.ctx._chk(self.lib.vba_btc_push_plane_cloud(self.h, len(a), a.ctypes.data_as(C.POINTER(C.c_float)), int(seq)))

    def num_frames(self):
        return self.lib.vba_btc_num_frames(self.h)

    def frame_seq(self, frame):
        s = C.c_int()
        self.ctx._chk(self.lib.vba_btc_frame_seq(self.h, frame, C.byref(s)))
        return s.value

    def add_stds(self, rows, bits):
        rows, bits, bp = _btc_query(rows, bits)
        self.ctx._chk(self.lib.vba_btc_add_stds(self.h, len(rows), _p(rows), bp))

    def search_loop(self, rows, bits, cur_db, cur_frame=-1):
        """SearchLoop against this database; pl_cur = plane cloud cur_frame of cur_db (-1: its last)."""
        rows, bits, bp = _btc_query(rows, bits)
        if cur_frame < 0:
            cur_frame = cur_db.num_frames() + cur_frame
        r = BtcResult()
        self.ctx._chk(self.lib.vba_btc_search_loop(self.h, len(rows), _p(rows), bp, cur_db.h, cur_frame, C.byref(r)))
        return _btc_result(r)

    def last_candidates(self):
        """list of dicts (frame, votes, match_len, max_vote_index, max_vote, score) of the last search"""
        n = C.c_int()
        out = (BtcCandidate * 256)()
        self.ctx._chk(self.lib.vba_btc_last_candidates(self.h, 256, out, C.byref(n)))
        return [dict(frame=o.frame, votes=o.votes, match_len=o.match_len, max_vote_index=o.max_vote_index, max_vote=o.max_vote,
                     score=o.score) for o in out[:n.value]]

    def set_gen_config(self, gcfg):
        self.ctx._chk(self.lib.vba_btc_set_gen_config(self.h, C.byref(gcfg)))
        self.gcfg = gcfg

    def gen_reserve(self, points=0, cells=0, frames=1):
        """capacity hint for generate_stds: clouds of `points` points, projection images of `cells` cells, `frames` more calls"""
        self.ctx._chk(self.lib.vba_btc_gen_reserve(self.h, points, cells, frames))

    def gen_allocations(self):
        n = C.c_int(); b = C.c_int64()
        self.ctx._chk(self.lib.vba_btc_gen_allocations(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def generate_stds(self, xyz, id, cap=None):
        """GenerateSTDescs(cloud, stds, id): pushes the plane cloud (seq = id); returns (rows [n][19], bits [n][3])"""
        a = np.ascontiguousarray(np.reshape(xyz, (-1, 3)), dtype=np.float32)
        if cap is None:
            cap = btc_max_stds(getattr(self, "gcfg", None) or btc_default_gen_config(0))
        rows = np.zeros((max(cap, 1), BTC_ROW_LEN)); bits = np.zeros((max(cap, 1), 3), dtype=np.uint64)
        n = C.c_int()
        self.ctx._chk(self.lib.vba_btc_generate_stds(self.h, len(a), a.ctypes.data_as(C.POINTER(C.c_float)), int(id),
                                                     cap, _p(rows), bits.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        return rows[:n.value].copy(), bits[:n.value].copy()

    def plane_cloud(self, frame):
        n = C.c_int()
        self.ctx._chk(self.lib.vba_btc_plane_cloud(self.h, frame, 0, None, C.byref(n)))
        out = np.zeros((max(n.value, 1), 6), dtype=np.float32)
        self.ctx._chk(self.lib.vba_btc_plane_cloud(self.h, frame, n.value, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        return out[:n.value].copy()

    def last_corners(self):
        """binary_list of the last generate_stds: (locations [n][3], summaries [n], masks [n])"""
        n = C.c_int()
        self.ctx._chk(self.lib.vba_btc_last_corners(self.h, 0, None, None, C.byref(n)))
        ls = np.zeros((max(n.value, 1), 4)); b = np.zeros(max(n.value, 1), dtype=np.uint64)
        self.ctx._chk(self.lib.vba_btc_last_corners(self.h, n.value, _p(ls), b.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        k = n.value
        return ls[:k, :3].copy(), ls[:k, 3].astype(np.int64), b[:k].copy()

    def icp_normal(self, src_frame, tar_db, tar_frame, t, R, icp_eigval):
        """icp_normal(plane cloud src_frame of this db, plane cloud tar_frame of tar_db, (t, R), icp_eigval)"""
        tt = _c(t).copy(); RR = _c(R).reshape(3, 3).copy()
        ok = C.c_int(); it = C.c_int(); eig = np.zeros(3)
        self.ctx._chk(self.lib.vba_btc_icp_normal(self.h, src_frame, tar_db.h, tar_frame, _p(tt), _p(RR),
                                                  icp_eigval, C.byref(ok), _p(eig), C.byref(it)))
        return dict(ok=ok.value, t=tt, R=RR, eig=eig, iters=it.value)

    def debug_icp_pass(self, src_frame, tar_db, tar_frame, state, ns, slices=0, prefill=None):
        """vba_debug_btc_icp_pass: ONE iteration of icp_normal from `state` (a BtcIcpState, left as given); ns = points of the source
        cloud.  Returns dict(state (the state after the step), key [ns] uint64, gate [ns] uint8, partial [nb][35], sums [35], dx [6],
        slices).  prefill: the value the float outputs hold before the call (NaN), to see what a call leaves untouched."""
        nb = max((ns + 255) // 256, 1)
        fill = np.nan if prefill is None else prefill
        st = BtcIcpState.from_buffer_copy(state)
        key = np.zeros(max(ns, 1), dtype=np.uint64); gate = np.full(max(ns, 1), 255, dtype=np.uint8)
        partial = np.full((nb, 35), fill); sums = np.full(35, fill); dx = np.full(6, fill); used = C.c_int(-1)
        self.ctx._chk(self.lib.vba_debug_btc_icp_pass(self.h, src_frame, tar_db.h, tar_frame, C.byref(st), slices,
                                                      key.ctypes.data_as(C.c_void_p), gate.ctypes.data_as(C.c_void_p), _p(partial),
                                                      _p(sums), _p(dx), C.byref(used)))
        return dict(state=st, key=key[:ns], gate=gate[:ns], partial=partial, sums=sums, dx=dx, slices=used.value)


class _Handle:
    """What the device-resident objects of a context share: PREFIX_create on the context, a place in the context's ``_kf`` list
    (Context.close() destroys those first, then the databases, then itself), PREFIX_destroy and PREFIX_allocations.  (BtcDb is not
    one of them: its create call takes a config and it has gen_allocations, not allocations.)"""
    PREFIX = None

    def __init__(self, ctx):
        self.ctx = ctx
        self.lib = ctx.lib
        h = C.c_void_p()
        ctx._chk(getattr(self.lib, self.PREFIX + "_create")(ctx.h, C.byref(h)))
        self.h = h
        ctx._kf.append(self)

    def close(self):
        if getattr(self, "h", None):
            getattr(self.lib, self.PREFIX + "_destroy")(self.h)
            self.h = None
        kf = getattr(self.ctx, "_kf", None)
        if kf is not None and self in kf:
            kf.remove(self)

    def allocations(self):
        n = C.c_int(); b = C.c_int64()
        self.ctx._chk(getattr(self.lib, self.PREFIX + "_allocations")(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value


def _dump_rows(fn, h, width):
    """The "ask for the size, then fill" leaf dumps: fn(h, NULL, 0) returns the leaf count, fn(h, out, n) fills out [n][width]."""
    n = fn(h, None, 0)
    out = np.zeros((max(n, 0), width))
    if n > 0:
        fn(h, _p(out), n)
    return out


class KeyframeStore(_Handle):
    """One vba_kf_store: the session's keyframes (``vector<Keyframe*> *keyframes``) resident in HBM."""
    PREFIX = "vba_kf"

    def reserve(self, points=0, keyframes=0, merge_points=0):
        self.ctx._chk(self.lib.vba_kf_reserve(self.h, points, keyframes, merge_points))

    def size(self):
        return self.lib.vba_kf_size(self.h)

    def build(self, scans, poses, voxel_size, id, jour=0.0, vars=None, db=None, cap=None, offsets=None):
        """The keyframe of VS:2354-2397 from ``scans`` (list of [n_i][3], or one [N][3] array with ``offsets``), ``vars`` the
        matching [n_i][9] covariances or None (the offline form), ``poses`` [k][12]; with ``db`` the descriptors of the merged cloud
        are generated too.  Returns (kept points, rows, bits); rows / bits are None without a database."""
        if offsets is None:
            off, pnt = Context._ragged(scans)
            var = np.ascontiguousarray(np.concatenate([np.reshape(v, (-1, 9)) for v in vars]), dtype=np.float64) if vars is not None else None
        else:
            off = np.ascontiguousarray(offsets, dtype=np.int32); pnt = _c(scans)
            var = _c(vars) if vars is not None else None
        poses = _c(poses).reshape(-1, 12)
        k = len(off) - 1
        if len(poses) != k:
            raise ValueError("one pose per scan")
        rows = bits = None; ns = C.c_int(); npt = C.c_int()
        if db is not None:
            if cap is None:
                cap = btc_max_stds(getattr(db, "gcfg", None) or btc_default_gen_config(0))
            rows = np.zeros((max(cap, 1), BTC_ROW_LEN)); bits = np.zeros((max(cap, 1), 3), dtype=np.uint64)
        self.ctx._chk(self.lib.vba_kf_build(self.h, k, off.ctypes.data_as(C.POINTER(C.c_int)), _p(pnt), _p(var), _p(poses),
                                            voxel_size, int(id), jour, db.h if db is not None else None,
                                            cap if db is not None else 0, _p(rows),
                                            bits.ctypes.data_as(C.POINTER(C.c_uint64)) if bits is not None else None, C.byref(ns), C.byref(npt)))
        if db is None:
            return npt.value, None, None
        return npt.value, rows[:ns.value].copy(), bits[:ns.value].copy()

    def build_from_log(self, log, first, poses, voxel_size, id, jour=0.0, db=None, cap=None):
        """``build`` with covariances from scans first .. first + len(poses) - 1 of the ScanLog ``log``, read in place."""
        poses = _c(poses).reshape(-1, 12)
        rows = bits = None; ns = C.c_int(); npt = C.c_int()
        if db is not None:
            if cap is None:
                cap = btc_max_stds(getattr(db, "gcfg", None) or btc_default_gen_config(0))
            rows = np.zeros((max(cap, 1), BTC_ROW_LEN)); bits = np.zeros((max(cap, 1), 3), dtype=np.uint64)
        self.ctx._chk(self.lib.vba_kf_build_from_log(self.h, log.h, first, len(poses), _p(poses), voxel_size,
                                                     int(id), jour, db.h if db is not None else None,
                                                     cap if db is not None else 0, _p(rows),
                                                     bits.ctypes.data_as(C.POINTER(C.c_uint64)) if bits is not None else None, C.byref(ns), C.byref(npt)))
        if db is None:
            return npt.value, None, None
        return npt.value, rows[:ns.value].copy(), bits[:ns.value].copy()

    def last_counts(self):
        n = C.c_int()
        self.ctx._chk(self.lib.vba_kf_last_counts(self.h, 0, None, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        self.ctx._chk(self.lib.vba_kf_last_counts(self.h, n.value, out.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n)))
        return out[:n.value].copy()

    def generate_stds(self, first, count, db, cap=None):
        """descriptors of keyframes [first, first + count) merged into the last one's frame (VS:384-409) -> (rows, bits)"""
        if cap is None:
            cap = btc_max_stds(getattr(db, "gcfg", None) or btc_default_gen_config(0))
        rows = np.zeros((max(cap, 1), BTC_ROW_LEN)); bits = np.zeros((max(cap, 1), 3), dtype=np.uint64); n = C.c_int()
        self.ctx._chk(self.lib.vba_kf_generate_stds(self.h, first, count, db.h, cap, _p(rows),
                                                    bits.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(n)))
        return rows[:n.value].copy(), bits[:n.value].copy()

    def set_poses(self, first, poses):
        poses = _c(poses).reshape(-1, 12)
        self.ctx._chk(self.lib.vba_kf_set_poses(self.h, first, len(poses), _p(poses)))

    def get(self, k):
        pose = np.zeros(12); i = C.c_int(); j = C.c_double(); e = C.c_int(); n = C.c_int()
        self.ctx._chk(self.lib.vba_kf_get(self.h, k, _p(pose), C.byref(i), C.byref(j), C.byref(e), C.byref(n)))
        return dict(x0=pose, id=i.value, jour=j.value, exist=e.value, n_points=n.value)

    def set_history(self, n_hist):
        self.ctx._chk(self.lib.vba_kf_set_history(self.h, n_hist))

    def history_size(self):
        return self.lib.vba_kf_history_size(self.h)

    def load(self, k, map_ctx, jour=0.0):
        self.ctx._chk(self.lib.vba_kf_load(self.h, k, map_ctx.h, jour))

    def load_nearby(self, map_ctx, p3, radius=10.0, jour=0.0):
        """keyframe_loading(jour) around p3 -> index of the loaded keyframe, -1 = none"""
        k = C.c_int(-1)
        self.ctx._chk(self.lib.vba_kf_load_nearby(self.h, map_ctx.h, _p(_c(p3)), radius, jour, C.byref(k)))
        return k.value

    def read(self, k):
        """keyframe k -> (xyz [n][3] float values in doubles, covariance diagonals float32 [n][3])"""
        n = C.c_int()
        self.ctx._chk(self.lib.vba_kf_read(self.h, k, 0, None, None, C.byref(n)))
        xyz = np.zeros((max(n.value, 1), 3)); vd = np.zeros((max(n.value, 1), 3), dtype=np.float32)
        self.ctx._chk(self.lib.vba_kf_read(self.h, k, n.value, _p(xyz), vd.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        return xyz[:n.value].copy(), vd[:n.value].copy()

    def hba_add_edge(self, ctx, first, count, poses, gba_voxel_size, gba_min_eigen_value, gba_eig, max_iter, thread_num):
        """vba_hba_add_edge on ``ctx`` over keyframes [first, first + count) read in place from the store (no upload of the clouds);
        poses [count][12] are the poses to optimise (the reference passes the keyframes' x0).  Result as Context.hba_add_edge."""
        d, off, _ = self.clouds()
        rel = np.ascontiguousarray(off[first:first + count + 1] - off[first], dtype=np.int32)
        base = C.c_void_p(d + 24 * int(off[first]))
        poses = _c(poses).reshape(count, 12).copy()
        npt = int(rel[-1])
        edges = np.zeros((count * (count - 1) // 2 + 1, 20)); ne = C.c_int(0)
        cloud = np.zeros((max(npt, 1), 3)); ccnt = np.zeros(max(npt, 1), dtype=np.int32); nc = C.c_int(0)
        rl = np.zeros((max_iter + 1, 2)); nl = C.c_int(0)
        ctx._chk(self.lib.vba_hba_add_edge(ctx.h, count, rel.ctypes.data_as(C.POINTER(C.c_int)), base, _p(poses),
                                           gba_voxel_size, gba_min_eigen_value, _p(_c(gba_eig)), max_iter,
                                           thread_num, _p(edges), C.byref(ne), _p(cloud), ccnt.ctypes.data_as(C.POINTER(C.c_int)),
                                           C.byref(nc), _p(rl), C.byref(nl)))
        return dict(poses=poses, edges=edges[:ne.value].copy(), cloud=cloud[:nc.value].copy(), cloud_count=ccnt[:nc.value].copy(),
                    resis=rl[:nl.value].copy())

    def clouds(self):
        """(device address of the point array, host offsets [n_kf + 1] (a copy), n_kf): the arguments of vba_hba_*"""
        d = C.c_void_p(); o = C.POINTER(C.c_int)(); n = C.c_int()
        self.ctx._chk(self.lib.vba_kf_clouds(self.h, C.byref(d), C.byref(o), C.byref(n)))
        off = np.array([o[i] for i in range(n.value + 1)], dtype=np.int32)
        return (d.value or 0), off, n.value

    def sizes(self):
        """point count of every keyframe (int32 [n_kf]): the ``sizes`` of kf_export_plan"""
        return np.diff(self.clouds()[1]).astype(np.int32)


class LoopMap(_Handle):
    """One vba_loop_map: ``map_loop`` of the loop-closure thread, a second voxel map resident in HBM."""
    PREFIX = "vba_loop_map"

    def reserve(self, fix_points=0, nodes=0):
        self.ctx._chk(self.lib.vba_loop_map_reserve(self.h, fix_points, nodes))

    def build(self, store, init_num=5, cumulative=True):
        """VS:2601-2625 from the last ``init_num`` keyframes of ``store`` at their current x0 -> points inserted.
        cumulative=True is the reference (pvec_tem is never cleared), False inserts every keyframe once."""
        n = C.c_int()
        self.ctx._chk(self.lib.vba_loop_map_build(self.h, store.h, init_num, int(cumulative), C.byref(n)))
        return n.value

    def num_roots(self):
        return self.lib.vba_loop_map_num_roots(self.h)

    def dump_leaves(self):
        return _dump_rows(self.lib.vba_loop_map_dump_leaves, self.h, 39)

    def dump_plane_var(self):
        return _dump_rows(self.lib.vba_loop_map_dump_plane_var, self.h, 86)


class SurfelRegParams(C.Structure):
    _fields_ = [("gate", C.c_double), ("neighbors", C.c_int), ("max_iter", C.c_int), ("min_matches", C.c_int),
                ("eps_rot", C.c_double), ("eps_tra", C.c_double)]


class SurfelRegReport(C.Structure):
    _fields_ = [("iters", C.c_int), ("converged", C.c_int), ("lost", C.c_int), ("singular", C.c_int), ("matches", C.c_int * 32),
                ("cost", C.c_double * 32), ("step_rot", C.c_double * 32), ("step_tra", C.c_double * 32),
                ("H", C.c_double * 21), ("g", C.c_double * 6), ("eig_tt", C.c_double * 3)]


def surfel_reg_default_params(**kw) -> SurfelRegParams:
    p = SurfelRegParams()
    load().vba_surfel_reg_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class SurfelMap(_Handle):
    """One vba_surfel_map: the cells of a surfel export in HBM and the registration of a scan against them.
    Arrays are numpy arrays (host) or integer device addresses."""
    PREFIX = "vba_surfel_map"

    def reserve(self, max_cells=0, max_points=0):
        self.ctx._chk(self.lib.vba_surfel_map_reserve(self.h, int(max_cells), int(max_points)))

    def build(self, surfels, cov, voxel_size, sigma=0.02, min_count=5, n=None):
        """from records float32 [n][12] and cov float64 [n][6] (numpy arrays, or two device addresses with ``n``) -> cells"""
        nc = C.c_int64(-1)
        if isinstance(surfels, (int, C.c_void_p)):
            args = (int(n), surfels, cov)
        else:
            rec = np.ascontiguousarray(surfels, dtype=np.float32).reshape(-1, 12); cv = _c(cov).reshape(-1, 6)
            if len(rec) != len(cv):
                raise ValueError("one covariance per record")
            args = (len(rec), rec.ctypes.data_as(C.c_void_p), _p(cv))
        self.ctx._chk(self.lib.vba_surfel_map_build(self.h, *args, float(voxel_size), float(sigma), int(min_count), C.byref(nc)))
        return nc.value

    def build_from_kf(self, stores, jump, voxel_size, sigma=0.02, min_count=5):
        hs = (C.c_void_p * len(stores))(*[s.h for s in stores])
        nc = C.c_int64(-1)
        self.ctx._chk(self.lib.vba_surfel_map_build_from_kf(self.h, len(stores), hs, int(jump), float(voxel_size), float(sigma), int(min_count),
                                                            C.byref(nc)))
        return nc.value

    def size(self):
        """(cells, voxel_size, sigma) of the map as built"""
        nc = C.c_int64(); v = C.c_double(); s = C.c_double()
        self.ctx._chk(self.lib.vba_surfel_map_size(self.h, C.byref(nc), C.byref(v), C.byref(s)))
        return nc.value, v.value, s.value

    def read(self):
        """vba_debug_surfel_map_read -> dict(slots, slot int64 [m], key uint64 [m], row int32 [m], c float32 [m][4], W [m][6]) in
        slot order"""
        n = C.c_int64(); ns = C.c_int64()
        self.ctx._chk(self.lib.vba_debug_surfel_map_read(self.h, 0, None, None, None, None, None, C.byref(n), C.byref(ns)))
        m = max(n.value, 1)
        slot = np.zeros(m, np.int64); key = np.zeros(m, np.uint64); row = np.zeros(m, np.int32); c4 = np.zeros((m, 4), np.float32); W = np.zeros((m, 6))
        self.ctx._chk(self.lib.vba_debug_surfel_map_read(self.h, m, slot.ctypes.data_as(C.c_void_p), key.ctypes.data_as(C.c_void_p),
                                                         row.ctypes.data_as(C.c_void_p), c4.ctypes.data_as(C.c_void_p), _p(W), C.byref(n), C.byref(ns)))
        k = n.value
        return dict(slots=ns.value, slot=slot[:k], key=key[:k], row=row[:k], c=c4[:k], W=W[:k])

    @staticmethod
    def _pnt(pnt, n):
        if isinstance(pnt, (int, C.c_void_p)):
            return int(n), pnt, None
        a = _c(pnt).reshape(-1, 3)
        return len(a), _p(a), a

    def register(self, pnt, R, t, params=None, n=None):
        """vba_surfel_register from the pose (R [3][3], t [3]) -> (R, t, SurfelRegReport); ``pnt`` [n][3] host array, or a device
        address with ``n``"""
        p = params if params is not None else surfel_reg_default_params()
        n, ptr, keep = self._pnt(pnt, n)
        R = _c(R).reshape(9).copy(); t = _c(t).reshape(3).copy(); rep = SurfelRegReport()
        self.ctx._chk(self.lib.vba_surfel_register(self.h, n, ptr, C.byref(p), _p(R), _p(t), C.byref(rep)))
        return R.reshape(3, 3), t, rep

    def debug_pass(self, pnt, R, t, params=None, n=None):
        """vba_debug_surfel_reg_pass: one iteration -> dict(R, t, cell int32 [n], gate uint8 [n], sums [29], dx [6])"""
        p = params if params is not None else surfel_reg_default_params()
        n, ptr, keep = self._pnt(pnt, n)
        R = _c(R).reshape(9).copy(); t = _c(t).reshape(3).copy()
        cell = np.full(n, -7, dtype=np.int32); gate = np.full(n, 7, dtype=np.uint8); sums = np.full(29, np.nan); dx = np.full(6, np.nan)
        self.ctx._chk(self.lib.vba_debug_surfel_reg_pass(self.h, n, ptr, C.byref(p), _p(R), _p(t), cell.ctypes.data_as(C.c_void_p),
                                                         gate.ctypes.data_as(C.c_void_p), _p(sums), _p(dx)))
        return dict(R=R.reshape(3, 3), t=t, cell=cell, gate=gate, sums=sums, dx=dx)


class ScanLog(_Handle):
    """One vba_scanlog: the marginalised scans of a session (the live ``ScanPose::pvec``) resident in HBM, between the map's scan
    ring and the keyframes.  Scans are numbered 0, 1, 2, ... in push order and released first in, first out."""
    PREFIX = "vba_scanlog"

    def reserve(self, points=0, scans=0):
        self.ctx._chk(self.lib.vba_scanlog_reserve(self.h, points, scans))

    def push_window(self, frame):
        """capture frame ``frame`` of the context's window from the map's scan ring (before margi) -> the scan's number"""
        seq = C.c_int64(-1)
        self.ctx._chk(self.lib.vba_scanlog_push_window(self.h, frame, C.byref(seq)))
        return seq.value

    def push_points(self, pnt, var=None):
        """push a host scan pnt [n][3] with var [n][9] (None: zeros) -> the scan's number"""
        pnt = _c(pnt).reshape(-1, 3)
        v = _c(var).reshape(-1, 9) if var is not None else None
        seq = C.c_int64(-1)
        self.ctx._chk(self.lib.vba_scanlog_push_points(self.h, len(pnt), _p(pnt), _p(v), C.byref(seq)))
        return seq.value

    def range(self):
        """(first, end, sizes int32 [end - first]) of the live scans"""
        a = C.c_int64(); b = C.c_int64()
        self.ctx._chk(self.lib.vba_scanlog_range(self.h, C.byref(a), C.byref(b), 0, None))
        sizes = np.zeros(max(b.value - a.value, 1), dtype=np.int32)
        self.ctx._chk(self.lib.vba_scanlog_range(self.h, C.byref(a), C.byref(b), len(sizes), sizes.ctypes.data_as(C.POINTER(C.c_int))))
        return a.value, b.value, sizes[:max(b.value - a.value, 0)].copy()

    def release(self, upto):
        self.ctx._chk(self.lib.vba_scanlog_release(self.h, upto))

    def read(self, seq, xyz=False):
        """scan ``seq`` -> (pnt [n][3], var [n][9]); with xyz=True also the float32 [n][3] form narrowed on the device"""
        n = C.c_int()
        self.ctx._chk(self.lib.vba_scanlog_read(self.h, seq, 0, None, None, None, C.byref(n)))
        m = max(n.value, 1)
        pnt = np.zeros((m, 3)); var = np.zeros((m, 9)); f = np.zeros((m, 3), dtype=np.float32) if xyz else None
        self.ctx._chk(self.lib.vba_scanlog_read(self.h, seq, n.value, _p(pnt), _p(var),
                                                f.ctypes.data_as(C.POINTER(C.c_float)) if xyz else None, C.byref(n)))
        out = (pnt[:n.value].copy(), var[:n.value].copy())
        return out + (f[:n.value].copy(),) if xyz else out

    def export_world(self, first, poses, stride=1, intensity=0.0, ctx=None, out=None, cap=None):
        """pub_localmap's point loop over scans first .. first + k - 1 at ``poses`` [k][12] on ``ctx``'s stream (default: the log's
        context).  Returns float32 [n][4] records x y z intensity; with ``out`` (the address of a 16-byte aligned DEVICE buffer of
        ``cap`` records) the call is stream-ordered, does not synchronise and returns the record count."""
        ctx = ctx or self.ctx
        poses = _c(poses).reshape(-1, 12)
        k = len(poses)
        n = C.c_int64()
        head = (ctx.h, self.h, first, k, _p(poses), int(stride), intensity)
        if out is not None:
            ctx._chk(self.lib.vba_scanlog_export_world(*head, int(cap), out if isinstance(out, C.c_void_p) else C.c_void_p(int(out)), C.byref(n)))
            return n.value
        if cap is None:
            a, b, sizes = self.range()
            s = sizes[first - a:first - a + k].astype(np.int64)
            cap = int(((s + stride - 1) // max(int(stride), 1)).sum())
        res = np.zeros((max(int(cap), 1), 4), dtype=np.float32)
        ctx._chk(self.lib.vba_scanlog_export_world(*head, int(cap), res.ctypes.data_as(C.c_void_p), C.byref(n)))
        return res[:n.value].copy()


SCAN_TIME_NONE, SCAN_TIME_F32, SCAN_TIME_U32_DIV1E9, SCAN_TIME_F64_REL_FIRST = range(4)
SCAN_INTENSITY_NONE, SCAN_INTENSITY_F32, SCAN_INTENSITY_U8 = range(3)


class ScanLayout(C.Structure):
    """vba_scan_layout: where the fields of one record of a raw sensor message lie (byte offsets, not necessarily aligned)."""
    _fields_ = [("point_step", C.c_int), ("off_x", C.c_int), ("off_y", C.c_int), ("off_z", C.c_int),
                ("off_intensity", C.c_int), ("intensity_type", C.c_int), ("off_time", C.c_int), ("time_type", C.c_int), ("filter", C.c_int)]


def scan_layout(name) -> ScanLayout:
    """Layouts of the reference's sensors as their drivers usually publish them; a node fills the struct from msg->fields instead
    (INTEGRATION.md).  livox: CustomPoint; velodyne: x y z intensity time ring, padded to 32; ouster: ouster_ros::Point (48);
    hesai: the 26-byte packed record of the XT32 driver (f64 timestamp at 16); tartanair: PointXYZ, no filter."""
    if name == "livox":
        l = ScanLayout()
        st = load().vba_scan_layout_livox(C.byref(l))
        if st != OK:
            raise VbaError(st, "vba_scan_layout_livox")
        return l
    table = {
        "velodyne": (32, 0, 4, 8, 0, SCAN_INTENSITY_NONE, 20, SCAN_TIME_F32, 1),
        "ouster": (48, 0, 4, 8, 16, SCAN_INTENSITY_F32, 20, SCAN_TIME_U32_DIV1E9, 1),
        "hesai": (26, 0, 4, 8, 12, SCAN_INTENSITY_F32, 16, SCAN_TIME_F64_REL_FIRST, 1),
        "tartanair": (16, 0, 4, 8, 0, SCAN_INTENSITY_NONE, 0, SCAN_TIME_NONE, 0),
    }
    return ScanLayout(*table[name])


def scan_layout_check(layout) -> int:
    """vba_scan_layout_check (host only): the status, OK or ERR_BAD_ARG."""
    return load().vba_scan_layout_check(C.byref(layout))


class ScanFrame(_Handle):
    """One vba_scan_frame: the device buffers of one scan from the raw message to var_init's output."""
    PREFIX = "vba_scan_frame"

    def __init__(self, ctx):
        super().__init__(ctx)
        self.n = 0
        self.n_ds = 0

    def reserve(self, max_raw_points, max_point_step):
        self.ctx._chk(self.lib.vba_scan_frame_reserve(self.h, max_raw_points, max_point_step))

    def decode(self, layout, raw, point_filter_num=1, blind2=0.0, n_raw=None):
        """raw: the message's bytes (bytes or a uint8 array).  Returns (n, last_curvature)."""
        buf = np.ascontiguousarray(np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else raw, dtype=np.uint8).ravel()
        if n_raw is None:
            n_raw = len(buf) // layout.point_step
        if len(buf) < n_raw * layout.point_step:
            raise ValueError("raw holds fewer than n_raw records")
        n = C.c_int(0); last = C.c_double(0.0)
        self.ctx._chk(self.lib.vba_scan_decode(self.h, C.byref(layout), buf.ctypes.data_as(C.c_void_p), n_raw, point_filter_num,
                                               blind2, C.byref(n), C.byref(last)))
        self.n = n.value; self.n_ds = 0
        return n.value, last.value

    def prepare(self, imu_poses22, end_pose12, ext_pose12, down_size, dept_err, beam_err, min_points=500, point_notime=False, ctx=None):
        """Returns (n, d_pnt_body, d_var_body): the count and two DEVICE addresses (integers) owned by the frame."""
        ctx = ctx or self.ctx
        ip = _c(imu_poses22) if imu_poses22 is not None else np.zeros((0, 22))
        end = _c(end_pose12) if end_pose12 is not None else None
        n = C.c_int(0); dp = C.c_void_p(); dv = C.c_void_p()
        ctx._chk(self.lib.vba_scan_prepare(ctx.h, self.h, len(ip), _p(ip), _p(end), _p(_c(ext_pose12)), int(point_notime),
                                           down_size, min_points, dept_err, beam_err,
                                           C.byref(n), C.byref(dp), C.byref(dv)))
        self.n_ds = n.value
        return n.value, dp.value or 0, dv.value or 0

    def read(self, stage):
        """stage 0 / 1: dict(pnt, intensity, curvature); 2: dict(pnt, count, first); 3: dict(pnt, var)."""
        n = self.n if stage < 2 else self.n_ds
        ip = C.POINTER(C.c_int)
        pnt = np.zeros((n, 3)); out = dict(pnt=pnt)
        inten = curv = cnt = first = var = None
        if stage < 2:
            inten = np.zeros(n, dtype=np.float32); curv = np.zeros(n); out.update(intensity=inten, curvature=curv)
        elif stage == 2:
            cnt = np.zeros(n, dtype=np.int32); first = np.zeros(n, dtype=np.int32); out.update(count=cnt, first=first)
        else:
            var = np.zeros((n, 9)); out.update(var=var)
        self.ctx._chk(self.lib.vba_scan_frame_read(self.h, stage, _p(pnt), inten.ctypes.data_as(C.POINTER(C.c_float)) if inten is not None else None,
                                                   _p(curv), cnt.ctypes.data_as(ip) if cnt is not None else None,
                                                   first.ctypes.data_as(ip) if first is not None else None, _p(var)))
        return out


class InitWindow(_Handle):
    """One vba_init_window: pl_origs of the LiDAR-inertial initialisation, resident in HBM."""
    PREFIX = "vba_init_window"

    def reserve(self, max_scans, max_points_per_scan):
        self.ctx._chk(self.lib.vba_init_window_reserve(self.h, max_scans, max_points_per_scan))

    def clear(self):
        self.ctx._chk(self.lib.vba_init_window_clear(self.h))

    def size(self):
        n = C.c_int()
        self.ctx._chk(self.lib.vba_init_window_size(self.h, C.byref(n), None))
        return n.value

    def offsets(self):
        off = np.zeros(self.size() + 1, dtype=np.int64)
        n = C.c_int()
        self.ctx._chk(self.lib.vba_init_window_size(self.h, C.byref(n), off.ctypes.data_as(C.POINTER(C.c_int64))))
        return off

    def push(self, frame, down_size, min_points=1000):
        """down_sampling_close + retry + sort of VS:1499-1511 from the frame's stage 0.  Returns (n_kept, retried)."""
        n = C.c_int(0); r = C.c_int(0)
        self.ctx._chk(self.lib.vba_init_window_push(self.h, frame.h, down_size, min_points, C.byref(n), C.byref(r)))
        return n.value, r.value

    def push_points(self, pnt, curv):
        """Appends host arrays pnt [n][3], curv [n] (ascending) as they are."""
        pnt = _c(np.reshape(pnt, (-1, 3))); curv = _c(np.ravel(curv))
        if len(pnt) != len(curv):
            raise ValueError("pnt and curv differ in length")
        self.ctx._chk(self.lib.vba_init_window_push_points(self.h, len(curv), _p(pnt), _p(curv)))

    def read(self, scan):
        """(pnt [n][3], curv [n]) of one scan."""
        off = self.offsets()
        if not 0 <= scan < len(off) - 1:
            raise IndexError(scan)
        n = int(off[scan + 1] - off[scan])
        pnt = np.zeros((n, 3)); curv = np.zeros(n)
        self.ctx._chk(self.lib.vba_init_window_read(self.h, scan, _p(pnt), _p(curv)))
        return pnt, curv


class OdomReport(C.Structure):
    """vba_odom_report (include/voxelba.h)."""
    _fields_ = [("iterations", C.c_int), ("match_num", C.c_int * 4), ("rot_add", C.c_double * 4), ("tra_add", C.c_double * 4),
                ("nnt_eig_min", C.c_double)]


class SurfelOdomParams(C.Structure):
    """vba_surfel_odom_params (include/voxelba.h)."""
    _fields_ = [("gate", C.c_double), ("neighbors", C.c_int), ("min_matches", C.c_int), ("min_eig", C.c_double)]


def surfel_odom_default_params(**kw) -> SurfelOdomParams:
    p = SurfelOdomParams()
    load().vba_surfel_odom_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _odom_report(rep):
    return dict(iterations=rep.iterations, match_num=np.array(rep.match_num[:], dtype=np.int64), rot_add=np.array(rep.rot_add[:]),
                tra_add=np.array(rep.tra_add[:]), nnt_eig_min=rep.nnt_eig_min)


class OdomState(_Handle):
    """One vba_odom_state:the odometry state and its covariance resident in HBM from one scan to the next, with the pose table of
    the IMU propagation."""
    PREFIX = "vba_odom_state"

    def reserve(self, max_imu_rows):
        self.ctx._chk(self.lib.vba_odom_state_reserve(self.h, max_imu_rows))

    def set(self, state25, cov225):
        self.ctx._chk(self.lib.vba_odom_state_set(self.h, _p(_c(state25)), _p(_c(cov225))))

    def get(self):
        """(state [25], cov [15][15]); synchronises"""
        st = np.zeros(25); cov = np.zeros((15, 15))
        self.ctx._chk(self.lib.vba_odom_state_get(self.h, _p(st), _p(cov)))
        return st, cov

    def poses(self):
        """(imu_poses [n][22], end_pose [12]) of the last propagation; synchronises"""
        n = C.c_int(0)
        self.ctx._chk(self.lib.vba_odom_state_poses(self.h, 0, None, None, C.byref(n)))
        rows = np.zeros((n.value, 22)); end = np.zeros(12)
        self.ctx._chk(self.lib.vba_odom_state_poses(self.h, n.value, _p(rows), _p(end), C.byref(n)))
        return rows, end

    def propagate(self, imu, noise12, last_pcl_end_time, pcl_beg_time, pcl_end_time, scale_gravity=1.0):
        """IMUEKF::motion_blur's propagation (ekf_imu.hpp:54-123) on the device state; returns the rows of the pose table.  No wait."""
        imu = _c(imu).reshape(-1, 7); n = C.c_int(0)
        self.ctx._chk(self.lib.vba_odom_state_propagate(self.h, _p(_c(noise12)), scale_gravity, len(imu), _p(imu),
                                                        last_pcl_end_time, pcl_beg_time, pcl_end_time, C.byref(n)))
        return n.value

    def prepare(self, frame, ext_pose12, down_size, dept_err, beam_err, min_points=500, point_notime=False, ctx=None):
        """ScanFrame.prepare with the table and end_pose of the last propagation read in place: (n, d_pnt_body, d_var_body)."""
        ctx = ctx or self.ctx
        n = C.c_int(0); dp = C.c_void_p(); dv = C.c_void_p()
        ctx._chk(self.lib.vba_scan_prepare_on_state(ctx.h, frame.h, self.h, _p(_c(ext_pose12)), int(point_notime), down_size,
                                                    min_points, dept_err, beam_err, C.byref(n), C.byref(dp), C.byref(dv)))
        frame.n_ds = n.value
        return n.value, dp.value or 0, dv.value or 0

    def lio_state_estimation(self, n, d_pnt_body, d_var_body, ctx=None):
        """Context.lio_state_estimation_resident on the resident state: (ok, state, report); the state object holds state and
        covariance afterwards."""
        ctx = ctx or self.ctx
        ok = C.c_int(0); rep = OdomReport(); st = np.zeros(25)
        ctx._chk(self.lib.vba_odom_lio_state_estimation_on_state(ctx.h, self.h, n, C.c_void_p(d_pnt_body), C.c_void_p(d_var_body), C.byref(ok),
                                                                 C.byref(rep), _p(st)))
        report = dict(iterations=rep.iterations, match_num=np.array(rep.match_num[:], dtype=np.int64), rot_add=np.array(rep.rot_add[:]),
                      tra_add=np.array(rep.tra_add[:]), nnt_eig_min=rep.nnt_eig_min)
        return bool(ok.value), st, report

    def surfel_update(self, smap, pnt, params=None, n=None, ctx=None):
        """Context.odom_surfel_update on the resident state: (ok, state, report); ``pnt`` a device address
        with ``n`` (read in place) or a host array [n][3] (staged in the map); the state object holds state and covariance
        afterwards."""
        ctx = ctx or self.ctx
        p = params if params is not None else surfel_odom_default_params()
        n, ptr, keep = SurfelMap._pnt(pnt, n)
        ok = C.c_int(0); rep = OdomReport(); st = np.zeros(25)
        ctx._chk(self.lib.vba_odom_surfel_update_on_state(ctx.h, self.h, smap.h, n, ptr, C.byref(p), C.byref(ok), C.byref(rep), _p(st)))
        return bool(ok.value), st, _odom_report(rep)

    def pvec_update_cut_voxel(self, win_count, n, d_pnt_body, d_var_body, multi=False, ctx=None):
        """Context.pvec_update_cut_voxel_dev with the pose and covariance blocks of the resident state."""
        ctx = ctx or self.ctx
        ctx._chk(self.lib.vba_map_pvec_update_cut_voxel_on_state(ctx.h, self.h, win_count, n, C.c_void_p(d_pnt_body),
                                                                 C.c_void_p(d_var_body), int(multi)))

    def lio_state_estimation_kdtree(self, ctx, n, d_pnt_body, want_state=True):
        """Context.lio_state_estimation_kdtree_resident on the resident state and ``ctx``'s point-cloud map:
        (iterations, report, state or None); the state object holds state and covariance afterwards.  A seeding call (map below 100
        points) returns 0 iterations and, with want_state=False, without waiting."""
        ctx = ctx or self.ctx
        it = C.c_int(0); rep = OdomReport(); st = np.zeros(25) if want_state else None
        ctx._chk(self.lib.vba_odom_lio_state_estimation_kdtree_on_state(ctx.h, self.h, n, C.c_void_p(d_pnt_body), C.byref(it), C.byref(rep), _p(st)))
        report = dict(iterations=rep.iterations, match_num=np.array(rep.match_num[:], dtype=np.int64), rot_add=np.array(rep.rot_add[:]),
                      tra_add=np.array(rep.tra_add[:]), nnt_eig_min=rep.nnt_eig_min)
        return it.value, report, st

    def export_scan(self, ctx, n, d_pnt_body, intensity=0.0, out=None):
        """pub_localtraj's scan (VS:37-45): the n device points in the pose of the resident state as float32 [n][4] records
        x y z intensity.  With ``out`` (the address of a 16-byte aligned DEVICE buffer of n records) the call is stream-ordered, does
        not synchronise and returns the record count."""
        ctx = ctx or self.ctx
        m = C.c_int64()
        head = (ctx.h, self.h, n, C.c_void_p(d_pnt_body), intensity, n)
        if out is not None:
            ctx._chk(self.lib.vba_odom_state_export_scan(*head, out if isinstance(out, C.c_void_p) else C.c_void_p(int(out)), C.byref(m)))
            return m.value
        res = np.zeros((max(n, 1), 4), dtype=np.float32)
        ctx._chk(self.lib.vba_odom_state_export_scan(*head, res.ctypes.data_as(C.c_void_p), C.byref(m)))
        return res[:m.value].copy()


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class VbaError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("libvoxelba status %d: %s" % (status, msg))
        self.status = status


def build(force: bool = False) -> str:
    """Compile libvoxelba.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    src = os.path.join(_PKG, "csrc")
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-C", src, "-s"])
    return LIB_PATH


_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libvoxelba.so is missing (run __graft_entry__.build()); there is no CPU fallback")
        lib = C.CDLL(LIB_PATH)
        for name, proto in PROTOTYPES.items():     # (a symbol the library lacks raises AttributeError here)
            fn = getattr(lib, name)
            ret, params = proto.split(":")
            fn.restype = KINDS[ret]
            fn.argtypes = [KINDS[k] for k in params]
        _lib = lib
    return _lib


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def default_options() -> Options:
    o = Options()
    load().vba_default_options(C.byref(o))
    # test-harness hook of THIS binding (the library itself reads no environment): "field=value,field=value" applied to every
    # options struct this process builds, e.g. VBA_PY_OPTIONS="residual_vpl_from=1" in the child pytest of tests/test_gpu_bigstore.py
    for kv in filter(None, os.environ.get("VBA_PY_OPTIONS", "").split(",")):
        k, v = kv.split("=")
        setattr(o, k.strip(), type(getattr(o, k.strip()))(float(v)))
    return o


def options_from_workload(wl, stream=None) -> Options:
    o = default_options()
    o.win_size = wl.win_size
    o.voxel_size = wl.voxel_size
    o.max_layer = wl.max_layer
    o.max_points = wl.max_points
    o.min_eigen_value = wl.min_eigen_value
    for i in range(4):
        o.plane_eigen_value_thre[i] = wl.plane_thre[i]
        o.min_point[i] = wl.min_point[i]
    o.imu_coef = wl.imu_coef
    if stream is not None:
        o.stream = stream
    return o


def shard_owner(key3, n_ranks: int) -> int:
    return load().vba_shard_owner(int(key3[0]), int(key3[1]), int(key3[2]), int(n_ranks))


def imu_preintegrate(t, gyr, acc, bg, ba, noise_meas, noise_walk, scale_gravity=1.0):
    t, gyr, acc, bg, ba, nm, nw = map(_c, (t, gyr, acc, bg, ba, noise_meas, noise_walk))
    out = np.empty(304)
    st = load().vba_imu_preintegrate(len(t), _p(t), _p(gyr), _p(acc), _p(bg), _p(ba), _p(nm), _p(nw), scale_gravity, _p(out))
    if st:
        raise VbaError(st)
    return out


def imu_give_evaluate(imu, st1, st2, with_g=False, jac=True):
    imu, st1, st2 = map(_c, (imu, st1, st2))
    nb = 33 if with_g else 30
    jtj = np.zeros((nb, nb)); gg = np.zeros(nb); r = C.c_double()
    st = load().vba_imu_give_evaluate(_p(imu), _p(st1), _p(st2), int(with_g), int(jac), _p(jtj), _p(gg), C.byref(r))
    if st:
        raise VbaError(st)
    return r.value, jtj, gg


def imu_ekf_propagate(imu, noise12, last_pcl_end_time, pcl_beg_time, pcl_end_time, state25, cov225, scale_gravity=1.0):
    """IMUEKF::motion_blur's propagation (ekf_imu.hpp:54-123) on the host: imu [m][7] after push_front(last_imu).  Returns
    (state, cov [15][15], imu_poses [n][22], end_pose [12])."""
    imu = _c(imu).reshape(-1, 7); st = _c(state25).copy(); cov = _c(cov225).reshape(15, 15).copy()
    rows = np.zeros((max(len(imu) - 1, 1), 22)); end = np.zeros(12); n = C.c_int(0)
    r = load().vba_imu_ekf_propagate(len(imu), _p(imu), _p(_c(noise12)), scale_gravity, last_pcl_end_time,
                                     pcl_beg_time, pcl_end_time, _p(st), _p(cov), _p(rows), _p(end), C.byref(n))
    if r:
        raise VbaError(r)
    return st, cov, rows[:n.value].copy(), end


def init_imu_poses(imu, state_c, state_l, beg_time, scale_gravity=1.0):
    """Backward IMU pose table of Initialization::motion_blur (voxelslam.cpp:508-544): rows [t, R(9), p(3), v(3), angvel(3), acc(3)]."""
    imu = _c(imu).reshape(-1, 7); xc = _c(state_c); xl = _c(state_l)
    m = len(imu)
    out = np.zeros((max(m - 1, 0), 22))
    st = load().vba_init_imu_poses(m, _p(imu), _p(xc), _p(xl), beg_time, scale_gravity, _p(out))
    if st:
        raise VbaError(st)
    return out


def init_align_gravity(states):
    """Initialization::align_gravity (voxelslam.cpp:470-497) on a copy of states [n][25]."""
    xs = _c(states).copy()
    st = load().vba_init_align_gravity(len(xs), _p(xs))
    if st:
        raise VbaError(st)
    return xs


def _io_chk(st):
    if st:
        raise VbaError(st, load().vba_status_string(st).decode())


def save_pcd(path, xyz):
    """FileReaderWriter::save_pcd (voxelslam.cpp:166-179): binary PCD of PointXYZI, intensity 0."""
    xyz = _c(xyz).reshape(-1, 3)
    _io_chk(load().vba_io_save_pcd(os.fsencode(path), len(xyz), _p(xyz)))


def load_pcd(path):
    """pcl::io::loadPCDFile as used by previous_map_read (voxelslam.cpp:337-340) -> (xyz [n,3], intensity [n])."""
    n = C.c_int(0)
    st = load().vba_io_load_pcd(os.fsencode(path), 0, None, None, C.byref(n))
    if st not in (0, 7):
        _io_chk(st)
    xyz = np.zeros((max(n.value, 1), 3)); inten = np.zeros(max(n.value, 1))
    _io_chk(load().vba_io_load_pcd(os.fsencode(path), n.value, _p(xyz), _p(inten), C.byref(n)))
    return xyz[:n.value], inten[:n.value]


def save_pose(path, states, v6):
    """FileReaderWriter::save_pose (voxelslam.cpp:181-204); writes nothing for fewer than 100 scans."""
    states = _c(states).reshape(-1, 25); v6 = _c(v6).reshape(-1, 6)
    _io_chk(load().vba_io_save_pose(os.fsencode(path), len(states), _p(states), _p(v6)))


def kf_export_plan(sizes, interval_size=5_000_000, jump=0):
    """vba_kf_export_plan (pub_globalmap, voxelslam.cpp:110-154; host only): ``sizes`` = the point counts of all keyframes of all
    exported sessions in publication order, jump 0 = the reference's rule.  Returns (jump in force, kf_begin int64 [n_kf + 1],
    msg_end_kf int32 [n_msgs]): message m is the exported points kf_begin[msg_end_kf[m - 1]] .. kf_begin[msg_end_kf[m]]."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int32).ravel()
    n = len(sizes)
    ip = C.POINTER(C.c_int)
    j = C.c_int(); nm = C.c_int()
    kb = np.zeros(n + 1, dtype=np.int64); me = np.zeros(n + 1, dtype=np.int32)
    _io_chk(load().vba_kf_export_plan(n, sizes.ctypes.data_as(ip), int(interval_size), int(jump), C.byref(j),
                                      kb.ctypes.data_as(C.POINTER(C.c_int64)), n + 1, me.ctypes.data_as(ip), C.byref(nm)))
    return j.value, kb, me[:nm.value].copy()


def read_lidarstate(path):
    """read_lidarstate (voxelslam.hpp:268-307) -> (states [n,25], v6 [n,6])."""
    n = C.c_int(0)
    st = load().vba_io_read_lidarstate(os.fsencode(path), 0, None, None, C.byref(n))
    if st not in (0, 7):
        _io_chk(st)
    states = np.zeros((max(n.value, 1), 25)); v6 = np.zeros((max(n.value, 1), 6))
    _io_chk(load().vba_io_read_lidarstate(os.fsencode(path), n.value, _p(states), _p(v6), C.byref(n)))
    return states[:n.value], v6[:n.value]


class Context:
    """One vba_ctx: a HIP stream, the HBM factor store (``LidarFactor``) and the device voxel map."""

    def __init__(self, opt: Options):
        self.lib = load()
        self.opt = opt
        self.W = opt.win_size
        h = C.c_void_p()
        st = self.lib.vba_create(C.byref(opt), C.byref(h))
        if st:
            raise VbaError(st, self.lib.vba_status_string(st).decode())
        self.h = h
        self._cb = None
        self._btc = []
        self._kf = []

    def close(self):
        for kf in list(getattr(self, "_kf", [])):      # (stores and databases belong to their context: destroyed first)
            kf.close()
        for db in list(getattr(self, "_btc", [])):
            db.close()
        if getattr(self, "h", None):
            self.lib.vba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st:
            raise VbaError(st, self.lib.vba_status_string(st).decode() + " | " + self.lib.vba_last_error(self.h).decode())

    def synchronize(self):
        self._chk(self.lib.vba_synchronize(self.h))

    # ---- LidarFactor (voxel_map.hpp:124-339)
    def clear(self):
        self._chk(self.lib.vba_factor_clear(self.h))

    def size(self) -> int:
        return self.lib.vba_factor_size(self.h)

    def push_voxels(self, clusters, fix, coe, eig_val, eig_vec, pcr_add):
        a = [_c(x) for x in (clusters, fix, coe, eig_val, eig_vec, pcr_add)]
        self._chk(self.lib.vba_factor_push_voxels(self.h, len(a[2]), *[_p(x) for x in a]))

    def push_dict(self, f):
        self.push_voxels(f["clusters"], f["fix"], f["coe"], f["eig_val"], f["eig_vec"], f["pcr_add"])

    def acc_evaluate2(self, poses, head=0, end=None):
        end = self.size() if end is None else end
        poses = _c(poses); n = 6 * self.W
        H = np.empty((n, n)); g = np.empty(n); r = C.c_double()
        self._chk(self.lib.vba_factor_acc_evaluate2(self.h, _p(poses), head, end, _p(H), _p(g), C.byref(r)))
        return H, g, r.value

    def evaluate_only_residual(self, poses, head=0, end=None):
        end = self.size() if end is None else end
        poses = _c(poses); r = C.c_double()
        self._chk(self.lib.vba_factor_evaluate_only_residual(self.h, _p(poses), head, end, C.byref(r)))
        return r.value

    def read_back(self):
        n = self.size()
        ev = np.empty((n, 3)); evec = np.empty((n, 9)); pa = np.empty((n, 10))
        self._chk(self.lib.vba_factor_read_back(self.h, _p(ev), _p(evec), _p(pa)))
        return ev, evec, pa

    def factor_occupancy(self) -> float:
        """Occupied (voxel, frame) slots per voxel in the factor store."""
        n = C.c_longlong(0)
        self._chk(self.lib.vba_factor_occupied_slots(self.h, C.byref(n)))
        return n.value / max(self.size(), 1)

    def factor_occupancy_masks(self):
        m = np.zeros(self.size(), dtype=np.uint32)
        self._chk(self.lib.vba_factor_occupancy_masks(self.h, m.ctypes.data_as(C.POINTER(C.c_uint))))
        return m

    # ---- optimizers
    def last_trace(self):
        rows = np.zeros((64, 5))
        n = self.lib.vba_last_lm_trace(self.h, _p(rows), 64)
        return rows[:n].copy()

    def lidar_ba_damping_iter(self, poses, max_iter=3, thd_num=2):
        """Lidar_BA_Optimizer::damping_iter (voxel_map.hpp:422-497)."""
        poses = _c(poses).copy(); n = 6 * self.W
        H = np.empty((n, n)); resis = np.zeros(2); conv = C.c_int(0)
        st = self.lib.vba_lidar_ba_damping_iter(self.h, _p(poses), _p(H), _p(resis), max_iter, thd_num, C.byref(conv))
        if st == ERR_TOO_FEW_VOXELS:
            return dict(poses=poses, hess=H, resis=resis, converge=False, status=-1, trace=self.last_trace())
        self._chk(st)
        return dict(poses=poses, hess=H, resis=resis, converge=bool(conv.value), status=0, trace=self.last_trace())

    def li_ba_damping_iter(self, states, imus, gravity=False, max_iter=3):
        """LI_BA_Optimizer::damping_iter (voxel_map.hpp:624-713) / LI_BA_OptimizerGravity::damping_iter (:878-975)."""
        states = _c(states).copy(); imus = _c(imus).copy()
        n = 15 * self.W + (3 if gravity else 0)
        H = np.empty((n, n)); resis = np.zeros(2)
        self._chk(self.lib.vba_li_ba_damping_iter(self.h, _p(states), _p(imus), int(gravity), max_iter, _p(H), _p(resis)))
        return dict(states=states, imus=imus, hess=H, resis=resis, trace=self.last_trace())

    SOLVE_KINDS = {"lidar": 0, "li": 1, "dense": 2}
    SOLVE_FLAGS = {"e_packed": 1, "copy_raw": 2, "from_raw": 4, "gravity": 8, "dense_mask": 16, "all_panels": 32}

    def debug_solve(self, kind, W, H, g, u, v=2.0, **flags):
        """vba_debug_solve: one linear solve of the LM loop through the production kernel on the system (H, g) (before the gauge).
        kind in SOLVE_KINDS, flags = names of SOLVE_FLAGS set to True.  Returns (dx [candidates][n], q1 [candidates])."""
        f = 0
        for k, on in flags.items():
            f |= self.SOLVE_FLAGS[k] if on else 0
        H = _c(H); g = _c(g); n = len(g)
        nc = 1 if kind == "dense" else (self.opt.lm_spec if 0 < self.opt.lm_spec < 4 else 4)
        dx = np.zeros((nc, n)); q1 = np.zeros(nc)
        self._chk(self.lib.vba_debug_solve(self.h, self.SOLVE_KINDS[kind], W, f, _p(H), _p(g),
                                           u, v, _p(dx), _p(q1)))
        return dx, q1

    IMU_FORMS = {"alone": 0, "h2": 1, "h3": 2}

    def debug_li_imu(self, states, imus, gravity=False, form="alone", trial=False, raw_flags=None):
        """vba_debug_li_imu: the IMU factor pass of LI-BA once, through the production kernels, on states [W][25] and imus [W-1][304].
        form in IMU_FORMS (alone / riding k_hessian2 / riding k_hessian3); trial=True also runs k_li_update on the same states.
        Returns dict(H [n][n] dense, no imu_coef), g [n], rimu [2], covinv [W-1][15][15] (what the kernels read))."""
        states = _c(states); imus = _c(imus)
        W = self.W; n = 15 * W + (3 if gravity else 0)
        f = (self.IMU_FORMS[form] | (4 if trial else 0)) if raw_flags is None else raw_flags
        H = np.zeros((n, n)); g = np.zeros(n); rimu = np.zeros(2); ci = np.zeros((max(W - 1, 1), 15, 15))
        self._chk(self.lib.vba_debug_li_imu(self.h, W, int(gravity), f, _p(states), _p(imus), _p(H), _p(g),
                                            _p(rimu), _p(ci)))
        return dict(H=H, g=g, rimu=rimu, covinv=ci)

    def lm_begin(self, poses, thd_num=2):
        poses = _c(poses)
        self._chk(self.lib.vba_lm_begin(self.h, _p(poses), thd_num))

    def lm_iterate(self, sync=True):
        """One LM iteration (loop body voxel_map.hpp:441-494).  sync=False only enqueues the launches."""
        if not sync:
            self._chk(self.lib.vba_lm_iterate(self.h, None, None))
            return None
        acc = C.c_int(0); stop = C.c_int(0)
        self._chk(self.lib.vba_lm_iterate(self.h, C.byref(acc), C.byref(stop)))
        return bool(acc.value), bool(stop.value)

    def lm_refresh_eigen(self):
        self._chk(self.lib.vba_lm_refresh_eigen(self.h))

    def lm_end(self, fetch=True):
        if not fetch:
            self._chk(self.lib.vba_lm_end(self.h, None, None, None))
            return None
        n = 6 * self.W
        poses = np.empty((self.W, 12)); H = np.empty((n, n)); resis = np.zeros(2)
        self._chk(self.lib.vba_lm_end(self.h, _p(poses), _p(H), _p(resis)))
        return poses, H, resis

    # ---- LiDAR-inertial initialisation (voxelslam.cpp:617-819)
    def motion_init(self, clouds, curvs, imus_raw, beg_times, ext_pose12, dept_err, beam_err, scale_gravity, noise_meas, noise_walk,
                    states, covs, imu_pre, point_notime=False, want_hess=False, want_pvec=True):
        """Initialization::motion_init on the context's map and factor store.  clouds / curvs / imus_raw: per-scan lists ([n][3], [n],
        [m][7]).  Returns a dict: converged, eigvalue3, iterations, thresholds_left_relaxed, round_log [rounds][5], states, imu_pre,
        hess (want_hess), pvec (list of (pnt [k][3], var [k][3][3]) per scan, want_pvec)."""
        W = len(clouds)
        pto = np.zeros(W + 1, dtype=np.int32); imo = np.zeros(W + 1, dtype=np.int32)
        pto[1:] = np.cumsum([len(x) for x in clouds]); imo[1:] = np.cumsum([len(x) for x in imus_raw])
        pnt = _c(np.concatenate([np.reshape(x, (-1, 3)) for x in clouds])) if pto[-1] else np.zeros((1, 3))
        cv = _c(np.concatenate([np.ravel(x) for x in curvs])) if pto[-1] else np.zeros(1)
        imu = _c(np.concatenate([np.reshape(x, (-1, 7)) for x in imus_raw])) if imo[-1] else np.zeros((1, 7))
        bt, ext, nm, nw = _c(beg_times), _c(ext_pose12), _c(noise_meas), _c(noise_walk)
        xs = _c(states).copy(); cov = _c(covs); ip = _c(imu_pre).copy()
        n = 15 * W + 3
        H = np.zeros((n, n)) if want_hess else None
        conv = C.c_int(0); iters = C.c_int(0); relax = C.c_int(0); eig = np.zeros(3); log = np.zeros((10, 5))
        ip_ = C.POINTER(C.c_int)
        pvo = np.zeros(W + 1, dtype=np.int32)
        cap = int(pto[-1] + imo[-1]) + 1 if want_pvec else 0
        po = np.zeros((cap, 3)) if want_pvec else None
        vo = np.zeros((cap, 9)) if want_pvec else None
        self._chk(self.lib.vba_motion_init(
            self.h, W, pto.ctypes.data_as(ip_), _p(pnt), _p(cv), imo.ctypes.data_as(ip_), _p(imu), _p(bt), _p(ext),
            dept_err, beam_err, scale_gravity, int(point_notime), _p(nm), _p(nw),
            _p(xs), _p(cov), _p(ip), _p(H), C.byref(conv), _p(eig), C.byref(iters), C.byref(relax), _p(log), 10,
            _p(po), _p(vo), pvo.ctypes.data_as(ip_), cap))
        out = dict(converged=conv.value, eigvalue3=eig, iterations=iters.value, thresholds_left_relaxed=relax.value,
                   round_log=log[:iters.value].copy(), states=xs, imu_pre=ip, hess=H, pvec_offsets=pvo)
        if want_pvec:
            out["pvec"] = [(po[pvo[i]:pvo[i + 1]].copy(), vo[pvo[i]:pvo[i + 1]].reshape(-1, 3, 3).copy()) for i in range(W)]
        return out

    def init_window(self) -> "InitWindow":
        return InitWindow(self)

    def motion_init_resident(self, window, imus_raw, beg_times, ext_pose12, dept_err, beam_err, scale_gravity, noise_meas, noise_walk,
                             states, covs, imu_pre, point_notime=False, want_hess=False, want_pvec=True):
        """motion_init with pl_origs read in place from an InitWindow (which is not cleared).  Returns the dict of motion_init."""
        W = len(imus_raw)
        off = window.offsets()
        imo = np.zeros(W + 1, dtype=np.int32)
        imo[1:] = np.cumsum([len(x) for x in imus_raw])
        imu = _c(np.concatenate([np.reshape(x, (-1, 7)) for x in imus_raw])) if imo[-1] else np.zeros((1, 7))
        bt, ext, nm, nw = _c(beg_times), _c(ext_pose12), _c(noise_meas), _c(noise_walk)
        xs = _c(states).copy(); cov = _c(covs); ip = _c(imu_pre).copy()
        n = 15 * W + 3
        H = np.zeros((n, n)) if want_hess else None
        conv = C.c_int(0); iters = C.c_int(0); relax = C.c_int(0); eig = np.zeros(3); log = np.zeros((10, 5))
        ip_ = C.POINTER(C.c_int)
        pvo = np.zeros(W + 1, dtype=np.int32)
        cap = int(off[-1] + imo[-1]) + 1 if want_pvec else 0
        po = np.zeros((cap, 3)) if want_pvec else None
        vo = np.zeros((cap, 9)) if want_pvec else None
        self._chk(self.lib.vba_motion_init_resident(
            self.h, W, window.h, imo.ctypes.data_as(ip_), _p(imu), _p(bt), _p(ext),
            dept_err, beam_err, scale_gravity, int(point_notime), _p(nm), _p(nw),
            _p(xs), _p(cov), _p(ip), _p(H), C.byref(conv), _p(eig), C.byref(iters), C.byref(relax), _p(log), 10,
            _p(po), _p(vo), pvo.ctypes.data_as(ip_), cap))
        out = dict(converged=conv.value, eigvalue3=eig, iterations=iters.value, thresholds_left_relaxed=relax.value,
                   round_log=log[:iters.value].copy(), states=xs, imu_pre=ip, hess=H, pvec_offsets=pvo)
        if want_pvec:
            out["pvec"] = [(po[pvo[i]:pvo[i + 1]].copy(), vo[pvo[i]:pvo[i + 1]].reshape(-1, 3, 3).copy()) for i in range(W)]
        return out

    # ---- loop retrieval (BTC.cpp, loop_refine.hpp)
    def btc_db(self, config=None) -> "BtcDb":
        return BtcDb(self, config if config is not None else btc_default_config(0))

    def kf_store(self) -> "KeyframeStore":
        return KeyframeStore(self)

    def loop_map(self) -> "LoopMap":
        return LoopMap(self)

    def surfel_map(self) -> "SurfelMap":
        return SurfelMap(self)

    def kf_export_world(self, stores, intensity, jump, begin=0, count=None, out=None):
        """vba_kf_export_world on this context's stream: exported points [begin, begin + count) of ``stores`` (KeyframeStore objects of
        this device, in publication order) at their current poses, ``intensity`` one float per store, ``jump`` >= 1 as kf_export_plan
        returned it.  count None = up to the end.  Returns float32 [count][4] records x y z intensity; with ``out`` (the address of a
        16-byte aligned DEVICE buffer of count records) the call is stream-ordered, does not synchronise and returns None."""
        inten = np.ascontiguousarray(intensity, dtype=np.float32).ravel()
        if len(inten) != len(stores):
            raise ValueError("one intensity per store")
        if count is None:
            j = max(int(jump), 1)
            count = sum(int(((s.sizes().astype(np.int64) + j - 1) // j).sum()) for s in stores) - int(begin)
        hs = (C.c_void_p * max(len(stores), 1))(*[(s.h.value if s is not None else None) for s in stores])
        args = (self.h, len(stores), hs, inten.ctypes.data_as(C.POINTER(C.c_float)), int(jump), int(begin), int(count))
        if out is not None:
            self._chk(self.lib.vba_kf_export_world(*args, out if isinstance(out, C.c_void_p) else C.c_void_p(int(out))))
            return None
        res = np.zeros((max(int(count), 0), 4), dtype=np.float32)
        self._chk(self.lib.vba_kf_export_world(*args, res.ctypes.data_as(C.c_void_p)))
        return res

    def kf_export_voxel(self, stores, intensity, jump, voxel_size, min_count=1, cap=None, out=None):
        """vba_kf_voxel_export on this context's stream: the records kf_export_world(stores, intensity, jump) would return, voxel
        down-sampled at ``voxel_size`` (one record per voxel in first-occurrence order: the centroid, the intensity of the voxel's
        first record), voxels of fewer than ``min_count`` records left out.  Returns (xyzi float32 [n][4], counts int32 [n]).
        ``cap`` None = room for every record (the result cannot be longer); a smaller ``cap`` raises VbaError(ERR_CAPACITY) when
        more voxels are kept.  With ``out`` = (xyzi address, counts address or None) of DEVICE buffers of ``cap`` entries (xyzi
        16-byte aligned) the result is written there stream-ordered and the call returns n."""
        inten = np.ascontiguousarray(intensity, dtype=np.float32).ravel()
        if len(inten) != len(stores):
            raise ValueError("one intensity per store")
        if cap is None:
            if out is not None:
                raise ValueError("a device result needs its capacity")
            j = max(int(jump), 1)
            cap = sum(int(((s.sizes().astype(np.int64) + j - 1) // j).sum()) for s in stores if s is not None)
        hs = (C.c_void_p * max(len(stores), 1))(*[(s.h.value if s is not None else None) for s in stores])
        n = C.c_int64(-1)
        args = (self.h, len(stores), hs, inten.ctypes.data_as(C.POINTER(C.c_float)), int(jump), float(voxel_size), int(min_count), int(cap))
        if out is not None:
            self._chk(self.lib.vba_kf_voxel_export(*args, out[0], out[1], C.byref(n)))
            return n.value
        xyzi = np.zeros((max(int(cap), 1), 4), dtype=np.float32); cnt = np.zeros(max(int(cap), 1), dtype=np.int32)
        self._chk(self.lib.vba_kf_voxel_export(*args, xyzi.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p), C.byref(n)))
        return xyzi[:n.value].copy(), cnt[:n.value].copy()

    def kf_export_voxel_size(self, stores, intensity, jump, voxel_size, min_count=1):
        """the size query of vba_kf_voxel_export (cap 0, no buffers): the number of voxels kf_export_voxel would keep"""
        inten = np.ascontiguousarray(intensity, dtype=np.float32).ravel()
        hs = (C.c_void_p * max(len(stores), 1))(*[s.h.value for s in stores])
        n = C.c_int64(-1)
        self._chk(self.lib.vba_kf_voxel_export(self.h, len(stores), hs, inten.ctypes.data_as(C.POINTER(C.c_float)), int(jump), float(voxel_size),
                                               int(min_count), 0, None, None, C.byref(n)))
        return n.value

    def kf_export_voxel_reserve(self, max_points):
        self._chk(self.lib.vba_kf_voxel_export_reserve(self.h, int(max_points)))

    def kf_export_voxel_allocations(self):
        n = C.c_int(); b = C.c_int64()
        self._chk(self.lib.vba_kf_voxel_export_allocations(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def kf_export_surfel(self, stores, intensity, jump, voxel_size, min_count=3, cap=None, out=None, want_cov=True, want_counts=True):
        """vba_kf_surfel_export on this context's stream: one surfel per voxel of kf_export_voxel(stores, intensity, jump, voxel_size,
        min_count), in its order.  Returns (surfels float32 [n][12], cov float64 [n][6] or None, counts int32 [n] or None): the
        mean, the intensity, the normal toward the sensor, sqrt of the three eigenvalues, l0 / trace and the count; the covariance
        xx xy xz yy yz zz.  ``cap`` None = room for every record.  With ``out`` = (surfels address, cov address or None, counts
        address or None) of DEVICE buffers of ``cap`` entries (surfels 16-byte, cov 8-byte aligned) the result is written there
        stream-ordered and the call returns n."""
        inten = np.ascontiguousarray(intensity, dtype=np.float32).ravel()
        if len(inten) != len(stores):
            raise ValueError("one intensity per store")
        if cap is None:
            if out is not None:
                raise ValueError("a device result needs its capacity")
            j = max(int(jump), 1)
            cap = sum(int(((s.sizes().astype(np.int64) + j - 1) // j).sum()) for s in stores if s is not None)
        hs = (C.c_void_p * max(len(stores), 1))(*[(s.h.value if s is not None else None) for s in stores])
        n = C.c_int64(-1)
        args = (self.h, len(stores), hs, inten.ctypes.data_as(C.POINTER(C.c_float)), int(jump), float(voxel_size), int(min_count), int(cap))
        if out is not None:
            self._chk(self.lib.vba_kf_surfel_export(*args, out[0], out[1], out[2], C.byref(n)))
            return n.value
        rows = max(int(cap), 1)
        rec = np.zeros((rows, 12), dtype=np.float32)
        cov = np.zeros((rows, 6), dtype=np.float64) if want_cov else None
        cnt = np.zeros(rows, dtype=np.int32) if want_counts else None
        self._chk(self.lib.vba_kf_surfel_export(*args, rec.ctypes.data_as(C.c_void_p), cov.ctypes.data_as(C.c_void_p) if want_cov else None,
                                                cnt.ctypes.data_as(C.c_void_p) if want_counts else None, C.byref(n)))
        m = n.value
        return rec[:m].copy(), (cov[:m].copy() if want_cov else None), (cnt[:m].copy() if want_counts else None)

    def kf_export_surfel_size(self, stores, intensity, jump, voxel_size, min_count=3):
        """the size query of vba_kf_surfel_export (cap 0, no buffers): the number of surfels kf_export_surfel would return"""
        inten = np.ascontiguousarray(intensity, dtype=np.float32).ravel()
        hs = (C.c_void_p * max(len(stores), 1))(*[s.h.value for s in stores])
        n = C.c_int64(-1)
        self._chk(self.lib.vba_kf_surfel_export(self.h, len(stores), hs, inten.ctypes.data_as(C.POINTER(C.c_float)), int(jump), float(voxel_size),
                                                int(min_count), 0, None, None, None, C.byref(n)))
        return n.value

    def kf_export_surfel_reserve(self, max_points, max_voxels):
        self._chk(self.lib.vba_kf_surfel_export_reserve(self.h, int(max_points), int(max_voxels)))

    def kf_export_surfel_allocations(self):
        n = C.c_int(); b = C.c_int64()
        self._chk(self.lib.vba_kf_surfel_export_allocations(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def loop_update(self, lm, poses_win, bl_scans=(), bl_poses=None, bl_vars=None, win_scans=None, win_vars=None, dx12=None):
        """loop_update() (VS:1255-1373) on this context's map: adopt ``lm``, insert the buf_lba2loop scans ``bl_scans`` (list of
        [n_i][3] body points, ``bl_vars`` the matching [n_i][9] or None) at ``bl_poses`` [k][12] as fixed points with covariances,
        re-insert the window's scans at ``poses_win`` [win_count][12] (``win_scans`` None: from the outgoing map's own scan ring,
        device to device) and recut.  Every pose is already moved by dx.  Returns the factor count."""
        poses_win = _c(poses_win).reshape(-1, 12)
        k = len(bl_scans)
        off = pnt = var = bp = None
        if k:
            off, pnt = Context._ragged(bl_scans)
            var = np.ascontiguousarray(np.concatenate([np.reshape(v, (-1, 9)) for v in bl_vars]), dtype=np.float64) if bl_vars is not None else None
            bp = _c(bl_poses).reshape(k, 12)
        woff = wp = wv = None
        if win_scans is not None:
            if len(win_scans) != len(poses_win):
                raise ValueError("one pose per window scan")
            woff, wp = Context._ragged(win_scans)
            wv = np.ascontiguousarray(np.concatenate([np.reshape(v, (-1, 9)) for v in win_vars]), dtype=np.float64) if win_vars is not None else None
        ip = C.POINTER(C.c_int)
        nf = C.c_int()
        self._chk(self.lib.vba_loop_update(self.h, lm.h, _p(_c(dx12)) if dx12 is not None else None, k,
                                           off.ctypes.data_as(ip) if off is not None else None, _p(pnt), _p(var), _p(bp),
                                           len(poses_win), _p(wp), _p(wv), woff.ctypes.data_as(ip) if woff is not None else None,
                                           _p(poses_win), C.byref(nf)))
        return nf.value

    def scan_log(self) -> "ScanLog":
        return ScanLog(self)

    def scanlog_loop_update(self, lm, poses_win, log, first, bl_poses, dx12=None):
        """``loop_update`` with the buf_lba2loop scans taken from the ScanLog ``log`` (scans first .. first + len(bl_poses) - 1, with
        their covariance rows) and the window from the outgoing map's scan ring.  Returns the factor count."""
        poses_win = _c(poses_win).reshape(-1, 12)
        bp = _c(bl_poses).reshape(-1, 12) if bl_poses is not None and len(bl_poses) else None
        k = len(bp) if bp is not None else 0
        nf = C.c_int()
        self._chk(self.lib.vba_scanlog_loop_update(self.h, lm.h, _p(_c(dx12)) if dx12 is not None else None, log.h, first, k,
                                                   _p(bp), len(poses_win), _p(poses_win), C.byref(nf)))
        return nf.value

    def btc_search_loop_sessions(self, dbs, rows, bits, cur_db, cur_frame=-1):
        """SearchLoop of one query against every database (VS:2417-2421): one upload, one synchronisation."""
        rows, bits, bp = _btc_query(rows, bits)
        if cur_frame < 0:
            cur_frame = cur_db.num_frames() + cur_frame
        arr = (C.c_void_p * max(len(dbs), 1))(*[d.h.value for d in dbs])
        res = (BtcResult * max(len(dbs), 1))()
        self._chk(self.lib.vba_btc_search_loop_sessions(len(dbs), arr, len(rows), _p(rows), bp, cur_db.h,
                                                        cur_frame, res))
        return [_btc_result(res[k]) for k in range(len(dbs))]

    # ---- voxel map
    def cut_voxel(self, win_count, pnt_body, pose12, var=None, multi=False):
        pnt_body = _c(pnt_body); pose12 = _c(pose12)
        v = _c(var) if var is not None else None
        self._chk(self.lib.vba_map_cut_voxel(self.h, win_count, len(pnt_body), _p(pnt_body), _p(v), _p(pose12), int(multi)))

    def pvec_update_cut_voxel(self, win_count, pnt_body, var_body, pose12, cov225, multi=False):
        """pvec_update (voxelslam.hpp:242-265) + cut_voxel[_multi], fused on the device."""
        pnt_body = _c(pnt_body); var_body = _c(var_body); pose12 = _c(pose12); cov = _c(cov225)
        self._chk(self.lib.vba_map_pvec_update_cut_voxel(self.h, win_count, len(pnt_body), _p(pnt_body), _p(var_body),
                                                         _p(pose12), _p(cov), int(multi)))

    def pvec_update_cut_voxel_dev(self, win_count, n, d_pnt_body, d_var_body, pose12, cov225, multi=False):
        """The same on DEVICE arrays (addresses as integers, e.g. what ScanFrame.prepare returns): consumed in place."""
        pose12 = _c(pose12); cov = _c(cov225)
        self._chk(self.lib.vba_map_pvec_update_cut_voxel(self.h, win_count, n, C.c_void_p(d_pnt_body), C.c_void_p(d_var_body),
                                                         _p(pose12), _p(cov), int(multi)))

    def scan_frame(self) -> "ScanFrame":
        return ScanFrame(self)

    def odom_state(self) -> "OdomState":
        return OdomState(self)

    def var_init(self, pnt, ext_pose12, dept_err, beam_err):
        """var_init (voxelslam.hpp:210-234): returns (pnt_out, var_out)."""
        pnt = _c(pnt); ext = _c(ext_pose12)
        po = np.empty_like(pnt); var = np.empty((len(pnt), 9))
        self._chk(self.lib.vba_scan_var_init(self.h, len(pnt), _p(pnt), _p(ext), dept_err, beam_err, _p(po), _p(var)))
        return po, var

    def down_sampling_voxel(self, pnt, voxel_size):
        pnt = _c(pnt); n = len(pnt)
        out = np.empty((max(n, 1), 3)); cnt = np.zeros(max(n, 1), dtype=np.int32); first = np.zeros(max(n, 1), dtype=np.int32)
        m = C.c_int(0)
        self._chk(self.lib.vba_scan_down_sampling_voxel(self.h, n, _p(pnt), voxel_size, _p(out),
                                                        cnt.ctypes.data_as(C.POINTER(C.c_int)), first.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m)))
        return out[:m.value].copy(), cnt[:m.value].copy(), first[:m.value].copy()

    def down_sampling_pvec(self, pnt, var, voxel_size):
        pnt = _c(pnt); var = _c(var); n = len(pnt)
        out = np.empty((max(n, 1), 3)); vd = np.empty((max(n, 1), 3)); cnt = np.zeros(max(n, 1), dtype=np.int32); m = C.c_int(0)
        self._chk(self.lib.vba_scan_down_sampling_pvec(self.h, n, _p(pnt), _p(var), voxel_size, _p(out), _p(vd),
                                                       cnt.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m)))
        return out[:m.value].copy(), vd[:m.value].copy(), cnt[:m.value].copy()

    def down_sampling_close(self, pnt, voxel_size):
        pnt = _c(pnt); n = len(pnt)
        idx = np.zeros(max(n, 1), dtype=np.int32); m = C.c_int(0)
        self._chk(self.lib.vba_scan_down_sampling_close(self.h, n, _p(pnt), voxel_size, idx.ctypes.data_as(C.POINTER(C.c_int)), C.byref(m)))
        return idx[:m.value].copy()

    def undistort(self, pnt, curv, imu_poses22, end_pose12, ext_pose12):
        pnt = _c(pnt).copy(); curv = _c(curv); ip = _c(imu_poses22)
        self._chk(self.lib.vba_scan_undistort(self.h, len(pnt), _p(pnt), _p(curv), len(ip), _p(ip), _p(_c(end_pose12)),
                                              _p(_c(ext_pose12))))
        return pnt

    def cut_voxel_fix(self, pnt_world, jour=0.0):
        pnt_world = _c(pnt_world)
        self._chk(self.lib.vba_map_cut_voxel_fix(self.h, len(pnt_world), _p(pnt_world), jour))

    def recut(self, win_count, poses, multi=False):
        poses = _c(poses)
        self._chk(self.lib.vba_map_recut(self.h, win_count, _p(poses), int(multi)))

    def margi(self, win_count, poses, jour=0.0):
        poses = _c(poses)
        self._chk(self.lib.vba_map_margi(self.h, win_count, _p(poses), jour))

    def slide(self, mgsize=1):
        self._chk(self.lib.vba_map_slide(self.h, mgsize))

    def prune(self, jour, dist=700):
        self._chk(self.lib.vba_map_prune(self.h, jour, dist))

    def map_reset(self):
        self._chk(self.lib.vba_map_reset(self.h))

    def num_roots(self):
        return self.lib.vba_map_num_roots(self.h)

    def num_slide_roots(self):
        return self.lib.vba_map_num_slide_roots(self.h)

    def map_stats(self):
        out = (C.c_longlong * 8)()
        self._chk(self.lib.vba_map_stats(self.h, out))
        keys = ("nodes_high_water", "free_roots", "free_blocks", "hash_capacity", "hash_used", "roots", "slide_roots", "fixed_points")
        return dict(zip(keys, [int(x) for x in out]))

    def dump_leaves(self):
        return _dump_rows(self.lib.vba_map_dump_leaves, self.h, 39)

    def dump_plane_var(self):
        """[kx,ky,kz,layer,path, plane_var(36), cov_add upper triangle (45)] per leaf."""
        return _dump_rows(self.lib.vba_map_dump_plane_var, self.h, 86)

    def map_display_sizes(self, win_count, poses, all_points=False):
        """the size query of vba_map_display: (n_points, n_planes, frame_begin int64 [win_count + 1])"""
        poses = _c(poses).reshape(-1, 12)
        npt = C.c_int64(-1); npl = C.c_int64(-1); fb = np.zeros(win_count + 1, dtype=np.int64)
        self._chk(self.lib.vba_map_display(self.h, win_count, _p(poses) if win_count else None, int(bool(all_points)), 0, None, None,
                                           fb.ctypes.data_as(C.c_void_p), 0, None, None, C.byref(npt), C.byref(npl)))
        return npt.value, npl.value, fb

    def map_display(self, win_count, poses, all_points=False, device_out=None):
        """vba_map_display (OctoTree::tras_display over the whole map): the planar leaves and the window's points that sit in them
        at ``poses`` [win_count][12]; ``all_points`` keeps every point that sits in a leaf.  Returns a dict: xyzi float32 [n][4],
        plane_of_point int32 [n], frame_begin int64 [win_count + 1], planes float32 [m][16], plane_key int64 [m][5].
        ``device_out`` = (cap_points, xyzi address, plane_of_point address or None, cap_planes, planes address or None, plane_key
        address or None) of DEVICE buffers (xyzi / planes 16-byte aligned): the result is written there stream-ordered and the dict
        holds n_points, n_planes and frame_begin."""
        poses = _c(poses).reshape(-1, 12)
        flags = int(bool(all_points))
        pp = _p(poses) if win_count else None
        npt = C.c_int64(-1); npl = C.c_int64(-1); fb = np.zeros(win_count + 1, dtype=np.int64)
        if device_out is not None:
            cap_pts, d_xyzi, d_pop, cap_pl, d_planes, d_key = device_out
            self._chk(self.lib.vba_map_display(self.h, win_count, pp, flags, int(cap_pts), d_xyzi, d_pop, fb.ctypes.data_as(C.c_void_p),
                                               int(cap_pl), d_planes, d_key, C.byref(npt), C.byref(npl)))
            return {"n_points": npt.value, "n_planes": npl.value, "frame_begin": fb}
        n, m, _ = self.map_display_sizes(win_count, poses, all_points)
        xyzi = np.zeros((max(n, 1), 4), dtype=np.float32); pop = np.zeros(max(n, 1), dtype=np.int32)
        planes = np.zeros((max(m, 1), 16), dtype=np.float32); key = np.zeros((max(m, 1), 5), dtype=np.int64)
        self._chk(self.lib.vba_map_display(self.h, win_count, pp, flags, max(n, 1), xyzi.ctypes.data_as(C.c_void_p), pop.ctypes.data_as(C.c_void_p),
                                           fb.ctypes.data_as(C.c_void_p), max(m, 1), planes.ctypes.data_as(C.c_void_p),
                                           key.ctypes.data_as(C.c_void_p), C.byref(npt), C.byref(npl)))
        return {"xyzi": xyzi[:npt.value].copy(), "plane_of_point": pop[:npt.value].copy(), "frame_begin": fb,
                "planes": planes[:npl.value].copy(), "plane_key": key[:npl.value].copy()}

    def map_display_reserve(self, max_points, max_planes):
        self._chk(self.lib.vba_map_display_reserve(self.h, int(max_points), int(max_planes)))

    def map_display_allocations(self):
        n = C.c_int(); b = C.c_int64()
        self._chk(self.lib.vba_map_display_allocations(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    # ---- odometry
    def lio_state_estimation(self, pnt_body, var_body, state25, cov225):
        """VOXEL_SLAM::lio_state_estimation (voxelslam.cpp:962-1098).  Returns (ok, state, cov)."""
        pnt_body = _c(pnt_body); var_body = _c(var_body)
        state = _c(state25).copy(); cov = _c(cov225).copy(); ok = C.c_int(0)
        self._chk(self.lib.vba_odom_lio_state_estimation(self.h, len(pnt_body), _p(pnt_body), _p(var_body), _p(state), _p(cov), C.byref(ok)))
        return bool(ok.value), state, cov

    def lio_state_estimation_dev(self, n, d_pnt_body, d_var_body, state25, cov225):
        """lio_state_estimation on DEVICE arrays (addresses as integers, e.g. what ScanFrame.prepare returns)."""
        state = _c(state25).copy(); cov = _c(cov225).copy(); ok = C.c_int(0)
        self._chk(self.lib.vba_odom_lio_state_estimation(self.h, n, C.c_void_p(d_pnt_body), C.c_void_p(d_var_body), _p(state), _p(cov), C.byref(ok)))
        return bool(ok.value), state, cov

    def lio_state_estimation_resident(self, n, d_pnt_body, d_var_body, state25, cov225):
        """The same update with its iterations resident on the device on DEVICE arrays (addresses as integers),
        read in place.  Returns (ok, state, cov, report) with report a dict: iterations, match_num[4], rot_add[4], tra_add[4] (entries
        of iterations that did not run are zero) and nnt_eig_min."""
        state = _c(state25).copy(); cov = _c(cov225).copy(); ok = C.c_int(0); rep = OdomReport()
        self._chk(self.lib.vba_odom_lio_state_estimation_resident(self.h, n, C.c_void_p(d_pnt_body), C.c_void_p(d_var_body), _p(state), _p(cov),
                                                                  C.byref(ok), C.byref(rep)))
        report = dict(iterations=rep.iterations, match_num=np.array(rep.match_num[:], dtype=np.int64), rot_add=np.array(rep.rot_add[:]),
                      tra_add=np.array(rep.tra_add[:]), nnt_eig_min=rep.nnt_eig_min)
        return bool(ok.value), state, cov, report

    def odom_surfel_update(self, smap, pnt, state25, cov225, params=None, n=None):
        """vba_odom_surfel_update: the iterated-EKF update of (state, cov) against the cells of ``smap``.
        ``pnt`` [n][3] host array, or a device address with ``n``.  Returns (ok, state, cov, report), report as in
        lio_state_estimation_resident with nnt_eig_min the smallest eigenvalue of the last iteration's sum of W."""
        p = params if params is not None else surfel_odom_default_params()
        n, ptr, keep = SurfelMap._pnt(pnt, n)
        state = _c(state25).reshape(25).copy(); cov = _c(cov225).reshape(225).copy(); ok = C.c_int(0); rep = OdomReport()
        self._chk(self.lib.vba_odom_surfel_update(self.h, smap.h, n, ptr, C.byref(p), _p(state), _p(cov), C.byref(ok), C.byref(rep)))
        return bool(ok.value), state, cov.reshape(15, 15), _odom_report(rep)

    def debug_odom_surfel_sums(self, smap, pnt, R, t, params=None, n=None):
        """vba_debug_odom_surfel_sums: ONE point loop of odom_surfel_update at the pose (R, t) -> dict(partial [nb][34], cost [nb],
        sums [34], cell int32 [n], gate uint8 [n], nb)"""
        p = params if params is not None else surfel_odom_default_params()
        n, ptr, keep = SurfelMap._pnt(pnt, n)
        R = _c(R).reshape(9); t = _c(t).reshape(3)
        rows = min((n + 255) // 256, 1024)
        partial = np.full((rows, 34), np.nan); cost = np.full(rows, np.nan); sums = np.full(34, np.nan); nb = C.c_int(-1)
        cell = np.full(n, -7, dtype=np.int32); gate = np.full(n, 7, dtype=np.uint8)
        self._chk(self.lib.vba_debug_odom_surfel_sums(self.h, smap.h, n, ptr, C.byref(p), _p(R), _p(t), rows, _p(partial), _p(cost), _p(sums),
                                                      cell.ctypes.data_as(C.c_void_p), gate.ctypes.data_as(C.c_void_p), C.byref(nb)))
        return dict(partial=partial, cost=cost, sums=sums, cell=cell, gate=gate, nb=nb.value)

    # ---- multi-GPU / timing
    def lio_state_estimation_kdtree(self, pnt_body, state25, cov225):
        pnt = _c(pnt_body); st = _c(state25).copy(); cov = _c(cov225).copy(); it = C.c_int(0)
        self._chk(self.lib.vba_odom_lio_state_estimation_kdtree(self.h, len(pnt), _p(pnt), _p(st), _p(cov), C.byref(it)))
        return it.value, st, cov

    def lio_state_estimation_kdtree_resident(self, n, d_pnt_body, state25, cov225):
        """The same odometry on a DEVICE array of n points (its address as an integer), read in place, with the iterations, the map
        append and the re-sampling resident on the device.  Returns (iterations, state, cov, report), report as
        in lio_state_estimation_resident (nnt_eig_min is 0: this variant has no nnt)."""
        st = _c(state25).copy(); cov = _c(cov225).copy(); it = C.c_int(0); rep = OdomReport()
        self._chk(self.lib.vba_odom_lio_state_estimation_kdtree_resident(self.h, n, C.c_void_p(d_pnt_body), _p(st), _p(cov), C.byref(it),
                                                                         C.byref(rep)))
        report = dict(iterations=rep.iterations, match_num=np.array(rep.match_num[:], dtype=np.int64), rot_add=np.array(rep.rot_add[:]),
                      tra_add=np.array(rep.tra_add[:]), nnt_eig_min=rep.nnt_eig_min)
        return it.value, st, cov, report

    ODOM_SUMS_KINDS = {"voxel": 0, "kd": 1}

    def debug_odom_sums(self, kind, pnt_body, var_body, state25, cov225, slices=0):
        """vba_debug_odom_sums: ONE point loop of a resident odometry update on host arrays.  kind in ODOM_SUMS_KINDS.  Returns
        dict(partial [nb][34], sums [34]) and, for "kd", cand [slices][n][5] (uint64), planes [n][4] and slices (the count that ran)."""
        pnt = _c(pnt_body).reshape(-1, 3); n = len(pnt); nb = (n + 255) // 256
        kd = self.ODOM_SUMS_KINDS[kind] == 1
        var = None if var_body is None else _c(var_body)
        st = _c(state25); cov = _c(cov225)
        partial = np.full((nb, 34), np.nan); sums = np.full(34, np.nan); used = C.c_int(-1)
        cand = np.zeros((8, max(n, 1), 5), dtype=np.uint64) if kd else None
        planes = np.full((max(n, 1), 4), np.nan) if kd else None
        self._chk(self.lib.vba_debug_odom_sums(self.h, self.ODOM_SUMS_KINDS[kind], n, _p(pnt), None if var is None else _p(var),
                                               _p(st), _p(cov), slices, _p(partial), _p(sums),
                                               cand.ctypes.data_as(C.c_void_p) if kd else None, _p(planes) if kd else None, C.byref(used)))
        out = dict(partial=partial, sums=sums)
        if kd:
            ns = used.value
            out.update(cand=cand.reshape(-1)[:ns * n * 5].reshape(ns, n, 5).copy(), planes=planes[:n], slices=ns)
        return out

    def debug_plane_update(self, rows67):
        """vba_debug_plane_update: plane_update alone on leaves [n][67] = add10 | ev3 | U9 | cov45 (host array, left as given).
        Returns [n][43] = centre3 | normal3 | radius | plane_var36."""
        rows = _c(rows67).reshape(-1, 67); n = len(rows)
        out = np.full((n, 43), np.nan)
        self._chk(self.lib.vba_debug_plane_update(self.h, n, _p(rows), _p(out)))
        return out

    def debug_pgo_step(self, poses, edges, priors):
        """vba_debug_pgo_step: one update of pgo_optimize (n_updates = 1) with every pass read back; the inputs are left as given.
        Returns dict(slot [F][121], pairs [P][2] (int32), blk [n + P][36], g [n][6], dx [n][6], cost, poses [n][12] = theta (+) delta)."""
        x = _c(poses).reshape(-1, 12); n = len(x)
        e = _c(edges).reshape(-1, 20); m = len(e)
        pr = _c(priors).reshape(-1, 19)
        slot = np.full((m + len(pr), 121), np.nan); npairs = C.c_int(-1)
        pairs = np.full((max(m, 1), 2), -1, dtype=np.int32); blk = np.full((n + m, 36), np.nan)
        g = np.full((n, 6), np.nan); dx = np.full((n, 6), np.nan); cost = C.c_double(np.nan); out = np.full((n, 12), np.nan)
        self._chk(self.lib.vba_debug_pgo_step(self.h, n, _p(x), m, _p(e) if m else None, len(pr), _p(pr) if len(pr) else None,
                                              _p(slot), C.byref(npairs), pairs.ctypes.data_as(C.c_void_p), _p(blk), _p(g), _p(dx),
                                              C.byref(cost), _p(out)))
        P = npairs.value
        return dict(slot=slot, pairs=pairs[:P].copy(), blk=blk[:n + P].copy(), g=g, dx=dx, cost=cost.value, poses=out)

    def kdtree_reserve(self, max_map_points, max_scan_points):
        self._chk(self.lib.vba_odom_kdtree_reserve(self.h, max_map_points, max_scan_points))

    def kdtree_allocations(self):
        n = C.c_int(); b = C.c_int64()
        self._chk(self.lib.vba_odom_kdtree_allocations(self.h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def kdtree_size(self):
        return self.lib.vba_odom_kdtree_size(self.h)

    def kdtree_points(self):
        n = self.kdtree_size(); out = np.zeros((max(n, 1), 3))
        if n:
            self._chk(self.lib.vba_odom_kdtree_points(self.h, _p(out)))
        return out[:n]

    # ---- hierarchical global BA
    @staticmethod
    def _ragged(clouds):
        off = np.zeros(len(clouds) + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(c) for c in clouds])
        return off, _c(np.concatenate(clouds))

    def gba_build(self, clouds, poses, gba_voxel_size, gba_min_eigen_value, gba_eig):
        off, pnt = self._ragged(clouds)
        self._chk(self.lib.vba_gba_build(self.h, len(clouds), off.ctypes.data_as(C.POINTER(C.c_int)), _p(pnt), _p(_c(poses)),
                                         gba_voxel_size, gba_min_eigen_value, _p(_c(gba_eig))))
        return self.size()

    def hba_add_edge(self, clouds, poses, gba_voxel_size, gba_min_eigen_value, gba_eig, max_iter, thread_num, want_cloud=True):
        W = len(clouds)
        off, pnt = self._ragged(clouds)
        poses = _c(poses).copy()
        edges = np.zeros((W * (W - 1) // 2 + 1, 20)); ne = C.c_int(0)
        cloud = np.zeros((max(len(pnt), 1), 3)); ccnt = np.zeros(max(len(pnt), 1), dtype=np.int32); nc = C.c_int(0)
        rl = np.zeros((max_iter + 1, 2)); nl = C.c_int(0)
        self._chk(self.lib.vba_hba_add_edge(self.h, W, off.ctypes.data_as(C.POINTER(C.c_int)), _p(pnt), _p(poses),
                                            gba_voxel_size, gba_min_eigen_value, _p(_c(gba_eig)), max_iter,
                                            thread_num, _p(edges), C.byref(ne), _p(cloud) if want_cloud else None,
                                            ccnt.ctypes.data_as(C.POINTER(C.c_int)), C.byref(nc), _p(rl), C.byref(nl)))
        return dict(poses=poses, edges=edges[:ne.value].copy(), cloud=cloud[:nc.value].copy(), cloud_count=ccnt[:nc.value].copy(),
                    resis=rl[:nl.value].copy())

    def hba_global(self, clouds, poses_x0, poses_now, gba_voxel_size, gba_min_eigen_value, gba_eig, total_max_iter, wdsize=10, mgsize=5):
        if isinstance(clouds, tuple):                # (offsets[n + 1], points[N][3]) already concatenated by the caller
            off, pnt = clouds
            n = len(off) - 1
        else:
            n = len(clouds)
            off, pnt = self._ragged(clouds)
        nwin = max(0, (n - wdsize) // mgsize + 1) if n >= wdsize else 0
        cap1 = nwin * (wdsize * (wdsize - 1) // 2) + 1; cap2 = nwin * (nwin - 1) // 2 + 1
        e1 = np.zeros((cap1, 20)); e2 = np.zeros((cap2, 20)); n1 = C.c_int(0); n2 = C.c_int(0)
        self._chk(self.lib.vba_hba_global(self.h, n, off.ctypes.data_as(C.POINTER(C.c_int)), _p(pnt), _p(_c(poses_x0)), _p(_c(poses_now)),
                                          gba_voxel_size, gba_min_eigen_value, _p(_c(gba_eig)), total_max_iter,
                                          wdsize, mgsize, _p(e1), cap1, C.byref(n1), _p(e2), cap2, C.byref(n2)))
        return e1[:n1.value].copy(), e2[:n2.value].copy()

    # ---- diagnostic entries of the any-window path (vba_debug_big_*; tests/test_gpu_big.py)
    @staticmethod
    def _i32(a):
        return np.ascontiguousarray(a, dtype=np.int32)

    @staticmethod
    def _pi(a):
        return a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None

    def debug_big_load(self, W, vptr, efr, ecl, eig_val, eig_vec, pcr_add, raw=False):
        """vba_debug_big_load: the caller's sparse store (CSR vptr [V+1], efr [E], ecl [E][10]; eig_val [V][3], eig_vec [V][9],
        pcr_add [V][10]) becomes the context's.  raw=True returns the status instead of raising."""
        vptr = self._i32(vptr); efr = self._i32(efr)
        a = [_c(x) for x in (ecl, eig_val, eig_vec, pcr_add)]
        st = self.lib.vba_debug_big_load(self.h, W, len(vptr) - 1, self._pi(vptr), self._pi(efr), *[_p(x) for x in a])
        if raw:
            return st
        self._chk(st)

    def debug_big_build(self, clouds, poses, gba_voxel_size, gba_min_eigen_value, gba_eig):
        """vba_debug_big_build: big_build on the clouds, as vba_hba_add_edge runs it for a window of another size -> (V, E)"""
        off, pnt = self._ragged(clouds)
        V = C.c_int(0); E = C.c_int(0)
        self._chk(self.lib.vba_debug_big_build(self.h, len(clouds), self._pi(off), _p(pnt), _p(_c(poses)), gba_voxel_size,
                                               gba_min_eigen_value, _p(_c(gba_eig)), C.byref(V), C.byref(E)))
        return V.value, E.value

    def debug_big_size(self):
        W = C.c_int(0); V = C.c_int(0); E = C.c_int(0)
        self._chk(self.lib.vba_debug_big_size(self.h, C.byref(W), C.byref(V), C.byref(E)))
        return W.value, V.value, E.value

    def debug_big_read(self):
        """vba_debug_big_read -> dict(W, vptr, efr, evox, eidx [V][W], ecl [E][10], eig_val, eig_vec, pcr_add) of the current store"""
        W, V, E = self.debug_big_size()
        vptr = np.zeros(V + 1, dtype=np.int32); efr = np.zeros(E, dtype=np.int32); evox = np.zeros(E, dtype=np.int32)
        eidx = np.zeros((V, W), dtype=np.int32); ecl = np.zeros((E, 10)); ev = np.zeros((V, 3)); evec = np.zeros((V, 9)); pa = np.zeros((V, 10))
        self._chk(self.lib.vba_debug_big_read(self.h, self._pi(vptr), self._pi(efr), self._pi(evox), self._pi(eidx), _p(ecl), _p(ev), _p(evec), _p(pa)))
        return dict(W=W, vptr=vptr, efr=efr, evox=evox, eidx=eidx, ecl=ecl, eig_val=ev, eig_vec=evec, pcr_add=pa)

    def debug_big_hessian(self, poses, slices=0):
        """vba_debug_big_hessian: the Hessian pass of the any-window path at poses -> (H [6W][6W], g [6W], r, blockdiag [W][W][6])"""
        W = self.debug_big_size()[0]
        poses = _c(poses); n = 6 * W
        assert poses.size == 12 * W
        H = np.full((n, n), np.nan); g = np.full(n, np.nan); r = C.c_double(np.nan); bd = np.full((W, W, 6), np.nan)
        self._chk(self.lib.vba_debug_big_hessian(self.h, _p(poses), slices, _p(H), _p(g), C.byref(r), _p(bd)))
        return H, g, r.value, bd

    def debug_big_residual(self, poses):
        """vba_debug_big_residual: the residual pass at poses (it rewrites the store's eigen-data and sums) -> r"""
        poses = _c(poses); r = C.c_double(np.nan)
        assert poses.size == 12 * self.debug_big_size()[0]
        self._chk(self.lib.vba_debug_big_residual(self.h, _p(poses), C.byref(r)))
        return r.value

    def pgo_optimize(self, poses, edges, priors, n_updates=6, relin_threshold=0.01):
        """build_graph + ISAM2 update() x n_updates + calculateEstimate() (VS:2078-2156, VS:2550-2561, VS:2769-2777):
        poses [n][12], edges [m][20] = i, j, rot(9), tra(3), var(6), priors [k][19] = k, R(9), p(3), var(6)
        -> (optimised poses [n][12], stats [n_updates][3] = relinearised nodes, cost at theta, max |delta|_inf)."""
        x = _c(poses).reshape(-1, 12).copy()
        e = _c(edges).reshape(-1, 20)
        pr = _c(priors).reshape(-1, 19)
        stats = np.zeros((max(int(n_updates), 1), 3))
        self._chk(self.lib.vba_pgo_optimize(self.h, len(x), _p(x), len(e), _p(e) if len(e) else None, len(pr),
                                            _p(pr) if len(pr) else None, int(n_updates), relin_threshold, _p(stats)))
        return x, stats

    def set_shard(self, rank, n_ranks):
        self._chk(self.lib.vba_set_shard(self.h, rank, n_ranks))

    def set_allreduce(self, pyfunc):
        """pyfunc(dev_ptr:int, n_doubles:int, stream:int) -> int; kept alive on the context."""
        def tramp(user, buf, n, stream):
            try:
                return int(pyfunc(buf, n, stream) or 0)
            except Exception:   # noqa: BLE001 - must not unwind through C
                import traceback
                traceback.print_exc()
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self._chk(self.lib.vba_set_allreduce(self.h, self._cb, None))

    def rccl_init(self, dist, rank, world):
        """Native exchange step: rank 0 makes an ncclUniqueId, torch.distributed (any backend) carries its 128 bytes to the other
        ranks, every rank builds the library's own RCCL communicator (vba_rccl_init also applies the voxel-bucket shard)."""
        buf = C.create_string_buffer(128)
        if rank == 0:
            self._chk(self.lib.vba_rccl_get_unique_id(buf))
        box = [bytes(buf.raw)]
        if world > 1:
            dist.broadcast_object_list(box, src=0)
        uid = C.create_string_buffer(box[0], 128)
        self._chk(self.lib.vba_rccl_init(self.h, uid, rank, world))

    def set_torch_allreduce(self, torch, dist):
        """torch.distributed SUM all-reduce (RCCL with backend "nccl", gloo in rehearsals) of the context's device buffers,
        ORDERED ON THE CONTEXT'S STREAM: the hook is handed the stream the kernels run on, and the collective is issued with
        that stream current.  (Issuing it on torch's default stream instead leaves it unordered against the context's own
        non-blocking stream: the sum then races with k_reduce_partials.)"""
        cache = {}
        streams = {}
        self.collective_calls = 0          # how many exchange steps the library asked for, and how many doubles they carried
        self.collective_doubles = 0

        def hook(ptr, n, stream):
            self.collective_calls += 1
            self.collective_doubles += int(n)
            key = (ptr, n)
            if key not in cache:
                class _Ext:
                    __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2, "strides": None}
                cache[key] = torch.as_tensor(_Ext(), device="cuda")
            skey = int(stream) if stream else 0
            if skey not in streams:                         # (the hook runs once per LM iteration: keep its host cost down)
                streams[skey] = torch.cuda.ExternalStream(skey) if skey else torch.cuda.default_stream()
            ext = streams[skey]
            if torch.cuda.current_stream() == ext:
                dist.all_reduce(cache[key], op=dist.ReduceOp.SUM)
            else:
                with torch.cuda.stream(ext):
                    dist.all_reduce(cache[key], op=dist.ReduceOp.SUM)
            return 0
        self.set_allreduce(hook)

    def timing_enable(self, on=True):
        self.lib.vba_timing_enable(self.h, int(on))

    def timing_calibration_read(self, n_bytes):
        self._chk(self.lib.vba_timing_calibration_read(self.h, n_bytes))

    def timing_select(self, name=None):
        self.lib.vba_timing_select(self.h, name.encode() if name else None)

    def timing_sample_every(self, n=1):
        self.lib.vba_timing_sample_every(self.h, int(n))

    def timing_launch_hessian(self):
        self._chk(self.lib.vba_timing_launch_hessian(self.h))

    def timing_null_spans(self, n=64):
        """Average duration in microseconds of an event pair that brackets nothing."""
        for _ in range(n):
            self.lib.vba_timing_null_span(self.h)
        t, k = self.timing_get("null")
        return t / max(k, 1)

    def timing_reset(self):
        self.lib.vba_timing_reset(self.h)

    def timing_get(self, name):
        tot = C.c_double(); cnt = C.c_int()
        self.lib.vba_timing_get(self.h, name.encode(), C.byref(tot), C.byref(cnt))
        return tot.value, cnt.value
