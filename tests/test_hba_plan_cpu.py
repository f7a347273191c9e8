"""The bottom-layer plan of vba_hba_global (csrc/vba_hba_plan.hpp) on the CPU: the window list with its lanes and chunk offsets, the
size and layout of d_hba_all, the one append loop of edge rows and the runner of the worker lanes.  tests/host/hba_plan_host.cpp is
built by g++ over the standard library alone, once with the address and undefined-behaviour sanitizers and once with the thread
sanitizer, and run as a child process, one case per run.  The plan is compared field by field with `restate` below, which is the
sizing arithmetic as vba_hba_global had it inline before the plan was taken out: it is the reference, not the header."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SANITIZERS = {"asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], "tsan": ["-fsanitize=thread"]}
CASES = ["append_shift", "append_lookup", "append_cap_exact", "append_cap_over", "append_empty",
         "upload_wanted", "lanes_ok", "lanes_stop", "lanes_bad_alloc", "lanes_runtime_error", "main_throws", "main_status"]
SEQUENTIAL, WORKERS, REPLICAS = 0, 1, 2


@pytest.fixture(scope="module", params=sorted(SANITIZERS))
def plan_host(request):
    out = os.path.join(tempfile.mkdtemp(prefix="vba_hba_plan_"), "hba_plan_host_" + request.param)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-pthread"] + SANITIZERS[request.param] + ["-o", out, os.path.join(HERE, "host", "hba_plan_host.cpp")])
    return out


def restate(n_kf, offsets, wdsize, mgsize, n_ranks, hba_workers):
    """the inline arithmetic of vba_hba_global, statement by statement (n_ranks: 1 without a collective)"""
    off = np.asarray(offsets, dtype=np.int64)
    starts = [s for s in range(0, max(n_kf, 0) + 1, mgsize) if s + wdsize <= n_kf]        # for (start = 0; start + wdsize <= n_kf; start += mgsize)
    nw = [int(off[s + wdsize] - off[s]) for s in starts]
    n_all, n_sub_cap, n_win_max, n_win = int(off[n_kf]), sum(nw), max(nw, default=0), len(starts)
    replicas = n_ranks > 1
    kl_opt = (hba_workers if hba_workers < 8 else 8) if hba_workers > 0 else 4
    KL = kl_opt if (not replicas and n_win >= 2 * kl_opt) else 1
    local_rep = KL > 1
    chunked = replicas or local_rep
    NR = n_ranks if replicas else KL
    meta_per = 3 + (wdsize * (wdsize - 1) // 2) * 20
    win_per_rank = (n_win + NR - 1) // NR if chunked else 0
    meta_chunk = meta_per * win_per_rank
    rank_cap, win_roff = [0] * NR, [0] * max(n_win, 1)
    if chunked:
        for w in range(n_win):
            win_roff[w] = rank_cap[w % NR]
            rank_cap[w % NR] += nw[w]
    chunk_pts = max(rank_cap) if chunked else 0
    need = (n_all + n_sub_cap + NR * chunk_pts) * 3 + NR * meta_chunk + 64
    off_sub = n_all * 3
    off_rep = off_sub + n_sub_cap * 3
    off_meta = off_rep + NR * chunk_pts * 3
    fields = dict(mode=REPLICAS if replicas else WORKERS if local_rep else SEQUENTIAL, n_win=n_win, KL=KL, NR=NR, n_all=n_all, n_sub_cap=n_sub_cap,
                  n_win_max=n_win_max, chunk_pts=chunk_pts, meta_per=meta_per, win_per_lane=win_per_rank, meta_chunk=meta_chunk, meta_len=NR * meta_chunk, need=need,
                  off_sub=off_sub, off_rep=off_rep, off_meta=off_meta)
    # start, lane, slot, points, offset inside the lane's chunk, record index meta[(w % NR) * meta_chunk + meta_per * (w / NR)]
    wins = [(starts[w], w % NR, w // NR, nw[w], win_roff[w], (w % NR) * meta_chunk + meta_per * (w // NR) if chunked else -1) for w in range(n_win)]
    return fields, wins, [r * meta_chunk for r in range(NR)]


def run_plan(exe, n_kf, offsets, wdsize, mgsize, n_ranks, hba_workers):
    r = subprocess.run([exe, "plan"] + [str(int(v)) for v in [n_kf, wdsize, mgsize, n_ranks, hba_workers] + list(offsets)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    fields, wins, lanes = {}, [], []
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "win":
            wins.append(tuple(int(v) for v in t[1:]))
        elif t[0] == "lane_recs":
            lanes.append(int(t[1]))
        else:
            fields[t[0]] = int(t[1])
    return fields, wins, lanes


def uniform(n_kf, pts=100):
    return [pts * i for i in range(n_kf + 1)]


def windows(n_win, wdsize=10, mgsize=5):
    """the keyframe count that gives exactly n_win windows"""
    return wdsize + (n_win - 1) * mgsize if n_win > 0 else wdsize - 1


def ragged(n_kf, seed, empty_every=4):
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 5000, n_kf)
    n[::empty_every] = 0                                  # empty keyframes
    return [0] + [int(v) for v in np.cumsum(n)]


PLAN_CASES = {
    "fewer_keyframes_than_a_window": (9, uniform(9), 10, 5, 1, 0),
    "no_keyframes": (0, [0], 10, 5, 1, 0),
    "exactly_one_window": (10, uniform(10), 10, 5, 1, 0),
    "two_ranks_7_windows": (windows(7), uniform(windows(7), 37), 10, 5, 2, 0),
    "three_ranks_7_windows": (windows(7), uniform(windows(7), 41), 10, 5, 3, 0),
    "three_ranks_one_window": (10, uniform(10), 10, 5, 3, 0),          # fewer windows than ranks
    "two_ranks_many_windows_no_workers": (windows(20), uniform(windows(20)), 10, 5, 2, 2),
    "ragged_with_empty_keyframes": (63, ragged(63, 1), 10, 5, 1, 0),
    "ragged_two_ranks": (38, ragged(38, 2), 10, 5, 2, 0),
    "ragged_stride_3_window_4": (29, ragged(29, 3, 3), 4, 3, 1, 2),
    # keyframes 10..19 are empty: window 2 of (wdsize 10, mgsize 5) has no point at all
    "one_window_of_zero_points": (50, [100 * min(i, 10) for i in range(21)] + [1000 + 70 * i for i in range(1, 31)], 10, 5, 1, 2),
    "one_window_of_zero_points_three_ranks": (50, [100 * min(i, 10) for i in range(21)] + [1000 + 70 * i for i in range(1, 31)], 10, 5, 3, 0),
    "stride_larger_than_the_window": (61, ragged(61, 4, 7), 4, 9, 1, 2),
    "stride_larger_than_the_window_two_ranks": (61, ragged(61, 5, 7), 4, 9, 2, 0),
    "small_gpu_test_shape": (25, uniform(25, 6000), 10, 5, 1, 2),
}


@pytest.mark.parametrize("name", sorted(PLAN_CASES))
def test_plan_equals_the_inline_arithmetic(plan_host, name):
    args = PLAN_CASES[name]
    fields, wins, lanes = run_plan(plan_host, *args)
    want_fields, want_wins, want_lanes = restate(*args)
    assert fields == want_fields
    assert wins == want_wins and lanes == want_lanes
    if args[4] > 1:
        assert fields["KL"] == 1 and fields["mode"] == REPLICAS and fields["NR"] == args[4]


@pytest.mark.parametrize("option,kl", [(0, 4), (1, 1), (2, 2), (8, 8), (9, 8)])
def test_worker_threshold(plan_host, option, kl):
    """n_win = 2 kl - 1: one window after the other; n_win = 2 kl: kl lanes"""
    for n_win, want in ((2 * kl - 1, 1), (2 * kl, kl)):
        args = (windows(n_win), uniform(windows(n_win), 53), 10, 5, 1, option)
        fields, wins, lanes = run_plan(plan_host, *args)
        assert (fields, wins, lanes) == restate(*args)
        assert fields["n_win"] == n_win and fields["KL"] == want and fields["mode"] == (WORKERS if want > 1 else SEQUENTIAL)
        two_ranks = run_plan(plan_host, *(args[:4] + (2, option)))[0]
        assert two_ranks["KL"] == 1 and two_ranks["mode"] == REPLICAS


@pytest.mark.parametrize("name", ["two_ranks_7_windows", "three_ranks_7_windows", "ragged_with_empty_keyframes", "stride_larger_than_the_window_two_ranks",
                                  "small_gpu_test_shape"])
def test_records_are_distinct_and_inside_the_chunks(plan_host, name):
    args = PLAN_CASES[name]
    fields, wins, _ = run_plan(plan_host, *args)
    NR, meta_chunk, meta_per = fields["NR"], fields["meta_chunk"], fields["meta_per"]
    assert fields["mode"] != SEQUENTIAL and len(wins) >= NR
    for lane in range(NR):
        own = [w for w in range(len(wins)) if wins[w][1] == lane]
        for w in (own[0], own[-1]):                   # the first and the last window of every lane
            assert wins[w][5] == (w % NR) * meta_chunk + meta_per * (w // NR)
            assert lane * meta_chunk <= wins[w][5] and wins[w][5] + meta_per <= (lane + 1) * meta_chunk
    recs = [w[5] for w in wins]
    assert len(set(recs)) == len(recs) and min(recs) >= 0 and max(recs) + meta_per <= NR * meta_chunk
    assert all(b - a >= meta_per for a, b in zip(sorted(recs), sorted(recs)[1:]))
    # a lane's clouds lie one behind the other inside its chunk
    for lane in range(NR):
        at = 0
        for w in wins:
            if w[1] == lane:
                assert w[4] == at
                at += w[3]
        assert at <= fields["chunk_pts"]


@pytest.mark.parametrize("case", CASES)
def test_append_and_runner(plan_host, case):
    r = subprocess.run([plan_host, case], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stderr == ""                     # no sanitizer report (no data race between the lanes and the uploader)


def test_unknown_case_is_an_error(plan_host):
    assert subprocess.run([plan_host, "no_such_case"], capture_output=True, timeout=60).returncode == 2
