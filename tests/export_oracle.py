"""Plain-Python/numpy restatement of ResultOutput::pub_globalmap (voxelslam.cpp:110-154) for the tests of vba_kf_export_plan and
vba_kf_export_world: which points of which keyframes are exported, where the messages are cut, and the exported values.  TEST
INFRASTRUCTURE only, written from the reference's loop.

Two deliberate differences from the reference, both stated in include/voxelba.h: psize is summed without the 32-bit wrap, and the
empty publish that clears the display (VS:113) is not a message of the plan.
"""
import numpy as np

import kf_oracle as ko


def plan(sizes, interval_size, jump=0):
    """(jump in force, kf_begin [n_kf + 1], msg_end_kf [n_msgs]) of the keyframe sizes in publication order: the double loop of
    VS:126-153 with a running pl_size in place of the cloud."""
    sizes = [int(s) for s in sizes]
    if jump == 0:
        psize = 0
        for s in sizes:                                       # VS:118-123
            psize += s
        jump = psize // (10 * int(interval_size)) + 1         # VS:124
    kf_begin, msg_end = [0], []
    pl_size = 0
    for i, size in enumerate(sizes):                          # VS:130
        j = pushed = 0
        while j < size:                                       # VS:133
            pl_size += 1                                      # VS:142
            pushed += 1
            j += jump
        kf_begin.append(kf_begin[-1] + pushed)
        if pl_size > interval_size:                           # VS:145
            msg_end.append(i + 1)                             # VS:147
            pl_size = 0                                       # VS:149
    msg_end.append(len(sizes))                                # VS:153
    return jump, np.array(kf_begin, dtype=np.int64), np.array(msg_end, dtype=np.int32)


def points(clouds, poses, intensities, jump):
    """float32 [n][4] records x y z intensity: clouds[k] [n_k][3] is keyframe k's plptr (float values), poses[k] its x0 [12],
    intensities[k] its session's id; every keyframe's stride starts at its own point 0 (VS:133), world = x0.R p + x0.p in the
    order of kf_oracle.world, each coordinate narrowed to float once (VS:139-141)."""
    out = []
    for c, x, it in zip(clouds, poses, intensities):
        c = np.asarray(c, dtype=np.float64).reshape(-1, 3)[::jump]
        w = ko.world(x, c).astype(np.float32)
        out.append(np.concatenate([w, np.full((len(w), 1), it, dtype=np.float32)], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 4), np.float32)
