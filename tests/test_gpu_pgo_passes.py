"""The passes of vba_pgo_optimize on the device, one update read back pass by pass through vba_debug_pgo_step (the production plan,
upload and launches), against tests/pgo_ref.py: the counted per-entry bars that the g++ build of the same header meets in
tests/test_pgo_ref_cpu.py.  No bar is formed from what the device returns.
  * linearise: slot[300][121] within k u M per entry, M = 0 entries exactly 0; sub-calls of 1, 255, 256, 257 factors give the same bits;
  * cost: bit for bit numpy's replay of k_pgo_cost's order over the returned slots;
  * assemble: blk and g bit for bit the in-order sums of the returned slots;
  * solve: dx against the system (H, -g) of the device's own blk, g with solve_ref's exact residuals and bars, on the smallest graphs
    that reach each path of the plan and of the elimination;
  * retraction: poses_out against theta (+) Exp(dx) of the device's own dx in the closed-form branch; vba_pgo_optimize(n_updates = 1)
    returns the same bits.
Measured on an MI355X (information, not bars): slots worst error / bar 0.021; solve backward / forward ratio at most 0.010 / 0.016
(skel1); retraction 0.053.  DESIGN.md §2, "What pins the pose-graph passes", lists them per class and per graph."""
import numpy as np
import pytest

import pgo_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import voxel_slam_amd  # noqa: F401
    from voxel_slam_amd import capi
    o = capi.default_options()
    o.device = 0
    c = capi.Context(o)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lin(ctx):
    inp, ref = R.lin_ref()
    keep = [a.copy() for a in inp]
    dev = ctx.debug_pgo_step(*inp)
    assert all(np.array_equal(a, b) for a, b in zip(inp, keep))                 # the caller's arrays are left as given
    return inp, ref, dev


def test_reference_the_device_is_held_to(lin):
    _, ref, _ = lin
    assert ref.margins() == [] and ref.branch_consistent() == []
    assert ref.counts() == R.COUNTS and R.taylor_truncation() == R.TRUNC


def test_linearise_within_bars(lin):
    _, ref, dev = lin
    ratio, bad = ref.check(dev["slot"])
    for a in range(len(R.ANGLES)):
        print("angle %-12.6g worst err / bar %.3g" % (R.ANGLES[a], max(ratio[f] for f in range(300) if R.lin_classes(f)[0] == a)))
    for t in range(len(R.TRANS)):
        print("translation %-6g worst err / bar %.3g" % (R.TRANS[t], max(ratio[f] for f in range(300) if R.lin_classes(f)[1] == t)))
    assert bad == []


@pytest.mark.parametrize("F", (1, 255, 256, 257))
def test_linearise_does_not_depend_on_the_launch(ctx, lin, F):
    inp, _, dev = lin
    p, e, q, idx = R.lin_subcall(inp, F)
    got = ctx.debug_pgo_step(p, e, q)["slot"]
    assert got.shape == (F, 121) and np.array_equal(got, dev["slot"][idx])


def test_cost_is_the_fixed_tree(lin):
    _, _, dev = lin
    assert dev["cost"] == R.replay_cost(dev["slot"])


def test_assembly_is_the_in_order_sum(lin):
    _, ref, dev = lin
    pairs, blk, g = R.replay_assemble(dev["slot"], ref.fi, ref.fj, 200)
    assert len(blk) == 300                                                       # a second workgroup of k_pgo_assemble
    assert np.array_equal(dev["pairs"], pairs) and np.array_equal(dev["blk"], blk) and np.array_equal(dev["g"], g)


@pytest.mark.parametrize("name", sorted(R.solve_graphs()))
def test_solve_within_bars(ctx, name):
    Y, ed, pr = R.solve_graphs()[name]
    n = len(Y)
    dev = ctx.debug_pgo_step(Y, ed, pr)
    _, blk, g = R.replay_assemble(dev["slot"], ed[:, 0].astype(int).tolist() + pr[:, 0].astype(int).tolist(),
                                  ed[:, 1].astype(int).tolist() + [-1] * len(pr), n)
    assert np.array_equal(dev["blk"], blk) and np.array_equal(dev["g"], g)
    bw, fw, zeros = R.solve_ratios(dev["blk"], dev["g"], dev["pairs"], n, dev["dx"])
    print("%-12s backward ratio %.3g forward ratio %.3g" % (name, bw, fw))
    assert bw <= 1 and fw <= 1 and zeros


@pytest.mark.parametrize("k", range(len(R.RETRACT_ANGLES)))
def test_retraction_within_bars(ctx, k):
    X, ed, pr = R.retract_graphs()[k]
    dev = ctx.debug_pgo_step(X, ed, pr)
    v, bar, cnt, taylor = R.retract_ref(X[0], dev["dx"][0])
    assert not taylor and cnt == R.K_RETRACT
    ratio = (v.err_to(dev["poses"][0]) / bar).max()
    print("prior %.1f rad away: |dx_w| %.3f, worst err / bar %.3g" % (R.RETRACT_ANGLES[k], np.linalg.norm(dev["dx"][0, :3]), ratio))
    assert ratio <= 1
    got, stats = ctx.pgo_optimize(X, ed, pr, 1, 0.01)
    assert np.array_equal(got, dev["poses"]) and stats[0, 1] == dev["cost"]


def test_one_update_of_the_production_call_gives_the_same_bits(ctx, lin):
    inp, _, dev = lin
    got, stats = ctx.pgo_optimize(*inp, 1, 0.01)
    assert np.array_equal(got, dev["poses"]) and stats[0, 1] == dev["cost"] and stats[0, 2] == np.abs(dev["dx"]).max()
