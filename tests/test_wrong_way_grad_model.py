"""The psi gradient of the wrong-way loss (include/tdship.h: tds_wrong_way_grad_f32), stated from the definition and checked on the
CPU: a float64 torch restatement of the loss for a given list of lanelet directions has, by autograd, the gradient -sin(delta) * [|delta| > thr] of
the lanelet that attains the minimum, and that is what central differences of the loss give.  The poses are Town01 poses drawn as
tests/test_lanelet2.py draws them; the directions come from the oracle (oracle/lanelet_oracle.py), which shares no code with the product.
In the reference the position passes through float() and is a constant, the directions are host floats, and `agent_state[2]` stays a tensor:
psi is the only input the loss can be differentiated to.  CPU only."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import lanelet_oracle as lo
from torchdrivesim_amd import lanelet2 as L
from test_lanelet2 import _agents

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
H = 1e-6                 # the step of the central differences
BOUND = 1e-6             # the bar of the other models
LEFT_OUT_CAP = 0.01
CASES = ((math.pi / 2, 1.0), (2.0, 0.25))


def loss64(directions, psi, thr):
    """the reference's loss for one agent in float64 torch: directions (n,) tensor, psi a 0-d tensor -> 0-d tensor"""
    delta = torch.remainder(directions - psi + math.pi, 2 * math.pi) - math.pi
    return (-torch.cos(delta) * (delta.abs() > thr).to(delta.dtype)).min()


def stated_gradient(directions, psi, thr):
    """-sin(delta) * [|delta| > thr] of the first lanelet that attains the minimum (normalize_angle has derivative 1; d delta / d psi = -1 and
    d (-cos delta) / d delta = sin delta) -> (loss, derivative, index of the winner), plain floats"""
    best, grad, win = None, 0.0, -1
    for i, d in enumerate(directions):
        delta = math.fmod(d - psi + math.pi, 2 * math.pi)
        delta = (delta + 2 * math.pi if delta < 0 else delta) - math.pi
        over = abs(delta) > thr
        l = -math.cos(delta) if over else 0.0
        if best is None or l < best:
            best, grad, win = l, (-math.sin(delta) if over else 0.0), i
    return best, grad, win


@pytest.fixture(scope='module')
def poses():
    """(x, y, psi, directions per (thr, tol)) for the Town01 poses of seeds 3 and 4, B = 2, A = 48, where the oracle finds a lanelet"""
    town01 = L.load_lanelet_map(os.path.join(GOLD, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    oracle = lo.load_osm(os.path.join(GOLD, 'carla_Town01.osm.gz'), origin=(0.0, 0.0))
    cls = oracle.centerlines()
    out = {case: [] for case in CASES}
    for seed in (3, 4):
        state = _agents(town01, 2, 48, seed).reshape(-1, 4)
        for x, y, psi, _ in state:
            if not (np.isfinite(x) and np.isfinite(y)):
                continue
            for thr, tol in CASES:
                try:
                    dirs = lo.find_lanelet_directions(oracle.laneletLayer, cls, float(x), float(y), ('parking',), tol)
                except lo.LaneletError:
                    continue
                if dirs:
                    out[(thr, tol)].append((float(psi), [float(d) for d in dirs]))
    return out


@pytest.mark.parametrize('case', CASES)
def test_autograd_of_the_loss_is_the_stated_gradient_and_central_differences_agree(poses, case):
    """-cos is smooth: a central difference at h = 1e-6 is off by h^2 / 6 = 2e-13, rounding adds 1e-16 / h = 1e-10.  The loss itself jumps where
    |delta| crosses the threshold and kinks where two lanelets' losses cross: a probe is left out only where the winner or its side of the
    threshold differs between psi - h and psi + h, and the share of such probes is capped."""
    thr, tol = case
    made = left_out = positive = several = 0
    worst_auto = worst_diff = 0.0
    for psi, dirs in poses[case]:
        d = torch.tensor(dirs, dtype=torch.float64)
        p = torch.tensor(psi, dtype=torch.float64, requires_grad=True)
        loss = loss64(d, p, thr)
        loss.backward()
        want_loss, want, win = stated_gradient(dirs, psi, thr)
        assert abs(float(loss.detach()) - want_loss) <= 1e-15
        made += 1
        positive += want_loss > 0
        several += len(dirs) > 1
        lo_, hi_ = stated_gradient(dirs, psi - H, thr), stated_gradient(dirs, psi + H, thr)
        if not (lo_[2] == hi_[2] == win and (lo_[1] != 0) == (hi_[1] != 0) == (want != 0)):
            left_out += 1
            continue
        # where several lanelets tie at the minimum exactly (two zeros), torch.min spreads or picks: the stated rule is the first -- both are 0 there
        worst_auto = max(worst_auto, abs(float(p.grad) - want))
        worst_diff = max(worst_diff, abs((hi_[0] - lo_[0]) / (2 * H) - want))
    print(f'thr {thr:.4f}, tol {tol}: {made} poses ({positive} with a positive loss, {several} within tolerance of several lanelets), {left_out} left out, '
          f'autograd against the stated gradient {worst_auto:.3g}, central differences {worst_diff:.3g} (bound {BOUND:g})')
    assert made >= 120 and positive >= 30 and several >= 40
    assert left_out <= LEFT_OUT_CAP * made and worst_auto <= 1e-12 and worst_diff <= BOUND


def test_hand_cases():
    """one lanelet along pi / 4 (the reference's known-answer map): against the lane the loss is 1 and the derivative -sin(pi) = 0; at
    pi / 4 + 2.5 the angle is -2.5, the loss -cos(2.5) and the derivative -sin(-2.5); along the lane both are 0; the first of equal losses wins"""
    d = [math.pi / 4]
    l, g, _ = stated_gradient(d, 5 * math.pi / 4, math.pi / 2)
    assert abs(l - 1) <= 1e-15 and abs(g) <= 1e-15
    l, g, _ = stated_gradient(d, math.pi / 4 + 2.5, math.pi / 2)
    assert abs(l + math.cos(2.5)) <= 1e-15 and abs(g - math.sin(2.5)) <= 1e-15 and g > 0.5
    assert stated_gradient(d, math.pi / 4 + 0.3, math.pi / 2)[:2] == (0.0, 0.0)
    assert stated_gradient([0.0, 0.0], 2.5, math.pi / 2)[2] == 0
    l, g, win = stated_gradient([0.3, 3.0], 0.0, math.pi / 2)          # -cos(3) = 0.99 loses to the 0 of the lane the agent follows
    assert (l, g, win) == (0.0, 0.0, 0)
