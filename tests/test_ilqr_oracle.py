"""CPU tests of the iLQR step's fp64 oracle (tests/ilqr_oracle.py): the loop of Riccati line searches with the closed-loop candidates,
k = 4, no disturbance, penyaw reward, on
  hover_03   make_problem(seed=17, time=37), hover + 0.3 noise   (choices 19, 23, 21, 20: closed-loop commits throughout)
  far_fast   the state atlas' entry of that name, hover mean     (choices 17, 17, 21, 6)
and, k = 2, on the input the GPU test of the fixed point uses (tests/test_gpu_ilqr.py):
  rest       at rest 1 cm beside the hovering task's target, identity attitude, hover mean: the sweep succeeds on rung 0 and no
             candidate is cheaper -- choice 0 from iteration 0, unflagged.

1. the costs chain: base[j + 1] == chosen[j] exactly -- the committed candidate is the next iteration's candidate 0 under one objective;
2. the costs are non-increasing, and strictly decreasing wherever something was committed;
3. after a choice 0 nothing moves; on `rest` that is the whole step.
"""
import functools

import numpy as np
import pytest

from oracle import ref_np as R
from tests import ilqr_oracle as IO
from tests.conftest import make_problem
from tests.state_atlas import atlas_state

K = 4


@functools.lru_cache(maxsize=None)
def _run(name):
    if name == "hover_03":
        s, p, rng = make_problem(seed=17, time=37)
        b = (R.hover_action(p, 32, np.float64) + 0.3 * rng.normal(size=(32, 4))).astype(np.float32).reshape(-1)
        k = K
    elif name == "far_fast":
        s, p, _ = atlas_state("far_fast")
        b = R.hover_action(p, 32, np.float64).astype(np.float32).reshape(-1)
        k = K
    else:
        s, p, b = IO.rest_case()
        k = 2
    means, its = IO.step(s, p, b, k)
    print(f"  {name}: choices {[i['choice'] for i in its]} rungs {[i['rung'] for i in its]} base {[i['base'] for i in its]} "
          f"chosen {[i['chosen'] for i in its]}")
    return s, p, means, its


@pytest.mark.parametrize("name", ["hover_03", "far_fast", "rest"])
def test_costs_chain_and_never_rise(name):
    s, p, means, its = _run(name)
    for j, it in enumerate(its):
        assert not it["flagged"] and np.isfinite(it["costs"]).all()
        assert it["chosen"] <= it["base"]
        assert (it["chosen"] < it["base"]) == (it["choice"] != 0)
        if j + 1 < len(its):
            assert its[j + 1]["base"] == it["chosen"], j  # exactly: the same sequence under the same objective
        # the committed mean is the chosen candidate: its own cost, evaluated alone, is the row's
        assert IO.plan_cost(s, p, means[j + 1])[0] == it["chosen"]


@pytest.mark.parametrize("name", ["hover_03", "far_fast", "rest"])
def test_after_a_choice_zero_nothing_moves(name):
    s, p, means, its = _run(name)
    choices = [it["choice"] for it in its]
    fixed = choices.index(0) if 0 in choices else len(its)
    for j in range(fixed, len(its)):
        assert its[j]["choice"] == 0 and means[j + 1].tobytes() == means[fixed].tobytes()
        assert its[j]["costs"].tobytes() == its[fixed]["costs"].tobytes()
    if name == "rest":
        assert fixed == 0 and its[0]["rung"] == 0  # the input of the GPU test's fixed-point check: stalled, not flagged
    else:
        assert all(c != 0 for c in choices[:fixed]) and fixed >= 1  # (the iterations before it moved)


def test_summary_is_its_definition():
    """IO.summary on hand-made rows: what the tally kernel's row holds"""
    rows = np.zeros((3, 8), dtype=np.float32)
    w = rows.view(np.int32)
    rows[:, 0], rows[:, 1], rows[:, 4] = (5.0, 4.0, 3.0), (4.0, 3.0, 3.0), (0.5, 0.25, 0.125)
    w[:, 2] = (19, 3, 0)
    w[:, 7] = (0x400, 0x500, 0x501)
    assert IO.summary(rows, 3) == (5.0, 3.0, 2, 2, 1, 0x400 | 0x500 | 0x501, 0.125)
    w[2, 2] = 7
    assert IO.summary(rows, 3)[2:5] == (3, 3, 1)
