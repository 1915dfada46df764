"""CPU: the seeds tests/test_gpu_iters.py::test_two_pass_step_against_the_oracle fixes are ones for which the oracle's own fp32 and
fp64 runs of the 2-pass definition (tests/iters_oracle.py, composed from oracle/ref_np.py) pick the same best sample in both passes
-- so that test never has to excuse a case for a small top-2 gap."""
import numpy as np
import pytest

from tests import iters_oracle as IO


@pytest.mark.parametrize("name", list(IO.CASES))
def test_fp32_and_fp64_oracle_agree_on_the_best_sample_of_both_passes(name):
    import __graft_entry__ as g
    g.build()  # (the C oracle's rollout)
    env = IO.make_env(name, None)
    obs, info, state, key = IO.problem(env, IO.CASES[name]["seed"])
    ns = info["noisy_state"]
    c32 = IO.oracle_chain(name, env, ns, IO.hover_mean(env), key, 2, np.float32)
    c64 = IO.oracle_chain(name, env, ns, IO.hover_mean(env), key, 2, np.float64)
    for j, (a, b) in enumerate(zip(c32, c64)):
        gap = float(np.diff(np.sort(b[1])[:2])[0])
        print(f"{name} pass {j}: best sample fp32 {int(np.argmin(a[1]))} fp64 {int(np.argmin(b[1]))}, top-2 gap {gap:.3e}, "
              f"|mean32 - mean64| {np.abs(a[2] - b[2]).max():.2e}")
        assert int(np.argmin(a[1])) == int(np.argmin(b[1])), (name, j)
        assert gap > 1e-3  # (the gap below which test_batched_mode_step_against_the_oracle would excuse a lam = 0.01 case)
        assert np.abs(a[2] - b[2]).max() < 1e-5, (name, j)
    assert not np.array_equal(c64[0][0], c64[1][0])  # the second pass drew its own samples
