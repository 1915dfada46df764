"""The definition of a k-pass control step composed from oracle/ref_np.py alone (no csrc/): shared by tests/test_gpu_iters.py (the
device against it) and tests/test_iters_oracle_seeds.py (CPU: the fixed seeds are ones for which the oracle's own fp32 and fp64 runs
pick the same best sample in every pass).

    start_0 = shift_mean(a_mean); key_0 = rng_act
    pass j:  act_key = split(key_j)[1]; step_key = split(split(key_j)[0])[1]; eps = philox normal(act_key)
             a = sample_actions_*(start_j, a_cov, eps); cost = rollout(a); start_{j+1} = softmax_update(cost, a, lam, gamma, start_j)
             key_{j+1} = split(split(key_j)[0])[0]
"""
import numpy as np

from covo_mpc_amd import random as cr
from oracle import c_oracle as CO
from oracle import ref_np as R
from oracle import rng_np

H, LAM, GAMMA, SIGMA = 32, 0.01, 0.8, 0.5
CASES = {"mppi": dict(N=1024, task="hovering", seed=0), "covo-offline": dict(N=2048, task="tracking_zigzag", seed=0)}


def make_env(name, device):
    import covo_mpc_amd as cm
    return cm.envs.Quad3D(task=CASES[name]["task"], enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                          generate_noisy_state=True, device=device)


def problem(env, seed):
    """-> (obs, info, state, raw key of the step) of the case's seed"""
    obs, info, state = env.reset(cr.PRNGKey(1000 + seed), env.default_params)
    return obs, info, state, np.asarray(cr.PRNGKey(2000 + seed))


def oracle_state(ns):
    return R.State(pos=ns.pos, vel=ns.vel, quat=ns.quat, omega=ns.omega, f_disturb=ns.f_disturb, pos_tar=ns.pos_tar,
                   vel_tar=ns.vel_tar, acc_tar=ns.acc_tar, time=ns.time, pos_traj=ns.pos_traj, vel_traj=ns.vel_traj,
                   acc_traj=ns.acc_traj).astype(np.float64)


def offline_sigma():
    """covo-offline's table row for these cases: a fixed dense SPD matrix known without a device (the controller's own table needs
    its reset on the GPU), of MPPI's scale: sigma^2 (0.6 I + B B^T), B = 0.05 x a seeded gaussian matrix.  float32, as the table is."""
    B = 0.05 * np.random.default_rng(7).standard_normal((H * 4, H * 4))
    return (SIGMA ** 2 * (0.6 * np.eye(H * 4) + B @ B.T)).astype(np.float32)


def hover_mean(env):
    dp = env.default_params
    th = np.float32((dp.m * dp.g / dp.max_thrust) * 2.0 - 1.0)
    return np.tile(np.array([th, 0.0, 0.0, 0.0], dtype=np.float32), (H, 1))


def next_raw_key(key):
    return cr.split(cr.split(key)[0])[0]


def pass_inputs(name, env, raw_key, N):
    """the pass's epsilon [N, 128] (Philox normal of act_key, oracle/rng_np.py) and shared disturbance vector"""
    rest, act_key = cr.split(raw_key)
    _, step_key = cr.split(rest)
    eps = rng_np.randn(int(act_key[0]), int(act_key[1]), 0, N, H * 4).astype(np.float32)
    fs = np.zeros(3)
    if name == "mppi":  # mppi.py:69,74: one shared non-deterministic draw for every sample and step
        fs = np.asarray(env.rollout_disturbance(step_key, env.default_params, deterministic=False), dtype=np.float64)
    return eps, fs


def oracle_pass(name, env, so, start, raw_key, N, dtype):
    """one pass in `dtype` around `start` [H, 4] -> (actions [N, H, 4], costs [N], new mean [H, 4])"""
    eps, fs = pass_inputs(name, env, raw_key, N)
    start = np.asarray(start, dtype=dtype)
    if name == "mppi":
        a_cov = np.tile((SIGMA ** 2 * np.eye(4)).astype(dtype), (H, 1, 1))
        a, _ = R.sample_actions_blockdiag(start, a_cov, eps.reshape(N, H, 4).astype(dtype))
    else:
        a, _ = R.sample_actions_full(start, offline_sigma().astype(dtype), eps.astype(dtype))
    po = R.Params().fp32()
    cost = CO.rollout(so.astype(dtype), po, a, 1.0, fs.astype(dtype), dtype=dtype)
    mean, _ = R.softmax_update(cost.astype(dtype), a, LAM, GAMMA, start)
    return a, cost, mean


def oracle_chain(name, env, ns, a_mean, raw_key, k, dtype):
    """the k passes of the definition in `dtype` -> per pass (actions, costs, new mean)"""
    so, N = oracle_state(ns), CASES[name]["N"]
    start, key, out = R.shift_mean(np.asarray(a_mean, dtype=dtype).reshape(H, 4)), np.asarray(raw_key), []
    for _ in range(k):
        out.append(oracle_pass(name, env, so, start, key, N, dtype))
        start, key = out[-1][2], next_raw_key(key)
    return out
