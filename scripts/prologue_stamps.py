#!/usr/bin/env python
"""Entry-to-first-work stamps of the Hessian's KC / KD launches and of merge_kernel: a few eager covo-online steps at N (default
65536) on a library built with -DKC_STAMPS -DKD_PROF (hessian_adj.hip) and -DMERGE_STAMPS (reduce.hip); the kernels print their
own lines (KC, merge: 10 ns wall-clock ticks from the workgroup's entry; KD: shader-clock cycles per phase).
    COVO_HIP_LIB=<that library> COVO_NO_GRAPH=1 python scripts/prologue_stamps.py [N]"""
import os, sys
os.environ.setdefault("COVO_NO_GRAPH", "1")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import covo_mpc_amd as cm
from covo_mpc_amd import random as cr

N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
env = cm.envs.Quad3D(task="tracking_zigzag", enable_randomizer=False, disturb_type="gaussian", disable_rollover_terminate=True,
                     generate_noisy_state=True, device="cuda:0")
c, _ = cm.envs.get_controller(env, "covo-online", f"N{N}_H32_lam0.01", device="cuda:0", compute_info=False)
params = env.default_params
obs, info, state = env.reset(cr.PRNGKey(1), params)
cp = c.reset(state, params, c.init_control_params, cr.PRNGKey(2))
key = cr.PRNGKey(3)
for step in range(12):
    key, k_act, k_step = cr.split(key, 3)
    u, cp, _ = c(obs, state, params, k_act, cp, info)
    torch.cuda.synchronize()
    print(f"-- step {step} done", flush=True)
    obs, state, reward, done, info = env.step(k_step, state, u.cpu().numpy(), params)
