"""CPU-only helpers between the product's host types and the oracle's (numpy and oracle/ alone: importable without torch or a GPU),
and the two error measures the tests' bars are stated in."""
import numpy as np

from oracle import ref_np as R


def oracle_state(ns):
    """ref_np.State (fp64) of a host env state (info["noisy_state"])"""
    return R.State(pos=ns.pos, vel=ns.vel, quat=ns.quat, omega=ns.omega, f_disturb=ns.f_disturb, pos_tar=ns.pos_tar,
                   vel_tar=ns.vel_tar, acc_tar=ns.acc_tar, time=ns.time, pos_traj=ns.pos_traj, vel_traj=ns.vel_traj,
                   acc_traj=ns.acc_traj).astype(np.float64)


def oracle_state_packed(packed, traj):
    """ref_np.State (fp64) from a packed float[32] state and the episode's (pos, vel, acc) trajectories"""
    st = np.asarray(packed, dtype=np.float32)
    return R.State(pos=st[0:3], vel=st[3:6], quat=st[6:10], omega=st[10:13], f_disturb=st[13:16], pos_tar=st[16:19],
                   vel_tar=st[19:22], acc_tar=st[22:25], time=int(st[25:26].view(np.int32)[0]), pos_traj=traj[0],
                   vel_traj=traj[1], acc_traj=traj[2]).astype(np.float64)


def oracle_params(params):
    """ref_np.Params of one domain-randomised instance (quadrotor.py:135-160 varies m, I, action_scale, alpha_bodyrate,
    disturb_params; I does not enter the body-rate model)."""
    return R.Params(m=float(params.m), action_scale=float(params.action_scale), alpha_bodyrate=float(params.alpha_bodyrate),
                    disturb_params=tuple(float(x) for x in params.disturb_params)).fp32()


def rel_err(x, ref):
    """|x - ref| / max(|ref|, 1) elementwise, in the arrays' own dtypes.  Not interchangeable with rel_err_scalar: for an fp32 x
    NumPy's promotion rules can leave the two a last bit apart."""
    return np.abs(x - ref) / np.maximum(np.abs(ref), 1.0)


def rel_err_scalar(x, ref):
    """The same measure of two scalars, both taken to Python floats first."""
    return abs(float(x) - float(ref)) / max(abs(float(ref)), 1.0)
