"""CPU: check_step_switches (covo_mpc_amd/controllers/_options.py) held to the chain it replaced -- check_refine, check_riccati,
check_riccati_feedback, check_plan_hold, check_riccati_box called one after the other with an entry point's own names -- over a grid
of values, alone and through the entry points themselves."""
import itertools

GRID = dict(refine=(False, True, "no"), riccati=(False, True, 1), riccati_feedback=(False, True, None), plan_hold=(1, 3, 0, True),
            riccati_box=(False, True, "yes"), sigma_period=(1, 4), disturb_type=("gaussian", "drag"), sharded=(False, True))
BATCH = "the env-batched %s controller"
# the names each entry point hands to (check_refine, check_riccati, the other three), as its chain of five calls did
NAMES = {
    "SamplingCore": ("online", "a sampling core", "a sampling core"),
    "CoVOController online": ("online", "online", "covo-online"),
    "CoVOController offline": ("covo-offline", "covo-offline", "covo-offline"),
    "MPPIController": ("MPPI", "MPPI", "MPPI"),
    "BatchedCoVOController online": ("online", "online", "online"),
    "BatchedCoVOController offline": (BATCH % "covo-offline",) * 3,
    "get_controller mppi": ("mppi", "mppi", "mppi"),
    "get_controller covo-offline": ("covo-offline", "covo-offline", "covo-offline"),
    "get_controller covo-online": ("online", "online", "online"),
    "eval_env_batched covo-online": ("online", "online", BATCH % "covo-online"),
    "eval_env_batched mppi": ("mppi", BATCH % "mppi", BATCH % "mppi"),
    "eval_env_batched covo-offline": ("covo-offline", BATCH % "covo-offline", BATCH % "covo-offline"),
}


def _points(**fixed):
    axes = {k: ((fixed[k],) if k in fixed else v) for k, v in GRID.items()}
    return [dict(zip(axes, values)) for values in itertools.product(*axes.values())]


def _chain(names, refine, riccati, riccati_feedback, plan_hold, riccati_box, sigma_period, disturb_type, sharded):
    """The reference: the five calls as the entry points wrote them out -> ("ok", None, record) or (the check that objected, the
    exception's type, its message)."""
    from covo_mpc_amd.controllers import _options as o
    n_refine, n_riccati, n_rest = names
    calls = (
        ("refine", lambda: o.check_refine(refine, n_refine, sigma_period=sigma_period, sharded=sharded)),
        ("riccati", lambda: o.check_riccati(riccati, n_riccati, refine=refine, sharded=sharded)),
        ("riccati_feedback", lambda: o.check_riccati_feedback(riccati_feedback, riccati=riccati, disturb_type=disturb_type, what=n_rest)),
        ("plan_hold", lambda: o.check_plan_hold(plan_hold, riccati=riccati, sigma_period=sigma_period, disturb_type=disturb_type,
                                                what=n_rest)),
        ("riccati_box", lambda: o.check_riccati_box(riccati_box, riccati=riccati, what=n_rest)))
    got = {}
    for name, call in calls:
        try:
            got[name] = call()
        except Exception as e:  # noqa: BLE001 - the outcome under comparison
            return name, type(e), str(e)
    return "ok", None, o.StepSwitches(**got)


def _outcome(call):
    try:
        return "ok", None, call()
    except Exception as e:  # noqa: BLE001
        return "refused", type(e), str(e)


def test_check_step_switches_is_the_chain_of_five_over_the_grid():
    from covo_mpc_amd.controllers._options import STEP_SWITCH_DEFAULTS, check_step_switches
    points = _points()
    assert len(points) == 3 * 3 * 3 * 4 * 3 * 2 * 2 * 2 == 2592  # each under every distinct triple of names below
    seen = set()
    for names in sorted(set(NAMES.values())):
        n_refine, n_riccati, n_rest = names
        for pt in points:
            stage, want_type, want = _chain(names, **pt)
            switches = {k: pt[k] for k in STEP_SWITCH_DEFAULTS}
            _, got_type, got = _outcome(lambda: check_step_switches(
                n_rest, mode_what=n_refine, riccati_what=n_riccati, sigma_period=pt["sigma_period"], disturb_type=pt["disturb_type"],
                sharded=pt["sharded"], **switches))
            assert (got_type, got) == (want_type, want), (names, pt)
            seen.add(stage)
    assert seen == {"ok", *STEP_SWITCH_DEFAULTS}  # every one of the five objected somewhere, and something was accepted


def test_the_entry_points_refuse_what_the_chain_refuses():
    """Through get_controller, BatchedCoVOController and SamplingCore, on the points the chain refuses (an accepted one would go on to
    build a handle): the same exception with the same message, under that entry point's names."""
    import covo_mpc_amd as cm
    from covo_mpc_amd import controllers
    from covo_mpc_amd.controllers._core import SamplingCore
    from covo_mpc_amd.controllers._options import STEP_SWITCH_DEFAULTS
    from covo_mpc_amd.envs.quadrotor import get_controller
    envs = {d: cm.envs.Quad3D(task="tracking_zigzag", disturb_type=d, enable_randomizer=False, disable_rollover_terminate=True,
                              generate_noisy_state=True, device=None) for d in GRID["disturb_type"]}
    through = {
        "get_controller mppi": lambda env, sw: get_controller(env, "mppi", "N256_H32_lam0.01", device="cpu", **sw),
        "get_controller covo-offline": lambda env, sw: get_controller(env, "covo-offline", "N256_H32_lam0.01", device="cpu", **sw),
        "get_controller covo-online": lambda env, sw: get_controller(env, "covo-online", "N256_H32_lam0.01", device="cpu", **sw),
        "BatchedCoVOController online": lambda env, sw: controllers.BatchedCoVOController(env, 3, 256, 32, 0.01, **sw),
        "BatchedCoVOController offline": lambda env, sw: controllers.BatchedCoVOController(env, 3, 256, 32, 0.01, mode="offline", **sw),
        "SamplingCore": lambda env, sw: SamplingCore(256, 32, 0.01, 1.0, **sw),  # (no env: the disturbance is not known there)
    }
    seen, texts = set(), set()
    for entry, build in through.items():
        for pt in _points(sigma_period=1, sharded=False):
            known = dict(pt, disturb_type=None) if entry == "SamplingCore" else pt
            stage, want_type, want = _chain(NAMES[entry], **known)
            if stage == "ok":
                continue
            _, got_type, got = _outcome(lambda: build(envs[pt["disturb_type"]], {k: pt[k] for k in STEP_SWITCH_DEFAULTS}))
            assert (got_type, got) == (want_type, want), (entry, pt)
            seen.add(stage)
            texts.add(got)
    assert seen == set(STEP_SWITCH_DEFAULTS)  # every one of the five objected through an entry point
    # check_riccati's env-batched refusal, which the names above reach through the offline batch only
    assert any(t.startswith("riccati=True with the env-batched covo-offline controller: ") for t in texts)
