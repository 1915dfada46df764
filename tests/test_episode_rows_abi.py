"""CPU: the ABI of the episode logs of the step attachments' rows (covo_set_episode_rows, include/covo_hip.h: COVO_HAS_EPISODE_ROWS)
and their Python surface: EPISODE_LOGS, the episodes' read_* and eval_env_batched(rows=)."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)

KINDS = ("LAM", "ELITE", "ITERS", "SIGMA", "POST_AUX", "POST_COV")
NAMES = ("diag_log", "trace", "fanlog", "arblog", "lamlog", "elitelog", "iterlog", "sigmalog", "postlog", "postcovlog")


def test_the_entry_point_exists_with_the_declared_types(built):
    lib = built.load_library()
    hdr = header_text()
    assert re.search(r"#define COVO_HAS_EPISODE_ROWS 1\b", hdr) and built.COVO_HAS_EPISODE_ROWS == 1
    for k, name in enumerate(KINDS):
        assert int(re.search(r"#define COVO_EPLOG_%s\s+(\d+)" % name, hdr).group(1)) == k == getattr(built, "COVO_EPLOG_" + name)
    assert int(re.search(r"#define COVO_EPLOG_KINDS\s+(\d+)", hdr).group(1)) == 6 == built.COVO_EPLOG_KINDS
    assert int(re.search(r"#define COVO_SIGMA_LOG_FLOATS\s+(\d+)", hdr).group(1)) == 4 == built.COVO_SIGMA_LOG_FLOATS
    assert built.SIGMA_LOG_FIELDS == ("age", "fallback", "scale", "logdet")
    assert re.search(r"\bint covo_set_episode_rows\(covo_handle_t h, int32_t kind, float \*log, int32_t stride\);", hdr)
    fn = lib.covo_set_episode_rows  # the built library exports it
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    assert "covo_set_episode_rows" in built.EXPORTS
    # the ABI version did not move: the symbol is additive
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == 10 == built.ABI_VERSION == lib.covo_abi_version()
    # a null handle is refused before anything else happens (no GPU needed)
    assert lib.covo_set_episode_rows(None, 0, None, 0) != 0 and b"null handle" in lib.covo_last_error()


def test_core_and_episodes_hold_the_same_ten_logs(built):
    from covo_mpc_amd.controllers._core import EPISODE_LOGS
    from covo_mpc_amd.envs.quadrotor import BatchedDeviceEpisode, DeviceEpisode, _EpisodeLogs
    assert tuple(EPISODE_LOGS) == NAMES == tuple(_EpisodeLogs.LOGS)
    kinds = {name: entry[3] for name, entry in EPISODE_LOGS.items()}
    assert [kinds[n] for n in NAMES[:4]] == [None] * 4                     # the four logs with setters of their own
    assert [kinds[n] for n in NAMES[4:]] == list(range(6))                 # one kind each, in the header's order
    assert all(entry[1] == "covo_set_episode_rows" for name, entry in EPISODE_LOGS.items() if kinds[name] is not None)
    assert [n for n, entry in EPISODE_LOGS.items() if entry[4] is not None] == ["postcovlog"]  # the one opt-in log
    for cls in (DeviceEpisode, BatchedDeviceEpisode):
        p = inspect.signature(cls.__init__).parameters
        assert p["log_post_cov"].default is False, cls
        for read in ("read_lam", "read_elite", "read_iters", "read_sigma", "read_post"):
            assert callable(getattr(cls, read)), (cls, read)
    # every fixed row width is the header's
    for name, (width, _, _, _) in _EpisodeLogs.LOGS.items():
        assert width is None and name == "iterlog" or isinstance(getattr(built, width), int), name
    assert built.COVO_POST_COV_FLOATS == 128 * 128


@pytest.mark.parametrize("read, option", [("read_lam", "ess_min"), ("read_elite", "elite"), ("read_iters", "iters"),
                                          ("read_sigma", "sigma_period"), ("read_post", "compute_post_cov")])
def test_reading_a_log_that_was_never_filled_names_the_option(built, read, option):
    from covo_mpc_amd.envs.quadrotor import DeviceEpisode, _EpisodeLogs

    class Standin(_EpisodeLogs):
        log, n_steps = None, 0

    ep = Standin()
    for name in _EpisodeLogs.LOGS:
        setattr(ep, name, None)
    with pytest.raises(RuntimeError, match=option):
        getattr(ep, read)()
    assert getattr(DeviceEpisode, read) is getattr(_EpisodeLogs, read)


def test_the_splits_view_words_as_integers(built):
    from covo_mpc_amd.envs import quadrotor as q
    rows = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    rows[..., 0] = np.array([0x7FC00123], dtype=np.uint32).view(np.float32)[0]  # a NaN with a payload: the word survives
    el = q.split_elite_rows(rows)
    assert tuple(el) == built.ELITE_FIELDS and el["threshold_cost_word"].dtype == np.uint32 == el["threshold_index_word"].dtype
    assert np.all(el["threshold_cost_word"] == 0x7FC00123) and el["cost_min"].shape == (2, 3)
    lam = q.split_lam_rows(rows[..., :4])
    assert tuple(lam) == built.LAM_FIELDS and lam["ess_lam0"].shape == (2, 3)
    sg = q.split_sigma_rows(np.array([[2.0, 1.0, 0.5, -3.0]], dtype=np.float32))
    assert tuple(sg) == built.SIGMA_LOG_FIELDS and sg["age"].dtype == np.int32 and sg["age"][0] == 2 and sg["logdet"][0] == -3.0
    post = q.split_post_rows(np.zeros((4, 132), dtype=np.float32))
    assert post["shift"].shape == (4, 128) and post["weight"].shape == (4,)


def test_eval_env_batched_takes_rows(built):
    from covo_mpc_amd.envs.quadrotor import eval_env_batched
    p = inspect.signature(eval_env_batched).parameters
    assert p["rows"].default is False
    assert "ess_min" not in p and "compute_post_cov" not in p
