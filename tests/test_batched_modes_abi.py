"""CPU: the ABI of the batched step with a mode (covo_mpc_step_batched_mode / covo_run_episode_batched_mode, include/covo_hip.h):
the ctypes structs match the header's layout, the covo-online entry points keep their argument struct -- a zero-initialised
covo_batch_args as controllers/batched.py fills it still selects covo-online -- and header, library and binding agree on the
version.  No GPU call."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

from tests.abi_support import built, header_text  # noqa: F401  (built: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_layout(structs):
    """sizeof / offsetof of the header's structs as the C compiler sees them: {struct: {"sizeof": n, field: offset}}."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "covo_hip.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append(f'printf("{name} sizeof %zu\\n", sizeof({name}));')
        for f in fields:
            lines.append(f'printf("{name} {f} %zu\\n", offsetof({name}, {f}));')
    lines += ["return 0; }"]
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), src, "-o", exe])
        out = subprocess.check_output([exe], text=True)
    res = {}
    for ln in out.splitlines():
        s, f, v = ln.split()
        res.setdefault(s, {})[f] = int(v)
    return res


def test_batch_structs_match_header(built):
    base_fields = [n for n, _ in built.BatchArgsC._fields_]
    mode_fields = [n for n, _ in built.BatchModeArgsC._fields_]
    lay = _header_layout({"covo_batch_args": base_fields, "covo_batch_mode_args": mode_fields})
    assert ctypes.sizeof(built.BatchArgsC) == lay["covo_batch_args"]["sizeof"] == 88  # unchanged by the mode entries
    for f in base_fields:
        assert getattr(built.BatchArgsC, f).offset == lay["covo_batch_args"][f], f
    assert ctypes.sizeof(built.BatchModeArgsC) == lay["covo_batch_mode_args"]["sizeof"] == 120
    for f in mode_fields:
        assert getattr(built.BatchModeArgsC, f).offset == lay["covo_batch_mode_args"][f], f
    # no hole the library's cache key could read garbage from: the fields tile the struct
    assert built.BatchModeArgsC.base.offset == 0 and built.BatchModeArgsC.mode.offset == 88
    assert built.BatchModeArgsC.pad_.offset + 4 == 120


def test_zeroed_batch_args_still_mean_covo_online(built):
    """Today's callers fill a zero-initialised covo_batch_args and never touch pad_: the struct has no mode field (COVO_MODE_MPPI
    is 0, so pad_ could not have become one), and the entry points that take it are covo-online's."""
    a = built.BatchArgsC()
    assert a.pad_ == 0 and not hasattr(a, "mode")
    assert built.MODE_MPPI == 0 and built.MODE_COVO_ONLINE == 1 and built.MODE_COVO_OFFLINE == 2
    hdr = header_text()
    body = re.search(r"typedef struct covo_batch_args \{(.*?)\} covo_batch_args;", hdr, flags=re.S).group(1)
    assert "pad_" in body and "mode" not in re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    lib = built.load_library()
    base_ptr = ctypes.POINTER(built.BatchArgsC)
    assert lib.covo_mpc_step_batched.argtypes[1] is base_ptr and lib.covo_run_episode_batched.argtypes[1] is base_ptr
    mode_ptr = ctypes.POINTER(built.BatchModeArgsC)
    assert lib.covo_mpc_step_batched_mode.argtypes[1] is mode_ptr and lib.covo_run_episode_batched_mode.argtypes[1] is mode_ptr
    # the controller's default stays covo-online through the unchanged entry point
    import inspect
    from covo_mpc_amd.controllers import BatchedCoVOController, BatchedMPPIController
    assert inspect.signature(BatchedCoVOController.__init__).parameters["mode"].default == "online"
    assert BatchedMPPIController.MODE == built.MODE_MPPI


def test_abi_versions_agree(built):
    hdr = header_text()
    v = int(re.search(r"#define COVO_ABI_VERSION (\d+)", hdr).group(1))
    assert v == built.ABI_VERSION == built.load_library().covo_abi_version() >= 9


def test_batched_mppi_refuses_covariance_adaptation_before_touching_the_gpu():
    from covo_mpc_amd.controllers import BatchedMPPIController
    with pytest.raises(NotImplementedError, match="gamma_sigma"):
        BatchedMPPIController(None, 4, 1024, 32, 0.01, gamma_sigma=0.1)
