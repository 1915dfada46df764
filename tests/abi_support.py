"""What every tests/test_*_abi.py needs before it can look at the C ABI: the built library's Python binding and the header's text."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    """covo_mpc_amd._lib of a finished build; an *_abi.py file imports this fixture by name and gets one per module."""
    import __graft_entry__ as g
    g.build()
    from covo_mpc_amd import _lib
    return _lib


def header_text():
    return open(os.path.join(ROOT, "include", "covo_hip.h")).read()
