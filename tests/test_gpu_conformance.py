"""GPU leg of the device conformance suite (tests/device_conformance.py): every op of tests/device/conformance.h, built for
gfx950 with the product's flags, at n = 1, a partial wave, exactly one wave and the whole table (several workgroups with a
ragged tail; directed edge cases share waves with random ones).  Each result must equal the big-integer reference AND
satisfy the primitive's output contract.  After a HIP error nothing more is launched."""
import ctypes
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import device_conformance as dc  # noqa: E402

pytestmark = pytest.mark.gpu

_state = {"lib": None, "hip_error": None}


@pytest.fixture(scope="module")
def lib():
    if _state["lib"] is None:
        _state["lib"] = ctypes.CDLL(dc.build_device())
    return _state["lib"]


@pytest.mark.parametrize("op", sorted(dc.SPECS, key=lambda k: dc.OPS[k]))
def test_device_primitive_conforms(lib, op):
    if _state["hip_error"]:
        pytest.fail("not launched after an earlier HIP error: %s" % _state["hip_error"])
    cases = dc.table(op)
    for n in dc.sizes(op, len(cases)):
        try:
            out, flags, rows = dc.run_device(lib, op, cases[:n])
        except AssertionError as e:
            _state["hip_error"] = str(e)
            raise
        bad = dc.check(op, cases[:n], out, flags, rows)
        assert not bad, "%s at n = %d: %d of %d jobs wrong\n%s" % (op, n, len(bad), n, "\n".join(bad[:12]))
