"""CPU (no GPU): omchat_decode_weight_format, the one rule that picks the weight format a decode step streams and the packed-x block count of
its GEMVs (include/omchat_hip.h), against an independent restatement over the whole table of cases."""
import ctypes as C
import itertools
import pytest
from omchat_amd import _lib

W16, W16P, E4M3, MX4, MX4P = 0, 1, 2, 3, 4       # enum omchat_weight_format


def fmt(rows, fp8=0, mode=0, ready=0, geometry=1):
    nb = C.c_int(-1)
    f = _lib.lib().omchat_decode_weight_format(rows, fp8, mode, ready, geometry, C.byref(nb))
    return f, nb.value


def rule(rows, fp8, mode, ready, geometry):
    """the rule as the issue states it, case by case"""
    if rows == 1:
        return (E4M3 if fp8 else MX4 if mode >= 1 else W16), 0
    if rows > 32:
        return W16, 0
    if not geometry:                                   # no packed x layout
        return (MX4P, 0) if mode == 2 else (W16, 0)    # (mode 2: refused at enable time; the step refuses a packed format without packed x)
    nb = 2 if rows > 16 else 1
    if mode == 2:
        return MX4P, nb
    return (W16P if ready else W16), nb


CASES = [c for c in itertools.product((1, 2, 16, 17, 32, 33), (0, 1), (0, 1, 2), (0, 1), (0, 1)) if not (c[1] and c[2])]


@pytest.mark.parametrize("rows,fp8,mode,ready,geometry", CASES)
def test_format_table(rows, fp8, mode, ready, geometry):
    assert fmt(rows, fp8, mode, ready, geometry) == rule(rows, fp8, mode, ready, geometry)


def test_anchors():
    assert fmt(1, fp8=1)[0] == E4M3
    assert fmt(1, mode=2) == (MX4, 0)
    assert fmt(32, mode=2, geometry=1) == (MX4P, 2)
    assert fmt(16, mode=1, ready=1) == (W16P, 1)
    for fp8, mode, ready, geometry in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1)):
        assert fmt(33, fp8, mode, ready, geometry) == (W16, 0)
    assert fmt(8, mode=0, ready=0, geometry=1) == (W16, 1)
    assert _lib.lib().omchat_decode_weight_format(8, 0, 0, 1, 1, None) == W16P      # the block count is optional
