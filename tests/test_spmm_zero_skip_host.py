"""The process-wide switch of the sweeps' zero-weight skip (include/bot_gnn.h bot_spmm_set_zero_skip): its range check, its place in
the binding, and the ABI number it leaves alone.  No GPU."""
import pytest

from bot_amd import _C

BOT_E_RANGE = -2      # include/bot_gnn.h


def test_setter_range():
    lib = _C._lib
    try:
        for bad in (2, -1):
            assert lib.bot_spmm_set_zero_skip(bad) == BOT_E_RANGE
            assert b"spmm_set_zero_skip" in lib.bot_last_error()
            with pytest.raises(_C.BotKernelError):
                _C.spmm_set_zero_skip(bad)
        for ok in (0, 1, 0):
            assert lib.bot_spmm_set_zero_skip(ok) == 0
            _C.spmm_set_zero_skip(ok)
    finally:
        assert lib.bot_spmm_set_zero_skip(1) == 0      # the default


def test_exported_and_abi_unchanged():
    assert "bot_spmm_set_zero_skip" in _C.EXPORTED
    assert _C._lib.bot_abi_version() == 19 == _C.ABI_VERSION
