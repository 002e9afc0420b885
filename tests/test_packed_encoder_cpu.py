"""Host-side checks of the packed-row encoder's interface: the library exports the new entry points and they refuse a NULL
handle without touching a device."""
import ctypes as C

from openhush_amd import engine as E

NEW = ("ohw_state_set_packed_encoder", "ohw_state_packed_encoder", "ohw_engine_set_packed_encoder", "ohw_pool_set_packed_encoder",
       "ohw_dbg_poison")


def test_library_exports_the_packed_encoder_symbols():
    raw = C.CDLL(E.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in E.EXPORTS, name


def test_null_handles_are_refused():
    lib = E.lib()
    assert lib.ohw_state_set_packed_encoder(None, 1) == E.OHW_E_INVALID_ARG
    assert lib.ohw_state_packed_encoder(None) == E.OHW_E_INVALID_ARG
    assert lib.ohw_engine_set_packed_encoder(None, 1) == E.OHW_E_INVALID_ARG
    assert lib.ohw_pool_set_packed_encoder(None, 1) == E.OHW_E_INVALID_ARG
    assert lib.ohw_dbg_poison(None, b"att") == E.OHW_E_INVALID_ARG
    assert lib.ohw_dbg_counter(None, b"enc_rows") == E.OHW_E_INVALID_ARG
