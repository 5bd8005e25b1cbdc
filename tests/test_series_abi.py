"""The series calls' argument checks that need no device: SML_ERR_ARG with a message on
null and out-of-range arguments, before anything touches a context."""
import ctypes

from speedy_ml_amd import _lib

SML_ERR_ARG = -1


def test_series_calls_refuse_without_a_device():
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()  # 16-byte aligned or not, never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)

    def stats(c=None, s4=147456, s2=4608, T=2):
        return L.sml_res_series_stats(c, p, s4, p, p, None, None, s2, T, p, None, None)

    def tile(c=None, s4=147456, s2=4608, T=2):
        return L.sml_res_tile_series(c, p, s4, p, p, None, None, s2, None, 0, None, 0, T, p, 1 << 40, None, 0, None)

    for call in (stats, tile):
        for kw, word in ((dict(T=0), b"T = 0"), (dict(T=-3), b"T = -3"), (dict(s4=147455), b"g4_stride"),
                         (dict(s4=0), b"g4_stride"), (dict(s2=4607), b"g2_stride"), (dict(s4=147457), b"16-byte"),
                         (dict(), b"null reservoir context")):
            assert call(**kw) == SML_ERR_ARG, (call.__name__, kw)
            assert word in L.sml_last_error(), (call.__name__, kw, L.sml_last_error())
    assert L.sml_res_set_mean_std_device(None, p, None) == SML_ERR_ARG
    assert b"null reservoir context" in L.sml_last_error()


def test_series_symbols_are_declared():
    for name in ("sml_res_series_stats", "sml_res_set_mean_std_device", "sml_res_tile_series"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
