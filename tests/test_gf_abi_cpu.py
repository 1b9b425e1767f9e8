"""CPU: the global-local filter's entry points refuse bad arguments before any device call, with the codes tests/test_abi.py holds the
other entry points to (-1 null pointer / non-positive size, -3 unsupported shape) and a message that names the limit."""
import ctypes as C

import pytest


def _lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    return _abi.lib()


def _call(lib, kind, x, w3, g, y, B, H, W, S):
    fn = getattr(lib, f"vip_global_local_filter_nhwc_{kind}")
    args = (x, w3, g, y, B, H, W, S) + ((None,) if kind == "h2" else ()) + (None,)
    return fn(*args)


def test_supported_is_a_pure_function():
    lib = _lib()
    for H, W, S, ok in ((14, 14, 960, 1), (7, 7, 1984, 1), (12, 12, 480, 1), (6, 6, 992, 1), (2, 2, 16, 1), (16, 16, 16, 1), (13, 14, 48, 1),
                        (5, 16, 32, 1), (1, 14, 16, 0), (14, 1, 16, 0), (17, 14, 16, 0), (14, 17, 16, 0), (14, 14, 8, 0), (14, 14, 24, 0),
                        (14, 14, 0, 0), (14, 14, -16, 0), (0, 0, 16, 0)):
        assert lib.vip_global_local_filter_supported(H, W, S) == ok, (H, W, S)
        assert (lib.vip_global_local_filter_plan(H, W, S, None, None) > 0) == bool(ok)


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
def test_argument_checks_do_not_need_a_gpu(kind):
    lib = _lib()
    p = C.c_void_p(64)
    for nulls in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert _call(lib, kind, *nulls, 2, 14, 14, 32) == -1 and b"null" in lib.vip_last_error()
    for dims in ((0, 14, 14, 32), (2, 0, 14, 32), (2, 14, -1, 32), (2, 14, 14, 0), (-3, 14, 14, 32)):
        assert _call(lib, kind, p, p, p, p, *dims) == -1 and b"non-positive" in lib.vip_last_error()
    for dims in ((2, 17, 14, 32), (2, 14, 32, 32), (2, 1, 14, 32), (2, 14, 14, 24), (2, 14, 14, 40)):
        assert _call(lib, kind, p, p, p, p, *dims) == -3
        msg = lib.vip_last_error()
        assert b"2 <= H, W <= 16" in msg and b"S % 16 == 0" in msg and f"vip_global_local_filter_nhwc_{kind}".encode() in msg
    assert _call(lib, kind, p, p, p, p, 70000, 14, 14, 32) == -3 and b"65535" in lib.vip_last_error()
