"""CPU: the Swin V2 attention entry points refuse bad arguments before any device call, with the codes tests/test_abi.py holds the other
entry points to (-1 null pointer / non-positive size, -3 unsupported configuration) and a message that names the limit; the plan dry
run (host arithmetic, nothing launched) agrees with the Python formula."""
import ctypes as C

import pytest


def _lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    return _abi.lib()


def _call(lib, kind, qkv, vb, tau, table, out, B, H, W, Cc, heads, ws, shift):
    fn = getattr(lib, f"vip_swin_attn_fwd_{kind}")
    return fn(qkv, vb, tau, table, out, B, H, W, Cc, heads, ws, shift, *((None,) if kind == "h2" else ()), None)


def test_supported_is_a_pure_function():
    lib = _lib()
    for Cc, heads, ws, shift, ok in ((96, 3, 8, 0, 1), (96, 3, 8, 4, 1), (768, 24, 7, 0, 1), (768, 24, 7, 3, 1), (32, 1, 2, 1, 1), (64, 2, 3, 1, 1),
                                     (1024, 32, 7, 0, 1), (96, 3, 8, 3, 0), (96, 3, 7, 4, 0), (96, 3, 3, 2, 0), (96, 3, 9, 0, 0), (96, 3, 16, 8, 0),
                                     (96, 3, 1, 0, 0), (96, 4, 8, 0, 0), (64, 1, 8, 0, 0), (0, 0, 8, 0, 0), (96, 3, 8, -4, 0)):
        assert lib.vip_swin_attn_supported(Cc, heads, ws, shift) == ok, (Cc, heads, ws, shift)


def test_plan_is_the_python_formula():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    for B, H, W, heads, ws, shift in ((256, 50, 50, 3, 8, 4), (256, 25, 25, 6, 8, 0), (2, 13, 13, 12, 8, 4), (3, 7, 7, 24, 7, 0), (1, 5, 9, 2, 4, 2),
                                      (3, 10, 10, 1, 3, 1), (1, 9, 9, 3, 2, 1), (4, 56, 56, 4, 8, 4), (1, 8, 12, 1, 4, 0)):
        hp, wp = -(-H // ws) * ws, -(-W // ws) * ws
        assert ops.swin_attn_plan(B, H, W, heads, ws, shift) == (hp, wp, B * (hp // ws) * (wp // ws) * heads)
    for bad in ((1, 8, 8, 1, 9, 0), (1, 8, 8, 1, 4, 1), (0, 8, 8, 1, 4, 0), (1, 8, 8, 0, 4, 0), (1, 0, 8, 1, 4, 0), (1, 8, 8, 1, 1, 0),
                (1 << 20, 56, 56, 32, 2, 0)):
        assert ops.swin_attn_plan(*bad) is None, bad


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
def test_argument_checks_do_not_need_a_gpu(kind):
    lib = _lib()
    p = C.c_void_p(64)
    who = f"vip_swin_attn_fwd_{kind}".encode()
    for nulls in ((None, p, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        assert _call(lib, kind, *nulls, 2, 8, 8, 96, 3, 8, 0) == -1 and b"null" in lib.vip_last_error()
    for dims in ((0, 8, 8, 96, 3), (2, 0, 8, 96, 3), (2, 8, -1, 96, 3), (2, 8, 8, 0, 3), (2, 8, 8, 96, 0)):
        assert _call(lib, kind, p, p, p, p, p, *dims, 8, 0) == -1 and b"non-positive" in lib.vip_last_error()
    for Cc, heads, ws, shift in ((96, 4, 8, 0), (64, 1, 8, 0), (96, 3, 9, 0), (96, 3, 16, 8), (96, 3, 1, 0), (96, 3, 8, 3), (96, 3, 7, 4)):
        assert _call(lib, kind, p, p, p, p, p, 2, 16, 16, Cc, heads, ws, shift) == -3
        msg = lib.vip_last_error()
        assert b"head_dim = C / heads = 32" in msg and b"2 <= ws <= 8" in msg and b"shift 0 or ws / 2" in msg and who in msg
    assert _call(lib, kind, p, p, p, p, p, 1 << 20, 56, 56, 1024, 32, 2, 0) == -3 and b"too many windows" in lib.vip_last_error()
