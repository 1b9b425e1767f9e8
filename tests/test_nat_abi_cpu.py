"""CPU: the neighbourhood-attention entry points refuse bad arguments before any device call, with the codes tests/test_abi.py holds the
other entry points to (-1 null pointer / non-positive size, -3 unsupported configuration) and a message that names the limit; the plan
dry run (host arithmetic, nothing launched) agrees with the item count tests/_nat_cases.py expects."""
import ctypes as C

import pytest

from tests import _nat_cases as T


def _lib():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    return _abi.lib()


def _call(lib, kind, qkv, pad, table, out, B, H, W, Cc, heads, K):
    fn = getattr(lib, f"vip_nat_attn_fwd_{kind}")
    return fn(qkv, pad, table, out, B, H, W, Cc, heads, K, *((None,) if kind == "h2" else ()), None)


def test_plan_is_the_table_s_item_count():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    for row in T.ROWS:
        assert ops.nat_attn_plan(row.B, row.H, row.W, row.heads, row.K) == \
            (max(row.H, row.K), max(row.W, row.K), T.plan_items(row.B, row.H, row.W, row.heads)), row.id
    assert ops.nat_attn_plan(256, 50, 50, 2) == (50, 50, 256 * 49 * 2) and ops.nat_attn_plan(256, 7, 7, 32) == (7, 7, 256 * 32)
    assert ops.nat_attn_plan(1, 2, 5, 1, 3) == (3, 5, 1)
    for bad in ((1, 8, 8, 1, 9), (1, 8, 8, 1, 4), (1, 8, 8, 1, 1), (0, 8, 8, 1, 7), (1, 8, 8, 0, 7), (1, 0, 8, 1, 7), (1, 8, -1, 1, 7),
                (1 << 20, 56, 56, 32, 7)):
        assert ops.nat_attn_plan(*bad) is None, bad


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
def test_argument_checks_do_not_need_a_gpu(kind):
    lib = _lib()
    p = C.c_void_p(64)
    who = f"vip_nat_attn_fwd_{kind}".encode()
    for nulls in ((None, p, p, p), (p, p, None, p), (p, p, p, None)):
        assert _call(lib, kind, *nulls, 2, 8, 8, 64, 2, 7) == -1 and b"null" in lib.vip_last_error() and who in lib.vip_last_error()
    for dims in ((0, 8, 8, 64, 2), (2, 0, 8, 64, 2), (2, 8, -1, 64, 2), (2, 8, 8, 0, 2), (2, 8, 8, 64, 0)):
        assert _call(lib, kind, p, p, p, p, *dims, 7) == -1 and b"non-positive" in lib.vip_last_error()
    for K in (9, 4, 1, 0, -7, 6):
        assert _call(lib, kind, p, p, p, p, 2, 16, 16, 64, 2, K) == -3
        msg = lib.vip_last_error()
        assert b"kernel_size 3, 5 or 7" in msg and who in msg
    for Cc, heads in ((96, 4), (64, 1), (48, 2), (32, 2)):
        assert _call(lib, kind, p, p, p, p, 2, 16, 16, Cc, heads, 7) == -3
        msg = lib.vip_last_error()
        assert b"head_dim = C / heads = 32" in msg and who in msg
    assert _call(lib, kind, p, p, p, p, 1 << 20, 56, 56, 1024, 32, 7) == -3
    assert b"too many query tiles" in lib.vip_last_error() and b"2^30" in lib.vip_last_error()
