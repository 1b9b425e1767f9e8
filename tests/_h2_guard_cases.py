"""The range guard of the packed STRICT storage (csrc/common.hpp, "packed STRICT storage"): one row per packed KERNEL that takes the
caller's status word, the operands that make exactly the named output elements leave the fp16 range, and the fp64 reference that says so.

A value with |v| > 65504 does not fit an fp16 (hi, lo) pair; every producer must then raise VIP_H2_OVERFLOW.  The guard is written in
several forms, and the sites disagree inside the band (65504, 65520):
  converted hi half, integer compare (raises from 65520: rn16(65519.99) = 65504, rn16(65520) = inf)
      h2_store8 of csrc/conv_igemm.hip - every epilogue<> / pw_epilogue<> kernel of the packed build (conv_igemm_kernel, pw_gemm_kernel,
      pwk_direct_kernel, pwk_gemm_kernel with and without im2col, gemm8p_kernel), plain and gated
  fp32 compare !(|v| <= 65504) (raises above 65504)
      h2_st4 (common.hpp): rows_gemm_kernel, the helpers of csrc/strict_ops.hip (spool2d, sgap, sscale_add_act, slayernorm, sdwconv, smul,
      sradix_combine, svit_tokens, sattn, pack_h2), swin_attn_kernel, nat_attn_kernel
      a running max + NaN-catching sum per thread over its whole persistent run: mlp_h2_kernel, dwconv_lds_h2_kernel (plain and pooling)
      a per-thread `bad`: dwconv_tile_h2_kernel, h2_layernorm_kernel (h2_overflows8), attn_h2_kernel
      h2_overflows8 per store: global_local_filter_kernel; its own compare: se_gate_kernel (plain and pooled)
Both forms are safe; the rows stay outside [65504 (1 - 2^-10), 2^16), so no test depends on which form a site uses.

Operands are exact in the sense of tests/_gemm_exact_cases.py: small integers, dyadic weights and parameters, so that the fp64 reference of
an out-of-range element is the true value and "is this output out of range?" needs no tolerance.  Trigger kinds, per row (KINDS below):
  clean    the operands as drawn: max |ref| <= 0.6 * 65504
  over+/-  ONE operand entry changed (all operands stay in range) so that exactly the elements the trigger names reach |ref| >= 2^16
  hidden   mlp_h2_kernel only: the first layer's activation passes 2^16 at one hidden channel of one token while W2 keeps the true
           output in range - the kernel packs the hidden value in registers, so that token's output row cannot be right
  nan      the hi half of one input element set to the fp16 NaN pattern in the packed tensor itself (no pack_h2 that would raise);
           the dependent outputs are those the fp64 reference turns non-finite
How a row overflows (the mechanism column of a row's `why`):
  one-hot  a zero input column c meets a weight row that is zero but for ONE entry of 256: the trigger puts +-512 at one (row, c), the
           product +-131072 lands on one output element (GEMMs, convolutions, depthwise filters, mul, radix_combine, scale_add_act,
           the global filter)
  sum      a bias / position entry of +-30000 (in range, inside the clean bound) meets a residual / patch entry of +-40000 (MLP, vit_tokens)
  gamma    LayerNorm: gamma of one channel becomes +-8192; only the row whose normalised value there is sqrt(C - 1) (a one-hot row)
           passes 2^16, every other row stays below 4 * 8192
Rows whose operation cannot overflow from finite in-range inputs (attention without a value bias, pools, the sigmoid gates) take `nan`
and `clean` only; NO_OVER says why.  pack_h2's only operand is the fp32 value itself, so its trigger IS the operand.

Positions: every row has an interior trigger and one in the last valid row and last channel group of its ragged last tile; the
persistent MLP row adds one in a tile a workgroup reaches on a later pass.

check(row, kind, pos) proves all of this in fp64 on the CPU (tests/test_h2_guard_cases_cpu.py); tests/test_gpu_h2_guard.py runs the rows."""
import math
import zlib
from collections import namedtuple

import torch

from oracle import ops_ref as R
from tests import _attn_cases, _dw_cases, _gf_cases, _h2_gemm_cases, _helper_cases, _ln_site_cases, _nat_cases, _swin_cases

H2_MAX = 65504.0
CLEAN_MAX = 0.6 * H2_MAX
BAND = (H2_MAX * (1.0 - 2.0 ** -10), 2.0 ** 16)          # no reference element may lie in [BAND[0], BAND[1])
NAN16 = 0x7E00
BIG_W, BIG_X = 256.0, 512.0                             # one-hot: 256 * 512 = 2^17
SUM_P, SUM_R = 30000.0, 40000.0                         # sum: 70000 >= 2^16, each term in range, 30000 inside the clean bound
ASSUMED_G = 512                                         # workgroups of the fused-MLP plan the CPU check assumes (2 per CU, 256 CUs)

# row: id, the C entry point, the kernel that must serve it, the trigger kinds it takes, why the others do not apply, builder
Row = namedtuple("Row", "id entry kernel kinds why build")
POSITIONS = ("interior", "edge")
# operand `name` gets `value` at `index`; `over`: the output elements that must leave the range; `dep`: outputs that depend on a
# poisoned value without the fp64 reference showing it (hidden); for nan the dependent set is where the reference is non-finite
Trigger = namedtuple("Trigger", "name index value over dep")
# operands: name -> fp64 host tensor; storage: name -> "packed" | "f32" (how the GPU test uploads it; packed ones are range-checked);
# ref(operands) -> fp64 output; run(ops, dev) -> packed output tensor on the device; triggers: (kind, pos) -> Trigger;
# confirm(ops) -> None or why the row does not reach its kernel (dry runs only)
Case = namedtuple("Case", "operands storage ref run triggers confirm")

NO_OVER = {
    "attention": "a convex combination of in-range values (no value bias on this path) is in range",
    "pool": "a mean or a maximum of in-range values is in range",
    "gate": "the gate is a sigmoid: it cannot overflow from finite inputs",
}
FINITE, GEMM_KINDS = ("clean", "nan"), ("clean", "over+", "over-", "nan")
POSITIVE = ("clean", "over+", "nan")                   # an epilogue that maps a large negative value to 0 leaves over- nothing to name


def single_kernel(ops):
    """`confirm` of an entry point with one kernel behind it: there is nothing to choose and no dry run is made"""
    return None


def _attn_confirm(kernel, mfma_shape, what):
    """the rule of csrc/strict_ops.hip (window_attn_impl / mhsa_impl<SH2>) and csrc/attn_h2.hip: the matrix-core kernel serves the call
    unless the process-wide switch VIP_ATTN_H2_MFMA is 0 or vip_*_h2_mfma declines the shape (window: ws other than 7 and 14; mhsa:
    N > 224); the fp32 VALU kernel sattn_kernel takes the rest.  The library exports no query for it, so the rule is restated here."""
    import os

    def confirm(ops):
        env = os.environ.get("VIP_ATTN_H2_MFMA")
        on = not (env is not None and env.strip().lstrip("+-").isdigit() and int(env) == 0)
        serves = "attn_h2_kernel" if (on and mfma_shape) else "sattn_kernel"
        return None if serves == kernel else f"{what}, VIP_ATTN_H2_MFMA={env!r}: the call goes to {serves}"
    return confirm


def _gen(rid):
    return torch.Generator().manual_seed(zlib.crc32(rid.encode()))


def _ints(g, shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _quarters(g, shape, lo=-2.0, hi=2.0):
    return torch.randint(int(lo * 4), int(hi * 4) + 1, shape, generator=g).double() / 4


def _sign(kind):
    return -1.0 if kind == "over-" else 1.0


def _pack(ops, t):
    return ops.pack_h2(t.float().cuda().contiguous())


def _f32(t):
    return None if t is None else t.float().cuda().contiguous()


def _by_image(operands, batched, fn):
    """ref(o) = fn(o) for an operation whose leading index (image, token) is independent across the operands named in `batched`: the
    clean reference is computed once, a triggered one recomputes only the images whose operands changed"""
    cache = {}

    def ref(o):
        if "clean" not in cache:
            cache["clean"] = fn(operands)
        if o is operands:
            return cache["clean"]
        if any(o[n] is not operands[n] for n in o if n not in batched):
            return fn(o)
        changed = torch.zeros(operands[batched[0]].shape[0], dtype=torch.bool)
        for n in batched:
            if o[n] is not operands[n]:
                changed |= (o[n] != operands[n]).reshape(changed.shape[0], -1).any(1)
        idx = changed.nonzero()[:, 0]
        sub = dict(o)
        for n in batched:
            sub[n] = o[n][idx]
        out = cache["clean"].clone()
        out[idx] = fn(sub)
        return out
    return ref


# ---- GEMMs and convolutions (vip_conv2d_nhwc_h2, vip_conv2d_gated_nhwc_h2): one-hot ------------------------------------------------------
def _conv_case(rid, geom, epi, kernel, gated=False):
    """geom = (B, H, W, Cin, Cout, k, stride, pad, groups); epi = (act, act_post, residual).  Input channels c1 (first group) and c2
    (last group) are zero; their weight rows are zero but for 256 at the centre tap towards output channel n1 / n2 = Cout - 1."""
    B, H, W, Cin, Cout, k, s, pad, groups = geom
    act, post, has_res = epi
    g = _gen(rid)
    Ho, Wo = (H + pad[0] + pad[1] - k) // s + 1, (W + pad[2] + pad[3] - k) // s + 1
    cg, ng = Cin // groups, Cout // groups
    c1, n1, c2, n2 = 1, ng // 2 + 1, Cin - 1, Cout - 1
    x = _ints(g, (B, H, W, Cin))
    w = _quarters(g, (k, k, cg, Cout))
    x[..., c1] = x[..., c2] = 0
    w[:, :, c1 % cg, :ng] = 0                               # weight [kh, kw, c within its group, n]: c1 feeds group 0, c2 the last group
    w[:, :, c2 % cg, Cout - ng:] = 0
    w[k // 2, k // 2, c1 % cg, n1] = w[k // 2, k // 2, c2 % cg, n2] = BIG_W
    o = dict(x=x, w=w, b=_quarters(g, (Cout,)))
    st = dict(x="packed", w="weight", b="weight")
    if gated:
        o["gate"] = torch.randint(0, 9, (B, Cin), generator=g).double() / 4
        o["gate"][:, c1] = o["gate"][:, c2] = 1.0
        st["gate"] = "packed"
    if has_res:
        o["r"] = _ints(g, (B, Ho, Wo, Cout))
        st["r"] = "packed"

    def inp(ho, wo):                                        # the input pixel under the centre tap of output (ho, wo)
        return ho * s - pad[0] + k // 2, wo * s - pad[2] + k // 2

    outs = {"interior": (B // 2, Ho // 2, Wo // 3, c1, n1), "edge": (B - 1, Ho - 1, Wo - 1, c2, n2)}
    trig = {}
    for pos, (b, ho, wo, c, n) in outs.items():
        hi, wi = inp(ho, wo)
        assert 0 <= hi < H and 0 <= wi < W, (rid, pos)
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("x", (b, hi, wi, c), _sign(kind) * BIG_X, [(b, ho, wo, n)], None)
        trig[("nan", pos)] = Trigger("x", (b, hi, wi, (c + 3) % Cin), math.nan, None, None)
        if post is not None:
            del trig[("over-", pos)]

    def ref(o):
        xe = o["x"] * o["gate"][:, None, None, :] if gated else o["x"]
        v = R.act(R.conv2d(xe, o["w"], o["b"], s, pad, groups), act)
        return R.act(v + o["r"], post) if has_res else v

    def weight(ops, o):
        with ops.precision("strict"):
            return ops.make_conv_weight(o["w"].float(), o["b"].float(), groups=groups)

    def run(ops, dev):
        return ops.conv2d(dev["x"], dev["w"], stride=s, pad=pad, act=act, act_post=post, residual=dev.get("r"), gate=dev.get("gate"))

    def confirm(ops):
        with ops.precision("strict"):
            ldw = ops.make_conv_weight(torch.zeros(k, k, cg, Cout), None, groups=groups, device="cpu").ldw
        d, _ = _h2_gemm_cases.conv_desc((B, H, W, Cin, Cout, k, s, pad, groups, act, has_res), ldw)
        d.act_post = ops._act(post)
        if gated:                                           # ops._conv2d_h2 folds the gate where it launches vip_conv2d_gated_nhwc_h2
            fold = ops._H2_GATED and (k, s, groups) == (1, 1, 1) and pad == (0, 0, 0, 0) and ops._epilogue_ok(act, post, o.get("r"))
            return None if fold else "the gate would be multiplied in by a separate pass"
        name = ops.conv_kernel_name_h2(d, has_res)
        return None if name == kernel else f"the dispatcher's dry run says {name}"

    return Case(o, dict(st, w=weight, b=None), _by_image(o, [n for n in ("x", "gate", "r") if n in o], ref), run, trig, confirm)


def _dense_geom(M, K, N):
    return (M, 1, 1, K, N, 1, 1, (0, 0, 0, 0), 1)


# ---- fused MLP (vip_mlp_fused_h2): sum for over, one-hot into the hidden layer for hidden ------------------------------------------------
MLP_C, MLP_HID, MLP_TILE = 96, 384, 256


def _mlp_case(rid, M, tokens):
    """tokens: position -> token index.  fc2's bias holds +30000 at channel CA and -30000 at CB; x column CX is zero and w1 row CX is
    zero but for 256 towards hidden channel HX, whose w2 row is 2^-6 throughout (131072 * 2^-6 = 2048: the true output stays in range)."""
    C, hid = MLP_C, MLP_HID
    g = _gen(rid)
    CA, CB, CX, HX = 37, C - 1, 5, hid - 3
    x = _ints(g, (M, C), -2, 2)
    w1, b1 = _quarters(g, (C, hid), -1, 1), _quarters(g, (hid,))
    w2, b2 = _quarters(g, (hid, C), -1, 1), _quarters(g, (C,))
    r = _ints(g, (M, C))
    x[:, CX] = 0
    w1[CX] = 0
    w1[CX, HX] = BIG_W
    w2[HX] = 2.0 ** -6
    b2[CA], b2[CB] = SUM_P, -SUM_P
    r[:, CA] = r[:, CB] = 0
    o = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, r=r)
    trig = {}
    for pos, m in tokens.items():
        trig[("over+", pos)] = Trigger("r", (m, CA), SUM_R, [(m, CA)], None)
        trig[("over-", pos)] = Trigger("r", (m, CB), -SUM_R, [(m, CB)], None)
        trig[("hidden", pos)] = Trigger("x", (m, CX), BIG_X, [], [(m, c) for c in range(C)])
        trig[("nan", pos)] = Trigger("x", (m, C - 1 if pos == "edge" else 11), math.nan, None, None)

    def ref(o):
        return R.dense(R.act(R.dense(o["x"], o["w1"], o["b1"]), "gelu"), o["w2"], o["b2"]) + o["r"]

    def fc(a, b):
        def make(ops, o):
            with ops.precision("strict"):
                return ops.make_dense_weight(o[a].float(), o[b].float())
        return make

    def run(ops, dev):
        return ops.mlp(dev["x"], dev["w1"], dev["w2"], act="gelu", residual=dev["r"])

    def confirm(ops):                                       # (the GPU test also reads the launch off the profiler hook)
        ok = ops._abi.lib().vip_mlp_fused_supported_h2(M, C, hid, ops._act("gelu"))
        return None if ok else "vip_mlp_fused_supported_h2 declines the shape"

    return Case(o, dict(x="packed", r="packed", w1=fc("w1", "b1"), b1=None, w2=fc("w2", "b2"), b2=None), _by_image(o, ["x", "r"], ref), run,
                trig, confirm)


def _mlp_tail(rid):
    M = _ln_site_cases.M_MLP
    return _mlp_case(rid, M, {"interior": 3 * MLP_TILE + 77, "edge": M - 1})


def _mlp_passes(rid, G=ASSUMED_G):
    """(2 G + 1) tiles - 37 rows: workgroup 3 reaches tile G + 3 on its second pass, workgroup 0 the ragged tile 2 G on its third"""
    M = (2 * G + 1) * MLP_TILE - 37
    return _mlp_case(rid, M, {"interior": 5 * MLP_TILE + 9, "pass2": (G + 3) * MLP_TILE + 130, "edge": M - 1})


# ---- depthwise (vip_dwconv2d_nhwc_h2, vip_dwconv2d_s1_h2, vip_dwconv2d_s1_pool_h2): one-hot ----------------------------------------------
def _dw_case(rid, kernel, B, H, W, C, k, s, pad, lds):
    """channels c1 and c2 = C - 1 of x are zero, their filters zero but for 256 at the centre tap"""
    g = _gen(rid)
    Ho, Wo = (H + pad[0] + pad[1] - k) // s + 1, (W + pad[2] + pad[3] - k) // s + 1
    c1, c2 = 9 % C, C - 1
    x, w, b = _ints(g, (B, H, W, C), -2, 2), _quarters(g, (k, k, C, 1), -1, 1), _quarters(g, (C,))
    for c in (c1, c2):
        x[..., c] = 0
        w[:, :, c] = 0
        w[k // 2, k // 2, c] = BIG_W
    o = dict(x=x, w=w, b=b)
    trig = {}
    for pos, (bb, ho, wo, c) in {"interior": (0, Ho // 2, Wo // 2, c1), "edge": (B - 1, Ho - 1, Wo - 1, c2)}.items():
        hi, wi = ho * s - pad[0] + k // 2, wo * s - pad[2] + k // 2
        assert 0 <= hi < H and 0 <= wi < W, (rid, pos)
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("x", (bb, hi, wi, c), _sign(kind) * BIG_X, [(bb, ho, wo, c)], None)
        trig[("nan", pos)] = Trigger("x", (bb, hi, wi, (c + 2) % C), math.nan, None, None)

    def ref(o):
        return R.dwconv2d(o["x"], o["w"], o["b"], s, pad)

    def filt(ops, o):
        return ops.make_dw_weight(o["w"].float())

    def run(ops, dev):
        if lds != "pool":
            old, ops._DW_H2_LDS = ops._DW_H2_LDS, (0 if lds is None else 3)     # 0: the documented switch to the tile kernel
            try:
                return ops.dwconv2d(dev["x"], dev["w"], dev["b"], k, s, pad, act=None)
            finally:
                ops._DW_H2_LDS = old
        # the pooling form alone (ops.dwconv2d_se follows it with the gate kernel, a second producer that would raise the word too)
        parts = ops._abi.lib().vip_dwconv2d_s1_pool_parts_h2(B, H, W, C, k, Ho, Wo)
        assert parts > 0
        out = torch.empty((B, Ho, Wo, C), dtype=ops.PACKED, device="cuda")
        partials = torch.empty((B, parts, C), dtype=torch.float32, device="cuda")
        ops._launch("vip_dwconv2d_s1_pool_h2", ops._p(dev["x"]), ops._p(ops._dw_quad_major(dev["w"], k)), ops._p(dev["b"]), ops._p(out),
                    ops._p(partials), parts, B, H, W, C, k, pad[0], pad[2], Ho, Wo, 0, status=True)
        return out

    def confirm(ops):
        row = _dw_cases.Row(rid, "h2", kernel, B, H, W, C, k, s, pad, None, None, "")
        return _dw_cases.reaches(row, ops)

    return Case(o, dict(x="packed", w=filt, b="f32"), ref, run, trig, confirm)


# ---- squeeze-excite gates (vip_se_gate_h2, vip_se_gate_pooled_h2): nan only ---------------------------------------------------------------
def _se_case(rid, pooled):
    B, HW, C, Cr, parts = 5, 6, 72, 16, 3
    g = _gen(rid)
    w1, b1, w2, b2 = _quarters(g, (C, Cr), -1, 1), _quarters(g, (Cr,)), _quarters(g, (Cr, C), -1, 1), _quarters(g, (C,))
    src = _ints(g, (B, parts, C)) if pooled else _ints(g, (B, HW, HW, C))
    o = dict(x=src, w1=w1, b1=b1, w2=w2, b2=b2)
    n = HW * HW
    where = {"interior": (2, 1, 17), "edge": (B - 1, parts - 1, C - 1)} if pooled else {"interior": (2, 3, 2, 17), "edge": (B - 1, HW - 1, HW - 1, C - 1)}
    trig = {("nan", pos): Trigger("x", idx, math.nan, None, None) for pos, idx in where.items()}

    def ref(o):
        mean = o["x"].sum(1) / n if pooled else o["x"].mean((1, 2))
        return torch.sigmoid(R.dense(R.act(R.dense(mean, o["w1"], o["b1"]), "silu"), o["w2"], o["b2"]))

    def fc(a, b):
        def make(ops, o):
            with ops.precision("strict"):
                return ops.make_dense_weight(o[a].float(), o[b].float())
        return make

    def run(ops, dev):
        fc1, fc2 = dev["w1"], dev["w2"]
        if not pooled:
            return ops.se_gate(dev["x"], fc1, fc2, "silu", "sigmoid")
        gate = torch.empty((B, C), dtype=ops.PACKED, device="cuda")
        ops._launch("vip_se_gate_pooled_h2", ops._p(dev["x"]), parts, ops._p(fc1.w), ops._p(fc1.bias), 1.0 / fc1.h2_scale, ops._p(fc2.w),
                    ops._p(fc2.bias), 1.0 / fc2.h2_scale, ops._p(gate), B, n, C, fc1.cout, fc1.ldw, fc2.cout, fc2.ldw, ops._act("silu"),
                    ops._act("sigmoid"), status=True)
        return gate

    def confirm(ops):
        ok = ops._SE_H2_FUSED and C * Cr + Cr * C <= ops.SE_FUSED_MAX_WEIGHTS
        return None if ok else "ops.se_gate would answer with pool + two Dense launches"

    return Case(o, dict(x="f32" if pooled else "packed", w1=fc("w1", "b1"), b1=None, w2=fc("w2", "b2"), b2=None), ref, run, trig, confirm)


# ---- the strict helpers (csrc/strict_ops.hip) ----------------------------------------------------------------------------------------------
def _ln_case(rid, C, kernel):
    """37 integer rows; row 20 is one-hot (8 at channel CG), so its normalised value there is sqrt(C - 1) (9.7 at C = 96, 45 at 2056)
    against at most 4 in a row of integers of [-4, 4] with variance >= 1: gamma[CG] = +-8192 overflows row 20 alone.  The edge trigger uses
    the last row and the last channel."""
    rows, eps = 37, _helper_cases.LN_EPS
    g = _gen(rid)
    x = _ints(g, (rows, C))
    x[:, 0], x[:, 1] = 3, -3                                  # no drawn row is constant
    spots = {"interior": (20, 40), "edge": (rows - 1, C - 1)}
    for r_, c_ in spots.values():
        x[r_] = 0
        x[r_, c_] = 8
    o = dict(x=x, gamma=_quarters(g, (C,), 0.5, 2), beta=_quarters(g, (C,)))
    trig = {}
    for pos, (r_, c_) in spots.items():
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("gamma", (c_,), _sign(kind) * 8192.0, [(r_, c_)], None)
        trig[("nan", pos)] = Trigger("x", (r_ - 1, c_), math.nan, None, None)

    def ref(o):
        return R.layernorm(o["x"], o["gamma"], o["beta"], eps)

    def run(ops, dev):
        return ops.layernorm(dev["x"], dev["gamma"], dev["beta"], eps)

    def confirm(ops):
        name = _helper_cases.ln_kernel("h2", C)[0]
        return None if name == kernel else f"layernorm_impl<SH2> takes C = {C} to {name}"

    return Case(o, dict(x="packed", gamma="f32", beta="f32"), ref, run, trig, confirm)


def _pool_case(rid, mode):
    p = dict(H=9, W=7, k=3, stride=2, pad=(1, 1, 1, 1), mode=mode, out_hw=None)
    B, C = 3, 24
    g = _gen(rid)
    o = dict(x=_ints(g, (B, 9, 7, C), 1 if mode == 0 else -4, 4))        # max: positive, so that the padded zero never hides the element
    trig = {("nan", "interior"): Trigger("x", (1, 4, 3, 9), math.nan, None, None),
            ("nan", "edge"): Trigger("x", (B - 1, 8, 6, C - 1), math.nan, None, None)}

    def ref(o):
        return _helper_cases.pool_ref(o["x"], p)[0]

    def run(ops, dev):
        return ops.pool2d(dev["x"], 3, 2, (1, 1, 1, 1), mode)

    return Case(o, dict(x="packed"), ref, run, trig, single_kernel)


def _gap_case(rid):
    B, HW, C = 3, 33, 72
    o = dict(x=_ints(_gen(rid), (B, HW, C)))
    trig = {("nan", "interior"): Trigger("x", (1, 16, 20), math.nan, None, None),
            ("nan", "edge"): Trigger("x", (B - 1, HW - 1, C - 1), math.nan, None, None)}
    return Case(o, dict(x="packed"), lambda o: o["x"].sum(1) / HW, lambda ops, dev: ops.global_avgpool(dev["x"]), trig, single_kernel)


def _saa_case(rid):
    """y = x * scale[b, c] + r and y2 = relu(y), stacked as [2, B, HW, C].  scale holds 256 at (b, c) of the two spots, x is zero in
    those channel maps: over+ takes y AND y2 out of range, over- y alone (relu of a negative value is 0)."""
    B, HW, C = 3, 5, 24
    g = _gen(rid)
    x, sc, r = _ints(g, (B, HW, C)), torch.randint(0, 9, (B, C), generator=g).double() / 4, _ints(g, (B, HW, C))
    spots = {"interior": (1, 2, 10), "edge": (B - 1, HW - 1, C - 1)}
    trig = {}
    for pos, (b, p_, c) in spots.items():
        x[b, :, c] = 0
        sc[b, c] = BIG_W
        trig[("over+", pos)] = Trigger("x", (b, p_, c), BIG_X, [(0, b, p_, c), (1, b, p_, c)], None)
        trig[("over-", pos)] = Trigger("x", (b, p_, c), -BIG_X, [(0, b, p_, c)], None)
        trig[("nan", pos)] = Trigger("x", (b, p_, c - 1), math.nan, None, None)

    def ref(o):
        y = o["x"] * o["scale"][:, None, :] + o["r"]
        return torch.stack([y, torch.where(torch.isnan(y), y, torch.relu(y))])

    def run(ops, dev):
        return torch.stack(ops.scale_add_act(dev["x"], dev["scale"], dev["r"], None, act2="relu"))

    return Case(dict(x=x, scale=sc, r=r), dict(x="packed", scale="packed", r="packed"), ref, run, trig, single_kernel)


def _radix_case(rid):
    B, HW, C, radix = 3, 5, 40, 2
    g = _gen(rid)
    x, sc = _ints(g, (B, 1, HW, radix * C)), torch.randint(0, 9, (B, radix * C), generator=g).double() / 4
    spots = {"interior": (1, 2, 0, 17), "edge": (B - 1, HW - 1, 1, C - 1)}            # (b, pixel, radix plane, output channel)
    trig = {}
    for pos, (b, p_, rd, c) in spots.items():
        x[b, 0, :, rd * C + c] = 0
        sc[b, rd * C + c] = BIG_W
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("x", (b, 0, p_, rd * C + c), _sign(kind) * BIG_X, [(b, 0, p_, c)], None)
        trig[("nan", pos)] = Trigger("x", (b, 0, p_, (1 - rd) * C + c), math.nan, None, None)

    def ref(o):
        return (o["x"].reshape(B, 1, HW, radix, C) * o["scale"].reshape(B, 1, 1, radix, C)).sum(3)

    return Case(dict(x=x, scale=sc), dict(x="packed", scale="packed"), ref, lambda ops, dev: ops.radix_combine(dev["x"], dev["scale"], radix),
                trig, single_kernel)


def _mul_case(rid):
    rows, C, lda, a_off, ldb, b_off = 37, 24, 56, 16, 48, 8
    g = _gen(rid)
    a, b = _ints(g, (rows, lda)), torch.randint(0, 9, (rows, ldb), generator=g).double() / 4
    spots = {"interior": (17, 10), "edge": (rows - 1, C - 1)}
    trig = {}
    for pos, (r_, c) in spots.items():
        a[r_, a_off + c] = 0
        b[r_, b_off + c] = BIG_W
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("a", (r_, a_off + c), _sign(kind) * BIG_X, [(r_, c)], None)
        trig[("nan", pos)] = Trigger("b", (r_, b_off + c - 1), math.nan, None, None)

    def ref(o):
        return o["a"][:, a_off:a_off + C] * o["b"][:, b_off:b_off + C]

    return Case(dict(a=a, b=b), dict(a="packed", b="packed"), ref, lambda ops, dev: ops.mul(dev["a"], dev["b"], C, a_off, b_off), trig,
                single_kernel)


def _vit_case(rid):
    """out[b, 0] = cls + pos[0], out[b, 1 + i] = patches[b, i] + pos[1 + i]; pos holds +-30000 at the two spots"""
    B, NP, D = 3, 17, 24
    g = _gen(rid)
    patches, cls, pos = _ints(g, (B, NP, D)), _ints(g, (D,)), _ints(g, (NP + 1, D))
    spots = {"interior": (1, 8, 10), "edge": (B - 1, NP, D - 1)}                        # (b, output token, channel)
    trig = {}
    for pos_name, (b, t, c) in spots.items():
        patches[:, t - 1, c] = 0
        for kind in ("over+", "over-"):
            trig[(kind, pos_name)] = Trigger("patches", (b, t - 1, c), _sign(kind) * SUM_R, [(b, t, c)], None)
        trig[("nan", pos_name)] = Trigger("patches", (b, t - 1, c - 1), math.nan, None, None)
    pos[8, 10], pos[NP, D - 1] = SUM_P, -SUM_P
    # over+ on a -30000 entry (and the reverse) would not overflow: each spot serves the sign of its position embedding
    del trig[("over-", "interior")], trig[("over+", "edge")]

    def ref(o):
        return torch.cat([o["cls"].expand(B, 1, D), o["patches"]], 1) + o["pos"][None]

    return Case(dict(patches=patches, cls=cls, pos=pos), dict(patches="packed", cls="packed", pos="packed"), ref,
                lambda ops, dev: ops.vit_tokens(dev["patches"], dev["cls"], dev["pos"]), trig, single_kernel)


def _pack_case(rid):
    """vip_pack_h2: the fp32 input IS the operand, so the trigger is a value of +-70000 (or an fp32 NaN) in it"""
    shape = (5, 33, 40)
    o = dict(x=_ints(_gen(rid), shape, -64, 64))
    trig = {}
    for pos, idx in {"interior": (2, 16, 21), "edge": (4, 32, 39)}.items():
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("x", idx, _sign(kind) * 70000.0, [idx], None)
        trig[("nan", pos)] = Trigger("x", idx, math.nan, None, None)
    return Case(o, dict(x="f32"), lambda o: o["x"].clone(), lambda ops, dev: ops.pack_h2(dev["x"]), trig, single_kernel)


# ---- attention cores, the global filter --------------------------------------------------------------------------------------------------
def _window_case(rid, ws, heads, kernel):
    """nan in a QUERY element: the outputs of that query in that head (32 channels) depend on it, nothing else does"""
    B, nwin, C = 2, (2, 1), heads * 32
    g = _gen(rid)
    Hp, Wp = nwin[0] * ws, nwin[1] * ws
    qkv = _ints(g, (B, Hp, Wp, 3 * C), -2, 2) / 2
    table = _quarters(g, ((2 * ws - 1) ** 2, heads), -1, 1)
    scale = 2.0 ** -3
    trig = {("nan", "interior"): Trigger("qkv", (0, ws // 2, ws // 2, 7), math.nan, None, None),
            ("nan", "edge"): Trigger("qkv", (B - 1, Hp - 1, Wp - 1, C - 1), math.nan, None, None)}

    def ref(o):
        return _attn_cases.window_ref(o["qkv"], None, o["table"], heads, ws, scale)

    def run(ops, dev):
        return ops.window_attention(dev["qkv"], None, dev["table"], heads, ws, scale)

    return Case(dict(qkv=qkv, table=table), dict(qkv="packed", table="f32"), ref, run, trig,
                _attn_confirm(kernel, ws in (7, 14), f"ws = {ws}"))


def _mhsa_case(rid, N, kernel):
    B, heads = 2, 2
    D = heads * 64
    qkv = _ints(_gen(rid), (B, N, 3 * D), -2, 2) / 2
    scale = 2.0 ** -3
    trig = {("nan", "interior"): Trigger("qkv", (0, N // 2, 21), math.nan, None, None),
            ("nan", "edge"): Trigger("qkv", (B - 1, N - 1, D - 1), math.nan, None, None)}
    return Case(dict(qkv=qkv), dict(qkv="packed"), lambda o: _attn_cases.mhsa_ref(o["qkv"], heads, scale),
                lambda ops, dev: ops.mhsa(dev["qkv"], heads, scale), trig, _attn_confirm(kernel, N <= 224, f"N = {N}"))


def _swin_case(rid):
    B, H, W, heads, ws, shift = 2, 9, 10, 2, 4, 2
    C = heads * 32
    g = _gen(rid)
    o = dict(qkv=_ints(g, (B, H, W, 3 * C), -2, 2) / 2, tau=torch.tensor([4.0, 8.0], dtype=torch.float64),
             table=_quarters(g, ((2 * ws - 1) ** 2, heads), -1, 1))
    trig = {("nan", "interior"): Trigger("qkv", (0, 4, 5, 7), math.nan, None, None),
            ("nan", "edge"): Trigger("qkv", (B - 1, H - 1, W - 1, C - 1), math.nan, None, None)}

    def ref(o):
        return _swin_cases.folded(o["qkv"], None, o["tau"], o["table"], heads, ws, shift, dtype=torch.float64)

    def run(ops, dev):
        return ops.swin_window_attention(dev["qkv"], None, dev["tau"], dev["table"], heads, ws, shift)

    def confirm(ops):
        return None if ops.swin_attn_plan(B, H, W, heads, ws, shift) else "vip_swin_attn_plan refuses the launch"

    return Case(o, dict(qkv="packed", tau="f32", table="f32"), ref, run, trig, confirm)


def _nat_case(rid):
    B, H, W, heads, K = 2, 9, 12, 2, 7
    C = heads * 32
    g = _gen(rid)
    o = dict(qkv=_ints(g, (B, H, W, 3 * C), -2, 2) / 2, table=_quarters(g, (heads, (2 * K - 1) ** 2), -1, 1))
    trig = {("nan", "interior"): Trigger("qkv", (0, 4, 5, 7), math.nan, None, None),
            ("nan", "edge"): Trigger("qkv", (B - 1, H - 1, W - 1, C - 1), math.nan, None, None)}

    def ref(o):
        return _nat_cases.folded(o["qkv"], None, o["table"], heads, K, dtype=torch.float64)

    def run(ops, dev):
        return ops.nat_attention(dev["qkv"], None, dev["table"], heads, K)

    def confirm(ops):
        return None if ops.nat_attn_plan(B, H, W, heads, K) else "vip_nat_attn_plan refuses the launch"

    return Case(o, dict(qkv="packed", table="f32"), ref, run, trig, confirm)


def _gf_case(rid):
    """output channel 2 c is the 3 x 3 local filter of input channel c, 2 c + 1 the circular whole-map filter of input channel half + c.
    One-hot through the GLOBAL filter: g[:, :, c] is zero but for 256 at (0, 0) (the identity tap) and the input map half + c is zero, so
    +-512 at one pixel overflows that pixel of output channel 2 c + 1 alone.  interior: c = 3; edge: the last pixel, c = half - 1.
    nan: a local-half channel at the interior spot (its 3 x 3 neighbourhood depends on it), a global-half one at the edge (the whole map)."""
    B, H, W, S = 2, 13, 14, 48
    half = S // 2
    gen = _gen(rid)
    x, w3, g = _ints(gen, (B, H, W, S), -2, 2), _quarters(gen, (3, 3, half), -1, 1), _quarters(gen, (H, W, half), -1, 1) / 16
    spots = {"interior": (0, 6, 7, 3), "edge": (B - 1, H - 1, W - 1, half - 1)}
    trig = {}
    for pos, (b, y, x_, c) in spots.items():
        x[..., half + c] = 0
        g[:, :, c] = 0
        g[0, 0, c] = BIG_W
        for kind in ("over+", "over-"):
            trig[(kind, pos)] = Trigger("x", (b, y, x_, half + c), _sign(kind) * BIG_X, [(b, y, x_, 2 * c + 1)], None)
    trig[("nan", "interior")] = Trigger("x", (0, 6, 7, 5), math.nan, None, None)
    trig[("nan", "edge")] = Trigger("x", (B - 1, H - 1, W - 1, S - 2), math.nan, None, None)

    def confirm(ops):
        return None if ops.global_filter_plan(H, W, S) else "vip_global_local_filter_plan declines the shape"

    return Case(dict(x=x, w3=w3, g=g), dict(x="packed", w3="f32", g="f32"), lambda o: _gf_cases.ref64(o["x"], o["w3"], o["g"]),
                lambda ops, dev: ops.global_local_filter(dev["x"], dev["w3"], dev["g"]), trig, confirm)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def _dense_row(rid, M, K, N, epi, kernel):
    return Row(rid, "vip_conv2d_nhwc_h2", kernel, GEMM_KINDS, f"one-hot; {M} x {K} x {N} of tests/_h2_gemm_cases.py, epilogue {epi}",
               lambda: _conv_case(rid, _dense_geom(M, K, N), _h2_gemm_cases.EPILOGUE[epi], kernel))


def _conv_row(rid, case, kernel, entry="vip_conv2d_nhwc_h2", gated=False, post=None):
    geom, (act, res) = case[:9], case[9:]
    return Row(rid, entry, kernel, POSITIVE if post else GEMM_KINDS,
               f"one-hot; conv {geom}, act {act}, residual {res}, act_post {post}" + ("; no over-: silu(-131072) is -0" if post else ""),
               lambda: _conv_case(rid, geom, (act, post, res), kernel, gated))


_C = _h2_gemm_cases.CONV_H2_CASES
ROWS = [
    # vip_conv2d_nhwc_h2: one row per epilogue carrier, the smallest shape tests/_h2_gemm_cases.py pins to it, each with an M tail
    _dense_row("pw_gemm", 65536 + 37, 32, 64, "none", "pw_gemm_kernel"),
    _dense_row("pwk_direct", 777, 72, 40, "none", "pwk_direct_kernel"),
    _dense_row("pwk_gemm", 257, 2048, 512, "none", "pwk_gemm_kernel"),
    _dense_row("gemm8p", 32513, 512, 256, "res", "gemm8p_kernel"),
    _dense_row("rows_gemm", 37, 264, 72, "none", "rows_gemm_kernel"),
    # epilogue<> applies act_post at run time (h2_store8<ACT, RES, 2>): residual, then SiLU.  (A ReLU there is `v > 0 ? v : 0`, which
    # stores 0 for a NaN accumulator - an in-range value, nothing to raise - so the nan kind needs an activation that keeps the NaN.)
    _conv_row("conv_igemm", _C[2][0][:9] + (None, True), "conv_igemm_kernel", post="silu"),
    _conv_row("pwk_gemm_im2col", _C[1][0], "pwk_gemm_kernel(im2col)"),
    _conv_row("gated", (4, 14, 14, 96, 40, 1, 1, (0, 0, 0, 0), 1, None, False), "pwk_direct_kernel", "vip_conv2d_gated_nhwc_h2", True),
    Row("mlp_tail", "vip_mlp_fused_h2", "mlp_h2_kernel", GEMM_KINDS + ("hidden",),
        "sum (bias +-30000 of fc2 + residual +-40000); hidden: one-hot into fc1; M = 8192 + 37: 32 tiles of 256 and 37 rows",
        lambda: _mlp_tail("mlp_tail")),
    Row("mlp_passes", "vip_mlp_fused_h2", "mlp_h2_kernel", GEMM_KINDS + ("hidden",),
        "the same at (2 G + 1) tiles - 37 rows: a trigger in tile G + 3 (second pass) and in the last row (third pass)",
        lambda G=ASSUMED_G: _mlp_passes("mlp_passes", G)),
    Row("dw_plain", "vip_dwconv2d_nhwc_h2", "sdwconv_kernel", GEMM_KINDS, "one-hot; stride 2: both stride-1 kernels decline",
        lambda: _dw_case("dw_plain", "sdwconv_kernel", 3, 10, 14, 40, 3, 2, (0, 1, 0, 1), None)),
    Row("dw_tile", "vip_dwconv2d_nhwc_h2", "dwconv_tile_h2_kernel", GEMM_KINDS, "one-hot; 7 x 5 outputs under the 2 x 2 register tile, C = 136",
        lambda: _dw_case("dw_tile", "dwconv_tile_h2_kernel", 2, 7, 5, 136, 5, 1, (2, 2, 2, 2), None)),
    Row("dw_lds", "vip_dwconv2d_s1_h2", "dwconv_lds_h2_kernel", GEMM_KINDS, "one-hot; 14 x 14, C = 72: the last 16-channel block half empty",
        lambda: _dw_case("dw_lds", "dwconv_lds_h2_kernel", 3, 14, 14, 72, 5, 1, (2, 2, 2, 2), "lds")),
    Row("dw_lds_pool", "vip_dwconv2d_s1_pool_h2", "dwconv_lds_h2_kernel/pool", GEMM_KINDS, "one-hot; the pooling form at 13 x 13, C = 72",
        lambda: _dw_case("dw_lds_pool", "dwconv_lds_h2_kernel/pool", 3, 13, 13, 72, 3, 1, (1, 1, 1, 1), "pool")),
    Row("se_gate", "vip_se_gate_h2", "se_gate_kernel", FINITE, NO_OVER["gate"], lambda: _se_case("se_gate", False)),
    Row("se_gate_pooled", "vip_se_gate_pooled_h2", "se_gate_kernel(pooled)", FINITE, NO_OVER["gate"] + "; nan sits in the fp32 partial sums",
        lambda: _se_case("se_gate_pooled", True)),
    Row("ln_h2", "vip_layernorm_h2", "h2_layernorm_kernel", GEMM_KINDS, "gamma; C = 96", lambda: _ln_case("ln_h2", 96, "h2_layernorm_kernel")),
    Row("ln_fallback", "vip_layernorm_h2", "slayernorm_kernel", GEMM_KINDS, "gamma; C = 2056: beyond the lanes-per-row kernel",
        lambda: _ln_case("ln_fallback", 2056, "slayernorm_kernel")),
    Row("pool_avg", "vip_pool2d_nhwc_h2", "spool2d_kernel", FINITE, NO_OVER["pool"], lambda: _pool_case("pool_avg", 1)),
    Row("pool_max", "vip_pool2d_nhwc_h2", "spool2d_kernel", FINITE, NO_OVER["pool"], lambda: _pool_case("pool_max", 0)),
    Row("gap", "vip_global_avgpool_h2", "sgap_kernel", FINITE, NO_OVER["pool"], lambda: _gap_case("gap")),
    Row("scale_add_act", "vip_scale_add_act_h2", "sscale_add_act_kernel", GEMM_KINDS, "one-hot through the scale; both outputs y and y2 = relu(y)",
        lambda: _saa_case("scale_add_act")),
    Row("radix_combine", "vip_radix_combine_h2", "sradix_combine_kernel", GEMM_KINDS, "one-hot through the scale", lambda: _radix_case("radix_combine")),
    Row("mul", "vip_mul_h2", "smul_kernel", GEMM_KINDS, "one-hot", lambda: _mul_case("mul")),
    Row("vit_tokens", "vip_vit_tokens_h2", "svit_tokens_kernel", GEMM_KINDS, "sum (position +-30000 + patch +-40000): over+ interior, over- edge",
        lambda: _vit_case("vit_tokens")),
    Row("pack", "vip_pack_h2", "pack_h2_kernel", GEMM_KINDS, "the fp32 input is the operand: +-70000 in it", lambda: _pack_case("pack")),
    Row("window_mfma", "vip_window_attn_fwd_h2", "attn_h2_kernel", FINITE, NO_OVER["attention"], lambda: _window_case("window_mfma", 7, 2, "attn_h2_kernel")),
    Row("window_valu", "vip_window_attn_fwd_h2", "sattn_kernel", FINITE, NO_OVER["attention"] + "; ws = 5 is not built on the MFMA kernel",
        lambda: _window_case("window_valu", 5, 2, "sattn_kernel")),
    Row("mhsa_mfma", "vip_mhsa_fwd_h2", "attn_h2_kernel", FINITE, NO_OVER["attention"], lambda: _mhsa_case("mhsa_mfma", 50, "attn_h2_kernel")),
    Row("mhsa_valu", "vip_mhsa_fwd_h2", "sattn_kernel", FINITE, NO_OVER["attention"] + "; N = 230 > 224 is not built on the MFMA kernel",
        lambda: _mhsa_case("mhsa_valu", 230, "sattn_kernel")),
    Row("global_filter", "vip_global_local_filter_nhwc_h2", "global_local_filter_kernel", GEMM_KINDS, "one-hot through the global filter",
        lambda: _gf_case("global_filter")),
    Row("swin", "vip_swin_attn_fwd_h2", "swin_attn_kernel", FINITE, NO_OVER["attention"] + " (v_bias only fills padded tokens)",
        lambda: _swin_case("swin")),
    Row("nat", "vip_nat_attn_fwd_h2", "nat_attn_kernel", FINITE, NO_OVER["attention"], lambda: _nat_case("nat")),
]
BY_ID = {r.id: r for r in ROWS}
ENTRY_POINTS = {r.entry for r in ROWS}
_CASES = {}


def case_of(row, *args):
    """the row's Case, built once per process (`args`: the MLP plan's workgroup count, on the GPU)"""
    key = (row.id,) + args
    if key not in _CASES:
        _CASES[key] = row.build(*args)
    return _CASES[key]


def positions(row, kind):
    """where a row's triggers of `kind` sit (static, so that collecting the tests builds no operands; check() holds it against the
    Case): interior and edge, a later pass for the persistent MLP row; vit_tokens' two spots serve one sign each"""
    if kind == "clean":
        return ("-",)
    if row.id == "vit_tokens" and kind in ("over+", "over-"):
        return ("interior",) if kind == "over+" else ("edge",)
    return ("interior", "pass2", "edge") if row.id == "mlp_passes" else POSITIONS


def params(rows=None):
    """(row id, kind, position) of every case, in table order"""
    return [(r.id, kind, pos) for r in rows or ROWS for kind in r.kinds for pos in positions(r, kind)]


def triggered(case, kind, pos):
    """(operands with the trigger applied, the Trigger or None)"""
    if kind == "clean":
        return case.operands, None
    t = case.triggers[(kind, pos)]
    o = dict(case.operands)
    o[t.name] = o[t.name].clone()
    o[t.name][t.index] = t.value
    return o, t


_REF = {}


def check(row, kind, pos, *args):
    """Asserts the issue's conditions in fp64 and returns (reference, mask of the elements a GPU result is NOT compared on: those out of
    range and those that depend on the poisoned value)."""
    key = (row.id, kind, pos) + args
    if key in _REF:
        return _REF[key]
    case = case_of(row, *args)
    assert {(k, p) for k in row.kinds for p in positions(row, k) if k != "clean"} == set(case.triggers), row.id
    o, t = triggered(case, kind, pos)
    for name, st in case.storage.items():
        if st == "packed" or (st == "f32" and row.id != "pack"):
            v = o[name][~torch.isnan(o[name])]
            assert v.abs().max() <= H2_MAX, f"{row.id}/{kind}: operand {name} leaves the range by itself"
    ref = case.ref(o)
    finite = torch.isfinite(ref)
    mag = torch.where(finite, ref.abs(), torch.zeros_like(ref))
    assert not ((mag >= BAND[0]) & (mag < BAND[1])).any(), f"{row.id}/{kind}/{pos}: a reference element lies in the band {BAND}"
    over = mag >= BAND[1]
    skip = over | ~finite
    if kind == "clean":
        assert finite.all() and mag.max() <= CLEAN_MAX, f"{row.id}: clean max |ref| {mag.max()} > {CLEAN_MAX}"
    elif kind == "nan":
        assert (~finite).any() and not over.any(), f"{row.id}/{pos}: nothing depends on the poisoned element, or something overflows"
        assert finite.any(), f"{row.id}/{pos}: every output depends on the poisoned element"
    else:
        assert finite.all()
        named = torch.zeros_like(over)
        for idx in t.over:
            named[idx] = True
        assert torch.equal(over, named), f"{row.id}/{kind}/{pos}: out of range {over.nonzero().tolist()[:8]}, named {t.over}"
        assert (kind == "hidden") != bool(t.over)
        if kind in ("over+", "over-"):
            assert all((ref[idx] > 0) == (kind == "over+") for idx in t.over)
        for idx in t.dep or ():
            skip[idx] = True
    _REF[key] = (ref, skip)
    return _REF[key]


def upload(ops, case, o, trigger=None):
    """the operands on the device: packed activations through pack_h2 (clean values; a nan trigger is then written into the hi half of
    the packed element itself), fp32 parameters as they are, weights through the project's constructors"""
    dev = {}
    for name, st in case.storage.items():
        if st is None:
            continue
        nan_here = trigger is not None and trigger.name == name and math.isnan(trigger.value)
        if st == "packed":
            dev[name] = _pack(ops, case.operands[name] if nan_here else o[name])
            if nan_here:
                poison(dev[name], trigger.index)
        elif st == "f32":
            dev[name] = _f32(o[name])
        else:
            dev[name] = st(ops, o)
    return dev


def poison(packed, index):
    """hi half of logical element `index` of a packed tensor := fp16 NaN; 8 channels are 32 bytes [hi x 8][lo x 8]"""
    halves = packed.view(torch.int16)                       # last axis: 2 C halfs
    c = index[-1]
    halves[tuple(index[:-1]) + ((c // 8) * 16 + c % 8,)] = NAN16
