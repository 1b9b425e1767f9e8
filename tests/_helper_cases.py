"""The memory-bound NHWC helper kernels of the three storages - pooling, global average pool, scale_add_act, mul, radix_combine, LayerNorm,
the classifier heads, the score kernels (csrc/pointwise.hip, csrc/strict_ops.hip) - at their own edge shapes, on operands whose correct
result is EXACT wherever that is possible.

Exact operands (operands(row), seeded by zlib.crc32 of the row id): activations x and residuals are integers in [-4, 4], gates and scales
multiples of 1/4 in [0, 2], fp32 parameters (LayerNorm gamma / beta, head matrices and biases) multiples of 1/4.  Every product is then
a multiple of 1/16 and every partial sum any kernel can form stays far below 2^24 of those units: the sums are exact in fp32 in ANY
order, with or without FMA.  What a row is held to is its `accept`:
  "exact"    the output equals the fp64 reference under torch.equal (numerically: -0.0 == +0.0); the reference is representable in the
             row's storage (fp16; packed: the lo plane is 0; fp32);
  "round16"  fp16 storage only: the exact value is a small integer over a tap / pixel count (pooling, global average pool) or an exact
             fp32 value with more than 11 bits (split gates); the output equals the fp64 reference ROUNDED TO FP16 bit for bit.  For the
             quotients tests/test_helper_cases_cpu.py enumerates every reachable sum over every divisor the table uses: the fp16
             rounding is the same whether the fp32 kernel divides, multiplies by a rounded reciprocal or lands 2 ulp32 off;
  a name     of TOLERANCES: only what cannot be exact (non-dyadic quotients in the 22 / 24 bit storages, silu / gelu / sigmoid,
             LayerNorm on structured rows, heads behind a LayerNorm or a 49-pixel mean, exp) - an existing tolerance of the project,
             none new, with the error taken per channel chunk (scale_add_act) or per row (LayerNorm) where the issue says so.
tests/test_helper_cases_cpu.py proves the claims, and that each classic mistake (MUTANTS) moves some row's reference by more than
the row accepts, without a GPU; tests/test_gpu_helpers.py runs the rows.

KERNELS is the list of (storage, kernel) every row's `kernel` field may name; the CPU test holds it against the __global__ functions of
the two files.  Not covered here: the depthwise kernels (tests/_dw_cases.py), the attention cores (tests/_attn_cases.py), vit_tokens,
pack / unpack (tests/test_gpu_strict.py), tile_aggregate (tests/test_gpu_tiles.py), and what sits behind a once-per-process environment
switch (the stride-1 sdwconv_kernel<SH2> of VIP_DW_H2_TILE=0, the VALU attention of VIP_ATTN_H2_MFMA=0).

Selection of the LayerNorm kernels (vip_layernorm_f16, layernorm_impl<SH2>): C8 = C / 8, lpr = the smallest of 8, 16, 32, 64 that is >= C8
(64 beyond), CPL = ceil(C8 / lpr) <= 4; the fp32 storage - and the packed one beyond 2048 channels - takes slayernorm_kernel with one
wave per row and 1, 2, 4, 8 or 16 float4 chunks per lane.  ln_geometry(C) is that formula."""
import math
import zlib
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ops_ref as R

Row = namedtuple("Row", "id op storage kernel accept what p")

STORAGES = ("f16", "h2", "s32")
CHUNK = {"f16": 8, "h2": 4, "s32": 4}                 # channels per thread of the elementwise kernels
GRID_CAP = 8192 * 256                                 # grid_for (pointwise.hip) / sgrid (strict_ops.hip): 8192 workgroups of 256 threads
TOL_OF = {"f16": "TOL_F16", "h2": "TOL_OP", "s32": "TOL_OP"}
# tolerance name -> where the project already uses it: a constant of tests/test_gpu_passes.py, or a literal of the test of
# tests/test_gpu_ops.py named here, for the operator named here
TOLERANCES = {
    "TOL_F16": ("test_gpu_passes", None),
    "TOL_OP": ("test_gpu_passes", None),
    "1e-5": ("test_gpu_ops", {"gap_dense": "test_scale_add_act_and_head", "gap_ln_dense": "test_gap_ln_dense_head"}),
    "1e-6": ("test_gpu_ops", {"gap_split": "test_split_vector_chain", "ensemble_mean": "test_score_kernels"}),
    "2e-6": ("test_gpu_ops", {"head_prob": "test_score_kernels", "head_act": "test_score_kernels"}),
}

KERNELS = (
    ("f16", "pool2d_kernel"), ("f16", "gap_kernel"), ("f16", "scale_add_act_kernel"), ("f16", "layernorm_kernel"),
    ("f16", "gap_dense_kernel"), ("f16", "gap_ln_dense_kernel"), ("f16", "mul_kernel"), ("f16", "radix_combine_kernel"),
    ("f32", "head_prob_kernel"), ("f32", "prob_to_score_kernel"), ("f32", "ensemble_mean_kernel"), ("f32", "head_act_kernel"),
    ("h2", "spool2d_kernel"), ("s32", "spool2d_kernel"), ("h2", "sgap_kernel"), ("s32", "sgap_kernel"),
    ("h2", "sscale_add_act_kernel"), ("s32", "sscale_add_act_kernel"), ("h2", "h2_layernorm_kernel"), ("h2", "slayernorm_kernel"),
    ("s32", "slayernorm_kernel"), ("h2", "smul_kernel"), ("s32", "smul_kernel"), ("h2", "sradix_combine_kernel"),
    ("s32", "sradix_combine_kernel"), ("h2", "sgap_ln_dense_kernel"), ("s32", "sgap_ln_dense_kernel"),
)
# the __global__ functions of the two files that this table leaves to other tests
ELSEWHERE = {"dwconv_kernel", "sdwconv_kernel", "tile_aggregate_kernel", "svit_tokens_kernel", "sattn_kernel", "pack_h2_kernel", "unpack_h2_kernel"}

_K = {"pool2d": ("pool2d_kernel", "spool2d_kernel"), "gap": ("gap_kernel", "sgap_kernel"),
      "scale_add_act": ("scale_add_act_kernel", "sscale_add_act_kernel"), "mul": ("mul_kernel", "smul_kernel"),
      "radix_combine": ("radix_combine_kernel", "sradix_combine_kernel")}


def _kernel(op, storage):
    return _K[op][0 if storage == "f16" else 1]


# ---- pool2d -----------------------------------------------------------------------------------------------------------------------------
MAX, AVG_VALID, AVG_FULL = 0, 1, 2
_POOL_GEOM = [
    # id, H, W, C, k, stride, pad, modes, x, out_hw, what
    ("k3s2-odd", 9, 7, 24, 3, 2, (1, 1, 1, 1), (0, 1, 2), "int", None, "k = 3 stride 2 pad 1 on an odd 9 x 7 map: 5 x 4 outputs, counts 4 / 6 / 9; C = 24: 3 fp16 chunks, 6 fp32 chunks"),
    ("k3s2-even", 8, 10, 8, 3, 2, (1, 1, 1, 1), (0, 1, 2), "int", None, "the same window on an even 8 x 10 map: only the top / left border is padded; C = 8: one chunk"),
    ("k2s2-odd", 9, 7, 136, 2, 2, (0, 1, 0, 1), (0, 1, 2), "int", None, "k = 2 stride 2 pad (0,1,0,1) on odd H and W: counts 1 / 2 / 4, all dyadic; C = 136 is no multiple of 64"),
    ("k3s1", 7, 5, 24, 3, 1, (1, 1, 1, 1), (0, 1, 2), "int", None, "k = 3 stride 1 pad 1: every border window is padded, 7 x 5 outputs"),
    ("max-negative", 9, 7, 8, 3, 2, (1, 1, 1, 1), (0,), "neg", None, "an all-negative map: the padded zero must win the max of every border window"),
    ("max-positive", 9, 7, 8, 3, 2, (1, 1, 1, 1), (0,), "pos", None, "an all-positive map: the padded zero never wins"),
    ("avg-small", 2, 2, 24, 3, 1, (1, 1, 1, 1), (1,), "int", None, "a 2 x 2 map under a 3 x 3 window: every count is 4 < k * k"),
    ("k1-pad", 5, 6, 24, 1, 1, (0, 1, 1, 2), (0,), "int", None, "k = 1 zero-padded copy, pad (0,1,1,2): 6 x 9 outputs (GCViT FitWindow)"),
    ("k1-crop", 6, 5, 136, 1, 1, (0, 0, 0, 0), (0,), "int", (4, 3), "k = 1 crop through out_hw = (4, 3)"),
]
_POOL_BIG = {"f16": (3, 300, 301, 64), "h2": (3, 300, 301, 32), "s32": (3, 300, 301, 32)}     # 2 167 200 chunks of 8 / 4 channels


def _pool_rows():
    out = []
    for st in STORAGES:
        for gid, H, W, Cc, k, s, pad, modes, xk, ohw, what in _POOL_GEOM:
            for m in modes:
                p = dict(B=3, H=H, W=W, C=Cc, k=k, stride=s, pad=pad, mode=m, x=xk, out_hw=ohw, ldx=None, ldy=None, big=False)
                out.append(Row(f"pool-{st}-{gid}-m{m}", "pool2d", st, _kernel("pool2d", st), None, what, p))
        p = dict(B=3, H=9, W=7, C=24, k=3, stride=2, pad=(1, 1, 1, 1), mode=1, x="int", out_hw=None, ldx=32, ldy=40, big=False)
        out.append(Row(f"pool-{st}-ld-m1", "pool2d", st, _kernel("pool2d", st), None,
                       "ldx = C + 8, ldy = C + 16: the input a channel slice of a wider tensor, the output a slice of a sentinel-filled buffer", p))
        B, H, W, Cc = _POOL_BIG[st]
        p = dict(B=B, H=H, W=W, C=Cc, k=1, stride=1, pad=(0, 0, 0, 0), mode=0, x="int", out_hw=None, ldx=None, ldy=None, big=True)
        out.append(Row(f"pool-{st}-second-pass", "pool2d", st, _kernel("pool2d", st), None,
                       f"k = 1 copy of {B * H * W * Cc // CHUNK[st]} chunks: the grid-stride loop runs a second pass past {GRID_CAP} threads", p))
    return [r._replace(accept=_pool_accept(r)) for r in out]


def pool_out_hw(p):
    if p["out_hw"]:
        return p["out_hw"]
    pt, pb, pl, pr = p["pad"]
    return (p["H"] + pt + pb - p["k"]) // p["stride"] + 1, (p["W"] + pl + pr - p["k"]) // p["stride"] + 1


def pool_ref(x, p, wrong=None):
    """[B,H,W,C] -> (pooled fp64 [B,Ho,Wo,C], valid-tap counts [Ho,Wo]); the window of output (ho, wo) starts at (ho * stride - pt,
    wo * stride - pl), as the entry points define it (pb / pr only decide Ho, Wo)"""
    k, s, mode = p["k"], p["stride"], p["mode"]
    pt, _, pl, _ = p["pad"]
    Ho, Wo = pool_out_hw(p)
    if wrong == "pads swapped between top and left":
        pt, pl = pl, pt
    H, W = x.shape[1:3]
    nh, nw = (Ho - 1) * s + k, (Wo - 1) * s + k
    geom = (pl, max(0, nw - W - pl), pt, max(0, nh - H - pt))
    fill = -math.inf if wrong == "max pooling with -inf padding" else 0.0
    xp = F.pad(x.double().permute(0, 3, 1, 2), geom, value=fill)[:, :, :nh, :nw]
    ones = F.pad(torch.ones(1, 1, H, W, dtype=torch.float64), geom)[:, :, :nh, :nw]
    cnt = F.avg_pool2d(ones, k, s, divisor_override=1)
    if mode == MAX:
        y = F.max_pool2d(xp, k, s)
    else:
        num = F.avg_pool2d(xp, k, s, divisor_override=1)              # exact integer sums
        valid = (mode == AVG_VALID) != (wrong in ("mode 1 divided by k*k", "mode 2 divided by the valid count"))
        y = num / (cnt.clamp(min=1) if valid else float(k * k))
    return y.permute(0, 2, 3, 1).contiguous(), cnt[0, 0]


def pool_divisors(p):
    """the divisors a row's outputs use"""
    if p["mode"] == MAX:
        return set()
    if p["mode"] == AVG_FULL:
        return {p["k"] * p["k"]}
    _, cnt = pool_ref(torch.zeros(1, p["H"], p["W"], 1), p)
    return {int(c) for c in cnt.flatten().tolist() if c > 0}


def _dyadic(n):
    return n & (n - 1) == 0


def _pool_accept(r):
    if r.storage == "f16":
        return "exact" if all(_dyadic(d) for d in pool_divisors(r.p)) else "round16"
    return "exact" if all(_dyadic(d) for d in pool_divisors(r.p)) else "TOL_OP"


# ---- global average pool ------------------------------------------------------------------------------------------------------------------
GAP_HW = (1, 5, 31, 32, 33, 49, 65, 143)
GAP_C = (8, 72, 136)


def _gap_rows():
    out = []
    forms = [("f16", False, "gap_kernel", "vip_global_avgpool_f16"), ("f16", True, "gap_kernel", "vip_global_avgpool_split_f16"),
             ("h2", False, "sgap_kernel", "vip_global_avgpool_h2"), ("s32", False, "sgap_kernel", "vip_global_avgpool_s32")]
    for st, split, kern, entry in forms:
        lanes = 32 if st == "f16" else 16
        tag = f"gap-{st}{'-split' if split else ''}"
        for HW in GAP_HW:
            for Cc in GAP_C:
                acc = "1e-6" if split else "round16" if st == "f16" else "exact" if _dyadic(HW) else "TOL_OP"
                what = (f"{entry}: {HW} pixels over {lanes} pixel lanes ({-(-HW // lanes)} turn(s), {HW % lanes or lanes} live in the last); "
                        f"C = {Cc}: {-(-Cc // 64)} slab(s), {Cc % 64 or 64} channels in the last")
                out.append(Row(f"{tag}-hw{HW}-c{Cc}", "gap", st, kern, acc, what, dict(B=3, HW=HW, C=Cc, split=split, ldx=None)))
        acc = "1e-6" if split else "round16" if st == "f16" else "TOL_OP"
        out.append(Row(f"{tag}-ld", "gap", st, kern, acc, f"{entry}: ldx = C + 8, the input a channel slice of a wider tensor; 33 pixels, C = 72",
                       dict(B=3, HW=33, C=72, split=split, ldx=80)))
    return out


def gap_ref(x, p, wrong=None):
    HW = p["HW"]
    div = -(-HW // 32) * 32 if wrong == "pooled mean divided by 32-rounded HW" else HW
    return x.double().sum(1) / div


# ---- scale_add_act ------------------------------------------------------------------------------------------------------------------------
SAA_SHAPE = (3, 5, 24)                    # B, HW, C: 15 chunks of 8 (30 of 4), idx / C8 / HW crosses the images inside one block
_SAA_BIG = {"f16": (3, 90300, 64), "h2": (3, 90300, 32), "s32": (3, 90300, 32)}
LO_UNIT = 2.0 ** -14                      # split gates / radix weights: the lo plane holds multiples of 2^-14 in [-4, 4] * 2^-14


def _saa_rows():
    out = []
    for st in STORAGES:
        kern = _kernel("scale_add_act", st)
        scales = (None, "plain", "split") if st == "f16" else (None, "plain")
        for sc in scales:
            for res in (False, True):
                name = f"{'gate' if sc == 'plain' else 'split' if sc else 'nogate'}-{'res' if res else 'nores'}"
                base = (f"scale {'absent' if sc is None else 'a split (hi, lo) gate, scale_planes = 2' if sc == 'split' else 'per image'}, "
                        f"residual {'present' if res else 'absent'}; HW = 5, C = 24: the image index changes mid-block")
                for act in (None, "relu"):
                    acc = "round16" if sc == "split" else "exact"
                    out.append(Row(f"saa-{st}-{name}-{act or 'none'}", "scale_add_act", st, kern, acc, base,
                                   dict(shape=SAA_SHAPE, scale=sc, res=res, act=act, act2=None, big=False)))
                for act in ("silu", "gelu", "sigmoid"):
                    out.append(Row(f"saa-{st}-{name}-{act}", "scale_add_act", st, kern, TOL_OF[st], base + f"; {act}: per channel chunk",
                                   dict(shape=SAA_SHAPE, scale=sc, res=res, act=act, act2=None, big=False)))
        for sc in scales[1:]:
            out.append(Row(f"saa-{st}-{'gate' if sc == 'plain' else 'split'}-two-outputs", "scale_add_act", st, kern,
                           "round16" if sc == "split" else "exact", "two outputs, y and act2 = relu of the rounded y, from one launch",
                           dict(shape=SAA_SHAPE, scale=sc, res=True, act=None, act2="relu", big=False)))
        B, HW, Cc = _SAA_BIG[st]
        out.append(Row(f"saa-{st}-second-pass", "scale_add_act", st, kern, "exact",
                       f"{B * HW * Cc // CHUNK[st]} chunks: a second pass of the grid-stride loop past {GRID_CAP} threads; gate, residual, relu",
                       dict(shape=_SAA_BIG[st], scale="plain", res=True, act="relu", act2=None, big=True)))
    return out


def _gate(g, shape, split):
    """(hi, lo) of a gate [B, C]; split: lo is a multiple of 2^-14, and every third channel has hi = 0"""
    hi = torch.randint(0, 9, shape, generator=g).float() / 4
    if not split:
        return hi, None
    lo = torch.randint(-4, 5, shape, generator=g).float() * LO_UNIT
    hi[..., ::3] = 0
    return hi, lo


def saa_ref(o, p, wrong=None):
    """(y, y2 or None) in fp64"""
    v = o["x"].double()
    if o["hi"] is not None:
        s = o["hi"].double()
        if o["lo"] is not None and wrong != "lo plane dropped":
            s = s + o["lo"].double()
        if wrong == "scale or gate taken from image 0":
            s = s[:1].expand_as(s)
        v = v * s[:, None, :]
    if o["r"] is not None:
        v = v + o["r"].double()
    y = R.act(v, p["act"])
    return y, (R.act(y, p["act2"]) if p["act2"] else None)


# ---- mul ----------------------------------------------------------------------------------------------------------------------------------
def _mul_rows():
    out = []
    for st in STORAGES:
        kern = _kernel("mul", st)
        out.append(Row(f"mul-{st}-slices", "mul", st, kern, "exact",
                       "a_off = 16 of lda = 56, b_off = 8 of ldb = 48, y_off = 24 of ldy = 64, C = 24, 37 rows: the output inside a sentinel-filled buffer",
                       dict(rows=37, C=24, lda=56, a_off=16, ldb=48, b_off=8, ldy=64, y_off=24, big=False)))
        out.append(Row(f"mul-{st}-c8", "mul", st, kern, "exact", "C = 8: one chunk per row, 5 rows",
                       dict(rows=5, C=8, lda=24, a_off=8, ldb=16, b_off=8, ldy=32, y_off=16, big=False)))
        Cc = 64 if st == "f16" else 32
        out.append(Row(f"mul-{st}-second-pass", "mul", st, kern, "exact",
                       f"{270900 * Cc // CHUNK[st]} chunks: a second pass of the grid-stride loop past {GRID_CAP} threads, still on slices",
                       dict(rows=270900, C=Cc, lda=Cc + 8, a_off=8, ldb=Cc + 16, b_off=16, ldy=Cc + 8, y_off=0, big=True)))
    return out


def mul_ref(o, p, wrong=None):
    a0, b0 = (0, 0) if wrong == "offsets ignored in mul" else (p["a_off"], p["b_off"])
    return o["a"][:, a0:a0 + p["C"]].double() * o["b"][:, b0:b0 + p["C"]].double()


# ---- radix_combine ------------------------------------------------------------------------------------------------------------------------
def _radix_rows():
    out = []
    for st in STORAGES:
        kern = _kernel("radix_combine", st)
        for planes in ((1, 2) if st == "f16" else (1,)):
            for radix in (1, 2, 4):
                for Cc in (8, 40):
                    out.append(Row(f"radix-{st}-r{radix}-c{Cc}{'-split' if planes == 2 else ''}", "radix_combine", st, kern,
                                   "round16" if planes == 2 else "exact",
                                   f"radix {radix}, C = {Cc}, HW = 5, B = 3: another scale per radix and per image"
                                   + ("; split (hi, lo) scales, planes = 2" if planes == 2 else ""),
                                   dict(B=3, HW=5, C=Cc, radix=radix, planes=planes, big=False)))
        Cc = 64 if st == "f16" else 32
        out.append(Row(f"radix-{st}-second-pass", "radix_combine", st, kern, "exact",
                       f"{3 * 90300 * Cc // CHUNK[st]} output chunks, radix 2: a second pass of the grid-stride loop past {GRID_CAP} threads",
                       dict(B=3, HW=90300, C=Cc, radix=2, planes=1, big=True)))
    return out


def radix_ref(o, p, wrong=None):
    B, HW, Cc, radix = p["B"], p["HW"], p["C"], p["radix"]
    s = o["hi"].double()
    if o["lo"] is not None and wrong != "lo plane dropped":
        s = s + o["lo"].double()
    if wrong == "scale or gate taken from image 0":
        s = s[:1].expand_as(s)
    s = s.reshape(B, 1, radix, Cc)
    if wrong == "radix order reversed":
        s = s.flip(2)
    return (o["x"].double().reshape(B, HW, radix, Cc) * s).sum(2)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------------------
LN_C = (8, 24, 64, 96, 136, 520, 1024, 1032, 1536, 2040, 2048)        # the issue's list, and 64 / 1024: CPL 1 and 2 with a full last chunk
LN_EPS = 1e-6


def ln_geometry(C):
    """(lpr, CPL, whether the last chunk turn is partial) of vip_layernorm_f16 / h2_layernorm_kernel; CPL > 4: not taken"""
    C8 = C // 8
    lpr = 8
    while lpr < 64 and lpr < C8:
        lpr <<= 1
    return lpr, -(-C8 // lpr), C8 % lpr != 0


def sln_template(C):
    """CPL template of slayernorm_kernel"""
    cpl = -(-(C // 4) // 64)
    return next(t for t in (1, 2, 4, 8, 16) if cpl <= t)


def ln_kernel(storage, C):
    if storage == "f16" or (storage == "h2" and ln_geometry(C)[1] <= 4):
        lpr, cpl, part = ln_geometry(C)
        name = "layernorm_kernel" if storage == "f16" else "h2_layernorm_kernel"
        return name, f"{name}<{cpl}> lpr {lpr} CPL {cpl}, last chunk turn {'partial' if part else 'full'}"
    t = sln_template(C)
    return "slayernorm_kernel", f"slayernorm_kernel<{t}>: {C // 4} float4 chunks over 64 lanes"


def _ln_rows():
    out = []
    for st in STORAGES:
        Cs = LN_C + {"f16": (), "h2": (2056,), "s32": (264, 2056, 4096)}[st]        # slayernorm_kernel<2>, <16>
        for Cc in Cs:
            kern, geo = ln_kernel(st, Cc)
            out.append(Row(f"ln-{st}-c{Cc}-const", "layernorm", st, kern, "exact", f"{geo}; 37 constant rows (a tail block): the output is beta",
                           dict(rows=37, C=Cc, kind="const")))
            out.append(Row(f"ln-{st}-c{Cc}-const-one-row", "layernorm", st, kern, "exact", f"{geo}; one row: a block with one live row",
                           dict(rows=1, C=Cc, kind="const")))
            out.append(Row(f"ln-{st}-c{Cc}-structured", "layernorm", st, kern, TOL_OF[st],
                           f"{geo}; 37 rows: scales 2^6 apart with means of either sign, one spike in a zero row, mean 100 with spread 0.25; "
                           "the error per row, and a row-permuted input gives the row-permuted output",
                           dict(rows=37, C=Cc, kind="structured")))
    return out


def ln_ref(o, p, wrong=None, storage="f16"):
    x, g, b = o["x"].double(), o["gamma"].double(), o["beta"].double()
    if wrong is None:
        return R.layernorm(x, g, b, LN_EPS)
    m = x.mean(-1, keepdim=True)
    sq = ((x - m) ** 2).sum(-1, keepdim=True)
    n = x.shape[-1]
    if wrong == "LayerNorm variance divided by the padded channel count":
        lpr, cpl, _ = ln_geometry(n)
        n = lpr * cpl * 8
    v = sq / n
    if wrong == "LayerNorm statistics shared between neighbouring rows":
        idx = torch.arange(x.shape[0]) // 2 * 2              # the even row's statistics serve the pair
        m, v = m[idx], v[idx]
    return (x - m) / torch.sqrt(v + LN_EPS) * g + b


# ---- classifier heads ---------------------------------------------------------------------------------------------------------------------
HEAD_C = (8, 264, 2056, 4096)
HEAD_HW = (1, 4, 49)
HEAD_EPS = 1e-6


def _head_rows():
    out = []
    forms = [("gap_dense", "f16", "gap_dense_kernel"), ("gap_ln_dense", "f16", "gap_ln_dense_kernel")]
    forms += [(k, st, "sgap_ln_dense_kernel") for st in ("h2", "s32") for k in ("gap_dense", "gap_ln_dense")]
    for kind, st, kern in forms:
        for i, Cc in enumerate(HEAD_C):
            for j, HW in enumerate(HEAD_HW):
                N, bias = (1, 5)[(i + j) % 2], (i + j // 2) % 2 == 0
                exact = kind == "gap_dense" and HW in (1, 4)
                acc = "exact" if exact else "1e-5" if st == "f16" else "TOL_OP"
                turns = f"{Cc // 8} chunks of 8 over 256 threads" if st == "f16" else f"{Cc // 4} chunks of 4 over 256 threads"
                out.append(Row(f"head-{kind}-{st}-c{Cc}-hw{HW}-n{N}{'' if bias else '-nobias'}", "head", st, kern, acc,
                               f"{kind}: C = {Cc} ({turns}), {HW} pixels, N = {N}, bias {'present' if bias else 'absent'}, B = 3",
                               dict(kind=kind, B=3, HW=HW, C=Cc, N=N, bias=bias, ldx=None)))
        if kind == "gap_ln_dense":
            out.append(Row(f"head-{kind}-{st}-ld", "head", st, kern, "1e-5" if st == "f16" else "TOL_OP",
                           "ldx = C + 8: the input a channel slice of a wider tensor; C = 264, 4 pixels, N = 5",
                           dict(kind=kind, B=3, HW=4, C=264, N=5, bias=True, ldx=272)))
    for st, kern in (("f16", "gap_dense_kernel"), ("h2", "sgap_ln_dense_kernel"), ("s32", "sgap_ln_dense_kernel")):
        for Cc, N, bias in ((8, 1, True), (2056, 5, False)):
            out.append(Row(f"head-cls_dense-{st}-c{Cc}-n{N}{'' if bias else '-nobias'}", "head", st, kern, "exact",
                           f"cls_dense_f32: token 0 of [3, 3, {Cc}] - one pixel, image stride 3 * C; N = {N}",
                           dict(kind="cls_dense", B=3, HW=1, C=Cc, N=N, bias=bias, ldx=None)))
    return out


def head_ref(o, p, wrong=None):
    x = o["x"].double()
    if p["kind"] == "cls_dense":
        x = x[:, :1]
    if wrong == "head reading channel c % 2048":
        x = x[..., torch.arange(x.shape[-1]) % 2048]
    HW = x.shape[1]
    div = -(-HW // 32) * 32 if wrong == "pooled mean divided by 32-rounded HW" else HW
    v = x.sum(1) / div
    if p["kind"] == "gap_ln_dense":
        v = R.layernorm(v, o["gamma"].double(), o["beta"].double(), HEAD_EPS)
    return R.dense(v, o["w"].double().t(), None if o["bias"] is None else o["bias"].double())


# ---- score kernels ------------------------------------------------------------------------------------------------------------------------
def _score_rows():
    out = []
    for B in (1, 257):
        for N in (1, 2, 5):
            shape = f"B = {B} ({'one live thread' if B == 1 else 'a second workgroup with one live thread'}), N = {N}; logits with +-100 and +-88"
            out.append(Row(f"score-head_prob-b{B}-n{N}", "score", "f32", "head_prob_kernel", "2e-6",
                           f"default pairing ({'sigmoid' if N == 1 else 'softmax'}); {shape}", dict(kind="head_prob", B=B, N=N, act="default")))
            out.append(Row(f"score-head_act-linear-b{B}-n{N}", "score", "f32", "head_act_kernel", "exact",
                           f"linear: a bit-exact copy; {shape}", dict(kind="head_act", B=B, N=N, act="linear")))
            out.append(Row(f"score-binary_score-b{B}-n{N}", "score", "f32", "prob_to_score_kernel", "exact",
                           f"{'p' if N == 1 else '1 - p[:, 0]'} in fp32, bit for bit; B = {B}, N = {N}", dict(kind="binary_score", B=B, N=N, act=None)))
        out.append(Row(f"score-head_act-sigmoid-b{B}-n5", "score", "f32", "head_act_kernel", "2e-6",
                       f"elementwise sigmoid on 5 classes; B = {B}", dict(kind="head_act", B=B, N=5, act="sigmoid")))
        out.append(Row(f"score-head_act-softmax-b{B}-n1", "score", "f32", "head_act_kernel", "exact",
                       f"softmax over one class: exactly 1.0; B = {B}", dict(kind="head_act", B=B, N=1, act="softmax")))
    for M in (1, 7, 8):
        out.append(Row(f"score-ensemble_mean-m{M}", "score", "f32", "ensemble_mean_kernel", "exact" if M in (1, 8) else "1e-6",
                       f"{M} members, 257 images in rows 264 floats apart" + ("; multiples of 2^-10: the mean is exact" if M in (1, 8) else ""),
                       dict(kind="ensemble_mean", M=M, n=257, ld=264)))
    return out


def logits(g, B, N):
    z = torch.randn(B, N, generator=g) * 4
    edge = torch.tensor([88.0, -100.0, 100.0, -88.0, 0.0])
    z[0] = edge[:N]
    if B > 4:
        z[1], z[2], z[3], z[4] = edge.roll(1)[:N], edge.roll(2)[:N], edge.roll(3)[:N], -edge[:N]
    return z


def score_ref(o, p):
    k = p["kind"]
    if k == "ensemble_mean":
        return o["s"].double().mean(0)
    z = o["z"].double()
    if k == "binary_score":                                   # o["z"] holds PROBABILITIES here; the arithmetic is one fp32 subtraction
        return (o["z"] if p["N"] == 1 else 1.0 - o["z"])[:, 0].double()
    act = p["act"]
    if act == "default":
        act = "sigmoid" if p["N"] == 1 else "softmax"
    return z if act == "linear" else torch.sigmoid(z) if act == "sigmoid" else torch.softmax(z, -1)


# ---- the table --------------------------------------------------------------------------------------------------------------------------
ROWS = _pool_rows() + _gap_rows() + _saa_rows() + _mul_rows() + _radix_rows() + _ln_rows() + _head_rows() + _score_rows()
BY_ID = {r.id: r for r in ROWS}

# the wrong variants the table must tell apart: name -> the operators whose reference functions know it
MUTANTS = {
    "mode 1 divided by k*k": ("pool2d",),
    "mode 2 divided by the valid count": ("pool2d",),
    "max pooling with -inf padding": ("pool2d",),
    "pads swapped between top and left": ("pool2d",),
    "scale or gate taken from image 0": ("scale_add_act", "radix_combine"),
    "lo plane dropped": ("scale_add_act", "radix_combine"),
    "radix order reversed": ("radix_combine",),
    "offsets ignored in mul": ("mul",),
    "LayerNorm statistics shared between neighbouring rows": ("layernorm",),
    "LayerNorm variance divided by the padded channel count": ("layernorm",),
    "pooled mean divided by 32-rounded HW": ("gap", "head"),
    "head reading channel c % 2048": ("head",),
}


def _gen(row):
    return torch.Generator().manual_seed(zlib.crc32(row.id.encode()))


def _ints(g, shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int8).float()


def _quarters(g, shape, lo, hi):
    return torch.randint(int(lo * 4), int(hi * 4) + 1, shape, generator=g).float() / 4


def h2_quantise(x):
    """what the packed storage holds of an fp32 tensor: hi = rn16(x), lo = rn16(x - hi), joined in fp32"""
    hi = x.half().float()
    return hi + (x - hi).half().float()


def _ln_structured(g, rows, Cc, storage):
    x = torch.zeros(rows, Cc)
    for r in range(rows):
        kind = r % 4
        if kind == 0:                                     # loud, positive mean
            x[r] = torch.randn(Cc, generator=g) * 64 + 96
        elif kind == 1:                                   # 2^-6 of its neighbour's scale, negative mean
            x[r] = torch.randn(Cc, generator=g) - 1.5
        elif kind == 2:                                   # one spike in a zero row
            x[r, (r * 7) % Cc] = 8.0
        else:                                             # mean 100, spread 0.25
            x[r] = torch.randn(Cc, generator=g) * 0.25 + 100
    return h2_quantise(x) if storage == "h2" else x.half().float()


def operands(row):
    """the row's operands as fp32 host tensors (None where absent), on the exact grid wherever the row is exact"""
    g, p = _gen(row), row.p
    if row.op == "pool2d":
        lo, hi = {"int": (-4, 4), "neg": (-4, -1), "pos": (1, 4)}[p["x"]]
        return dict(x=_ints(g, (p["B"], p["H"], p["W"], p["C"]), lo, hi))
    if row.op == "gap":
        return dict(x=_ints(g, (p["B"], p["HW"], p["C"])))
    if row.op == "scale_add_act":
        B, HW, Cc = p["shape"]
        o = dict(x=_ints(g, (B, HW, Cc)), hi=None, lo=None, r=None)
        if p["scale"]:
            o["hi"], o["lo"] = _gate(g, (B, Cc), p["scale"] == "split")
        if p["res"]:
            o["r"] = _ints(g, (B, HW, Cc))
            if p["scale"] == "split":
                o["r"][..., ::3] = 0                      # with hi = 0 there: x * lo is the whole result
        return o
    if row.op == "mul":
        return dict(a=_ints(g, (p["rows"], p["lda"])), b=torch.randint(0, 9, (p["rows"], p["ldb"]), generator=g, dtype=torch.int8).float() / 4)
    if row.op == "radix_combine":
        hi, lo = _gate(g, (p["B"], p["radix"], p["C"]), p["planes"] == 2)      # split: hi = 0 in every third OUTPUT channel, for every radix
        hi, lo = hi.reshape(p["B"], -1), None if lo is None else lo.reshape(p["B"], -1)
        return dict(x=_ints(g, (p["B"], p["HW"], p["radix"] * p["C"])), hi=hi, lo=lo)
    if row.op == "layernorm":
        rows, Cc = p["rows"], p["C"]
        if p["kind"] == "const":
            x = ((torch.arange(rows) * 5) % 9 - 4).float()[:, None].expand(rows, Cc).contiguous()
        else:
            x = _ln_structured(g, rows, Cc, row.storage)
        return dict(x=x, gamma=_quarters(g, (Cc,), 0.5, 2), beta=_quarters(g, (Cc,), -2, 2))
    if row.op == "head":
        B, HW, Cc, N = p["B"], p["HW"], p["C"], p["N"]
        tokens = 3 if p["kind"] == "cls_dense" else HW
        o = dict(x=_ints(g, (B, tokens, Cc)), w=_quarters(g, (N, Cc), -2, 2), bias=_quarters(g, (N,), -2, 2) if p["bias"] else None)
        if p["kind"] == "gap_ln_dense":
            o["gamma"], o["beta"] = _quarters(g, (Cc,), 0.5, 2), _quarters(g, (Cc,), -2, 2)
        return o
    if row.op == "score":
        if p["kind"] == "ensemble_mean":
            s = torch.randint(0, 1025, (p["M"], p["n"]), generator=g).float() / 1024 if p["M"] in (1, 8) else torch.rand(p["M"], p["n"], generator=g)
            return dict(s=s)
        if p["kind"] == "binary_score":
            return dict(z=torch.rand(p["B"], p["N"], generator=g))
        return dict(z=logits(g, p["B"], p["N"]))
    raise ValueError(row.op)


def reference(row, o, wrong=None):
    """the fp64 reference of a row on its operands (a tuple for two-output rows); `wrong`: one of MUTANTS instead"""
    p = row.p
    if row.op == "pool2d":
        return pool_ref(o["x"], p, wrong)[0]
    if row.op == "gap":
        return gap_ref(o["x"], p, wrong)
    if row.op == "scale_add_act":
        y, y2 = saa_ref(o, p, wrong)
        return y if y2 is None else (y, y2)
    if row.op == "mul":
        return mul_ref(o, p, wrong)
    if row.op == "radix_combine":
        return radix_ref(o, p, wrong)
    if row.op == "layernorm":
        return ln_ref(o, p, wrong, row.storage)
    if row.op == "head":
        return head_ref(o, p, wrong)
    assert wrong is None
    return score_ref(o, p)


def round16(t):
    """fp64 -> the nearest fp16 (ties to even, ONE rounding), as fp64"""
    return torch.from_numpy(t.numpy().astype(np.float16).astype(np.float64))


def expected(row, ref):
    """what an exact row's output must equal: the reference itself, or its fp16 rounding"""
    return round16(ref) if row.accept == "round16" else ref


def tolerance(row, passes):
    """the value of the row's tolerance name (None for exact rows); `passes`: the module tests/test_gpu_passes.py"""
    if row.accept in ("exact", "round16"):
        return None
    return getattr(passes, row.accept) if row.accept.startswith("TOL_") else float(row.accept)


def group_of(row):
    """how a tolerance row takes its error: 'chunk' (per channel chunk of the storage, over all pixels and images), 'row' (per row against
    that row's own absmax) or 'global' (the existing metric: the global maximum)"""
    return {"scale_add_act": "chunk", "layernorm": "row"}.get(row.op, "global")


def rel_error(row, got, ref):
    """the worst error of `got` against `ref` relative to the output scale of its group (+ 1e-6, as tests/test_gpu_ops.py::check), and
    where: (worst relative error, flat index of that element)"""
    how = group_of(row)
    d = (got - ref).abs()
    if how == "chunk":
        ch = CHUNK[row.storage]
        scale = ref.abs().reshape(-1, ref.shape[-1] // ch, ch).amax((0, 2))                   # [chunks]
        scale = scale.repeat_interleave(ch).expand_as(ref.reshape(-1, ref.shape[-1])).reshape(ref.shape)
    elif how == "row":
        scale = ref.abs().amax(-1, keepdim=True).expand_as(ref)
    else:
        scale = ref.abs().max().expand_as(ref)
    rel = (d / (scale + 1e-6)).flatten()
    i = int(rel.argmax())
    return rel[i].item(), i
