"""Every GEMM and k x k convolution kernel of the three storages on operands whose result is EXACT: no tolerance anywhere.

Kernels: conv_igemm_kernel, pw_gemm_kernel, pwk_direct_kernel, pwk_gemm_kernel with and without im2col staging, gemm8p_kernel and
rows_gemm_kernel of csrc/conv_igemm.hip (fp16 storage) and of its packed build csrc/conv_h2.hip, sconv_kernel and sconv6_kernel of
csrc/strict_conv.hip (fp32 storage).  tests/test_gemm_exact_cases_cpu.py holds this table without a GPU (condition EXACT per element,
the dispatch of every row, geometry and rounding mutants); tests/test_gpu_gemm_exact.py runs the rows.

Condition EXACT: all products of one output are multiples of a granule g and sum_k |x_k w_k| + |bias| + |residual| <= 2^24 g.  Every
partial sum is then an fp32 value in ANY order, with or without FMA, so a correct kernel returns ONE documented rounding of the fp64
reference post(act(x . W + b) + r): (f16)v on the fp16 storage, hi = rn16(v), lo = rn16(v - hi) on the packed storage (h2_store8),
v itself on the fp32 storage.  bound() computes the left side per output element in fp64; the CPU test asserts it for every row.

Operand kinds (no operand plane holds an fp16 subnormal):
  f16 "a"     x integers in [-2, 2], W multiples of 1/4 in [-1, 1] (diffuse_round_f16 leaves them alone), bias multiples of 1/4 in
              [-2, 2], residual integers in [-8, 8]; g = 1/4.  CARRIER channels make a premature rounding visible: the last input
              channel of every group is 1 at every pixel, its weight is 2048 into every fourth output channel at ONE tap (the centre tap
              of an odd filter, else tap (0, 0)) and 0 elsewhere, and in residual epilogues the residual of those output channels is
              -2048 where that tap lies inside the image.  The accumulator 2048 + s is no fp16 value; the result is the small s + b
              (residual epilogues) or one rounding of 2048 + s + b.
  f16 gated   the split input gate [B, 2, K]: hi = 2^-((2 image + 2 channel) % 3), one of {1, 1/2, 1/4}; by (image + 2 channel) % 3 the
              gate is hi alone, lo alone (hi = 0) or hi + hi / 32 on both planes; fma(x, hi, x * lo) stays an fp16 value; g = 2^-9;
              the carrier channel has the gate (1, 0).
              Neighbouring images never share a gate.  (An input gate keeps a launch on pwk_direct_kernel at any M and K; the gated
              modes of pw_gemm_kernel are the OUTPUT-gated ones, which tests/_out_gate_cases.py holds exactly.)
  f16 hilo    two-term weights W = i/4 + j 2^-13 (j != 0 only where |i| >= 2, so w_lo alone carries j); g = 2^-13.  NO carriers: 2048 + s
              would need 25 bits.  The sums themselves are no fp16 values, which is what the carriers are for.
  h2 "a"      x and W hi-only, as on fp16, no carriers (split_h2_weights scales the largest |W| into [4096, 8192): one |W| = 1 per matrix
              keeps the scale at 2^12, a weight of 2048 would not)
  h2 "b"      x = i + j 2^-13 (j != 0 only where i != 0: the lo plane is live), W multiples of 1/2 (g = 2^-14: with multiples of 1/4 the
              output's lo plane would hold fp16 subnormals); W is thinned to about 160 non-zero k per output so that EXACT holds
  h2 "c"      x hi-only, W 2^12 = 4 q + r, |q| in 512 ... 1024, r in {-1, 0, 1}: hi = 4 q, lo = r; g = 2^-12
  s32 "a"     as f16 "a" without carriers; torch.equal on the fp32 result (sconv_kernel and sconv6_kernel)
  s32 "p2"    sconv6_kernel only: W = i/4 + j 2^-10, two live bf16 planes; g = 2^-10
Between kinds a, b, c each of the three MFMAs of a packed fragment pair (w_lo x_hi, w_hi x_hi, w_hi x_lo) is the sole carrier of
some bits.  GELU / SiLU / sigmoid epilogues are not part of this table.

Not reached: pwx_kernel and pwx_ln_kernel (VIP_PWX=1 / LayerNorm sites: default dispatch does not reach pwx_kernel), the fused MLP and
SE-gate kernels, the output-gated modes (tests/_out_gate_cases.py holds them), every kernel behind an environment switch
(VIP_PWK_CONV, VIP_G8P_MINK, VIP_PW, ...), the bf16x2 arithmetic of the fp32 storage, gated rows of the strict storages."""
import zlib
from collections import namedtuple

import torch
import torch.nn.functional as Fn

from oracle import ops_ref as R
from tests import _f16_gemm_cases as F16
from tests import _h2_gemm_cases as H2

# epilogue family -> (act, act_post, residual) of ops.dense / ops.conv2d
EPI = {"none": (None, None, False), "relu": ("relu", None, False), "res": (None, None, True), "res_relu": (None, "relu", True),
       "relu_res": ("relu", None, True)}
POINTWISE = ("none", "relu", "res", "res_relu")       # what pw_epilogue<> carries; relu_res is conv_igemm_kernel's epilogue<>
MODE = {"f16": "fast", "h2": "strict", "s32": "f32"}
SENTINEL = 977.0
CARRIER = 2048.0

# case = (B, H, W, Cin, Cout, k, stride, pad(t,b,l,r), groups); slice = None or (name, ld, off)
Row = namedtuple("Row", "id storage kind kernel variant case epi gated hilo slice what")


def dense_case(M, K, N):
    return (M, 1, 1, K, N, 1, 1, (0, 0, 0, 0), 1)


def is_dense(row):
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    return (H, W, k, s, groups) == (1, 1, 1, 1, 1) and not row.gated and not row.hilo and row.slice is None


def out_hw(case):
    B, H, W, Cin, Cout, k, s, pad, groups = case
    return (H + pad[0] + pad[1] - k) // s + 1, (W + pad[2] + pad[3] - k) // s + 1


# ---- (1) rows by instantiation ------------------------------------------------------------------------------------------------------------
# pw_gemm<KS=1..6> are reached by tests/test_gpu_ops.py's PW_CASES, not by the table: their K and N, 37 rows past the M = 65 536 switch
_PW_ROWS = [(65573, 24, 144, "pw_gemm<KS=1> 1 x 192"), (65573, 64, 256, "pw_gemm<KS=2> 1 x 256"), (65573, 96, 384, "pw_gemm<KS=3> 2 x 192"),
            (65573, 128, 56, "pw_gemm<KS=4> 1 x 64"), (65573, 160, 960, "pw_gemm<KS=6> 8 x 128")]
# rows_gemm_kernel carries an activation, no residual; one row of 104 channels: 26 carrier channels, so that every mutant has elements to show in
_ROWS_GEMM = [(1, 72, 104), (37, 264, 72), (256, 2048, 512)]
_GATED_PT1 = [(4, 9, 9, 200, 72, "pwk_direct<2,gated> PT=1"), (2, 57, 56, 144, 32, "pwk_direct<1,gated> PT=1")]   # test_gpu_ops.GATED_CASES
_HILO = [(4, 56, 56, 32, 192, "pw_gemm<KS=1,hilo> 1 x 192"), (3, 28, 28, 160, 40, "pw_gemm<KS=6,hilo> 1 x 64"),
         (2, 24, 24, 256, 72, "pw_gemm<KS=8,hilo> 2 x 64")]                                                        # test_conv2d_two_term_weights


def _fan_out(table, storage):
    """a table's rows with the four pointwise families on the first row of each instantiation (and where the table has them all)"""
    out, full = [], set()
    for i, (M, K, N, epis, kernel, variant, what) in enumerate(table):
        inst = F16.instantiation(variant)
        epis_ = POINTWISE if (len(epis) > 1 or inst not in full) else ("none",)
        full.add(inst)
        for j, epi in enumerate(epis_):
            kinds = ("a",) if storage == "f16" else (("a", "b", "c") if (epi == "none" and len(epis_) > 1) else ("abc"[(i + j) % 3],))
            for kind in kinds:
                out.append(Row(f"{storage}-{kind}-{M}x{K}x{N}-{epi}", storage, kind, kernel, variant, dense_case(M, K, N), epi, False, False,
                               None, what))
    return out


def _inst_rows():
    out = _fan_out(F16._DENSE_ROWS, "f16")
    for M, K, N, variant in _PW_ROWS:
        for epi in POINTWISE:
            out.append(Row(f"f16-a-{M}x{K}x{N}-{epi}", "f16", "a", "pw_gemm_kernel", variant, dense_case(M, K, N), epi, False, False, None,
                           "a k-step template the table leaves to PW_CASES"))
    for M, K, N in _ROWS_GEMM:
        for epi in ("none", "relu"):
            out.append(Row(f"f16-a-{M}x{K}x{N}-{epi}", "f16", "a", "rows_gemm_kernel", "rows_gemm", dense_case(M, K, N), epi, False, False,
                           None, "at most 256 rows"))
    out.append(Row("f16-a-1000x256x768-relu_res", "f16", "a", "conv_igemm_kernel", "conv_igemm<64,128>", dense_case(1000, 256, 768),
                   "relu_res", False, False, None, "an activation AND a residual on a Dense: the tile kernel's <64,128>"))
    gated = [(B, 7, 7, K, N, v) for B, K, N, _, v, _ in F16._GATED_ROWS] + _GATED_PT1
    for B, H, W, K, N, variant in gated:
        for epi in ("none", "res"):
            out.append(Row(f"f16-gated-{B}x{H}x{W}x{K}-{N}-{epi}", "f16", "gated", "pwk_direct_kernel", variant,
                           (B, H, W, K, N, 1, 1, (0, 0, 0, 0), 1), epi, True, False, None, "split input gate"))
    for B, H, W, K, N, variant in _HILO:
        for epi in ("none", "res"):
            out.append(Row(f"f16-hilo-{B}x{H}x{W}x{K}-{N}-{epi}", "f16", "hilo", "pw_gemm_kernel", variant,
                           (B, H, W, K, N, 1, 1, (0, 0, 0, 0), 1), epi, False, True, None, "two-term weights"))
    out += _fan_out(H2._DENSE_ROWS, "h2")
    for (M, K, N), kind in zip(_ROWS_GEMM, "abc"):
        out.append(Row(f"h2-{kind}-{M}x{K}x{N}-none", "h2", kind, "rows_gemm_kernel", "rows_gemm", dense_case(M, K, N), "none", False, False,
                       None, "at most 256 rows"))
    return out


# ---- (2) convolution geometry -----------------------------------------------------------------------------------------------------------------
# tests/test_gpu_ops.py's CONV_CASES as (geometry, activation?, residual?) - the list is restated so that importing this module does not
# import a GPU test; the CPU test asserts that it is the same list
CONV_GEOMS = [
    ((2, 9, 9, 8, 32, 3, 2, (1, 1, 1, 1), 1), True, False), ((2, 12, 10, 32, 64, 3, 1, (1, 1, 1, 1), 1), True, False),
    ((3, 7, 7, 64, 256, 1, 1, (0, 0, 0, 0), 1), False, True), ((2, 13, 13, 128, 128, 3, 2, (1, 1, 1, 1), 1), True, False),
    ((1, 20, 20, 24, 40, 3, 1, (1, 1, 1, 1), 1), True, False), ((2, 8, 8, 128, 128, 3, 1, (1, 1, 1, 1), 2), True, False),
    ((2, 10, 10, 16, 200, 4, 2, (0, 0, 0, 0), 1), False, False), ((2, 6, 6, 512, 72, 1, 1, (0, 0, 0, 0), 1), True, False),
    ((1, 33, 31, 64, 64, 3, 1, (1, 1, 1, 1), 1), True, True), ((2, 9, 9, 64, 64, 5, 1, (2, 2, 2, 2), 1), False, False),
    ((2, 9, 9, 96, 96, 2, 2, (0, 0, 0, 0), 1), False, False), ((2, 9, 9, 32, 32, 3, 2, (0, 1, 0, 1), 1), True, False),
]
EXTRA_GEOMS = [
    ((2, 9, 9, 32, 64, 3, 1, (0, 2, 2, 0), 1), False, True),     # shifted pad: all of the vertical pad below, all of the horizontal pad left
    ((2, 3, 4, 32, 64, 5, 1, (2, 2, 2, 2), 1), True, False),     # a map smaller than the filter: every window reaches all four borders
    ((2, 8, 8, 64, 80, 3, 1, (1, 1, 1, 1), 2), False, True),     # groups = 2 with Cout_g = 40, no multiple of 64
]
SLICE_GEOM = (2, 9, 7, 40, 72, 3, 1, (1, 1, 1, 1), 1)
SLICES = [("ldx", 64, 16, "relu"), ("ldy", 96, 16, "res"), ("ldr", 104, 24, "res_relu")]

# the dispatcher's answer per geometry and epilogue class (plain = none / relu / res / res_relu agree unless listed), fp16 then packed.
# A change of plan()'s rules fails the CPU test: re-derive this table then, never the rows.
_IG = "conv_igemm_kernel"
_IM = "pwk_gemm_kernel(im2col)"
GEO_KERNELS = {
    # geometry: ((f16 plain, f16 relu_res), (h2 plain, h2 relu_res))
    CONV_GEOMS[0][0]: (((_IM, "im2col<1>"), (_IG, "conv_igemm<64,64>")),) * 2,
    CONV_GEOMS[1][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    CONV_GEOMS[2][0]: (((None, None), (_IG, "conv_igemm<64,128>")),) * 2,         # plain: by epilogue, see _POINT_1x1
    CONV_GEOMS[3][0]: (((_IG, "conv_igemm<128,128>"),) * 2,) * 2,
    CONV_GEOMS[4][0]: (((_IG, "conv_igemm<64,64>"),) * 2, ((_IG, "conv_igemm<128,64>"),) * 2),
    CONV_GEOMS[5][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    CONV_GEOMS[6][0]: (((_IM, "im2col<2>"), (_IG, "conv_igemm<64,128>")), ((_IM, "im2col<2>"), (_IG, "conv_igemm<128,128>"))),
    CONV_GEOMS[7][0]: (((None, None), (_IG, "conv_igemm<128,128>")),) * 2,
    CONV_GEOMS[8][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    CONV_GEOMS[9][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    CONV_GEOMS[10][0]: (((_IG, "conv_igemm<128,128>"),) * 2,) * 2,
    CONV_GEOMS[11][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    EXTRA_GEOMS[0][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    EXTRA_GEOMS[1][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    EXTRA_GEOMS[2][0]: (((_IG, "conv_igemm<128,64>"),) * 2,) * 2,
    SLICE_GEOM: (((_IG, "conv_igemm<128,128>"),) * 2,) * 2,
}
# the two 1 x 1 geometries of CONV_CASES are Dense layers: few rows without a residual, a pointwise kernel with one
_POINT_1x1 = {
    (CONV_GEOMS[2][0], "f16", False): ("rows_gemm_kernel", "rows_gemm"), (CONV_GEOMS[2][0], "f16", True): ("pwk_direct_kernel", "pwk_direct<2> PT=1"),
    (CONV_GEOMS[2][0], "h2", False): ("rows_gemm_kernel", "rows_gemm"), (CONV_GEOMS[2][0], "h2", True): ("pwk_direct_kernel", "pwk_direct<2> PT=1"),
    (CONV_GEOMS[7][0], "f16", False): ("rows_gemm_kernel", "rows_gemm"), (CONV_GEOMS[7][0], "f16", True): ("pwk_direct_kernel", "pwk_direct<2> PT=1"),
    (CONV_GEOMS[7][0], "h2", False): ("rows_gemm_kernel", "rows_gemm"), (CONV_GEOMS[7][0], "h2", True): ("pwk_gemm_kernel", "pwk_gemm<2,1> 1 x 1"),
}


def geo_kernel(geom, storage, epi):
    if storage == "s32":
        return None, None
    plain, both = GEO_KERNELS[geom][0 if storage == "f16" else 1]
    if epi == "relu_res":
        return both
    return plain if plain[0] else _POINT_1x1[(geom, storage, EPI[epi][2])]


def _geo_id(geom):
    return "x".join(str(v) for v in geom[:7]) + "p" + "".join(str(v) for v in geom[7]) + f"g{geom[8]}"


def _geo_rows():
    out = []

    def add(storage, kind, geom, epi, kernel, variant, what, sl=None):
        tag = f"-{sl[0]}" if sl else ""
        out.append(Row(f"{storage}-{kind}-{_geo_id(geom)}-{epi}{tag}", storage, kind, kernel, variant, geom, epi, False, False, sl, what))

    def small(geom, act, res):
        """the geometry's own epilogue class without a transcendental, then the tile kernel's activation + residual"""
        return ("res" if res else "relu" if act else "none"), "relu_res"

    for geom, act, res in CONV_GEOMS + EXTRA_GEOMS:
        for epi in small(geom, act, res):
            add("f16", "a", geom, epi, *geo_kernel(geom, "f16", epi), "CONV_CASES geometry" if (geom, act, res) in CONV_GEOMS else "extra geometry")
            add("h2", "abc"[len(out) % 3], geom, epi, *geo_kernel(geom, "h2", epi), "geometry, packed")
            add("s32", "p2", geom, epi, "sconv6_kernel", "bf16x3", "geometry, fp32 storage, three bf16 planes")
            add("s32", "a", geom, epi, "sconv_kernel", "f32", "geometry, fp32 storage, f32-input MFMA")
        add("s32", "a", geom, "none" if res else "res", "sconv6_kernel", "bf16x3", "geometry, fp32 storage, hi-only operands")
    for (case, kernel, variant, what) in F16.CONV_F16_CASES:
        epi = "relu_res" if (case[9] and case[10]) else "res" if case[10] else "relu" if case[9] else "none"
        add("f16", "a", case[:9], epi, kernel, variant, what)
    for i, (case, kernel, variant, what) in enumerate(H2.CONV_H2_CASES):
        epi = "res" if case[10] else "relu" if case[9] else "none"
        add("h2", "abc"[i % 3], case[:9], epi, kernel, variant, what)
    # ---- (3) slices: the entry points themselves, 977 in every output element before the launch
    for name, ld, off, epi in SLICES:
        sl = (name, ld, off)
        add("f16", "a", SLICE_GEOM, epi, *geo_kernel(SLICE_GEOM, "f16", epi), f"{name} = {ld}, offset {off}", sl)
        add("h2", "c", SLICE_GEOM, epi, *geo_kernel(SLICE_GEOM, "h2", epi), f"{name} = {ld}, offset {off}", sl)
        add("s32", "p2", SLICE_GEOM, epi, "sconv6_kernel", "bf16x3", f"{name} = {ld}, offset {off}", sl)
    return out


INST_ROWS = _inst_rows()
GEO_ROWS = _geo_rows()
ROWS = INST_ROWS + GEO_ROWS
IDS = [r.id for r in ROWS]
assert len(set(IDS)) == len(IDS), sorted(i for i in IDS if IDS.count(i) > 1)
# the instantiations of the packed build the table of tests/_h2_gemm_cases.py names (it keeps no set of its own)
H2_INSTANTIATIONS = {F16.instantiation(r[5]) for r in H2._DENSE_ROWS} | {c[2] for c in H2.CONV_H2_CASES} | {"rows_gemm"}


# ---- operands -------------------------------------------------------------------------------------------------------------------------------
def carrier_tap(k):
    return (k // 2, k // 2) if k % 2 else (0, 0)


def has_carriers(row):
    return row.storage == "f16" and row.kind in ("a", "gated")


def tap_validity(case):
    """[Ho, Wo] 1.0 where the carrier tap of the output pixel lies inside the image"""
    B, H, W, Cin, Cout, k, s, pad, groups = case
    Ho, Wo = out_hw(case)
    tr, tc = carrier_tap(k)
    ih = torch.arange(Ho) * s - pad[0] + tr
    iw = torch.arange(Wo) * s - pad[2] + tc
    return (((ih >= 0) & (ih < H))[:, None] & ((iw >= 0) & (iw < W))[None, :]).double()


def granule(row):
    return {("f16", "a"): 2.0 ** -2, ("f16", "gated"): 2.0 ** -9, ("f16", "hilo"): 2.0 ** -13, ("h2", "a"): 2.0 ** -2, ("h2", "b"): 2.0 ** -14,
            ("h2", "c"): 2.0 ** -12, ("s32", "a"): 2.0 ** -2, ("s32", "p2"): 2.0 ** -10}[(row.storage, row.kind)]


_cache = {}


def operands(row):
    """fp64 host tensors of the row's shape, seeded by (storage, kind, case): dict x [B,H,W,Cin], w [k,k,Cin_g,Cout] (HWIO), b [Cout],
    r [B,Ho,Wo,Cout] (the residual of a residual epilogue), gate [B,2,Cin] or None, y = conv(x * gate, w) + b.  The last three shapes
    are kept: the epilogue cases of a shape are neighbouring rows.  Nothing here is written to afterwards (bound() adds its sum)."""
    key = (row.storage, row.kind, row.case)
    if key in _cache:
        return _cache[key]
    while len(_cache) >= 3:
        del _cache[next(iter(_cache))]
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    cin_g, cout_g = Cin // groups, Cout // groups
    Ho, Wo = out_hw(row.case)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).double()
    x = ints(-2, 2, B, H, W, Cin)
    w = ints(-4, 4, k, k, cin_g, Cout) / 4
    b = ints(-8, 8, Cout) / 4
    r = ints(-8, 8, B, Ho, Wo, Cout)
    gate = None
    kind = row.kind
    if kind == "hilo":
        j = ints(-1, 1, k, k, cin_g, Cout)
        w = w + torch.where(w.abs() >= 0.5, j, torch.zeros_like(j)) * 2.0 ** -13
    elif kind == "p2":
        w = w + ints(-1, 1, k, k, cin_g, Cout) * 2.0 ** -10
    elif kind == "b":
        j = ints(-1, 1, B, H, W, Cin)
        x = x + torch.where(x != 0, j, torch.zeros_like(j)) * 2.0 ** -13
        keep = torch.rand(k, k, cin_g, Cout, generator=g) < min(1.0, 160.0 / (k * k * cin_g))
        w = torch.where(keep, ints(-2, 2, k, k, cin_g, Cout) / 2, torch.zeros_like(w))
    elif kind == "c":
        q = ints(512, 1024, k, k, cin_g, Cout) * (ints(0, 1, k, k, cin_g, Cout) * 2 - 1)
        w = (4 * q + ints(-1, 1, k, k, cin_g, Cout)).clamp(-4096, 4096) / 4096
    if row.storage == "h2":
        w[0, 0, 0, 0] = 1.0                                  # the weights' scale is then 2^12 for every kind
    if has_carriers(row):
        tr, tc = carrier_tap(k)
        x[..., cin_g - 1::cin_g] = 1.0
        w[:, :, cin_g - 1, :] = 0.0
        car = (torch.arange(Cout) % cout_g) % 4 == 0
        w[tr, tc, cin_g - 1, car] = CARRIER
        r[..., car] = -CARRIER * tap_validity(row.case)[None, :, :, None]
    xe = x
    if kind == "gated":
        bi, ci = torch.arange(B)[:, None], torch.arange(Cin)[None, :]
        hi = torch.pow(2.0, -((bi * 2 + ci * 2) % 3).double())
        form = (bi + ci * 2) % 3
        gate = torch.stack([torch.where(form == 1, torch.zeros_like(hi), hi),
                            torch.where(form == 1, hi, torch.where(form == 2, hi / 32, torch.zeros_like(hi)))], 1)
        gate[:, 0, Cin - 1], gate[:, 1, Cin - 1] = 1.0, 0.0
        xe = x * (gate[:, 0] + gate[:, 1])[:, None, None, :]
    op = dict(x=x, w=w, b=b, r=r, gate=gate, xe=xe, y=conv64(xe, w, b, row.case))
    _cache[key] = op
    return op


def conv64(x, w, b, case):
    """fp64 x . W + b: `@` for Dense rows, the oracle's conv2d on double tensors otherwise"""
    B, H, W, Cin, Cout, k, s, pad, groups = case
    if (k, s, groups) == (1, 1, 1) and pad == (0, 0, 0, 0):
        y = (x.reshape(-1, Cin) @ w[0, 0]).reshape(B, H, W, Cout)
        return y if b is None else y + b
    return R.conv2d(x, w, b, s, pad, groups)


def bound(row, op):
    """sum_k |x_k w_k| + |bias| + |residual| per output element, fp64 (the residual only where the epilogue has one); the sum is kept
    with the operands, for the other epilogue cases of the shape"""
    if "abs" not in op:
        op["abs"] = conv64(op["xe"].abs(), op["w"].abs(), op["b"].abs(), row.case)
    return op["abs"] + op["r"].abs() if EPI[row.epi][2] else op["abs"]


def epilogue64(y, r, epi):
    act, post, res = EPI[epi]
    v = R.act(y, act)
    if res:
        v = v + r
    return R.act(v, post)


def ref64(row, op):
    """post(act(x . W + b) + r) on double tensors"""
    return epilogue64(op["y"], op["r"], row.epi)


def rn16(v):
    return v.to(torch.float16).double()


def split16(v):
    """the packed storage's documented split of an exact value: hi = rn16(v), lo = rn16(v - hi)"""
    hi = rn16(v)
    return hi, rn16(v - hi)


def expected(row, v):
    """the ONE documented rounding of the storage: (f16)v -> fp16 tensor; (hi, lo) planes as fp64; v as fp32"""
    if row.storage == "f16":
        return v.to(torch.float16)
    if row.storage == "h2":
        return split16(v)
    return v.to(torch.float32)


def planes_of_packed(t):
    """a packed int32 tensor [..., C] (host) -> its (hi, lo) planes as fp64 [..., C]: 8 channels = [hi x 8][lo x 8] halfs"""
    h = t.contiguous().view(torch.float16).reshape(*t.shape[:-1], t.shape[-1] // 8, 2, 8).double()
    return h[..., 0, :].reshape(t.shape), h[..., 1, :].reshape(t.shape)


# ---- geometry mutants of the reference: (name, applies(case), y(op, case)) ---------------------------------------------------------------
def _m_transposed(op, case):
    return conv64(op["xe"], op["w"].transpose(0, 1), op["b"], case)


def _m_pads_swapped(op, case):
    p = case[7]
    return conv64(op["xe"], op["w"], op["b"], case[:7] + ((p[1], p[0], p[3], p[2]),) + case[8:])


def _m_clamp(op, case):
    B, H, W, Cin, Cout, k, s, pad, groups = case
    xp = Fn.pad(op["xe"].permute(0, 3, 1, 2), (pad[2], pad[3], pad[0], pad[1]), mode="replicate").permute(0, 2, 3, 1)
    return R.conv2d(xp, op["w"], op["b"], s, (0, 0, 0, 0), groups)


def _m_origin(op, case):
    B, H, W, Cin, Cout, k, s, pad, groups = case
    xp = Fn.pad(op["xe"].permute(0, 3, 1, 2), (pad[2] + 1, pad[3] - 1, pad[0] + 1, pad[1] - 1)).permute(0, 2, 3, 1)
    return R.conv2d(xp, op["w"], op["b"], s, (0, 0, 0, 0), groups)


def _m_groups(op, case):
    return conv64(op["xe"], op["w"].roll(case[4] // case[8], 3), op["b"], case)


def _m_last_col(op, case):
    y = op["y"].clone()
    y[:, :, -1, :] = 0.0
    return y


def reads_padding(c):
    """does any window reach outside the image?  (TF SAME (0,1,0,1) on an odd map at stride 2 pads a row and a column that no window reads)"""
    B, H, W, Cin, Cout, k, s, pad, groups = c
    Ho, Wo = out_hw(c)
    return pad[0] > 0 or pad[2] > 0 or (Ho - 1) * s + k - pad[0] > H or (Wo - 1) * s + k - pad[2] > W


GEOMETRY_MUTANTS = [
    ("transposed taps", lambda c: c[5] > 1, _m_transposed),
    ("top / bottom and left / right pads swapped", lambda c: c[7][0] != c[7][1] or c[7][2] != c[7][3], _m_pads_swapped),
    ("clamp instead of zero padding", reads_padding, _m_clamp),
    ("window origin off by one at stride 2", lambda c: c[6] == 2, _m_origin),
    ("group order swapped", lambda c: c[8] > 1, _m_groups),
    ("last output column dropped", lambda c: True, _m_last_col),
]


# ---- CPU emulation of the kernels' rounding points ---------------------------------------------------------------------------------------
def im2col(x, case, rows=None):
    """[M', groups, k k Cin_g] in the kernels' K order (tap-major, channel innermost) of the first `rows` output pixels"""
    B, H, W, Cin, Cout, k, s, pad, groups = case
    Ho, Wo = out_hw(case)
    nb = B if rows is None else min(B, -(-rows // (Ho * Wo)))
    xp = Fn.pad(x[:nb].permute(0, 3, 1, 2), (pad[2], pad[3], pad[0], pad[1]))
    cols = Fn.unfold(xp, k, stride=s).reshape(nb, groups, Cin // groups, k * k, Ho * Wo)
    return cols.permute(0, 4, 1, 3, 2).reshape(nb * Ho * Wo, groups, k * k * (Cin // groups))


def emulate_f16(row, op, mutant=None, rows=2048, operands_=None):
    """csrc/conv_igemm.hip's fp16 rounding points on the first `rows` output pixels: fp32 accumulators over 64-k chunks (exact here, so
    fp64 holds them), + fp32 bias, activation, + residual in fp32, post, ONE (f16) cast (epilogue<> / pw_epilogue<>).  mutant:
      "M1" the accumulator rounded to fp16 before the residual add      "M2" the bias added after that rounding, in fp16
      "M3" fp16 partial sums between the 64-k chunks                     "M4" the input gate's lo plane dropped
      "M5" w_lo dropped                                                  "M6" the last 8 k of a K tail read as zero
    -> fp16 [M', Cout]"""
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    x, w, b, r = op["x"], op["w"], op["b"], op["r"]
    if row.gated:
        gt = op["gate"]
        scale = gt[:, 0] if mutant == "M4" else gt[:, 0] + gt[:, 1]
        x = rn16(x * scale[:, None, None, :])            # fma(x, hi, x * lo) in fp16: exact on these operands
    if row.hilo and mutant == "M5":
        w = rn16(w)
    A = im2col(x, row.case, rows)
    Mp, K = A.shape[0], A.shape[2]
    if mutant == "M6":
        A = A.clone()
        A[:, :, K - 8:] = 0.0
    cout_g = Cout // groups
    acc = torch.zeros(Mp, Cout, dtype=torch.float64)
    for gi in range(groups):
        wg = w[..., gi * cout_g:(gi + 1) * cout_g].reshape(K, cout_g)
        a = acc[:, gi * cout_g:(gi + 1) * cout_g]
        for c0 in range(0, K, 64):
            a += A[:, gi, c0:c0 + 64] @ wg[c0:c0 + 64]
            if mutant == "M3":
                a.copy_(rn16(a))
    if mutant == "M2":
        acc = rn16(rn16(acc) + b)
    else:
        acc = acc + b
    if mutant == "M1":
        acc = rn16(acc)
    return epilogue64(acc, r.reshape(-1, Cout)[:Mp], row.epi).to(torch.float16)


def mutant_applies(row, m):
    K = row.case[5] ** 2 * row.case[3] // row.case[8]
    return {"M1": EPI[row.epi][2], "M2": True, "M3": True, "M4": row.gated, "M5": row.hilo, "M6": K % 64 != 0}[m]


def emulate_h2(row, op, mutant=None, rows=1024):
    """the packed build's arithmetic on the first `rows` pixels: the (hi, lo) planes of x and of W 2^12, three products per fragment pair,
    the scale undone, + bias, activation, + residual, post, the split of h2_store8.  mutant: "M7a" / "M7b" / "M7c" drop w_lo x_hi /
    w_hi x_hi / w_hi x_lo; "M8" takes the output's lo plane from the rounded sum (rn16(rn16(v) - hi) = 0) -> (hi, lo) fp64 [M', Cout]"""
    B, H, W, Cin, Cout, k, s, pad, groups = row.case
    xh, xl = split16(op["x"])
    wh, wl = split16(op["w"] * 4096.0)
    Ah, Al = im2col(xh, row.case, rows), im2col(xl, row.case, rows)
    Mp, K = Ah.shape[0], Ah.shape[2]
    cout_g = Cout // groups
    acc = torch.zeros(Mp, Cout, dtype=torch.float64)
    for gi in range(groups):
        sl = slice(gi * cout_g, (gi + 1) * cout_g)
        h_, l_ = wh[..., sl].reshape(K, cout_g), wl[..., sl].reshape(K, cout_g)
        terms = {"M7a": Ah[:, gi] @ l_, "M7b": Ah[:, gi] @ h_, "M7c": Al[:, gi] @ h_}
        acc[:, sl] = sum(t for name, t in terms.items() if name != mutant)
    v = epilogue64(acc / 4096.0 + op["b"], op["r"].reshape(-1, Cout)[:Mp], row.epi)
    hi, lo = split16(v)
    return (hi, torch.zeros_like(lo)) if mutant == "M8" else (hi, lo)


def h2_mutant_applies(row, m):
    return {"M7a": row.kind == "c", "M7b": True, "M7c": row.kind == "b", "M8": row.kind in ("b", "c")}[m]
