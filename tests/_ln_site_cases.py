"""The four kernels that compute a LayerNorm in their own prologue instead of calling layernorm_kernel - mlp_fused_kernel and
mlp_stream_kernel (csrc/mlp_fused.hip, ln_fragments of csrc/frag.hpp), mlp_h2_kernel (csrc/mlp_h2.hip, ln_fragments_h2) and pwx_ln_kernel
(csrc/conv_igemm.hip, behind ops.ln_dense: its own statistics code with masked K-tail channels) - on STRUCTURED rows, against an fp64
reference, with the error taken PER ROW.  The inputs every other test of these kernels draws (x ~ 1.5 randn + 0.3, i.i.d. over rows, one
eps per storage, max|err| / max|ref| over the whole tensor) cannot tell a one-pass variance, a dropped eps or a fixed eps from the correct
kernel (tests/test_ln_site_cases_cpu.py holds the witness); these rows can.

Rows: row r of an [M, C] input has kind r % 7 - seven is coprime with the 16-token MFMA tile, so every kind lands on every lane position
and next to every other kind:
  0  64 randn + 96                         a loud row next to quiet ones
  1  randn - 1.5                           2^-6 of its neighbour's scale, negative mean
  2  zeros with one 8.0 at channel 7r % C  statistics carried by one lane
  3  fp16: 0.25 randn + 100; packed: 0.25 randn + 16 on the fp16 grid (lo plane zero)      cancellation in the variance
  4  the constant (5r) % 9 - 4             variance 0: the normalised row is exactly beta
  5  2^-6 randn                            a quiet row
  6  2^-10 randn                           variance ~ 1e-6 ~ eps
(kind 3 differs by storage: plain fp32 arithmetic on h2_quantise(0.25 randn + 100) is already 3.9e-5 .. 7.0e-5 per row away from fp64,
above TOL_OP, before any kernel is involved; mean 16 on the fp16 grid is at most 3.3e-6.)  MILDER records what a case had to soften:
nothing.

gamma on the quarter grid in [0.5, 2], beta on the quarter grid in [-2, 2] (as tests/_helper_cases.py), weights randn / sqrt(K) (fp16-
rounded for the fp16 storage), biases 0.1 randn in fp32, the residual an INDEPENDENT randn - a loud x as the residual would hide the
MLP's error behind itself.  All draws come from a CPU generator seeded by the case's shape, so the cases of one shape (eps, residual,
mode) share their operands.

forward(case, o, ...) is the one statement of the arithmetic: in float64 without roundings it is the reference (reference()), through
oracle/ops_ref.py's dtype-generic functions; tests/test_ln_site_cases_cpu.py runs it in float32 with the kernels' documented rounding
points as the emulation, and with wrong=<one of WRONG> as the classic mistakes the rows must tell apart.  tests/test_gpu_ln_sites.py
runs the cases."""
import functools
import zlib
from collections import namedtuple

import torch

from oracle import ops_ref as R
from tests._helper_cases import h2_quantise

Case = namedtuple("Case", "id site storage route kernel C N M eps res mode tile tol what")

KINDS = 7
KIND_NAMES = ("loud 64 randn + 96", "randn - 1.5", "one 8.0 in a zero row", "mean 100 (packed: 16), spread 0.25", "constant", "2^-6 randn",
              "2^-10 randn")
EPS = (1e-6, 1e-5)
M_MLP = 8192 + 37            # vip_mlp_fused_supported(_h2): M >= 8192; 16 tiles of 512 tokens and 37 rows
M_LN = 16384 + 37            # vip_ln_gemm_supported: M >= 16384
M_SMALL = 37                 # below both: ops.mlp answers with LayerNorm + two Dense launches
MOVE_TILE = 512              # the largest tile of the four kernels (mlp_fused_kernel: 512 tokens): a row that leaves its 512-row tile leaves
                             # its 256-, 128- and 16-row tile too
TOLERANCES = {"TOL_MLP_F16": 4e-3, "TOL_OP": 2e-5}      # tests/test_gpu_passes.py; 4e-3 is also test_gpu_ln_gemm.py's literal
MILDER = {}                  # case id -> (kind, what was softened): no case needed it

MLP_F16 = ((64, 256), (96, 384), (192, 768), (192, 96))
MLP_H2 = ((64, 256), (96, 384), (128, 384))
LN_DENSE = ((72, 256), (128, 256), (136, 256), (200, 1024), (256, 512), (320, 384), (384, 1152))
LN_MODES = ("none", "gelu", "res")
# (site, kernel) pairs the table must hold
KERNELS = (("mlp", "mlp_fused_kernel"), ("mlp", "mlp_stream_kernel"), ("mlp", "h2:mlp_h2_kernel"), ("ln_dense", "pwx_ln_kernel"),
           ("mlp", None))


def _e(eps):
    return "eps1e-6" if eps == 1e-6 else "eps1e-5"


def _mlp_cases():
    out = []
    for eps in EPS:
        for res in (False, True):
            tag = f"{_e(eps)}-{'res' if res else 'nores'}"
            for C, hid in MLP_F16:
                kern = "mlp_fused_kernel" if C <= 96 else "mlp_stream_kernel"
                out.append(Case(f"mlp-f16-c{C}-h{hid}-{tag}", "mlp", "f16", "fused", kern, C, hid, M_MLP, eps, res, "gelu", MOVE_TILE,
                                "TOL_MLP_F16", f"{kern}: ln_fragments<{C // 32}>, {hid // 32} hidden slices"))
            for C, hid in MLP_H2:
                out.append(Case(f"mlp-h2-c{C}-h{hid}-{tag}", "mlp", "h2", "fused", "h2:mlp_h2_kernel", C, hid, M_MLP, eps, res, "gelu",
                                MOVE_TILE, "TOL_OP", f"mlp_h2_kernel: ln_fragments_h2<{C // 32}>, {hid // 32} hidden slices"))
            # the answers ops.mlp gives without the fused kernels: the same rows, the same reference, the same tolerance
            for C, hid in ((96, 384), (192, 768)):
                out.append(Case(f"mlp-f16-c{C}-h{hid}-small-{tag}", "mlp", "f16", "small", None, C, hid, M_SMALL, eps, res, "gelu", 16,
                                "TOL_MLP_F16", "37 rows, below the fused kernels' 8192: layernorm + dense + dense"))
                out.append(Case(f"mlp-f16-c{C}-h{hid}-unfused-{tag}", "mlp", "f16", "unfused", None, C, hid, M_MLP, eps, res, "gelu",
                                MOVE_TILE, "TOL_MLP_F16", "inside ops.unfused(): layernorm + dense + dense"))
            out.append(Case(f"mlp-h2-c96-h384-unfused-{tag}", "mlp", "h2", "unfused", None, 96, 384, M_MLP, eps, res, "gelu", MOVE_TILE,
                            "TOL_OP", "inside ops.unfused(): the three launches of the packed storage"))
    return out


def ln_chunks(K):
    """64-channel chunks of pwx_ln_kernel's resident fragments, and the channels of the last one that are masked"""
    ksc = -(-K // 64)
    return ksc, 64 * ksc - K


def _ln_dense_cases():
    out = []
    for eps in EPS:
        for mode in LN_MODES:
            for K, N in LN_DENSE:
                ksc, masked = ln_chunks(K)
                out.append(Case(f"ln_dense-f16-k{K}-n{N}-{mode}-{_e(eps)}", "ln_dense", "f16", "fused", "pwx_ln_kernel", K, N, M_LN, eps,
                                mode == "res", mode, MOVE_TILE, "TOL_MLP_F16",
                                f"pwx_ln_kernel: {ksc} chunks of 64 channels, {masked} masked; {-(-N // 128)} channel tiles of 128"))
    return out


CASES = _mlp_cases() + _ln_dense_cases()
BY_ID = {c.id: c for c in CASES}
MLP_CASES = [c for c in CASES if c.site == "mlp"]
LN_DENSE_CASES = [c for c in CASES if c.site == "ln_dense"]

# ---- the classic mistakes ---------------------------------------------------------------------------------------------------------------
SHARED, PAD_DIV, PAD_SQ, ONE_PASS, NO_EPS, OTHER_EPS, NEIGHBOUR = (
    "statistics shared by rows r and r ^ 1",
    "variance divided by the padded channel count",
    "the padded channels' (0 - mean)^2 included in the variance",
    "one-pass variance E[x^2] - mean^2 in fp32",
    "eps dropped",
    "eps fixed at the other value",
    "gamma and beta of the neighbouring 8-channel group",
)
WRONG = (SHARED, PAD_DIV, PAD_SQ, ONE_PASS, NO_EPS, OTHER_EPS, NEIGHBOUR)


def padded(case):
    """the channel count the kernel's fragments cover: 64-channel chunks (pwx_ln_kernel), 32-channel MFMA steps (the MLP kernels)"""
    q = 64 if case.site == "ln_dense" else 32
    return -(-case.C // q) * q


def applies(case, wrong):
    return padded(case) != case.C if wrong in (PAD_DIV, PAD_SQ) else True


def _lane_sum(t):
    """the row sums of an fp32 [M, C] in the order the four prologues add: lane lq of a token holds channels 32 ks + 8 lq + 0..7 and adds
    them one after the other, then two lane exchanges (channels beyond C are zeros)"""
    M, C = t.shape
    t = torch.nn.functional.pad(t, (0, -C % 32)).reshape(M, -1, 4, 8)
    acc = torch.zeros(M, 4)
    for ks in range(t.shape[1]):
        for j in range(8):
            acc = acc + t[:, ks, :, j]
    return ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3]))[:, None]


def layernorm(x, gamma, beta, eps, wrong=None, pad=None):
    """oracle/ops_ref.py::layernorm in x's dtype; `wrong`: one of WRONG instead"""
    if wrong is None:
        return R.layernorm(x, gamma, beta, eps)
    n = x.shape[-1]
    m = x.mean(-1, keepdim=True)
    sq = ((x - m) ** 2).sum(-1, keepdim=True)
    if wrong == PAD_SQ:
        sq = sq + (pad - n) * m * m
    v = sq / (pad if wrong == PAD_DIV else n)
    if wrong == ONE_PASS:                                       # in fp32 whatever the dtype of the rest; a careful one: clamped at 0
        x32 = x.float()
        m32 = _lane_sum(x32) / n
        v = (_lane_sum(x32 * x32) / n - m32 * m32).clamp(min=0).to(x.dtype)
    if wrong == SHARED:
        idx = torch.arange(x.shape[0]) // 2 * 2                 # the even row's statistics serve the pair
        m, v = m[idx], v[idx]
    if wrong == NO_EPS:
        eps = 0.0
    if wrong == OTHER_EPS:
        eps = 1e-5 if eps == 1e-6 else 1e-6
    if wrong == NEIGHBOUR:
        gamma, beta = gamma.roll(-8), beta.roll(-8)
    return (x - m) / torch.sqrt(v + eps) * gamma + beta


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def structured_rows(g, M, C, storage):
    """[M, C] fp32 on the storage's grid, row r of kind r % 7"""
    r = torch.arange(M)
    kind = (r % KINDS)[:, None]
    z = torch.randn(M, C, generator=g)
    spike = torch.zeros(M, C)
    spike[r, (7 * r) % C] = 8.0
    const = ((5 * r) % 9 - 4).float()[:, None].expand(M, C)
    centre = 100.0 if storage == "f16" else 16.0
    x = torch.where(kind == 0, 64 * z + 96, torch.where(kind == 1, z - 1.5, torch.where(kind == 2, spike, torch.where(
        kind == 3, 0.25 * z + centre, torch.where(kind == 4, const, torch.where(kind == 5, z / 64, z / 1024))))))
    x16 = x.half().float()
    if storage == "f16":
        return x16
    return torch.where(kind == 3, x16, h2_quantise(x))          # kind 3: on the fp16 grid, the lo plane is zero


def _quarters(g, shape, lo, hi):
    return torch.randint(int(lo * 4), int(hi * 4) + 1, shape, generator=g).float() / 4


@functools.lru_cache(maxsize=16)
def _operands(site, storage, C, N, M):
    g = torch.Generator().manual_seed(zlib.crc32(f"{site}-{storage}-{C}-{N}-{M}".encode()))
    q = (lambda t: t.half().float()) if storage == "f16" else (lambda t: t)         # packed: the library quantises the fp32 weights
    o = dict(x=structured_rows(g, M, C, storage), gamma=_quarters(g, (C,), 0.5, 2), beta=_quarters(g, (C,), -2, 2),
             w1=q(torch.randn(C, N, generator=g) / C ** 0.5), b1=torch.randn(N, generator=g) * 0.1)
    if site == "mlp":
        o["w2"], o["b2"] = q(torch.randn(N, C, generator=g) / N ** 0.5), torch.randn(C, generator=g) * 0.1
    res = torch.randn(M, C if site == "mlp" else N, generator=g)
    o["res"] = res.half().float() if storage == "f16" else h2_quantise(res)
    return o


def operands(case):
    """the case's operands as fp32 host tensors, as the kernel is given them; shared by the cases of one shape - do not write to them.
    `res` is always there: a case without a residual does not pass it on"""
    return _operands(case.site, case.storage, case.C, case.N, case.M)


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def forward(case, o, wrong=None, dtype=torch.float64, q=None, qw=None):
    """fc2(gelu(fc1(LN(x)))) (+ residual) for ops.mlp, act(fc1(LN(x))) (+ residual) for ops.ln_dense, in `dtype`.  q: the rounding a
    kernel applies to the normalised row, the hidden activations and the output (None: none - the reference); qw: to the weights."""
    q = q or (lambda t: t)
    qw = qw or (lambda t: t)
    t = lambda name: o[name].to(dtype)  # noqa: E731
    xn = q(layernorm(t("x"), t("gamma"), t("beta"), case.eps, wrong, padded(case)))
    y = R.dense(xn, qw(t("w1")), t("b1"))
    if case.site == "mlp":
        y = R.dense(q(R.act(y, "gelu")), qw(t("w2")), t("b2"))
    elif case.mode == "gelu":
        y = R.act(y, "gelu")
    if case.res:
        y = y + t("res")
    return q(y)


def reference(case, o, wrong=None):
    """fp64, no rounding anywhere"""
    return forward(case, o, wrong)


# ---- the metric -------------------------------------------------------------------------------------------------------------------------
def tolerance(case):
    return TOLERANCES[case.tol]


def row_rel(got, ref):
    """|got - ref| / (max_c |ref[r, :]| + 1e-6) per element, as tests/_helper_cases.py::rel_error takes it for "row"; not finite: inf"""
    rel = (got.to(ref.dtype) - ref).abs() / (ref.abs().amax(-1, keepdim=True) + 1e-6)
    return torch.where(torch.isfinite(rel), rel, torch.full_like(rel, float("inf")))


def worst_by_kind(got, ref):
    """[(worst per-row error, row, channel)] for the seven kinds"""
    rel = row_rel(got, ref)
    per_row, ch = rel.max(-1)
    out = []
    for k in range(KINDS):
        i = int(per_row[k::KINDS].argmax())
        r = k + KINDS * i
        out.append((per_row[r].item(), r, int(ch[r])))
    return out


def move_rows(M, tile, seed=0):
    """a fixed permutation p of the M rows with p[i] // tile != i // tile for every i: the row at position i of the moved input comes from
    another tile (and so goes to another one), and lands among other neighbours"""
    assert M >= 2 * tile
    g = torch.Generator().manual_seed(1000003 * seed + M)
    within = torch.cat([t0 + torch.randperm(min(tile, M - t0), generator=g) for t0 in range(0, M, tile)])     # shuffles every tile in itself
    shift = min(tile + tile // 2 + 3, M - tile)                 # tile <= shift <= M - tile: position i draws from another tile, a
    return within[(torch.arange(M) + shift) % M]                # position's tile from two of them
