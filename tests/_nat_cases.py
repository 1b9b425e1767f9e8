"""ops.nat_attention (csrc/nat_attn.hip) on operands whose result is EXACT, and on random ones.

Reference: ref64(row) - tests/_nat_ref.core in float64, the layer as the reference writes it (zero-pad, K x K patches of the VALID
positions, replicate-pad, the bias gathered through the concatenated ramps and the reversal, crop).  folded(...) is an fp32 EMULATION of
the kernel's formula (block origin by a clamp, table index by the key-minus-query offset, keys outside the block masked) with switchable
MUTANTS; tests/test_nat_cases_cpu.py holds the two together and shows that each mutant moves some row by more than the row accepts.

EXACT rows (operands are fp16 values; every query's winner set of logits is >= 40 nats above the rest, so the softmax is uniform over that
set in every storage):
  N1 spike    keys are +-2^a e_d, the 49 slots of any 7 x 7 block getting distinct ones by (y mod 7, x mod 7); q = M k_target with the
              target cycling through all K^2 relative positions of the query's block, 2^-2.5 M |k|^2 = 90: out = v[target] bit for bit
  N2 self     q = 0, table +40 at offset (0, 0) and -40 elsewhere: out = v[self] bit for bit
  N3 table    q = 0, +40 on a fixed set of offsets reaching to +-(K - 1): the mean of v over those neighbours that sit at such an offset -
              corner and edge queries see other subsets than interior ones
  N4 uniform  q = 0, constant table: the mean over the K^2 neighbours
  N5 padded   N4 (N5u) and N1 (N5s) on the padded geometries with kv_pad set, and with None (N5un, N5sn): padded keys count, with
              v = kv_pad; in the N1 form a padded slot is the target of some queries
Where the size of the winner set is a power of two: torch.equal on the fp16 and packed storages; otherwise, and on the fp32 storage
throughout, the rule of scenario S3 of tests/_attn_cases.py: 0.5 ulp16(ref) + N 2^-23 max|v| per element, N = K^2.
BOUNDED rows (b): randn q, k, v (fp16 values), table ~ 0.5 randn, kv_pad ~ 0.3 randn - TOL_F16 on fp16, TOL_OP on packed / fp32, times
max|ref|; one such row per shape the two registered members hand the operator.
"""
import zlib
from collections import namedtuple

import torch

from tests import _nat_ref as ref

F64 = torch.float64
HD = 32
SCALE = 2.0 ** -2.5
TOL_F16 = 2e-3          # tests/test_gpu_passes.py TOL_F16
TOL_OP = 2e-5           # tests/test_gpu_passes.py TOL_OP
GAP = 40.0

Row = namedtuple("Row", "id kind B H W heads K")

# (H, W, K, B, heads): the issue's table
GEOMS = [(7, 7, 7, 3, 2), (8, 8, 7, 3, 1), (9, 12, 7, 3, 3), (16, 9, 7, 3, 2), (13, 13, 7, 3, 1), (25, 25, 7, 3, 2),
         (5, 7, 7, 3, 1), (3, 10, 7, 3, 2), (7, 4, 7, 3, 3), (2, 2, 7, 3, 1),
         (9, 9, 3, 3, 2), (6, 11, 5, 3, 3), (2, 5, 3, 3, 1),
         (50, 50, 7, 2, 1)]
EXACT_KINDS = ("N1", "N2", "N3", "N4", "N5u", "N5un", "N5s", "N5sn")
BOUNDED_KINDS = ("b",)
# every (heads, H) the two registered members hand the operator (C = 32 heads, K = 7), written out so that this table does not depend
# on the package (test_nat_cases_cpu.py compares the two)
MEMBER_SHAPES = [(2, 50), (4, 25), (8, 13), (16, 7), (4, 56), (8, 28), (16, 14), (32, 7)]


def member_shapes():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import nat
    out = []
    for name, hw in (("nat_mini", 200), ("nat_base", 224)):
        cfg = nat.CONFIGS[name]
        out += [(cfg["num_heads"][si], h) for si, (h, _) in enumerate(nat.stack_maps(hw))]
    return out


def padded(H, W, K):
    return H < K or W < K


def _rows():
    out = []
    for H, W, K, B, heads in GEOMS:
        kinds = ("N1", "N2", "N3", "N4") + (("N5u", "N5un", "N5s", "N5sn") if padded(H, W, K) else ()) + BOUNDED_KINDS
        for kind in kinds:
            out.append(Row(f"{kind}-{H}x{W}-k{K}-h{heads}", kind, B, H, W, heads, K))
    for heads, h in MEMBER_SHAPES:
        out.append(Row(f"member-{h}x{h}-k7-h{heads}", "b", 1, h, h, heads, 7))
    return out


ROWS = _rows()
EXACT = [r for r in ROWS if r.kind in EXACT_KINDS]
BOUNDED = [r for r in ROWS if r.kind in BOUNDED_KINDS]


def h(t):
    return t.to(torch.float16).to(torch.float32)


def ulp16(x):
    """fp16 unit in the last place at |x| (fp64 tensor): 2^(floor(log2|x|) - 10), 2^-24 in the subnormal range"""
    e = torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 10)


def _spike(j, a):
    """the j-th of the 64 vectors +-e_d (d = j mod 32, minus for j >= 32), times 2^a"""
    v = torch.zeros(HD)
    v[j % HD] = (1.0 if j < HD else -1.0) * 2.0 ** a
    return v


N3_OFFSETS = lambda K: [(0, 0), (K - 1, K - 1), (1 - K, 1 - K), (K - 1, 1 - K), (1 - K, K - 1), (K - 1, 0), (0, 1 - K), (1, -2), (-2, 1),  # noqa: E731
                        (K // 2 + 1, -1)]


def operands(row):
    """(qkv [B,H,W,3C], kv_pad [2C] or None, table [heads, (2K-1)^2]) as fp32 host tensors holding fp16 values (qkv) and fp32 parameters,
    seeded by the row's id"""
    gen = torch.Generator().manual_seed(zlib.crc32(row.id.encode()))
    B, H, W, heads, K = row.B, row.H, row.W, row.heads, row.K
    C, T, tw = heads * HD, (2 * K - 1) ** 2, 2 * K - 1
    Hp, Wp = max(H, K), max(W, K)
    kind = row.kind
    if kind in BOUNDED_KINDS:
        qkv = h(torch.randn(B, H, W, 3 * C, generator=gen))
        return qkv, 0.3 * torch.randn(2 * C, generator=gen), 0.5 * torch.randn(heads, T, generator=gen)

    spike = kind in ("N1", "N5s", "N5sn")
    with_pad = padded(H, W, K) and kind not in ("N5un", "N5sn")
    q = torch.zeros(B, H, W, heads, HD)

    def vals(*shape):                                                        # fp16 values, no subnormal and nothing near one
        t = h(torch.randn(*shape, generator=gen))
        return torch.where(t.abs() < 2.0 ** -10, torch.full_like(t, 0.5), t)

    # the mean rows hold POSITIVE values: a mean that cancels to 0 would leave the float64 reference at the e^-80 weight of the losers
    pos = (lambda t: t) if (spike or kind == "N2") else torch.abs
    k, v = vals(B, H, W, heads, HD), pos(vals(B, H, W, heads, HD))
    kv_pad = None
    if with_pad:
        vp, kp = pos(vals(heads, HD)), vals(heads, HD)
        if spike:                                                            # the padded key: a vector no real slot carries
            kp = torch.stack([_spike(49 + hh, float(torch.randint(-2, 3, (1,), generator=gen))) for hh in range(heads)])
        kv_pad = torch.cat([kp.reshape(-1), vp.reshape(-1)])
    table = torch.full((heads, T), 0.5)
    if kind == "N2":
        table = torch.full((heads, T), -40.0)
        table[:, (K - 1) * tw + K - 1] = 40.0
    elif kind == "N3":
        table = torch.full((heads, T), -40.0)
        for hh in range(heads):
            for dy, dx in N3_OFFSETS(K) + [(-(hh % K), hh % K)]:
                if abs(dy) < K and abs(dx) < K:
                    table[hh, (dy + K - 1) * tw + dx + K - 1] = 40.0
    if spike:
        kfull = torch.zeros(B, Hp, Wp, heads, HD)                           # the padded map's keys
        for y in range(Hp):
            for x in range(Wp):
                if y < H and x < W:
                    for b in range(B):
                        for hh in range(heads):
                            kfull[b, y, x, hh] = _spike((y % 7) * 7 + x % 7, float(torch.randint(-2, 3, (1,), generator=gen)))
                elif with_pad:
                    kfull[:, y, x] = kv_pad[:C].reshape(heads, HD)
        k = kfull[:, :H, :W].clone()
        r = K // 2
        for y in range(H):
            for x in range(W):
                sy, sx = min(max(y - r, 0), Hp - K), min(max(x - r, 0), Wp - K)
                for b in range(B):
                    for hh in range(heads):
                        jy, jx = divmod((y * W + x + b + 3 * hh) % (K * K), K)
                        kt = kfull[b, sy + jy, sx + jx, hh]
                        n2 = float((kt * kt).sum())
                        if n2 > 0:                                           # a padded target without kv_pad: q = 0, a uniform block
                            q[b, y, x, hh] = kt * (2.0 ** 9 / n2)            # q . k_target = 2^9: the logit is 90.5
    qkv = torch.cat([q.reshape(B, H, W, C), k.reshape(B, H, W, C), v.reshape(B, H, W, C)], -1)
    assert torch.equal(h(qkv), qkv), row.id                                  # representable in fp16
    return qkv.contiguous(), kv_pad, table


def ref64(row, ops_=None):
    """the layer as the reference writes it, float64, one head at a time (the K^2 patch copies of a whole map are large)"""
    qkv, kv_pad, table = ops_ if ops_ is not None else operands(row)
    C = row.heads * HD
    outs = []
    for hh in range(row.heads):
        sl = [slice(p * C + hh * HD, p * C + (hh + 1) * HD) for p in range(3)]
        one = torch.cat([qkv[..., s] for s in sl], -1).to(F64)
        pad = None if kv_pad is None else torch.cat([kv_pad[hh * HD:(hh + 1) * HD], kv_pad[C + hh * HD:C + (hh + 1) * HD]]).to(F64)
        outs.append(ref.core(one, pad, table[hh:hh + 1].to(F64), 1, row.K))
    return torch.cat(outs, -1)


MUTANTS = ("no-low-clamp", "high-clamp-plus-one", "table-by-window-position", "offset-exchanged", "table-stride-K", "hw-exchanged",
           "no-scale", "bias-scaled", "halo-unmasked", "padded-keys-masked", "padded-values-zero", "k-from-v-plane", "image-0-for-all")


def folded(qkv, kv_pad, table, heads, K=7, mutant=None, dtype=torch.float32, round16=False, want_logits=False):
    """The kernel's formula in `dtype` arithmetic, dense and masked as the kernel computes it: every query against every token of the
    padded map, tokens outside the query's K x K block masked; block origin sy = clamp(y - r, 0, Hp - K), table index by the
    key-minus-query offset.  round16: the fp16 kernel's roundings (the unnormalised probabilities and kv_pad to fp16).  `mutant`: one
    deliberate mistake (MUTANTS)."""
    B, H, W, C3 = qkv.shape
    C = C3 // 3
    r, tw = K // 2, 2 * K - 1
    Hp, Wp = max(H, K), max(W, K)
    x = qkv.to(dtype)
    fill = torch.zeros(2 * C, dtype=dtype)
    if kv_pad is not None:
        fill = (kv_pad.to(torch.float16) if round16 else kv_pad).to(dtype).clone()
        if mutant == "padded-values-zero":
            fill[C:] = 0
    kv = fill.expand(B, Hp, Wp, 2 * C).clone()
    kv[:, :H, :W] = x[..., C:]
    if mutant == "image-0-for-all":
        kv = kv[:1].expand(B, Hp, Wp, 2 * C)
    q = x[..., :C].reshape(B, H * W, heads, HD).permute(0, 2, 1, 3)                               # [B, heads, HW, hd]
    kk = kv[..., (C if mutant == "k-from-v-plane" else 0):][..., :C].reshape(B, Hp * Wp, heads, HD).permute(0, 2, 1, 3)
    vv = kv[..., C:].reshape(B, Hp * Wp, heads, HD).permute(0, 2, 1, 3)

    y, xx = torch.arange(H)[:, None].expand(H, W).reshape(-1), torch.arange(W)[None, :].expand(H, W).reshape(-1)
    ky, kx = torch.arange(Hp)[:, None].expand(Hp, Wp).reshape(-1), torch.arange(Wp)[None, :].expand(Hp, Wp).reshape(-1)
    Lh, Lw = (Wp, Hp) if mutant == "hw-exchanged" else (Hp, Wp)
    hi_y, hi_x = (Lh - K + 1, Lw - K + 1) if mutant == "high-clamp-plus-one" else (Lh - K, Lw - K)
    lo = -10 ** 6 if mutant == "no-low-clamp" else 0
    sy, sx = (y - r).clamp(lo, hi_y), (xx - r).clamp(lo, hi_x)
    inblk = (ky[None] >= sy[:, None]) & (ky[None] < sy[:, None] + K) & (kx[None] >= sx[:, None]) & (kx[None] < sx[:, None] + K)   # [HW, HpWp]
    if mutant == "halo-unmasked":                                                                 # the whole halo of the query's 8 x 8 tile
        def ext(t, n, np_):
            t0 = (t // 8) * 8
            o = (t0 - r).clamp(0, np_ - K)
            e = (torch.minimum(t0 + 7, torch.tensor(n - 1)) - r).clamp(0, np_ - K) + K
            return o, e
        oy, ey = ext(y, H, Hp)
        ox, ex = ext(xx, W, Wp)
        inblk = (ky[None] >= oy[:, None]) & (ky[None] < ey[:, None]) & (kx[None] >= ox[:, None]) & (kx[None] < ex[:, None])
    if mutant == "padded-keys-masked":
        inblk = inblk & ((ky < H) & (kx < W))[None]
    dy, dx = ky[None] - y[:, None], kx[None] - xx[:, None]
    if mutant == "offset-exchanged":
        dy, dx = -dy, -dx
    if mutant == "table-by-window-position":
        dy, dx = ky[None] - sy[:, None] - r, kx[None] - sx[:, None] - r
    dy, dx = (dy + K - 1).clamp(0, tw - 1), (dx + K - 1).clamp(0, tw - 1)
    idx = dy * K + dx if mutant == "table-stride-K" else dy * tw + dx
    bias = table.to(dtype)[:, idx]                                                                # [heads, HW, HpWp]
    scale = 1.0 if mutant == "no-scale" else SCALE
    dots = q @ kk.transpose(-1, -2)
    logits = (dots + bias[None]) * scale if mutant == "bias-scaled" else dots * scale + bias[None]
    logits = logits.masked_fill(~inblk[None, None], float("-inf"))
    if want_logits:
        return logits
    m = logits.max(-1, keepdim=True).values
    e = torch.exp(logits - m)
    o = ((e.to(torch.float16).to(dtype) if round16 else e) @ vv) / e.sum(-1, keepdim=True)
    return o.permute(0, 2, 1, 3).reshape(B, H, W, C)


def emulate(row, ops_, mutant=None, round16=False):
    qkv, kv_pad, table = ops_
    return folded(qkv, kv_pad, table, row.heads, row.K, mutant=mutant, round16=round16)


def top_sets(row, ops_):
    """(gap, count) [B, heads, HW]: how far each query's winner set of logits (within 1e-9 of the maximum) is above the rest, and the
    size of that set - float64, the folded form's logits"""
    logits = folded(*ops_, row.heads, row.K, dtype=F64, want_logits=True)
    m = logits.max(-1, keepdim=True).values
    top = logits >= m - 1e-9
    rest = logits.masked_fill(top, float("-inf")).max(-1).values
    return m[..., 0] - rest, top.sum(-1)


def pow2_mask(row, ops_):
    """[B, H, W, C] bool: outputs whose winner set has a power-of-two size (their mean is exact in every storage)"""
    _, cnt = top_sets(row, ops_)
    p2 = ((cnt & (cnt - 1)) == 0).permute(0, 2, 1)                                                # [B, HW, heads]
    return p2[..., None].expand(*p2.shape, HD).reshape(row.B, row.H, row.W, row.heads * HD)


def s3_bound(ref_out, v_absmax, N):
    """scenario S3 of tests/_attn_cases.py, per element: one fp16 rounding of the mean + the round-to-nearest bound of an N-term fp32 sum"""
    return 0.5 * ulp16(ref_out) + N * 2.0 ** -23 * v_absmax


def tolerance(row, storage, ref_out):
    """the absolute bound a BOUNDED row accepts on `storage` ("f16" | "h2" | "s32")"""
    return (TOL_F16 if storage == "f16" else TOL_OP) * ref_out.abs().max().item()


def v_absmax(row, ops_):
    vmax = ops_[0][..., 2 * row.heads * HD:].abs().max().item()
    return vmax if ops_[1] is None else max(vmax, ops_[1][row.heads * HD:].abs().max().item())


def plan_items(B, H, W, heads):
    """work items of a launch: B x 8 x 8 query tiles x heads"""
    return B * (-(-H // 8)) * (-(-W // 8)) * heads
