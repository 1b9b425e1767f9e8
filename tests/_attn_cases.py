"""Attention scenarios with structured logits, and their fp64 reference (CPU only).

Every attention kernel computes exp2(s - m) over one row of logits, masks its padded key slots by VALUE and divides by the row sum.
With N(0, 1) logits and `check()` (maximum error over max|ref|) a wrong running maximum, a padded slot left at logit 0, a hard-coded
scale or Hp / Wp exchanged in the window index all pass.  The scenarios below make each of them visible:

  S1  permutation spike   q_i = 64 k_pi(i): every key position dominates some query by >= 40 nats; the attention core returns
                          v[pi(i)] BIT FOR BIT (every other p <= e^-40 is 0 in fp16, the row sum rounds to 1, 1.0 * v is exact)
  S2  common offset       k_j = u + e_j, q_i = a u + r_i with e_j orthogonal to u: the ordinary random softmax, every logit + 600
  S3  uniform             q = 0, no bias: the mean of v over exactly the N real keys, to one fp16 rounding
  S4  bias-dominated      q, k ~ 0.1 randn, table entries +-40: the relative-position table decides (window kernels)
  S5  far below zero      S2 with a < 0: every real logit near -600, so a padded key slot left at 0 would take the whole row
  S6  off-default         randn inputs, scale 0.25 / 0.09, maps (ws, 3 ws) and (2 ws, ws)

A case is a `Case`: the kernel's inputs (fp16-representable fp32 tensors), the attention core in fp64 ([G, heads, N, hd] q, k, v and
the bias [heads, N, N]), `finish` (the core's output -> the kernel's output layout, fp64) and `ref` = finish(core).  `ref` goes through
the oracle's own dtype-generic functions on float64 tensors.

Where the S2 / S5 note says "e_j orthogonal to u": with plain randn e_j the term scale * a * (u . e_j) = 600 (u . e_j) / |u|^2 would
spread the logits of one row by ~100 nats - a second spike scenario, not a shifted random softmax.
"""
import math

import torch

from oracle import gcvit_ref
from oracle import ops_ref as R

F64 = torch.float64
G_SPIKE = 64.0            # S1: q = G_SPIKE * k[pi]  (a power of two: exact in fp16 and through every rounding of k)
OFFSET = 600.0            # S2 / S5: |common logit offset| in nats
MIN_GAP = 40.0            # S1 precondition (nats): e^-40 = 4.2e-18 rounds to 0 in fp16 (smallest subnormal 6e-8)
MIN_WEIGHT = 1.0 - 2.0 ** -30
TOL_F16 = 3e-3            # the fp16 kernels' own tests: check(..., tol=3e-3) in tests/test_gpu_ops.py / test_gpu_tfimm.py
TOL_STRICT = 2e-5         # tests/test_gpu_strict.py TOL_OP


def h(t):
    """fp16-rounded fp32 copy of t (what the kernels are given)"""
    return t.to(torch.float16).to(torch.float32)


def ulp16(x):
    """spacing of fp16 at |x| (float64 tensor): 2^(e-10) for normals, 2^-24 below 2^-14"""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(torch.tensor(2.0, dtype=F64), e - 10)


# ---- the core in fp64 -----------------------------------------------------------------------------------------------------------
def rel_bias(table, ws):
    """[(2ws-1)^2, heads] -> [heads, N, N]"""
    idx = R.relative_position_index(ws).reshape(-1)
    return table[idx].reshape(ws * ws, ws * ws, -1).permute(2, 0, 1)


def core_logits(q, k, bias, scale):
    s = scale * (q @ k.transpose(-1, -2))
    return s if bias is None else s + bias[None]


def core_from_logits(logits, v):
    return torch.softmax(logits, dim=-1) @ v


def split_window(qkv, qg, heads, ws):
    """feature map [B, Hp, Wp, nq C] (+ q_global [B, N, C]) -> q, k, v [B_, heads, N, hd], as the existing window tests do"""
    B, Hp, Wp, CC = qkv.shape
    nq = 2 if qg is not None else 3
    C, N = CC // nq, ws * ws
    hd = C // heads
    win = R.window_partition(qkv, ws).reshape(-1, N, nq, heads, hd).permute(2, 0, 3, 1, 4)
    B_ = win.shape[1]
    if qg is not None:
        q = torch.repeat_interleave(qg.reshape(B, N, C), B_ // B, dim=0).reshape(B_, N, heads, hd).permute(0, 2, 1, 3)
        return q, win[0], win[1]
    return win[0], win[1], win[2]


def merge_window(o, ws, Hp, Wp):
    """[B_, heads, N, hd] -> [B, Hp, Wp, C]"""
    B_, heads, N, hd = o.shape
    return R.window_reverse(o.permute(0, 2, 1, 3).reshape(B_, N, heads * hd), ws, Hp, Wp, heads * hd)


def window_ref(qkv, qg, table, heads, ws, scale, dtype=F64):
    """vip_window_attn_fwd_*: the oracle's attention core between the oracle's window partition / reverse, in `dtype`"""
    qkv, table = qkv.to(dtype), table.to(dtype)
    q, k, v = split_window(qkv, None if qg is None else qg.to(dtype), heads, ws)
    return merge_window(gcvit_ref.window_attention_core(q, k, v, table, ws, scale), ws, qkv.shape[1], qkv.shape[2])


def mhsa_ref(qkv, heads, scale, dtype=F64):
    """vip_mhsa_fwd_*: the expression of tests/test_gpu_tfimm.py::test_mhsa, in `dtype`"""
    qkv = qkv.to(dtype)
    B, N, D3 = qkv.shape
    D = D3 // 3
    q, k, v = qkv.reshape(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    attn = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    return (attn @ v).permute(0, 2, 1, 3).reshape(B, N, D)


def block_ref(x, qg, gam, bet, wq, bq, wp, bp, table, heads, ws, scale, dtype=F64):
    """vip_gcvit_attn_block_f16: the restatement of tests/test_gpu_ops.py::test_gcvit_attn_block_fused, in `dtype`"""
    x = x.to(dtype)
    qkv = R.dense(R.layernorm(x, gam.to(dtype), bet.to(dtype), 1e-5), wq.to(dtype), bq.to(dtype))
    att = window_ref(qkv, qg, table, heads, ws, scale, dtype)
    return x + R.dense(att, wp.to(dtype), bp.to(dtype))


class Case:
    """one scenario for one kernel family.  kind: "window" | "mhsa" | "block"; inputs: what the kernel is given (fp32, fp16-exact)"""

    def __init__(self, kind, scen, name, inputs, heads, scale, q, k, v, bias, finish, ref, designed, ws=None, exact=None, items=None, pi=None,
                 exact_rule=None):
        self.kind, self.scen, self.name, self.inputs, self.heads, self.scale, self.ws = kind, scen, name, inputs, heads, scale, ws
        self.q, self.k, self.v, self.bias = q, k, v, bias          # fp64 core operands [G, heads, N, hd], bias [heads, N, N] or None
        self.finish = finish                                       # core output [G, heads, N, hd] -> kernel output layout (fp64)
        self.ref = ref                                             # fp64, through the oracle's functions
        self.designed = designed                                   # bool, broadcastable to ref: the elements the scenario is about
        self.items = torch.ones(q.shape[0], dtype=torch.bool) if items is None else items   # bool [G]: core items holding designed queries
        self.exact = exact                                         # S1 attention core: the expected fp16 values (as fp32), bit for bit
        self.pi = pi                                               # S1: [G, heads, N] the key each query was built from
        self.exact_rule = exact_rule                               # S1 fused block: x + proj(v[pi]) in fp64 (what a saturated softmax leaves)

    @property
    def N(self):
        return self.q.shape[2]

    def logits(self):
        return core_logits(self.q, self.k, self.bias, self.scale)


def spike_precondition(case):
    """S1: (smallest weight of the target key, smallest gap to the runner-up in nats) over the designed queries, in fp64.
    The target of query i is the key with the largest logit; `case.pi` names the key it was built from."""
    L = case.logits()[case.items]
    pi = case.pi[case.items]
    tgt = L.gather(-1, pi[..., None])[..., 0]
    assert torch.equal(L.argmax(-1), pi) or case.N == 1
    rest = L.scatter(-1, pi[..., None], -math.inf).max(-1).values
    w = torch.softmax(L, dim=-1).gather(-1, pi[..., None])[..., 0]
    return w.min().item(), (tgt - rest).min().item()


def conditioning(case, tol, seed=4242):
    """The fused block rounds q and k to fp16 on its own.  A case is compared only where the fp64 reference moves by
    less than a quarter of its tolerance (tol * max|ref|, as check() measures) when every logit is perturbed by max|logit| * 2^-10 with
    seeded signs.  Returns (bool mask like ref: well conditioned, largest movement / (tol * max|ref|))."""
    L = case.logits()
    g = torch.Generator().manual_seed(seed)
    sign = torch.randint(0, 2, L.shape, generator=g).to(F64) * 2 - 1
    moved = case.finish(core_from_logits(L + sign * (L.abs().max() * 2.0 ** -10), case.v))
    d = (moved - case.ref).abs()
    lim = tol * case.ref.abs().max()
    return d < 0.25 * lim, (d.max() / lim).item()


def uniform_bound(case):
    """S3, per element: one fp16 rounding of the mean + twice the round-to-nearest bound of an N-term fp32 sum of |v| <= max|v|"""
    return 0.5 * ulp16(case.ref) + case.N * 2.0 ** -23 * case.v.abs().max()


# ---- scenario cores: q, k, v [G, heads, N, hd] (fp16-exact fp32) -------------------------------------------------------------------
def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen)


def _perms(gen, G, heads, N):
    return torch.stack([torch.randperm(N, generator=gen) for _ in range(G * heads)]).reshape(G, heads, N)


def _gaps(q, k, bias, scale, pi):
    L = core_logits(q.to(F64), k.to(F64), bias, scale)
    tgt = L.gather(-1, pi[..., None])[..., 0]
    return tgt - L.scatter(-1, pi[..., None], -math.inf).max(-1).values


def _spike_core(gen, G, heads, N, hd, scale, bias):
    """k ~ randn, redrawn row by row (seeded) until every query q_i = 64 k[pi(i)] beats its runner-up by MIN_GAP + 4 nats: with
    plain randn rows 2 - 5 % of the queries of a 49- or 196-key window have a neighbour within 40 nats"""
    k = h(_randn(gen, G, heads, N, hd))
    pi = _perms(gen, G, heads, N)
    for _ in range(500):
        q = G_SPIKE * k.gather(2, pi[..., None].expand_as(k))
        bad = _gaps(q, k, bias, scale, pi) < MIN_GAP + 4.0                    # per query i
        if not bad.any():
            return q, k, pi
        rows = torch.zeros_like(bad).scatter_(2, pi, bad)                      # the key rows those queries were built from
        k = torch.where(rows[..., None], h(_randn(gen, G, heads, N, hd)), k)
    raise AssertionError("S1: no separated key set found")


def _offset_core(gen, G, heads, N, hd, scale, offset, u=None):
    """k_j = u + e_j (e_j orthogonal to u), q_i = a u + r_i, a = offset / (scale |u|^2)"""
    u = _randn(gen, G, heads, 1, hd) if u is None else u
    e, r = _randn(gen, G, heads, N, hd), _randn(gen, G, heads, N, hd)
    uu = (u * u).sum(-1, keepdim=True)
    e = e - (e * u).sum(-1, keepdim=True) / uu * u
    a = offset / (scale * uu)
    return h(a * u + r), h(u + e)


def _table(gen, ws, heads, scen):
    n = (2 * ws - 1) ** 2
    if scen == "S3":
        return torch.zeros(n, heads)
    if scen == "S4":
        sign = torch.randint(0, 2, (n, heads), generator=gen).float() * 2 - 1
        return 40.0 * sign + _randn(gen, n, heads)
    return _randn(gen, n, heads) * 0.5


def _tokens_to_map(parts, ws, Hp, Wp):
    """q / k / v [B_, heads, N, hd] each -> feature map [B, Hp, Wp, len(parts) * C] with channels (part, head, hd)"""
    t = torch.stack(parts, 0)                                                  # [nq, B_, heads, N, hd]
    nq, B_, heads, N, hd = t.shape
    tok = t.permute(1, 3, 0, 2, 4).reshape(B_, N, nq * heads * hd)
    return R.window_reverse(tok.reshape(B_, ws, ws, -1), ws, Hp, Wp, tok.shape[-1])


def window_case(scen, ws, heads, global_q, seed, nwin=(1, 1), scale=None, offset=OFFSET, B=2, hd=32):
    """inputs of vip_window_attn_fwd_f16 / _h2 / _s32: qkv [B, Hp, Wp, nq C], q_global [B, N, C] or None, table [(2ws-1)^2, heads]"""
    gen = torch.Generator().manual_seed(seed)
    N, C = ws * ws, heads * hd
    Hp, Wp = nwin[0] * ws, nwin[1] * ws
    nW = nwin[0] * nwin[1]
    G = B * nW
    scale = hd ** -0.5 if scale is None else scale
    table = _table(gen, ws, heads, scen)
    bias = rel_bias(table.to(F64), ws)
    v = h(_randn(gen, G, heads, N, hd))
    pi = None
    if scen == "S1":
        q, k, pi = _spike_core(gen, G, heads, N, hd, scale, bias)
    elif scen in ("S2", "S5"):
        q, k = _offset_core(gen, G, heads, N, hd, scale, offset if scen == "S2" else -offset)
    elif scen == "S3":
        q, k = torch.zeros(G, heads, N, hd), h(_randn(gen, G, heads, N, hd))
    elif scen == "S4":
        q, k = h(0.1 * _randn(gen, G, heads, N, hd)), h(0.1 * _randn(gen, G, heads, N, hd))
    else:                                                                      # S6, and "S0": the present style of case
        q, k = h(_randn(gen, G, heads, N, hd)), h(_randn(gen, G, heads, N, hd))
    designed = torch.ones(1, dtype=torch.bool)
    qg = None
    if global_q:
        # one query set per image, taken from its window 0: only those windows are the designed ones of S1
        qg = q[::nW].permute(0, 2, 1, 3).reshape(B, N, C).contiguous()
        q = torch.repeat_interleave(q[::nW], nW, dim=0)
        if scen == "S1":
            pi = torch.repeat_interleave(pi[::nW], nW, dim=0)
            win0 = torch.zeros(B, nwin[0], 1, nwin[1], 1, 1, dtype=torch.bool)
            win0[:, 0, :, 0] = True
            designed = win0.expand(B, nwin[0], ws, nwin[1], ws, 1).reshape(B, Hp, Wp, 1)
    qkv = _tokens_to_map([k, v] if global_q else [q, k, v], ws, Hp, Wp).contiguous()
    ref = window_ref(qkv, qg, table, heads, ws, scale)
    q64, k64, v64 = split_window(qkv.to(F64), None if qg is None else qg.to(F64), heads, ws)
    case = Case("window", scen, f"{scen} ws{ws} heads{heads} map{Hp}x{Wp} global={int(global_q)} scale={scale:.3g}",
                dict(qkv=qkv, qg=qg, table=table), heads, scale, q64, k64, v64, bias, lambda o: merge_window(o, ws, Hp, Wp), ref,
                designed, ws=ws, items=(torch.arange(G) % nW == 0) if (global_q and scen == "S1") else None, pi=pi,
                exact=merge_window(v.gather(2, pi[..., None].expand_as(v)), ws, Hp, Wp) if scen == "S1" else None)
    return case


def mhsa_case(scen, N, heads, seed, scale=None, offset=OFFSET, B=2, hd=64):
    """input of vip_mhsa_fwd_f16 / _h2 / _s32: qkv [B, N, 3 D] with channels (q | k | v, head, hd)"""
    gen = torch.Generator().manual_seed(seed)
    scale = hd ** -0.5 if scale is None else scale
    v = h(_randn(gen, B, heads, N, hd))
    pi = None
    if scen == "S1":
        q, k, pi = _spike_core(gen, B, heads, N, hd, scale, None)
    elif scen in ("S2", "S5"):
        q, k = _offset_core(gen, B, heads, N, hd, scale, offset if scen == "S2" else -offset)
    elif scen == "S3":
        q, k = torch.zeros(B, heads, N, hd), h(_randn(gen, B, heads, N, hd))
    else:
        q, k = h(_randn(gen, B, heads, N, hd)), h(_randn(gen, B, heads, N, hd))
    qkv = torch.stack([q, k, v], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * heads * hd).contiguous()
    ref = mhsa_ref(qkv, heads, scale)
    q64, k64, v64 = qkv.to(F64).reshape(B, N, 3, heads, hd).permute(2, 0, 3, 1, 4)

    def finish(o):
        return o.permute(0, 2, 1, 3).reshape(B, N, heads * hd)
    case = Case("mhsa", scen, f"{scen} N{N} heads{heads} scale={scale:.3g}", dict(qkv=qkv), heads, scale, q64, k64, v64, None, finish, ref,
                torch.ones(1, dtype=torch.bool), pi=pi, exact=finish(v.gather(2, pi[..., None].expand_as(v))) if scen == "S1" else None)
    return case


def block_case(scen, heads, global_q, seed, nwin=(1, 1), offset=OFFSET, B=2, hd=32):
    """inputs of vip_gcvit_attn_block_f16 (x, LayerNorm, qkv and proj weights, table, q_global), drawn as test_gcvit_attn_block_fused
    draws them and then shaped so that the q, k the block computes form the scenario:
      S1  Wq = 64 Wk, bq = 64 bk (pi = identity); global: q_global = 64 * the reference's fp16-rounded k of window 0
      S2 / S5  the k weights of each head projected orthogonal to u, bk = u, bq = a u; global: q_global = a u + randn
      S3  Wq = 0, bq = 0 (global: q_global = 0), table = 0"""
    gen = torch.Generator().manual_seed(seed)
    ws = 14 if heads == 8 else 7
    C, N = heads * hd, ws * ws
    Hp, Wp = nwin[0] * ws, nwin[1] * ws
    nW = nwin[0] * nwin[1]
    nq = 2 if global_q else 3
    scale = hd ** -0.5
    ko = (nq - 2) * C                                                          # first k channel of the qkv output
    x = h(_randn(gen, B, Hp, Wp, C) * 1.5 + 0.2)
    gam, bet = _randn(gen, C) * 0.2 + 1.0, _randn(gen, C) * 0.1
    wq, bq = _randn(gen, C, nq * C) / math.sqrt(C), _randn(gen, nq * C) * 0.1
    wp, bp = h(_randn(gen, C, C) / math.sqrt(C)), _randn(gen, C) * 0.1
    table = _table(gen, ws, heads, scen)
    qg = h(_randn(gen, B, N, C)) if global_q else None
    if scen == "S1" and not global_q:
        wq[:, :C], bq[:C] = G_SPIKE * h(wq[:, ko:ko + C]), G_SPIKE * bq[ko:ko + C]
    elif scen in ("S2", "S5"):
        u = _randn(gen, heads, hd)
        uu = (u * u).sum(-1, keepdim=True)
        a = (offset if scen == "S2" else -offset) / (scale * uu)
        wk = wq[:, ko:ko + C].reshape(C, heads, hd)
        wq[:, ko:ko + C] = (wk - (wk * u).sum(-1, keepdim=True) / uu * u).reshape(C, C)
        bq[ko:ko + C] = u.reshape(C)
        if global_q:
            qg = h((a * u).reshape(1, 1, C) + _randn(gen, B, N, C))
        else:
            bq[:C] = (a * u).reshape(C)
    elif scen == "S3":
        if global_q:
            qg = torch.zeros(B, N, C)
        else:
            wq[:, :C], bq[:C] = 0.0, 0.0
    wq = h(wq)

    def qkv_of(xx):
        return R.dense(R.layernorm(xx.to(F64), gam.to(F64), bet.to(F64), 1e-5), wq.to(F64), bq.to(F64))
    bias = rel_bias(table.to(F64), ws)
    designed = torch.ones(1, dtype=torch.bool)
    if scen == "S1":
        # pi = identity.  Tokens whose query has a neighbour within MIN_GAP + 4 nats in any head are redrawn (seeded).
        ident = torch.arange(N).reshape(1, 1, N).expand(B * nW, heads, N)
        for _ in range(500):
            k = split_window(qkv_of(x)[..., ko:ko + 2 * C], torch.zeros(B, N, C, dtype=F64), heads, ws)[1]
            bad = (_gaps(G_SPIKE * h(k), k, bias, scale, ident) < MIN_GAP + 4.0).any(1)          # [B_, N] tokens
            if global_q:
                bad[torch.arange(B * nW) % nW != 0] = False                                     # only window 0 of an image is designed
            if not bad.any():
                break
            badmap = R.window_reverse(bad.reshape(-1, ws, ws, 1), ws, Hp, Wp, 1)
            x = torch.where(badmap, h(_randn(gen, B, Hp, Wp, C) * 1.5 + 0.2), x)
        else:
            raise AssertionError("S1 (block): no separated token set found")
        if global_q:
            qg = (G_SPIKE * h(k[::nW])).permute(0, 2, 1, 3).reshape(B, N, C).float().contiguous()
            win0 = torch.zeros(B, nwin[0], 1, nwin[1], 1, 1, dtype=torch.bool)
            win0[:, 0, :, 0] = True
            designed = win0.expand(B, nwin[0], ws, nwin[1], ws, 1).reshape(B, Hp, Wp, 1)
    ref = block_ref(x, qg, gam, bet, wq, bq, wp, bp, table, heads, ws, scale)
    q64, k64, v64 = split_window(qkv_of(x), None if qg is None else qg.to(F64), heads, ws)

    def finish(o):
        return x.to(F64) + R.dense(merge_window(o, ws, Hp, Wp), wp.to(F64), bp.to(F64))
    s1 = scen == "S1"
    return Case("block", scen, f"{scen} C{C} heads{heads} ws{ws} map{Hp}x{Wp} global={int(global_q)}",
                dict(x=x, qg=qg, gam=gam, bet=bet, wq=wq, bq=bq, wp=wp, bp=bp, table=table), heads, scale, q64, k64, v64, bias, finish,
                ref, designed, ws=ws, items=(torch.arange(B * nW) % nW == 0) if (global_q and s1) else None,
                pi=torch.arange(N).reshape(1, 1, N).expand(B * nW, heads, N) if s1 else None, exact_rule=finish(v64) if s1 else None)


# ---- the case tables (shared by the CPU and the GPU tests) ------------------------------------------------------------------------
_CACHE = {}


def build(spec):
    """spec = (kind, scen, kwargs-as-sorted-tuple); cases are built once per process and never modified"""
    if spec not in _CACHE:
        kind, scen, kw = spec
        _CACHE[spec] = {"window": window_case, "mhsa": mhsa_case, "block": block_case}[kind](scen, **dict(kw))
    return _CACHE[spec]


def _s(kind, scen, **kw):
    return (kind, scen, tuple(sorted(kw.items())))


def spec_id(spec):
    return f"{spec[0]}-{spec[1]}-" + "-".join(f"{k}{v}" for k, v in spec[2]).replace(" ", "").replace("(", "").replace(")", "").replace(",", "x")


# vip_window_attn_fwd_f16: ws 7 (one wave per item, 49 of 64 key slots real) and ws 14 (four waves per item, 196 of 224), local and
# global query, heads 2 / 4 / 8, one or two windows a side; S6: both scales and both non-square maps
WINDOW_F16 = [
    _s("window", "S1", ws=7, heads=2, global_q=False, seed=101, nwin=(1, 2)),
    _s("window", "S1", ws=7, heads=4, global_q=True, seed=102, nwin=(2, 2)),
    _s("window", "S1", ws=14, heads=8, global_q=False, seed=103),
    _s("window", "S1", ws=14, heads=4, global_q=True, seed=104, nwin=(2, 1)),
    _s("window", "S2", ws=7, heads=4, global_q=False, seed=111, nwin=(2, 2)),
    _s("window", "S2", ws=7, heads=2, global_q=True, seed=112),
    _s("window", "S2", ws=14, heads=8, global_q=False, seed=113),
    _s("window", "S2", ws=14, heads=2, global_q=True, seed=114, nwin=(1, 2)),
    _s("window", "S3", ws=7, heads=2, global_q=False, seed=121, nwin=(2, 1)),
    _s("window", "S3", ws=7, heads=8, global_q=True, seed=122),
    _s("window", "S3", ws=14, heads=4, global_q=False, seed=123),
    _s("window", "S3", ws=14, heads=2, global_q=True, seed=124),
    _s("window", "S4", ws=7, heads=2, global_q=False, seed=131, nwin=(2, 2)),
    _s("window", "S4", ws=7, heads=4, global_q=True, seed=132),
    _s("window", "S4", ws=14, heads=8, global_q=False, seed=133),
    _s("window", "S4", ws=14, heads=2, global_q=True, seed=134),
    _s("window", "S5", ws=7, heads=2, global_q=False, seed=141),
    _s("window", "S5", ws=7, heads=8, global_q=True, seed=142, nwin=(1, 2)),
    _s("window", "S5", ws=14, heads=4, global_q=False, seed=143),
    _s("window", "S5", ws=14, heads=2, global_q=True, seed=144),
    _s("window", "S6", ws=7, heads=2, global_q=False, seed=151, nwin=(1, 3), scale=0.25),
    _s("window", "S6", ws=7, heads=4, global_q=True, seed=152, nwin=(2, 1), scale=0.09),
    _s("window", "S6", ws=14, heads=2, global_q=False, seed=153, nwin=(2, 1), scale=0.09),
    _s("window", "S6", ws=14, heads=2, global_q=True, seed=154, nwin=(1, 3), scale=0.25),
]

# window_attn_pipe_kernel: ws 14, B * nW * nW * heads >= 1024 items as its existing test.  (spec, rep): the 4 images of the case are given
# to the kernel `rep` times over (the reference is computed once); compared with the rule AND bit for bit with the plain kernel
WINDOW_PIPE = [
    (_s("window", "S1", ws=14, heads=8, global_q=False, seed=201, B=4), 32),                 # 1024 items
    (_s("window", "S2", ws=14, heads=8, global_q=True, seed=202, B=4, nwin=(2, 2)), 9),      # 1152 items
    (_s("window", "S5", ws=14, heads=4, global_q=False, seed=203, B=4, nwin=(2, 2)), 17),    # 1088 items
]

# vip_mhsa_fwd_f16: N in {1, 16, 17, 33, 197, 224} (one key; a full tile; one key into the second tile / the second PV step; ViT's 197;
# the 224-row limit), heads 1 / 3
MHSA_F16 = [_s("mhsa", scen, N=N, heads=heads, seed=300 + 10 * i + j)
            for i, scen in enumerate(["S1", "S2", "S3", "S5"])
            for j, (N, heads) in enumerate([(1, 1), (16, 3), (17, 1), (33, 3), (197, 3), (224, 1)])] + [
    _s("mhsa", "S6", N=33, heads=3, seed=351, scale=0.25), _s("mhsa", "S6", N=197, heads=1, seed=352, scale=0.09),
    _s("mhsa", "S6", N=224, heads=3, seed=353, scale=0.25), _s("mhsa", "S6", N=17, heads=1, seed=354, scale=0.09)]

# vip_gcvit_attn_block_f16 and its four-launch fallback: C 64 / 2 heads (a wave per window), C 128 / 4 heads (two waves per window),
# C 256 / 8 heads (ws 14, experiments build).  The block rounds q and k to fp16 itself, so conditioning() decides what is compared:
# S1 and S3 pass it everywhere; S2 / S5 / S6 cannot (plain randn logits already move the reference by 0.29 - 0.33 of the tolerance,
# above the quarter the rule allows), so they are compared element by element where the rule holds.  At |offset| 600 that is 3 - 6 % of
# the elements, and an fp32 emulation with the block's own fp16 roundings of q and k is already 5.7e-3 * max|ref| off on those: no
# kernel that stores q, k in fp16 can be held to 3e-3 there, so the block's S2 / S5 use |offset| 8 (85 - 99 % compared; -8 against 49
# or 196 real keys is still enough for a padded key slot left at logit 0 to take the row).  Large logits reach the block through S1.
BLOCK_CFGS = [(2, False, (1, 2)), (2, True, (2, 1)), (4, False, (2, 1)), (4, True, (1, 3)), (8, False, (1, 1)), (8, True, (2, 1))]
BLOCK = [_s("block", scen, heads=heads, global_q=gq, seed=400 + 10 * i + j, nwin=nwin, **({"offset": off} if off else {}))
         for i, (scen, off) in enumerate([("S1", None), ("S2", 8.0), ("S3", None), ("S5", 8.0), ("S6", None)])
         for j, (heads, gq, nwin) in enumerate(BLOCK_CFGS) if not (scen == "S6" and nwin[0] == nwin[1])]

# vip_window_attn_fwd_h2 / _s32, vip_mhsa_fwd_h2 / _s32 (MFMA cores of attn_h2.hip, the fp32 VALU kernels of strict_ops.hip)
STRICT = [
    _s("window", "S1", ws=7, heads=2, global_q=False, seed=501, nwin=(1, 2)),
    _s("window", "S1", ws=14, heads=4, global_q=True, seed=502, nwin=(2, 1)),
    _s("window", "S3", ws=7, heads=4, global_q=True, seed=521),
    _s("window", "S3", ws=14, heads=2, global_q=False, seed=522),
    _s("mhsa", "S1", N=17, heads=1, seed=531), _s("mhsa", "S1", N=197, heads=3, seed=532), _s("mhsa", "S1", N=224, heads=1, seed=533),
    _s("mhsa", "S3", N=1, heads=1, seed=541), _s("mhsa", "S3", N=33, heads=3, seed=542), _s("mhsa", "S3", N=197, heads=1, seed=543),
]
# S2 / S5 for the strict kernels, compared over ALL elements at TOL_STRICT.  These kernels are given fp16-exact operands and keep q, k
# as they are, so conditioning() - an fp16 rounding of q and k - does not describe them; what limits them is fp32 logit arithmetic: one
# fp32 ulp of a logit near 600 is 6.1e-5 nats, and a plain fp32 evaluation (tests/emul_ops.py) is 3.8e-5 .. 1.2e-4 * max|ref| off there.
# STRICT_OFFSET_NATS is the largest power of two at which that plain fp32 evaluation stays within HALF of TOL_STRICT on these four
# cases (64: <= 9.2e-6; 128: 1.9e-5), asserted by test_attn_cases_cpu.py.  +64 still moves the maximum far from 0 and at -64 a padded key
# slot left at logit 0 outweighs the real keys by e^64.
STRICT_OFFSET_NATS = 64.0
STRICT_OFFSET = [
    _s("window", "S2", ws=7, heads=2, global_q=False, seed=511, offset=STRICT_OFFSET_NATS),
    _s("window", "S5", ws=14, heads=2, global_q=True, seed=512, offset=STRICT_OFFSET_NATS),
    _s("mhsa", "S2", N=33, heads=3, seed=513, offset=STRICT_OFFSET_NATS),
    _s("mhsa", "S5", N=197, heads=1, seed=514, offset=STRICT_OFFSET_NATS),
]
MIN_COMPARED = 0.75        # judge() fails a case of which conditioning() leaves less than this share of the designed elements


# ---- the expected-output rule (shared by the CPU emulation test and the GPU test) -------------------------------------------------
def judge(case, got, storage="f16"):
    """got: the kernel's (or an emulation's) output, any float dtype, on the CPU.  storage "f16" | "strict".
    Returns (ok, line): line = max error over the compared elements, max|ref|, exactness, the share of the designed elements that was
    compared and (reported only) the error over all of them - what the `[attn]` report lines carry.
      finite everywhere, always;
      S1 on an fp16 attention core: the designed elements equal v[pi(i)] bit for bit;
      S3 on an fp16 attention core: |got - ref64| <= 0.5 ulp16(ref64) + N 2^-23 max|v| per element;
      everything else: max error over the compared elements <= tol * max|ref| (tol = the kernel's own test's).  The fused block rounds
      q and k to fp16 itself, so there only well-conditioned elements (conditioning()) are compared - at least MIN_COMPARED of the
      designed ones, or the case fails.  The strict kernels keep their fp16-exact operands: every designed element is compared."""
    got = got.to(F64)
    ref = case.ref
    if got.shape != ref.shape:
        return False, f"shape {tuple(got.shape)} != {tuple(ref.shape)}"
    finite = bool(torch.isfinite(got).all())
    tol = TOL_STRICT if storage == "strict" else TOL_F16
    sel = case.designed.expand_as(ref).clone()
    kept = 1.0
    if case.kind == "block":
        well, _ = conditioning(case, tol)
        kept = (well & sel).sum().item() / sel.sum().item()
        sel &= well
    d = torch.where(sel & torch.isfinite(got), (got - ref).abs(), torch.zeros_like(ref))
    err, scale = d.max().item(), ref.abs().max().item() + 1e-6
    dall = torch.where(case.designed.expand_as(ref) & torch.isfinite(got), (got - ref).abs(), torch.zeros_like(ref)).max().item()
    exact = None
    if case.exact is not None:
        dsel = case.designed.expand_as(ref)
        exact = bool(torch.equal(got[dsel], case.exact.to(F64)[dsel]))
    core16 = case.kind != "block" and storage == "f16"
    if core16 and case.scen == "S1":
        ok, rule = exact, "bit-exact"
    elif core16 and case.scen == "S3":
        ok, rule = bool((d <= uniform_bound(case)).all()), "0.5 ulp16 + N 2^-23 max|v|"
        exact = bool(torch.equal(got.to(torch.float16), ref.to(torch.float16)))
    else:
        ok, rule = err <= tol * scale, f"{tol:g} * max|ref|"
    line = (f"{case.name}: max_abs_err={err:.3e} ref_absmax={scale:.3e} rel={err / scale:.3e} rule={rule} "
            f"exact={exact} compared={kept:.4f} rel_over_all_designed={dall / scale:.3e} finite={finite}")
    return bool(ok and finite and kept >= MIN_COMPARED), line
