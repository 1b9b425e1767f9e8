"""The grammar of a stress chain (``--stress-chain``, ``pipeline.apply_chain``): pure text handling, no torch and no library, so that
``main.py`` can refuse a bad chain before anything heavy is imported.  ``pipeline`` re-exports every name.

A chain is 2..8 steps joined by ``+``.  A step is exactly a single-variant label as ``ensemble.stress_labels`` prints it, with that
label's ranges, in that canonical spelling only, matched against the whole token:

    re-save      q<Q>                                   quality 1..100
    resize       r<P>                                   percent 10..400, not 100
    smoothing    b<TT>  m3  m5                          TT = ten times sigma, 03..50
    geometry     fliph  flipv  crop<PP>                 percent 50..99
                 rot<TTT>  rotm<TTT>                    ten times |degrees|, 001..450; m: negative
    colour       gray  bgr  hue<DDD>  huem<DDD>         |degrees| 001..180
                 sat<PPP>  con<PPP>                     percent 000..200, not 100
                 bri<PP>  brim<PP>                      |percent| 01..50
                 gam<PPP>                               100 times gamma, 050..200, not 100
    noise        n<TTT>  nm<TTT>                        ten times sigma, 005..500
                 spk<PP>                                percent 01..50
                 imp<TTT>                               ten times the percent, 001..500
    sharpening   shp<PPP>                               percent 001..500
    tone         ac<PP>  acl<PP>                        cutoff percent 00..49 (acl: one curve from the luma)
                 eq
                 clahe<TT>                              ten times the clip limit, 10..99

``parse_chain`` returns ``(kind, arg)`` per step: ``kind`` names the ``pipeline`` function (``recompress``, ``rescale``, ``blur``,
``median``, ``flip``, ``crop``, ``rotate``, ``gray``, ``bgr``, ``hue``, ``saturation``, ``contrast``, ``brightness``, ``gamma``,
``sharpen``) or, for the noise steps, the kind of ``pipeline.noise`` (``gaussian``, ``mono``, ``speckle``, ``impulse``) and, for the tone
steps, the mode of ``pipeline.tone`` (``autocontrast``, ``autocontrast_luma``, ``equalize``, ``clahe``); ``arg`` is that function's
argument in the user's units (None for ``gray``, ``bgr`` and ``equalize``)."""
import re
from typing import List, Optional, Sequence, Tuple

MIN_STEPS, MAX_STEPS, MAX_CHAINS = 2, 8, 16
NOISE_STEPS = ("gaussian", "mono", "speckle", "impulse")
TONE_STEPS = ("autocontrast", "autocontrast_luma", "equalize", "clahe")

# (pattern of the whole token, kind, lowest, highest, banned value, units per one of the argument, the family's own flag); a pattern's
# optional "m" group marks a negative value; scale None: the step has no number
_STEPS = (
    (r"q([1-9]\d{0,2})", "recompress", 1, 100, None, 1, "--stress-jpeg"),
    (r"r([1-9]\d{1,2})", "rescale", 10, 400, 100, 1, "--stress-resize"),
    (r"b(\d\d)", "blur", 3, 50, None, 10, "--stress-blur"),
    (r"m([35])", "median", 3, 5, None, 1, "--stress-median"),
    (r"flip([hv])", "flip", None, None, None, None, "--stress-flip"),
    (r"crop(\d\d)", "crop", 50, 99, None, 1, "--stress-crop"),
    (r"rot(m?)(\d{3})", "rotate", 1, 450, None, 10, "--stress-rotate"),
    (r"(gray)", "gray", None, None, None, None, "--stress-gray"),
    (r"(bgr)", "bgr", None, None, None, None, "--stress-bgr"),
    (r"hue(m?)(\d{3})", "hue", 1, 180, None, 1, "--stress-hue"),
    (r"sat(\d{3})", "saturation", 0, 200, 100, 1, "--stress-saturation"),
    (r"con(\d{3})", "contrast", 0, 200, 100, 1, "--stress-contrast"),
    (r"bri(m?)(\d\d)", "brightness", 1, 50, None, 1, "--stress-brightness"),
    (r"gam(\d{3})", "gamma", 50, 200, 100, 100, "--stress-gamma"),
    (r"n(\d{3})", "gaussian", 5, 500, None, 10, "--stress-noise"),
    (r"nm(\d{3})", "mono", 5, 500, None, 10, "--stress-noise-mono"),
    (r"spk(\d\d)", "speckle", 1, 50, None, 1, "--stress-speckle"),
    (r"imp(\d{3})", "impulse", 1, 500, None, 10, "--stress-impulse"),
    (r"shp(\d{3})", "sharpen", 1, 500, None, 1, "--stress-sharpen"),
    (r"ac(\d\d)", "autocontrast", 0, 49, None, 1, "--stress-autocontrast"),
    (r"acl(\d\d)", "autocontrast_luma", 0, 49, None, 1, "--stress-autocontrast-luma"),
    (r"(eq)", "equalize", None, None, None, None, "--stress-equalize"),
    (r"clahe(\d\d)", "clahe", 10, 99, None, 10, "--stress-clahe"),
)
STEP_FLAGS = {kind: flag for _, kind, _, _, _, _, flag in _STEPS}


def parse_step(token: str) -> Tuple[str, object]:
    """one step of a chain -> ``(kind, arg)``; ValueError naming the token when it is no canonical single-variant label in range"""
    for pattern, kind, lo, hi, banned, scale, _ in _STEPS:
        m = re.fullmatch(pattern, token, re.ASCII) if isinstance(token, str) else None
        if m is None:
            continue
        if scale is None:                                 # flip<axis>, gray, bgr, eq
            return kind, (m.group(1) if kind == "flip" else None)
        v = int(m.group(m.lastindex))
        if not lo <= v <= hi or v == banned:
            break
        v = -v if m.lastindex == 2 and m.group(1) else v
        return kind, (v if scale == 1 else v / scale)
    raise ValueError(f"chain step {token!r}: expected a single-variant stress label in its canonical spelling and range (q<Q>, r<P>, "
                     "b<TT>, m3, m5, fliph, flipv, crop<PP>, rot<TTT>, rotm<TTT>, gray, bgr, hue<DDD>, huem<DDD>, sat<PPP>, con<PPP>, "
                     "bri<PP>, brim<PP>, gam<PPP>, n<TTT>, nm<TTT>, spk<PP>, imp<TTT>, shp<PPP>, ac<PP>, acl<PP>, eq, clahe<TT>)")


def parse_chain(text: str) -> List[Tuple[str, object]]:
    """``STEP+STEP[+STEP...]`` -> the ``(kind, arg)`` of its 2..8 steps, left to right.  ValueError with the offending step for a token
    that is no step (an empty one included), for a one-step chain (naming the flag that gives that row), for more than 8 steps and for
    a chain whose ``r`` percents multiply to a size outside 10..400 % of the source's."""
    if not isinstance(text, str):
        raise ValueError(f"chain {text!r}: expected a string of steps joined by '+'")
    steps = [parse_step(token) for token in text.split("+")]
    if len(steps) < MIN_STEPS:
        raise ValueError(f"chain {text!r}: a chain has {MIN_STEPS}..{MAX_STEPS} steps; this single step is the row that "
                         f"{STEP_FLAGS[steps[0][0]]} gives")
    if len(steps) > MAX_STEPS:
        raise ValueError(f"chain {text!r}: {len(steps)} steps: a chain has {MIN_STEPS}..{MAX_STEPS}")
    scale, unit = 1, 1                                    # the product of the r percents over 100^k, in integers
    for kind, arg in steps:
        if kind == "rescale":
            scale, unit = scale * int(arg), unit * 100
            if not 10 * unit <= 100 * scale <= 400 * unit:
                raise ValueError(f"chain {text!r}: the resize steps up to r{arg} multiply to {100 * scale / unit:g} % of the source's "
                                 "size: expected 10..400 %")
    return steps


def parse_chains(text: str) -> List[str]:
    """``CHAIN[,CHAIN...]`` -> the chain texts in the order given, each checked by ``parse_chain``; at most 16, a chain listed twice is
    refused (ValueError)"""
    chains = text.split(",") if isinstance(text, str) else [None]
    for chain in chains:
        parse_chain(chain)
    if len(chains) > MAX_CHAINS:
        raise ValueError(f"chains {text!r}: {len(chains)} chains: at most {MAX_CHAINS} may be listed")
    twice = sorted({c for c in chains if chains.count(c) > 1})
    if twice:
        raise ValueError(f"chains {text!r}: chain {twice[0]!r} is listed twice")
    return chains


def chain_kinds(chains: Sequence[str]) -> set:
    """the step kinds that occur in ``chains`` (chain texts)"""
    return {kind for text in chains for kind, _ in parse_chain(text)}


def chain_noise_seeds(steps: Sequence[Tuple[str, object]], noise_seed: int = 0) -> List[Optional[int]]:
    """per step of a parsed chain the seed of its random field, None for a step that draws nothing: the k-th noise step (k = 0, 1, ...)
    uses ``(noise_seed + k) mod 2^32``, so a chain that starts with one noise step sees the field of that step's own row"""
    out, k = [], 0
    for kind, _ in steps:
        out.append((int(noise_seed) + k) & 0xFFFFFFFF if kind in NOISE_STEPS else None)
        k += kind in NOISE_STEPS
    return out
