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
    WebP re-save w<Q>                                   quality 1..100 (lossy WebP)

``parse_chain`` returns ``(kind, arg)`` per step: ``kind`` names the ``pipeline`` function (``recompress``, ``rescale``, ``blur``,
``median``, ``flip``, ``crop``, ``rotate``, ``gray``, ``bgr``, ``hue``, ``saturation``, ``contrast``, ``brightness``, ``gamma``,
``sharpen``, ``webp_recompress``) or, for the noise steps, the kind of ``pipeline.noise`` (``gaussian``, ``mono``, ``speckle``, ``impulse``) and, for the tone
steps, the mode of ``pipeline.tone`` (``autocontrast``, ``autocontrast_luma``, ``equalize``, ``clahe``); ``arg`` is that function's
argument in the user's units (None for ``gray``, ``bgr`` and ``equalize``)."""
import re
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

MIN_STEPS, MAX_STEPS, MAX_CHAINS = 2, 8, 16

# Everything that is particular to a step kind, one row per kind IN ROW ORDER: ``ensemble.stress_batch`` scores its variants kind by kind
# in the order of this table.
#   prefix, digits, signed   the label: the prefix, "m" for a negative value of a signed kind, the number in label units as that many
#                            digits (0: as it is, no leading zeros; None: the kind has no number)
#   lo, hi, banned           the range of the number's magnitude in label units, and the one value in it that is no step
#   scale                    label units per one of the argument (10: the label counts tenths)
#   flag                     the command-line flag that gives the kind's rows
#   keyword, order           the keyword of ``stress_batch`` / ``stress_labels`` that lists the kind's values (a bool for a kind without
#                            a number), and how a list is put in row order: "asc", "desc" ("h" before "v" is "asc"); ``recompress`` has
#                            no keyword of this kind: the qualities multiply the other rows and stay as given, the CLI lists them "desc"
#   family                   the word for the kind's family in the CLI's refusals; the flags of one family share their ``stress.json`` settings
Step = namedtuple("Step", "prefix digits signed kind lo hi banned scale flag keyword order family")
STEPS = {row.kind: row for row in (
    Step("q", 0, False, "recompress", 1, 100, None, 1, "--stress-jpeg", None, "desc", "recompression"),
    Step("r", 0, False, "rescale", 10, 400, 100, 1, "--stress-resize", "scales", "desc", "resize"),
    Step("b", 2, False, "blur", 3, 50, None, 10, "--stress-blur", "blurs", "asc", "smoothing"),
    Step("m", 1, False, "median", 3, 5, 4, 1, "--stress-median", "medians", "asc", "smoothing"),
    Step("flip", None, False, "flip", None, None, None, None, "--stress-flip", "flips", "asc", "geometric"),
    Step("crop", 2, False, "crop", 50, 99, None, 1, "--stress-crop", "crops", "desc", "geometric"),
    Step("rot", 3, True, "rotate", 1, 450, None, 10, "--stress-rotate", "rotations", "asc", "geometric"),
    Step("gray", None, False, "gray", None, None, None, None, "--stress-gray", "gray", None, "colour"),
    Step("bgr", None, False, "bgr", None, None, None, None, "--stress-bgr", "bgr", None, "colour"),
    Step("hue", 3, True, "hue", 1, 180, None, 1, "--stress-hue", "hues", "asc", "colour"),
    Step("sat", 3, False, "saturation", 0, 200, 100, 1, "--stress-saturation", "saturations", "asc", "colour"),
    Step("con", 3, False, "contrast", 0, 200, 100, 1, "--stress-contrast", "contrasts", "asc", "colour"),
    Step("bri", 2, True, "brightness", 1, 50, None, 1, "--stress-brightness", "brightnesses", "asc", "colour"),
    Step("gam", 3, False, "gamma", 50, 200, 100, 100, "--stress-gamma", "gammas", "asc", "colour"),
    Step("n", 3, False, "gaussian", 5, 500, None, 10, "--stress-noise", "noises", "asc", "noise"),
    Step("nm", 3, False, "mono", 5, 500, None, 10, "--stress-noise-mono", "mono_noises", "asc", "noise"),
    Step("spk", 2, False, "speckle", 1, 50, None, 1, "--stress-speckle", "speckles", "asc", "noise"),
    Step("imp", 3, False, "impulse", 1, 500, None, 10, "--stress-impulse", "impulses", "asc", "noise"),
    Step("shp", 3, False, "sharpen", 1, 500, None, 1, "--stress-sharpen", "sharpens", "asc", "sharpening"),
    Step("ac", 2, False, "autocontrast", 0, 49, None, 1, "--stress-autocontrast", "autocontrasts", "asc", "tone"),
    Step("acl", 2, False, "autocontrast_luma", 0, 49, None, 1, "--stress-autocontrast-luma", "autocontrast_lumas", "asc", "tone"),
    Step("eq", None, False, "equalize", None, None, None, None, "--stress-equalize", "equalize", None, "tone"),
    Step("clahe", 2, False, "clahe", 10, 99, None, 10, "--stress-clahe", "clahes", "asc", "tone"),
    Step("w", 0, False, "webp_recompress", 1, 100, None, 1, "--stress-webp", "webps", "desc", "recompression"),
)}
STEP_FLAGS = {kind: row.flag for kind, row in STEPS.items()}
NOISE_STEPS = tuple(kind for kind, row in STEPS.items() if row.family == "noise")
TONE_STEPS = tuple(kind for kind, row in STEPS.items() if row.family == "tone")


def step_units(kind: str, arg) -> int:
    """the number of a step's label: ``arg`` in label units (7.5 degrees -> 75); the signed integer that orders the kind's rows"""
    scale = STEPS[kind].scale
    return int(arg) if scale == 1 else int(round(float(arg) * scale))


def step_arg(kind: str, units: int):
    """the argument of the ``pipeline`` function for a number in label units: an int where the label counts ones, else a float"""
    scale = STEPS[kind].scale
    return units if scale == 1 else units / scale


def step_label(kind: str, arg=None) -> str:
    """``(kind, arg)`` -> the single-variant label: the inverse of ``parse_step``, and the only place that spells a label.  Formats what
    it is given: the ranges are ``parse_step``'s"""
    row = STEPS[kind]
    if row.digits is None:
        return row.prefix + (str(arg) if kind == "flip" else "")
    v = step_units(kind, arg)
    return f"{row.prefix}{'m' if row.signed and v < 0 else ''}{abs(v) if row.signed else v:0{row.digits}d}"


def _pattern(row: Step) -> str:
    if row.digits is None:
        return row.prefix + ("([hv])" if row.kind == "flip" else "")
    return row.prefix + ("(m?)" if row.signed else "()") + (rf"(\d{{{row.digits}}})" if row.digits else r"([1-9]\d{0,2})")


def parse_step(token: str) -> Tuple[str, object]:
    """one step of a chain -> ``(kind, arg)``; ValueError naming the token when it is no canonical single-variant label in range"""
    for kind, row in STEPS.items():
        m = re.fullmatch(_pattern(row), token, re.ASCII) if isinstance(token, str) else None
        if m is None:
            continue
        if row.digits is None:                            # flip<axis>, gray, bgr, eq
            return kind, (m.group(1) if kind == "flip" else None)
        v = int(m.group(2))
        if not row.lo <= v <= row.hi or v == row.banned:
            break
        return kind, step_arg(kind, -v if m.group(1) else v)
    raise ValueError(f"chain step {token!r}: expected a single-variant stress label in its canonical spelling and range (q<Q>, r<P>, "
                     "b<TT>, m3, m5, fliph, flipv, crop<PP>, rot<TTT>, rotm<TTT>, gray, bgr, hue<DDD>, huem<DDD>, sat<PPP>, con<PPP>, "
                     "bri<PP>, brim<PP>, gam<PPP>, n<TTT>, nm<TTT>, spk<PP>, imp<TTT>, shp<PPP>, ac<PP>, acl<PP>, eq, clahe<TT>, w<Q>)")


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
