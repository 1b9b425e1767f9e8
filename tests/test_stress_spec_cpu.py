"""CPU: the stress rows across all families at once - every single-variant label of ``ensemble.stress_labels`` is a step of the chain grammar
with the argument ``stress_batch`` uses, and the order, arguments and options of every ``pipeline`` call that ``stress_batch`` makes."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# keyword of stress_labels, step kind, lowest, highest and banned value in label units, label units per one of the argument, signed
NUMBERED = [("scales", "rescale", 10, 400, 100, 1, False), ("blurs", "blur", 3, 50, None, 10, False), ("medians", "median", 3, 5, 4, 1, False),
            ("crops", "crop", 50, 99, None, 1, False), ("rotations", "rotate", 1, 450, None, 10, True), ("hues", "hue", 1, 180, None, 1, True),
            ("saturations", "saturation", 0, 200, 100, 1, False), ("contrasts", "contrast", 0, 200, 100, 1, False),
            ("brightnesses", "brightness", 1, 50, None, 1, True), ("gammas", "gamma", 50, 200, 100, 100, False),
            ("noises", "gaussian", 5, 500, None, 10, False), ("mono_noises", "mono", 5, 500, None, 10, False),
            ("speckles", "speckle", 1, 50, None, 1, False), ("impulses", "impulse", 1, 500, None, 10, False),
            ("sharpens", "sharpen", 1, 500, None, 1, False), ("autocontrasts", "autocontrast", 0, 49, None, 1, False),
            ("autocontrast_lumas", "autocontrast_luma", 0, 49, None, 1, False), ("clahes", "clahe", 10, 99, None, 10, False)]


def _every_value():
    """``(stress_labels arguments, keywords, kind, argument)`` of every in-range value of the 23 step kinds"""
    for q in range(1, 101):
        yield ([q],), {}, "recompress", q
    for keyword, kind, lo, hi, banned, scale, signed in NUMBERED:
        for units in range(lo, hi + 1):
            for v in ((units, -units) if signed else (units,)):
                if units != banned:
                    arg = v if scale == 1 else v / scale
                    yield ([],), {keyword: [arg]}, kind, arg
    for axis in "hv":
        yield ([],), {"flips": [axis]}, "flip", axis
    for keyword, kind in (("gray", "gray"), ("bgr", "bgr"), ("equalize", "equalize")):
        yield ([],), {keyword: True}, kind, None


def test_every_single_variant_label_is_a_chain_step_with_the_same_argument():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import chain, ensemble
    n = 0
    for args, keywords, kind, arg in _every_value():
        labels = ensemble.stress_labels(*args, **keywords)
        assert len(labels) == 1, (keywords, labels)
        got_kind, got_arg = chain.parse_step(labels[0])
        assert (got_kind, got_arg) == (kind, arg) and type(got_arg) is type(arg), (labels[0], got_kind, got_arg, kind, arg)
        n += 1
    assert n == 4737


def test_step_label_is_the_inverse_of_parse_step():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import chain, ensemble
    for args, keywords, kind, arg in _every_value():
        label = ensemble.stress_labels(*args, **keywords)[0]
        assert chain.step_label(kind, arg) == label and chain.step_label(*chain.parse_step(label)) == label


# ---- the calls of stress_batch ------------------------------------------------------------------------------------------------------------------
def _traced(monkeypatch):
    """``pipeline``'s step functions and ``ensemble._score_batch`` replaced by recorders on fake batches; a fake batch's ``tag`` is the
    expression that made it, so a recorded call shows what it was applied to"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline
    trace = []
    keys, mean = torch.tensor([11, 22]), object()

    def fake(tag):
        b = object.__new__(pipeline.DecodedBatch)
        b.tag = tag
        return b

    def show(x):
        return "KEYS" if x is keys else "MEAN" if x is mean else repr(x)

    def recorder(name):
        def call(batch, *args):
            trace.append(f"{name}({', '.join([batch.tag] + [show(x) for x in args])})")
            return fake(trace[-1])
        return call

    for name in ("recompress", "rescale", "blur", "median", "flip", "crop", "rotate", "gray", "bgr", "hue", "saturation", "contrast", "brightness",
                 "gamma", "noise", "sharpen", "tone"):
        monkeypatch.setattr(pipeline, name, recorder(name))

    def noise_keys_device(batch, given=None):
        trace.append(f"noise_keys_device({batch.tag}, {given!r})")
        return keys

    def mean_colour(batch):
        trace.append(f"mean_colour({batch.tag})")
        return mean

    def score(batch, members, flags=None, after_fork=None):
        assert flags is None and members == MEMBERS
        trace.append(f"score({batch.tag})" + (" after_fork" if after_fork is not None else ""))
        return torch.full((1, 2), float(sum(t.startswith("score(") for t in trace) - 1))

    monkeypatch.setattr(pipeline, "noise_keys_device", noise_keys_device)
    monkeypatch.setattr(pipeline.DecodedBatch, "mean_colour", mean_colour)
    monkeypatch.setattr(ensemble, "_score_batch", score)
    return ensemble, fake("plain"), trace


MEMBERS = [("a member's spec", None)]                     # not resident: nothing asks for its dtype

EVERYTHING = dict(scales=[50, 200], blurs=[2.5, 0.5], medians=[3], flips=["v", "h"], crops=[60, 90], rotations=[7.5, -3], gray=True, bgr=True,
                  hues=[30, -30], saturations=[50], contrasts=[120], brightnesses=[-10], gammas=[0.8], noises=[3], mono_noises=[3],
                  speckles=[20], impulses=[1], sharpens=[150, 80], autocontrasts=[2], autocontrast_lumas=[1], equalize=True, clahes=[2],
                  chains=["n030+r50+q75", "r50+con120+nm030"],
                  subsampling="4:4:4", resize_filter="lanczos", blur_radius=2, crop_origin="topleft", rotate_fill="black", noise_seed=9,
                  noise_keys=[5, 6], sharpen_sigma=0.8, sharpen_radius=3, sharpen_threshold=4, clahe_grid=4)

# one line per row group, calls separated by ' | ': the call that makes a variant, its score, and for each quality its re-save and that score;
# a chain's steps and its one score
WANT = """
score(plain) after_fork
recompress(plain, 90, '4:4:4') | score(recompress(plain, 90, '4:4:4'))
recompress(plain, 70, '4:4:4') | score(recompress(plain, 70, '4:4:4'))
rescale(plain, 200, 'lanczos') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
rescale(plain, 50, 'lanczos') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
blur(plain, 0.5, 2) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
blur(plain, 2.5, 2) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
median(plain, 3) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
flip(plain, 'h') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
flip(plain, 'v') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
crop(plain, 90, 'topleft') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
crop(plain, 60, 'topleft') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
rotate(plain, -3.0, 'black') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
rotate(plain, 7.5, 'black') | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
mean_colour(plain)
gray(plain) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
bgr(plain) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
hue(plain, -30) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
hue(plain, 30) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
saturation(plain, 50) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
contrast(plain, 120, MEAN) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
brightness(plain, -10) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
gamma(plain, 0.8) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
noise_keys_device(plain, [5, 6])
noise(plain, 'gaussian', 3.0, 9, KEYS) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
noise(plain, 'mono', 3.0, 9, KEYS) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
noise(plain, 'speckle', 20, 9, KEYS) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
noise(plain, 'impulse', 1.0, 9, KEYS) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
sharpen(plain, 80, 0.8, 3, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
sharpen(plain, 150, 0.8, 3, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
tone(plain, 'autocontrast', 2, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
tone(plain, 'autocontrast_luma', 1, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
tone(plain, 'equalize', None, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
tone(plain, 'clahe', 2.0, 4) | score($) | recompress($, 90, '4:4:4') | score(@) | recompress($, 70, '4:4:4') | score(@)
noise(plain, 'gaussian', 3.0, 9, KEYS) | rescale(@, 50, 'lanczos') | recompress(@, 75, '4:4:4') | score(@)
rescale(plain, 50, 'lanczos') | contrast(@, 120) | noise(@, 'mono', 3.0, 9, KEYS) | score(@)
"""


def _calls(text):
    """the literal above as a list of calls: ``$`` stands for the first call on the line, ``@`` for the call just before"""
    out = []
    for line in text.strip().splitlines():
        first = len(out)
        for call in line.split(" | "):
            out.append(call.replace("$", out[first] if len(out) > first else "").replace("@", out[-1] if len(out) > first else ""))
    return out


def test_stress_batch_calls_in_row_order_with_every_option(monkeypatch):
    ensemble, plain, trace = _traced(monkeypatch)
    rows, labels = ensemble.stress_batch(plain, MEMBERS, [90, 70], after_fork=lambda: None, **EVERYTHING)
    assert trace == _calls(WANT), [(k, a, b) for k, (a, b) in enumerate(zip(trace, _calls(WANT))) if a != b][:3]
    assert trace.count("mean_colour(plain)") == 1 and trace.count("noise_keys_device(plain, [5, 6])") == 1
    assert not any(t.startswith("noise_keys_device") and t != "noise_keys_device(plain, [5, 6])" for t in trace)
    singles = ["r200", "r50", "b05", "b25", "m3", "fliph", "flipv", "crop90", "crop60", "rotm030", "rot075", "gray", "bgr", "huem030",
               "hue030", "sat050", "con120", "brim10", "gam080", "n030", "nm030", "spk20", "imp010", "shp080", "shp150", "ac02",
               "acl01", "eq", "clahe20"]
    assert labels == ["q90", "q70"] + [f"{v}{q}" for v in singles for q in ("", "_q90", "_q70")] + EVERYTHING["chains"]
    named = {k: v for k, v in EVERYTHING.items() if k not in ("subsampling", "resize_filter", "blur_radius")}
    assert labels == ensemble.stress_labels([90, 70], **{**named, "scales": [200, 50]})
    assert rows.shape == (1 + len(labels), 1, 2) and rows[:, 0, 0].tolist() == list(range(1 + len(labels)))      # row k is the k-th score


def test_stress_batch_with_qualities_alone_returns_the_rows(monkeypatch):
    ensemble, plain, trace = _traced(monkeypatch)
    rows = ensemble.stress_batch(plain, MEMBERS, [90, 70], "4:4:4")
    assert isinstance(rows, torch.Tensor) and rows.shape == (3, 1, 2)
    assert trace == ["score(plain)"] + _calls(WANT)[1:5]                      # no after_fork was given
    empty = {k: (False if isinstance(v, bool) else ()) for k, v in EVERYTHING.items() if isinstance(v, (list, bool)) and k != "noise_keys"}
    assert isinstance(ensemble.stress_batch(plain, MEMBERS, [90], **empty), torch.Tensor)
