"""Drop-in CLI for the reference entry point (main.py:151-235):

    python3 vip-cup-2022_amd/main.py <input.csv> <output.csv> [--scores-out scores.csv] [--synthetic] [--webp-lossy]
                                     [--heatmaps DIR [--heatmap-format npy|png] [--heatmap-members]]
                                     [--stress-jpeg Q[,Q...] --stress-out FILE.csv [--stress-subsampling 420|444]]
                                     [--stress-resize P[,P...] --stress-out FILE.csv [--stress-resize-filter bilinear|bicubic|lanczos]]
                                     [--stress-blur S[,S...] --stress-out FILE.csv [--stress-blur-radius R]]
                                     [--stress-median K[,K...] --stress-out FILE.csv]
                                     [--stress-flip h[,v] --stress-out FILE.csv]
                                     [--stress-crop P[,P...] --stress-out FILE.csv [--stress-crop-origin centre|topleft]]
                                     [--stress-rotate D[,D...] --stress-out FILE.csv [--stress-rotate-fill crop|mirror|black]]
                                     [--stress-gray] [--stress-bgr] [--stress-hue D[,D...]] [--stress-saturation P[,P...]]
                                     [--stress-contrast P[,P...]] [--stress-brightness P[,P...]] [--stress-gamma G[,G...]]   (--stress-out FILE.csv)
                                     [--stress-noise S[,S...]] [--stress-noise-mono S[,S...]] [--stress-speckle P[,P...]]
                                     [--stress-impulse P[,P...]] [--stress-noise-seed N]                                     (--stress-out FILE.csv)
                                     [--stress-sharpen P[,P...]] [--stress-sharpen-sigma S] [--stress-sharpen-radius R]
                                     [--stress-sharpen-threshold T]                                                          (--stress-out FILE.csv)
                                     [--stress-autocontrast C[,C...]] [--stress-autocontrast-luma C[,C...]] [--stress-equalize]
                                     [--stress-clahe L[,L...]] [--stress-clahe-grid G]                                       (--stress-out FILE.csv)
                                     [--stress-webp Q[,Q...] --stress-out FILE.csv]
                                     [--stress-chain STEP+STEP[+STEP...][,CHAIN...]]                                         (--stress-out FILE.csv)
                                     [--tiles-out FILE.csv [--tile-size 200] [--tile-stride S] [--tile-max 256] [--tile-agg mean|max]]
                                     [--occlusion DIR [--occlusion-grid 8] [--occlusion-window 2] [--occlusion-fill mean|gray]
                                                      [--occlusion-format npy|png] [--occlusion-members]]
    python -m torch.distributed.run --nproc-per-node N ... vip-cup-2022_amd/main.py in.csv out.csv

Same contract: the input CSV has a ``filename`` column with paths relative to the CSV's directory (main.py:77-79,
155-164); the output CSV has columns ``filename,logit`` with logit in {0.0, 1.0} = (ensemble mean > 0.487)
(main.py:143-145,225).  The files may be JPEG, PNG or lossless WebP in any mix; the format is picked from each file's first
bytes (animated WebP is refused, and so is lossy WebP unless ``--webp-lossy`` or ``VIP_WEBP_LOSSY=1`` turns its decoder on: VP8 key
frames, libwebp's pixels bit for bit; off by default).  ``--scores-out`` additionally writes the continuous ensemble mean (the reference keeps
it only in memory).  The ensemble manifest is ``ckpts/ckpts.json`` ([name, [H,W], idx],
main.py:171-198); members whose graph is not built yet are reported and skipped only under ``--allow-missing``.
``--heatmaps DIR`` additionally writes, per input file, the ensemble's Grad-CAM evidence map (``<name>.npy``: fp32 in [0, 1] at the
image's own size; or with ``--heatmap-format png`` a jet overlay ``<name>.png``), with ``--heatmap-members`` every member's
low-resolution map and peak in ``<name>.members.npz``, and ``heatmaps.json`` (per member: supported or why not).  The CSV outputs do
not change with the flag.
``--stress-jpeg 90,70,50 --stress-out stress.csv`` additionally scores every image as it would come back from a JPEG save at each listed
quality (dataset/augment.py:110-113 ``JpegCompress``; the decoded image is re-saved at its own size, before the members' resize, with
libjpeg's default 4:2:0 chroma or ``--stress-subsampling 444``) and writes, per input file, ``filename, p, decision, p_q<Q>...,
decision_q<Q>..., stable, flips_at`` (``flips_at``: the highest listed quality at which the decision differs from the unperturbed one) and
``stress.json`` with the per-quality flip counts, flip rates, mean |p_q - p| and the settings.  The CSV outputs do not change with the flag.
``--stress-resize 150,50 --stress-out stress.csv`` rescales every decoded image to each listed percent of its own size first (an antialiased
bicubic by default, ``--stress-resize-filter``; integer arithmetic and a uint8 result, what an image editor or an upload does) and scores
it unsaved (``r<P>``) and, with ``--stress-jpeg``, re-saved at every quality (``r<P>_q<Q>``): resized, then compressed, the way the
challenge's test images were made.  The table is then ``filename, p, decision, p_<label>..., decision_<label>..., stable, flips_at, flips``
over the labels ``q<Q>..., r<P>, r<P>_q<Q>...`` (``stable`` over all variants, ``flips_at`` over the 100 % rows as before, ``flips`` the
``;``-joined labels whose decision differs) and ``stress.json`` lists the labels under ``variants`` and keys its counts by label.
``--stress-blur 0.5,1,2.5 --stress-out stress.csv`` smooths every decoded image at its own size with a Gaussian of each listed sigma (pixels,
0.3..5.0 in steps of 0.1; cut off at three sigma, or at ``--stress-blur-radius``) and ``--stress-median 3,5`` with a 3 x 3 / 5 x 5 median -
the two filters of dataset/augment.py:131-140 ``Blur``, edges mirrored as there - and scores it unsaved (``b<TT>``, ``TT`` = ten times
sigma as two digits; ``m<K>``) and, with ``--stress-jpeg``, re-saved at every quality (``b<TT>_q<Q>``, ``m<K>_q<Q>``).  The rows follow
those of ``--stress-resize`` in the same table layout; smoothing is not combined with resizing.  ``stress.json`` then lists
``blur_sigmas``, ``blur_radius`` (null: three sigma) and ``medians`` under ``settings``.
``--stress-flip h,v``, ``--stress-crop 90,80`` and ``--stress-rotate -3,7.5`` (all with ``--stress-out stress.csv``) are the geometric
perturbations, dataset/augment.py:68-120 on the decoded image at its own size: mirrored left-right / top-bottom (``fliph``, ``flipv``),
cropped to each listed percent of its sides (50..99; ``crop<PP>``, largest first; from the middle, or with ``--stress-crop-origin
topleft`` from the corner, which keeps a JPEG source's 8 x 8 grid) and rotated counter-clockwise by each listed angle (degrees, non-zero,
-45..45 in steps of 0.1; ``rot<TTT>`` / ``rotm<TTT>`` for a negative angle, ``TTT`` = ten times the angle as three digits, ascending;
bilinear, then cut down to the largest upright rectangle inside the rotated image, or with ``--stress-rotate-fill mirror|black`` kept at
its size with the corners mirrored / black).  Each is scored unsaved and, with ``--stress-jpeg``, re-saved at every quality
(``<label>_q<Q>``); the rows follow those of ``--stress-median``.  Geometry is not combined with resizing or smoothing.  ``stress.json``
then lists ``flips``, ``crops``, ``crop_origin``, ``rotations`` and ``rotate_fill`` under ``settings``.  (A list that starts with a
negative angle is written ``--stress-rotate=-3,7.5``.)
``--stress-gray``, ``--stress-bgr``, ``--stress-hue -30,30``, ``--stress-saturation 0,50,150``, ``--stress-contrast 50,150``,
``--stress-brightness -10,10`` and ``--stress-gamma 0.8,1.25`` (all with ``--stress-out stress.csv``) are the colour perturbations,
dataset/augment.py:122-129 and :142-151 on the decoded image at its own size, per pixel and in integers: ``v = clamp((M (R, G, B) + K
mean + O + 32768) >> 16, 0, 255)`` with Q16 coefficients, then a 256-entry table.  ``gray``: Pillow's luma (19595 R + 38470 G + 7471 B)
in three channels; ``bgr``: red and blue exchanged; ``hue<DDD>`` / ``huem<DDD>``: the chroma rotated by a non-zero integer angle in
-180..180 degrees, as a rotation in the NTSC YIQ plane; ``sat<PPP>``: PPP % saturation (0..200, not 100), as a blend with the luma image -
both are the LINEAR forms, not ``tf.image``'s HSV round trip; ``con<PPP>``: PPP % contrast (0..200, not 100) about the image's own mean
colour, ``(x - mean) f + mean``; ``bri<PP>`` / ``brim<PP>``: PP % of full scale added (non-zero, -50..50); ``gam<PPP>``: ``255 (x / 255)
** g`` with PPP = 100 g, g in 0.50..2.00 with at most two decimals, not 1.  Each is scored unsaved and, with ``--stress-jpeg``, re-saved
at every quality (``<label>_q<Q>``); the rows follow those of ``--stress-rotate`` in this order, each list ascending.  Colour is not
combined with resizing, smoothing or geometry.  ``stress.json`` then lists ``gray``, ``bgr``, ``hues``, ``saturations``, ``contrasts``,
``brightnesses`` and ``gammas`` under ``settings``.  (A list that starts with a negative value is written ``--stress-hue=-30,30``.)
``--stress-noise 1,3,10``, ``--stress-noise-mono 3``, ``--stress-speckle 5,20`` and ``--stress-impulse 0.5,2`` (all with ``--stress-out
stress.csv``) are the noise perturbations - the reference has none - on the decoded image at its own size, per pixel and in integers:
``n<TTT>``: Gaussian noise of sigma = TTT / 10 levels (0.5..50.0 in steps of 0.1) on every channel independently, ``clamp(X + ((a z +
2^19) >> 20), 0, 255)`` with ``a = round(256 sigma)`` and z a Q12 standard normal; ``nm<TTT>``: one such sample on all three channels
(luminance noise); ``spk<PP>``: speckle, every sample times ``1 + PP / 100 z`` (integer percents 1..50); ``imp<TTT>``: TTT / 10 percent
of the pixels (0.1..50.0 in steps of 0.1) black or white.  The random words are Philox4x32-10 of the pixel's position under the key
(``--stress-noise-seed`` N, default 0; crc32 of the file's basename): a file gets the same noise at any place in the CSV, at any batch
size, on any rank, in every run, and all listed amounts see the same field at different gains.  Each is scored unsaved and, with
``--stress-jpeg``, re-saved at every quality (``<label>_q<Q>``); the rows follow those of the colour flags in this order, each list
ascending; a value listed twice is refused.  Noise is not combined with the other families.  ``stress.json`` then lists
``noise_sigmas``, ``noise_mono_sigmas``, ``speckles``, ``impulses`` and ``noise_seed`` under ``settings``.
``--stress-sharpen 80,150 --stress-out stress.csv`` is the sharpening perturbation - the unsharp mask a platform adds after a downscale; the
reference has none - on the decoded image at its own size, per byte and in integers: with ``B`` the Gaussian of ``--stress-blur`` at
``--stress-sharpen-sigma`` (0.3..5.0, default 1.0) and ``--stress-sharpen-radius`` (1..15, default three sigma), bit for bit, and ``d = X -
B``, a sample stays ``X`` where ``|d| <= T`` (``--stress-sharpen-threshold``, 0..255, default 0) and becomes ``clamp(X + ((a d + 128) >> 8),
0, 255)`` elsewhere, ``a = round(256 P / 100)``, P an integer percent in 1..500 - at most one level from ``round(X + P / 100 (X - B))``
clamped, one launch (Pillow's ``UnsharpMask`` blurs with a box approximation: close, not bit for bit).  ``shp<PPP>`` is scored unsaved and,
with ``--stress-jpeg``, re-saved at every quality (``shp<PPP>_q<Q>``); the rows follow those of the noise flags, ascending; a value listed
twice is refused.  Sharpening is not combined with the other families except through a chain.  ``stress.json`` then lists
``sharpen_percents``, ``sharpen_sigma``, ``sharpen_radius`` and ``sharpen_threshold`` under ``settings``.
``--stress-autocontrast 2 --stress-autocontrast-luma 2 --stress-equalize --stress-clahe 2,4 --stress-out stress.csv`` is the tone
perturbation - what a gallery's "auto", a messenger's "enhance" or a scanner does: a curve MEASURED from the picture's own histogram.
``ac<PP>`` is Pillow's ``ImageOps.autocontrast(cutoff=PP)`` per channel and ``acl<PP>`` its ``preserve_tone=True`` form (one curve from the
luma), cutoffs integer percents 0..49; ``eq`` is ``ImageOps.equalize``; all three bit for bit.  ``clahe<TT>`` (clip limits 1.0..9.9, ``TT`` =
ten times the limit) is contrast-limited adaptive equalisation of the luma on ``--stress-clahe-grid`` (1..16, default 8) tiles per axis
of at least 16 pixels, the tile tables blended bilinearly and the chroma kept, in integers (include/vipcup_hip.h).  Each variant is
three launches - histograms, tables, pixels - and nothing returns to the host.  The rows follow the sharpening rows in the order
``ac``, ``acl``, ``eq``, ``clahe``, each list ascending, unsaved and - with ``--stress-jpeg`` - re-saved (``<label>_q<Q>``); a value listed twice is
refused.  ``stress.json`` then lists ``autocontrast_cutoffs``, ``autocontrast_luma_cutoffs``, ``equalize``, ``clahe_limits`` and ``clahe_grid``
under ``settings``.
``--stress-webp 90,75,50 --stress-out stress.csv`` is the lossy WebP re-save - what CDNs and messengers transcode uploads to; the
reference has none: the decoded image at its own size goes through the project's own VP8 key-frame encoder on the GPU (libwebp's colour
conversion and quality curve; 4 x 4 transforms, 16 x 16 and 4 x 4 intra prediction chosen by prediction error, the in-loop filter, 4:2:0
chroma with the fancy upsampler; include/vipcup_hip.h states the rules) and comes back as libwebp would decode the file, bit for bit.
Qualities are integers in 1..100, highest first; a value listed twice is refused.  The rows ``w<Q>`` follow the tone rows, unsaved and -
with ``--stress-jpeg`` - re-saved as JPEG (``w<Q>_q<Q'>``).  The refusals are those of ``--stress-jpeg``.  ``stress.json`` then lists
``webp_qualities`` under ``settings`` (also when only a chain holds a ``w`` step).
``--stress-chain r50+shp080+q75,q90+crop95+q75 --stress-out stress.csv`` scores every image after a SEQUENCE of perturbations, as files
are laundered in practice (downscale, sharpen, re-save; a second JPEG on a shifted block grid).  A chain is 2..8 steps joined by ``+``;
up to 16 chains, separated by commas, keep the order given; a chain listed twice is refused.  A step is exactly a single-variant label
of the flags above in its canonical spelling and range, matched against the whole token: ``q<Q>``, ``r<P>``, ``b<TT>``, ``m3``, ``m5``,
``fliph``, ``flipv``, ``crop<PP>``, ``rot<TTT>``, ``rotm<TTT>``, ``gray``, ``bgr``, ``hue<DDD>``, ``huem<DDD>``, ``sat<PPP>``, ``con<PPP>``, ``bri<PP>``,
``brim<PP>``, ``gam<PPP>``, ``n<TTT>``, ``nm<TTT>``, ``spk<PP>``, ``imp<TTT>``, ``shp<PPP>``, ``ac<PP>``, ``acl<PP>``, ``eq``, ``clahe<TT>``, ``w<Q>``; a one-step chain is refused with the name of the
flag that gives that row; the ``r`` percents of a chain must multiply to 10..400 %.  The steps run left to right on the decoded image
at its own size, each with the options of its family's flags (``--stress-subsampling`` for ``q``, ``--stress-resize-filter`` for ``r``,
``--stress-blur-radius`` for ``b``, ``--stress-crop-origin`` for ``crop``, ``--stress-rotate-fill`` for ``rot``, ``--stress-sharpen-sigma`` /
``-radius`` / ``-threshold`` for ``shp``, ``--stress-noise-seed`` for the noise steps, ``--stress-clahe-grid`` for ``clahe``), which are accepted when a chain holds the step they
govern.  A ``con`` step takes the mean colour, and a tone step the histogram, of the image as it reaches that step; the k-th noise step of a chain draws from seed + k on
the image as it reaches that step, so ``n030+q75`` sees the field of the row ``n030``.  The result is scored once, as written:
``--stress-jpeg`` does not multiply chain rows.  The chain rows come last under the chain's text (``p_<chain>``, ``decision_<chain>``), count
for ``stable`` and ``flips`` and not for ``flips_at``; ``stress.json`` keys them by label and lists ``chains`` under ``settings``.  C chains
cost C plain runs.
``--tiles-out tiles.csv`` additionally scores every image that is at least ``--tile-size`` (200) pixels high and wide at its own resolution:
it is cut into ``tile x tile`` crops - ``--tile-stride`` apart at most (default: the tile size), spread so that the first starts at 0 and the
last ends at the image's edge, at most ``--tile-max`` per image (beyond that the grid is an evenly spaced sample with gaps) - and each
crop goes through the members as a 200 x 200 file would (dataset/dataset.py:31-38 on the crop).  ``tiles.csv`` holds, per input file,
``filename, width, height, tiles, grid`` (``<rows>x<columns>``; ``0x0`` for a file that is smaller than a tile, or exactly one tile),
``p, decision`` (the plain run), ``p_tiles_mean, p_tiles_max, frac_tiles`` (the ensemble's tile scores: mean, max, fraction above the
threshold), ``decision_tiles`` (``--tile-agg`` of them ``> 0.487``; the plain decision for an untiled file) and ``agrees``; ``tiles.json`` the
settings, the counts of tiled and untiled files, the files that disagree and the files whose grid ``--tile-max`` thinned; and, with
one rank, ``tiles.tiles.csv`` every tile: ``filename, ty, tx, y0, x0, p`` and one column per member.  The CSV outputs do not change with
the flag.
``--occlusion DIR`` additionally asks which part of each image the verdict depends on: the image is divided into ``--occlusion-grid`` (8) x
8 cells (cell g of an axis of length L = pixels ``(g L) // G .. ((g + 1) L) // G - 1``) and scored again with every window of
``--occlusion-window`` (2) x 2 cells hidden behind the image's own mean colour (``--occlusion-fill gray``: 128, 128, 128) - 49 variants at
the defaults, each through the members' ordinary input path.  Per input file ``DIR/<name>.npy`` holds the ensemble's map at the image's
own size, fp32, in units of delta-p: every pixel carries the mean of ``p - p_variant`` over the windows that cover its cell, positive
where hiding the region lowers the synthetic score (``--occlusion-format png``: ``<name>.png`` instead, the map scaled to the image's
largest ``|value|`` around 128 = no effect, through the jet table, blended over the image, alpha 0.4); with ``--occlusion-members``
``<name>.members.npz`` every member's (and the ensemble's) ``[G, G]`` cells, plain score and per-variant scores, plus the variants'
pixel rectangles.  It needs no gradients, so the ViT members have maps too.  ``DIR/occlusion.csv`` holds, per input file, ``filename,
width, height, variants, p, decision, delta_max, delta_min, cell_max`` (``gy,gx``: the first cell of the window with the largest delta-p)
and ``flips`` (variants whose decision differs); ``DIR/occlusion.json`` the settings, the counts, the skipped files (lower or narrower
than the grid: no variants, empty columns) and the files with ``flips > 0``.  A run costs 1 plain run plus ``(G - K + 1)^2`` member
passes per image.  The CSV outputs do not change with the flag.

Checkpoints: ``<script dir>/ckpts/<name>/ckpt/*.h5`` (Keras weight / model files, as in the reference), else ``ckpt/saved_model.pb`` (a
Keras SavedModel directory: its variables are read by ``tfbundle``), or ``*.npz`` (a flat dict of
Keras-named arrays), one file per fold.
The reference ships none (README.md:13) and raises when a directory is empty (main.py:194); so does this CLI,
unless ``--synthetic`` asks for the seeded synthetic checkpoints.
"""
import argparse
import inspect
import json
import os
import re
import sys
import time
from collections import namedtuple
from glob import glob

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vipcup_amd import chain as grammar  # noqa: E402  (text handling only: nothing heavy is imported)


def _heatmap_writer(a, names, members, rank):
    """the ``batch_scorer`` of ``--heatmaps``: ``explain_batch`` on every batch, the files of its images written as they come (under
    ``--shard images`` a rank only ever sees its own images: nothing is exchanged), the scores handed on unchanged"""
    from vipcup_amd import cam, ensemble, ops
    os.makedirs(a.heatmaps, exist_ok=True)
    why = ensemble.cam_support(members)
    if rank == 0:
        with open(os.path.join(a.heatmaps, "heatmaps.json"), "w") as f:
            json.dump({"target": "score", "format": a.heatmap_format, "alpha": 0.4 if a.heatmap_format == "png" else None,
                       "members": [{"name": spec.name, "cam_supported": why[spec.name] is None, "reason": why[spec.name]}
                                   for spec, _ in members]}, f, indent=1)
    if all(v is not None for v in why.values()):
        raise SystemExit("vipcup_amd main: --heatmaps: no member of this ensemble can produce an evidence map: "
                         + "; ".join(f"{k}: {v}" for k, v in why.items()))

    def score(staged, sub, b0, b1, after_fork):
        ex = ensemble.explain_batch(staged, sub, target="score", out="u8" if a.heatmap_format == "png" else "f32", after_fork=after_fork)
        sizes = ex.batch.sizes_host
        if a.heatmap_format == "png":
            full = ops.cam_overlay(ex.batch.rgb, ex.map, cam.jet_table_device(ex.map.device), 0.4).cpu().numpy()
        else:
            full = ex.map.cpu().numpy()
        low = None
        if a.heatmap_members:
            low = [(n, m, p) for n, m, p in zip(ex.names, ex.maps, ex.peaks) if m is not None]
            low = [(n, [t.cpu().numpy() for t in (m if isinstance(m, (list, tuple)) else [m])],
                    [t.cpu().numpy() for t in (p if isinstance(p, (list, tuple)) else [p])]) for n, m, p in low]
        for i in range(b1 - b0):
            h, w = sizes[i]
            stem = os.path.join(a.heatmaps, cam.heatmap_stem(names[b0 + i]))
            if a.heatmap_format == "png":
                cam.write_png(stem + ".png", full[i, :h, :w])
            else:
                np.save(stem + ".npy", np.ascontiguousarray(full[i, :h, :w]))
            if low is not None:
                arrays = {}
                for n, ms, ps in low:
                    for k, (m, p) in enumerate(zip(ms, ps)):
                        key = n if len(ms) == 1 else f"{n}/fold{k}"
                        arrays[key + "/cam"], arrays[key + "/peak"] = m[i], p[i]
                np.savez(stem + ".members.npz", **arrays)
        return ex.scores
    return score


# ---- the --stress-* flags ------------------------------------------------------------------------------------------------------------------
# A step kind's label, range, keyword, row order and family are rows of ``chain.STEPS``; what is left for the CLI is per kind, in ``_LISTS``:
# the syntax of a list token (None: whatever ``int()`` reads), what becomes of a value listed twice (ONCE: the list is refused; DROP: the
# copies go; DROP_BANNED: so does the one value that is no step, without a word), the refusal's words for what a list holds, and the key
# of the list in ``stress.json``'s settings.  The switches (--stress-gray, --stress-bgr, --stress-equalize) are stored under their keyword.
DROP, DROP_BANNED, ONCE = "drop", "drop, the banned value too", "once"
_TENTHS, _PERCENT = r"\d{1,2}(\.\d)?", r"-?\d{1,3}"
_List = namedtuple("_List", "syntax twice expected setting")
_LISTS = {kind: _List(*row) for kind, row in {
    "recompress": (None, DROP, "integer qualities in 1..100", "qualities"),
    "rescale": (None, DROP_BANNED, "integer percents in 10..400", "scales"),
    "blur": (_TENTHS, DROP, "sigmas in 0.3..5.0 with at most one fractional digit", "blur_sigmas"),
    "median": (None, DROP, "windows, each 3 or 5", "medians"),
    "flip": (r"[hv]", DROP, None, "flips"),
    "crop": (None, DROP, "integer percents in 50..99", "crops"),
    "rotate": ("-?" + _TENTHS, DROP, "non-zero angles in -45..45 with at most one fractional digit", "rotations"),
    "hue": (_PERCENT, DROP, "non-zero integer degrees in -180..180", "hues"),
    "saturation": (_PERCENT, DROP, "integer percents in 0..200 other than 100", "saturations"),
    "contrast": (_PERCENT, DROP, "integer percents in 0..200 other than 100", "contrasts"),
    "brightness": (_PERCENT, DROP, "non-zero integer percents in -50..50", "brightnesses"),
    "gamma": (r"\d(\.\d{1,2})?", DROP, "decimals in 0.50..2.00 with at most two fractional digits, other than 1", "gammas"),
    "gaussian": (_TENTHS, ONCE, "sigmas in 0.5..50.0 with at most one fractional digit", "noise_sigmas"),
    "mono": (_TENTHS, ONCE, "sigmas in 0.5..50.0 with at most one fractional digit", "noise_mono_sigmas"),
    "speckle": (r"\d{1,2}", ONCE, "integer percents in 1..50", "speckles"),
    "impulse": (_TENTHS, ONCE, "percents in 0.1..50.0 with at most one fractional digit", "impulses"),
    "sharpen": (r"\d{1,3}", ONCE, "integer percents in 1..500", "sharpen_percents"),
    "autocontrast": (r"\d{1,2}", ONCE, "integer cutoff percents in 0..49", "autocontrast_cutoffs"),
    "autocontrast_luma": (r"\d{1,2}", ONCE, "integer cutoff percents in 0..49", "autocontrast_luma_cutoffs"),
    "clahe": (_TENTHS, ONCE, "clip limits in 1.0..9.9 with at most one fractional digit", "clahe_limits"),
    "webp_recompress": (None, ONCE, "integer qualities in 1..100", "webp_qualities"),
}.items()}
# An option flag: its keyword of ``stress_batch``, the step kind whose flag it is read after (and written after, in the settings), the kinds
# it governs - it is accepted with the flag of one of them or with a chain that holds one -, the refusal otherwise, its integer range
# and the value that stands for "not given".
_SHARPEN_NEEDS = ("--stress-sharpen-sigma / --stress-sharpen-radius / --stress-sharpen-threshold need --stress-sharpen P[,P...] or a "
                  "--stress-chain with a shp step")
_Option = namedtuple("_Option", "flag keyword after kinds needs lo hi unset")
_OPTIONS = tuple(_Option(*row) for row in (
    ("--stress-resize-filter", "resize_filter", "rescale", ("rescale",), "--stress-resize-filter needs --stress-resize P[,P...]", None, None, None),
    ("--stress-blur-radius", "blur_radius", "blur", ("blur",), "--stress-blur-radius needs --stress-blur S[,S...]", 1, 15, None),
    ("--stress-crop-origin", "crop_origin", "crop", ("crop",), "--stress-crop-origin needs --stress-crop P[,P...]", None, None, None),
    ("--stress-rotate-fill", "rotate_fill", "rotate", ("rotate",), "--stress-rotate-fill needs --stress-rotate D[,D...]", None, None, None),
    ("--stress-noise-seed", "noise_seed", "impulse", grammar.NOISE_STEPS,
     "--stress-noise-seed needs --stress-noise, --stress-noise-mono, --stress-speckle or --stress-impulse", 0, 0xFFFFFFFF, None),
    ("--stress-sharpen-sigma", "sharpen_sigma", "sharpen", ("sharpen",), _SHARPEN_NEEDS, None, None, 1.0),
    ("--stress-sharpen-radius", "sharpen_radius", "sharpen", ("sharpen",), _SHARPEN_NEEDS, 1, 15, None),
    ("--stress-sharpen-threshold", "sharpen_threshold", "sharpen", ("sharpen",), _SHARPEN_NEEDS, 0, 255, 0),
    ("--stress-clahe-grid", "clahe_grid", "clahe", ("clahe",),
     "--stress-clahe-grid needs --stress-clahe L[,L...] or a --stress-chain with a clahe step", 1, 16, 8),
))
# the options a chain's steps add to the settings when the family whose flags carry them is absent, in the order these keys have always had
_CHAIN_SETTINGS = ("crop_origin", "rotate_fill", "noise_seed", "clahe_grid", "resize_filter", "blur_radius")


def _dest(flag):
    return flag[2:].replace("-", "_")


def _units(token, syntax, scale):
    """a token of a list in label units (``2.5`` at 10 units per one -> 25); None when it is not in the flag's syntax"""
    if syntax is None:
        try:
            return int(token)
        except ValueError:
            return None
    if not re.fullmatch(syntax, token):
        return None
    whole, _, frac = token.lstrip("-").partition(".")
    v = int(whole) * scale + int((frac + "00")[:len(str(scale)) - 1] or 0)
    return -v if token[0] == "-" else v


def _stress_list(kind, text):
    """the values of one ``--stress-*`` list as ``stress_batch`` takes them, in row order; the range is ``chain.STEPS``'s"""
    row, (syntax, twice, expected, _) = grammar.STEPS[kind], _LISTS[kind]
    tokens = text.split(",")
    if kind == "flip":
        if not all(re.fullmatch(syntax, t) for t in tokens):
            raise SystemExit(f"vipcup_amd main: {row.flag} {text!r}: expected h, v or h,v")
        return sorted(set(tokens))
    units = [_units(t, syntax, row.scale) for t in tokens]
    bad = None in units or not all(row.lo <= (abs(v) if row.signed else v) <= row.hi for v in units)
    if twice == ONCE:
        bad = bad or len(set(units)) != len(units)
    elif twice == DROP_BANNED:
        units = [v for v in units if v != row.banned]
    if bad or row.banned in units:
        raise SystemExit(f"vipcup_amd main: {row.flag} {text!r}: expected a comma-separated list of {expected}"
                         + (", each listed once" if twice == ONCE else ""))
    if not units:
        raise SystemExit(f"vipcup_amd main: {row.flag} {text!r}: nothing left after dropping {row.banned} (the unperturbed row)")
    return [grammar.step_arg(kind, v) for v in sorted(units if twice == ONCE else set(units), reverse=row.order == "desc")]


def _stress_option(option, value, default, present):
    """the value of an option flag for ``stress_batch``; ``present``: the step kinds of this run's flags and chains"""
    flag, lo, hi = option.flag, option.lo, option.hi
    if value != default:
        if not present & set(option.kinds):
            raise SystemExit("vipcup_amd main: " + option.needs)
        if option.keyword == "sharpen_sigma":                   # a decimal: the sigmas of --stress-blur
            blur = grammar.STEPS["blur"]
            units = _units(value, _TENTHS, blur.scale)
            if units is None or not blur.lo <= units <= blur.hi:
                raise SystemExit(f"vipcup_amd main: {flag} {value!r}: expected a sigma in 0.3..5.0 with at most one fractional digit")
            return grammar.step_arg("blur", units)
        if lo is not None and not lo <= value <= hi:
            raise SystemExit(f"vipcup_amd main: {flag} {value}: expected an integer in {lo}..{hi}")
    return option.unset if value is None else value


def _refuse_context(a, flag, family):
    """what every stress flag asks of the run: --stress-out, --shard images and --tta 1, no --heatmaps"""
    if a.stress_out is None:
        raise SystemExit(f"vipcup_amd main: {flag} needs --stress-out FILE.csv")
    if a.shard != "images" or a.tta > 1:
        # the scores of one image would be spread over ranks (members / hybrid) or over augmented copies (TTA): not built
        one = family in ("recompression", "resize")
        raise SystemExit(f"vipcup_amd main: {flag} works with --shard images and --tta 1 only (got --shard {a.shard} --tta {a.tta}): "
                         f"the {family} stress test{'' if one else 's'} under member sharding or TTA {'is' if one else 'are'} not implemented")
    if a.heatmaps is not None:
        raise SystemExit(f"vipcup_amd main: {flag} and --heatmaps cannot be combined (both replace the batch scorer): "
                         "run them one after the other")


def _stress_labels(spec):
    """the labels of the rows that ``spec`` (the keywords of ``stress_batch``) asks for"""
    from vipcup_amd import ensemble
    return ensemble.stress_labels(**{k: v for k, v in spec.items() if k in inspect.signature(ensemble.stress_labels).parameters})


def _stress_scorer(spec, names, kept):
    """the ``batch_scorer`` of the ``--stress-*`` flags: ``stress_batch`` with ``spec``, the run's keywords, on every batch (every batch's
    ``noise_keys`` come from its files' ``names``: by file, not by batch position); the unperturbed row is handed on unchanged, the rows
    of the perturbed batches ``[V, M, n]`` stay on this rank (``kept``, in batch order) until the run's one extra collective"""
    from vipcup_amd import ensemble, pipeline

    def score(staged, sub, b0, b1, after_fork):
        rows = ensemble.stress_batch(staged, sub, after_fork=after_fork, noise_keys=pipeline.noise_keys(names[b0:b1]), **spec)
        rows = rows[0] if isinstance(rows, tuple) else rows      # (rows, labels) with any variant but the qualities
        kept.append(rows[1:])
        return rows[0]
    return score


def _write_stress(a, names, members, per_model, stressed, spec, mode):
    """``--stress-out``: the per-file table as CSV and, next to it, the summary and settings as JSON"""
    import pandas as pd
    from vipcup_amd import ensemble
    scores = np.concatenate([per_model[None].astype(np.float32), stressed.astype(np.float32)], axis=0)
    qualities, labels = spec["qualities"], _stress_labels(spec)
    mixed = len(labels) > len(qualities)
    table, summary = ensemble.stress_table(names, scores, labels if mixed else qualities)
    cols = {"filename": table["filename"], "p": table["p"], "decision": table["decision"]}
    for k, v in enumerate(labels):
        cols[f"p_{v}"] = table["p_q"][:, k]
    for k, v in enumerate(labels):
        cols[f"decision_{v}"] = table["decision_q"][:, k]
    cols["stable"] = table["stable"].astype(np.int64)
    cols["flips_at"] = ["" if q is None else str(q) for q in table["flips_at"]]
    if mixed:
        cols["flips"] = table["flips"]
    pd.DataFrame(cols).to_csv(a.stress_out, index=False)
    settings = {"qualities": list(qualities), "subsampling": spec["subsampling"], "threshold": ensemble.THR, "precision": mode,
                "batch_size": a.batch_size, "n_images": len(names), "members": [member.name for member, _ in members]}
    in_chain = grammar.chain_kinds(spec.get("chains", ()))
    rows = [row for kind, row in grammar.STEPS.items() if kind != "recompress"]
    # a family with one of its flags given writes all its lists (empty ones too) and options; sharpening also with a shp step in a chain
    present = {row.family for row in rows if row.keyword in spec} | ({"sharpening"} if "sharpen" in in_chain else set())
    if "webp_recompress" in in_chain:                   # the WebP re-save shares its family with --stress-jpeg, whose settings stand above
        present.add("recompression")
    for row in rows:
        if row.family in present:
            if row.kind in _LISTS:
                settings[_LISTS[row.kind].setting] = spec.get(row.keyword, [])
            else:
                settings[row.keyword] = spec.get(row.keyword, False)
            settings.update({option.keyword: spec[option.keyword] for option in _OPTIONS if option.after == row.kind})
    if "chains" in spec:
        settings["chains"] = list(spec["chains"])
        for key in _CHAIN_SETTINGS:                     # the options of chain steps whose family's flags are absent
            family = next(grammar.STEPS[option.after].family for option in _OPTIONS if option.keyword == key)
            governed = {kind for option in _OPTIONS if grammar.STEPS[option.after].family == family for kind in option.kinds}
            if family not in present and in_chain & governed:
                settings[key] = spec[key]
    summary["settings"] = settings
    with open(os.path.splitext(a.stress_out)[0] + ".json", "w") as f:
        json.dump(summary, f, indent=1)


def _tile_scorer(a, kept, kept_tiles):
    """the ``batch_scorer`` of ``--tiles-out``: ``tile_batch`` on every batch; the plain rows are handed on unchanged, the per-image
    aggregates ``[3, M + 1, n]`` plus two rows holding every image's height and width stay on this rank (``kept``, in batch order) until
    the run's one extra collective, and so do the per-tile scores ``[M + 1, T]`` (``kept_tiles``), which are only written with one rank"""
    import torch
    from vipcup_amd import ensemble

    def score(staged, sub, b0, b1, after_fork):
        plain, tiles, agg, plan = ensemble.tile_batch(staged, sub, a.tile_size, a.tile_stride, a.tile_max, after_fork=after_fork)
        hw = torch.tensor(plan.sizes, dtype=torch.float32, device=agg.device).t()          # [2, n]: exact in fp32 (sides < 2^24)
        kept.append(torch.cat([agg, hw[:, None, :].expand(2, agg.shape[1], agg.shape[2])], dim=0))
        kept_tiles.append(tiles)
        return plain
    return score


def _write_tiles(a, names, members, per_model, rows, tiles, mode, world):
    """``--tiles-out``: the per-file table as CSV, the summary and settings as JSON next to it and, with one rank, the long form"""
    import pandas as pd
    from vipcup_amd import ensemble, pipeline
    sizes = [(int(h), int(w)) for h, w in zip(rows[3, 0], rows[4, 0])]
    plan = pipeline.tile_plan(sizes, a.tile_size, a.tile_stride, a.tile_max)         # a function of the sizes alone: every rank's plans again
    table, summary = ensemble.tile_table(names, per_model, rows[:3], plan, ensemble.THR, a.tile_agg)
    table["agrees"] = table["agrees"].astype(np.int64)
    pd.DataFrame(table).to_csv(a.tiles_out, index=False)
    stem = os.path.splitext(a.tiles_out)[0]
    long_form = stem + ".tiles.csv" if world == 1 else None
    summary["settings"] = {"tile": plan.tile, "stride": plan.stride, "max_tiles": plan.max_tiles, "tile_agg": a.tile_agg,
                           "threshold": ensemble.THR, "precision": mode, "batch_size": a.batch_size, "n_images": len(names),
                           "members": [spec.name for spec, _ in members]}
    summary["tiles_file"] = None if long_form is None else os.path.basename(long_form)
    if long_form is None:
        summary["tiles_file_skipped"] = f"the per-tile scores stay on the rank that computed them: written with one rank only (got {world})"
    with open(stem + ".json", "w") as f:
        json.dump(summary, f, indent=1)
    if long_form is not None:
        tab = plan.tab
        assert tiles.shape == (len(members) + 1, tab.shape[0]), (tiles.shape, tab.shape)
        nx = np.array([max(plan.grids[i][1], 1) for i in tab[:, 0]], dtype=np.int64)
        k = np.arange(tab.shape[0]) - plan.seg[tab[:, 0]]
        cols = {"filename": [names[i] for i in tab[:, 0]], "ty": k // nx, "tx": k % nx, "y0": tab[:, 1], "x0": tab[:, 2], "p": tiles[-1]}
        for (spec, _), row in zip(members, tiles):
            cols[spec.name] = row
        pd.DataFrame(cols).to_csv(long_form, index=False)


def _occlusion_scorer(a, names, members, kept):
    """the ``batch_scorer`` of ``--occlusion``: ``occlusion_batch`` on every batch, the files of its images written as they come (under
    ``--shard images`` a rank only ever sees its own images); the plain rows are handed on unchanged, the per-image statistics
    ``[4, M + 1, n]`` plus two rows holding every image's height and width stay on this rank (``kept``, in batch order) until the run's one
    extra collective"""
    import torch
    from vipcup_amd import cam, ensemble, ops, pipeline
    os.makedirs(a.occlusion, exist_ok=True)
    png = a.occlusion_format == "png"

    def score(staged, sub, b0, b1, after_fork):
        batch = staged if isinstance(staged, pipeline.DecodedBatch) else pipeline.decode_staged(staged)     # the read-ahead may have decoded it
        # chunks of the run's own batch size: a member pass over variants then has the shape of a plain pass
        plain, variants, cells, stats, plan = ensemble.occlusion_batch(batch, sub, a.occlusion_grid, a.occlusion_window, a.occlusion_fill,
                                                                       chunk=min(max(a.batch_size, 1), 65535), after_fork=after_fork)
        full = ops.occlusion_map(cells[-1], batch.sizes, batch.rgb.shape[1:3], out="u8" if png else "f32")
        if png:
            rgb = batch.rgb if batch.rgb.is_contiguous() else batch.rgb.contiguous()
            full = ops.cam_overlay(rgb, full, cam.jet_table_device(full.device), 0.4)
        full = full.cpu().numpy()
        hw = torch.tensor(plan.sizes, dtype=torch.float32, device=stats.device).t()        # [2, n]: exact in fp32 (sides < 2^24)
        kept.append(torch.cat([stats.permute(2, 0, 1), hw[:, None, :].expand(2, stats.shape[0], stats.shape[1])], dim=0))
        if a.occlusion_members:
            cells_h, variants_h = cells.cpu().numpy(), variants.cpu().numpy()
            plain_h = (plain.cpu().numpy(), ops.ensemble_mean(plain).cpu().numpy())
        for i in range(b1 - b0):
            h, w = plan.sizes[i]
            stem = os.path.join(a.occlusion, cam.heatmap_stem(names[b0 + i]))
            if png:
                cam.write_png(stem + ".png", full[i, :h, :w])
            else:
                np.save(stem + ".npy", np.ascontiguousarray(full[i, :h, :w]))
            if a.occlusion_members:
                lo, hi = int(plan.seg[i]), int(plan.seg[i + 1])
                arrays = {"rects": plan.tab[lo:hi, 1:5]}
                for m, key in enumerate([spec.name for spec, _ in sub] + ["ensemble"]):
                    arrays[key + "/cells"], arrays[key + "/variants"] = cells_h[m, i], variants_h[m, lo:hi]
                    arrays[key + "/p"] = plain_h[0][m, i] if m < len(sub) else plain_h[1][i]
                np.savez(stem + ".members.npz", **arrays)
        return plain
    return score


def _write_occlusion(a, names, members, per_model, rows, mode):
    """``--occlusion``: the per-file table ``DIR/occlusion.csv`` and the summary and settings ``DIR/occlusion.json``"""
    import pandas as pd
    from vipcup_amd import ensemble, pipeline
    sizes = [(int(h), int(w)) for h, w in zip(rows[4, 0], rows[5, 0])]
    plan = pipeline.occlusion_plan(sizes, a.occlusion_grid, a.occlusion_window)     # a function of the sizes alone: every rank's plans again
    table, summary = ensemble.occlusion_table(names, per_model, np.ascontiguousarray(rows[:4].transpose(1, 2, 0)), plan, ensemble.THR)
    pd.DataFrame(table).to_csv(os.path.join(a.occlusion, "occlusion.csv"), index=False)
    summary["settings"] = {"grid": plan.grid, "window": plan.window, "fill": a.occlusion_fill, "format": a.occlusion_format,
                           "alpha": 0.4 if a.occlusion_format == "png" else None, "members_files": bool(a.occlusion_members),
                           "threshold": ensemble.THR, "precision": mode, "batch_size": a.batch_size, "n_images": len(names),
                           "members": [spec.name for spec, _ in members]}
    with open(os.path.join(a.occlusion, "occlusion.json"), "w") as f:
        json.dump(summary, f, indent=1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("input_csv")
    ap.add_argument("output_csv")
    ap.add_argument("--scores-out", default=None)
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--allow-missing", action="store_true")
    ap.add_argument("--webp-lossy", action="store_true",
                    help="accept lossy WebP files (VP8 key frames; env VIP_WEBP_LOSSY=1 does the same): token decode on the host, "
                         "reconstruction on the GPU, libwebp's pixels bit for bit.  Off by default: such files are refused")
    ap.add_argument("--ckpt-cfg", default=os.path.join(HERE, "ckpts", "ckpts.json"))
    ap.add_argument("--batch-size", type=int, default=128)  # main.py:85
    ap.add_argument("--debug", type=int, default=0)         # main.py:82-83: first 100 images
    ap.add_argument("--tta", type=int, default=1)           # main.py:167: passes under apply_augment, averaged
    ap.add_argument("--tta-seed", type=int, default=0)
    ap.add_argument("--shard", default="images", choices=["images", "members", "hybrid"],
                    help="how N > 1 ranks split the (member, image-shard) grid: images = every rank all members on its image shard "
                         "(MirroredStrategy's split, utils/device.py:7); members = rank r owns members r mod N and scores every "
                         "image (one model per GPU); hybrid = LPT packing by measured ms/image.  One all-gather in every mode.")
    ap.add_argument("--precision", default=None, choices=["fast", "strict", "f32"],
                    help="fast (default; env VIP_PRECISION): fp16 storage, the throughput path - member logits at the fp16 storage floor "
                         "(7e-4 ... 8e-3 vs an fp32 run).  strict: every activation and weight stored as a pair of fp16 values (hi, lo: "
                         "22 significant bits), fp32 accumulation - every member's logit within 1e-3 of the reference's fp32 "
                         "TensorFlow run (main.py:107-109); a value must satisfy |v| <= 65504, and a run in which an activation "
                         "leaves that range ends with an error that says to switch to f32.  f32: fp32 storage and fp32 matrix "
                         "arithmetic, no range limit, the slowest of the three.")
    ap.add_argument("--calibration-images", default=None, metavar="DIR",
                    help="fast mode: a directory of JPEGs (up to 32 are read) for the bias calibration of the fp16 weights instead of the "
                         "built-in seeded synthetic batch - use real images with real checkpoints (the correction needs typical "
                         "per-channel input means; inputs only, no labels)")
    ap.add_argument("--no-bias-calibration", action="store_true",
                    help="fast mode: plain fp16 weights, no calibration pass at load time")
    ap.add_argument("--heatmaps", default=None, metavar="DIR",
                    help="write the ensemble's Grad-CAM evidence map of every input file into DIR (the mean over the members that have "
                         "a spatial map, each normalised to its own peak; ViT members are listed as unsupported in DIR/heatmaps.json)")
    ap.add_argument("--heatmap-format", default="npy", choices=["npy", "png"],
                    help="npy: the fp32 map in [0, 1] at the image's size; png: the jet colour table blended over the image (alpha 0.4)")
    ap.add_argument("--heatmap-members", action="store_true",
                    help="also write every member's low-resolution map and peak: DIR/<name>.members.npz")
    ap.add_argument("--stress-jpeg", default=None, metavar="Q[,Q...]",
                    help="recompression stress test: also score every image re-saved as JPEG at each quality (1..100; duplicates are "
                         "dropped, highest first) and report whether the decision survives; needs --stress-out")
    ap.add_argument("--stress-out", default=None, metavar="FILE.csv",
                    help="per input file: filename, p, decision, p_q<Q>..., decision_q<Q>..., stable, flips_at; FILE.json next to it "
                         "holds the per-quality flip counts and rates, mean |p_q - p| and the settings")
    ap.add_argument("--stress-subsampling", default="420", choices=["420", "444"],
                    help="chroma sampling of the simulated re-save: 420 (libjpeg's default) or 444")
    ap.add_argument("--stress-resize", default=None, metavar="P[,P...]",
                    help="resize stress test: also score every image rescaled to each percent of its own size (integers in 10..400; "
                         "duplicates and 100 are dropped, largest first), unsaved and - with --stress-jpeg - re-saved at every quality; "
                         "needs --stress-out, whose table becomes filename, p, decision, p_<label>..., decision_<label>..., stable, "
                         "flips_at, flips over the labels q<Q>, r<P>, r<P>_q<Q>")
    ap.add_argument("--stress-resize-filter", default="bicubic", choices=["bilinear", "bicubic", "lanczos"],
                    help="the antialiased filter of the simulated resize (what an image editor's resize offers)")
    ap.add_argument("--stress-blur", default=None, metavar="S[,S...]",
                    help="blur stress test: also score every image under a Gaussian blur of each sigma (pixels; decimals in 0.3..5.0 with at "
                         "most one fractional digit; duplicates are dropped, smallest first), unsaved and - with --stress-jpeg - re-saved at "
                         "every quality; needs --stress-out, whose table gains the labels b<TT>, b<TT>_q<Q> (TT = ten times sigma, two "
                         "digits) in the layout of --stress-resize")
    ap.add_argument("--stress-blur-radius", type=int, default=None, metavar="R",
                    help="cut the Gaussian off R pixels from its centre (1..15; default ceil(3 sigma)); --stress-blur 1 "
                         "--stress-blur-radius 1 is exactly the reference's gaussian_filter2d(filter_shape=3) (dataset/augment.py:131-140)")
    ap.add_argument("--stress-median", default=None, metavar="K[,K...]",
                    help="median stress test: also score every image under a K x K median filter (K = 3 or 5; 3 is the reference's "
                         "median_filter2d), unsaved and - with --stress-jpeg - re-saved at every quality; needs --stress-out, whose table "
                         "gains the labels m<K>, m<K>_q<Q>")
    ap.add_argument("--stress-flip", default=None, metavar="h[,v]",
                    help="flip stress test: also score every image mirrored left-right (h) and / or top-bottom (v), unsaved and - with "
                         "--stress-jpeg - re-saved at every quality; needs --stress-out, whose table gains the labels fliph, flipv and "
                         "their _q<Q> in the layout of --stress-resize (dataset/augment.py:115-120)")
    ap.add_argument("--stress-crop", default=None, metavar="P[,P...]",
                    help="crop stress test: also score every image cropped to each listed percent of its sides (integers in 50..99; "
                         "duplicates are dropped, largest first), unsaved and - with --stress-jpeg - re-saved at every quality; needs "
                         "--stress-out, whose table gains the labels crop<PP>, crop<PP>_q<Q>")
    ap.add_argument("--stress-crop-origin", default="centre", choices=["centre", "topleft"],
                    help="where the crop is taken: the middle of the image (off a JPEG source's 8 x 8 grid unless the offset happens to "
                         "be a multiple of 8), or its top-left corner (on the grid)")
    ap.add_argument("--stress-rotate", default=None, metavar="D[,D...]",
                    help="rotation stress test: also score every image rotated counter-clockwise by each listed angle (degrees; non-zero "
                         "decimals in -45..45 with at most one fractional digit; duplicates are dropped, ascending), bilinear, unsaved and "
                         "- with --stress-jpeg - re-saved at every quality; needs --stress-out, whose table gains the labels rot<TTT> / "
                         "rotm<TTT> (negative) and their _q<Q>, TTT = ten times the angle, three digits (dataset/augment.py:68-107); write a "
                         "list that starts with a negative angle as --stress-rotate=-3,7.5")
    ap.add_argument("--stress-rotate-fill", default="crop", choices=["crop", "mirror", "black"],
                    help="what a rotated image's corners become: crop - the image is cut down to the largest upright rectangle inside the "
                         "rotated one (an editor's 'straighten'); mirror / black - the size is kept and the corners are mirrored / black "
                         "(black is the reference's constant fill)")
    ap.add_argument("--stress-gray", action="store_true",
                    help="colour stress test: also score every image as a gray image (Pillow's luma in three channels; "
                         "dataset/augment.py:142-146), unsaved and - with --stress-jpeg - re-saved at every quality; needs --stress-out, whose "
                         "table gains the labels gray, gray_q<Q> in the layout of --stress-resize")
    ap.add_argument("--stress-bgr", action="store_true",
                    help="colour stress test: also score every image with red and blue exchanged (dataset/augment.py:148-151); labels bgr, "
                         "bgr_q<Q>; needs --stress-out")
    ap.add_argument("--stress-hue", default=None, metavar="D[,D...]",
                    help="colour stress test: also score every image with its chroma rotated by each listed angle (non-zero integer degrees "
                         "in -180..180; duplicates are dropped, ascending) - a rotation in the YIQ plane, the linear form of a hue shift, not "
                         "tf.image's HSV round trip; labels hue<DDD> / huem<DDD> (negative) and their _q<Q>; needs --stress-out; write a "
                         "list that starts with a negative angle as --stress-hue=-30,30")
    ap.add_argument("--stress-saturation", default=None, metavar="P[,P...]",
                    help="colour stress test: also score every image at each listed percent of its saturation (integers in 0..200 other than "
                         "100; ascending) - a blend with the luma image, the linear form; 0 is --stress-gray; labels sat<PPP>, "
                         "sat<PPP>_q<Q>; needs --stress-out")
    ap.add_argument("--stress-contrast", default=None, metavar="P[,P...]",
                    help="colour stress test: also score every image at each listed percent of its contrast about its own mean colour "
                         "(integers in 0..200 other than 100; ascending; tf.image.adjust_contrast); labels con<PPP>, con<PPP>_q<Q>; needs "
                         "--stress-out")
    ap.add_argument("--stress-brightness", default=None, metavar="P[,P...]",
                    help="colour stress test: also score every image with each listed percent of full scale added (non-zero integers in "
                         "-50..50; ascending; tf.image.adjust_brightness); labels bri<PP> / brim<PP> (negative) and their _q<Q>; needs "
                         "--stress-out; write a list that starts with a negative value as --stress-brightness=-10,10")
    ap.add_argument("--stress-gamma", default=None, metavar="G[,G...]",
                    help="colour stress test: also score every image under 255 (x / 255) ** G for each listed G (decimals in 0.50..2.00 with "
                         "at most two fractional digits, other than 1; ascending; below 1 brightens; tf.image.adjust_gamma); labels "
                         "gam<PPP>, gam<PPP>_q<Q> with PPP = 100 G; needs --stress-out")
    ap.add_argument("--stress-noise", default=None, metavar="S[,S...]",
                    help="noise stress test: also score every image with Gaussian noise of each listed sigma (levels, 0.5..50.0 with at "
                         "most one fractional digit; ascending; a value listed twice is refused) added to every channel independently, "
                         "unsaved and - with --stress-jpeg - re-saved at every quality; integer arithmetic from Philox4x32-10 keyed by "
                         "--stress-noise-seed and the crc32 of the file's basename, so a file gets the same noise in any order, batch "
                         "size or rank; needs --stress-out, whose table gains the labels n<TTT>, n<TTT>_q<Q> (TTT = ten times sigma)")
    ap.add_argument("--stress-noise-mono", default=None, metavar="S[,S...]",
                    help="noise stress test: as --stress-noise with ONE sample per pixel on all three channels (luminance noise); labels "
                         "nm<TTT>, nm<TTT>_q<Q>; needs --stress-out")
    ap.add_argument("--stress-speckle", default=None, metavar="P[,P...]",
                    help="noise stress test: also score every image with every sample multiplied by 1 + P / 100 z, z standard normal "
                         "(integer percents in 1..50; ascending; a value listed twice is refused); labels spk<PP>, spk<PP>_q<Q>; needs "
                         "--stress-out")
    ap.add_argument("--stress-impulse", default=None, metavar="P[,P...]",
                    help="noise stress test: also score every image with each listed percent of its pixels (0.1..50.0 with at most one "
                         "fractional digit; ascending; a value listed twice is refused) turned black or white, half each; labels "
                         "imp<TTT>, imp<TTT>_q<Q> (TTT = ten times the percent); needs --stress-out")
    ap.add_argument("--stress-noise-seed", type=int, default=0, metavar="N",
                    help="the seed of the noise stress tests' random field (0..4294967295, default 0); needs one of --stress-noise, "
                         "--stress-noise-mono, --stress-speckle, --stress-impulse")
    ap.add_argument("--stress-sharpen", default=None, metavar="P[,P...]",
                    help="sharpening stress test: also score every image under an unsharp mask of each listed gain (integer percents in "
                         "1..500; ascending; a value listed twice is refused): out = X + P / 100 (X - blurred X) where |X - blurred X| "
                         "exceeds the threshold, in integers on the Gaussian of --stress-blur (one launch; close to Pillow's UnsharpMask, "
                         "which blurs with a box approximation, not bit for bit), unsaved and - with --stress-jpeg - re-saved at every "
                         "quality; needs --stress-out, whose table gains the labels shp<PPP>, shp<PPP>_q<Q> after the noise rows")
    ap.add_argument("--stress-sharpen-sigma", default=None, metavar="S",
                    help="sigma of the unsharp mask's Gaussian in pixels (0.3..5.0 with at most one fractional digit, default 1.0); needs "
                         "--stress-sharpen or a --stress-chain with a shp step")
    ap.add_argument("--stress-sharpen-radius", type=int, default=None, metavar="R",
                    help="cut the unsharp mask's Gaussian off R pixels from its centre (1..15; default ceil(3 sigma)); needs "
                         "--stress-sharpen or a --stress-chain with a shp step")
    ap.add_argument("--stress-sharpen-threshold", type=int, default=None, metavar="T",
                    help="leave a sample as it is where it differs from its blurred value by at most T levels (0..255, default 0); needs "
                         "--stress-sharpen or a --stress-chain with a shp step")
    ap.add_argument("--stress-autocontrast", default=None, metavar="C[,C...]",
                    help="tone stress test: also score every image after Pillow's ImageOps.autocontrast(cutoff=C) per channel, bit for bit "
                         "(integer percents 0..49; ascending; a value listed twice is refused): the levels stretched to the full range "
                         "after C %% of the pixels are cut off either end of the image's own histogram; three launches (histograms, "
                         "tables, pixels), unsaved and - with --stress-jpeg - re-saved at every quality; needs --stress-out, whose table "
                         "gains the labels ac<PP>, ac<PP>_q<Q> after the sharpening rows")
    ap.add_argument("--stress-autocontrast-luma", default=None, metavar="C[,C...]",
                    help="tone stress test: the same with ONE curve from the luma's histogram on all three channels "
                         "(autocontrast(cutoff=C, preserve_tone=True)); labels acl<PP>, acl<PP>_q<Q>; needs --stress-out")
    ap.add_argument("--stress-equalize", action="store_true",
                    help="tone stress test: also score every image with its histogram flattened per channel (Pillow's ImageOps.equalize, "
                         "bit for bit); labels eq, eq_q<Q>; needs --stress-out")
    ap.add_argument("--stress-clahe", default=None, metavar="L[,L...]",
                    help="tone stress test: also score every image after contrast-limited adaptive equalisation of its luma at each listed "
                         "clip limit (1.0..9.9 with at most one fractional digit; ascending; a value listed twice is refused), per tile "
                         "with the tile tables blended bilinearly and the chroma kept, in integers; labels clahe<TT>, clahe<TT>_q<Q> (TT = "
                         "ten times the limit); needs --stress-out")
    ap.add_argument("--stress-clahe-grid", type=int, default=None, metavar="G",
                    help="tiles per axis of --stress-clahe (1..16, default 8; fewer on an axis shorter than 16 G pixels, a tile is at "
                         "least 16 pixels wide); needs --stress-clahe or a --stress-chain with a clahe step")
    ap.add_argument("--stress-webp", default=None, metavar="Q[,Q...]",
                    help="lossy WebP stress test: also score every image as it comes back from a lossy WebP save at each quality (integers "
                         "in 1..100; highest first; a value listed twice is refused) - the project's own VP8 key-frame encoder on the GPU, "
                         "decoded as libwebp decodes the file -, unsaved and - with --stress-jpeg - re-saved as JPEG at every quality; needs "
                         "--stress-out, whose table gains the labels w<Q>, w<Q>_q<Q'> after the tone rows")
    ap.add_argument("--stress-chain", default=None, metavar="STEP+STEP[+STEP...][,CHAIN...]",
                    help="stress chains: also score every image after a SEQUENCE of perturbations, e.g. r50+shp080+q75 (downscale, "
                         "sharpen, re-save: what a messenger does) or q90+crop95+q75 (double compression on a shifted block grid).  A "
                         "chain is 2..8 steps joined by +, up to 16 chains separated by commas, kept in the order given; a chain listed "
                         "twice is refused.  A step is a single-variant label of the other stress flags in its canonical spelling: q<Q>, "
                         "r<P>, b<TT>, m3, m5, fliph, flipv, crop<PP>, rot<TTT>, rotm<TTT>, gray, bgr, hue<DDD>, huem<DDD>, sat<PPP>, "
                         "con<PPP>, bri<PP>, brim<PP>, gam<PPP>, n<TTT>, nm<TTT>, spk<PP>, imp<TTT>, shp<PPP>, ac<PP>, acl<PP>, eq, "
                         "clahe<TT>, w<Q>; it takes the options of its "
                         "family's flags (--stress-subsampling, --stress-resize-filter, --stress-blur-radius, --stress-crop-origin, "
                         "--stress-rotate-fill, --stress-sharpen-sigma / -radius / -threshold, --stress-noise-seed, --stress-clahe-grid), which "
                         "are accepted "
                         "when a chain holds the step they govern.  The result is scored once, as written: --stress-jpeg does not "
                         "multiply chain rows.  Needs --stress-out, whose table gains one column pair per chain under the chain's text, "
                         "after all other rows; they count for stable and flips, not for flips_at")
    ap.add_argument("--tiles-out", default=None, metavar="FILE.csv",
                    help="native-resolution tiles: also score every image at least --tile-size pixels high and wide as a grid of tile x "
                         "tile crops, each taken as an image of its own; per input file: filename, width, height, tiles, grid, p, decision, "
                         "p_tiles_mean, p_tiles_max, frac_tiles, decision_tiles, agrees; FILE.json next to it holds the settings and "
                         "counts, FILE.tiles.csv (one rank only) every tile's scores")
    ap.add_argument("--tile-size", type=int, default=200, help="side of a tile in pixels, 16..1024 (200: the challenge's own image size)")
    ap.add_argument("--tile-stride", type=int, default=None, metavar="S",
                    help="largest distance between neighbouring tiles, 1..tile size (default: the tile size, no more overlap than needed)")
    ap.add_argument("--tile-max", type=int, default=256,
                    help="most tiles per image, 1..4096; a larger grid is thinned to an evenly spaced sample (listed in FILE.json)")
    ap.add_argument("--tile-agg", default="mean", choices=["mean", "max"],
                    help="decision_tiles = this statistic of the ensemble's tile scores > 0.487")
    ap.add_argument("--occlusion", default=None, metavar="DIR",
                    help="occlusion sensitivity: also score every image with each window of a grid hidden and write into DIR, per input "
                         "file, the ensemble's full-size map of delta-p (what hiding the region takes off the synthetic score), plus "
                         "DIR/occlusion.csv and DIR/occlusion.json; needs no gradients, so ViT members are covered; costs "
                         "(grid - window + 1)^2 extra member passes per image, 49 at the defaults")
    ap.add_argument("--occlusion-grid", type=int, default=8, help="cells per axis, 2..32; an image lower or narrower than this is skipped")
    ap.add_argument("--occlusion-window", type=int, default=2, help="side of the hidden window in cells, 1..grid")
    ap.add_argument("--occlusion-fill", default="mean", choices=["mean", "gray"],
                    help="what hides a window: the image's own mean colour, or (128, 128, 128)")
    ap.add_argument("--occlusion-format", default="npy", choices=["npy", "png"],
                    help="npy: the fp32 delta-p map at the image's size; png: the map scaled to its largest |value| around 128 = no "
                         "effect, through the jet colour table, blended over the image (alpha 0.4)")
    ap.add_argument("--occlusion-members", action="store_true",
                    help="also write every member's [grid, grid] cells and per-variant scores: DIR/<name>.members.npz")
    a = ap.parse_args(argv)
    chains, in_chain = None, set()                      # the chain texts, and the step kinds they hold
    if a.stress_chain is not None:
        try:
            chains = grammar.parse_chains(a.stress_chain)
        except ValueError as e:
            raise SystemExit(f"vipcup_amd main: --stress-chain {a.stress_chain!r}: {e}")
        in_chain = grammar.chain_kinds(chains)
    flagged = {kind for kind, row in grammar.STEPS.items() if getattr(a, _dest(row.flag)) not in (None, False)}
    stress_run = bool(flagged) or chains is not None    # the one question: does any stress flag replace the batch scorer
    if a.occlusion is not None:
        if a.shard != "images" or a.tta > 1:
            # as for the heat maps: the scores of one image would be spread over ranks or over augmented copies
            raise SystemExit("vipcup_amd main: --occlusion works with --shard images and --tta 1 only (got --shard "
                             f"{a.shard} --tta {a.tta}): occlusion maps under member sharding or TTA are not implemented")
        if a.heatmaps is not None or stress_run or a.stress_out is not None or a.tiles_out is not None:
            raise SystemExit("vipcup_amd main: --occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out (each replaces the "
                             "batch scorer): run them one after the other")
        if not 2 <= a.occlusion_grid <= 32:
            raise SystemExit(f"vipcup_amd main: --occlusion-grid {a.occlusion_grid}: expected an integer in 2..32")
        if not 1 <= a.occlusion_window <= a.occlusion_grid:
            raise SystemExit(f"vipcup_amd main: --occlusion-window {a.occlusion_window}: expected an integer in 1..{a.occlusion_grid} (the grid)")
    elif a.occlusion_grid != 8 or a.occlusion_window != 2 or a.occlusion_fill != "mean" or a.occlusion_format != "npy" or a.occlusion_members:
        raise SystemExit("vipcup_amd main: --occlusion-grid / --occlusion-window / --occlusion-fill / --occlusion-format / --occlusion-members "
                         "need --occlusion DIR")
    if a.tiles_out is not None:
        if a.shard != "images" or a.tta > 1:
            # as for the stress runs: the scores of one image would be spread over ranks or over augmented copies
            raise SystemExit("vipcup_amd main: --tiles-out works with --shard images and --tta 1 only (got --shard "
                             f"{a.shard} --tta {a.tta}): tile scoring under member sharding or TTA is not implemented")
        if a.heatmaps is not None or stress_run or a.stress_out is not None:
            raise SystemExit("vipcup_amd main: --tiles-out cannot be combined with --heatmaps or --stress-* (each replaces the batch scorer): "
                             "run them one after the other")
        if not 16 <= a.tile_size <= 1024:
            raise SystemExit(f"vipcup_amd main: --tile-size {a.tile_size}: expected an integer in 16..1024")
        if a.tile_stride is not None and not 1 <= a.tile_stride <= a.tile_size:
            raise SystemExit(f"vipcup_amd main: --tile-stride {a.tile_stride}: expected an integer in 1..{a.tile_size} (the tile size)")
        if not 1 <= a.tile_max <= 4096:
            raise SystemExit(f"vipcup_amd main: --tile-max {a.tile_max}: expected an integer in 1..4096")
    elif a.tile_size != 200 or a.tile_stride is not None or a.tile_max != 256 or a.tile_agg != "mean":
        raise SystemExit("vipcup_amd main: --tile-size / --tile-stride / --tile-max / --tile-agg need --tiles-out FILE.csv")
    # the run's keywords of stress_batch / stress_labels: the list or switch of every flag given, every option, the chains
    stress = {"qualities": [], "subsampling": {"420": "4:2:0", "444": "4:4:4"}[a.stress_subsampling]}
    waiting = []                                        # (flag, family) whose shared refusals follow once every list is read

    def read(kind):
        row = grammar.STEPS[kind]
        if kind in flagged:
            stress[row.keyword or "qualities"] = _stress_list(kind, getattr(a, _dest(row.flag))) if kind in _LISTS else True
            if row.family in ("recompression", "resize"):
                _refuse_context(a, row.flag, row.family)
            else:
                waiting.append((row.flag, row.family))
        for option in _OPTIONS:
            if option.after == kind:
                dest = _dest(option.flag)
                stress[option.keyword] = _stress_option(option, getattr(a, dest), ap.get_default(dest), flagged | in_chain)

    for kind in grammar.STEPS:                          # in row order; the qualities last, after the others' shared refusals
        if kind != "recompress":
            read(kind)
    if chains is not None:
        stress["chains"] = chains
        waiting.append(("--stress-chain", "chained"))
    for flag, family in waiting:
        _refuse_context(a, flag, family)
    read("recompress")
    if a.stress_jpeg is None and ((a.stress_out is not None and not stress_run) or
                                  (a.stress_subsampling != "420" and "recompress" not in in_chain)):
        raise SystemExit("vipcup_amd main: --stress-out / --stress-subsampling need --stress-jpeg Q[,Q...]"
                         + (" (--stress-out alone also goes with --stress-resize P[,P...])" if a.stress_out is not None else ""))
    if a.heatmaps is not None and (a.shard != "images" or a.tta > 1):
        # the maps of one image would be spread over ranks (members / hybrid) or over augmented copies (TTA): not built
        raise SystemExit("vipcup_amd main: --heatmaps works with --shard images and --tta 1 only (got --shard "
                         f"{a.shard} --tta {a.tta}): evidence maps under member sharding or TTA are not implemented")
    if a.heatmaps is None and (a.heatmap_members or a.heatmap_format != "npy"):
        raise SystemExit("vipcup_amd main: --heatmap-format / --heatmap-members need --heatmaps DIR")

    import pandas as pd
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, ops, pipeline, zoo

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if not torch.cuda.is_available():
        raise SystemExit("vipcup_amd main: no GPU visible — the HIP path has no CPU fallback")
    backend = os.environ.get("VIP_DIST_BACKEND", "nccl")     # gloo: several ranks may share one card (rehearsals on a 1-GPU box)
    dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
    torch.cuda.set_device(dev_index)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    infer_path = os.path.dirname(os.path.abspath(a.input_csv))   # main.py:161-164
    test_csv = pd.read_csv(a.input_csv)
    names = test_csv.filename.values.tolist()
    if a.debug:
        names = names[:100]
    paths = [os.path.join(infer_path, n) for n in names]

    manifest = []
    for name, dim, idx in json.load(open(a.ckpt_cfg)):           # main.py:171-198
        key = zoo.by_ckpt_name(name)
        if key is None:
            if a.allow_missing:
                if rank == 0:
                    print(f"> SKIP {name}: graph not built in this round")
                continue
            raise ValueError(f"manifest member {name} has no graph in vipcup_amd.zoo")
        manifest.append((name, dim, idx, key))
    mode = a.precision or ops.PRECISION
    calib = None
    if a.calibration_images and mode == "fast" and not a.no_bias_calibration:
        files = sorted(glob(os.path.join(a.calibration_images, "*.jpg")) + glob(os.path.join(a.calibration_images, "*.jpeg")) +
                       glob(os.path.join(a.calibration_images, "*.JPG")) + glob(os.path.join(a.calibration_images, "*.png")) +
                       glob(os.path.join(a.calibration_images, "*.PNG")))[:32]
        if not files:
            raise ValueError(f"--calibration-images {a.calibration_images}: no *.jpg / *.jpeg / *.png files")
        calib = pipeline.decode_images([open(f, "rb").read() for f in files])
        if rank == 0:
            print(f"> BIAS CALIBRATION on {len(files)} images from {a.calibration_images}")
    build = dict(bias_calibration=not a.no_bias_calibration, precision=mode, calibration_batch=calib)
    plan = ensemble.ShardPlan("members" if a.shard == "members" else "images", len(manifest), world)
    mine = {m for ms in plan.units[rank].values() for m in ms}   # members mode: a rank loads only the members it owns
    members = []
    for mi, (name, dim, idx, key) in enumerate(manifest):
        spec = zoo.MEMBERS[key]
        assert [spec.input_hw, spec.input_hw] == list(dim), (name, dim)
        ckpts = sorted(glob(os.path.join(HERE, "ckpts", name, "ckpt", "*.npz")) + glob(os.path.join(HERE, "ckpts", name, "ckpt", "*.h5")))
        sm_path = os.path.join(HERE, "ckpts", name, "ckpt", "saved_model.pb")
        if not ckpts and os.path.isfile(sm_path):                  # SavedModel format, when there are no .h5 folds (main.py:186-191)
            ckpts = [sm_path]
        if mi not in mine:
            if not ckpts and not a.synthetic:
                raise ValueError(f"no checkpoints under ckpts/{name}/ckpt (pass --synthetic for seeded synthetic weights)")
            members.append((spec, None))
            continue
        if ckpts:
            # graph family from the directory name, variant (first_strides / classes / head activation) from the file's model_config
            folds = [zoo.construct(spec, zoo.match_variable_names(spec, zoo.read_checkpoint(c)), variant=zoo.checkpoint_variant(spec, c),
                                   **build) for c in ckpts]
        elif a.synthetic:
            folds = [zoo.build_member(key, **build)[1]]
        else:
            raise ValueError(f"no checkpoints under ckpts/{name}/ckpt (pass --synthetic for seeded synthetic weights)")
        members.append((spec, zoo.FoldMean(folds)))                # mean over folds, main.py:121
        if rank == 0:
            print(f"> MODEL({len(members)}): {name} | DIM: {dim} | folds: {len(folds)} | precision: {mode}")

    def jpegs_for(lo, hi):
        out = []
        for p in paths[lo:hi]:
            with open(p, "rb") as f:
                out.append(f.read())
        return out

    batch_scorer = None
    if a.heatmaps is not None:
        batch_scorer = _heatmap_writer(a, names, members, rank)
    stress_rows = []
    if stress_run:
        batch_scorer = _stress_scorer(stress, names, stress_rows)
    tile_rows, tile_scores = [], []
    if a.tiles_out is not None:
        batch_scorer = _tile_scorer(a, tile_rows, tile_scores)
    occlusion_rows = []
    if a.occlusion is not None:
        batch_scorer = _occlusion_scorer(a, names, members, occlusion_rows)

    t0 = time.time()
    costs = None
    lossy_webp = True if a.webp_lossy else None          # None: the VIP_WEBP_LOSSY knob decides
    if a.shard == "hybrid" and world > 1:
        costs = ensemble.measure_costs(members, jpegs_for(0, min(len(paths), a.batch_size)), dist, rank, lossy_webp=lossy_webp)
        if rank == 0:
            print("> HYBRID PLAN:", ensemble.ShardPlan("hybrid", len(members), world, costs).describe())
    per_model = ensemble.score_files(jpegs_for, len(paths), members, a.batch_size, rank, world, dist,
                                     tta=a.tta, tta_seed=a.tta_seed, shard=a.shard, costs=costs, batch_scorer=batch_scorer,
                                     lossy_webp=lossy_webp)
    uniq, score, decision = ensemble.aggregate(names, per_model)
    stressed = None
    if stress_run:                                      # the one extra collective of a stress run: every rank's [V, M, n_local] rows
        stressed = ensemble.gather_stress_rows(stress_rows, len(_stress_labels(stress)), len(members), len(paths), rank, world, dist)
    tiled = None
    if a.tiles_out is not None:                         # the one extra collective of a tile run: every rank's [3 + 2, M + 1, n_local] rows
        tiled = ensemble.gather_stress_rows(tile_rows, 5, len(members) + 1, len(paths), rank, world, dist)
    occluded = None
    if a.occlusion is not None:                         # the one extra collective of an occlusion run: every rank's [4 + 2, M + 1, n_local] rows
        occluded = ensemble.gather_stress_rows(occlusion_rows, 6, len(members) + 1, len(paths), rank, world, dist)
    if rank == 0:
        pd.DataFrame({"filename": uniq, "logit": decision}).to_csv(a.output_csv, index=False)  # main.py:143-145
        if a.scores_out:
            cols = {"filename": names, "ensemble_mean": per_model.mean(axis=0)}
            for (spec, _), row in zip(members, per_model):
                cols[spec.name] = row
            pd.DataFrame(cols).to_csv(a.scores_out, index=False)
        if stressed is not None:
            _write_stress(a, names, members, per_model, stressed, stress, mode)
            print(f"> STRESS TABLE SAVED TO {a.stress_out}")
        if tiled is not None:
            per_tile = None
            if world == 1:
                per_tile = torch.cat(tile_scores, dim=1).cpu().numpy() if tile_scores else np.zeros((len(members) + 1, 0), np.float32)
            _write_tiles(a, names, members, per_model, tiled, per_tile, mode, world)
            print(f"> TILE REPORT SAVED TO {a.tiles_out}")
        if occluded is not None:
            _write_occlusion(a, names, members, per_model, occluded, mode)
            print(f"> OCCLUSION MAPS AND REPORT SAVED TO {a.occlusion}")
        dt = time.time() - t0
        print(f"> FINAL PREDICTION SAVED TO {a.output_csv}")
        print(f"> TIME TO INFER: {dt / 60:.2f} min ({len(paths) / dt:.1f} images/s on {world} GPU(s))")  # main.py:231-235
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
