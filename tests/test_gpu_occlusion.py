"""GPU: occlusion evidence maps.  The mean colour against numpy's integer rule; the gather kernel (``DecodedBatch.occluded``) against the
parent pipeline on numpy-occluded copies of the images (``DecodedBatch.resized``: exact); the cell, statistics and map kernels against
numpy loops in the stated order; and ``main.py --occlusion`` end to end - with a grid of one window the only variant of an image is the
image at its mean colour, so its scores are those of a plain run on a flat file of that colour, exactly, and on a flat file every variant
is the plain input, so every delta is exactly 0."""
import functools
import io
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests._jpeg_enc_ref import content  # noqa: E402
from tools.make_synth import synth_pixels  # noqa: E402

SIZES = [(13, 13), (14, 40), (29, 16), (40, 37)]                       # (height, width): those of tests/test_gpu_tiles.py
GRIDS = [(3, 2), (5, 1), (4, 4)]                                       # (grid, window)
SIDES = [13, 16, 8]                                                    # 13: the identity branch for the 13 x 13 image, bicubic for the others


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(71 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _batch(imgs, pad: int = 3):
    """a DecodedBatch holding ``imgs`` in slots of the largest size + pad, the rest of every slot filled with noise (as
    tests/test_gpu_tiles.py builds it): a kernel that read past an image's own edge would pick the noise up"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    sizes = [(im.shape[0], im.shape[1]) for im in imgs]
    maxH, maxW = max(h for h, _ in sizes) + pad, max(w for _, w in sizes) + pad
    rgb = np.random.default_rng(5).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


def _mean_rule(im) -> np.ndarray:
    """(sum + h w // 2) // (h w) per channel, in Python integers; byte 3 is 0"""
    hw = im.shape[0] * im.shape[1]
    sums = [int(im[..., c].astype(np.int64).sum()) for c in range(3)]
    return np.array([(s + hw // 2) // hw for s in sums] + [0], np.uint8)


def test_mean_colour_against_the_integer_rule():
    tie = np.zeros((2, 2, 3), np.uint8)
    tie[..., 0] = [[0, 0], [0, 1]]                                       # 0.25 -> 0
    tie[..., 1] = [[0, 1], [1, 0]]                                       # 0.5 -> 1: halves go up
    tie[..., 2] = [[255, 255], [254, 254]]                               # 254.5 -> 255
    wide = content(75, 301, 7)                                           # more than one pass of the 64-pixel column loop, an odd width
    imgs = list(_images()) + [tie, wide]
    batch = _batch(imgs)
    before = batch.rgb.clone()
    got = batch.mean_colour()
    torch.cuda.synchronize()
    assert got.dtype == torch.uint8 and got.shape == (len(imgs), 4) and got.is_cuda
    want = np.stack([_mean_rule(im) for im in imgs])
    assert want[4].tolist() == [0, 1, 255, 0]
    assert np.array_equal(got.cpu().numpy(), want), (got.cpu().numpy(), want)
    assert torch.equal(batch.rgb, before)
    # an all-255 image in a slot of its own size: the rule is exact at the top of the range
    full = np.full((70, 130, 3), 255, np.uint8)
    assert _batch([full], pad=0).mean_colour().cpu().numpy().tolist() == [[255, 255, 255, 0]]


@functools.lru_cache(maxsize=None)
def _plan(grid: int, window: int):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    return pipeline.occlusion_plan(SIZES, grid, window)


def _occluded_copies(tab, fill):
    """the variants as images of their own: a DecodedBatch of numpy copies with the rectangle overwritten - what the parent's ``resized`` sees"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    maxH, maxW = max(h for h, _ in SIZES), max(w for _, w in SIZES)
    rgb = np.zeros((len(tab), maxH, maxW, 3), np.uint8)
    sizes = []
    for v, (i, y0, x0, y1, x1, *_) in enumerate(tab.tolist()):
        im = imgs[i].copy()
        im[y0:y1, x0:x1] = fill[i, :3]
        rgb[v, :im.shape[0], :im.shape[1]] = im
        sizes.append((im.shape[0], im.shape[1]))
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("grid,window", GRIDS, ids=[f"g{g}k{k}" for g, k in GRIDS])
def test_gather_equals_resized_on_occluded_copies(grid, window, side):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    batch = _batch(_images())
    before = batch.rgb.clone()
    tab = _plan(grid, window).tab
    V = len(tab)
    assert V == len(SIZES) * (grid - window + 1) ** 2
    tab_d = torch.from_numpy(tab).cuda()
    mean_d = batch.mean_colour()
    assert np.array_equal(mean_d.cpu().numpy(), np.stack([_mean_rule(im) for im in _images()]))
    gray_d = torch.tensor([[128, 128, 128, 0]] * len(SIZES), dtype=torch.uint8, device="cuda")
    cut = max(1, V // 3)
    for fill_d in (mean_d, gray_d):
        alone = _occluded_copies(tab, fill_d.cpu().numpy())
        for c_out in (8, 4):
            for dtype in (torch.float16, torch.float32) + ((ops.PACKED,) if c_out == 8 else ()):
                got = batch.occluded(tab_d, 0, V, fill_d, side, side, c_out, dtype)
                want = alone.resized(side, side, c_out, dtype)
                torch.cuda.synchronize()
                assert got.shape == (V, side, side, c_out) and got.dtype == dtype
                assert torch.equal(got, want), (grid, window, side, c_out, dtype, int((got != want).sum()))
                if dtype != ops.PACKED:
                    assert got[..., 3:].abs().max().item() == 0.0
                else:
                    assert torch.equal(got, ops.pack_h2(batch.occluded(tab_d, 0, V, fill_d, side, side, c_out, torch.float32)))
                if V > 1:       # a table split in two calls (how ``occlusion_batch`` walks it in chunks) gives the same rows
                    part = torch.cat([batch.occluded(tab_d, 0, cut, fill_d, side, side, c_out, dtype),
                                      batch.occluded(tab_d, cut, V, fill_d, side, side, c_out, dtype)])
                    assert torch.equal(part, got)
    # a variant differs from the plain input where a tap reads a hidden pixel
    plain = batch.resized(side, side, 8, torch.float32)
    got = batch.occluded(tab_d, 0, V, gray_d, side, side, 8, torch.float32)
    for i in range(len(SIZES)):
        assert any(not torch.equal(got[v], plain[i]) for v in range(V) if tab[v, 0] == i), i
    assert torch.equal(batch.rgb, before), "occluded() changed its input"


def test_gather_with_unequal_sides_and_refusals():
    import vipcup_amd  # noqa: F401
    batch = _batch(_images())
    tab = _plan(3, 2).tab
    V = len(tab)
    tab_d = torch.from_numpy(tab).cuda()
    fill_d = batch.mean_colour()
    got = batch.occluded(tab_d, 0, V, fill_d, 14, 40)                    # the identity branch of the 14 x 40 image, out_h != out_w
    want = _occluded_copies(tab, fill_d.cpu().numpy()).resized(14, 40)
    assert torch.equal(got, want)
    for bad in (tab_d.long(), tab_d[:, :4].contiguous(), tab_d.cpu(), tab_d.t().contiguous().t()):
        with pytest.raises(ValueError, match="tab_d"):
            batch.occluded(bad, 0, 1, fill_d, 13, 13)
    for lo, hi in ((0, 0), (-1, 2), (0, V + 1), (3, 2)):
        with pytest.raises(ValueError, match="rows"):
            batch.occluded(tab_d, lo, hi, fill_d, 13, 13)
    for bad in (fill_d.int(), fill_d[:, :3].contiguous(), fill_d[:3].contiguous(), fill_d.cpu()):
        with pytest.raises(ValueError, match="fill_d"):
            batch.occluded(tab_d, 0, 1, bad, 13, 13)
    with pytest.raises(ValueError, match="dtype"):
        batch.occluded(tab_d, 0, 1, fill_d, 13, 13, 8, torch.float64)
    # a row outside its image (not one ``occlusion_plan`` makes) reads nothing and gives a zero output: image index, rectangle past
    # the image's own height (still inside the slot), negative origin, reversed rectangle
    off = torch.tensor([[0, 0, 0, 5, 5, 0, 0, 0], [4, 0, 0, 5, 5, 0, 0, 0], [-1, 0, 0, 5, 5, 0, 0, 0], [1, 0, 0, 15, 5, 0, 0, 0],
                        [1, 0, -1, 5, 5, 0, 0, 0], [2, 6, 0, 5, 5, 0, 0, 0], [2, 0, 0, 5, 17, 0, 0, 0]], dtype=torch.int32, device="cuda")
    for dtype in (torch.float16, torch.float32):
        got = batch.occluded(off, 0, 7, fill_d, 13, 16, 8, dtype)
        torch.cuda.synchronize()
        assert got[0].abs().max().item() > 0 and got[1:].abs().max().item() == 0.0


# ---- cells, statistics, maps ----------------------------------------------------------------------------------------------------------
def _cells_ref(scores, plain, seg, G, K, thr):
    """numpy fp32 restatement, in the stated order: delta = plain - score; per cell the windows covering it row-major, a sequential sum,
    one division"""
    R, n, W = scores.shape[0], len(seg) - 1, G - K + 1
    cells = np.full((R, n, G, G), np.nan, np.float32)
    stats = np.full((R, n, 4), np.nan, np.float32)
    for r in range(R):
        for i in range(n):
            lo, hi = int(seg[i]), int(seg[i + 1])
            if hi == lo:
                continue
            d = (plain[r, i] - scores[r, lo:hi]).astype(np.float32)
            for gy in range(G):
                for gx in range(G):
                    acc, cnt = np.float32(0), 0
                    for wy in range(max(0, gy - K + 1), min(gy, W - 1) + 1):
                        for wx in range(max(0, gx - K + 1), min(gx, W - 1) + 1):
                            acc = np.float32(acc + d[wy * W + wx])
                            cnt += 1
                    cells[r, i, gy, gx] = acc / np.float32(cnt)
            flips = int(((scores[r, lo:hi] > np.float32(thr)) != (plain[r, i] > np.float32(thr))).sum())
            stats[r, i] = (d.max(), d.min(), np.float32(int(d.argmax())), np.float32(flips))
    return cells, stats


def _map_ref(cells_row, sizes, maxH, maxW, G):
    out = np.zeros((len(sizes), maxH, maxW), np.float32)
    for i, (h, w) in enumerate(sizes):
        cy = np.zeros(h, np.int64)
        cx = np.zeros(w, np.int64)
        for g in range(G):
            cy[(g * h) // G:((g + 1) * h) // G] = g
            cx[(g * w) // G:((g + 1) * w) // G] = g
        out[i, :h, :w] = cells_row[i][cy][:, cx]
    return out


@pytest.mark.parametrize("grid,window", [(5, 2), (4, 4)], ids=["g5k2", "g4k4"])
def test_cells_stats_and_maps_against_numpy(grid, window):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops, pipeline
    sizes = [(13, 13), (3, 50), (29, 16), (40, 37)]                      # image 1 is lower than either grid: no variants
    plan = pipeline.occlusion_plan(sizes, grid, window)
    per = (grid - window + 1) ** 2
    assert plan.seg.tolist() == [0, per, per, 2 * per, 3 * per] and plan.skipped == [1]
    rng = np.random.default_rng(13)
    rows, n, V, thr = 3, 4, 3 * per, 0.487
    scores = rng.random((rows, V), dtype=np.float32)
    plain = rng.random((rows, n), dtype=np.float32)
    plain[1, 0] = np.float32(thr)                                        # exactly the threshold: not above it
    scores[1, 0] = np.float32(thr)
    scores[2, 2 * per:] = plain[2, 3]                                    # row 2, image 3: every delta is 0
    if per > 2:
        scores[0, per + 2] = scores[0, per + 1] = scores[0, per:2 * per].min()      # a tie for the largest delta: the first one is reported
    cells, stats = ops.occlusion_cells(torch.from_numpy(scores).cuda(), torch.from_numpy(plain).cuda(), plan.seg, grid, window, thr)
    torch.cuda.synchronize()
    want_c, want_s = _cells_ref(scores, plain, plan.seg, grid, window, thr)
    assert cells.shape == (rows, n, grid, grid) and stats.shape == (rows, n, 4) and cells.dtype == stats.dtype == torch.float32
    got_c, got_s = cells.cpu().numpy(), stats.cpu().numpy()
    assert np.isnan(got_c[:, 1]).all() and np.isnan(got_s[:, 1]).all() and not np.isnan(np.delete(got_c, 1, axis=1)).any()
    assert np.array_equal(got_c, want_c, equal_nan=True), np.abs(got_c - want_c).max()
    assert np.array_equal(got_s, want_s, equal_nan=True), (got_s, want_s)
    assert (got_c[2, 3] == 0).all() and got_s[2, 3].tolist() == [0.0, 0.0, 0.0, 0.0]
    # no variants at all: nothing is launched, everything is NaN
    none_c, none_s = ops.occlusion_cells(torch.zeros((rows, 0), device="cuda"), torch.from_numpy(plain).cuda(), np.zeros((n + 1,), np.int32),
                                         grid, window, thr)
    assert none_c.shape == (rows, n, grid, grid) and torch.isnan(none_c).all() and torch.isnan(none_s).all()
    # full-size maps: the slots are larger than every image
    maxH, maxW = 43, 53
    sizes_d = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    for r in range(rows):
        f32 = ops.occlusion_map(cells[r], sizes_d, (maxH, maxW), out="f32").cpu().numpy()
        want = _map_ref(want_c[r], sizes, maxH, maxW, grid)
        assert f32.shape == (n, maxH, maxW) and np.array_equal(f32, want, equal_nan=True), r
        u8 = ops.occlusion_map(cells[r], sizes_d, (maxH, maxW), out="u8").cpu().numpy()
        assert u8.dtype == np.uint8
        for i, (h, w) in enumerate(sizes):
            assert (u8[i, h:] == 0).all() and (u8[i, :, w:] == 0).all()
            peak = np.abs(want_c[r, i]).max()
            if np.isnan(peak) or peak == 0:
                assert (u8[i, :h, :w] == 128).all(), (r, i)              # the skipped image, and row 2's image without any effect
                continue
            ref = np.float32(255) * (np.float32(0.5) + np.float32(0.5) * (want[i, :h, :w] / np.float32(peak)))
            assert np.abs(u8[i, :h, :w].astype(np.float32) - ref).max() <= 1.0, (r, i)
            assert u8[i, :h, :w].max() == 255 or u8[i, :h, :w].min() == 0    # the peak itself is at one end of the scale
    assert np.isnan(want_c[0, 1]).all() and (want_c[2, 3] == 0).all()      # both 128 cases were met above


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(px)).save(buf, format="PNG")
    return buf.getvalue()


def _csv(d, names):
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return str(d / "test.csv")


@pytest.mark.parametrize("precision", ["fast", "strict"])
def test_cli_occlusion_end_to_end(tmp_path, precision):
    """four synthetic 200 x 200 PNGs and four flat PNGs of their mean colours, plain and under a one-window grid; then the flat files,
    a 5 x 300 strip and one synthetic image at the default grid"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, main as cli, zoo
    keys = ("resnet_rs50", "vit_tiny_patch16_224")                       # a 200 x 200 member and a 224 x 224 ViT
    members = [zoo.MEMBERS[k].name for k in keys]
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4", "--precision", precision]
    px = [synth_pixels(i) for i in range(4)]
    colours = [_mean_rule(p)[:3] for p in px]
    flat = [np.broadcast_to(c, (200, 200, 3)).copy() for c in colours]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    names_a = [f"s{k}.png" for k in range(4)] + [f"flat{k}.png" for k in range(4)]
    for k in range(4):
        (a / f"s{k}.png").write_bytes(_png(px[k]))
        (a / f"flat{k}.png").write_bytes(_png(flat[k]))
        (b / f"flat{k}.png").write_bytes(_png(flat[k]))
    (b / "strip.png").write_bytes(_png(px[0][:5, :].repeat(2, axis=1)[:, :300]))         # 5 x 300: lower than the grid of 8
    (b / "s0.png").write_bytes(_png(px[0]))
    names_b = [f"flat{k}.png" for k in range(4)] + ["strip.png", "s0.png"]
    csv_a, csv_b = _csv(a, names_a), _csv(b, names_b)
    thr = np.float32(ensemble.THR)

    cli.main([csv_a, str(a / "o0.csv"), "--scores-out", str(a / "s0.csv"), *extra])
    cli.main([csv_a, str(a / "o1.csv"), "--scores-out", str(a / "s1.csv"), *extra, "--occlusion", str(a / "occ"), "--occlusion-grid", "2",
              "--occlusion-window", "2", "--occlusion-members"])
    # (c) the outputs of a plain run do not change
    assert (a / "o0.csv").read_bytes() == (a / "o1.csv").read_bytes()
    assert (a / "s0.csv").read_bytes() == (a / "s1.csv").read_bytes()
    plain = pd.read_csv(a / "s0.csv").set_index("filename")
    # (a) one variant per image, the whole image at its mean colour: the members see what they see of the flat file
    for k in range(4):
        z = np.load(a / "occ" / f"s{k}.members.npz")
        assert z["rects"].tolist() == [[0, 0, 200, 200]]
        for m in members:
            assert z[f"{m}/variants"].shape == (1,) and z[f"{m}/cells"].shape == (2, 2)
            assert z[f"{m}/variants"][0] == np.float32(plain.loc[f"flat{k}.png", m]), (k, m)
            assert z[f"{m}/p"] == np.float32(plain.loc[f"s{k}.png", m])
            assert (z[f"{m}/cells"] == np.float32(z[f"{m}/p"] - z[f"{m}/variants"][0])).all()
        rows = np.array([z[f"{m}/variants"][0] for m in members], np.float32)
        assert z["ensemble/variants"][0] == (rows[0] + rows[1]) / np.float32(2)
        full = np.load(a / "occ" / f"s{k}.npy")
        assert full.shape == (200, 200) and full.dtype == np.float32 and (full == z["ensemble/cells"][0, 0]).all()
    # (d) the report follows from the per-variant scores
    table = pd.read_csv(a / "occ" / "occlusion.csv")
    assert list(table.columns) == ["filename", "width", "height", "variants", "p", "decision", "delta_max", "delta_min", "cell_max", "flips"]
    assert table.filename.tolist() == sorted(names_a) and table.variants.tolist() == [1] * 8
    assert table.width.tolist() == [200] * 8 and table.height.tolist() == [200] * 8
    for _, row in table.iterrows():
        z = np.load(a / "occ" / (os.path.splitext(row.filename)[0] + ".members.npz"))
        p, v = np.float32(z["ensemble/p"]), z["ensemble/variants"]
        assert np.float32(row.p) == np.float32(plain.loc[row.filename, "ensemble_mean"]) == p
        assert np.float32(row.delta_max) == np.float32(row.delta_min) == np.float32(p - v[0]) and row.cell_max == "0,0"
        assert row.flips == float((v[0] > thr) != (p > thr))
    info = json.loads((a / "occ" / "occlusion.json").read_text())
    assert info["n_files"] == 8 and info["n_skipped"] == 0 and info["skipped"] == [] and info["variants_per_image"] == 1
    assert info["flipped"] == [n for n, f in zip(table.filename, table.flips) if f > 0]

    cli.main([csv_b, str(b / "o.csv"), "--scores-out", str(b / "s.csv"), *extra, "--occlusion", str(b / "occ"), "--occlusion-members"])
    table = pd.read_csv(b / "occ" / "occlusion.csv")
    assert table.filename.tolist() == sorted(names_b) == ["flat0.png", "flat1.png", "flat2.png", "flat3.png", "s0.png", "strip.png"]
    assert table.variants.tolist() == [49, 49, 49, 49, 49, 0]
    # (b) a flat image at its own mean colour is the image again: every variant is the plain input
    for k in range(4):
        z = np.load(b / "occ" / f"flat{k}.members.npz")
        for m in members + ["ensemble"]:
            assert z[f"{m}/variants"].shape == (49,) and (z[f"{m}/variants"] == z[f"{m}/p"]).all(), (k, m)
            assert (z[f"{m}/cells"] == 0).all()
        full = np.load(b / "occ" / f"flat{k}.npy")
        assert full.shape == (200, 200) and (full == 0).all()
        assert table.delta_max[k] == 0 and table.delta_min[k] == 0 and table.flips[k] == 0 and table.cell_max[k] == "0,0"
    # (d) again, on an image with 49 different variants: cells, map, report
    z = np.load(b / "occ" / "s0.members.npz")
    p, v = np.float32(z["ensemble/p"]), z["ensemble/variants"]
    rows = np.stack([z[f"{m}/variants"] for m in members])
    assert np.array_equal(v, (rows[0] + rows[1]) / np.float32(2)) and len(set(v.tolist())) > 1
    assert z["rects"].shape == (49, 4) and z["rects"][0].tolist() == [0, 0, 50, 50] and z["rects"][-1].tolist() == [150, 150, 200, 200]
    seg = np.array([0, 49], np.int32)
    for m in members + ["ensemble"]:
        want_c, _ = _cells_ref(z[f"{m}/variants"][None], np.float32(z[f"{m}/p"]).reshape(1, 1), seg, 8, 2, thr)
        assert np.array_equal(z[f"{m}/cells"], want_c[0, 0]), m
    full = np.load(b / "occ" / "s0.npy")
    assert np.array_equal(full, _map_ref(z["ensemble/cells"][None], [(200, 200)], 200, 200, 8)[0])
    d = (p - v).astype(np.float32)
    row = table.iloc[4]
    assert np.float32(row.delta_max) == d.max() and np.float32(row.delta_min) == d.min()
    assert row.cell_max == f"{int(d.argmax()) // 7},{int(d.argmax()) % 7}"
    assert row.flips == float(((v > thr) != (p > thr)).sum())
    # (e) the strip is lower than the grid: listed, skipped, empty columns
    strip = table.iloc[5]
    assert strip.width == 300 and strip.height == 5 and strip.variants == 0
    assert np.isnan(strip.delta_max) and np.isnan(strip.delta_min) and np.isnan(strip.flips) and pd.isna(strip.cell_max)
    assert not np.isnan(strip.p)
    zs = np.load(b / "occ" / "strip.members.npz")
    assert zs["ensemble/variants"].shape == (0,) and np.isnan(zs["ensemble/cells"]).all()
    # (f) the settings, and both members - the ViT included - are named
    info = json.loads((b / "occ" / "occlusion.json").read_text())
    assert info["n_files"] == 6 and info["n_explained"] == 5 and info["n_skipped"] == 1 and info["skipped"] == ["strip.png"]
    assert info["settings"]["members"] == members and any("vit" in m.lower() for m in info["settings"]["members"])
    assert info["settings"]["grid"] == 8 and info["settings"]["window"] == 2 and info["settings"]["fill"] == "mean"
    assert info["settings"]["format"] == "npy" and info["settings"]["precision"] == precision and info["settings"]["batch_size"] == 4
    assert info["variants_per_image"] == 49 and info["flipped"] == [n for n, f in zip(table.filename, table.flips) if f > 0]
