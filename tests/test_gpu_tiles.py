"""GPU: native-resolution tile scoring.  The gather kernel (``DecodedBatch.tiles``) against the parent pipeline on stand-alone crops
(``DecodedBatch.resized``: exact), against numpy on the identity branch (exact) and against the oracle's resize on the bicubic branch;
the aggregation kernel against numpy; and ``main.py --tiles-out`` on a 400 x 400 PNG made of four 200 x 200 images against a plain run on
the four files - the tile batch and the plain batch are then the same tensors, so the per-tile scores are the plain scores, exactly."""
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
from oracle import ops_ref as R  # noqa: E402
from tests._jpeg_enc_ref import content  # noqa: E402
from tools.make_synth import synth_pixels  # noqa: E402

SIZES = [(13, 13), (14, 40), (29, 16), (40, 37)]                       # (height, width)
CASES = [(13, 13), (16, 16), (13, 16), (16, 13), (13, 8)]             # (tile, network input side)


@functools.lru_cache(maxsize=None)
def _images():
    out = [content(71 + k, w, h) for k, (h, w) in enumerate(SIZES)]
    for px in out:
        px.setflags(write=False)
    return tuple(out)


def _batch(imgs, pad: int = 3):
    """a DecodedBatch holding ``imgs`` in slots of the largest size + pad, the rest of every slot filled with noise (as
    tests/test_gpu_resample.py builds it): a tile that read past its own edge would pick the noise up"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    sizes = [(im.shape[0], im.shape[1]) for im in imgs]
    maxH, maxW = max(h for h, _ in sizes) + pad, max(w for _, w in sizes) + pad
    rgb = np.random.default_rng(5).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


@functools.lru_cache(maxsize=None)
def _tab(tile: int, stride: int):
    """the table ``tile_plan`` would make, also for tiles below its smallest size (16): (tab int32 [T, 4], crops uint8 [T, tile, tile, 3])"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    rows, crops = [], []
    for i, im in enumerate(_images()):
        h, w = im.shape[:2]
        if h < tile or w < tile:
            continue
        ys = pipeline._tile_positions(h, tile, -(-(h - tile) // stride) + 1)
        xs = pipeline._tile_positions(w, tile, -(-(w - tile) // stride) + 1)
        for y in ys:
            for x in xs:
                rows.append((i, y, x, 0))
                crops.append(im[y:y + tile, x:x + tile])
    tab = np.asarray(rows, np.int32)
    if tile >= 16:
        plan = pipeline.tile_plan(SIZES, tile, stride, 4096)
        assert np.array_equal(plan.tab, tab)
    return tab, np.stack(crops)


@functools.lru_cache(maxsize=None)
def _crop_batch(tile: int, stride: int):
    """the tiles as stand-alone images: what the parent's ``resized`` sees"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    _, crops = _tab(tile, stride)
    T = len(crops)
    return pipeline.DecodedBatch(torch.from_numpy(crops.copy()).cuda(), torch.tensor([[tile, tile]] * T, dtype=torch.int32, device="cuda"),
                                 [(tile, tile)] * T)


def test_the_tables_hold_the_cases_the_kernel_can_get_wrong():
    tab, _ = _tab(13, 5)
    assert {int(x) % 4 for x in tab[:, 2]} == {0, 1, 2, 3}                                   # source rows at every byte alignment
    assert len(tab) % 256 and len(tab) % 64 and len(tab) > 64
    for tile in (13, 16):
        for stride in (5, tile):
            tab, _ = _tab(tile, stride)
            right = [r for r in tab if r[2] + tile == SIZES[r[0]][1] and SIZES[r[0]][1] < 37]     # at an image's edge, inside a wider slot
            bottom = [r for r in tab if r[1] + tile == SIZES[r[0]][0] and SIZES[r[0]][0] < 40]
            assert right and bottom, (tile, stride)


@pytest.mark.parametrize("tile,out", CASES, ids=[f"{t}to{o}" for t, o in CASES])
def test_gather_equals_resized_on_stand_alone_crops(tile, out, report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    batch = _batch(_images())
    before = batch.rgb.clone()
    for stride in (5, tile):
        tab, crops = _tab(tile, stride)
        T = len(tab)
        tab_d = torch.from_numpy(tab).cuda()
        alone = _crop_batch(tile, stride)
        for c_out in (8, 4):
            for dtype in (torch.float16, torch.float32) + ((ops.PACKED,) if c_out == 8 else ()):
                got = batch.tiles(tab_d, 0, T, tile, out, c_out, dtype)
                want = alone.resized(out, out, c_out, dtype)
                torch.cuda.synchronize()
                assert got.shape == (T, out, out, c_out) and got.dtype == dtype
                assert torch.equal(got, want), (tile, out, stride, c_out, dtype, int((got != want).sum()))
                if dtype != ops.PACKED:
                    assert got[..., 3:].abs().max().item() == 0.0
                # a sub-range of the table (how ``tile_batch`` walks it in chunks) gives the same rows
                part = torch.cat([batch.tiles(tab_d, 0, 5, tile, out, c_out, dtype), batch.tiles(tab_d, 5, T, tile, out, c_out, dtype)])
                assert torch.equal(part, got)
                if dtype == ops.PACKED:
                    assert torch.equal(got, ops.pack_h2(batch.tiles(tab_d, 0, T, tile, out, c_out, torch.float32)))     # the fp32 values, split once
                    continue
                if tile == out:                             # identity branch: p / 255, rounded once
                    ref = crops.astype(np.float32) / np.float32(255)
                    ref = ref.astype(np.float16) if dtype == torch.float16 else ref
                    assert np.array_equal(got[..., :3].cpu().numpy(), ref), (tile, stride, c_out, dtype)
                elif dtype == torch.float16 and c_out == 8:  # bicubic branch against the oracle, at test_gpu_pipeline's tolerance
                    g = got[..., :3].float().cpu()
                    worst = max((g[t] - R.decode_resize_normalize(crops[t], out, out).to(torch.float16).float()).abs().max().item()
                                for t in range(T))
                    report(f"[tiles] gather {tile} -> {out} stride {stride}: {T} tiles, max |hip - oracle| = {worst:.3e} (fp16 values)")
                    assert worst <= 1e-3, (tile, out, stride, worst)
    assert torch.equal(batch.rgb, before), "tiles() changed its input"


def test_gather_refuses_a_table_it_cannot_use():
    import vipcup_amd  # noqa: F401
    batch = _batch(_images())
    tab, _ = _tab(13, 13)
    tab_d = torch.from_numpy(tab).cuda()
    for bad in (tab_d.long(), tab_d[:, :3].contiguous(), tab_d.cpu(), tab_d.t().contiguous().t()):
        with pytest.raises(ValueError, match="tab_d"):
            batch.tiles(bad, 0, 1, 13, 13)
    for lo, hi in ((0, 0), (-1, 2), (0, len(tab) + 1), (3, 2)):
        with pytest.raises(ValueError, match="rows"):
            batch.tiles(tab_d, lo, hi, 13, 13)
    with pytest.raises(ValueError, match="does not fit"):
        batch.tiles(tab_d, 0, 1, 44, 13)                  # the slots are 43 x 43
    # a row outside the slot (not one ``tile_plan`` makes) reads nothing and gives a zero tile
    off = torch.tensor([[0, 0, 0, 0], [1, 40, 0, 0], [1, 0, -1, 0], [0, 31, 28, 0]], dtype=torch.int32, device="cuda")
    got = batch.tiles(off, 0, 4, 13, 16)
    assert got[0].abs().max().item() > 0 and got[1:].abs().max().item() == 0.0


def test_aggregate_against_numpy():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    rng = np.random.default_rng(11)
    rows, T = 4, 37
    seg = np.array([0, 9, 9, 20, 36, 37], np.int32)                      # image 1 has no tiles, image 4 one
    thr = 0.487
    s = rng.random((rows, T), dtype=np.float32)
    s[1, 3] = s[2, 12] = np.float32(thr)                                 # exactly the threshold: not above it
    s[0, 9:20] = 1.0
    s[3, 20:36] = 0.0
    got = ops.tile_aggregate(torch.from_numpy(s).cuda(), torch.from_numpy(seg).cuda(), thr).cpu().numpy()
    assert got.shape == (3, rows, 5) and got.dtype == np.float32
    assert np.isnan(got[:, :, 1]).all() and not np.isnan(np.delete(got, 1, axis=2)).any()
    for i in (0, 2, 3, 4):
        lo, hi = int(seg[i]), int(seg[i + 1])
        part = s[:, lo:hi]
        err = np.abs(got[0, :, i].astype(np.float64) - part.astype(np.float64).mean(axis=1)).max()
        assert err <= (hi - lo) * 2.0 ** -24, (i, err)                   # values in [0, 1], a sequential fp32 sum, one division
        assert np.array_equal(got[1, :, i], part.max(axis=1))
        above = (part > np.float32(thr)).sum(axis=1)
        assert np.array_equal(got[2, :, i], above.astype(np.float32) / np.float32(hi - lo))
    assert got[0, 0, 2] == 1.0 and got[2, 0, 2] == 1.0 and got[0, 3, 3] == 0.0 and got[2, 3, 3] == 0.0
    # no tiles at all: nothing is launched, every image reports NaN
    none = ops.tile_aggregate(torch.zeros((rows, 0), device="cuda"), torch.zeros((6,), dtype=torch.int32, device="cuda"), thr)
    assert none.shape == (3, rows, 5) and torch.isnan(none).all()


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(px)).save(buf, format="PNG")
    return buf.getvalue()


def _csv(d, names):
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return str(d / "test.csv")


@pytest.mark.parametrize("precision", ["fast", "strict"])
def test_cli_tiles_end_to_end(tmp_path, precision):
    """one 400 x 400 PNG of four synthetic 200 x 200 images (plus two files that are not tiled) under --tiles-out, against a plain run on
    the four images as files of their own at the same batch size"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, main as cli, zoo
    keys = ("resnet_rs50", "vit_tiny_patch16_224")                       # a 200 x 200 member and a 224 x 224 one
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    extra = ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4", "--precision", precision]
    px = [synth_pixels(i) for i in range(7)]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    big = np.concatenate([np.concatenate([px[0], px[1]], axis=1), np.concatenate([px[2], px[3]], axis=1)], axis=0)
    (a / "big.png").write_bytes(_png(big))
    (a / "small.png").write_bytes(_png(px[4]))                            # exactly one tile: scored the plain way only
    (a / "odd.png").write_bytes(_png(np.concatenate([px[5][:150], px[6][:150, :100]], axis=1)))      # 150 x 300: lower than a tile
    names_a = ["big.png", "small.png", "odd.png"]
    names_b = [f"t{k}.png" for k in range(4)]
    for k, name in enumerate(names_b):
        (b / name).write_bytes(_png(px[k]))
    csv_a, csv_b = _csv(a, names_a), _csv(b, names_b)
    cli.main([csv_a, str(a / "o0.csv"), "--scores-out", str(a / "s0.csv"), *extra])
    cli.main([csv_a, str(a / "o1.csv"), "--scores-out", str(a / "s1.csv"), *extra, "--tiles-out", str(a / "t.csv")])
    cli.main([csv_b, str(b / "o.csv"), "--scores-out", str(b / "s.csv"), *extra])
    # the outputs of a plain run do not change
    assert (a / "o0.csv").read_bytes() == (a / "o1.csv").read_bytes()
    assert (a / "s0.csv").read_bytes() == (a / "s1.csv").read_bytes()
    # per tile: the member columns are the plain scores of the four files
    long_form = pd.read_csv(a / "t.tiles.csv")
    plain_b = pd.read_csv(b / "s.csv")
    members = [zoo.MEMBERS[k].name for k in keys]
    assert list(long_form.columns) == ["filename", "ty", "tx", "y0", "x0", "p"] + members
    assert long_form.filename.tolist() == ["big.png"] * 4
    assert long_form[["ty", "tx", "y0", "x0"]].values.tolist() == [[0, 0, 0, 0], [0, 1, 0, 200], [1, 0, 200, 0], [1, 1, 200, 200]]
    for m in members:
        assert np.array_equal(long_form[m].to_numpy(np.float32), plain_b[m].to_numpy(np.float32)), (m, long_form[m], plain_b[m])
    rows = np.stack([plain_b[m].to_numpy(np.float32) for m in members])
    p = long_form.p.to_numpy(np.float32)
    assert np.array_equal(p, (rows[0] + rows[1]) / np.float32(2))
    # per file: the report follows from the tile scores
    table = pd.read_csv(a / "t.csv")
    assert list(table.columns) == ["filename", "width", "height", "tiles", "grid", "p", "decision", "p_tiles_mean", "p_tiles_max",
                                   "frac_tiles", "decision_tiles", "agrees"]
    assert table.filename.tolist() == sorted(names_a) == ["big.png", "odd.png", "small.png"]
    assert table.width.tolist() == [400, 300, 200] and table.height.tolist() == [400, 150, 200]
    assert table.tiles.tolist() == [4, 0, 0] and table.grid.tolist() == ["2x2", "0x0", "0x0"]
    s0 = pd.read_csv(a / "s0.csv")
    uniq, p_plain, dec = ensemble.aggregate(s0.filename.tolist(), np.stack([s0[m].to_numpy(np.float32) for m in members]))
    assert uniq == table.filename.tolist()
    assert np.array_equal(table.p.to_numpy(np.float32), p_plain) and np.array_equal(table.decision.to_numpy(np.float32), dec)
    mean = (((p[0] + p[1]) + p[2]) + p[3]) / np.float32(4)                # the kernel's sum: sequential, fp32
    above = int((p > np.float32(ensemble.THR)).sum())
    assert np.float32(table.p_tiles_mean[0]) == mean and np.float32(table.p_tiles_max[0]) == p.max()
    assert np.float32(table.frac_tiles[0]) == np.float32(above) / np.float32(4)
    assert table.decision_tiles[0] == float(mean > np.float32(ensemble.THR))
    assert table[["p_tiles_mean", "p_tiles_max", "frac_tiles"]].iloc[1:].isna().all().all()
    assert table.decision_tiles[1:].tolist() == table.decision[1:].tolist()
    assert table.agrees.tolist() == [int(x == y) for x, y in zip(table.decision_tiles, table.decision)]
    info = json.loads((a / "t.json").read_text())
    assert info["n_files"] == 3 and info["n_tiled"] == 1 and info["n_untiled"] == 2 and info["thinned"] == []
    assert info["disagreements"] == [n for n, ok in zip(table.filename, table.agrees) if not ok]
    assert info["settings"]["tile"] == 200 and info["settings"]["stride"] == 200 and info["settings"]["max_tiles"] == 256
    assert info["settings"]["tile_agg"] == "mean" and info["settings"]["precision"] == precision and info["settings"]["members"] == members
    assert info["tiles_file"] == "t.tiles.csv"
