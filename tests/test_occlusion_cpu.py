"""CPU: the host side of occlusion evidence maps (``main.py --occlusion``) - ``pipeline.occlusion_plan`` against a brute-force
restatement of its definition, ``ensemble.occlusion_table`` on hand-made arrays, the entry points' argument checks and the refusals of
the CLI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(13, 13), (14, 40), (29, 16), (40, 37), (4, 50)]              # tests/test_gpu_tiles.py's sizes plus one lower than a grid of 5
GRIDS = [(3, 2), (5, 1), (4, 4), (5, 2)]                               # (grid, window)


def _pipeline():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    return pipeline


def _cell_of_pixels(length, grid):
    """per pixel of an axis its cell, from the definition alone: cell g covers [(g L) // G, ((g + 1) L) // G)"""
    out = np.full(length, -1, np.int64)
    for g in range(grid):
        for p in range((g * length) // grid, ((g + 1) * length) // grid):
            assert out[p] == -1                                          # cells do not overlap
            out[p] = g
    return out


@pytest.mark.parametrize("grid,window", GRIDS, ids=[f"g{g}k{k}" for g, k in GRIDS])
def test_plan_against_a_brute_force_restatement(grid, window):
    P = _pipeline()
    plan = P.occlusion_plan(SIZES, grid, window)
    tab, seg = plan                                                      # unpacks as the pair
    assert tab.dtype == np.int32 and seg.dtype == np.int32 and tab.ndim == 2 and tab.shape[1] == 8 and seg.shape == (len(SIZES) + 1,)
    assert plan.grid == grid and plan.window == window and plan.sizes == SIZES
    per = grid - window + 1
    want_rows, want_seg, want_skipped = [], [0], []
    for i, (h, w) in enumerate(SIZES):
        if h < grid or w < grid:
            want_skipped.append(i)
        else:
            for wy in range(per):
                for wx in range(per):
                    want_rows.append((i, (wy * h) // grid, (wx * w) // grid, ((wy + window) * h) // grid, ((wx + window) * w) // grid, 0, 0, 0))
        want_seg.append(len(want_rows))
    assert tab.shape[0] == len(want_rows) and tab.tolist() == [list(r) for r in want_rows]     # row count and order
    assert seg.tolist() == want_seg and plan.skipped == want_skipped
    assert plan.skipped == ([4] if grid == 5 else [])                    # (4, 50) has no row of cells for a grid of 5
    for i, (h, w) in enumerate(SIZES):
        rows = tab[seg[i]:seg[i + 1]]
        if i in plan.skipped:
            assert len(rows) == 0
            continue
        assert len(rows) == per * per and (rows[:, 0] == i).all()
        cy, cx = _cell_of_pixels(h, grid), _cell_of_pixels(w, grid)
        assert (cy >= 0).all() and (cx >= 0).all()                        # the union of the cells is the whole image
        assert len(set(cy.tolist())) == grid and len(set(cx.tolist())) == grid      # and no cell is empty
        cover = np.zeros((h, w), np.int64)
        for _, y0, x0, y1, x1, *_ in rows.tolist():
            assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w
            cover[y0:y1, x0:x1] += 1
        # a cell is covered by the windows whose offset lies in [g - window + 1, g], cut to 0 .. grid - window: per axis
        per_axis = np.array([min(g, per - 1) - max(g - window + 1, 0) + 1 for g in range(grid)])
        assert per_axis.max() <= window and per_axis.min() >= 1
        assert np.array_equal(cover, per_axis[cy][:, None] * per_axis[cx][None, :])
        # a window's edges are cell edges: all pixels of a cell are hidden together
        for _, y0, x0, y1, x1, *_ in rows.tolist():
            assert set(cy[y0:y1].tolist()).isdisjoint(cy[:y0].tolist() + cy[y1:].tolist())
            assert set(cx[x0:x1].tolist()).isdisjoint(cx[:x0].tolist() + cx[x1:].tolist())


def test_the_tables_hold_every_source_alignment():
    P = _pipeline()
    seen = set()
    for grid, window in GRIDS:
        tab = P.occlusion_plan(SIZES, grid, window).tab
        seen |= {(int(x0) * 3) % 4 for x0 in tab[:, 2]}
    assert seen == {0, 1, 2, 3}                                           # the byte offsets x0 * 3 of the rectangles' first pixels
    one = P.occlusion_plan(SIZES, 5, 1).tab
    assert {(int(x0) * 3) % 4 for x0 in one[:, 2]} == {0, 1, 2, 3}
    empty = P.occlusion_plan([(1, 9), (9, 1)])
    assert empty.tab.shape == (0, 8) and empty.seg.tolist() == [0, 0, 0] and empty.skipped == [0, 1]
    assert P.occlusion_plan([(200, 200)]).tab.shape == (49, 8)            # the defaults: 8 x 8 cells, 2 x 2 windows
    assert P.occlusion_bounds(200, 8) == [0, 25, 50, 75, 100, 125, 150, 175, 200] and P.occlusion_bounds(5, 3) == [0, 1, 3, 5]


@pytest.mark.parametrize("kwargs", [dict(grid=1), dict(grid=33), dict(grid=8.0), dict(grid="8"), dict(grid=True), dict(grid=None),
                                    dict(window=0), dict(window=9), dict(window=1.5), dict(grid=4, window=5), dict(window=None)])
def test_plan_arguments_are_checked(kwargs):
    P = _pipeline()
    with pytest.raises(ValueError, match="expected an integer in"):
        P.occlusion_plan([(50, 50)], **kwargs)


def test_occlusion_table_on_hand_made_arrays():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    P = _pipeline()
    names = ["b.png", "a.png", "c.png", "a.png", "d.png"]                    # a.png twice; c.png is too low for the grid
    sizes = [(40, 60), (30, 30), (3, 300), (30, 30), (20, 20)]
    plan = P.occlusion_plan(sizes, 4, 2)                                    # 3 x 3 windows
    plain = np.array([[0.9, 0.2, 0.6, 0.4, 0.1], [0.7, 0.4, 0.6, 0.2, 0.3]], np.float32)
    nan = np.float32("nan")
    stats = np.zeros((3, 5, 4), np.float32)
    stats[2, :, 0] = [0.50, 0.10, nan, 0.30, 0.00]                          # ensemble row: largest delta
    stats[2, :, 1] = [-0.10, -0.20, nan, 0.00, 0.00]                        # smallest
    stats[2, :, 2] = [5, 8, nan, 0, 0]                                      # variant index of the largest
    stats[2, :, 3] = [3, 0, nan, 1, 0]                                      # flips
    table, summary = ensemble.occlusion_table(names, plain, stats, plan, 0.487)
    assert list(table) == ["filename", "width", "height", "variants", "p", "decision", "delta_max", "delta_min", "cell_max", "flips"]
    assert table["filename"] == ["a.png", "b.png", "c.png", "d.png"]
    assert table["width"] == [30, 60, 300, 20] and table["height"] == [30, 40, 3, 20]
    assert table["variants"] == [9, 9, 0, 9]
    np.testing.assert_allclose(table["p"], [0.3, 0.8, 0.6, 0.2], rtol=1e-6)
    assert table["decision"].tolist() == [0.0, 1.0, 1.0, 0.0]
    np.testing.assert_allclose(table["delta_max"][[0, 1, 3]], [0.20, 0.50, 0.0], rtol=1e-6)      # a.png: the mean of its two rows
    np.testing.assert_allclose(table["delta_min"][[0, 1, 3]], [-0.10, -0.10, 0.0], rtol=1e-6)
    np.testing.assert_allclose(table["flips"][[0, 1, 3]], [0.5, 3.0, 0.0])
    for key in ("delta_max", "delta_min", "flips"):
        assert np.isnan(table[key][2]) and table[key].dtype == np.float32
    assert table["cell_max"] == ["2,2", "1,2", "", "0,0"]                   # a.png: its first row's window, index 8 of 3 x 3
    assert summary["n_files"] == 4 and summary["n_explained"] == 3 and summary["n_skipped"] == 1 and summary["skipped"] == ["c.png"]
    assert summary["flipped"] == ["a.png", "b.png"] and summary["grid"] == 4 and summary["window"] == 2
    assert summary["variants_per_image"] == 9 and summary["threshold"] == pytest.approx(0.487)


def test_entry_points_check_arguments_without_a_gpu():
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    lib = _abi.lib()
    p = C.c_void_p(64)
    assert lib.vip_image_mean_u8(p, None, 4, 40, 40, p, None) == -1 and b"null" in lib.vip_last_error()
    assert lib.vip_image_mean_u8(p, p, 0, 40, 40, p, None) == -1 and b"bad size" in lib.vip_last_error()
    assert lib.vip_image_mean_u8(p, p, 4, 40, 40, C.c_void_p(66), None) == -2
    for fn in (lib.vip_occlude_resize_bicubic_norm_f16, lib.vip_occlude_resize_bicubic_norm_s32):
        assert fn(p, p, None, p, p, 4, 9, 40, 40, p, 16, 16, 8, None) == -1 and b"null" in lib.vip_last_error()
        assert fn(p, p, p, p, p, 4, 0, 40, 40, p, 16, 16, 8, None) == -1 and b"bad size" in lib.vip_last_error()
        assert fn(p, p, p, p, p, 4, 65536, 40, 40, p, 16, 16, 8, None) == -1
        assert fn(p, p, p, p, p, 0, 9, 40, 40, p, 16, 16, 8, None) == -1
        assert fn(p, p, p, p, p, 4, 9, 40, 40, p, 16, 16, 2, None) == -1
        assert fn(p, p, p, p, p, 4, 9, 40, 40, C.c_void_p(72), 16, 16, 8, None) == -2
        assert fn(p, p, C.c_void_p(66), p, p, 4, 9, 40, 40, p, 16, 16, 8, None) == -2
    cells = lib.vip_occlusion_cells_f32
    assert cells(p, p, None, 4, 3, 36, 4, 2, 0.5, p, p, None) == -1 and b"null" in lib.vip_last_error()
    assert cells(p, p, p, 4, 0, 36, 4, 2, 0.5, p, p, None) == -1 and b"bad dimension" in lib.vip_last_error()
    assert cells(p, p, p, 4, 3, 36, 33, 2, 0.5, p, p, None) == -1 and b"grid 33" in lib.vip_last_error()
    assert cells(p, p, p, 4, 3, 36, 4, 5, 0.5, p, p, None) == -1 and b"window 5" in lib.vip_last_error()
    assert lib.vip_occlusion_map(p, None, 4, 40, 40, 4, p, 0, None) == -1 and b"null" in lib.vip_last_error()
    assert lib.vip_occlusion_map(p, p, 4, 0, 40, 4, p, 0, None) == -1 and b"bad size" in lib.vip_last_error()
    assert lib.vip_occlusion_map(p, p, 4, 40, 40, 1, p, 1, None) == -1 and b"grid 1" in lib.vip_last_error()
    # a segment table that is not whole sets of windows is an argument error, found on the host copy before anything is launched
    scores, plain = torch.zeros((2, 18)), torch.zeros((2, 3))
    for seg in ([0, 9, 9, 17], [0, 9, 13, 18], [1, 10, 10, 19], [0, 9, 18, 27]):
        with pytest.raises(ValueError, match="occlusion_cells"):
            ops.occlusion_cells(scores, plain, np.asarray(seg, np.int32), 4, 2, 0.5)
    with pytest.raises(ValueError, match="seg must be"):
        ops.occlusion_cells(scores, plain, np.asarray([0, 9, 9, 18], np.int64), 4, 2, 0.5)
    with pytest.raises(ValueError, match="expected 2 <= grid"):
        ops.occlusion_cells(scores, plain, np.asarray([0, 9, 9, 18], np.int32), 4, 5, 0.5)
    with pytest.raises(ValueError, match="expected 'f32' or 'u8'"):
        ops.occlusion_map(torch.zeros((1, 4, 4)), torch.zeros((1, 2), dtype=torch.int32), (8, 8), out="f16")


def test_occlusion_batch_checks_its_settings_first():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    with pytest.raises(ValueError, match="chunk"):
        ensemble.occlusion_batch([], [], chunk=0)
    with pytest.raises(ValueError, match="fill 'blur'"):
        ensemble.occlusion_batch([], [], fill="blur")


REFUSALS = [
    (["--occlusion", "O", "--tta", "2"], "--occlusion works with --shard images and --tta 1 only"),
    (["--occlusion", "O", "--shard", "members"], "--occlusion works with --shard images and --tta 1 only"),
    (["--occlusion", "O", "--shard", "hybrid"], "--occlusion works with --shard images and --tta 1 only"),
    (["--occlusion", "O", "--heatmaps", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--occlusion", "O", "--stress-jpeg", "70", "--stress-out", "S"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--occlusion", "O", "--stress-resize", "50", "--stress-out", "S"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--occlusion", "O", "--stress-out", "S"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--occlusion", "O", "--tiles-out", "T"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--occlusion-grid", "4"], "need --occlusion DIR"),
    (["--occlusion-window", "1"], "need --occlusion DIR"),
    (["--occlusion-fill", "gray"], "need --occlusion DIR"),
    (["--occlusion-format", "png"], "need --occlusion DIR"),
    (["--occlusion-members"], "need --occlusion DIR"),
    (["--occlusion", "O", "--occlusion-grid", "1"], "--occlusion-grid 1: expected an integer in 2..32"),
    (["--occlusion", "O", "--occlusion-grid", "33"], "--occlusion-grid 33: expected an integer in 2..32"),
    (["--occlusion", "O", "--occlusion-window", "0"], "--occlusion-window 0: expected an integer in 1..8"),
    (["--occlusion", "O", "--occlusion-grid", "4", "--occlusion-window", "5"], "--occlusion-window 5: expected an integer in 1..4"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_touching_the_gpu(tmp_path, monkeypatch, extra, message):
    """every refusal is a SystemExit raised while the arguments are read: no file is opened or made and torch's GPU state is not asked for"""
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli

    def touched(*a, **k):
        raise AssertionError("the CLI reached the GPU set-up before refusing")
    for name in ("is_available", "set_device", "device_count", "init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    paths = {"O": "occ", "T": "tiles.csv", "S": "stress.csv", "H": "hm"}
    extra = [str(tmp_path / paths[t]) if t in paths else t for t in extra]
    with pytest.raises(SystemExit) as e:                  # the input CSV does not exist: it is never opened
        cli.main([str(tmp_path / "missing.csv"), str(tmp_path / "o.csv"), "--synthetic", *extra])
    assert message in str(e.value), e.value
    assert not os.listdir(tmp_path)
