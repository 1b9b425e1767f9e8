"""CPU: the host side of native-resolution tile scoring (``main.py --tiles-out``) - ``pipeline.tile_grid`` / ``tile_plan`` (pure
arithmetic), ``ensemble.tile_table`` on hand-made arrays, the entry points' argument checks and the refusals of the CLI."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _pipeline():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    return pipeline


def test_tile_grid_fixed_cases():
    P = _pipeline()
    assert P.tile_grid(200, 200) == ([0], [0])
    assert P.tile_grid(199, 5000) == ([], []) and P.tile_grid(5000, 199) == ([], [])
    assert P.tile_grid(401, 200) == ([0, 101, 201], [0])
    assert P.tile_grid(400, 400) == ([0, 200], [0, 200])
    assert P.tile_grid(400, 400, stride=100) == ([0, 100, 200], [0, 100, 200])
    assert P.tile_grid(16, 17, tile=16) == ([0], [0, 1])
    assert P.tile_grid(1024, 2000, tile=1024, stride=1, max_tiles=4096) == ([0], list(range(977)))


def test_tile_grid_properties_over_random_sizes():
    P = _pipeline()
    rng = np.random.default_rng(7)
    for _ in range(300):
        tile = int(rng.integers(16, 300))
        stride = int(rng.integers(1, tile + 1))
        h, w = int(rng.integers(tile, 6 * tile)), int(rng.integers(tile, 6 * tile))
        full = (-(-(h - tile) // stride) + 1) * (-(-(w - tile) // stride) + 1)
        for max_tiles in (4096, int(rng.integers(1, 40))):
            if full > 4096:
                continue
            ys, xs = P.tile_grid(h, w, tile, stride, max_tiles)
            assert 1 <= len(ys) * len(xs) <= max_tiles
            thinned = len(ys) * len(xs) < full
            assert thinned == (full > max_tiles)
            for pos, L in ((ys, h), (xs, w)):
                assert pos[0] == 0 and all(b > a for a, b in zip(pos, pos[1:])), (pos, L, tile, stride)
                assert len(pos) == 1 or pos[-1] == L - tile
                if not thinned:
                    assert pos[-1] == L - tile and all(b - a <= stride for a, b in zip(pos, pos[1:])), (pos, L, tile, stride)


def test_tile_grid_thinning_order():
    P = _pipeline()
    # 3 x 3 with at most 8: a tie, so a row goes -> 2 x 3; at most 5: then the larger count, the columns -> 2 x 2
    assert P.tile_grid(600, 600, max_tiles=8) == ([0, 400], [0, 200, 400])
    assert P.tile_grid(600, 600, max_tiles=5) == ([0, 400], [0, 400])
    assert P.tile_grid(600, 600, max_tiles=1) == ([0], [0])
    assert P.tile_grid(200, 1000, max_tiles=3) == ([0], [0, 400, 800])


@pytest.mark.parametrize("kwargs", [dict(tile=15), dict(tile=1025), dict(tile=200.0), dict(tile="200"), dict(tile=True),
                                    dict(stride=0), dict(stride=201), dict(stride=1.5), dict(tile=64, stride=65),
                                    dict(max_tiles=0), dict(max_tiles=4097), dict(max_tiles=None), dict(max_tiles=2.0)])
def test_tile_arguments_are_checked(kwargs):
    P = _pipeline()
    with pytest.raises(ValueError, match="expected an integer in"):
        P.tile_grid(500, 500, **kwargs)
    with pytest.raises(ValueError, match="expected an integer in"):
        P.tile_plan([(500, 500)], **{"tile": 200, "stride": None, "max_tiles": 256, **kwargs})


def test_tile_plan_tab_and_seg_are_consistent():
    P = _pipeline()
    sizes = [(400, 400), (200, 200), (150, 300), (401, 200), (1000, 1300), (200, 201)]
    plan = P.tile_plan(sizes, 200, None, 12)
    tab, seg = plan                                       # unpacks as the pair
    assert tab.dtype == np.int32 and seg.dtype == np.int32 and tab.shape[1] == 4 and seg.shape == (len(sizes) + 1,)
    assert seg[0] == 0 and seg[-1] == tab.shape[0] and (np.diff(seg) >= 0).all() and (tab[:, 3] == 0).all()
    assert plan.grids == [(2, 2), (0, 0), (0, 0), (3, 1), (3, 4), (1, 2)]       # 200 x 200 IS one tile: left out; 5 x 7 thinned to 12
    assert plan.thinned == [False, False, False, False, True, False] and plan.sizes == sizes
    for i, (h, w) in enumerate(sizes):
        rows = tab[seg[i]:seg[i + 1]]
        assert (rows[:, 0] == i).all() and len(rows) == plan.grids[i][0] * plan.grids[i][1] <= 12
        if len(rows):
            ys, xs = P.tile_grid(h, w, 200, None, 12)
            assert rows[:, 1:3].tolist() == [[y, x] for y in ys for x in xs]     # row-major
            assert (rows[:, 1] + 200 <= h).all() and (rows[:, 2] + 200 <= w).all() and (rows[:, 1:3] >= 0).all()
    empty = P.tile_plan([(10, 10)])
    assert empty.tab.shape == (0, 4) and empty.seg.tolist() == [0, 0]


def test_tile_table_on_hand_made_arrays():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    P = _pipeline()
    names = ["b.png", "a.png", "c.png", "a.png", "d.png"]                    # a.png twice
    sizes = [(400, 400), (400, 600), (150, 300), (400, 600), (200, 200)]
    plan = P.tile_plan(sizes)
    plain = np.array([[0.9, 0.2, 0.6, 0.4, 0.1], [0.7, 0.4, 0.6, 0.2, 0.3]], np.float32)
    nan = np.float32("nan")
    agg = np.zeros((3, 3, 5), np.float32)
    agg[0, 2] = [0.30, 0.50, nan, 0.60, nan]                                # ensemble row: tile mean
    agg[1, 2] = [0.95, 0.70, nan, 0.90, nan]                                # tile max
    agg[2, 2] = [0.25, 0.50, nan, 1.00, nan]                                # fraction
    table, summary = ensemble.tile_table(names, plain, agg, plan, 0.487)
    assert table["filename"] == ["a.png", "b.png", "c.png", "d.png"]
    assert table["width"] == [600, 400, 300, 200] and table["height"] == [400, 400, 150, 200]
    assert table["tiles"] == [6, 4, 0, 0] and table["grid"] == ["2x3", "2x2", "0x0", "0x0"]
    np.testing.assert_allclose(table["p"], [0.3, 0.8, 0.6, 0.2], rtol=1e-6)
    assert table["decision"].tolist() == [0.0, 1.0, 1.0, 0.0]
    np.testing.assert_allclose(table["p_tiles_mean"][:2], [0.55, 0.30], rtol=1e-6)
    np.testing.assert_allclose(table["p_tiles_max"][:2], [0.80, 0.95], rtol=1e-6)
    np.testing.assert_allclose(table["frac_tiles"][:2], [0.75, 0.25], rtol=1e-6)
    for key in ("p_tiles_mean", "p_tiles_max", "frac_tiles"):
        assert np.isnan(table[key][2:]).all() and table[key].dtype == np.float32
    assert table["decision_tiles"].tolist() == [1.0, 0.0, 1.0, 0.0]          # untiled files keep the plain decision
    assert table["agrees"].tolist() == [False, False, True, True]
    assert summary["n_files"] == 4 and summary["n_tiled"] == 2 and summary["n_untiled"] == 2 and summary["n_disagree"] == 2
    assert summary["disagreements"] == ["a.png", "b.png"] and summary["thinned"] == [] and summary["tile_agg"] == "mean"
    by_max, s_max = ensemble.tile_table(names, plain, agg, plan, 0.487, tile_agg="max")
    assert by_max["decision_tiles"].tolist() == [1.0, 1.0, 1.0, 0.0] and s_max["disagreements"] == ["a.png"]
    thin, s_thin = ensemble.tile_table(names, plain, agg, P.tile_plan(sizes, max_tiles=4), 0.487)
    assert thin["grid"] == ["2x2", "2x2", "0x0", "0x0"] and s_thin["thinned"] == ["a.png"]
    with pytest.raises(ValueError, match="mean"):
        ensemble.tile_table(names, plain, agg, plan, 0.487, tile_agg="median")


def test_entry_points_check_arguments_without_a_gpu():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    p = C.c_void_p(64)
    for fn in (lib.vip_tile_resize_bicubic_norm_f16, lib.vip_tile_resize_bicubic_norm_s32):
        assert fn(p, None, p, 4, 40, 40, 16, p, 16, 16, 8, None) == -1 and b"null" in lib.vip_last_error()
        assert fn(p, p, p, 0, 40, 40, 16, p, 16, 16, 8, None) == -1 and b"bad size" in lib.vip_last_error()
        assert fn(p, p, p, 65536, 40, 40, 16, p, 16, 16, 8, None) == -1
        assert fn(p, p, p, 4, 40, 40, 16, p, 16, 16, 2, None) == -1
        assert fn(p, p, p, 4, 40, 15, 16, p, 16, 16, 8, None) == -1 and b"does not fit" in lib.vip_last_error()
        assert fn(p, p, p, 4, 40, 40, 16, C.c_void_p(72), 16, 16, 8, None) == -2
    assert lib.vip_tile_aggregate_f32(p, None, 4, 3, 10, 0.5, p, None) == -1 and b"null" in lib.vip_last_error()
    assert lib.vip_tile_aggregate_f32(p, p, 4, 0, 10, 0.5, p, None) == -1 and b"bad dimension" in lib.vip_last_error()
    assert lib.vip_tile_aggregate_f32(p, p, 4, 3, 0, 0.5, p, None) == -1


REFUSALS = [
    (["--tiles-out", "T", "--tta", "2"], "--tiles-out works with --shard images and --tta 1 only"),
    (["--tiles-out", "T", "--shard", "members"], "--tiles-out works with --shard images and --tta 1 only"),
    (["--tiles-out", "T", "--shard", "hybrid"], "--tiles-out works with --shard images and --tta 1 only"),
    (["--tiles-out", "T", "--heatmaps", "H"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--tiles-out", "T", "--stress-jpeg", "70", "--stress-out", "S"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--tiles-out", "T", "--stress-resize", "50", "--stress-out", "S"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--tiles-out", "T", "--stress-out", "S"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--tile-size", "100"], "need --tiles-out"),
    (["--tile-stride", "100"], "need --tiles-out"),
    (["--tile-max", "16"], "need --tiles-out"),
    (["--tile-agg", "max"], "need --tiles-out"),
    (["--tiles-out", "T", "--tile-size", "15"], "--tile-size 15: expected an integer in 16..1024"),
    (["--tiles-out", "T", "--tile-stride", "201"], "--tile-stride 201: expected an integer in 1..200"),
    (["--tiles-out", "T", "--tile-max", "0"], "--tile-max 0: expected an integer in 1..4096"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_touching_the_gpu(tmp_path, monkeypatch, extra, message):
    """every refusal is a SystemExit raised while the arguments are read: no file is opened and torch's GPU state is not asked for"""
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli

    def touched(*a, **k):
        raise AssertionError("the CLI reached the GPU set-up before refusing")
    for name in ("is_available", "set_device", "device_count", "init"):
        monkeypatch.setattr(torch.cuda, name, touched)
    extra = [str(tmp_path / {"T": "tiles.csv", "S": "stress.csv", "H": "hm"}[t]) if t in ("T", "S", "H") else t for t in extra]
    with pytest.raises(SystemExit) as e:                  # the input CSV does not exist: it is never opened
        cli.main([str(tmp_path / "missing.csv"), str(tmp_path / "o.csv"), "--synthetic", *extra])
    assert message in str(e.value), e.value
    assert not os.listdir(tmp_path)
