"""CPU: the noise stress tests without a GPU - the restatement of tests/_noise_ref.py against Philox4x32-10's published known answers, the
inverse-normal table (``pipeline.noise_table`` against the restatement's own bisection), the statistics of the field, its keying by
position, seed and key, the 32-bit headroom of every mode, labels and table, ``pipeline.noise``'s and the entry point's argument checks,
and ``main.py``'s refusals.  The statistical bounds are five standard errors of the sample sizes used and follow from those alone."""
import ctypes as C
import math
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _noise_ref as R  # noqa: E402


# ---- the generator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, want):
    assert " ".join(f"{int(v):08x}" for v in R.philox(*counter, *key)) == want
    got = R.philox(*[np.full((2, 3), c, np.uint64) for c in counter], *key)                       # and element by element on arrays
    assert all(v.shape == (2, 3) and (v == int(w, 16)).all() for v, w in zip(got, want.split()))


def test_table():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    T = R.table()
    got = pipeline.noise_table()
    assert got.dtype == np.int32 and got.shape == (4097,) and np.array_equal(got, T)
    assert pipeline.noise_table() is got and not got.flags.writeable
    assert T[0] == -16384 and T[4096] == 16384 and T[2048] == 0
    assert np.array_equal(T, -T[::-1]), "odd symmetry"
    steps = np.diff(T)
    assert (steps > 0).all() and steps.max() <= 2101
    # against the definition, away from the two cut ends: Phi(T[i] / 4096) is i / 4096 to within half a unit of T
    for i in (1, 2, 100, 1024, 2047, 3000, 4095):
        lo, hi = R._phi((T[i] - 0.5) / 4096), R._phi((T[i] + 0.5) / 4096)
        assert lo <= i / 4096 <= hi, i
    # z at the ends of the word range and inside a bin
    assert R.z(0) == -16384 and R.z(0xFFFFFFFF) == T[4095] + ((T[4096] - T[4095]) * 0x7FFF + 16384 >> 15) and R.z(0x80000000) == 0
    assert R.z((7 << 20) | (0x4000 << 5)) == T[7] + ((T[8] - T[7]) * 0x4000 + 16384 >> 15)
    assert (np.diff(R.z(np.arange(0, 1 << 32, 65521, dtype=np.uint64))) >= 0).all(), "z is non-decreasing in w"


def test_amounts():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for kind, values in (("gaussian", [t / 10 for t in range(5, 501)]), ("mono", [0.5, 3, 50]), ("speckle", list(range(1, 51))),
                         ("impulse", [t / 10 for t in range(1, 501)])):
        for v in values:
            assert pipeline.noise_amount(kind, v) == R.amount(kind, v), (kind, v)
    assert pipeline.noise_amount("gaussian", 0.5) == 128 and pipeline.noise_amount("gaussian", 50) == 12800
    assert pipeline.noise_amount("gaussian", 3) == 768 and pipeline.noise_amount("mono", 1.5) == 384
    assert pipeline.noise_amount("speckle", 1) == 3 and pipeline.noise_amount("speckle", 50) == 128
    assert pipeline.noise_amount("impulse", 0.1) == 4294967 and pipeline.noise_amount("impulse", 50.0) == 1 << 31


def _field(h=200, w=200, seed=0, key=0):
    w0, w1, w2, _ = R.words(h, w, seed, key)
    return np.stack([R.z(w0), R.z(w1), R.z(w2)], axis=2) / 4096.0


def test_normal_statistics_of_one_field():
    z = _field(seed=20221, key=zlib.crc32(b"img_00000.jpg"))
    N = z.size
    assert N == 120000
    assert abs(z.mean()) <= 5 / math.sqrt(N), z.mean()
    assert abs(z.std() - 1) <= 5 / math.sqrt(2 * N) + 1e-4, z.std()
    assert np.abs(z).max() <= 4.0

    def corr(a, b):
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    # between channels: the three pairs pooled, N pairs; between horizontal neighbours: all channels, 119 400 pairs
    r_channels = corr(np.concatenate([z[..., 0], z[..., 1], z[..., 2]]), np.concatenate([z[..., 1], z[..., 2], z[..., 0]]))
    r_neighbours = corr(z[:, :-1], z[:, 1:])
    assert abs(r_channels) <= 5 / math.sqrt(N), r_channels
    assert abs(r_neighbours) <= 5 / math.sqrt(N), r_neighbours
    assert abs(corr(z[:-1], z[1:])) <= 5 / math.sqrt(N)                                          # and vertical ones


def test_impulse_counts():
    px = np.full((200, 200, 3), 128, np.uint8)
    N = 200 * 200
    for percent in (0.1, 5, 50):
        thr = R.amount("impulse", percent)
        p = thr / 2 ** 32
        out = R.apply(px, "impulse", percent, seed=3, key=77)
        hit = (out != 128).any(axis=2)
        assert ((out == 128) | (out == 0) | (out == 255)).all() and (out[..., 0] == out[..., 1]).all() and (out[..., 1] == out[..., 2]).all()
        k = int(hit.sum())
        assert abs(k - N * p) <= 5 * math.sqrt(N * p * (1 - p)), (percent, k)
        white = int((out[..., 0] == 255).sum())
        assert abs(white - k / 2) <= 5 * math.sqrt(k) / 2, (percent, white, k)
    # a smaller percent hits a subset of the pixels of a larger one: the same field under another threshold
    assert not ((R.apply(px, "impulse", 5, 3, 77) != 128) & (R.apply(px, "impulse", 50, 3, 77) == 128)).any()


def test_field_is_keyed_by_seed_key_and_position():
    px = np.random.default_rng(1).integers(0, 256, (40, 56, 3), dtype=np.uint8)
    for kind, value in (("gaussian", 3), ("mono", 3), ("speckle", 20), ("impulse", 10)):
        base = R.apply(px, kind, value, seed=5, key=9)
        assert np.array_equal(base, R.apply(px.copy(), kind, value, seed=5, key=9)), kind
        assert not np.array_equal(base, R.apply(px, kind, value, seed=6, key=9)), kind
        assert not np.array_equal(base, R.apply(px, kind, value, seed=5, key=10)), kind
        assert not np.array_equal(base, R.apply(px, kind, value, seed=9, key=5)), kind                # seed and key are not interchangeable
        assert not np.array_equal(base, px), kind
        # position, not size: the crop of a larger image gets the crop of its noise
        assert np.array_equal(R.apply(px[:17, :23], kind, value, seed=5, key=9), base[:17, :23]), kind
    big, small = R.words(64, 300, 5, 9), R.words(37, 53, 5, 9)
    assert all(np.array_equal(b[:37, :53], s) for b, s in zip(big, small))
    # (x, y) is not (y, x): a transposed image does not get the transposed field
    assert not np.array_equal(R.words(8, 8, 0, 0)[0], R.words(8, 8, 0, 0)[0].T)
    # two sigmas, one field: the noise of a mid-gray image scales with sigma
    gray = np.full((64, 64, 3), 128, np.uint8)
    d3, d6 = R.apply(gray, "gaussian", 3).astype(int) - 128, R.apply(gray, "gaussian", 6).astype(int) - 128
    assert np.abs(d6 - 2 * d3).max() <= 1
    m = R.apply(gray, "mono", 10)
    assert (m[..., 0] == m[..., 1]).all() and (m[..., 1] == m[..., 2]).all() and len(np.unique(m)) > 20


def test_every_sum_stays_inside_32_bits():
    white, black = np.full((64, 64, 3), 255, np.uint8), np.zeros((64, 64, 3), np.uint8)
    assert int(np.abs(R.table()).max()) == 16384
    for kind, a, bound in (("gaussian", 12800, 12800 * 16384 + (1 << 19)), ("mono", 12800, 12800 * 16384 + (1 << 19)),
                           ("speckle", 128, 255 * 128 * 16384 + (1 << 19))):
        assert bound < 2 ** 31
        for px in (white, black):
            assert R.headroom(px, kind, a, seed=1, key=2) <= bound
        up, down = R.apply_int(white, kind, a, seed=1, key=2), R.apply_int(black, kind, a, seed=1, key=2)
        assert up.max() == 255 and up.min() < 255 and down.min() == 0, "the largest amount reaches both clamps"
        assert (down == 0).all() if kind == "speckle" else down.max() > 0                     # speckle leaves black alone
    assert R.apply_int(white, "speckle", 128, 1, 2).min() == 0, "z < -2 at 50 % takes white to the lower clamp"
    # the interpolation product of z: the largest step times the largest fraction
    assert int(np.diff(R.table()).max()) * 0x7FFF + 16384 < 2 ** 27


# ---- pipeline and the entry point: argument checks need no GPU -----------------------------------------------------------------------------
def test_pipeline_noise_checks_its_arguments(monkeypatch):
    import torch
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    monkeypatch.setattr(pipeline, "_launch", lambda *a, **k: pytest.fail("a refused call reached the launch"))
    batch = pipeline.DecodedBatch(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.tensor([[4, 4], [2, 3]], dtype=torch.int32),
                                  [(4, 4), (2, 3)])
    bad = [("gauss", 3, {}), (None, 3, {}), ("gaussian", 0.4, {}), ("gaussian", 50.1, {}), ("gaussian", 0.55, {}), ("gaussian", "3", {}),
           ("gaussian", True, {}), ("gaussian", float("nan"), {}), ("mono", 0, {}), ("mono", 51, {}), ("speckle", 0, {}), ("speckle", 51, {}),
           ("speckle", 2.5, {}), ("speckle", 2.0, {}), ("impulse", 0.05, {}), ("impulse", 50.1, {}), ("impulse", -1, {}),
           ("gaussian", 3, {"seed": -1}), ("gaussian", 3, {"seed": 1 << 32}), ("gaussian", 3, {"seed": 1.0}),
           ("gaussian", 3, {"keys": [1]}), ("gaussian", 3, {"keys": [1, 2, 3]}), ("gaussian", 3, {"keys": [-1, 2]}),
           ("gaussian", 3, {"keys": [1, 1 << 32]}), ("gaussian", 3, {"keys": [0.5, 1]}), ("impulse", 1, {"keys": "ab"})]
    for kind, amount, kw in bad:
        with pytest.raises(ValueError):
            pipeline.noise(batch, kind, amount, **kw)
    for fn, v in ((pipeline.gaussian_noise, 0.4), (pipeline.mono_noise, 60), (pipeline.speckle, 0), (pipeline.impulse, 0)):
        with pytest.raises(ValueError):
            fn(batch, v)
    with pytest.raises(ValueError, match="int32"):                                    # a device tensor of keys of the wrong kind
        pipeline.noise(batch, "gaussian", 3, keys=torch.zeros(2, dtype=torch.int64))
    assert pipeline._noise_keys_arg(None, 3).tolist() == [0, 1, 2]
    assert pipeline._noise_keys_arg([0xFFFFFFFF, 0], 2).dtype == np.uint32


def test_crc32_keys():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    assert pipeline.noise_keys(["123456789"]) == [0xCBF43926]                          # the CRC-32 check value
    names = ["a/b/img_00001.jpg", "img_00001.jpg", "/x/img_00002.jpg", "img_00001.png"]
    keys = pipeline.noise_keys(names)
    assert keys == [zlib.crc32(os.path.basename(n).encode()) for n in names]
    assert keys[0] == keys[1] and len(set(keys)) == 3 and all(0 <= k <= 0xFFFFFFFF for k in keys)
    assert pipeline.noise_keys([]) == []


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    f = lib.vip_noise_rgb_u8
    p, s, q, k, t = (C.c_void_p(v) for v in (1 << 20, 1 << 28, 1 << 24, 1 << 29, 1 << 30))
    good = [p, s, 8, 8, q, 8, 8, 0, 768, 0, k, t, 1, None]
    for i in (0, 1, 4, 10, 11):
        args = list(good)
        args[i] = None
        assert f(*args) == -1 and b"null" in lib.vip_last_error(), i
    for i in (2, 3, 5, 6, 12):
        for v in (0, -1):
            args = list(good)
            args[i] = v
            assert f(*args) == -1 and b"bad size" in lib.vip_last_error(), (i, v)
    args = list(good)
    args[4] = p
    assert f(*args) == -1 and b"overlap" in lib.vip_last_error()
    args[4] = C.c_void_p((1 << 20) + 191)
    assert f(*args) == -1 and b"overlap" in lib.vip_last_error()
    for mode, amount in [(0, 127), (0, 12801), (1, 127), (1, 12801), (2, 2), (2, 129), (3, 4294966), (3, (1 << 31) + 1), (0, -768), (3, -1),
                         (0, 0), (4, 768), (-1, 768), (0, 1 << 40)]:
        args = list(good)
        args[7], args[8] = mode, amount
        assert f(*args) == -1 and b"amount" in lib.vip_last_error(), (mode, amount)
    for i in (1, 10, 11):
        args = list(good)
        args[i] = C.c_void_p(good[i].value + 2)
        assert f(*args) == -2 and b"4-byte" in lib.vip_last_error(), i
    g = lib.vip_noise_rgb_u8_placed
    assert g(*good[:12], 2, 1, None) == -1 and b"placement" in lib.vip_last_error()


# ---- ensemble -----------------------------------------------------------------------------------------------------------------------------
def test_stress_labels_order():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([75], noises=[3], impulses=[1]) == ["q75", "n030", "n030_q75", "imp010", "imp010_q75"]
    got = ensemble.stress_labels([90, 70], [50], [1.0], [3], flips=["h"], gammas=[0.8], gray=True, impulses=[50, 0.1, 2.5], speckles=[20, 5],
                                 mono_noises=[10, 0.5], noises=[50, 3, 1.5], noise_seed=7, noise_keys=[1, 2])
    variants = ["r50", "b10", "m3", "fliph", "gray", "gam080", "n015", "n030", "n500", "nm005", "nm100", "spk05", "spk20", "imp001", "imp025",
                "imp500"]
    assert got == ["q90", "q70"] + [v + s for v in variants for s in ("", "_q90", "_q70")]
    assert ensemble.stress_labels([], speckles=[1, 50]) == ["spk01", "spk50"]
    none = dict(noises=(), mono_noises=(), speckles=(), impulses=(), noise_seed=0, noise_keys=None)
    for args, kw in ((([90, 70],), {}), (([], []), {}), (([80], [50], [1.0], [3]), {}), (([75],), dict(flips=["h"], gray=True, hues=[30]))):
        assert ensemble.stress_labels(*args, **kw, **none) == ensemble.stress_labels(*args, **kw)
    assert ensemble.stress_labels([75], gray=True, hues=[30]) == ["q75", "gray", "gray_q75", "hue030", "hue030_q75"]


def test_stress_table_with_noise_labels():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg"]
    labels = ensemble.stress_labels([75], noises=[3], speckles=[20])
    assert labels == ["q75", "n030", "n030_q75", "spk20", "spk20_q75"]
    s = np.zeros((6, 2, 4), dtype=np.float32)                 # [1 + V, M = 2, n = 4]; a.jpg is rows 1 and 3
    s[0] = [[0.9, 0.2, 0.3, 0.6]] * 2                         # a 0.4 -> 0, b 0.9 -> 1, c 0.3 -> 0
    s[1] = [[0.4, 0.2, 0.3, 0.6]] * 2                         # q75: b flips
    s[2] = [[0.9, 0.2, 0.3, 0.6]] * 2                         # n030: nothing flips
    s[3] = [[0.9, 0.9, 0.3, 0.7]] * 2                         # n030_q75: a -> 0.8 flips
    s[4] = [[0.9, 0.2, 0.9, 0.6]] * 2                         # spk20: c flips
    s[5] = [[0.1, 0.9, 0.9, 0.9]] * 2                         # spk20_q75: everything flips
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg"] and table["labels"] == labels
    for k in range(6):                                        # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert table["flips_at"] == [None, 75, None]              # flips_at: the plain q rows only - n030 is not a quality
    assert table["flips"] == ["n030_q75;spk20_q75", "q75;spk20_q75", "spk20;spk20_q75"]
    assert summary["variants"] == labels and summary["qualities"] == [75] and summary["n_stable"] == 0
    assert summary["flips"] == {"q75": 1, "n030": 0, "n030_q75": 1, "spk20": 1, "spk20_q75": 3}
    table, summary = ensemble.stress_table(names, s[[0, 2, 4]], ["n030", "spk20"])                     # noise only: no q rows
    assert table["flips_at"] == [None] * 3 and table["flips"] == ["", "", "spk20"] and summary["qualities"] == []


# ---- CLI refusals: everything is refused before torch is imported or a model is built --------------------------------------------------------
REFUSALS = [
    (["--stress-noise", "3"], "--stress-noise needs --stress-out"),
    (["--stress-noise-mono", "3"], "--stress-noise-mono needs --stress-out"),
    (["--stress-speckle", "5"], "--stress-speckle needs --stress-out"),
    (["--stress-impulse", "1"], "--stress-impulse needs --stress-out"),
    (["--stress-noise-seed", "5", "--stress-jpeg", "75", "--stress-out", "S"], "--stress-noise-seed needs --stress-noise"),
    (["--stress-noise", "3", "--stress-noise-seed", "4294967296", "--stress-out", "S"], "--stress-noise-seed 4294967296: expected an integer in 0..4294967295"),
    (["--stress-noise", "3", "--stress-noise-seed=-1", "--stress-out", "S"], "expected an integer in 0..4294967295"),
    (["--stress-noise", "0.4", "--stress-out", "S"], "--stress-noise '0.4': expected a comma-separated list of sigmas in 0.5..50.0"),
    (["--stress-noise", "50.1", "--stress-out", "S"], "sigmas in 0.5..50.0"),
    (["--stress-noise", "3.25", "--stress-out", "S"], "sigmas in 0.5..50.0"),
    (["--stress-noise", "3,,5", "--stress-out", "S"], "sigmas in 0.5..50.0"),
    (["--stress-noise=-3", "--stress-out", "S"], "sigmas in 0.5..50.0"),
    (["--stress-noise", "3,5,3", "--stress-out", "S"], "each listed once"),
    (["--stress-noise", "3,3.0", "--stress-out", "S"], "--stress-noise '3,3.0'"),
    (["--stress-noise-mono", "0", "--stress-out", "S"], "--stress-noise-mono '0': expected a comma-separated list of sigmas in 0.5..50.0"),
    (["--stress-noise-mono", "2,2", "--stress-out", "S"], "each listed once"),
    (["--stress-speckle", "0", "--stress-out", "S"], "--stress-speckle '0': expected a comma-separated list of integer percents in 1..50"),
    (["--stress-speckle", "51", "--stress-out", "S"], "integer percents in 1..50"),
    (["--stress-speckle", "2.5", "--stress-out", "S"], "integer percents in 1..50"),
    (["--stress-speckle", "5,05", "--stress-out", "S"], "each listed once"),
    (["--stress-impulse", "0", "--stress-out", "S"], "--stress-impulse '0': expected a comma-separated list of percents in 0.1..50.0"),
    (["--stress-impulse", "50.1", "--stress-out", "S"], "percents in 0.1..50.0"),
    (["--stress-impulse", "0.05", "--stress-out", "S"], "percents in 0.1..50.0"),
    (["--stress-impulse", "1,1.0", "--stress-out", "S"], "each listed once"),
    (["--stress-noise", "3", "--stress-out", "S", "--tta", "2"], "--stress-noise works with --shard images and --tta 1 only"),
    (["--stress-impulse", "1", "--stress-out", "S", "--shard", "members"], "the noise stress tests under member sharding or TTA are not implemented"),
    (["--stress-speckle", "5", "--stress-out", "S", "--shard", "hybrid"], "--stress-speckle works with --shard images and --tta 1 only"),
    (["--stress-noise", "3", "--stress-out", "S", "--heatmaps", "H"], "--stress-noise and --heatmaps cannot be combined"),
    (["--stress-noise-mono", "3", "--stress-out", "S", "--heatmaps", "H"], "--stress-noise-mono and --heatmaps cannot be combined"),
    (["--stress-noise", "3", "--stress-out", "S", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-impulse", "1", "--tiles-out", "T"], "--tiles-out cannot be combined with --heatmaps or --stress-*"),
    (["--stress-noise", "3", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
    (["--stress-speckle", "5", "--stress-out", "S", "--occlusion", "H"], "--occlusion cannot be combined with --heatmaps, --stress-* or --tiles-out"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_scoring(tmp_path, monkeypatch, extra, message):
    """in-process: the refusals come before main.py imports torch or looks at a file, so nothing is built and nothing written"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    from vipcup_amd import zoo
    monkeypatch.setattr(zoo, "build_member", lambda *a, **k: pytest.fail("a member was built"))
    (tmp_path / "test.csv").write_text("filename\nimg_00000.jpg\n")
    paths = {"S": "stress.csv", "H": "maps", "T": "tiles.csv"}
    extra = [str(tmp_path / paths[t]) if t in paths else t for t in extra]
    with pytest.raises(SystemExit) as e:
        cli.main([str(tmp_path / "test.csv"), str(tmp_path / "o.csv"), "--synthetic", *extra])
    assert message in str(e.value), str(e.value)
    assert sorted(os.listdir(tmp_path)) == ["test.csv"]
