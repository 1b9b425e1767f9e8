"""CPU: the resize stress test's host side - the integer restatement of an antialiased 8-bit resize (tests/_resample_ref.py, the suite's
oracle for csrc/resample.hip) against Pillow's ``Image.resize`` itself, ``vip_resample_coeffs_h`` against the restatement's tables,
argument checks, and ``ensemble.stress_table`` with resize labels.  The arbiter is Pillow (tests/test_oracle_jpeg.py pins the build);
its 8-bit resize is integer arithmetic over tables computed in double precision, so every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _resample_ref as R  # noqa: E402

SIZES = [(1, 1), (2, 3), (7, 5), (17, 31), (64, 48), (33, 200), (97, 131), (200, 200)]        # (height, width)
PERCENTS = [25, 50, 75, 90, 110, 150, 175, 200]
PAIRS = [(1, 1), (1, 4), (3, 1), (200, 50), (200, 400), (200, 200), (7, 7), (200, 100), (200, 180), (131, 33), (17, 26), (256, 64),
         (192, 288), (5, 2), (2, 5), (400, 40), (40, 160)]                                    # (in, out)


@pytest.mark.parametrize("filter", R.FILTERS)
def test_restatement_equals_pillow(filter):
    cases = bad = 0
    for k, (h, w) in enumerate(SIZES):
        for percent in PERCENTS:
            ho, wo = R.scaled_size(h, w, percent)
            for px in (R.noise(100 + k, h, w), R.two_level(200 + k, h, w)):
                got, want = R.resize(px, ho, wo, filter), R.pil_resize(px, ho, wo, filter)
                assert got.shape == want.shape == (ho, wo, 3)
                bad += int((got != want).any(axis=2).sum())
                cases += 1
    assert cases == 128 and bad == 0, f"{filter}: {bad} pixels differ from Pillow over {cases} cases"


def test_restatement_skips_a_pass_whose_size_is_unchanged():
    px = R.noise(7, 40, 30)
    assert np.array_equal(R.resize(px, 40, 30, "lanczos"), px)
    for ho, wo in ((40, 17), (23, 30)):
        assert np.array_equal(R.resize(px, ho, wo, "bicubic"), R.pil_resize(px, ho, wo, "bicubic"))


def _lib_coeffs(lib, n_in, n_out, filter_id):
    ksize = C.c_int(-1)
    assert lib.vip_resample_coeffs_h(n_in, n_out, filter_id, None, 0, None, 0, C.byref(ksize)) == 0          # size query
    bounds = np.full((n_out, 2), -7, np.int32)
    k = np.full((n_out, ksize.value), -7, np.int32)
    st = lib.vip_resample_coeffs_h(n_in, n_out, filter_id, bounds.ctypes.data_as(C.c_void_p), bounds.size, k.ctypes.data_as(C.c_void_p),
                                   k.size, C.byref(ksize))
    assert st == 0, lib.vip_last_error()
    return bounds, k, ksize.value


@pytest.mark.parametrize("filter", R.FILTERS)
def test_library_tables_equal_the_restatement(filter):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    lib = _abi.lib()
    for n_in, n_out in PAIRS:
        bounds, k, ksize = _lib_coeffs(lib, n_in, n_out, R.FILTER_ID[filter])
        want_b, want_k, want_ksize = R.coeffs(n_in, n_out, filter)
        assert ksize == want_ksize == 2 * int(np.ceil(R.SUPPORT[filter] * max(n_in / n_out, 1.0))) + 1, (n_in, n_out)
        assert np.array_equal(bounds, want_b), (n_in, n_out, "bounds")
        assert np.array_equal(k, want_k), (n_in, n_out, int((k != want_k).sum()), "coefficients differ")
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] >= 1).all() and (bounds.sum(axis=1) <= n_in).all() and (bounds[:, 1] <= ksize).all()
        for x in range(n_out):                                      # unused slots are 0, a row sums to 1 within the rounding
            assert not k[x, bounds[x, 1]:].any()
        assert np.abs(k.sum(axis=1) - (1 << R.PRECISION_BITS)).max() <= ksize
        cached = pipeline.resample_coeffs(n_in, n_out, filter)      # the Python layer hands out the same tables, once per key
        assert np.array_equal(cached[0], bounds) and np.array_equal(cached[1], k) and cached[2] == ksize
        assert pipeline.resample_coeffs(n_in, n_out, filter)[1] is cached[1]
    assert R.FILTER_ID == pipeline.RESAMPLE_FILTERS


def test_coefficient_arguments_are_checked_before_any_work():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    ksize = C.c_int(-1)
    bounds = np.full((8, 2), -7, np.int32)
    k = np.full((8, 16), -7, np.int32)
    pb, pk = bounds.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p)

    def untouched():
        return (bounds == -7).all() and (k == -7).all()

    for n_in, n_out in ((0, 4), (4, 0), (-1, 4), (4, (1 << 20) + 1)):
        assert lib.vip_resample_coeffs_h(n_in, n_out, 1, pb, bounds.size, pk, k.size, C.byref(ksize)) == -1
        assert b"outside 1.." in lib.vip_last_error() and untouched()
    for f in (-1, 3, 99):
        assert lib.vip_resample_coeffs_h(16, 8, f, pb, bounds.size, pk, k.size, C.byref(ksize)) == -1
        assert b"unknown filter" in lib.vip_last_error() and untouched()
    # 16 -> 8 bicubic: ksize 9, so 16 bounds and 72 coefficients
    assert lib.vip_resample_coeffs_h(16, 8, 1, pb, 15, pk, k.size, C.byref(ksize)) == -1
    assert b"too short" in lib.vip_last_error() and untouched()
    assert lib.vip_resample_coeffs_h(16, 8, 1, pb, bounds.size, pk, 71, C.byref(ksize)) == -1
    assert b"too short" in lib.vip_last_error() and untouched()
    assert lib.vip_resample_coeffs_h(16, 8, 1, pb, bounds.size, None, 0, C.byref(ksize)) == -1 and untouched()
    assert lib.vip_resample_coeffs_h(16, 8, 1, pb, bounds.size, pk, k.size, None) == -1 and untouched()
    assert lib.vip_resample_coeffs_h(16, 8, 1, pb, bounds.size, pk, 72, C.byref(ksize)) == 0 and ksize.value == 9
    assert np.array_equal(k.reshape(-1)[:72].reshape(8, 9), R.coeffs(16, 8, "bicubic")[1]) and (k.reshape(-1)[72:] == -7).all()
    # the device entry point refuses bad arguments before it launches anything
    p = C.c_void_p(64)
    assert lib.vip_resample_rgb_u8(None, p, 8, 8, p, p, 4, 4, p, p, 1, 1, 9, None) == -1
    assert lib.vip_resample_rgb_u8(p, p, 8, 8, p, p, 4, 0, p, p, 1, 1, 9, None) == -1
    assert lib.vip_resample_rgb_u8(p, p, 8, 8, p, p, 4, 4, C.c_void_p(66), p, 1, 1, 9, None) == -2
    rows, nbytes, window = C.c_int(0), C.c_int(0), C.c_int(0)
    assert lib.vip_resample_tile_shape(C.byref(rows), C.byref(nbytes), C.byref(window)) == 0 and nbytes.value % 4 == 0
    assert window.value >= 2 * 3 * 14 + 1       # 10 % Lanczos of a side that keeps one sample (14 -> 1): the widest row rescale can ask for
    assert lib.vip_resample_rgb_u8(p, p, 8, 8, p, p, 4, 4, p, p, 1, 1, window.value + 1, None) == -3
    assert b"exceeds" in lib.vip_last_error()


def test_rescale_checks_its_arguments_without_a_gpu():
    """percent and filter are validated before the batch is looked at"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    for percent in (9, 401, 0, -50, 50.5, "50", None, True):
        with pytest.raises(ValueError, match="10..400"):
            pipeline.rescale(None, percent)
    for name in ("nearest", "LANCZOS", "", None):
        with pytest.raises(ValueError, match="bilinear, bicubic, lanczos"):
            pipeline.rescale(None, 50, name)
    with pytest.raises(ValueError, match="bilinear, bicubic, lanczos"):
        pipeline.resample_coeffs(8, 4, "box")
    assert pipeline.scaled_size(200, 200, 50) == (100, 100) and pipeline.scaled_size(1, 3, 10) == (1, 1)
    assert pipeline.scaled_size(33, 200, 75) == (25, 150) == R.scaled_size(33, 200, 75) and pipeline.scaled_size(7, 5, 90) == (6, 5)


# ---- stress_table ---------------------------------------------------------------------------------------------------------------------
def test_stress_labels_order():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    assert ensemble.stress_labels([90, 70]) == ["q90", "q70"] and ensemble.stress_labels([], []) == []
    assert ensemble.stress_labels([90, 70], [150, 50]) == ["q90", "q70", "r150", "r150_q90", "r150_q70", "r50", "r50_q90", "r50_q70"]
    assert ensemble.stress_labels([], [50]) == ["r50"]


def test_stress_table_with_resize_labels():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    names = ["b.jpg", "a.jpg", "c.jpg", "a.jpg", "d.jpg"]
    labels = ["q90", "q70", "r50", "r50_q90", "r50_q70"]
    s = np.zeros((6, 2, 5), dtype=np.float32)                 # [1 + V, M = 2, n = 5]; a.jpg is rows 1 and 3
    s[0] = [[0.9, 0.2, 0.3, 0.6, 0.1]] * 2                    # a 0.4 -> 0, b 0.9 -> 1, c 0.3 -> 0, d 0.1 -> 0
    s[1] = [[0.8, 0.2, 0.3, 0.6, 0.1]] * 2                    # q90: nothing flips
    s[2] = [[0.4, 0.2, 0.3, 0.6, 0.1]] * 2                    # q70: b flips
    s[3] = [[0.9, 0.9, 0.3, 0.7, 0.1]] * 2                    # r50: a -> 0.8 flips
    s[4] = [[0.2, 0.2, 0.9, 0.6, 0.1]] * 2                    # r50_q90: b and c flip
    s[5] = [[0.2, 0.9, 0.9, 0.9, 0.1]] * 2                    # r50_q70: a, b and c flip
    table, summary = ensemble.stress_table(names, s, labels)
    assert table["filename"] == ["a.jpg", "b.jpg", "c.jpg", "d.jpg"] and table["labels"] == labels
    for k in range(6):                                        # every row IS aggregate's
        uniq, p, dec = ensemble.aggregate(names, s[k])
        got_p, got_d = (table["p"], table["decision"]) if k == 0 else (table["p_q"][:, k - 1], table["decision_q"][:, k - 1])
        assert uniq == table["filename"] and np.array_equal(p, got_p) and np.array_equal(dec, got_d)
    assert table["stable"].tolist() == [False, False, False, True]                  # over ALL variants
    assert table["flips_at"] == [None, 70, None, None]                              # the 100 % rows only
    assert table["flips"] == ["r50;r50_q70", "q70;r50_q90;r50_q70", "r50_q90;r50_q70", ""]
    assert summary["variants"] == labels and summary["qualities"] == [90, 70] and summary["n_stable"] == 1 and summary["n_files"] == 4
    assert summary["flips"] == {"q90": 0, "q70": 1, "r50": 1, "r50_q90": 2, "r50_q70": 3}
    assert summary["flip_rate"] == {"q90": 0.0, "q70": 0.25, "r50": 0.25, "r50_q90": 0.5, "r50_q70": 0.75}
    want = np.abs(table["p_q"].astype(np.float64) - table["p"].astype(np.float64)[:, None]).mean(axis=0)
    assert list(summary["mean_abs_dp"]) == labels
    assert [summary["mean_abs_dp"][v] for v in labels] == pytest.approx(want.tolist(), rel=1e-12)
    # resize-only: no 100 % rows, so flips_at is empty everywhere
    table, summary = ensemble.stress_table(names, s[[0, 3]], ["r50"])
    assert table["flips_at"] == [None] * 4 and table["flips"] == ["r50", "", "", ""] and table["stable"].tolist() == [False, True, True, True]
    assert summary["qualities"] == [] and summary["variants"] == ["r50"] and summary["flips"] == {"r50": 1}


def test_stress_table_quality_labels_give_the_earlier_result():
    """with ``q`` labels alone - as strings or as the integers callers passed so far - the result is what the function gave before"""
    import json
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble
    rng = np.random.default_rng(3)
    names = [f"f{k % 7}.jpg" for k in range(10)]
    s = rng.random((4, 3, 10)).astype(np.float32)
    qs = [90, 70, 50]
    t_int, s_int = ensemble.stress_table(names, s, qs)
    t_str, s_str = ensemble.stress_table(names, s, [f"q{q}" for q in qs])
    assert list(t_int) == list(t_str) == ["filename", "p", "decision", "p_q", "decision_q", "stable", "flips_at"]
    for key in t_int:
        a, b = t_int[key], t_str[key]
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, key
    assert json.dumps(s_int) == json.dumps(s_str)
    # ... spelled out: the earlier function's rules
    agg = [ensemble.aggregate(names, row) for row in s]
    differs = np.stack([a[2] for a in agg[1:]], axis=1) != agg[0][2][:, None]
    assert list(s_int) == ["n_files", "threshold", "qualities", "n_stable", "flips", "flip_rate", "mean_abs_dp"]
    assert s_int["qualities"] == qs and s_int["flips"] == {str(q): int(differs[:, k].sum()) for k, q in enumerate(qs)}
    assert t_int["flips_at"] == [max((q for q, d in zip(qs, row) if d), default=None) for row in differs]
    assert t_int["stable"].tolist() == (~differs.any(axis=1)).tolist()
