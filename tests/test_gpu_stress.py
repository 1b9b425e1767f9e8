"""GPU: the recompression stress test - csrc/jpeg_encode.hip against the files Pillow (libjpeg-turbo) writes and reads, coefficient by
coefficient and pixel by pixel, ``pipeline.recompress``, and ``main.py --stress-jpeg`` against plain runs on Pillow-re-saved files.
Every comparison is exact: all stages are integer arithmetic, and the member passes see the same pixels in the same batch positions."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _parity as P  # noqa: E402
from tests._jpeg_enc_ref import content, pil_jpeg  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

N_IMG = int(os.environ.get("VIP_E2E_N", "16"))   # as tests/test_gpu_e2e.py
QUALITIES = [30, 75, 95, 100]
SAMPLINGS = ["4:2:0", "4:4:4"]
SIZES = [(1, 1), (17, 13), (33, 250), (200, 200), (256, 192), (40, 24), (199, 200)]   # (width, height); image 5 is gray


def _images():
    out = [content(11 + k, w, h) for k, (w, h) in enumerate(SIZES)]
    out[5] = np.ascontiguousarray(out[5][..., :1].repeat(3, axis=2))                   # R = G = B
    return out


def _batch(imgs, pad: int = 0):
    """a DecodedBatch holding ``imgs`` in slots of the largest size (+ pad), the rest of every slot filled with noise"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    sizes = [(im.shape[0], im.shape[1]) for im in imgs]
    maxH, maxW = max(h for h, _ in sizes) + pad, max(w for _, w in sizes) + pad
    rgb = np.random.default_rng(5).integers(0, 256, (len(imgs), maxH, maxW, 3), dtype=np.uint8)
    for i, im in enumerate(imgs):
        rgb[i, :im.shape[0], :im.shape[1]] = im
    return pipeline.DecodedBatch(torch.from_numpy(rgb).cuda(), torch.tensor(sizes, dtype=torch.int32, device="cuda"), sizes)


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("q", QUALITIES)
def test_coefficients_equal_pillows_files(q, sampling):
    """vip_jpeg_fdct_quant_u8 on a mixed-size batch == the host entropy decode of the files Pillow saves from the same pixels"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    from vipcup_amd.ops import _p, _stream
    imgs = _images()
    for pad in (0, 3):                                    # pad 3: slot rows at an odd pitch (the unaligned load path)
        batch = _batch(imgs, pad)
        n, maxH, maxW, _ = batch.rgb.shape
        desc, total, max_blocks = pipeline.encode_layout(batch.sizes_host, q, sampling)
        want_desc, want = pipeline.entropy_decode([pil_jpeg(im, q, sampling) for im in imgs])
        assert want.size == total
        guard = 4096
        coef = torch.full((total + 2 * guard,), -31000, dtype=torch.int16, device="cuda")
        planes = torch.full((total + 2 * guard,), 0xAB, dtype=torch.uint8, device="cuda")
        desc_d = torch.from_numpy(np.frombuffer(bytes(desc), dtype=np.uint8).copy()).cuda()
        st = _abi.lib().vip_jpeg_fdct_quant_u8(_p(batch.rgb), _p(desc_d), n, max_blocks, _p(planes[guard:]), _p(coef[guard:]), maxH, maxW,
                                               _stream())
        _abi.check(st, "vip_jpeg_fdct_quant_u8")
        got = coef.cpu().numpy()
        pl = planes.cpu().numpy()
        assert (got[:guard] == -31000).all() and (got[guard + total:] == -31000).all(), "coefficients written outside the buffer"
        assert (pl[:guard] == 0xAB).all() and (pl[guard + total:] == 0xAB).all(), "planes written outside the workspace"
        got = got[guard:guard + total]
        for i in range(n):
            for c in range(3):
                off, nb = want_desc[i].coef_off[c], want_desc[i].blocks_w[c] * want_desc[i].blocks_h[c] * 64
                assert desc[i].coef_off[c] == off
                bad = int((got[off:off + nb] != want[off:off + nb]).sum())
                assert bad == 0, f"image {i} {SIZES[i]} component {c} q{q} {sampling} pad {pad}: {bad} coefficients differ"


def _pil_round_trip(px, q, sampling):
    return np.asarray(Image.open(io.BytesIO(pil_jpeg(px, q, sampling))).convert("RGB"))


@pytest.mark.parametrize("sampling", SAMPLINGS)
@pytest.mark.parametrize("q", QUALITIES)
def test_recompress_pixels_equal_pillows_round_trip(q, sampling):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    imgs = _images()
    batch = _batch(imgs)
    before = batch.rgb.clone()
    out = pipeline.recompress(batch, q, sampling)
    again = pipeline.recompress(batch, q, sampling)
    torch.cuda.synchronize()
    assert torch.equal(batch.rgb, before), "recompress changed its input"
    assert out.rgb.data_ptr() != batch.rgb.data_ptr() and torch.equal(out.rgb, again.rgb), "recompress is not bit-repeatable"
    assert out.sizes_host == batch.sizes_host and torch.equal(out.sizes, batch.sizes)
    got = out.rgb.cpu().numpy()
    for i, im in enumerate(imgs):
        h, w = im.shape[:2]
        want = _pil_round_trip(im, q, sampling)
        bad = int((got[i, :h, :w] != want).any(axis=2).sum())
        assert bad == 0, f"image {i} {SIZES[i]} q{q} {sampling}: {bad} pixels differ from Pillow's save + load"


def _png(px) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, format="PNG")
    return buf.getvalue()


@pytest.mark.parametrize("mixed", [False, True], ids=["png", "png+jpeg"])
def test_recompress_png_and_mixed_sources(mixed):
    """any DecodedBatch goes through: decoded PNGs, and a batch of PNGs and JPEGs of different sizes"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    raws = [_png(content(21, 200, 200)), _png(content(22, 57, 31)), _png(content(23, 16, 16)[..., 0])]       # the last one gray
    if mixed:
        raws = [raws[0], synth_jpeg(149), raws[1], synth_jpeg(101), raws[2]]                                 # 149: 256 x 192
    batch = pipeline.decode_images(raws)
    src = batch.rgb.cpu().numpy()
    for q, sampling in ((75, "4:2:0"), (90, "4:4:4")):
        got = pipeline.recompress(batch, q, sampling).rgb.cpu().numpy()
        for i, (h, w) in enumerate(batch.sizes_host):
            want = _pil_round_trip(np.ascontiguousarray(src[i, :h, :w]), q, sampling)
            assert np.array_equal(got[i, :h, :w], want), (i, (h, w), q, sampling)
    assert np.array_equal(batch.rgb.cpu().numpy(), src)


def test_recompress_rejects_bad_arguments():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, pipeline
    batch = _batch(_images()[:2])
    with pytest.raises(_abi.VipError, match="1..100"):
        pipeline.recompress(batch, 0)
    with pytest.raises(_abi.VipError, match="1..100"):
        pipeline.recompress(batch, 101)
    with pytest.raises(ValueError, match="4:2:0"):
        pipeline.recompress(batch, 75, "4:2:2")


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def _write_set(d, n):
    names = []
    for i in P.e2e_image_ids(n):
        name = f"img_{i:05d}.jpg"
        (d / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (d / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def _resave_set(src, dst, names, q, sampling="4:2:0"):
    """the files a user would get by opening every image and saving it as JPEG at quality q (Pillow = libjpeg-turbo both ways)"""
    dst.mkdir()
    for name in names:
        px = np.asarray(Image.open(io.BytesIO((src / name).read_bytes())).convert("RGB"))
        (dst / name).write_bytes(pil_jpeg(px, q, sampling))
    (dst / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")


def _check_stress_run(tmp_path, names, qs, extra, sampling="4:2:0", report=None):
    """plain run vs stress run (byte-identical CSVs), then one plain run per quality on Pillow-re-saved files against the columns"""
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, main as cli
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--scores-out", str(tmp_path / "s0.csv"), *extra])
    stress_args = ["--stress-jpeg", ",".join(str(q) for q in qs), "--stress-out", str(tmp_path / "stress.csv")]
    if sampling != "4:2:0":
        stress_args += ["--stress-subsampling", "444"]
    cli.main([csv, str(tmp_path / "o1.csv"), "--scores-out", str(tmp_path / "s1.csv"), *extra, *stress_args])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    table = pd.read_csv(tmp_path / "stress.csv", dtype={"flips_at": str}, keep_default_na=False)
    order = sorted(qs, reverse=True)
    assert list(table.columns) == ["filename", "p", "decision"] + [f"p_q{q}" for q in order] + [f"decision_q{q}" for q in order] + \
        ["stable", "flips_at"]
    assert table.filename.tolist() == sorted(names)

    def plain(scores_csv, out_csv):
        s = pd.read_csv(scores_csv)
        members = [c for c in s.columns if c not in ("filename", "ensemble_mean")]
        uniq, p, dec = ensemble.aggregate(s.filename.tolist(), np.stack([s[m].to_numpy(np.float32) for m in members]))
        o = pd.read_csv(out_csv)
        assert o.filename.tolist() == uniq and np.array_equal(o.logit.to_numpy(np.float32), dec)
        return uniq, p, dec

    uniq, p, dec = plain(tmp_path / "s0.csv", tmp_path / "o0.csv")
    assert np.array_equal(table.p.to_numpy(np.float32), p) and np.array_equal(table.decision.to_numpy(np.float32), dec)
    for q in order:
        d = tmp_path / f"q{q}"
        _resave_set(tmp_path, d, names, q, sampling)
        cli.main([str(d / "test.csv"), str(d / "o.csv"), "--scores-out", str(d / "s.csv"), *extra])
        uq, pq, dq = plain(d / "s.csv", d / "o.csv")
        got_p, got_d = table[f"p_q{q}"].to_numpy(np.float32), table[f"decision_q{q}"].to_numpy(np.float32)
        if report is not None:
            report(f"[stress cli] q{q} {sampling}: max|p_q - p(resaved files)| {float(np.abs(got_p - pq).max()):.3e}, "
                   f"mean|p_q - p| {float(np.abs(got_p - p).mean()):.3e}, flips {int((got_d != dec).sum())}/{len(uniq)}")
        assert uq == uniq and np.array_equal(got_p, pq), (q, np.abs(got_p - pq).max())
        assert np.array_equal(got_d, dq), q
    # the table's own columns and the JSON next to it
    dq = np.stack([table[f"decision_q{q}"].to_numpy(np.float32) for q in order], axis=1)
    differs = dq != dec[:, None]
    assert table.stable.tolist() == [int(not r.any()) for r in differs]
    assert table.flips_at.tolist() == ["" if not r.any() else str(max(q for q, f in zip(order, r) if f)) for r in differs]
    info = json.loads((tmp_path / "stress.json").read_text())
    assert info["qualities"] == order and info["n_files"] == len(uniq) and info["n_stable"] == int(table.stable.sum())
    for k, q in enumerate(order):
        assert info["flips"][str(q)] == int(differs[:, k].sum())
        assert info["flip_rate"][str(q)] == pytest.approx(differs[:, k].mean(), abs=1e-12)
        want = np.abs(table[f"p_q{q}"].to_numpy(np.float32).astype(np.float64) - p.astype(np.float64)).mean()
        assert info["mean_abs_dp"][str(q)] == pytest.approx(want, rel=1e-9, abs=1e-12)
    assert info["settings"]["subsampling"] == sampling and info["settings"]["qualities"] == order
    return info


def test_cli_stress_end_to_end(tmp_path, report):
    """--stress-jpeg 90,70,50 on the synthetic set: the CSVs of a plain run unchanged, every column == a plain run on Pillow-re-saved files"""
    names = _write_set(tmp_path, N_IMG)
    info = _check_stress_run(tmp_path, names, [90, 70, 50], ["--synthetic", "--batch-size", "8"], report=report)
    assert info["settings"]["batch_size"] == 8 and len(info["settings"]["members"]) == 7 and info["settings"]["precision"] == "fast"


def test_cli_stress_quality_list_is_deduplicated_and_sorted(tmp_path):
    import pandas as pd
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli, zoo
    _write_set(tmp_path, 3)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in ["resnet_rs50"]]))
    cli.main([str(tmp_path / "test.csv"), str(tmp_path / "o.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--stress-jpeg", "70,90,50,90",
              "--stress-out", str(tmp_path / "st.csv")])
    cols = list(pd.read_csv(tmp_path / "st.csv").columns)
    assert cols[3:6] == ["p_q90", "p_q70", "p_q50"] and len(cols) == 3 + 3 + 3 + 2
    assert json.loads((tmp_path / "st.json").read_text())["qualities"] == [90, 70, 50]


def test_cli_stress_strict_precision(tmp_path, report):
    """one small case in the packed strict storage (two members, 4:4:4)"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import zoo
    names = _write_set(tmp_path, 4)
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in ["resnet_rs50", "convnext_tiny_in22k"]]))
    info = _check_stress_run(tmp_path, names, [60], ["--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "4", "--precision", "strict"],
                             sampling="4:4:4", report=report)
    assert info["settings"]["precision"] == "strict"


def test_stress_batch_row0_is_score_batch(report):
    """library level: row 0 bit for bit ``_score_batch``; rows 1.. = ``_score_batch`` of ``recompress``; qualities in the order given"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ensemble, pipeline, zoo
    members = [(zoo.MEMBERS[k], zoo.FoldMean([P.gpu_member(k)[1]])) for k in ["resnet_rs50", "efficientnet_v2t"]]
    raws = [synth_jpeg(i) for i in P.e2e_image_ids(6)]
    rows = ensemble.stress_batch(raws, members, [40, 80], "4:2:0")
    assert rows.shape == (3, 2, 6) and rows.dtype == torch.float32
    batch = pipeline.decode_images(raws)
    assert torch.equal(rows[0], ensemble._score_batch(raws, members))
    assert torch.equal(rows[1], ensemble._score_batch(pipeline.recompress(batch, 40), members))
    assert torch.equal(rows[2], ensemble._score_batch(pipeline.recompress(batch, 80), members))
    report(f"[stress batch] mean |dp| q40 {float((rows[1] - rows[0]).abs().mean()):.3e}, q80 {float((rows[2] - rows[0]).abs().mean()):.3e}")


REFUSALS = [
    (["--stress-jpeg", "90", "--stress-out", "S", "--shard", "members"], "--stress-jpeg works with --shard images and --tta 1 only"),
    (["--stress-jpeg", "90", "--stress-out", "S", "--shard", "hybrid"], "--stress-jpeg works with --shard images and --tta 1 only"),
    (["--stress-jpeg", "90", "--stress-out", "S", "--tta", "2"], "--stress-jpeg works with --shard images and --tta 1 only"),
    (["--stress-jpeg", "90", "--stress-out", "S", "--heatmaps", "H"], "--stress-jpeg and --heatmaps cannot be combined"),
    (["--stress-jpeg", "90"], "--stress-jpeg needs --stress-out"),
    (["--stress-jpeg", "90,0", "--stress-out", "S"], "integer qualities in 1..100"),
    (["--stress-jpeg", "101", "--stress-out", "S"], "integer qualities in 1..100"),
    (["--stress-jpeg", "high", "--stress-out", "S"], "integer qualities in 1..100"),
    (["--stress-out", "S"], "need --stress-jpeg"),
    (["--stress-subsampling", "444"], "need --stress-jpeg"),
]


@pytest.mark.parametrize("extra,message", REFUSALS, ids=lambda v: "".join(v) if isinstance(v, list) else None)
def test_cli_refuses_before_scoring(tmp_path, extra, message):
    _write_set(tmp_path, 2)
    extra = [str(tmp_path / "stress.csv") if t == "S" else str(tmp_path / "hm") if t == "H" else t for t in extra]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                        "--synthetic", *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and message in (r.stderr + r.stdout), r.stderr[-400:]
    assert not (tmp_path / "o.csv").exists() and not (tmp_path / "stress.csv").exists() and "MODEL(" not in r.stdout
