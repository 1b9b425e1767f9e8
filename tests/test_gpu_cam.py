"""GPU: the evidence-map (Grad-CAM) kernels of csrc/cam.hip against the fp64 definition in tests/_cam_ref.py - the operator in all
three storages, compose and overlay, the map-capable members against autograd through the fp32 oracle graphs, and the CLI."""
import importlib
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
from tests import _cam_ref as CR  # noqa: E402
from tests import _parity as P  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402

# ---- operator -------------------------------------------------------------------------------------------------------------------------
SHAPES = [(5, 7, 7, 2048), (3, 7, 7, 768), (2, 7, 7, 1792), (4, 13, 13, 96), (1, 1, 1, 64)]
# tolerance on the normalised map: 64 * 2^-24 * kappa, kappa = max_hw sum_c |F g| / peak from the fp64 reference: a position's dot
# product is about 38 dependent fp32 additions for C = 2048 over 64 lanes (32 per lane + 6 reduction steps) plus the rounding of g,
# rounded up to 64 half-ulps of the largest partial sum, which kappa relates to the peak the map is divided by
MAP_EPS = 64 * 2.0 ** -24
KAPPA_MAX = 100.0           # asserted on the reference alone: the bound never exceeds 4e-4
SEED = 4                    # the seed for which every case below has kappa <= KAPPA_MAX


def _case(shape, N, ln, seed=SEED):
    """fp32 host tensors: features, head matrix, bias, LayerNorm parameters"""
    B, H, W, C = shape
    g = torch.Generator().manual_seed(seed * 1000 + C + 7 * N + int(ln))
    f = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(N, C, generator=g) / C ** 0.5
    b = torch.randn(N, generator=g) * 0.3
    lnp = (1.0 + 0.2 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 1e-6) if ln else None
    return f, w, b, lnp


def _store(f, kind, pitch_pad=0):
    """(device tensor in the storage `kind`, the STORED values as fp64 on the host); pitch_pad > 0: images at a pitch of their own"""
    from vipcup_amd import ops
    B, H, W, C = f.shape
    if kind == "f16":
        d = f.to(torch.float16).cuda()
        stored = d.cpu().double()
    elif kind == "s32":
        d = f.cuda()
        stored = f.double()
    else:
        d = ops.pack_h2(f.cuda().contiguous())
        stored = ops.unpack_h2(d).cpu().double()
    if pitch_pad:
        big = torch.zeros((B, H * W * C + pitch_pad), dtype=d.dtype, device="cuda")
        big[:, :H * W * C] = d.reshape(B, -1)
        d = big[:, :H * W * C].view(B, H, W, C)
        assert not d.is_contiguous() or B == 1
    return d, stored


def _check_op(report, tag, d, stored, w, b, lnp, act, target, z_head=None):
    from vipcup_amd import ops
    wd, bd = w.cuda().contiguous(), b.cuda()
    lnd = None if lnp is None else (lnp[0].cuda(), lnp[1].cuda(), lnp[2])
    cam, peak, z = ops.cam(d, wd, bd, ln=lnd, act=act, target=target)
    cam2, peak2, z2 = ops.cam(d, wd, bd, ln=lnd, act=act, target=target)
    torch.cuda.synchronize()
    assert torch.equal(cam, cam2) and torch.equal(peak, peak2) and torch.equal(z, z2), f"{tag}: not bit-repeatable"
    rc, rp, rz, kappa = CR.cam_closed_form(stored, w, b, lnp, act, target)
    ops.cam_check(peak, tag)
    if lnp is not None and stored.shape[1] * stored.shape[2] == 1:
        # One position and a LayerNorm head: F = v, and the gradient that comes back through the LayerNorm is orthogonal to both 1 and
        # (v - mean v), so sum_c F g vanishes but for the LayerNorm's eps (O(eps / var) of sum_c |F g|): the true map is empty to 1e-6
        # of its terms and kappa, a ratio to that peak, is in the millions for any seed.  The same bound is applied to the
        # un-normalised value instead: |cam - reference| <= MAP_EPS * sum_c |F g|  (what MAP_EPS * kappa is, times the peak).
        absum = CR.abs_sum(stored, w, b, lnp, act, target)
        assert float(rp.max()) <= 1e-5 * float(absum.max()), (tag, rp.tolist(), absum.tolist())
        err = (cam.cpu().double() - rc).abs().flatten(1).max(1).values
        report(f"[cam op] {tag}: map empty but for eps; max|d cam| {float(err.max()):.2e} bound {float((MAP_EPS * absum).max()):.2e}")
        assert bool((err <= MAP_EPS * absum).all()), (tag, err.tolist(), absum.tolist())
    else:
        assert float(kappa.max()) <= KAPPA_MAX, (tag, kappa.tolist())                   # a property of the reference alone
        got = CR.normalise(cam.cpu().double(), peak.cpu().double())
        want = CR.normalise(rc, rp)
        err = (got - want).abs().flatten(1).max(1).values
        bound = MAP_EPS * kappa
        report(f"[cam op] {tag}: max|d map| {float(err.max()):.2e} bound {float(bound.max()):.2e} kappa {float(kappa.max()):.1f}")
        assert bool((err <= bound).all()), (tag, err.tolist(), bound.tolist())
        assert bool(((rp > 0) == (peak.cpu() > 0)).all()), (tag, rp.tolist(), peak.tolist())
    assert float((z.cpu().double() - rz).abs().max()) <= 1e-4 * max(1.0, float(rz.abs().max())), tag
    if z_head is not None:
        dz = (z - z_head).abs()
        assert bool((dz <= 1e-6 * z_head.abs()).all()), (tag, z.tolist(), z_head.tolist())


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
@pytest.mark.parametrize("ln", [False, True], ids=["plain", "layernorm"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_cam_operator(shape, ln, kind, report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    for N, targets in ((1, ("score",)), (3, ("score", 0, 2))):
        f, w, b, lnp = _case(shape, N, ln)
        d, stored = _store(f, kind)
        wd, bd = w.cuda().contiguous(), b.cuda()
        z_head = (ops.gap_ln_dense_f32(d, lnp[0].cuda(), lnp[1].cuda(), lnp[2], wd, bd) if ln else ops.gap_dense_f32(d, wd, bd))
        for t in targets:
            _check_op(report, f"{kind} {shape} N={N} ln={ln} target={t}", d, stored, w, b, lnp, "default", t, z_head)


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
def test_cam_operator_other_activations_and_pitch(kind, report):
    """element-wise sigmoid and linear heads on three classes; images at a pitch of their own"""
    import vipcup_amd  # noqa: F401
    f, w, b, lnp = _case((3, 7, 7, 768), 3, True)
    d, stored = _store(f, kind, pitch_pad=64)
    for act, t in (("sigmoid", 1), ("linear", 2), ("linear", "score"), ("softmax", "score")):
        _check_op(report, f"{kind} pitch act={act} target={t}", d, stored, w, b, lnp, act, t)


@pytest.mark.parametrize("kind", ["f16", "s32", "h2"])
def test_cam_all_negative_image_gives_a_zero_map(kind):
    """positive head weights, one image with negative features everywhere: every position is below zero -> zero map, peak 0, no NaN"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    g = torch.Generator().manual_seed(2)
    f = torch.randn(2, 7, 7, 768, generator=g)
    f[0] = -f[0].abs() - 0.05
    w = torch.rand(1, 768, generator=g) + 0.1
    d, stored = _store(f, kind)
    cam, peak, z = ops.cam(d, w.cuda(), None, target="score")
    assert float(peak[0]) == 0.0 and float(cam[0].abs().max()) == 0.0 and float(peak[1]) > 0
    assert torch.isfinite(cam).all() and torch.isfinite(peak).all() and torch.isfinite(z).all()
    sizes = torch.tensor([[7, 7], [7, 7]], dtype=torch.int32, device="cuda")       # the grid's own size: the resampling is the identity
    full = ops.cam_compose([cam], [peak], sizes, (7, 7))
    assert torch.isfinite(full).all() and float(full[0].abs().max()) == 0.0 and abs(float(full[1].max()) - 1.0) <= 1e-6


def test_cam_rejects_bad_arguments():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, ops
    f = torch.zeros(1, 2, 2, 64, dtype=torch.float16, device="cuda")
    w = torch.zeros(3, 64, device="cuda")
    with pytest.raises(ValueError):
        ops.cam(f, w, None, target=3)
    with pytest.raises(ValueError):
        ops.cam(f, w, None, act="tanh")
    with pytest.raises(_abi.VipError):
        ops.cam(f.permute(0, 2, 1, 3), w, None)
    nan = torch.full((1, 2, 2, 64), float("nan"), dtype=torch.float32, device="cuda")
    _, peak, _ = ops.cam(nan, w, None)
    with pytest.raises(_abi.VipError, match="not finite"):
        ops.cam_check(peak)


# ---- compose and overlay --------------------------------------------------------------------------------------------------------------
def _u8_close(got, want, valid):
    """uint8 tensors: at most one level apart, and that on at most 0.1 % of the pixels (rounding ties)"""
    d = (got.int() - want.int()).abs()[valid]
    assert int(d.max()) <= 1, int(d.max())
    assert float((d > 0).float().mean()) <= 1e-3, float((d > 0).float().mean())


def test_compose_and_overlay(report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import cam as camlib, ops
    sizes_host = [(200, 200), (31, 57), (1, 1), (64, 200), (200, 3)]
    n, maxH, maxW = len(sizes_host), 200, 200
    g = torch.Generator().manual_seed(9)
    maps = [torch.rand(n, 7, 7, generator=g) * 3.0, torch.rand(n, 13, 9, generator=g) * 0.02, torch.rand(n, 1, 1, generator=g)]
    peaks = [m.flatten(1).max(1).values.clone() for m in maps]
    maps[1][3] = 0.0
    peaks[1][3] = 0.0                                                     # a member with an empty map for image 3
    weights = [0.5, 0.25, 0.25]
    sizes = torch.tensor(sizes_host, dtype=torch.int32, device="cuda")
    md, pd_ = [m.cuda() for m in maps], [p.cuda() for p in peaks]
    want = CR.compose_ref(maps, peaks, sizes_host, (maxH, maxW), weights)
    got = ops.cam_compose(md, pd_, sizes, (maxH, maxW), weights, out="f32").cpu()
    err = float((got.double() - want).abs().max())
    report(f"[cam compose] fp32 max|d| {err:.2e}")
    assert err <= 1e-6
    valid = torch.zeros((n, maxH, maxW), dtype=torch.bool)
    for i, (h, w) in enumerate(sizes_host):
        valid[i, :h, :w] = True
    assert float(got[~valid].abs().max()) == 0.0
    got8 = ops.cam_compose(md, pd_, sizes, (maxH, maxW), weights, out="u8")
    _u8_close(got8.cpu(), CR.to_u8(want), valid)
    # default weights: the plain mean
    got_m = ops.cam_compose(md, pd_, sizes, (maxH, maxW)).cpu()
    assert float((got_m.double() - CR.compose_ref(maps, peaks, sizes_host, (maxH, maxW))).abs().max()) <= 1e-6
    # overlay on the uint8 map the op produced
    rgb = torch.randint(0, 256, (n, maxH, maxW, 3), generator=g, dtype=torch.uint8)
    table = torch.from_numpy(camlib.jet_table())
    for alpha in (0.4, 1.0):
        ov = ops.cam_overlay(rgb.cuda(), got8, table.cuda(), alpha).cpu()
        _u8_close(ov, CR.overlay_ref(rgb, got8.cpu(), table, alpha), valid[..., None].expand(-1, -1, -1, 3))


# ---- members --------------------------------------------------------------------------------------------------------------------------
N_MEMBER_IMAGES = 16


def _oracle_features(key, params, x):
    from vipcup_amd import zoo
    spec = zoo.MEMBERS[key]
    ref = importlib.import_module(f"oracle.{spec.oracle}")
    if spec.oracle == "resnet_rs_ref":
        return ref.forward_features(params, x, depth=int(key[9:]))
    if spec.oracle == "tfimm_ref":
        return ref.convnext_features(params, x, key)
    if spec.oracle == "kecam_ref":
        return ref.features(key, params, x)
    if spec.oracle == "gcvit_ref":
        return ref.forward_features(params, x, ref.NAME2CONFIG[key])
    return ref.forward_features(params, x, ref.CONFIGS[key])


_ORACLE_MAPS = {}


def oracle_member_map(key, raws):
    """(normalised map, peak, kappa) in fp64: autograd through the head on the fp32 oracle graph's features"""
    from vipcup_amd import zoo
    if key not in _ORACLE_MAPS:
        spec = zoo.MEMBERS[key]
        params = zoo.build_params(key)
        x = torch.stack([R.decode_resize_normalize(p, spec.input_hw, spec.input_hw) for p in P.decode_pixels(raws)])
        with torch.no_grad():
            f = torch.cat([_oracle_features(key, params, x[i:i + 8]) for i in range(0, len(raws), 8)])
        ln = None
        if spec.oracle == "tfimm_ref":
            ln = (params["head/norm/gamma"], params["head/norm/beta"], 1e-6)
        cam, peak, _, kappa = CR.cam_autograd(f, params[f"{spec.head}/kernel"].t().contiguous(), params[f"{spec.head}/bias"], ln, "default", "score")
        _ORACLE_MAPS[key] = (CR.normalise(cam, peak), peak, kappa)
    return _ORACLE_MAPS[key]


def measure_member(key, precision):
    """worst |normalised map - oracle map| over the 16 images, plus what predict_with_cam must keep: bit-equal probabilities"""
    from vipcup_amd import ops, pipeline
    raws = [synth_jpeg(i) for i in P.e2e_image_ids(N_MEMBER_IMAGES)]
    want, wpeak, kappa = oracle_member_map(key, raws)
    spec, model = P.gpu_member(key, precision)
    x = pipeline.decode_images(raws).resized(spec.input_hw, spec.input_hw, dtype=ops.act_dtype(precision))
    p, cam, peak = model.predict_with_cam(x)
    p0 = model.predict(x)
    torch.cuda.synchronize()
    if precision == "strict":
        ops.h2_check(f"{key} strict")
    assert torch.equal(p, p0), f"{key} {precision}: predict_with_cam probabilities differ from predict"
    ops.cam_check(peak, key)
    got = CR.normalise(cam.cpu().double(), peak.cpu().double())
    assert got.shape == want.shape, (got.shape, want.shape)
    err = (got - want).abs().flatten(1).max(1).values
    return float(err.max()), float(err.mean()), int((wpeak > 0).sum()), float(kappa.max())


# Measured on an MI355X (profiles/cam_parity.log: worst |d map| over the 16 images, one weight seed); asserted: four times that
# (16 images under-sample the tail), strict never above 1e-2.
MEASURED = {
    ("convnext_tiny_in22k", "fast"): 1.070e-03,
    ("resnest50", "fast"): 2.001e-04,
    ("gcvit_tiny", "fast"): 1.387e-02,
    ("efficientnet_v2t", "fast"): 9.041e-04,
    ("efficientnet_v1b4", "fast"): 7.719e-04,
    ("eca_nfnet_l0", "fast"): 4.421e-04,
    ("resnet_rs50", "fast"): 0.000e+00,
    ("convnext_tiny_in22k", "strict"): 1.062e-06,
    ("resnest50", "strict"): 2.689e-07,
    ("gcvit_tiny", "strict"): 1.068e-05,
    ("efficientnet_v2t", "strict"): 1.061e-06,
    ("efficientnet_v1b4", "strict"): 7.769e-07,
    ("eca_nfnet_l0", "strict"): 5.369e-07,
    ("resnet_rs50", "strict"): 0.000e+00,
}
# resnet_rs50: with the shipped synthetic head every one of the 16 images has an EMPTY score map, in the oracle and here (its features are
# post-ReLU and the pooled gradient of the score is negative), so that row only says "empty on both sides"; its head_spec() is pinned by
# tests/test_cam_cpu.py and its arithmetic by the operator test above.  gcvit_tiny's fast-mode figure is the fp16 feature map seen
# through maps whose peak is small against their terms (kappa up to 530 on these images).


@pytest.mark.parametrize("precision", ["fast", "strict"])
@pytest.mark.parametrize("key", ["convnext_tiny_in22k", "resnest50", "gcvit_tiny", "efficientnet_v2t", "efficientnet_v1b4", "eca_nfnet_l0",
                                 "resnet_rs50"])
def test_member_maps_match_the_oracle(key, precision, report):
    import vipcup_amd  # noqa: F401
    worst, mean, n_pos, kappa = measure_member(key, precision)
    bound = 4.0 * MEASURED[(key, precision)]
    if precision == "strict":
        bound = min(bound, 1e-2)
    report(f"[cam member] {key:22s} {precision:6s} max|d map| {worst:.3e} mean {mean:.3e} bound {bound:.3e} "
           f"(non-empty oracle maps {n_pos}/{N_MEMBER_IMAGES}, kappa {kappa:.1f})")
    assert worst <= bound, (key, precision, worst, bound)


# ---- CLI ------------------------------------------------------------------------------------------------------------------------------
def _write_set(tmp_path, n):
    idx = P.e2e_image_ids(n)
    names = []
    for i in idx:
        name = f"img_{i:05d}.jpg"
        (tmp_path / name).write_bytes(synth_jpeg(i))
        names.append(name)
    (tmp_path / "test.csv").write_text("filename\n" + "\n".join(names) + "\n")
    return names


def test_cli_heatmaps(tmp_path, report):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import main as cli
    names = _write_set(tmp_path, 16)
    csv = str(tmp_path / "test.csv")
    cli.main([csv, str(tmp_path / "o0.csv"), "--synthetic", "--scores-out", str(tmp_path / "s0.csv"), "--batch-size", "8"])
    hm = tmp_path / "hm"
    cli.main([csv, str(tmp_path / "o1.csv"), "--synthetic", "--scores-out", str(tmp_path / "s1.csv"), "--batch-size", "8",
              "--heatmaps", str(hm), "--heatmap-members"])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    assert (tmp_path / "s0.csv").read_bytes() == (tmp_path / "s1.csv").read_bytes()
    info = json.loads((hm / "heatmaps.json").read_text())
    assert len(info["members"]) == 7 and all(m["cam_supported"] and m["reason"] is None for m in info["members"])
    nonzero = 0
    for name in names:
        w, h = Image.open(io.BytesIO((tmp_path / name).read_bytes())).size
        m = np.load(hm / (os.path.splitext(name)[0] + ".npy"))
        assert m.shape == (h, w) and m.dtype == np.float32, (name, m.shape, (h, w))
        assert np.isfinite(m).all() and m.min() >= 0.0 and m.max() <= 1.0 + 1e-6
        nonzero += int(m.max() > 0)
        low = np.load(hm / (os.path.splitext(name)[0] + ".members.npz"))
        assert len(low.files) == 14 and low["resnet_rs50/cam"].shape == (7, 7) and low["gcvit_tiny/peak"].shape == ()
    report(f"[cam cli] {nonzero} of {len(names)} ensemble maps are not empty")
    assert nonzero > 0


def test_cli_heatmap_png_and_vit(tmp_path, report):
    """an ensemble with a ViT member: it is named as unsupported and left out of the mean; the PNG files hold the overlay the op makes"""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import cam as camlib, ensemble, main as cli, ops, pipeline, zoo
    names = _write_set(tmp_path, 8)
    keys = ["resnet_rs50", "vit_tiny_patch16_224", "convnext_tiny_in22k"]
    cfg = tmp_path / "ckpts.json"
    cfg.write_text(json.dumps([[zoo.MEMBERS[k].ckpt_name, [zoo.MEMBERS[k].input_hw] * 2, 0] for k in keys]))
    hm = tmp_path / "hm"
    common = [str(tmp_path / "test.csv"), "--synthetic", "--ckpt-cfg", str(cfg), "--batch-size", "8"]
    cli.main([common[0], str(tmp_path / "o0.csv"), *common[1:]])
    cli.main([common[0], str(tmp_path / "o1.csv"), *common[1:], "--heatmaps", str(hm), "--heatmap-format", "png"])
    assert (tmp_path / "o0.csv").read_bytes() == (tmp_path / "o1.csv").read_bytes()
    info = {m["name"]: m for m in json.loads((hm / "heatmaps.json").read_text())["members"]}
    assert info["vit_tiny_patch16_224"]["cam_supported"] is False and "class token" in info["vit_tiny_patch16_224"]["reason"]
    assert info["resnet_rs50"]["cam_supported"] and info["convnext_tiny_in22k"]["cam_supported"]
    # the same members, the same batch, through the library
    members = [(zoo.MEMBERS[k], zoo.FoldMean([zoo.build_member(k)[1]])) for k in keys]
    raws = [(tmp_path / n).read_bytes() for n in names]
    ex = ensemble.explain_batch(raws, members, out="u8")
    assert ex.maps[1] is None and list(ex.unsupported) == ["vit_tiny_patch16_224"]
    with pytest.raises(Exception, match="class token"):
        members[1][1].folds[0].cam(ex.batch.resized(224, 224))
    rows = ensemble._score_batch(raws, members)
    assert torch.equal(rows, ex.scores)
    # the map is the mean over the two members that have one
    want = ops.cam_compose([ex.maps[0], ex.maps[2]], [ex.peaks[0], ex.peaks[2]], ex.batch.sizes, ex.batch.rgb.shape[1:3], out="u8")
    assert torch.equal(want, ex.map)
    ov = ops.cam_overlay(ex.batch.rgb, ex.map, camlib.jet_table_device("cuda"), 0.4).cpu().numpy()
    dec = pipeline.decode_images([(hm / (os.path.splitext(n)[0] + ".png")).read_bytes() for n in names])
    got = dec.rgb.cpu().numpy()
    for i, (h, w) in enumerate(ex.batch.sizes_host):
        assert dec.sizes_host[i] == (h, w)
        assert np.array_equal(got[i, :h, :w], ov[i, :h, :w]), names[i]


@pytest.mark.parametrize("extra", [["--shard", "members"], ["--shard", "hybrid"], ["--tta", "2"]], ids=lambda e: "".join(e))
def test_cli_refuses_heatmaps_under_member_sharding_and_tta(tmp_path, extra):
    import subprocess
    _write_set(tmp_path, 2)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vip-cup-2022_amd", "main.py"), str(tmp_path / "test.csv"), str(tmp_path / "o.csv"),
                        "--synthetic", "--heatmaps", str(tmp_path / "hm"), *extra], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--heatmaps works with --shard images and --tta 1 only" in (r.stderr + r.stdout), r.stderr[-400:]
    assert not (tmp_path / "o.csv").exists()
