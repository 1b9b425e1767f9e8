"""CPU: the evidence-map (Grad-CAM) feature above the kernels - the closed form against autograd, ``head_spec()`` of every member
family through the emulated host graphs, the ViT refusal, the compose / overlay references, the PNG writer."""
import dataclasses
import struct
import zlib

import numpy as np
import pytest
import torch

from oracle import ops_ref as R
from tests import _cam_ref as CR
from tests import emul_ops


def _head(C, N, ln, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, C, generator=g, dtype=torch.float64) / C ** 0.5
    b = torch.randn(N, generator=g, dtype=torch.float64) * 0.3
    lnp = (1.0 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64), 0.1 * torch.randn(C, generator=g, dtype=torch.float64), 1e-6) if ln else None
    return w, b, lnp


@pytest.mark.parametrize("ln", [False, True], ids=["plain", "layernorm"])
@pytest.mark.parametrize("N,act,target", [(1, "sigmoid", "score"), (1, "default", 0), (3, "softmax", "score"), (3, "softmax", 0),
                                          (3, "softmax", 2), (3, "sigmoid", 1), (3, "linear", 1), (3, "linear", "score")])
def test_closed_form_equals_autograd(ln, N, act, target):
    """the closed-form gradient of the head (what csrc/cam.hip computes) against torch.autograd.grad through R.global_avgpool /
    R.layernorm / R.dense, in fp64: 1e-12"""
    g = torch.Generator().manual_seed(11)
    f = torch.randn(4, 5, 6, 40, generator=g, dtype=torch.float64)
    w, b, lnp = _head(40, N, ln, 12)
    cam_a, peak_a, z_a, _ = CR.cam_autograd(f, w, b, lnp, act, target)
    cam_c, peak_c, z_c, _ = CR.cam_closed_form(f, w, b, lnp, act, target)
    scale = max(1.0, float(cam_a.abs().max()))
    assert float((cam_a - cam_c).abs().max()) <= 1e-12 * scale
    assert float((peak_a - peak_c).abs().max()) <= 1e-12 * scale
    assert float((z_a - z_c).abs().max()) <= 1e-12
    assert float(peak_a.max()) > 0                      # the case is not degenerate
    # the head really is what the oracle composes: z through the primitives directly
    u = R.global_avgpool(f)
    if lnp is not None:
        u = R.layernorm(u, lnp[0], lnp[1], lnp[2])
    assert float((R.dense(u, w.t(), b) - z_c).abs().max()) <= 1e-12


def test_all_negative_map_is_zero_not_nan():
    f = -torch.rand(2, 3, 3, 8, dtype=torch.float64) - 0.1
    w = torch.ones(1, 8, dtype=torch.float64)
    cam, peak, _, kappa = CR.cam_closed_form(f, w, None, None, "sigmoid", "score")
    assert float(peak.max()) == 0.0 and float(kappa.max()) == 0.0
    n = CR.normalise(cam, peak)
    assert torch.isfinite(n).all() and float(n.abs().max()) == 0.0


# ---- host graphs: head_spec() of every family ----------------------------------------------------------------------------------------
def _x(n, hw, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, hw, hw, 3, generator=g).to(torch.float16).to(torch.float32)


# fp16-rounded weights against the fp32 oracle, end to end: the bound tests/test_host_graphs_cpu.py holds the logits of the same
# emulated graphs to (2e-2 of the output scale).  The normalised map is the same kind of quantity - a linear functional of the same
# final feature map, scaled to [0, 1] - times its conditioning kappa (cancellation among the C terms of a position).
E2E_TOL = 2e-2
# the same feature tensor on both sides (only the head differs: product's head_spec() vs the checkpoint's raw variables through the
# oracle primitives); the stand-in returns fp32, so the rounding of cam and peak to fp32 (2^-24 relative each) is all that is allowed
HEAD_TOL = 4 * 2.0 ** -24


def _check_family(tag, model_ctor, x, feat_ref, kernel, bias, ln, targets=("score",)):
    """model.cam(x) through the emulation vs (a) autograd through the oracle head on the SAME emulated features - pins head_spec():
    which LayerNorm, which activation, the weight orientation - and (b) the oracle's own features, end to end"""
    with torch.no_grad(), emul_ops.patched(round_act=False), CR.patched():
        model = model_ctor()
        x8 = emul_ops.to_device_nhwc8(x)
        feats = model.features(x8).float()
        got = {t: model.cam(x8, target=t) for t in targets}
    assert model.cam_supported
    w_nc = kernel.t().contiguous()
    for t in targets:
        cam, peak, z = got[t]
        assert cam.shape == feats.shape[:3] and peak.shape == (x.shape[0],) and z.shape == (x.shape[0], kernel.shape[1])
        ca, pa, za, ka = CR.cam_autograd(feats, w_nc, bias, ln, "default", t)
        assert float(pa.min()) > 0, (tag, "degenerate case: pick another seed")
        d = (CR.normalise(cam.double(), peak.double()) - CR.normalise(ca, pa)).abs().flatten(1).max(1).values
        assert bool((d <= HEAD_TOL * torch.clamp(ka, min=1.0)).all()), (tag, t, d.tolist(), ka.tolist())
        assert float((z.double() - za).abs().max()) <= 1e-5 * max(1.0, float(za.abs().max())), tag
        co, po, zo, ko = CR.cam_autograd(feat_ref, w_nc, bias, ln, "default", t)
        d = (CR.normalise(cam.double(), peak.double()) - CR.normalise(co, po)).abs().flatten(1).max(1).values
        print(f"{tag} target={t}: end-to-end |d map| {d.tolist()} kappa {ko.tolist()}")
        assert bool((d <= E2E_TOL * torch.clamp(ko, min=1.0)).all()), (tag, t, d.tolist(), ko.tolist())


def test_resnet_rs_cam():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import resnet_rs
    from oracle import resnet_rs_ref as ref
    ba = [(64, 2), (128, 1), (256, 1), (512, 1)]
    p = resnet_rs.synth_params(50, seed=3, block_args=ba)
    x = _x(2, 64)
    with torch.no_grad():
        f = ref.forward_features(p, x, block_args=ba)
    _check_family("resnet_rs", lambda: resnet_rs.ResNetRS(p, depth=50, block_args=ba, device="cpu"), x, f,
                  p["predictions/kernel"], p["predictions/bias"], None, ("score", 0))


def test_gcvit_cam():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import gcvit
    from oracle import gcvit_ref as ref
    cfg = dict(ref.NAME2CONFIG["gcvit_tiny"], depths=(2, 2, 2, 2))
    p = gcvit.synth_params(cfg, seed=4)
    x = _x(1, 224)
    with torch.no_grad():
        f = ref.forward_features(p, x, cfg)                  # after the final LayerNorm: the tensor gradcam.py:16 takes
    _check_family("gcvit", lambda: gcvit.GCViT(p, **cfg, device="cpu"), x, f, p["head/kernel"], p["head/bias"], None)


def test_convnext_cam_and_vit_refusal():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi, cam as camlib, tfimm_models as tm
    from oracle import tfimm_ref as ref
    name = "convnext_tiny_in22k"
    cfg = dataclasses.replace(tm.CONVNEXT_CONFIGS[name], nb_blocks=(1, 1, 2, 1))
    p = tm.convnext_synth_params(cfg, seed=5)
    x = _x(2, 72)
    with torch.no_grad():
        f = ref.convnext_features(p, x, name, nb_blocks=cfg.nb_blocks)
    _check_family(name, lambda: tm.ConvNeXt(p, cfg, device="cpu"), x, f, p["head/fc/kernel"], p["head/fc/bias"],
                  (p["head/norm/gamma"], p["head/norm/beta"], ref.LN_EPS))
    # a three-class ConvNeXt: softmax head, "score" = 1 - p0 and a class index
    cfg3 = dataclasses.replace(cfg, nb_classes=3)
    p3 = tm.convnext_synth_params(cfg3, seed=15)
    with torch.no_grad():
        f3 = ref.convnext_features(p3, x, name, nb_blocks=cfg3.nb_blocks)
    _check_family(name + "/3", lambda: tm.ConvNeXt(p3, cfg3, device="cpu"), x, f3, p3["head/fc/kernel"], p3["head/fc/bias"],
                  (p3["head/norm/gamma"], p3["head/norm/beta"], ref.LN_EPS), ("score", 1))
    # ViT: the head reads the class token only - no spatial map
    vcfg = dataclasses.replace(tm.VIT_CONFIGS["vit_tiny_patch16_224"], nb_blocks=1)
    with emul_ops.patched(round_act=False), CR.patched():
        vit = tm.ViT(tm.vit_synth_params(vcfg, seed=6), vcfg, device="cpu")
        assert vit.cam_supported is False and "class token" in camlib.unsupported_reason(vit)
        with pytest.raises(_abi.VipError, match="class token"):
            vit.cam(emul_ops.to_device_nhwc8(_x(1, 224)))
        with pytest.raises(_abi.VipError, match="class token"):
            vit.predict_with_cam(emul_ops.to_device_nhwc8(_x(1, 224)))


def test_kecam_cam():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import kecam_models as km
    from oracle import kecam_ref as ref
    x = _x(2, 96)
    # seeds: with seed 7 ResNetD's score map is negative everywhere (post-ReLU features, negative pooled gradient): a legitimate all-zero
    # map that pins nothing, so that graph takes the next seed whose map is not empty
    for tag, cfg, attn, seed in (("ResNest", dict(km.RESNEST50, num_blocks=(1, 1, 1, 1)), "sa", 7),
                                 ("ResNetD", dict(km.RESNET200D, num_blocks=(1, 2, 1, 1)), None, 37)):
        p = km.resnest_synth_params(seed, cfg=cfg)
        with torch.no_grad():
            f = ref.resnest_features(p, x, num_blocks=cfg["num_blocks"], stem_width=cfg["stem_width"], attn=attn)
        _check_family(tag, lambda: km.ResNest(p, cfg=cfg, device="cpu"), x, f, p["predictions/kernel"], p["predictions/bias"], None)
    cfg = dict(km.NFNET_L0, num_blocks=(1, 2, 1, 1))
    p = km.nfnet_synth_params(8, cfg=cfg)
    with torch.no_grad():
        f = ref.nfnet_features(p, x, num_blocks=cfg["num_blocks"], num_features_factor=cfg["num_features_factor"])
    _check_family("ECA_NFNet", lambda: km.NormFreeNet(p, cfg=cfg, device="cpu"), x, f, p["predictions/kernel"], p["predictions/bias"], None)
    # (seed 9 gives EfficientNetV1B4 an empty score map, like ResNetD above)
    for base, depthes, seed in (("EfficientNetV2T", [1, 2, 1, 2, 1, 1], 9), ("EfficientNetV1B4", [1, 2, 1, 1, 2, 1, 1], 29)):
        name = base + "_small"
        km.EFFNET[name] = ref.EFFNET[name] = dict(km.EFFNET[base], depthes=depthes)
        try:
            p = km.effnet_synth_params(name, seed)
            with torch.no_grad():
                f = ref.effnet_features(p, x, name)
            _check_family(name, lambda: km.EfficientNet(p, name, device="cpu"), x, f, p["predictions/kernel"], p["predictions/bias"], None)
        finally:
            del km.EFFNET[name], ref.EFFNET[name]


def test_hornet_cam():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import hornet
    from oracle import hornet_ref as ref
    cfg = dict(hornet.CONFIGS["hornet_tiny"], num_blocks=(1, 1, 2, 1))
    p = hornet.synth_params(cfg, 10)
    x = _x(2, 64)
    with torch.no_grad():
        f = ref.forward_features(p, x, cfg)
    _check_family("hornet", lambda: hornet.HorNet(p, **cfg, device="cpu"), x, f, p["predictions/kernel"], p["predictions/bias"],
                  (p["pre_output_ln/gamma"], p["pre_output_ln/beta"], ref.LN_EPS))


# ---- compose, overlay, colour table, PNG -----------------------------------------------------------------------------------------------
def test_compose_reference_matches_interpolate():
    """the bilinear rule of the composition (half-pixel centres, edge clamp) is torch's align_corners=False rule"""
    g = torch.Generator().manual_seed(3)
    maps = [torch.rand(3, 7, 7, generator=g, dtype=torch.float64), torch.rand(3, 13, 9, generator=g, dtype=torch.float64)]
    peaks = [m.flatten(1).max(1).values for m in maps]
    peaks[1][2] = 0.0                                                   # one member has nothing to say about image 2
    maps[1][2] = 0.0
    sizes = [(200, 200), (31, 57), (1, 1)]
    out = CR.compose_ref(maps, peaks, sizes, (200, 200))
    F = torch.nn.functional
    for i, (h, w) in enumerate(sizes):
        want = sum(F.interpolate(CR.normalise(m, p)[i][None, None], size=(h, w), mode="bilinear", align_corners=False)[0, 0]
                   for m, p in zip(maps, peaks)) / 2
        assert float((out[i, :h, :w] - want).abs().max()) <= 1e-12
        assert float(out[i, h:].abs().max() if h < 200 else 0) == 0 and float(out[i, :, w:].abs().max() if w < 200 else 0) == 0
    assert float(out.min()) >= 0 and float(out.max()) <= 1 + 1e-12


def test_jet_table_and_overlay_reference():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import cam as camlib
    t = camlib.jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    # the published breakpoints: dark blue at 0, dark red at 1, green saturated in the middle, blue gone past 0.65
    assert t[0].tolist() == [0, 0, 128] and t[255].tolist() == [128, 0, 0]
    assert t[128, 1] == 255 and int(t[170:, 2].max()) == 0 and int(t[:89, 0].max()) == 0
    assert (np.diff(t[:96, 1].astype(int)) >= 0).all() and (np.diff(t[164:, 1].astype(int)) <= 0).all()
    rgb = torch.tensor([[[[10, 250, 100], [0, 0, 0]]]], dtype=torch.uint8)
    m = torch.tensor([[[255, 0]]], dtype=torch.uint8)
    o = CR.overlay_ref(rgb, m, torch.from_numpy(t), 0.4)
    assert o[0, 0, 0].tolist() == [61, 250, 100] and o[0, 0, 1].tolist() == [0, 0, 51]     # 10 + 0.4 * 128 = 61.2; 0.4 * 128 = 51.2
    assert CR.overlay_ref(rgb, m, torch.from_numpy(t), 4.0)[0, 0, 0].tolist() == [255, 250, 100]   # clipped


def _read_png(raw):
    """minimal reader for what the writer emits: 8-bit gray / RGB, not interlaced, filter type 0 on every row"""
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, ihdr = 8, b"", None
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        data = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + data) & 0xFFFFFFFF
        if tag == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", data)
        if tag == b"IDAT":
            idat += data
        pos += 12 + n
    w, h, depth, ctype, comp, flt, lace = ihdr
    assert (depth, comp, flt, lace) == (8, 0, 0, 0) and ctype in (0, 2)
    ch = 3 if ctype == 2 else 1
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape((h, w, 3) if ch == 3 else (h, w))


@pytest.mark.parametrize("shape", [(5, 7, 3), (1, 1, 3), (9, 4)])
def test_png_writer_round_trip(shape, tmp_path):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import cam as camlib, pipeline
    img = np.random.default_rng(1).integers(0, 256, size=shape, dtype=np.uint8)
    path = tmp_path / "o.png"
    camlib.write_png(str(path), img)
    raw = path.read_bytes()
    assert np.array_equal(_read_png(raw), img)
    st = pipeline.inflate_pngs([raw])                       # the project's own PNG header parser and inflate accept the file
    d = st.desc[0]
    assert (d.height, d.width, d.bit_depth, d.color_type, d.interlace) == (shape[0], shape[1], 8, 2 if len(shape) == 3 else 0, 0)
    with pytest.raises(Exception):
        camlib.png_bytes(img.astype(np.float32))


def test_heatmap_stems_do_not_collide():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import cam as camlib
    assert camlib.heatmap_stem("a/1.jpg") != camlib.heatmap_stem("b/1.jpg") and camlib.heatmap_stem("x.png") == "x"


def test_cam_entry_points_check_arguments_without_a_gpu():
    import ctypes as C
    import vipcup_amd  # noqa: F401
    from vipcup_amd import _abi
    lib = _abi.lib()
    p = C.c_void_p(64)
    for fn in (lib.vip_cam_f32, lib.vip_cam_s32, lib.vip_cam_h2):
        assert fn(None, None, None, 0.0, p, None, p, p, p, 2, 49, 64, 64, 49 * 64, 1, 1, -1, None) == -1
        assert fn(p, p, None, 1e-6, p, None, p, p, p, 2, 49, 64, 64, 49 * 64, 1, 1, -1, None) == -1          # gamma without beta
        assert fn(p, None, None, 0.0, p, None, p, p, p, 2, 49, 64, 64, 49 * 64, 3, 2, 3, None) == -1 and b"target" in lib.vip_last_error()
        assert fn(p, None, None, 0.0, p, None, p, p, p, 2, 49, 64, 64, 49 * 64, 1, 5, -1, None) == -1 and b"activation" in lib.vip_last_error()
        assert fn(p, None, None, 0.0, p, None, p, p, p, 2, 49, 8192, 8192, 49 * 8192, 1, 1, -1, None) == -3
        assert fn(p, None, None, 0.0, p, None, p, p, p, 2, 49, 60, 60, 49 * 60 + 2, 1, 1, -1, None) == -2
    one = (C.c_void_p * 1)(64)
    gi = (C.c_int * 1)(7)
    wf = (C.c_float * 1)(1.0)
    assert lib.vip_cam_compose_f32(one, gi, gi, one, wf, 17, p, 1, 8, 8, p, 0, None) == -1 and b"members" in lib.vip_last_error()
    assert lib.vip_cam_compose_f32(one, gi, gi, one, wf, 1, None, 1, 8, 8, p, 0, None) == -1
    assert lib.vip_cam_compose_f32(one, (C.c_int * 1)(0), gi, one, wf, 1, p, 1, 8, 8, p, 0, None) == -1
    assert lib.vip_cam_overlay_u8(p, p, None, 0.4, 1, 8, 8, p, None) == -1
    assert lib.vip_cam_overlay_u8(p, p, p, -1.0, 1, 8, 8, p, None) == -1
