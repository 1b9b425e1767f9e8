"""The depthwise case table (tests/_dw_cases.py) checks itself, without a GPU: the operands really make the reference exact, every row
reaches the kernel it names (the project's dry runs; nothing is launched), the operands tell the classic depthwise mistakes apart, the
rows hold the edges they claim, and the table carries every (k, stride, pad) the models hand the depthwise operators."""
import contextlib
import dataclasses

import pytest
import torch

from tests import _dw_cases as T
from tests import emul_ops

ALL = T.ROWS + T.POOL            # every row runs exactly with its `act` (None / relu)


def _ops():
    import vipcup_amd  # noqa: F401
    from vipcup_amd import ops
    return ops


_REF = {}


def _ref(row, act="row"):
    """ref64 of a row, computed once (act = None: the linear map)"""
    act = row.act if act == "row" else act
    key = (row.id, act)
    if key not in _REF:
        x, w, b = T.operands(row)
        _REF[key] = T.ref64(x, w, b, row.stride, row.pad, act)
    return _REF[key]


def test_table_is_well_formed():
    ids = [r.id for r in ALL]
    assert len(set(ids)) == len(ids)
    for r in ALL:
        assert r.act in T.EXACT_ACTS and r.nonlinear in (None, "silu", "gelu"), r.id
        assert r.storage in ("f16", "h2", "s32") and r.C % 8 == 0 and r.what, r.id
        assert _ref(r).shape == (r.B, *T.out_hw(r), r.C), r.id


@pytest.mark.parametrize("row", ALL, ids=lambda r: r.id)
def test_reference_is_exact(row):
    x, w, b = T.operands(row)
    assert torch.equal(x, x.round()) and x.abs().max() <= 2
    assert torch.equal(w * 4, (w * 4).round()) and w.abs().max() <= 1
    assert torch.equal(b * 4, (b * 4).round()) and b.abs().max() <= 2
    ref = _ref(row)
    assert torch.equal(ref.half().double(), ref), "the reference leaves the fp16 grid"
    assert 4 * ref.abs().max().item() < 2048
    # any summation order is exact: the largest partial sum any kernel can form is sum |x| |w| + |b|, in quarter units below 2^11
    worst = T.ref64(x.abs(), w.abs(), b.abs(), row.stride, row.pad, None)
    assert 4 * worst.max().item() < 2048
    # fp32 arithmetic gives the same bits
    ref32 = T.R.act(T.R.dwconv2d(x, w, b, row.stride, row.pad), row.act)
    assert torch.equal(ref32.double(), ref)
    # the outputs are not trivially zero.  The bound is on the LINEAR map (the issue's 90 %); ReLU zeroes the negative half of a
    # distribution that is symmetric up to the bias, so an activated map keeps at least a third of its elements
    lin = _ref(row, None)
    assert (lin != 0).double().mean().item() >= 0.90
    if row.act == "relu":
        assert (ref != 0).double().mean().item() >= 1 / 3
    assert len({tuple(f.tolist()) for f in w[..., 0].reshape(-1, row.C).t()}) == row.C, "two channels share a filter"


@pytest.mark.parametrize("row", ALL, ids=lambda r: r.id)
def test_row_reaches_its_kernel(row):
    ops = _ops()
    assert ops._DW_H2_LDS == 3, "the table is written for the default switch"
    assert T.reaches(row, ops) is None, T.reaches(row, ops)


def test_dry_run_of_the_packed_tile_kernel():
    """vip_dwconv2d_tile_plan_h2 is the arithmetic of launch_tile_h2: 4-channel chunks, 32 per block, 24 on the ConvNeXt widths"""
    ops = _ops()
    lib = ops._abi.lib()
    assert ops.dwconv_tile_plan(2, 7, 9, 40, 3, packed=True) == (1, 1, dict(cb=10, tiles_per_block=25, channel_blocks=1, cap=2048))
    assert ops.dwconv_tile_plan(2, 8, 8, 96, 5, pad=(1, 2, 2, 1), packed=True)[2] == dict(cb=24, tiles_per_block=10, channel_blocks=1, cap=2048)
    assert ops.dwconv_tile_plan(2, 7, 5, 136, 5, packed=True)[2] == dict(cb=32, tiles_per_block=8, channel_blocks=2, cap=1024)
    assert ops.dwconv_tile_plan(2, 7, 9, 40, 3, packed=True, pooled=True) is None            # no pooling form
    assert lib.vip_dwconv2d_tile_plan_h2(2, 14, 15, 64, 3, 2, 1, 1, 7, 8, None, None) == 0    # stride 2
    assert lib.vip_dwconv2d_tile_plan_h2(2, 14, 15, 64, 4, 1, 1, 1, 14, 15, None, None) == 0  # k = 4
    assert lib.vip_dwconv2d_tile_plan_h2(2, 14, 15, 60, 3, 1, 1, 1, 14, 15, None, None) == 0  # C % 8
    assert lib.vip_dwconv2d_tile_plan_h2(2, 14, 15, 64, 3, 1, 1, 1, 30, 15, None, None) == 0  # no stride-1 window gives that many rows


def test_lds_kernel_declines_no_small_shape():
    """the search the table's header reports: over maps up to 40 x 40 (and a few long, thin ones), every k and pad extent, batches and
    channel counts, the LDS-staged kernel takes everything - so dwconv_tile_h2_kernel is reached through the switch, never by rejection"""
    lib = _ops()._abi.lib()
    sizes = list(range(1, 41)) + [99, 224, 1000]
    for k in (3, 5, 7):
        for H in sizes:
            for W in (1, 2, H, 40, 1000):
                for grow in (0, k - 1, 2 * (k - 1)):              # VALID ... the widest pad the kernels take
                    Ho, Wo = H + grow - k + 1, W + grow - k + 1
                    if Ho <= 0 or Wo <= 0:
                        continue
                    for B, C in ((1, 8), (3, 40), (256, 136)):
                        if 4 * B * max(H * W, Ho * Wo) * C >= 1 << 31:          # its one limit: tensors of 4 GiB; stay well below
                            continue
                        assert lib.vip_dwconv2d_s1_supported_h2(B, H, W, C, k, Ho, Wo) == 1, (B, H, W, C, k, Ho, Wo)


def _row(rid):
    return next(r for r in ALL if r.id == rid)


def test_rows_hold_the_edges_they_claim():
    ops = _ops()
    # fp16 tile kernel: the channel-block cases, tile tails on both axes on every stride-1 row
    geom = {r.C: ops.dwconv_tile_plan(r.B, r.H, r.W, r.C, r.k, pad=r.pad)[2] for r in T.ROWS if r.kernel == "dwconv_tile_kernel"}
    assert (geom[8]["cb"], geom[8]["tiles_per_block"]) == (1, 256)
    assert (geom[40]["cb"], geom[40]["tiles_per_block"]) == (5, 51)                          # 255 live lanes
    assert (geom[96]["cb"], geom[96]["tiles_per_block"]) == (12, 21)                         # 252 live lanes
    assert (geom[136]["cb"], geom[136]["channel_blocks"]) == (16, 2)                         # the second block: 1 of 16 chunks
    geom = {r.C: ops.dwconv_tile_plan(r.B, r.H, r.W, r.C, r.k, pad=r.pad, packed=True)[2] for r in T.ROWS if r.kernel == "dwconv_tile_h2_kernel"}
    assert geom[40]["cb"] == 10 and geom[96]["cb"] == 24 and (geom[136]["cb"], geom[136]["channel_blocks"]) == (32, 2)   # second block: 2 chunks
    for r in T.ROWS:
        Ho, Wo = T.out_hw(r)
        if r.stride == 1:
            t, tw = T.TILE[r.k]
            assert Ho % t and Wo % tw and Wo % 4, (r.id, Ho, Wo)                             # Wo % 4: the plain strict kernel's thread tile
        else:
            assert Wo % 2 == 1, (r.id, Wo)
    assert any(r.C % 16 for r in T.ROWS if r.kernel == "dwconv_lds_h2_kernel")
    assert any(r.H < r.k and r.W < r.k for r in T.ROWS if r.stride == 1)
    for kernel in sorted({(r.storage, r.kernel) for r in T.ROWS}):
        mine = [r for r in T.ROWS if (r.storage, r.kernel) == kernel]
        assert any(r.pad[0] != r.pad[1] or r.pad[2] != r.pad[3] for r in mine), f"{kernel}: no asymmetric pad"
        assert any(r.nonlinear for r in mine), f"{kernel}: no silu / gelu row"
        if mine[0].stride == 1 and kernel[0] != "s32":
            assert {r.k for r in mine} == {3, 5, 7}, kernel
    # TF SAME at stride 2, per storage: the pads of every parity
    for storage in ("f16", "h2", "s32"):
        pads = {(r.k, r.pad) for r in T.ROWS if r.storage == storage and r.stride == 2}
        assert pads >= {(3, (0, 1, 0, 1)), (3, (1, 1, 1, 1)), (3, (0, 1, 1, 1)), (5, (1, 2, 1, 2)), (5, (2, 2, 2, 2)), (5, (1, 2, 2, 2))}
    for r in T.ROWS:
        if r.stride == 2:                                                                     # the pads ARE TensorFlow's for the map
            from vipcup_amd.kecam_models import same_pad
            assert r.pad == (*same_pad(r.H, r.k, 2), *same_pad(r.W, r.k, 2)), r.id
    # uneven XCD bands, one row per tile kernel
    for rid, packed in (("f16-tile-k3-c64-xcd", False), ("h2-tile-k3-c64-xcd", True)):
        r = _row(rid)
        groups, workgroups, _ = ops.dwconv_tile_plan(r.B, r.H, r.W, r.C, r.k, pad=r.pad, packed=packed)
        assert groups in T.XCD_GROUPS and workgroups == groups, (rid, groups, workgroups)      # gridDim.x >= 8: the band split runs
        chunk = -(-groups // 8)
        bands = [max(0, min(groups, (x + 1) * chunk) - x * chunk) for x in range(8)]
        assert bands[-1] == 0 and sum(bands) == groups, bands                                  # the last XCD's band is empty
    # the pooling form of the fp16 tile kernel
    plans = []
    for r in T.POOL:
        if r.storage != "f16":
            continue
        Ho, Wo = T.out_hw(r)
        parts = ops._abi.lib().vip_dwconv2d_pool_parts(r.B, r.H, r.W, r.C, r.k, 1, Ho, Wo)
        groups, _, g = ops.dwconv_tile_plan(r.B, r.H, r.W, r.C, r.k, pad=r.pad, pooled=True)
        assert groups == r.B * parts
        t, tw = T.TILE[r.k]
        tiles = -(-Ho // t) * -(-Wo // tw)
        plans.append((parts, tiles % g["tiles_per_block"], Ho % t, Wo % tw))
    assert any(p[0] > 1 for p in plans) and any(p[1] for p in plans) and any(p[2] and p[3] for p in plans), plans
    assert T.MFMA and all(r.k in (5, 7) and r.C % 16 == 0 and r.stride == 1 for r in T.MFMA)


@pytest.mark.parametrize("row", ALL, ids=lambda r: r.id)
def test_operands_discriminate(row):
    """a kernel that makes one of these mistakes cannot pass the row"""
    x, w, b = T.operands(row)
    ref = _ref(row)
    pt, pb, pl, pr = row.pad
    wrong = {}
    if pt != pb:
        wrong["pt / pb swapped"] = T.ref64(x, w, b, row.stride, (pb, pt, pl, pr), row.act)
    if pl != pr:
        wrong["pl / pr swapped"] = T.ref64(x, w, b, row.stride, (pt, pb, pr, pl), row.act)
    wrong["filter transposed"] = T.ref64(x, w.transpose(0, 1).contiguous(), b, row.stride, row.pad, row.act)
    if row.C > 8:                                   # on 8 channels a rotation by 8 is the identity
        wrong["filter rotated by 8 channels"] = T.ref64(x, torch.roll(w, 8, 2), b, row.stride, row.pad, row.act)
    wrong["filter rotated by 4 channels"] = T.ref64(x, torch.roll(w, 4, 2), b, row.stride, row.pad, row.act)   # the strict kernels' chunk
    xr, xc = x.clone(), x.clone()
    xr[:, -1] = 0
    xc[:, :, -1] = 0
    wrong["last input row read as zero"] = T.ref64(xr, w, b, row.stride, row.pad, row.act)
    wrong["last input column read as zero"] = T.ref64(xc, w, b, row.stride, row.pad, row.act)
    for what, bad in wrong.items():
        assert bad.shape == ref.shape and not torch.equal(bad, ref), f"{row.id} cannot tell: {what}"


# ---- the table against the models --------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _recording(seen):
    """inside emul_ops.patched(): the three depthwise entry points of vipcup_amd.ops also record (k, stride, pad)"""
    ops = _ops()
    saved = {n: getattr(ops, n) for n in ("dwconv2d", "dwconv2d_se", "mbconv_expand_dw")}

    def wrap(fn, at):
        def rec(*a, **kw):
            k, s, pad = a[at:at + 3]
            seen.add((int(k), int(s), tuple(int(p) for p in pad)))
            return fn(*a, **kw)
        return rec
    try:
        ops.dwconv2d = wrap(saved["dwconv2d"], 3)                       # (x, w, bias, k, stride, pad, ...)
        ops.dwconv2d_se = wrap(saved["dwconv2d_se"], 3)
        ops.mbconv_expand_dw = wrap(saved["mbconv_expand_dw"], 4)       # (x, cw, w, bias, k, stride, pad, ...)
        yield
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)


def _members():
    """(tag, constructor, input size from zoo): the reduced-depth constructors of tests/test_host_graphs_cpu.py"""
    import vipcup_amd  # noqa: F401
    from oracle import gcvit_ref
    from vipcup_amd import gcvit, hornet, kecam_models as km, tfimm_models as tm, zoo

    def effnet(base, depthes):
        def ctor():
            name = base + "_dw_cases"
            km.EFFNET[name] = dict(km.EFFNET[base], depthes=depthes)
            try:
                return km.EfficientNet(km.effnet_synth_params(name, 9), name, device="cpu")
            finally:
                del km.EFFNET[name]
        return ctor

    def gcv():
        cfg = dict(gcvit_ref.NAME2CONFIG["gcvit_tiny"], depths=(1, 1, 1, 1))
        return gcvit.GCViT(gcvit.synth_params(cfg, seed=4), **cfg, device="cpu")

    def convnext():
        cfg = dataclasses.replace(tm.CONVNEXT_CONFIGS["convnext_tiny_in22k"], nb_blocks=(1, 1, 1, 1))
        return tm.ConvNeXt(tm.convnext_synth_params(cfg, seed=5), cfg, device="cpu")

    def hor():
        cfg = dict(hornet.CONFIGS["hornet_tiny"], num_blocks=(1, 1, 1, 1))
        return hornet.HorNet(hornet.synth_params(cfg, 10), **cfg, device="cpu")

    size = lambda key: zoo.MEMBERS[key].input_hw  # noqa: E731
    return [("EfficientNetV2T", effnet("EfficientNetV2T", [1, 1, 1, 1, 1, 1]), size("efficientnet_v2t")),
            ("EfficientNetV1B4", effnet("EfficientNetV1B4", [1, 1, 1, 1, 1, 1, 1]), size("efficientnet_v1b4")),
            ("EfficientNetV2M", effnet("EfficientNetV2M", [1, 1, 1, 1, 1, 1, 1]), size("efficientnet_v2m")),
            ("GCViT", gcv, size("gcvit_tiny")), ("ConvNeXt", convnext, size("convnext_tiny_in22k")), ("HorNet", hor, size("hornet_base"))]


def test_table_holds_every_pad_the_models_use():
    seen = {}
    for tag, ctor, hw in _members():
        mine = set()
        x = torch.zeros(1, hw, hw, 3)
        with torch.no_grad(), emul_ops.patched(round_act=False), _recording(mine):
            ctor().logits(emul_ops.to_device_nhwc8(x))
        assert mine, f"{tag} made no depthwise call"
        seen[tag] = mine
    assert (3, 2, (0, 1, 0, 1)) in seen["EfficientNetV1B4"] and (5, 2, (1, 2, 1, 2)) in seen["EfficientNetV1B4"]     # the asymmetric pads
    for storage in ("f16", "h2"):
        table = {(r.k, r.stride, r.pad) for r in ALL if r.storage == storage}
        for tag, mine in seen.items():
            assert mine <= table, f"{tag}: {sorted(mine - table)} have no {storage} row"
