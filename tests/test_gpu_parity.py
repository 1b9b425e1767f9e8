"""GPU parity beyond the 16-image CLI test: images that are NOT from the synthetic family, every shipped member
inside a 256-image batch (the kernels bench.py times), and the BASELINE config-4 / config-5 member lists."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _parity as P  # noqa: E402
from tools.make_synth import synth_jpeg  # noqa: E402


def _gpu_logits(key, raws, batch=None):
    import vipcup_amd  # noqa: F401
    from vipcup_amd import pipeline
    spec, model = P.gpu_member(key)
    x = pipeline.decode_jpegs(raws).resized(spec.input_hw, spec.input_hw)
    return model.logits(x)[:, 0].float().cpu().numpy()


def _members():
    from vipcup_amd import zoo
    return list(zoo.ENSEMBLE)


def test_real_photo_tiles_match_oracle(report):
    """Off the calibration distribution: the bias calibration (ops.calibration) is fitted on a seeded batch of the synthetic family;
    these 12 tiles are photographs.  Same bounds as on the synthetic set."""
    raws = P.real_photo_tiles()
    assert len(raws) >= 12
    probs_g, probs_o, over = [], [], {}
    for key in _members():
        z = P.oracle_logits(key, "photo_tiles", raws)
        zg = _gpu_logits(key, raws)
        dz = np.abs(zg - z)
        # photographs drive the synthetic heads far outside their calibrated range (logits to +-20, where the sigmoid is flat):
        # the error of a logit grows with its distance from the bias, so the per-image bound is relative beyond |z| = 3 (2 sigma
        # of the calibrated spread)
        rel = dz / np.maximum(1.0, np.abs(z) / 3.0)
        report(f"[photo] {key:22s} max|dz|={dz.max():.3e} mean|dz|={dz.mean():.3e} max|dz|/max(1,|z|/3)={rel.max():.3e} "
               f"z range [{z.min():+.2f},{z.max():+.2f}]{'' if dz.max() <= P.TOL_NORTH_STAR else '   ABOVE north-star 1e-3'}")
        if dz.max() > P.MEMBER_CEILING_PHOTO_ABS[key]:             # absolute: no |z|-relative discount
            over[key] = float(dz.max())
        probs_g.append(P.sigmoid(zg))
        probs_o.append(P.sigmoid(z))
    pg, po = np.mean(probs_g, 0), np.mean(probs_o, 0)
    dm = np.abs(pg - po).max()
    dl = np.abs(P.logit(pg) - P.logit(po)).max()
    report(f"[photo] ensemble mean max|dp|={dm:.3e}  max|d logit(mean)|={dl:.3e}")
    assert not over, f"members above their absolute fast-mode ceiling on photo tiles: {over}"
    assert dm <= P.TOL_ENSEMBLE_PROB and dl <= P.FAST_ENSEMBLE_LOGIT_CEILING["ensemble"]


@pytest.mark.parametrize("key", ["convnext_tiny_in22k", "resnest50", "gcvit_tiny", "efficientnet_v2t", "efficientnet_v1b4",
                                 "eca_nfnet_l0", "resnet_rs50"])
def test_member_inside_batch_256(key, report):
    """The dispatcher keys on the row count M = B x pixels, so at B = 256 the deep stages run on other kernels than in the
    8-image model tests (and the fused MLP / streaming GEMMs switch on).  The batch-edge images P.B256_EDGE_IMAGES (first, middle and
    last of the 256: the last M tile, the tile where a persistent workgroup wraps around) vs the oracle, and vs the same 8 images
    scored alone."""
    raws = [synth_jpeg(1000 + i) for i in range(256)]
    idx = P.B256_EDGE_IMAGES
    edge = [raws[i] for i in idx]
    z = P.oracle_logits(key, "b256_edges", edge)
    z256 = _gpu_logits(key, raws)
    z8 = _gpu_logits(key, edge)
    assert np.isfinite(z256).all()
    d_or = np.abs(z256[idx] - z).max()
    d_self = np.abs(z256[idx] - z8).max()
    report(f"[b256] {key:22s} images {idx} of a 256-batch: max|dz| vs oracle {d_or:.3e}, vs the B=8 run {d_self:.3e}; "
           f"logit spread over the batch {z256.std():.2f}")
    assert d_or <= P.MEMBER_CEILING[key]
    assert d_self <= 2 * P.MEMBER_CEILING[key]      # two independent fp16 realisations of the same graph


@pytest.mark.parametrize("precision", ["fast", "strict"])
@pytest.mark.parametrize("name", ["ensemble4", "ensemble8"])
def test_workload_scores_match_oracle(name, precision, report):
    """BASELINE configs 4 and 5 through the bench's own workload object: JPEG bytes in host RAM -> scores.  strict: logit(ensemble
    mean) within the north-star 1e-3; fast: within its stated fp16-storage ceiling (tests/_parity.py)."""
    import vipcup_amd  # noqa: F401
    from vipcup_amd import workloads
    n = 16
    raws = [synth_jpeg(300 + i) for i in range(n)]
    wl = workloads.build(name, batch=n, jpegs=raws, precision=precision,
                         models=[P.gpu_member(k, precision) for k in workloads.member_list(name)])
    got = wl.step().float().cpu().numpy().reshape(-1)
    got2 = wl.step().float().cpu().numpy().reshape(-1)        # the second step runs on the member streams
    probs = [P.sigmoid(P.oracle_logits(k, "wl16", raws)) for k in wl.members]
    want = np.mean(probs, 0)
    d, d2 = np.abs(got - want).max(), np.abs(got2 - want).max()
    dl = max(np.abs(P.logit(got) - P.logit(want)).max(), np.abs(P.logit(got2) - P.logit(want)).max())
    report(f"[{name}/{precision}] {len(wl.members)} members, 16 JPEGs -> ensemble mean: max|dp| vs oracle {d:.3e} (step 2: {d2:.3e}), "
           f"max|d logit(mean)| {dl:.3e}")
    tol = P.TOL_NORTH_STAR if precision == "strict" else P.FAST_ENSEMBLE_LOGIT_CEILING[name]
    assert dl <= tol
    # pipelined steps (what bench.py times): step i's scores come back from step i+1, the last from flush(); same images, same scores
    assert wl.step(pipelined=True) is None
    p1 = wl.step(pipelined=True).float().cpu().numpy().reshape(-1)
    p2 = wl.flush().float().cpu().numpy().reshape(-1)
    assert wl.flush() is not None                                # nothing in flight any more: the last scores again
    dp = max(np.abs(p1 - got2).max(), np.abs(p2 - got2).max())
    report(f"[{name}/{precision}] pipelined steps vs joined steps: max|dp| {dp:.3e}")
    # the same kernels on the same inputs in another enqueue order: bitwise equal, or it is a race
    assert dp == 0.0
    wl.close()
