"""What the evidence maps cost: the ensemble step on a resident decoded batch without maps (``ensemble._score_batch``) and with them
(``ensemble.explain_batch`` + the copy of the full-size maps to the host) in fp32 and uint8.  One process, one GPU; every figure is the
mean over ``--steps`` synchronised steps after ``--warmup``.  Prints one line per variant and a JSON summary.

    python tools/bench_cam.py [--workload ensemble8] [--batch 256] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default=None)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_cam.py needs a GPU: the HIP path has no CPU fallback")
    import vipcup_amd  # noqa: F401
    from tools.make_synth import synth_jpeg
    from vipcup_amd import ensemble, pipeline, workloads, zoo
    name = a.workload or workloads.DEFAULT
    keys = workloads.member_list(name)
    members = [zoo.build_member(k) for k in keys]
    batch = pipeline.decode_jpegs([synth_jpeg(i) for i in range(a.batch)])
    why = ensemble.cam_support(members)

    def plain():
        return ensemble._score_batch(batch, members)

    def maps(fmt):
        def run():
            ex = ensemble.explain_batch(batch, members, out=fmt)
            ex.map.cpu()
            return ex.scores
        return run

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.steps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sum(ts) / len(ts), min(ts), max(ts)

    out = {"workload": name, "batch": a.batch, "steps": a.steps, "members_with_map": [k for k, v in why.items() if v is None],
           "members_without_map": [k for k, v in why.items() if v is not None], "ms_per_step": {}}
    ref = plain()
    for tag, fn in (("scores only", plain), ("scores + maps fp32 -> host", maps("f32")), ("scores + maps uint8 -> host", maps("u8")),
                    ("scores only (again)", plain)):
        mean, lo, hi = timed(fn)
        same = bool(torch.equal(fn(), ref))
        out["ms_per_step"][tag] = {"mean": mean, "min": lo, "max": hi, "scores_equal": same}
        print(f"{tag:30s} {mean:8.2f} ms/step (min {lo:.2f}, max {hi:.2f}) over {a.steps} steps; scores bit-equal to the plain step: {same}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
