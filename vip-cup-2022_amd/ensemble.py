"""Ensemble scoring — the MI355X counterpart of ``predict_soln`` (main.py:58-149).

Reference flow per model: rebuild the dataset (re-decoding every JPEG), ``model.predict`` in batches of 128,
mean over TTA (:111), multi-class -> binary ``1 - p[:,0]`` (:113-114), mean over folds (:121); then across
models: concat, ``groupby(filename).mean()`` (:142-143), ``(mean > thr) * 1.0`` (:144), CSV (:145).

Here: each batch of files is decoded ONCE, every member consumes the resident pixels at its own resolution.
With N > 1 processes the work is a grid of (member, image-shard) units dealt to the ranks by a ``ShardPlan``:
``images`` (every rank holds all members and scores its own image shard - what MirroredStrategy does, utils/device.py:7),
``members`` (rank r owns members m = r mod world and sees every image - the one-model-per-GPU split of BASELINE.json) or
``hybrid`` (longest-processing-time-first packing of the units by measured ms/image).  In every mode the only exchange step
is ONE all-gather of the ranks' score payloads at the end.
"""
import inspect
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import chain

THR = 0.487          # main.py:225
REF_BATCH = 128      # 8 * NAME2BS.get(name, 16) for every shipped member (main.py:43-56,85)
NAME2BS = {          # main.py:43-56: per-replica batch of the larger members of earlier ensembles (x 8 replicas, :85)
    "convnext_large_384_in22ft1k-200x200": 16, "convnext_large_in22ft1k-200x200": 16, "convnext_base_384_in22ft1k-200x200": 32,
    "HorNetBase-200x200": 32, "EfficientNetV2M-200x200": 64, "convnext_base_in22k-200x200": 32, "ECA_NFNetL2-200x200": 32,
    "GCViTBase-224x224": 48, "ResNest200-200x200": 64, "EfficientNetV2L-200x200": 32, "ResNetRS200-200x200": 32,
    "ResNet200D-200x200": 32,
}


def ref_batch(ckpt_name: str) -> int:
    """the reference's batch size for a checkpoint directory name (main.py:85)"""
    return 8 * NAME2BS.get(ckpt_name, 16)


def shard_bounds(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous, balanced image shard of rank ``rank``: sizes differ by at most one."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


SHARD_MODES = ("images", "members", "hybrid")


class ShardPlan:
    """Who scores what: ``units[r]`` = {image-shard s: [member index, ...]} for rank r; image-shard s = ``shard_bounds(n, s, world)``.
    Every (member, shard) pair is owned by exactly one rank.  The plan is a pure function of (mode, n_members, world, costs), so
    every rank derives the same one without talking to the others."""

    def __init__(self, mode: str, n_members: int, world: int, costs: Optional[Sequence[float]] = None):
        if mode not in SHARD_MODES:
            raise ValueError(f"shard mode {mode!r}: expected one of {SHARD_MODES}")
        self.mode, self.n_members, self.world = mode, n_members, world
        units: List[Dict[int, List[int]]] = [dict() for _ in range(world)]
        if mode == "images" or world == 1:
            for r in range(world):
                units[r][r] = list(range(n_members))
        elif mode == "members":
            for r in range(world):
                mine = [m for m in range(n_members) if m % world == r]
                if mine:
                    for s in range(world):
                        units[r][s] = list(mine)
        else:       # hybrid: LPT over the n_members x world units; a unit costs the member's ms/image (shards are equal-sized)
            c = [1.0] * n_members if costs is None else [float(v) for v in costs]
            assert len(c) == n_members
            order = sorted(((c[m], m, s) for m in range(n_members) for s in range(world)), key=lambda t: (-t[0], t[1], t[2]))
            load = [0.0] * world
            for cost, m, s in order:
                # least-loaded rank; ties go to the rank that already decodes shard s (no extra decode), then to the lowest rank
                r = min(range(world), key=lambda k: (round(load[k], 9), 0 if s in units[k] else 1, k))
                units[r].setdefault(s, []).append(m)
                load[r] += cost
            for r in range(world):
                for s in units[r]:
                    units[r][s].sort()
            self.load = load
        self.units = units

    def payload_len(self, rank: int, n_images: int) -> int:
        return sum(len(ms) * (shard_bounds(n_images, s, self.world)[1] - shard_bounds(n_images, s, self.world)[0])
                   for s, ms in self.units[rank].items())

    def describe(self) -> str:
        return "; ".join(f"rank {r}: " + ", ".join(f"shard {s} x members {ms}" for s, ms in sorted(u.items()))
                         for r, u in enumerate(self.units))


def plan_payload(plan: ShardPlan, rank: int, n_images: int, device):
    """This rank's exchange payload and where each of its units' scores go in it: ``(mine [width] fp32, {(s, m): 1-D view of mine})``.
    Producers write their scores STRAIGHT into the views (``ops.binary_score(p, out=view)``) - no staging copies."""
    world = plan.world
    width = max(max(plan.payload_len(r, n_images) for r in range(world)), 1)
    mine = torch.zeros((width,), dtype=torch.float32, device=device)
    views, off = {}, 0
    for s in sorted(plan.units[rank]):
        lo, hi = shard_bounds(n_images, s, world)
        for m in plan.units[rank][s]:
            views[(s, m)] = mine[off:off + (hi - lo)]
            off += hi - lo
    assert off == plan.payload_len(rank, n_images)
    return mine, views


def exchange_payload(plan: ShardPlan, rank: int, n_images: int, mine: torch.Tensor, dist=None) -> torch.Tensor:
    """The exchange step: ONE ``all_gather_into_tensor`` of the ranks' payloads (RCCL over xGMI on GPUs, gloo in the CPU tests);
    returns ``[n_members, n_images]`` on every rank.  One rank with the ``images`` plan: the payload already IS that matrix."""
    world, width = plan.world, mine.numel()
    gathered = dist is not None and world > 1
    if not gathered and world == 1 and width == plan.n_members * n_images and n_images > 0:
        return mine.view(plan.n_members, n_images)
    if gathered:
        allp = torch.empty((world * width,), dtype=torch.float32, device=mine.device)     # flat: every backend accepts this form
        dist.all_gather_into_tensor(allp, mine)
        allp = allp.view(world, width)
    else:
        allp = mine.view(1, width)
    full = torch.zeros((plan.n_members, n_images), dtype=torch.float32, device=mine.device)
    for r in (range(world) if gathered else [rank]):     # without an exchange only this rank's units are known
        off = 0
        for s in sorted(plan.units[r]):
            lo, hi = shard_bounds(n_images, s, world)
            for m in plan.units[r][s]:
                full[m, lo:hi] = allp[r if gathered else 0, off:off + (hi - lo)]
                off += hi - lo
    return full


def gather_plan_scores(plan: ShardPlan, rank: int, n_images: int, local: Dict[Tuple[int, int], torch.Tensor], dist=None,
                       device=None) -> torch.Tensor:
    """``plan_payload`` + ``exchange_payload`` for callers that hold their units' scores as separate tensors: ``local[(s, m)]`` =
    scores of member m on image-shard s (1-D, this rank's units).  Each rank's payload (its units back to back, in (shard, member)
    order, padded to the longest payload) goes through ONE ``all_gather_into_tensor``; returns ``[n_members, n_images]`` on every rank."""
    if device is None:
        device = next(iter(local.values())).device if local else torch.device("cpu")
    mine, views = plan_payload(plan, rank, n_images, device)
    for key, view in views.items():
        view.copy_(local[key].reshape(-1).to(torch.float32))
    return exchange_payload(plan, rank, n_images, mine, dist)


def to_binary(pred: np.ndarray) -> np.ndarray:
    """main.py:113-114: a multi-class head reports P(real) in column 0 -> P(synthetic) = 1 - p[:,0]"""
    pred = np.asarray(pred, dtype=np.float32)
    if pred.ndim == 1:
        pred = pred[:, None]
    return 1.0 - pred[:, 0:1] if pred.shape[1] > 1 else pred


def aggregate(filenames: Sequence[str], per_model: np.ndarray, thr: float = THR):
    """per_model ``[M, N]`` probabilities -> (sorted unique filenames, mean score, decision).
    Mirrors concat + groupby('filename').mean() (rows sorted by filename, duplicates averaged) and the strict
    ``> thr`` of main.py:142-144.  (The reference's own frame has a string-typed 'logit' column and fails on
    current pandas; the evident intent — the arithmetic mean — is what is computed.)"""
    names = np.asarray(filenames)
    uniq, inv = np.unique(names, return_inverse=True)
    mean_per_image = per_model.astype(np.float64).mean(axis=0)            # mean over models per row
    sums = np.zeros(len(uniq), np.float64)
    cnts = np.zeros(len(uniq), np.float64)
    np.add.at(sums, inv, mean_per_image)
    np.add.at(cnts, inv, 1.0)
    score = (sums / cnts).astype(np.float32)
    return uniq.tolist(), score, (score > thr).astype(np.float32)


def tta_flags(n_images: int, tta: int, seed: int = 0) -> np.ndarray:
    """The random draws of ``apply_augment`` (dataset/augment.py:153-182 with RandomFlip :115-120, RandomGray
    :142-146) for every (pass, image): bool ``[tta, n_images, 3]`` = (hflip, vflip, gray).  With probability 0.2 an
    image is left alone (``random_float() > 0.80``), otherwise hflip / vflip with p = 0.5 each and gray with p = 0.3.
    TensorFlow's RNG stream cannot be reproduced, so the draws come from a seeded numpy generator; they are a function
    of (seed, pass, image index) only, so the scores do not depend on batch size or on how images are sharded."""
    return np.stack([tta_flags_pass(n_images, t, seed) for t in range(tta)]) if tta > 0 else np.zeros((0, n_images, 3), dtype=bool)


def tta_flags_pass(n_images: int, t: int, seed: int = 0) -> np.ndarray:
    """the draws of pass ``t`` alone: bool ``[n_images, 3]`` (``tta_flags(n, T, seed)[t]`` for any T > t)"""
    out = np.zeros((n_images, 3), dtype=bool)
    u = np.random.default_rng([int(seed), int(t)]).random((n_images, 4))
    on = ~(u[:, 0] > 0.80)
    out[:, 0] = on & (u[:, 1] < 0.5)
    out[:, 1] = on & (u[:, 2] < 0.5)
    out[:, 2] = on & (u[:, 3] < 0.3)
    return out


def score_files(jpegs_for: Callable[[int, int], List[bytes]], n_images: int, members: List[Tuple[object, object]],
                batch_size: int = REF_BATCH, rank: int = 0, world: int = 1, dist=None,
                scorer: Optional[Callable] = None, tta: int = 1, tta_seed: int = 0,
                shard: str = "images", costs: Optional[Sequence[float]] = None,
                batch_scorer: Optional[Callable] = None, lossy_webp: Optional[bool] = None) -> np.ndarray:
    """Score images [0, n_images) with every member; returns ``[M, n_images]`` fp32 probabilities on every rank.
    ``lossy_webp``: the lossy WebP switch of ``pipeline.host_decode`` (None: the ``VIP_WEBP_LOSSY`` knob).

    ``jpegs_for(lo, hi)`` returns the JPEG / PNG byte strings of images lo..hi-1 (read lazily, per batch).
    ``members`` = [(spec, model)] with ``spec.input_hw`` and ``model.predict(x) -> [n, C]``.
    ``tta`` > 1: every image is scored ``tta`` times under ``apply_augment`` draws and the predictions are averaged
    (main.py:92,109-111, ``CFG.agg = 'mean'``); the JPEGs are still decoded once.
    ``shard`` / ``costs``: the ShardPlan mode and, for ``hybrid``, the per-member cost (ms/image; identical on every rank).
    A rank only calls ``model.predict`` of the members its plan names, so under ``members`` / ``hybrid`` the others need not
    be resident (``members[i][1]`` may be None there).
    ``scorer(raws, members[, flags]) -> [M, n]`` replaces the GPU path in the CPU (gloo) tests.
    ``batch_scorer(staged, members, b0, b1, after_fork) -> [M, n]`` replaces ``_score_batch`` for images b0..b1-1 and keeps the staged
    host decode and read-ahead (``main.py --heatmaps``: ``explain_batch`` plus the files it writes); not with ``tta`` > 1."""
    if batch_scorer is not None and tta > 1:
        raise ValueError("score_files: batch_scorer does not take TTA passes")
    plan = ShardPlan(shard, len(members), world, costs)
    flags_all = tta_flags(n_images, tta, tta_seed) if tta > 1 else None
    work = []                                   # (shard, member indices, b0, b1)
    for s in sorted(plan.units[rank]):
        lo, hi = shard_bounds(n_images, s, world)
        for b0 in range(lo, hi, batch_size):
            work.append((s, plan.units[rank][s], b0, min(b0 + batch_size, hi)))

    def host_stage(item):
        """file read + Huffman decode / inflate of one batch (C++ threads, the GIL is released inside the ctypes call)"""
        raws = jpegs_for(item[2], item[3])
        if scorer is not None:
            return raws
        from . import pipeline
        return pipeline.host_decode(raws, pinned=True, lossy_webp=lossy_webp)

    # read-ahead (the overlap the reference gets from tf.data's prefetch, dataset/dataset.py:101): while the GPU scores batch i the
    # host stage of batch i+2 runs on a worker thread, and the DEVICE half of batch i+1 (H2D of the coefficients, IDCT, colour) is
    # enqueued on the launching stream between the fork of the member streams and their join - that stream idles while the members
    # run, so the work lands under them instead of at the head of the next batch (MemberStreams.predict_all(after_fork=...))
    from collections import deque
    from concurrent.futures import ThreadPoolExecutor
    chunks: Dict[Tuple[int, int], List[torch.Tensor]] = {}
    with ThreadPoolExecutor(max_workers=1) as pool:
        todo = iter(work)
        futs: deque = deque()

        def submit_next():
            item = next(todo, None)
            if item is not None:
                futs.append(pool.submit(host_stage, item))

        submit_next()
        decoded = [None]

        def after_fork():
            if scorer is None and futs and decoded[0] is None:
                from . import pipeline
                st = futs.popleft().result()
                submit_next()
                decoded[0] = pipeline.decode_staged(st)

        for i, (s, midx, b0, b1) in enumerate(work):
            if decoded[0] is not None:
                staged, decoded[0] = decoded[0], None
            else:
                staged = futs.popleft().result()
                submit_next()
            sub = [members[m] for m in midx]
            fl = None if flags_all is None else flags_all[:, b0:b1]
            if scorer is not None:
                rows = scorer(staged, sub) if fl is None else scorer(staged, sub, fl)
            elif batch_scorer is not None:
                rows = batch_scorer(staged, sub, b0, b1, after_fork)
            else:
                rows = _score_batch(staged, sub, fl, after_fork=after_fork)
            for j, m in enumerate(midx):
                chunks.setdefault((s, m), []).append(rows[j])
    local = {k: torch.cat(v) for k, v in chunks.items()}
    if scorer is None:
        from . import ops
        if any(model is not None and member_dtype(model) == ops.PACKED for _, model in members):
            # packed strict members: no activation of any batch left the fp16 range of the storage.  The word is sticky, so ONE read
            # after the last batch covers them all, and the copy to the host below synchronises anyway: read-ahead and stream overlap
            # are untouched.  With several ranks the one that overflowed raises HERE, before the collective below, like any exception
            # in the middle of a run: the launcher ends the job, the other ranks do not get scores either
            ops.h2_check("score_files")
    dev = None
    if not local:
        dev = torch.device("cuda" if (scorer is None and torch.cuda.is_available()) else "cpu")
    for s in plan.units[rank]:                  # empty shards (more ranks than images)
        for m in plan.units[rank][s]:
            if (s, m) not in local:
                local[(s, m)] = torch.zeros((0,), dtype=torch.float32, device=dev or next(iter(local.values())).device)
    full = gather_plan_scores(plan, rank, n_images, local, dist, dev)
    return full.detach().float().cpu().numpy()


def member_dtype(model) -> torch.dtype:
    """activation dtype a member was built for (zoo.construct): packed pairs for "strict", fp32 for "f32", fp16 otherwise"""
    from . import ops
    return ops.act_dtype(getattr(model, "precision", "fast"))


def input_key(spec, model):
    """key of a member's input tensor in the ``inputs`` dictionaries below: one resize launch per (resolution, dtype)"""
    return (spec.input_hw, member_dtype(model))


def member_inputs(batch, members) -> Dict:
    """``{input_key: tensor}``: the decoded batch resized (cast -> bicubic -> /255, dataset.py:31-38) once per distinct
    (resolution, dtype) among ``members`` = [(spec, model)] (model None = not resident on this rank: skipped)."""
    out: Dict = {}
    for spec, model in members:
        if model is None:
            continue
        k = input_key(spec, model)
        if k not in out:
            out[k] = batch.resized(spec.input_hw, spec.input_hw, dtype=k[1])
    return out


def _record_stream(t, stream):
    if isinstance(t, torch.Tensor) and t.is_cuda:
        t.record_stream(stream)
    elif isinstance(t, (tuple, list)):             # a member call that returns several tensors (predict_with_cam)
        for u in t:
            _record_stream(u, stream)


def _predict(model, x):
    return model.predict(x)


def _input_for(inputs, spec, model):
    k = input_key(spec, model)
    return inputs[k] if k in inputs else inputs[spec.input_hw]      # plain {resolution: tensor} dictionaries are accepted too


class MemberStreams:
    """Runs the (independent) ensemble members on several HIP streams.

    A member's deep layers launch grids far smaller than the chip (M = 256*7*7 pixels, SE/ECA layers with M = 256)
    and every launch pays a dispatch gap; with the members spread over a few streams the hardware queues fill
    those holes with another member's kernels.  Members are packed onto streams longest-first from a one-off
    timing of each member.  The reference scores the checkpoints one after another (main.py:199-217); the
    result is order-independent (a mean over members), so only the schedule differs."""

    def __init__(self, n_streams: int):
        self.n = max(1, int(n_streams))
        self.streams = [torch.cuda.Stream() for _ in range(self.n)] if self.n > 1 else []
        self._assign: Dict[Tuple[str, ...], List[List[int]]] = {}    # per member list (a ShardPlan may hand over sub-lists)
        self.cost_ms: Dict[str, float] = {}                              # last one-off timing per member (ms per batch)

    def _calibrate(self, members, inputs, call=_predict):
        """one serial, timed pass; its predictions ARE the first batch's result (nothing is computed twice)"""
        cost, out = [], []
        for i, (spec, model) in enumerate(members):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out.append(call(model, _input_for(inputs, spec, model)))
            e1.record()
            e1.synchronize()
            cost.append(e0.elapsed_time(e1))
            self.cost_ms[spec.name] = cost[-1]
        order = sorted(range(len(members)), key=lambda i: -cost[i])
        load = [0.0] * self.n
        assign: List[List[int]] = [[] for _ in range(self.n)]
        for i in order:                                   # longest-processing-time-first packing
            j = min(range(self.n), key=lambda k: load[k])
            assign[j].append(i)
            load[j] += cost[i]
        self._assign[tuple(spec.name for spec, _ in members)] = assign
        return out

    def predict_all(self, members, inputs, after_fork=None, defer_join: bool = False, call=_predict):
        """inputs: {input_hw: tensor} produced on the current stream.  Returns member.predict() per member - or, with ``call``, whatever
        ``call(model, x)`` returns (a tensor or a tuple of tensors: ``explain_batch`` asks for the evidence map along with the prediction).
        ``after_fork()`` is called once the members are enqueued on their streams and BEFORE the current stream joins them: work it
        enqueues on the current stream (the next batch's H2D + IDCT) runs under the members instead of in front of the next step.
        ``defer_join``: return ``(predictions, join_events)`` without making the current stream wait - the caller joins later
        (``MemberStreams.join``), so the next batch's members can start on the streams that finish first."""
        if self.n <= 1 or len(members) <= 1:
            out = [call(model, _input_for(inputs, spec, model)) for spec, model in members]
            if after_fork is not None:
                after_fork()
            return (out, []) if defer_join else out
        assign = self._assign.get(tuple(spec.name for spec, _ in members))
        if assign is None:
            out = self._calibrate(members, inputs, call)
            if after_fork is not None:
                after_fork()
            return (out, []) if defer_join else out
        main = torch.cuda.current_stream()
        ready = torch.cuda.Event()
        ready.record(main)
        out = [None] * len(members)
        joins = []
        for st, idxs in zip(self.streams, assign):
            if not idxs:
                continue
            st.wait_event(ready)
            with torch.cuda.stream(st):
                for i in idxs:
                    spec, model = members[i]
                    x = _input_for(inputs, spec, model)
                    # allocator hygiene across streams: the input was allocated on the launching stream and is read here, the
                    # prediction is allocated here and read on the launching stream - tell the caching allocator, so that neither
                    # block can be handed out again while the other stream still has work queued on it (a caller that drops its
                    # reference early - or a deferred join - would otherwise race with the block's next owner)
                    _record_stream(x, st)
                    out[i] = call(model, x)
                    _record_stream(out[i], main)
            done = torch.cuda.Event()
            done.record(st)
            joins.append(done)
        if after_fork is not None:
            after_fork()
        if defer_join:
            return out, joins
        self.join(joins)
        return out

    @staticmethod
    def join(joins):
        main = torch.cuda.current_stream()
        for done in joins:
            main.wait_event(done)


def measure_costs(members, raws: Sequence[bytes], dist=None, rank: int = 0, lossy_webp: Optional[bool] = None) -> List[float]:
    """ms per image of every member on a sample batch (JPEG / PNG byte strings), timed on rank 0 (a serial pass, the one
    ``MemberStreams._calibrate`` makes) and broadcast so that every rank derives the SAME hybrid ShardPlan.  Set-up traffic
    (one float per member), not part of the per-image data path."""
    from . import pipeline
    costs = torch.zeros((len(members),), dtype=torch.float64, device="cuda")
    if rank == 0:
        batch = pipeline.decode_images(list(raws), lossy_webp=lossy_webp)
        inputs = member_inputs(batch, members)
        ms = MemberStreams(2)
        ms._calibrate(members, inputs)          # warm-up: first-launch costs (module load, attribute calls)
        ms._calibrate(members, inputs)
        costs = torch.tensor([ms.cost_ms[spec.name] / max(len(raws), 1) for spec, _ in members], dtype=torch.float64, device="cuda")
    if dist is not None:
        dist.broadcast(costs, src=0)
    return [float(v) for v in costs.cpu()]


def default_streams() -> int:
    import os
    return int(os.environ.get("VIP_STREAMS", "3"))


_MEMBER_STREAMS: Optional[MemberStreams] = None


def _score_batch(staged, members, flags: Optional[np.ndarray] = None, after_fork=None) -> torch.Tensor:
    """``staged`` = ``pipeline.host_decode(raws)`` (or the raw JPEG / PNG byte strings, or an already decoded batch).  ``after_fork``:
    called once, between the fork and the join of the member streams (see ``MemberStreams.predict_all``).  Decode once -> per member: resize
    to its resolution, predict, multi->binary.  Returns [M, n] (device).
    ``flags`` bool [tta, n, 3] (hflip, vflip, gray): one pass per row over augmented copies of the resized batch, mean
    over passes (the mean commutes with the multi->binary map 1 - p0)."""
    from . import pipeline
    batch = pipeline.as_batch(staged)
    hook = [after_fork]
    global _MEMBER_STREAMS
    if _MEMBER_STREAMS is None:
        _MEMBER_STREAMS = MemberStreams(default_streams())
    cache = member_inputs(batch, members)

    def one_pass(inputs):
        from . import ops
        preds = _MEMBER_STREAMS.predict_all(members, inputs, after_fork=hook[0])     # [n, C] fp32 each
        hook[0] = None
        rows = torch.empty((len(preds), preds[0].shape[0]), dtype=torch.float32, device=preds[0].device)
        for m, p in enumerate(preds):
            ops.binary_score(p, out=rows[m])                     # main.py:113-114
        return rows

    if flags is None:
        return one_pass(cache)
    acc = None
    for fl in flags:                                             # augment AFTER decode+resize, as dataset.py:88-99 maps it
        aug = {key: pipeline.apply_augment(x, fl[:, 0], fl[:, 1], fl[:, 2]) for key, x in cache.items()}
        s = one_pass(aug)
        acc = s if acc is None else acc + s
    return acc / float(len(flags))


def stress_variants(spec) -> List[Tuple[str, str, object]]:
    """``(label, kind, arg)`` of every single-variant row that ``spec`` asks for, in row order.  ``spec`` maps keywords of ``stress_batch``
    to their values; only the lists and switches of ``chain.STEPS`` are read, an absent one is empty.  The rows go kind by kind in the
    order of that table, each list in the table's order for its kind (sorted, never de-duplicated); ``(kind, arg)`` is what
    ``chain.parse_step(label)`` gives and what ``pipeline.apply_step`` takes."""
    out = []
    for kind, row in chain.STEPS.items():
        given = spec.get(row.keyword, ()) if row.keyword else ()
        if row.order is None:                                    # gray, bgr, equalize: a switch
            args = [None] if given else []
        elif kind == "flip":
            args = sorted(str(axis) for axis in given)
        else:
            args = [chain.step_arg(kind, u) for u in sorted((chain.step_units(kind, v) for v in given), reverse=row.order == "desc")]
        out += [(chain.step_label(kind, arg), kind, arg) for arg in args]
    return out


def _row_labels(qualities, variants, chains) -> List[str]:
    resaved = [chain.step_label("recompress", q) for q in qualities]
    return resaved + [v for label, _, _ in variants for v in [label] + [f"{label}_{q}" for q in resaved]] + [str(text) for text in chains]


def stress_labels(*args, **keywords) -> List[str]:
    """``stress_labels(qualities, scales=(), blurs=(), ...)``: the variant labels of ``stress_batch`` rows 1.., in row order.  Takes
    ``stress_batch``'s keywords in ``stress_batch``'s order, less the batch, the members, ``after_fork``, ``subsampling``,
    ``resize_filter`` and ``blur_radius``; the remaining options are accepted and change no label.
    ``q<Q>`` for every quality as given, then every single-variant label of ``stress_variants`` (spelled by ``chain.step_label``: the
    grammar is in ``chain``'s docstring; ``scales``, ``crops`` and ``webps`` largest first, every other list ascending by signed value, ``h``
    before ``v``), each followed by its ``_q<Q>`` labels, and last the ``chains`` in the order given, each under its own text
    (``r50+shp080+q75``) and never followed by ``_q<Q>`` labels."""
    spec = _LABEL_SIGNATURE.bind(*args, **keywords).arguments
    return _row_labels(spec["qualities"], stress_variants(spec), spec.get("chains", ()))


def stress_batch(staged, members, qualities: Sequence[int], subsampling: str = "4:2:0", after_fork=None, scales: Sequence[int] = (),
                 resize_filter: str = "bicubic", blurs: Sequence[float] = (), medians: Sequence[int] = (), blur_radius: Optional[int] = None,
                 flips: Sequence[str] = (), crops: Sequence[int] = (), rotations: Sequence[float] = (), crop_origin: str = "centre",
                 rotate_fill: str = "crop", gray: bool = False, bgr: bool = False, hues: Sequence[int] = (), saturations: Sequence[int] = (),
                 contrasts: Sequence[int] = (), brightnesses: Sequence[int] = (), gammas: Sequence[float] = (), noises: Sequence[float] = (),
                 mono_noises: Sequence[float] = (), speckles: Sequence[int] = (), impulses: Sequence[float] = (), noise_seed: int = 0,
                 noise_keys=None, sharpens: Sequence[int] = (), sharpen_sigma: float = 1.0, sharpen_radius: Optional[int] = None,
                 sharpen_threshold: int = 0, chains: Sequence[str] = (), autocontrasts: Sequence[int] = (),
                 autocontrast_lumas: Sequence[int] = (), equalize: bool = False, clahes: Sequence[float] = (), clahe_grid: int = 8,
                 webps: Sequence[int] = ()):
    """Stress test of one batch: ``_score_batch`` on the batch as it is - the same inputs, streams and calls, so row 0 is bit for bit what a
    plain run returns - and then on perturbed copies of the decoded pixels, each image at its own size, before any member's resize.
    ``staged`` as for ``_score_batch``; it is decoded once.
    Rows 1..Q: the batch re-saved as JPEG at every quality of ``qualities``, in the order given (``pipeline.recompress`` with
    ``subsampling``; dataset/augment.py:110-113).  With nothing else asked for the result is these rows, ``[1 + Q, M, n]`` fp32 (device).
    Then the variants of ``stress_variants``: every value of every list below, kind by kind in the order of ``chain.STEPS``, each made
    from the decoded batch by ``pipeline.apply_step``, scored unsaved and then re-saved at every quality - perturb first, ``recompress``
    second, the order in which the challenge's test images were made.  Kinds are combined only through a chain, so the grid stays linear:
    V variants cost V (1 + Q) plain runs, one perturbed batch alive at a time.
      ``scales`` (percents, largest first): ``pipeline.rescale`` with ``resize_filter``
      ``blurs`` (sigmas; ``blur_radius`` None = three sigma), ``medians`` (windows): ``pipeline.blur`` / ``median`` (dataset/augment.py:131-140)
      ``flips`` (axes "h" / "v"), ``crops`` (percents, largest first; ``crop_origin`` "centre" or "topleft"), ``rotations`` (degrees;
        ``rotate_fill`` "crop", "mirror" or "black"): ``pipeline.flip`` / ``crop`` / ``rotate`` (dataset/augment.py:68-120)
      ``gray``, ``bgr``, ``hues`` (integer degrees), ``saturations`` / ``contrasts`` (percents), ``brightnesses`` (percents of full scale),
        ``gammas``: the ``pipeline`` function of that name (dataset/augment.py:122-129, :142-151); the batch's mean colour, which
        ``contrast`` takes, is computed at most once
      ``noises`` / ``mono_noises`` (sigmas in levels), ``speckles``, ``impulses`` (percents): ``pipeline.noise``.  ``noise_seed`` and
        ``noise_keys`` (one integer per image, None: 0..n-1; ``pipeline.noise_keys`` of the file names makes a file's noise independent
        of its batch) select the random field, which all noise variants of a batch share; the keys go to the device at most once
      ``sharpens`` (integer percents 1..500): ``pipeline.sharpen`` with ``sharpen_sigma``, ``sharpen_radius`` (None = three sigma) and
        ``sharpen_threshold``, one launch per variant
      ``autocontrasts`` / ``autocontrast_lumas`` (integer cutoff percents 0..49), ``equalize``, ``clahes`` (clip limits 1.0..9.9;
        ``clahe_grid`` tiles per axis): ``pipeline.tone``, a curve measured from each image's own histogram, nothing returns to the host
      ``webps`` (qualities 1..100, largest first): ``pipeline.webp_recompress``, the image as a lossy WebP save gives it back
    Every list but ``scales``, ``crops`` and ``webps`` is taken ascending; no list is de-duplicated.
    Last the ``chains`` (chain texts, ``pipeline.parse_chain``: ``"r50+shp080+q75"``; scored in the order given): the decoded batch goes
    through each chain's steps left to right (``pipeline.apply_chain`` with this call's options, ``noise_seed`` and ``noise_keys``) and
    the result is scored ONCE, exactly as the chain is written: ``qualities`` do not multiply chain rows, a chain that should end in a
    re-save ends in a ``q`` step.  One chain's batch is alive at a time; C chains cost C plain runs.
    With any variant or chain the result is ``(rows [1 + V, M, n], labels)``, ``labels`` = ``stress_labels`` of the same keywords, the
    names of rows 1.. ."""
    spec = dict(locals())                                        # the keywords above by name: the variants' lists and the steps' options
    from . import ops, pipeline
    batch = pipeline.as_batch(staged)
    variants = stress_variants(spec)
    kinds = {kind for _, kind, _ in variants}
    qualities, chains = [int(q) for q in qualities], [str(text) for text in chains]
    rows = [_score_batch(batch, members, None, after_fork=after_fork)]
    rows += [_score_batch(pipeline.apply_step(batch, "recompress", q, spec), members) for q in qualities]
    mean = keys_d = None
    for _, kind, arg in variants:                                # one perturbed batch alive at a time
        if mean is None and "contrast" in kinds and chain.STEPS[kind].family == "colour":
            mean = batch.mean_colour()                           # once per batch, in front of the colour rows
        if keys_d is None and kind in chain.NOISE_STEPS:
            keys_d = pipeline.noise_keys_device(batch, noise_keys)                                 # once per batch
        made = pipeline.apply_step(batch, kind, arg, spec, mean, keys_d)
        rows.append(_score_batch(made, members))
        rows += [_score_batch(pipeline.apply_step(made, "recompress", q, spec), members) for q in qualities]
    for text in chains:                                          # scored once, as written: the qualities do not multiply chain rows
        rows.append(_score_batch(pipeline.apply_chain(batch, pipeline.parse_chain(text), noise_keys=keys_d if keys_d is not None else noise_keys,
                                                      **{key: spec[key] for key in pipeline.STEP_OPTIONS}), members))
    if any(model is not None and member_dtype(model) == ops.PACKED for _, model in members):
        ops.h2_check("stress_batch")                             # no activation of a re-saved image left the packed storage's range
    if not variants and not chains:
        return torch.stack(rows)
    return torch.stack(rows), _row_labels(qualities, variants, chains)


# stress_labels' parameters: stress_batch's, in their order, less the batch, the members, after_fork and the three options of the
# re-save, the resize and the blur, which it has never taken
_LABEL_SIGNATURE = inspect.Signature([p for name, p in inspect.signature(stress_batch).parameters.items()
                                      if name not in ("staged", "members", "subsampling", "after_fork", "resize_filter", "blur_radius")])
stress_labels.__signature__ = _LABEL_SIGNATURE


def gather_stress_rows(kept: Sequence[torch.Tensor], n_q: int, n_members: int, n_images: int, rank: int = 0, world: int = 1,
                       dist=None) -> np.ndarray:
    """The extra exchange step of a stress run under the ``images`` plan: ``kept`` = this rank's ``stress_batch`` rows ``[Q, M, n_batch]`` in
    batch order (its image shard, ``shard_bounds(n_images, rank, world)``).  ONE ``all_gather_into_tensor`` of the ranks' rows, padded to the
    longest shard; returns ``[Q, M, n_images]`` fp32 (numpy) on every rank."""
    lo, hi = shard_bounds(n_images, rank, world)
    dev = kept[0].device if kept else torch.device("cuda" if torch.cuda.is_available() else "cpu")
    local = torch.cat(list(kept), dim=2).to(torch.float32) if kept else torch.zeros((n_q, n_members, 0), dtype=torch.float32, device=dev)
    assert tuple(local.shape) == (n_q, n_members, hi - lo), (tuple(local.shape), (n_q, n_members, hi - lo))
    if dist is None or world == 1:
        return local.cpu().numpy()
    width = max(shard_bounds(n_images, r, world)[1] - shard_bounds(n_images, r, world)[0] for r in range(world))
    mine = torch.zeros((n_q, n_members, max(width, 1)), dtype=torch.float32, device=dev)
    mine[:, :, :hi - lo] = local
    allp = torch.empty((world * mine.numel(),), dtype=torch.float32, device=dev)
    dist.all_gather_into_tensor(allp, mine.reshape(-1))
    allp = allp.view(world, n_q, n_members, max(width, 1))
    full = torch.zeros((n_q, n_members, n_images), dtype=torch.float32, device=dev)
    for r in range(world):
        rlo, rhi = shard_bounds(n_images, r, world)
        full[:, :, rlo:rhi] = allp[r, :, :, :rhi - rlo]
    return full.cpu().numpy()


def stress_table(names: Sequence[str], scores: np.ndarray, qualities: Sequence, thr: float = THR):
    """``scores`` ``[1 + Q, M, n]`` (``stress_batch`` rows over all images, in the order of ``names``) -> ``(table, summary)``; numpy only.
    ``table``: per sorted unique filename (duplicates averaged first, decision = mean ``> thr``: the rule of ``aggregate``) ``filename``,
    ``p`` / ``decision`` unperturbed, ``p_q`` / ``decision_q`` ``[F, Q]``, ``stable`` (every decision equals the unperturbed one) and
    ``flips_at`` (the highest listed quality whose decision differs, None when stable).  ``summary``: per quality the number and rate of
    files whose decision differs and the mean ``|p_q - p|``, plus the number of stable files.
    ``qualities`` may instead be the label list of ``stress_labels`` (``q<Q>``, ``r<P>``, ``r<P>_q<Q>``, ``b<TT>...``, ``m<K>...``,
    ``flip<A>...``, ``crop<PP>...``, ``rot<TTT>...``, ``gray...``, ``bgr...``, ``hue<DDD>...``, ``sat<PPP>...``, ``con<PPP>...``,
    ``bri<PP>...``, ``gam<PPP>...``, ``n<TTT>...``, ``nm<TTT>...``, ``spk<PP>...``, ``imp<TTT>...``, ``shp<PPP>...`` and chain labels such as
    ``r50+shp080+q75``, which count for ``stable`` and ``flips`` like any variant and never for ``flips_at``, even when they start with a
    ``q`` step).
    With ``q`` labels alone the result is the one above.  With rescaled, smoothed or warped variants ``p_q`` / ``decision_q`` are ``[F, V]`` over
    all variants, ``stable`` is taken over all of them, ``flips_at`` keeps its meaning (the ``q`` labels, i.e. the rows at 100 %, only),
    ``table`` gains ``labels`` and ``flips`` (per file the ``;``-joined labels whose decision differs), and ``summary`` gains ``variants``
    (the labels in order) and keys its per-variant counts by label; ``summary["qualities"]`` lists the qualities of the 100 % rows."""
    scores = np.asarray(scores)
    labels = [v if isinstance(v, str) else f"q{int(v)}" for v in qualities]
    plain = [int(v[1:]) if v[:1] == "q" and v[1:].isdigit() else None for v in labels]
    mixed = any(q is None for q in plain)
    assert scores.ndim == 3 and scores.shape[0] == 1 + len(labels) and scores.shape[2] == len(names), (scores.shape, len(labels), len(names))
    agg = [aggregate(names, s, thr) for s in scores]
    uniq = agg[0][0]
    p, dec = agg[0][1], agg[0][2]
    F = len(uniq)
    p_q = np.stack([a[1] for a in agg[1:]], axis=1) if labels else np.zeros((F, 0), np.float32)
    dec_q = np.stack([a[2] for a in agg[1:]], axis=1) if labels else np.zeros((F, 0), np.float32)
    differs = dec_q != dec[:, None]
    stable = ~differs.any(axis=1)
    flips_at = [max((q for q, d in zip(plain, row) if d and q is not None), default=None) for row in differs]
    table = {"filename": uniq, "p": p, "decision": dec, "p_q": p_q, "decision_q": dec_q, "stable": stable, "flips_at": flips_at}
    keys = labels if mixed else [str(q) for q in plain]
    summary = {"n_files": F, "threshold": float(thr), "qualities": [q for q in plain if q is not None], "n_stable": int(stable.sum()),
               "flips": {key: int(differs[:, k].sum()) for k, key in enumerate(keys)},
               "flip_rate": {key: (float(differs[:, k].mean()) if F else 0.0) for k, key in enumerate(keys)},
               "mean_abs_dp": {key: (float(np.abs(p_q[:, k].astype(np.float64) - p.astype(np.float64)).mean()) if F else 0.0)
                               for k, key in enumerate(keys)}}
    if mixed:
        table["labels"] = labels
        table["flips"] = [";".join(v for v, d in zip(labels, row) if d) for row in differs]
        summary["variants"] = labels
    return table, summary


def tile_batch(staged, members, tile: int = 200, stride: Optional[int] = None, max_tiles: int = 256, chunk: int = 128,
               after_fork=None):
    """One batch scored the plain way and as native-resolution tiles.  ``staged`` as for ``_score_batch``; it is decoded once.  Row 0 is
    ``_score_batch`` on the batch as it is - the same inputs, streams and calls, so bit for bit what a plain run returns.  Then every
    image at least ``tile`` pixels high and wide is cut into ``tile x tile`` crops (``pipeline.tile_plan``) and each crop is scored as an
    image of its own: at most ``chunk`` tiles at a time, in plan order, one gather launch per distinct ``input_key``
    (``DecodedBatch.tiles``: identity for a member whose resolution is ``tile``, the training pipeline's bicubic for the others), then
    ``MemberStreams.predict_all`` and ``ops.binary_score`` exactly as a plain pass makes them.
    Returns ``(plain [M, n], tiles [M + 1, T], agg [3, M + 1, n], plan)`` (device tensors, fp32): ``tiles[m]`` = member m's score of
    every tile, ``tiles[M]`` their ensemble mean (``ops.ensemble_mean``); ``agg`` = per row and image the mean / max / fraction ``> THR``
    of its tiles (``ops.tile_aggregate``), NaN for an image without tiles."""
    from . import ops, pipeline
    chunk = pipeline._int_arg("chunk", chunk, 1, 65535)
    batch = pipeline.as_batch(staged)
    plan = pipeline.tile_plan(batch.sizes_host, tile, stride, max_tiles)
    plain = _score_batch(batch, members, None, after_fork=after_fork)
    device = batch.rgb.device
    M, T = len(members), int(plan.tab.shape[0])
    tiles = torch.empty((M + 1, T), dtype=torch.float32, device=device)
    seg_d = torch.from_numpy(plan.seg).to(device)
    if T:
        tab_d = torch.from_numpy(plan.tab).to(device)
        for lo in range(0, T, chunk):
            hi = min(lo + chunk, T)
            inputs: Dict = {}
            for spec, model in members:
                k = input_key(spec, model)
                if k not in inputs:
                    inputs[k] = batch.tiles(tab_d, lo, hi, plan.tile, spec.input_hw, dtype=k[1])
            preds = _MEMBER_STREAMS.predict_all(members, inputs)
            for m, p in enumerate(preds):
                ops.binary_score(p, out=tiles[m, lo:hi])             # main.py:113-114
        ops.ensemble_mean(tiles[:M], out=tiles[M])
    if any(model is not None and member_dtype(model) == ops.PACKED for _, model in members):
        ops.h2_check("tile_batch")                                   # no activation of a tile left the packed storage's range
    return plain, tiles, ops.tile_aggregate(tiles, seg_d, THR), plan


def tile_table(names: Sequence[str], plain: np.ndarray, agg: np.ndarray, plan, thr: float = THR, tile_agg: str = "mean"):
    """The per-file report of a tile run; numpy only.  ``plain`` ``[M, n]`` and ``agg`` ``[3, M + 1, n]`` (``tile_batch``'s, over all images in
    the order of ``names``), ``plan`` = ``pipeline.tile_plan`` of the same images (its ``sizes``, ``grids`` and ``thinned`` are read).
    Returns ``(table, summary)``: ``table`` per sorted unique filename (duplicates averaged first, the rule of ``aggregate``) ``filename,
    width, height, tiles, grid`` (``"<ny>x<nx>"``, ``"0x0"`` when not tiled), ``p`` / ``decision`` of the plain run, ``p_tiles_mean,
    p_tiles_max, frac_tiles`` of the ensemble row (NaN when not tiled), ``decision_tiles`` (the ``tile_agg`` column ``> thr``; the plain
    decision when not tiled) and ``agrees``; ``summary``: the counts of tiled and untiled files, the files that disagree and the
    files whose grid ``max_tiles`` thinned."""
    if tile_agg not in ("mean", "max"):
        raise ValueError(f"tile_agg {tile_agg!r}: expected 'mean' or 'max'")
    plain, agg = np.asarray(plain), np.asarray(agg)
    n = len(names)
    assert plain.ndim == 2 and plain.shape[1] == n and agg.shape == (3, plain.shape[0] + 1, n) and len(plan.sizes) == n, \
        (plain.shape, agg.shape, n, len(plan.sizes))
    uniq, p, dec = aggregate(names, plain, thr)
    _, inv = np.unique(np.asarray(names), return_inverse=True)
    first = np.full(len(uniq), -1, np.int64)
    for i in range(n - 1, -1, -1):
        first[inv[i]] = i                                            # size and grid of a file: those of its first row
    cnts = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    cols = []
    for k in range(3):                                               # duplicates: the mean of their rows (NaN stays NaN)
        sums = np.zeros(len(uniq), np.float64)
        np.add.at(sums, inv, agg[k, -1].astype(np.float64))
        cols.append((sums / cnts).astype(np.float32))
    p_mean, p_max, frac = cols
    grids = [plan.grids[i] for i in first]
    tiled = np.array([g[0] * g[1] > 0 for g in grids], dtype=bool)
    pick = p_mean if tile_agg == "mean" else p_max
    dec_tiles = np.where(tiled, (np.nan_to_num(pick, nan=0.0) > thr).astype(np.float32), dec).astype(np.float32)
    agrees = dec_tiles == dec
    table = {"filename": uniq, "width": [plan.sizes[i][1] for i in first], "height": [plan.sizes[i][0] for i in first],
             "tiles": [g[0] * g[1] for g in grids], "grid": [f"{g[0]}x{g[1]}" for g in grids], "p": p, "decision": dec,
             "p_tiles_mean": p_mean, "p_tiles_max": p_max, "frac_tiles": frac, "decision_tiles": dec_tiles, "agrees": agrees}
    summary = {"n_files": len(uniq), "threshold": float(thr), "tile_agg": tile_agg, "n_tiled": int(tiled.sum()),
               "n_untiled": int((~tiled).sum()), "n_disagree": int((~agrees).sum()),
               "disagreements": [u for u, a in zip(uniq, agrees) if not a],
               "thinned": [u for u, i in zip(uniq, first) if plan.thinned[i]]}
    return table, summary


OCCLUSION_FILLS = ("mean", "gray")


def occlusion_batch(staged, members, grid: int = 8, window: int = 2, fill: str = "mean", chunk: int = 128, after_fork=None):
    """One batch scored the plain way and with every window of an occlusion grid hidden.  ``staged`` as for ``_score_batch``; it is decoded
    once.  Row 0 is ``_score_batch`` on the batch as it is - the same inputs, streams and calls, so bit for bit what a plain run returns.
    Then every image at least ``grid`` pixels high and wide is scored once per window of ``pipeline.occlusion_plan`` with the window's
    pixels replaced by ``fill`` - ``"mean"``: the image's own mean colour (``DecodedBatch.mean_colour``), ``"gray"``: (128, 128, 128) - at
    most ``chunk`` variants at a time, in plan order, one gather launch per distinct ``input_key`` (``DecodedBatch.occluded``: the member's
    ordinary input path on the occluded pixels), then ``MemberStreams.predict_all`` and ``ops.binary_score`` exactly as a plain pass makes
    them.  No gradients and no knowledge of a member's head: every member has a map, ViTs included.
    Returns ``(plain [M, n], variants [M + 1, V], cells [M + 1, n, G, G], stats [M + 1, n, 4], plan)`` (device tensors, fp32):
    ``variants[m]`` = member m's score of every variant, ``variants[M]`` their ensemble mean (``ops.ensemble_mean``); ``cells`` and ``stats``
    (``ops.occlusion_cells`` at ``THR``) are taken on delta = plain - variant per row, row M against the ensemble mean of ``plain``:
    positive where hiding the region lowers the synthetic score.  NaN for an image without variants."""
    from . import ops, pipeline
    chunk = pipeline._int_arg("chunk", chunk, 1, 65535)
    if fill not in OCCLUSION_FILLS:
        raise ValueError(f"fill {fill!r}: expected one of {', '.join(OCCLUSION_FILLS)}")
    batch = pipeline.as_batch(staged)
    plan = pipeline.occlusion_plan(batch.sizes_host, grid, window)
    plain = _score_batch(batch, members, None, after_fork=after_fork)
    device = batch.rgb.device
    M, n, V = len(members), len(batch), int(plan.tab.shape[0])
    variants = torch.empty((M + 1, V), dtype=torch.float32, device=device)
    if V:
        tab_d = torch.from_numpy(plan.tab).to(device)
        if fill == "mean":
            fill_d = batch.mean_colour()
        else:
            fill_d = torch.tensor([[128, 128, 128, 0]] * n, dtype=torch.uint8, device=device)
        for lo in range(0, V, chunk):
            hi = min(lo + chunk, V)
            inputs: Dict = {}
            for spec, model in members:
                k = input_key(spec, model)
                if k not in inputs:
                    inputs[k] = batch.occluded(tab_d, lo, hi, fill_d, spec.input_hw, spec.input_hw, dtype=k[1])
            preds = _MEMBER_STREAMS.predict_all(members, inputs)
            for m, p in enumerate(preds):
                ops.binary_score(p, out=variants[m, lo:hi])          # main.py:113-114
        ops.ensemble_mean(variants[:M], out=variants[M])
    if any(model is not None and member_dtype(model) == ops.PACKED for _, model in members):
        ops.h2_check("occlusion_batch")                              # no activation of a variant left the packed storage's range
    rows = torch.empty((M + 1, n), dtype=torch.float32, device=device)
    rows[:M] = plain
    ops.ensemble_mean(plain, out=rows[M])
    cells, stats = ops.occlusion_cells(variants, rows, plan.seg, plan.grid, plan.window, THR)
    return plain, variants, cells, stats, plan


def occlusion_table(names: Sequence[str], plain: np.ndarray, stats: np.ndarray, plan, thr: float = THR):
    """The per-file report of an occlusion run; numpy only.  ``plain`` ``[M, n]`` and ``stats`` ``[M + 1, n, 4]`` (``occlusion_batch``'s, over all
    images in the order of ``names``; the ensemble row is read), ``plan`` = ``pipeline.occlusion_plan`` of the same images (its ``sizes``,
    ``seg``, ``grid`` and ``window`` are read).  Returns ``(table, summary)``: ``table`` per sorted unique filename (duplicates averaged first,
    the rule of ``aggregate``; size, variant count and ``cell_max`` are those of a file's first row) ``filename, width, height, variants``
    (0 for a skipped file), ``p`` / ``decision`` of the plain run, ``delta_max, delta_min`` (the largest and smallest delta-p of the ensemble
    over the file's variants), ``cell_max`` (``"gy,gx"``: the first cell of the window with the largest delta; empty when skipped) and
    ``flips`` (variants whose decision differs from the plain one) - NaN for a skipped file; ``summary``: the counts, the skipped files
    and the files with ``flips > 0``."""
    plain, stats = np.asarray(plain), np.asarray(stats)
    n = len(names)
    assert plain.ndim == 2 and plain.shape[1] == n and stats.shape == (plain.shape[0] + 1, n, 4) and len(plan.sizes) == n, \
        (plain.shape, stats.shape, n, len(plan.sizes))
    uniq, p, dec = aggregate(names, plain, thr)
    _, inv = np.unique(np.asarray(names), return_inverse=True)
    first = np.full(len(uniq), -1, np.int64)
    for i in range(n - 1, -1, -1):
        first[inv[i]] = i
    cnts = np.bincount(inv, minlength=len(uniq)).astype(np.float64)
    cols = []
    for k in (0, 1, 3):                                              # duplicates: the mean of their rows (NaN stays NaN)
        sums = np.zeros(len(uniq), np.float64)
        np.add.at(sums, inv, stats[-1, :, k].astype(np.float64))
        cols.append((sums / cnts).astype(np.float32))
    d_max, d_min, flips = cols
    per_axis = plan.grid - plan.window + 1
    variants = [int(plan.seg[i + 1] - plan.seg[i]) for i in first]
    cell_max = []
    for i, v in zip(first, variants):
        at = stats[-1, i, 2]
        cell_max.append("" if v == 0 or np.isnan(at) else f"{int(at) // per_axis},{int(at) % per_axis}")
    table = {"filename": uniq, "width": [plan.sizes[i][1] for i in first], "height": [plan.sizes[i][0] for i in first],
             "variants": variants, "p": p, "decision": dec, "delta_max": d_max, "delta_min": d_min, "cell_max": cell_max, "flips": flips}
    skipped = [u for u, v in zip(uniq, variants) if v == 0]
    summary = {"n_files": len(uniq), "threshold": float(thr), "grid": plan.grid, "window": plan.window,
               "variants_per_image": per_axis * per_axis, "n_explained": len(uniq) - len(skipped), "n_skipped": len(skipped),
               "skipped": skipped, "flipped": [u for u, f in zip(uniq, flips) if f > 0]}
    return table, summary


class Explanation:
    """What ``explain_batch`` returns: ``scores`` ``[M, n]`` (device; exactly what ``_score_batch`` returns), per member ``maps[m]``
    ``[n, gh, gw]`` fp32 (un-normalised, ``ops.cam``) and ``peaks[m]`` ``[n]`` - None for a member without a map, with the reason in
    ``unsupported[name]`` - the composed full-size map ``map`` ``[n, maxH, maxW]`` (fp32 in [0, 1] or uint8; None when no member can
    produce one), and the decoded ``batch`` it belongs to (``batch.sizes_host[i]`` = the image's own height and width)."""

    def __init__(self, scores, names, maps, peaks, unsupported, full, batch):
        self.scores, self.names, self.maps, self.peaks, self.unsupported, self.map, self.batch = scores, names, maps, peaks, unsupported, full, batch


def cam_support(members) -> Dict[str, Optional[str]]:
    """``{member name: None | why it has no evidence map}`` for ``members`` = [(spec, model)]"""
    from . import cam
    return {spec.name: cam.unsupported_reason(model) for spec, model in members}


def explain_batch(staged, members, target="score", out: str = "u8", after_fork=None) -> Explanation:
    """``_score_batch`` plus Grad-CAM evidence: every map-capable member runs ``predict_with_cam`` (ONE pass through its body: the
    probabilities of ``predict``, bit for bit, and the low-resolution map), the others ``predict``; the members run on ``MemberStreams``
    as they do for scoring.  The maps are normalised, resampled to each image's own size and averaged over the members that have one
    in a single launch (``ops.cam_compose``; ``out`` = ``"u8"`` or ``"f32"``).  A fold ensemble contributes the mean of its folds' maps.
    Raises ``VipError`` when a map is not finite."""
    from . import ops, pipeline
    batch = pipeline.as_batch(staged)
    global _MEMBER_STREAMS
    if _MEMBER_STREAMS is None:
        _MEMBER_STREAMS = MemberStreams(default_streams())
    inputs = member_inputs(batch, members)
    why = cam_support(members)

    def call(model, x):
        if getattr(model, "cam_supported", False):
            return model.predict_with_cam(x, target)
        return (model.predict(x), None, None)

    res = _MEMBER_STREAMS.predict_all(members, inputs, after_fork=after_fork, call=call)
    rows = torch.empty((len(res), res[0][0].shape[0]), dtype=torch.float32, device=res[0][0].device)
    maps, peaks, parts, weights = [], [], [], []
    n_cam = sum(1 for r in res if r[1] is not None)
    for m, (p, cm, pk) in enumerate(res):
        ops.binary_score(p, out=rows[m])                         # main.py:113-114
        maps.append(cm)
        peaks.append(pk)
        if cm is not None:
            folds = list(zip(cm, pk)) if isinstance(cm, (list, tuple)) else [(cm, pk)]
            for c_, p_ in folds:
                parts.append((c_, p_))
                weights.append(1.0 / (n_cam * len(folds)))
    full = None
    if parts:
        # one transfer for every member's peaks (a synchronising check: a non-finite map is an error, not an output)
        ops.cam_check(torch.stack([p_ for _, p_ in parts]), "explain_batch: members "
                      + ", ".join(spec.name for (spec, _), pk in zip(members, peaks) if pk is not None) + " (row, image)")
        full = ops.cam_compose([c_ for c_, _ in parts], [p_ for _, p_ in parts], batch.sizes, batch.rgb.shape[1:3], weights, out=out)
    return Explanation(rows, [spec.name for spec, _ in members], maps, peaks, {k: v for k, v in why.items() if v is not None}, full, batch)
