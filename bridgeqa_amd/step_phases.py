"""What the two ways to run a training step -- pipeline.PhasedTrainStep and graphed.GraphedRunner -- have to agree on, stated
once: what the phases they share do, the rules of capturing a phase as a HIP graph, what invalidates a captured set, and the
instrumentation of a replay.  Plain functions and one small class: each runner keeps its own phase list, streams, events and
schedule (the eager loop, the replayed loop and the phased step run the same kernels and agree bit for bit)."""
import contextlib
import gc
import time

import torch

from . import fusion_ops as ops


# ---- the phases' shared parts -------------------------------------------------------------------------------------------
def _into(dst, src):
    """src's tensors into the persistent set dst (cloned the first time, copied in place afterwards)"""
    if dst is None:
        return {k: v.clone() for k, v in src.items()}
    for k, v in src.items():
        dst[k].copy_(v)
    return dst


class GeometryBuffers(object):
    """The sampling / grouping indices of a point-cloud batch (Pointnet2Backbone.precompute_geometry: FPS picks, centres,
    ball-query groups of the four SA levels, three-NN of the two FP levels -- coordinates only, no parameters) in two
    persistent sets: `next`, which a prefetch fills under the fusion of the step before, and `cur`, which the detector
    forward reads.  No tensor exists before the first call, which the runner makes inside a phase: a captured graph's pool
    and a tensor's stream affinity depend on where it is born."""

    def __init__(self):
        self.next, self.cur = None, None

    def compute(self, backbone, point_clouds):
        from .pointnet2_utils import background_geometry
        with background_geometry():   # (the gentle ball-query grid: this phase runs beside the fusion chain)
            geo = backbone.precompute_geometry(point_clouds)
        self.next = _into(self.next, geo)

    def rotate(self):
        """next -> cur, in front of the detector forward: this step's backward keeps reading `cur` while the prefetch under
        its fusion refills `next`"""
        self.cur = _into(self.cur, self.next)
        return self.cur


PREP_LEAVES = ("q_embeds", "a_embeds")   # what BLIP_VQA3D.prepare_text differentiates: the question / answer embeddings


def cut_for_fusion(image_embeds, det_dict, prep=None):
    """Autograd is cut at the tensors that cross streams: the fusion differentiates w.r.t. detached leaves, and the branch
    backwards are seeded with the leaves' .grad afterwards -- the same gradients as one backward over the whole graph (chain
    rule).  prep: prepare_text's dict where the token-only prologue ran ahead of the fusion, or None.  Returns (the detector's
    dict with every tensor detached, image leaf, object_feat leaf, prep with its embeddings replaced by leaves, {key: leaf})."""
    img_leaf = image_embeds.detach().requires_grad_(True)
    obj_leaf = det_dict["object_feat"].detach().requires_grad_(True)
    dd = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in det_dict.items()}
    prep_leaves = {}
    if prep is not None:
        prep = dict(prep)
        prep_leaves = {k: prep[k].detach().requires_grad_(True) for k in PREP_LEAVES if k in prep}
        prep.update(prep_leaves)
    return dd, img_leaf, obj_leaf, prep, prep_leaves


def text_prologue_backward(prep, prep_leaves):
    """the prologue's backward (LayerNorm + embedding tables; the decoder's table is tied to the LM head: this adds to the
    gradient the fusion's backward left there), continued from the gradients the fusion gave the leaves of cut_for_fusion"""
    roots = [(prep[k], leaf.grad) for k, leaf in prep_leaves.items() if leaf.grad is not None]
    if roots:
        torch.autograd.backward([t for t, _ in roots], [g for _, g in roots])


@contextlib.contextmanager
def deferred_wgrad():
    """weight / bias gradients of every linear are parked during the backward inside and produced by ONE grouped GEMM launch
    per tile class + one grouped column-sum launch at its end (fusion_wgrad), also when the backward raises"""
    ops.begin_deferred_wgrad()
    try:
        yield
    finally:
        ops.flush_deferred_wgrad()


def t_refresh(dev, max_wgs=0):
    """the K-contiguous copies of the text side's weights that this step's small input-gradient GEMMs read
    (fusion_state.transposed_shadow): ONE launch re-transposes all of them from the operands the last optimizer step left.
    (A capture cannot build the device table: with the registry dirty the launch is left out of the graph.)"""
    if not (torch.cuda.is_current_stream_capturing() and ops._T_STATE["dirty"]):
        ops.refresh_transposed(dev, max_wgs=max_wgs)


def prepare_t_refresh(dev):
    """before capturing t_refresh: build the device table of what the warm-up registered (not possible inside a capture).
    The captured launch reads this generation's tables: the caller keeps the returned generation alive beside its graphs."""
    ops.refresh_transposed(dev)
    return ops.transposed_generation()


# ---- capture ----------------------------------------------------------------------------------------------------------------
def collect_dead_autograd():
    """An earlier eager forward can survive as a reference CYCLE (fusion_ops.HoistedKV <-> its autograd node): its
    AccumulateGrad nodes -- born on the caller's stream -- would be reused by the passes that follow, and hipStreamEndCapture
    faults on them.  Called before the eager warm-up on the phase streams, and again by capture_phases."""
    gc.collect()


def capture_phases(order, body, streams, pools, what, single_stream=True, before_phase=None):
    """One HIP graph per phase: for every (name, stream, pool) of `order`, body(name) runs under capture on streams[stream]
    into pools[pool], with a synchronize after each; returns {name: graph}.  before_phase(name) runs outside the capture, in
    front of it.  `what` opens the error message.  Pools: graphs of one stream share one when they always replay in capture
    order; streams that run concurrently, and graphs that replay out of capture order, get pools of their own.
    single_stream: no fusion_ops.fork inside a phase (the decoder's hoisted K/V projection stays on the chain's stream).
    This runtime enqueues a graph with an internal fork node by node: the fusion graph's launch held the host for 35-38 ms
    and the phase ran 14.2 ms; without the fork 2.2 ms of host time and 12.7-13.4 ms (round 4, A/B/A on one box: 39.5 /
    40.7 / 38.6 ms per step; behind the reference's loop 8.8 ms of host time and 12.2 ms on the GPU instead of ~4.5)."""
    collect_dead_autograd()
    prev_overlap = ops.set_overlap(not single_stream)
    graphs = {}
    try:
        for name, which, pool in order:
            if before_phase is not None:
                before_phase(name)
            g = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(g, pool=pools[pool], stream=streams[which]):
                    body(name)
            except Exception as e:
                raise RuntimeError("%s: phase '%s' could not be captured: %s" % (what, name, e)) from e
            graphs[name] = g
            torch.cuda.synchronize(streams[which].device)
    finally:
        ops.set_overlap(prev_overlap)
    return graphs


def batchnorm_modules(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def replay_signature(bn_modules):
    """What a captured set is only valid for, compared by value before every replay.  BatchNorm momentum is a HOST scalar
    baked into the captured launches (F.batch_norm and the bq BN kernels take it by value): the reference's
    BNMomentumScheduler (lib/pointnet2/pytorch_utils.py, stepped once per epoch) would have no effect under replay.  The
    deterministic mode selects other kernels.  A change of either captures again."""
    return tuple(m.momentum for m in bn_modules) + (("deterministic", ops.is_deterministic()),)


# ---- replay instrumentation ---------------------------------------------------------------------------------------------
def timed_launch(name, launch, dev, host_times, phase_events):
    """launch() on the current stream of `dev`; host_times / phase_events: None, or the dicts that collect the host time of
    the call (ms) and the (start, end) events that bracket it on its stream, per name"""
    if host_times is None and phase_events is None:
        return launch()
    if phase_events is not None:
        s_ = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s_)
    t0 = time.perf_counter()
    launch()
    if host_times is not None:
        host_times.setdefault(name, []).append((time.perf_counter() - t0) * 1e3)
    if phase_events is not None:
        e1.record(s_)
        phase_events.setdefault(name, []).append((e0, e1))


def phase_gpu_ms(phase_events, ref):
    """after a synchronize: {phase: (mean start, mean end)} in ms relative to the start of phase `ref`, over the steps every
    phase was recorded in (aligned at the END: a step that ran a phase twice has an extra, earlier entry)"""
    steps = min(len(v) for v in phase_events.values())
    t0 = [e[0] for e in phase_events[ref][-steps:]]
    out = {}
    for name, evs in phase_events.items():
        evs = evs[-steps:]
        out[name] = (sum(t0[i].elapsed_time(evs[i][0]) for i in range(steps)) / steps,
                     sum(t0[i].elapsed_time(evs[i][1]) for i in range(steps)) / steps)
    return out
