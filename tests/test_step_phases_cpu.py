"""bridgeqa_amd.step_phases on CPU tensors: what pipeline.PhasedTrainStep and graphed.GraphedRunner share -- the geometry double
buffer, the autograd cut in front of the fusion with the text prologue's backward, the deferred weight-gradient bracket, the
replay signature and the per-phase GPU times -- held to what each promises, with stand-ins for the model and for HIP events."""
import pytest
import torch

from bridgeqa_amd import step_phases as sp


# ---- the geometry double buffer -------------------------------------------------------------------------------------------
class _Backbone(object):
    def precompute_geometry(self, point_clouds):
        xyz = point_clouds[..., :3]
        return {"centres": xyz * 2.0, "order": xyz.sum(-1).argsort(-1).to(torch.int32)}


def _clouds(seed):
    return torch.randn(2, 16, 4, generator=torch.Generator().manual_seed(seed))


def test_compute_clones_once_then_writes_in_place():
    geo, bb = sp.GeometryBuffers(), _Backbone()
    assert geo.next is None and geo.cur is None           # no tensor before the first call
    pc = _clouds(0)
    geo.compute(bb, pc)
    want = bb.precompute_geometry(pc)
    assert all(torch.equal(geo.next[k], want[k]) and geo.next[k].data_ptr() != want[k].data_ptr() for k in want)
    ptrs = {k: v.data_ptr() for k, v in geo.next.items()}
    pc2 = _clouds(1)
    geo.compute(bb, pc2)
    want2 = bb.precompute_geometry(pc2)
    assert all(torch.equal(geo.next[k], want2[k]) for k in want2)
    assert {k: v.data_ptr() for k, v in geo.next.items()} == ptrs


def test_rotate_keeps_cur_while_next_is_refilled():
    geo, bb = sp.GeometryBuffers(), _Backbone()
    first, second, third = (bb.precompute_geometry(_clouds(s)) for s in (0, 1, 2))
    geo.compute(bb, _clouds(0))
    cur = geo.rotate()
    assert cur is geo.cur and all(torch.equal(cur[k], first[k]) and cur[k].data_ptr() != geo.next[k].data_ptr() for k in first)
    ptrs = {k: v.data_ptr() for k, v in cur.items()}
    geo.compute(bb, _clouds(1))                           # the prefetch refills `next` ...
    assert all(torch.equal(geo.next[k], second[k]) for k in second)
    assert all(torch.equal(cur[k], first[k]) for k in first)   # ... and the running step's indices stay
    cur2 = geo.rotate()
    assert cur2 is cur and all(torch.equal(cur[k], second[k]) for k in second)
    geo.compute(bb, _clouds(2))
    assert all(torch.equal(geo.rotate()[k], third[k]) for k in third)
    assert {k: v.data_ptr() for k, v in geo.cur.items()} == ptrs


# ---- the cut in front of the fusion ---------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    """detector -> fuse -> loss in small: every parameter receives at most two gradient contributions, so the order in which
    they are added cannot change a bit (fp32 addition is commutative, not associative)"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.w_img, self.w_det, self.w_fuse = (torch.nn.Parameter(torch.randn(8, 8, generator=g) * 0.3) for _ in range(3))
        self.emb_q = torch.nn.Parameter(torch.randn(11, 8, generator=g))   # tied: the prologue AND the fusion read it
        self.emb_a = torch.nn.Parameter(torch.randn(11, 8, generator=g))   # its embeddings are not used by the fusion
        self.x_img, self.pts = torch.randn(2, 5, 8, generator=g), torch.randn(2, 6, 8, generator=g)
        self.ids = torch.tensor([[1, 4, 4, 9], [0, 2, 10, 1]])

    def encode_image(self):
        return torch.tanh(self.x_img @ self.w_img)

    def detect(self):
        feat = torch.relu(self.pts @ self.w_det)
        return {"object_feat": feat, "objectness": feat.sum(-1) * 0.1, "num_proposal": 6}

    def prepare_text(self):
        return {"q_embeds": self.emb_q[self.ids] * 1.5, "a_embeds": self.emb_a[self.ids], "targets": self.ids}

    def fuse(self, dd, img, obj, prep):
        h = (img.mean(1, keepdim=True) + obj + prep["q_embeds"].mean(1, keepdim=True)) @ self.w_fuse
        return (h @ self.emb_q.t()).logsumexp(-1).sum() / dd["num_proposal"]

    @staticmethod
    def det_loss(dd):
        return dd["objectness"].pow(2).sum()


def _grads(m):
    out = {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}
    m.zero_grad(set_to_none=True)
    return out


def test_backward_through_the_cut_is_bit_equal_and_skips_unused_prologue_leaves():
    m = _Toy()
    img, dd, prep = m.encode_image(), m.detect(), m.prepare_text()
    (m.det_loss(dd) + m.fuse(dd, img, dd["object_feat"], prep)).backward()
    whole = _grads(m)
    assert whole["emb_a"] is None and all(whole[k] is not None for k in ("w_img", "w_det", "w_fuse", "emb_q"))

    img, dd, prep = m.encode_image(), m.detect(), m.prepare_text()
    cut, img_leaf, obj_leaf, prep_cut, leaves = sp.cut_for_fusion(img, dd, prep)
    assert set(leaves) == {"q_embeds", "a_embeds"} and prep_cut is not prep and prep_cut["targets"] is prep["targets"]
    assert all(prep_cut[k] is leaves[k] and leaves[k].is_leaf and prep[k].grad_fn is not None for k in leaves)
    assert cut["num_proposal"] == 6 and not any(v.requires_grad for v in cut.values() if torch.is_tensor(v))
    m.fuse(cut, img_leaf, obj_leaf, prep_cut).backward()
    assert leaves["q_embeds"].grad is not None and leaves["a_embeds"].grad is None
    sp.text_prologue_backward(prep, leaves)                    # (the a_embeds leaf got no gradient: skipped, no error)
    torch.autograd.backward([m.det_loss(dd), dd["object_feat"]], [None, obj_leaf.grad])
    img.backward(img_leaf.grad)
    parts = _grads(m)
    assert parts["emb_a"] is None
    for k, g in whole.items():
        if g is not None:
            assert torch.equal(parts[k], g), k


def test_cut_without_a_prologue():
    m = _Toy()
    cut, img_leaf, obj_leaf, prep, leaves = sp.cut_for_fusion(m.encode_image(), m.detect())
    assert prep is None and leaves == {} and img_leaf.is_leaf and obj_leaf.is_leaf and img_leaf.requires_grad
    sp.text_prologue_backward(None, leaves)                    # nothing to continue from


# ---- the deferred weight-gradient bracket ---------------------------------------------------------------------------------
def test_deferred_wgrad_flushes_when_the_body_raises(monkeypatch):
    calls = []
    monkeypatch.setattr(sp.ops, "begin_deferred_wgrad", lambda: calls.append("begin"))
    monkeypatch.setattr(sp.ops, "flush_deferred_wgrad", lambda: calls.append("flush"))
    with sp.deferred_wgrad():
        calls.append("body")
    assert calls == ["begin", "body", "flush"]
    del calls[:]
    with pytest.raises(ZeroDivisionError):
        with sp.deferred_wgrad():
            1 / 0
    assert calls == ["begin", "flush"]


# ---- per-phase GPU times ----------------------------------------------------------------------------------------------------
class _Event(object):
    def __init__(self, t):
        self.t = t

    def elapsed_time(self, other):
        return other.t - self.t


def _steps(spans, step_ms, n, first=0):
    return [(_Event(step_ms * i + spans[0]), _Event(step_ms * i + spans[1])) for i in range(first, n)]


def test_phase_gpu_ms_aligns_ragged_lists_at_the_end():
    ev = {"image_fwd": _steps((1.0, 5.0), 40.0, 3, first=1), "det_fwd": _steps((2.0, 4.5), 40.0, 3, first=1),
          # the first recorded step computed its own geometry in front of its detector forward: an extra, EARLIER entry
          "geometry": [(_Event(40.25), _Event(40.75))] + _steps((6.0, 9.5), 40.0, 3, first=1)}
    out = sp.phase_gpu_ms(ev, "image_fwd")
    assert list(out) == list(ev)
    assert out == {"image_fwd": (0.0, 4.0), "det_fwd": (1.0, 3.5), "geometry": (5.0, 8.5)}
    assert sp.phase_gpu_ms(ev, "det_fwd")["geometry"] == (4.0, 7.5)


def test_phase_gpu_ms_equal_lengths_give_the_start_aligned_means():
    ev = {"det_fwd": _steps((0.3, 7.1), 37.7, 5), "image_fwd": _steps((0.9, 11.3), 37.7, 5),
          "finish": _steps((35.2, 37.4), 37.7, 5)}
    out = sp.phase_gpu_ms(ev, "det_fwd")
    steps = min(len(v) for v in ev.values())
    for name, evs in ev.items():     # (PhasedTrainStep.phase_gpu_ms before step_phases: entries paired from the start)
        a = [ev["det_fwd"][i][0].elapsed_time(evs[i][0]) for i in range(steps)]
        b = [ev["det_fwd"][i][0].elapsed_time(evs[i][1]) for i in range(steps)]
        assert out[name] == (sum(a) / steps, sum(b) / steps)


# ---- what invalidates a captured set --------------------------------------------------------------------------------------
def test_replay_signature_follows_momentum_and_mode():
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.BatchNorm1d(4), torch.nn.Sequential(torch.nn.BatchNorm2d(4)))
    mods = sp.batchnorm_modules(model)
    assert mods == [model[1], model[2][0]]
    prev = sp.ops.set_deterministic(False)
    try:
        sig = sp.replay_signature(mods)
        assert sp.replay_signature(mods) == sig
        model[2][0].momentum = 0.05
        assert sp.replay_signature(mods) != sig
        model[2][0].momentum = 0.1
        assert sp.replay_signature(mods) == sig
        sp.ops.set_deterministic(True)
        assert sp.replay_signature(mods) != sig
        sp.ops.set_deterministic(False)
        assert sp.replay_signature(mods) == sig
    finally:
        sp.ops.set_deterministic(prev)
