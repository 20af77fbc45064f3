"""The detection-loss kernels of csrc/detloss.hip (det_loss_kernel, det_loss_finish_kernel, det_loss_bwd_kernel) held to the exact
decisions and the per-element fp64 bound of tests/detloss_ref.py, through loss_helper.get_detection_loss with distinct upstream
weights per term, on every case of detloss_ref.CASES in the three layouts the kernel reads (`packed`: slices of one head output
inside the autograd graph; `slices`: independent leaves with the slices' strides; `contiguous`).  Labels, mask and assignment
must EQUAL the reference; the eight terms, both ratios and every gradient element must lie within the bound (`not (err <= tol)`
fails, so NaN fails; a tolerance of 0 demands equality), and the channels of the packed gradient that no term reads must be
exactly 0.  The poisoned runs hand every buffer the two wrappers allocate to the kernels NaN-filled (integers: a negative
pattern) and demand bitwise the results of the plain run: every element autograd reads was written by a kernel.

Which mechanism each case reaches is said in the docstring of tests/detloss_ref.py.  The largest
|err| / bound per case and output is printed at the end of the module (pytest -s); on an MI355X, the largest over all cases:
    terms 0.032  ratios 0.924  g_vote_xyz 0.194  g_objectness_scores 0.555  g_center 0.534  g_heading_scores 0.593
    g_heading_residuals_normalized 0.458  g_size_scores 0.564  g_size_residuals_normalized 0.896  g_sem_cls_scores 0.561
-- the same figures as detloss_ref.emulate() gives on the CPU; every label, mask and assignment equalled the reference, the
poisoned runs repeated the plain ones bit for bit, and no kernel needed a change.
"""
import pytest
import torch

import detloss_ref as R

pytestmark = pytest.mark.gpu

LAYOUTS = ("packed", "slices", "contiguous")
_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, w in _WORST.items():
        print("\n%s: " % name + "  ".join("%s %.3g" % kv for kv in w.items()), end="")
    print()


def _run(dev, name, layout, monkeypatch=None):
    """-> compare()'s form, plus `seen`: det_loss_bwd's own outputs (with monkeypatch) and `center_leaf` (packed)"""
    from bridgeqa_amd import _ext
    from bridgeqa_amd import loss_helper as lh
    d, net, cfg = R.case(name)
    NH, NS = cfg.num_heading_bin, cfg.num_size_cluster
    d = {k: v.to(dev) for k, v in d.items()}
    vote = d["vote_xyz"].clone().requires_grad_(True)
    base = net.to(dev).requires_grad_(True)
    dd = R.decode(base, dict(d, vote_xyz=vote), NH, NS)
    leaves = {}
    if layout != "packed":
        for k in R.SCORES + ("center",):
            v = dd[k].detach()
            leaves[k] = dd[k] = (v.contiguous() if layout == "contiguous" else v).requires_grad_(True)
    else:
        dd["center"].retain_grad()
    seen = {}
    if monkeypatch is not None:
        real_bwd = _ext.det_loss_bwd

        def spy(grads, upstream, packing=None):
            outs = real_bwd(grads, upstream, packing=packing)
            seen.update(outs)
            return outs
        monkeypatch.setattr(_ext, "det_loss_bwd", spy)
    mode = lh._fused_ok(dd)
    # (B = K = 1: the strides of extent-1 dimensions say nothing, det_loss_packing declines and the slices are read one by one)
    assert (mode is not None) and (bool(mode) == (layout == "packed") or base.shape[0] * base.shape[1] == 1), (layout, mode)
    _, dd = lh.get_detection_loss(dd, cfg)
    terms = torch.stack([dd[k] for k in R.TERMS])
    (terms * torch.tensor(R.TW, device=dev)).sum().backward()
    out = dict(terms=terms.detach(), ratios=torch.stack([dd["pos_ratio"], dd["neg_ratio"]]))
    out.update({k: dd[k] for k in R.LABELS})
    if layout == "packed":
        sl = R.decode(base.grad, {"aggregated_vote_xyz": torch.zeros_like(d["aggregated_vote_xyz"])}, NH, NS)
        grads = {k: sl[k] for k in R.SCORES}
        grads["center"] = sl["center"]                 # (the centre's gradient reaches the head output through its offset channels)
        out["center_leaf"] = dd["center"].grad
    else:
        grads = {k: v.grad for k, v in leaves.items()}
    grads["vote_xyz"] = vote.grad
    out["grads"] = grads
    out["seen"] = seen
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", R.CASES)
def test_detection_loss_within_the_fp64_bound(dev, name, layout, monkeypatch):
    ref = R.reference_of(name)
    out = _run(dev, name, layout, monkeypatch)
    worst, fails = R.compare(out, ref)
    if layout == "packed":
        # the kernel wrote exact zeros where no term reads, so the head output's gradient there is the centre's, bit for bit
        unc = out["seen"]["packed"][:, :, 2:5] if "packed" in out["seen"] else torch.zeros(1)
        if name != "one" and "packed" not in out["seen"]:
            fails.append("the packed gradient buffer was not produced")
        if not bool((unc == 0).all()):
            fails.append("packed gradient: %d nonzero elements in the channels no term reads" % int((unc != 0).sum()))
        if not torch.equal(out["grads"]["center"], out["center_leaf"]):
            fails.append("the head output's gradient at the centre offsets differs from the centre's gradient")
    w = _WORST.setdefault(name, {})
    for k, v in worst.items():
        w[k] = max(w.get(k, 0.0), v)
    print("\n%s %s: " % (name, layout) + "  ".join("%s %.3g" % kv for kv in worst.items()))
    assert not fails, "%s %s:\n%s" % (name, layout, "\n".join(fails))


def _flat(out):
    ts = [out["terms"], out["ratios"]] + [out[k] for k in R.LABELS] + [out["grads"][k] for k in sorted(out["grads"])]
    return [t.detach().cpu().contiguous() for t in ts]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ("limits", "two_trips_A"))
def test_every_element_read_was_written_by_a_kernel(dev, name, layout, monkeypatch):
    from bridgeqa_amd import _ext
    plain = _flat(_run(dev, name, layout))
    real = {k: getattr(torch, k) for k in ("empty", "empty_like", "empty_strided")}

    hits = []

    def poisoned(fn):
        def make(*a, **kw):
            t = fn(*a, **kw)
            if not t.is_cuda:
                return t
            hits.append(t.numel())
            return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(-0x55555555)
        return make
    for k, fn in real.items():
        monkeypatch.setattr(_ext.torch, k, poisoned(fn))
    try:
        out = _run(dev, name, layout)
    finally:
        monkeypatch.undo()
    torch.cuda.synchronize()
    got = _flat(out)
    assert len(got) == len(plain) and len(hits) >= 10, "the wrappers' buffers were not poisoned"
    for i, (a, b) in enumerate(zip(got, plain)):
        assert bool(torch.isfinite(a.double()).all()), "output %d holds a NaN of the poisoned buffers" % i
        assert a.dtype == b.dtype and torch.equal(a, b), "output %d differs from the plain run" % i
