"""Reference, bound, inputs and a fp32 emulation of the detection-loss kernels of csrc/detloss.hip (det_loss_kernel,
det_loss_finish_kernel, det_loss_bwd_kernel behind _ext.det_loss_fwd / det_loss_bwd and loss_helper._DetLossFn), for
tests/test_detloss_bound_cpu.py and tests/test_detloss_bound_gpu.py.  Nothing here needs a GPU or the extension.

REFERENCE.  fp64 from the fp32 tensors the kernel reads, the formulas of the reference's loss_helper / nn_distance:
    vote        T[j] = vote_label[seed_inds][j] + seed_xyz, d[j, v] = sum_c |vote[v] - T[j]|, best = min over (j, v),
                vote_loss = sum(best m) / (sum m + 1e-6), m = vote_label_mask[seed_inds]
    objectness  d1 = min_g |agg - gt_g|^2 (i1 = its index = object_assignment), eu = sqrt(d1 + 1e-6), label = eu < 0.3,
                mask = label or eu > 0.6, loss = sum(w[label] CE(scores, label) mask) / (sum mask + 1e-6), w = fp32 (0.2, 0.8)
    centre      dc = min_g |c - gt_g|^2 (ic), d2[g] = min_k |c_k - gt_g|^2 (k2), npos = sum label,
                loss = sum(dc label) / (npos + 1e-6) + sum(d2 bm) / (sum bm + 1e-6)
    heading / size / sem   labels gathered through i1; CE of the scores; Huber (delta 1) of residual[y] - label / (pi / NH), and the
                mean over 3 of Huber of size_residual[y] - label / mean_size[y]; each sum(. label) / (npos + 1e-6)
    ratios      pos = npos / (B K), neg = sum mask / (B K) - pos
Gradients in closed form (no autograd, so every pick is explicit): the vote gradient is m sign(vote[bv] - T[bj]) / den at the
picked vote only; the centre gradient is 2 (c - gt[ic]) label / npos plus 2 bm_g (c - gt_g) / den_bm for every g with k2[g] = k;
CE gives (softmax - onehot), Huber gives clamp(e, -1, 1) at the labelled bin / cluster only (/ 3 for the size residual).
Every output belongs to exactly one term: grads[name] is d term[NAMES.index(name)] / d name.

DECISIONS.  u = 2^-24.  A squared distance (ax ax + ay ay) + az az of rounded differences errs by 5 u d: u per difference, hence
2 u per square, u per product, and the first term passes 2 adds (-ffp-contract=off: every product and add rounds).  The L1 vote
distance errs by u sum_c |T_c| (the rounding of vote_label + seed_xyz, 0 where that sum is an fp32 number) + 3 u d.  A first-min
pick (i1, ic, k2, the vote pick) is CONTESTED when another candidate at a DIFFERENT fp64 value lies within the two errors of the
minimum (for the squared distances: a relative gap below 10 u; the issue says "about 8 u", the count above gives 2 x 5 u).
Candidates at the same value are exact ties -- identical rows, or exact dyadic arithmetic --: the first index wins, here as in
the kernel.  eu carries 5 u (d1) + u (the add), halved by the root, + u (sqrtf is correctly rounded) = 4 u; with the fp32
rounding of 0.3 / 0.6 / 1e-6 a threshold is contested within 8 u relative of eu.  sign(e) of the vote gradient is contested where
|e| <= u |T_c| and T_c is not an fp32 number (the kernel takes the sign of vote - fl(T), and that subtraction has the exact
sign).  Conditions, not tolerances: reference() asserts that NO pick and NO threshold is contested; contested signs may be at
most SIGN_CAP = 1e-3 of a case's g_vote elements and are compared against the interval [-m / den, +m / den].

BOUND.  Sums: every thread adds its n_t = ceil(count / 16384) items in order, the wave folds 64 lanes in a 6-step butterfly, 4
waves are added in order onto 0 and 64 block partials in order onto 0: a chain of at most D = n_t + 6 + 3 + 63 inexact adds, so
    tol_sum = D u sum|terms| + sum e_term,      tol_term = tol_sum / den + 3 u |term|
(den = count + 1e-6 with an integer count: the add, the reciprocal and the product round once each; the constant's own rounding
is below u in either regime).  The centre term adds two of these and rounds once more; pos_ratio is one division, neg_ratio two
and a subtraction.  Per element e_term:
    vote        u sum|T_c| + 3 u best                                (min is 1-Lipschitz)
    distances   5 u d
    CE, n > 1   t_i = x_i - max (u |t_i|), expf and logf 2 ulp = 4 u each -- TWICE the 1 ulp OCML documents for them --:
                rel_se = u (sum_i q_i |t_i| + 4 + n - 1)  (q = softmax: the rounding of t_i enters exp as u |t_i| relative and is
                weighted by q_i, so far-off logits do not inflate it),  e_l = u |t_y| + rel_se + 4 u |lse| + u |l|,
                e_q_i = q_i (u |t_i| + 4 u + rel_se + 2 u)  (1 / se and the product), gradient: e_q_i + u |q_i - onehot|
                n = 1: x - max = 0, expf(0) = 1, logf(1) = 0 and 1 / 1 are exact: loss and gradient are exactly 0, tolerance 0
                underflow: a softmax value below 2^-126 is a subnormal or flushed to 0, and no relative bound holds there: expf,
                the product with 1 / se, the normalisation and the backward's product may each lose up to 2^-126 absolute
                (3 + 1 times 2^-126 on every CE gradient whose tolerance is not 0; `limits` has logits 90 below their maximum)
    objectness  the weight is one more product: u |w l|
    Huber       heading: pi / NH is formed in fp32 (pi rounded, one division) and divides the label: 3 u |label / bin|, then the
                subtraction u |e|; size: one division and the subtraction, u |label / mean| + u |e|.  Huber and the clamp are
                1-Lipschitz, Huber's own arithmetic adds 2 u h; the size term adds three (2 u), divides by 3 (u); its gradient
                multiplies by fl(1 / 3): 2 u
    gradients   (e_unnormalised / den + 3 u |g|), the centre gradient u per own difference, 2 u per share (difference, product),
                and one add per GT box that picks the proposal; det_loss_bwd_kernel multiplies once more: u |g up|.
The comparison is ln_ref.excess: `not (err <= tol)` fails, so NaN fails, and a tolerance of 0 demands equality.

Against the issue: (1) the contested gap is 10 u, not 8 u (above).  (2) CE over ONE logit has tolerance 0 instead of the n > 1
formula, which is what makes case `one` exact as the issue requires.  (3) the heading quotient carries 3 u for the fp32 pi / NH the
launcher forms; the issue's list does not name it.  (3a) the fp32 torch composition on the CPU is held to the same bound except
at the two Huber gradients, where autograd_slack() adds the cancellation of torch's own backward (2 u of the UPSTREAM gradient:
16 u and more of a small e); the kernel and its emulation get no such term.  (4) the underflow term of the CE gradients (above): the issue's relative
bounds cannot hold for results below the smallest normal number.  Nothing else differs.

CASES (the smallest shapes that reach each mechanism; 16384 = the grid's threads).
    two_trips_A   3 x 5500 seeds: the second trip of pass A and of the g_vote scaling, the batch index on the second trip
    two_trips_B   3 x 5500 proposals, VF = 3: the second trip of pass B and of the finish loop; pass C scans 5500 proposals
    two_trips_C   2 x 8200 GT rows, the real boxes last: the second trip of pass C, a long GT scan per proposal
    one           B = S = K = G = N = NH = NS = NC = 1: CE of one logit is exactly 0 with zero gradient
    limits        NH = NS = NC = 32, rows of logits spread beyond |x - max| = 60, int64 seed_inds, center_label (B, G, 6)
    bench_like    B = 4, S = 1024, K = 256, G = 128, VF = 2, NH = 12, NS = NC = 18
    no_positive, all_grey, no_vote_mask, no_box   one denominator each is 0 + 1e-6 (no_positive: npos; all_grey: npos and sum mask)
    ties          every value a multiple of 1/8 below 64, residual labels and mean sizes powers of two (heading residual labels 0,
                  as pi / NH is no dyadic): two real boxes at one centre with different labels, padded rows at the origin with a
                  proposal next to them, two identical proposals nearest to a box, three identical votes, three equal GT votes
                  (a point inside one object carries its vote three times), a vote on its target, two votes equally far on
                  either side, Huber errors at exactly 0, +-1, +-2; all fp32 arithmetic up to the reductions is exact
"""
import functools
import math
import types

import numpy as np
import torch

from ln_ref import excess  # noqa: F401  (the comparison of the test modules)

U = 2.0 ** -24
TINY = 2.0 ** -126     # the smallest normal fp32 number
DL_ALL = 16384
SIGN_CAP = 1e-3
NEAR, FAR = 0.3, 0.6
W_OBJ = (float(np.float32(0.2)), float(np.float32(0.8)))
TERMS = ("vote_loss", "objectness_loss", "center_loss", "heading_cls_loss", "heading_reg_loss", "size_cls_loss", "size_reg_loss",
         "sem_cls_loss")
NAMES = ("vote_xyz", "objectness_scores", "center", "heading_scores", "heading_residuals_normalized", "size_scores",
         "size_residuals_normalized", "sem_cls_scores")           # NAMES[t] is the output term t differentiates
SCORES = tuple(n for n in NAMES if n not in ("vote_xyz", "center"))
TW = tuple(float(np.float32(v)) for v in (1.0, 0.5, 1.3, 0.1, 0.7, 0.2, 1.1, 0.3))   # distinct upstream gradients per term, as fp32 holds them
LABELS = ("objectness_label", "objectness_mask", "object_assignment")


def _cdiv(a, b):
    return -(-a // b)


def depth(count):
    """the longest chain of dependent adds a term of a `count`-item sum passes through"""
    return _cdiv(count, DL_ALL) + 6 + 3 + 63


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _random_case(B, S, K, G, N, NH, NS, NC, VF, seed, n_real=8, room=(8.0, 8.0, 3.0), i64=False, cl_w=3, logit_rows=0,
                 real_last=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    rn = lambda *s: torch.randn(*s, generator=g)
    room = torch.tensor(room)
    n_real = min(n_real, G)
    gt = torch.full((B, G, cl_w), -100.0)
    first = G - n_real if real_last else 0                          # real boxes in the rows first .. first + n_real - 1
    gt[:, first:first + n_real, :3] = r(B, n_real, 3) * room
    if cl_w > 3:
        gt[:, :, 3:] = 7.0 + r(B, G, cl_w - 3)                      # box sizes: what a wrong row stride would read as centres
    bm = torch.zeros(B, G)
    bm[:, first:first + n_real] = 1
    seed_xyz = r(B, S, 3) * room
    # proposals at 0.1 / 0.2 / 0.45 / 1.5 of a real centre: near, near, grey zone, far
    pick = G - 1 - torch.arange(K) % n_real if real_last else torch.arange(K) % n_real
    dirs = torch.nn.functional.normalize(rn(B, K, 3), dim=-1)
    rad = torch.tensor([0.1, 0.2, 0.45, 1.5])[(torch.arange(K) // min(n_real, max(K // 4, 1))) % 4]
    agg = gt[:, pick, :3] + dirs * rad[None, :, None]
    C = 2 + 3 + 2 * NH + 4 * NS + NC
    si = torch.randint(0, N, (B, S), generator=g)
    d = dict(seed_xyz=seed_xyz, vote_xyz=seed_xyz.repeat_interleave(VF, 1) + 0.3 * rn(B, S * VF, 3),
             seed_inds=si if i64 else si.int(), vote_label=rn(B, N, 9), vote_label_mask=(r(B, N) > 0.5).long(),
             center_label=gt, box_label_mask=bm, aggregated_vote_xyz=agg,
             heading_class_label=torch.randint(0, NH, (B, G), generator=g), heading_residual_label=0.3 * rn(B, G),
             size_class_label=torch.randint(0, NS, (B, G), generator=g), size_residual_label=0.5 * rn(B, G, 3),
             sem_cls_label=torch.randint(0, NC, (B, G), generator=g))
    net = 2.0 * rn(B, K, C)                                          # Huber's linear branch and both CE regimes are hit
    net[:, :, 2:5] *= 0.15                                           # centres stay near their proposal: ic and k2 are real contests
    if logit_rows:
        net[:, ::logit_rows] *= 8.0                                  # rows whose logits spread to |x - max| ~ 60 and beyond
        net[:, ::logit_rows, 2:5] /= 8.0
    mean_size = 0.5 + np.random.RandomState(seed).rand(NS, 3)
    return d, net, dict(NH=NH, NS=NS, NC=NC, mean_size_arr=mean_size)


def _ties_case():
    """every value a small dyadic; see the issue's table and test_the_ties_case_holds_its_ties"""
    B, S, VF, N, K, G, NH, NS, NC = 2, 6, 3, 6, 12, 8, 2, 3, 4
    g = torch.Generator().manual_seed(7)
    dy = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).float() / 8.0
    gt = torch.zeros(B, G, 3)                                       # padded rows 5 .. 7 sit at the origin, as ScanNet's do
    real = torch.tensor([[2.0, 2.0, 1.0], [2.0, 2.0, 1.0], [5.0, 1.0, 1.0], [1.0, 5.0, 2.0], [6.0, 6.0, 1.0]])   # 0 and 1: one centre
    gt[:, :5] = real
    gt[1, :5] += 0.125
    bm = torch.zeros(B, G)
    bm[:, :5] = 1
    agg = torch.cat([dy(0, 64, B, K, 2), dy(0, 24, B, K, 1)], -1)
    for b in range(B):
        o = gt[b]
        agg[b, 0] = o[0] + torch.tensor([0.125, 0.0, 0.0])          # near boxes 0 = 1: the first wins
        agg[b, 1] = torch.tensor([0.125, 0.0, 0.0])                 # near the padded rows at the origin: row 5
        agg[b, 2] = o[2] + torch.tensor([0.375, 0.25, 0.0])         # grey zone
        agg[b, 3] = o[3] + torch.tensor([1.0, 0.0, 0.0])            # far
        agg[b, 4] = agg[b, 5] = o[4] + torch.tensor([0.125, 0.125, 0.0])   # two identical proposals
        agg[b, 6] = o[2] + torch.tensor([0.0, 0.0, 0.25])           # near box 2
    C = 2 + 3 + 2 * NH + 4 * NS + NC
    net = dy(-16, 17, B, K, C)
    net[:, :, 2:5] = dy(-1, 2, B, K, 3)
    net[:, 4, :] = net[:, 5, :]                                     # ... with identical head outputs: identical centres
    net[:, 4:6, 2:5] = torch.tensor([0.0, 0.0, 0.125])
    net[:, 6, 2:5] = 0.0                                            # its centre is the nearest to box 2, alone
    hcl = torch.randint(0, NH, (B, G), generator=g)
    scl = torch.randint(0, NS, (B, G), generator=g)
    sem = torch.randint(0, NC, (B, G), generator=g)
    for lab in (hcl, scl, sem):                                     # boxes 0 and 1 share a centre and differ in every label
        lab[:, 1] = (lab[:, 0] + 1) % (2 if lab is hcl else 3)
    hrl = torch.zeros(B, G)                                         # label / (pi / NH) is exactly 0: e = the residual itself
    srl = torch.tensor([0.5, 1.0, 2.0]).repeat(B, G, 1)
    mean_size = np.array([[0.5, 1.0, 2.0], [1.0, 2.0, 0.5], [2.0, 0.5, 1.0]])
    # Huber errors at exactly 0, +-1, +-2 on the positive proposals 0, 1, 4 (= 5), 6: write the residual of EVERY bin / cluster
    o_hr, o_sr = 5 + NH, 5 + 2 * NH + NS
    want = {0: (0.0, (1.0, -1.0, 2.0)), 1: (1.0, (-2.0, 0.0, 1.0)), 4: (-1.0, (2.0, -2.0, 0.0)), 5: (-1.0, (2.0, -2.0, 0.0)),
            6: (2.0, (0.0, 1.0, -1.0)), 2: (-2.0, (1.0, 1.0, 1.0))}
    msz = torch.from_numpy(mean_size).float()
    for k, (eh, es) in want.items():
        net[:, k, o_hr:o_hr + NH] = eh
        for y in range(NS):
            net[:, k, o_sr + 3 * y:o_sr + 3 * y + 3] = torch.tensor(es) + srl[0, 0] / msz[y]
    seed_xyz = dy(0, 64, B, S, 3)
    vl = dy(-8, 9, B, N, 9)
    si = torch.stack([torch.randperm(N, generator=g) for _ in range(B)])
    vote = (seed_xyz[:, :, None] + dy(-8, 9, B, S, VF, 3)).clone()
    for b in range(B):
        row = lambda s: vl[b, si[b, s]]
        row(0)[3:6] = row(0)[0:3]; row(0)[6:9] = row(0)[0:3]        # all three GT votes equal ...
        vote[b, 0, :] = seed_xyz[b, 0] + row(0)[0:3] + torch.tensor([0.25, -0.125, 0.0])   # ... and three identical votes
        vote[b, 1, 1] = seed_xyz[b, 1] + row(1)[0:3]                # a vote that hits its target: d = 0, sign(0) = 0
        vote[b, 2, :] = vote[b, 2, 0]                               # three identical votes, distinct GT votes
        row(3)[3:6] = row(3)[0:3]; row(3)[6:9] = row(3)[0:3]        # all three GT votes equal, distinct votes
        t4 = seed_xyz[b, 4] + row(4)[0:3]                           # two votes at the same distance on either side, then a farther one
        row(4)[3:6] = row(4)[0:3] + 4.0; row(4)[6:9] = row(4)[0:3] - 4.0
        vote[b, 4, 0] = t4 + torch.tensor([0.125, 0.0, 0.0])
        vote[b, 4, 1] = t4 - torch.tensor([0.125, 0.0, 0.0])
        vote[b, 4, 2] = t4 + torch.tensor([0.0, 0.25, 0.0])
    vm = torch.ones(B, N, dtype=torch.long)
    vm[0, si[0, 5]] = 0
    d = dict(seed_xyz=seed_xyz, vote_xyz=vote.reshape(B, S * VF, 3).contiguous(), seed_inds=si.int(), vote_label=vl,
             vote_label_mask=vm, center_label=gt, box_label_mask=bm, aggregated_vote_xyz=agg, heading_class_label=hcl,
             heading_residual_label=hrl, size_class_label=scl, size_residual_label=srl, sem_cls_label=sem)
    return d, net, dict(NH=NH, NS=NS, NC=NC, mean_size_arr=mean_size)


def _grey(d, lo, hi):
    """every proposal at a distance in [lo, hi] of its real centre, 3 m and more from every other one"""
    B, K = d["aggregated_vote_xyz"].shape[:2]
    g = torch.Generator().manual_seed(11)
    gt = d["center_label"]
    gt[:, :8, :3] = torch.tensor([[1.0 + 3.0 * (i % 3), 1.0 + 3.0 * (i // 3), 1.0] for i in range(8)])
    dirs = torch.nn.functional.normalize(torch.randn(B, K, 3, generator=g), dim=-1)
    rad = lo + (hi - lo) * torch.rand(B, K, 1, generator=g)
    d["aggregated_vote_xyz"] = gt[:, torch.arange(K) % 8, :3] + dirs * rad


# name: builder keywords.  The seeds come from a CPU search for "nothing contested, all three label classes", which the first
# seed tried passes for every case; test_case_holds_the_conditions_of_the_bound (tests/test_detloss_bound_cpu.py) holds them to it
_SHAPES = {
    "two_trips_A": dict(B=3, S=5500, K=64, G=16, N=6000, NH=1, NS=18, NC=18, VF=1, seed=0),
    "two_trips_B": dict(B=3, S=64, K=5500, G=8, N=100, NH=2, NS=3, NC=4, VF=3, seed=0),
    "two_trips_C": dict(B=2, S=64, K=8, G=8200, N=100, NH=2, NS=3, NC=4, VF=2, seed=0, n_real=4100, room=(80.0, 80.0, 3.0),
                        real_last=True),       # the real boxes last: the second trip of pass C holds real rows
    "one": dict(B=1, S=1, K=1, G=1, N=1, NH=1, NS=1, NC=1, VF=1, seed=0),
    "limits": dict(B=2, S=96, K=72, G=24, N=200, NH=32, NS=32, NC=32, VF=2, seed=0, i64=True, cl_w=6, logit_rows=3),
    "bench_like": dict(B=4, S=1024, K=256, G=128, N=5000, NH=12, NS=18, NC=18, VF=2, seed=0),
    "no_positive": dict(B=2, S=64, K=48, G=16, N=100, NH=2, NS=3, NC=4, VF=1, seed=0),
    "all_grey": dict(B=2, S=64, K=48, G=16, N=100, NH=2, NS=3, NC=4, VF=1, seed=0),
    "no_vote_mask": dict(B=2, S=64, K=48, G=16, N=100, NH=2, NS=3, NC=4, VF=1, seed=0),
    "no_box": dict(B=2, S=64, K=48, G=16, N=100, NH=2, NS=3, NC=4, VF=1, seed=0),
}
CASES = tuple(_SHAPES) + ("ties",)
RANDOM_CASES = ("two_trips_A", "two_trips_B", "two_trips_C", "limits", "bench_like")   # held to the label-ratio caps


def decode(net, d, NH, NS):
    """proposal_module.decode_scores' slicing of the head output (B, K, 2 + 3 + 2 NH + 4 NS + NC)"""
    B, K = net.shape[:2]
    o, out = 0, dict(d)
    out["objectness_scores"] = net[:, :, o:o + 2]; o += 2
    out["center"] = d["aggregated_vote_xyz"] + net[:, :, o:o + 3]; o += 3
    out["heading_scores"] = net[:, :, o:o + NH]; o += NH
    out["heading_residuals_normalized"] = net[:, :, o:o + NH]; o += NH
    out["size_scores"] = net[:, :, o:o + NS]; o += NS
    out["size_residuals_normalized"] = net[:, :, o:o + NS * 3].view(B, K, NS, 3); o += NS * 3
    out["sem_cls_scores"] = net[:, :, o:]
    return out


@functools.lru_cache(maxsize=None)
def case(name, seed=None):
    """-> (d, net, cfg): the label / input tensors, the head output (B, K, channels) and the config namespace, all on the CPU.
    Shared between tests: do not write to the tensors."""
    if name == "ties":
        d, net, c = _ties_case()
    else:
        kw = dict(_SHAPES[name])
        if seed is not None:
            kw["seed"] = seed
        d, net, c = _random_case(**kw)
        if name == "one":
            d["aggregated_vote_xyz"] = d["center_label"][:, :1, :3] + 0.1          # the one proposal is positive
            d["vote_label_mask"] = torch.ones_like(d["vote_label_mask"])
        elif name == "no_positive":
            _grey(d, 0.35, 0.9)
        elif name == "all_grey":
            _grey(d, 0.35, 0.55)
        elif name == "no_vote_mask":
            d["vote_label_mask"] = torch.zeros_like(d["vote_label_mask"])
        elif name == "no_box":
            d["box_label_mask"] = torch.zeros_like(d["box_label_mask"])
    cfg = types.SimpleNamespace(num_heading_bin=c["NH"], num_size_cluster=c["NS"], num_class=c["NC"], mean_size_arr=c["mean_size_arr"])
    return d, net, cfg


def tensors(name, seed=None):
    """the dict reference() and emulate() read: the inputs plus the decoded head outputs"""
    d, net, cfg = case(name, seed)
    return decode(net, d, cfg.num_heading_bin, cfg.num_size_cluster), cfg


# ---- reference and bound ----------------------------------------------------------------------------------------------------------
def _first_min(x, e):
    """first index of the minimum along the last dim, the minimum, the relative gap to the next DIFFERENT value, and whether
    another value lies within the errors e of it"""
    n = x.shape[-1]
    lo = x.amin(-1, keepdim=True)
    idx = torch.where(x == lo, torch.arange(n), n).amin(-1)
    other = x != lo
    e_lo = e.gather(-1, idx.unsqueeze(-1))
    contested = (other & (x - e <= lo + e_lo)).any(-1)
    nxt = torch.where(other, x, torch.full_like(x, float("inf"))).amin(-1)
    margin = (nxt - lo[..., 0]) / lo[..., 0].clamp_min(1e-300)
    return idx, lo[..., 0], margin, contested


def _ce(x, y):
    """fp64 -log_softmax(x)[y] over the last dim, the softmax q, and their errors e_l, e_q (docstring)"""
    n = x.shape[-1]
    t = x - x.amax(-1, keepdim=True)
    p = t.exp()
    se = p.sum(-1, keepdim=True)
    q = p / se
    lse = se.log()[..., 0]
    ty = t.gather(-1, y.unsqueeze(-1))[..., 0]
    l = -(ty - lse)
    if n == 1:
        return l, q, torch.zeros_like(l), torch.zeros_like(q)
    rel_se = U * ((q * t.abs()).sum(-1) + 4 + n - 1)
    e_l = U * ty.abs() + rel_se + 4 * U * lse.abs() + U * l.abs()
    e_q = q * (U * t.abs() + 4 * U + rel_se.unsqueeze(-1) + 2 * U)
    return l, q, e_l, e_q


def _huber(e):
    a = e.abs()
    q = a.clamp(max=1.0)
    return 0.5 * q * q + (a - q)


def _onehot(y, n):
    return torch.nn.functional.one_hot(y, n).double()


def reference(t, cfg, check=True):
    """-> dict: terms (8,), tol_terms, ratios (2,), tol_ratios, the three label tensors, grads / tol_grads {name: fp64 like the
    output} (of the term alone: unit upstream gradient), sign_contested (bool like vote_xyz), m_over_den (like vote_xyz),
    picks i1 ic k2 bj bv, margins {decision: smallest fp64 margin}, contested {decision: count}.  check: assert the conditions"""
    f = lambda k: t[k].double()
    B, S = t["seed_xyz"].shape[:2]
    VF = t["vote_xyz"].shape[1] // S
    K, G = t["center"].shape[1], t["center_label"].shape[1]
    NH, NS, NC = t["heading_scores"].shape[2], t["size_scores"].shape[2], t["sem_cls_scores"].shape[2]
    R = dict(margins={}, contested={})

    def summed(vals, e_vals, count, den):
        """(sum / den, its tolerance without the 3 u of the normalisation)"""
        s = vals.sum()
        return s / den, (depth(count) * U * vals.abs().sum() + e_vals.sum()) / den

    # vote
    ind = t["seed_inds"].long()
    m = torch.gather(t["vote_label_mask"], 1, ind).double()
    vl = torch.gather(f("vote_label"), 1, ind.unsqueeze(-1).expand(-1, -1, 9)).view(B, S, 3, 3)
    T = vl + f("seed_xyz")[:, :, None, :]                                    # (B, S, j, c)
    rT = U * T.abs() * (T.float().double() != T)
    vx = f("vote_xyz").view(B, S, VF, 3)
    e = vx[:, :, None, :, :] - T[:, :, :, None, :]                           # (B, S, j, v, c)
    dist = e.abs().sum(-1)
    e_dist = rT.sum(-1, keepdim=True) + 3 * U * dist
    pick, best, mg, ct = _first_min(dist.reshape(B, S, 3 * VF), e_dist.reshape(B, S, 3 * VF))
    bj, bv = pick // VF, pick % VF
    e_best = e_dist.reshape(B, S, 3 * VF).gather(-1, pick.unsqueeze(-1))[..., 0]
    R["margins"]["vote_pick"], R["contested"]["vote_pick"] = float(mg.min()), int(ct.sum())
    den_v = m.sum() + 1e-6
    vote_loss, tol_vote = summed(best * m, e_best * m, B * S, den_v)
    ix = pick.view(B, S, 1, 1).expand(-1, -1, 1, 3)
    e_pick = e.reshape(B, S, 3 * VF, 3).gather(2, ix)[:, :, 0]               # (B, S, 3): vote[bv] - T[bj]
    rT_pick = rT.gather(2, bj.view(B, S, 1, 1).expand(-1, -1, 1, 3))[:, :, 0]
    sel = torch.nn.functional.one_hot(bv, VF).double().unsqueeze(-1)         # (B, S, VF, 1)
    g_vote = (sel * (m[:, :, None] * torch.sign(e_pick) / den_v).unsqueeze(2)).reshape(B, S * VF, 3)
    R["sign_contested"] = ((sel > 0) & ((rT_pick > 0) & (e_pick.abs() <= rT_pick)).unsqueeze(2)).reshape(B, S * VF, 3) & (m > 0).repeat_interleave(VF, 1).unsqueeze(-1)
    held = (rT_pick > 0) & (m > 0).unsqueeze(-1)                            # |e| in units of the rounding it must clear
    R["margins"]["sign"] = float((e_pick.abs() / rT_pick.clamp_min(1e-300))[held].min()) if held.any() else float("inf")
    R["m_over_den"] = (sel * (m / den_v)[:, :, None, None]).expand(-1, -1, -1, 3).reshape(B, S * VF, 3)

    # objectness
    gt = f("center_label")[:, :, :3]
    D1 = (f("aggregated_vote_xyz")[:, :, None] - gt[:, None]).square().sum(-1)   # (B, K, G)
    i1, d1, mg, ct = _first_min(D1, 5 * U * D1)
    R["margins"]["i1"], R["contested"]["i1"] = float(mg.min()), int(ct.sum())
    eu = (d1 + 1e-6).sqrt()
    near = eu < NEAR
    msk = (near | (eu > FAR)).double()
    lab = near.double()
    thr = torch.minimum((eu - NEAR).abs() / NEAR, (eu - FAR).abs() / FAR)
    R["margins"]["threshold"], R["contested"]["threshold"] = float(thr.min()), int((thr <= 8 * U).sum())
    w = torch.tensor(W_OBJ, dtype=torch.float64)[near.long()]
    l, q, e_l, e_q = _ce(f("objectness_scores"), near.long())
    den_o = msk.sum() + 1e-6
    obj_loss, tol_obj = summed(w * l * msk, (w * e_l + U * (w * l).abs()) * msk, B * K, den_o)
    wm = (w * msk).unsqueeze(-1)
    g_obj = wm * (q - _onehot(near.long(), 2))
    e_obj = wm * e_q + 2 * U * g_obj.abs()
    npos = lab.sum()
    den_p = npos + 1e-6

    # centre
    c = f("center")
    D2 = (c[:, :, None] - gt[:, None]).square().sum(-1)                      # (B, K, G)
    ic, dc, mg, ct = _first_min(D2, 5 * U * D2)
    R["margins"]["ic"], R["contested"]["ic"] = float(mg.min()), int(ct.sum())
    D2t = D2.transpose(1, 2)
    k2, d2, mg, ct = _first_min(D2t, 5 * U * D2t)                            # (B, G)
    R["margins"]["k2"], R["contested"]["k2"] = float(mg.min()), int(ct.sum())
    bmask = f("box_label_mask")
    den_b = bmask.sum() + 1e-6
    c1, tol_c1 = summed(dc * lab, 5 * U * dc * lab, B * K, den_p)
    c2, tol_c2 = summed(d2 * bmask, 5 * U * d2 * bmask, B * G, den_b)
    center_loss = c1 + c2
    tol_center = tol_c1 + tol_c2 + 3 * U * (c1.abs() + c2.abs()) + U * center_loss.abs()
    own = 2.0 * (c - torch.gather(gt, 1, ic.unsqueeze(-1).expand(-1, -1, 3))) * lab.unsqueeze(-1) / den_p
    hit = torch.nn.functional.one_hot(k2, K).double() * bmask.unsqueeze(-1)  # (B, G, K)
    share = 2.0 * hit.transpose(1, 2).unsqueeze(-1) * (c[:, :, None] - gt[:, None]) / den_b   # (B, K, G, 3)
    g_center = own + share.sum(2)
    mag = own.abs() + share.abs().sum(2)
    n_add = hit.sum(1).unsqueeze(-1)                                         # adds onto the own share
    e_center = (U + 3 * U) * own.abs() + (2 * U + 3 * U) * share.abs().sum(2) + n_add * U * mag

    # heading, size, semantic class: labels of the assigned box
    def boxlab(k):
        return torch.gather(t[k], 1, i1)
    grads = {"vote_xyz": g_vote, "objectness_scores": g_obj / den_o, "center": g_center}
    tols = {"vote_xyz": 3 * U * g_vote.abs(), "objectness_scores": e_obj / den_o + 3 * U * (g_obj / den_o).abs(), "center": e_center}
    terms = [vote_loss, obj_loss, center_loss]
    tol_terms = [tol_vote + 3 * U * vote_loss.abs(), tol_obj + 3 * U * obj_loss.abs(), tol_center]

    def add_ce(name, scores, y):
        l, q, e_l, e_q = _ce(scores, y)
        term, tol = summed(l * lab, e_l * lab, B * K, den_p)
        g = lab.unsqueeze(-1) * (q - _onehot(y, scores.shape[-1])) / den_p
        tg = lab.unsqueeze(-1) * (e_q / den_p) + (U + 3 * U) * g.abs()
        grads[name], tols[name] = g, tg + 3 * TINY * (tg > 0)
        terms.append(term); tol_terms.append(tol + 3 * U * term.abs())

    yh = boxlab("heading_class_label")
    add_ce("heading_scores", f("heading_scores"), yh)
    quot = boxlab("heading_residual_label").double() / (math.pi / NH)
    e = torch.gather(f("heading_residuals_normalized"), 2, yh.unsqueeze(-1))[..., 0] - quot
    e_e = 3 * U * quot.abs() + U * e.abs()
    h = _huber(e)
    term, tol = summed(h * lab, (e_e + 2 * U * h) * lab, B * K, den_p)
    terms.append(term); tol_terms.append(tol + 3 * U * term.abs())
    oh = _onehot(yh, NH)
    g = oh * (lab * e.clamp(-1.0, 1.0) / den_p).unsqueeze(-1)
    grads["heading_residuals_normalized"], tols["heading_residuals_normalized"] = g, oh * (lab * e_e / den_p).unsqueeze(-1) + 3 * U * g.abs()

    ys = boxlab("size_class_label")
    add_ce("size_scores", f("size_scores"), ys)
    srl = torch.gather(f("size_residual_label"), 1, i1.unsqueeze(-1).expand(-1, -1, 3))
    msz = torch.from_numpy(np.ascontiguousarray(np.asarray(cfg.mean_size_arr, dtype=np.float32))).double()
    quot = srl / msz[ys]
    e = torch.gather(f("size_residuals_normalized"), 2, ys.view(B, K, 1, 1).expand(-1, -1, 1, 3))[:, :, 0] - quot   # (B, K, 3)
    e_e = U * quot.abs() + U * e.abs()
    h3 = _huber(e)
    h = h3.sum(-1) / 3.0
    term, tol = summed(h * lab, ((e_e + 2 * U * h3).sum(-1) / 3.0 + 3 * U * h) * lab, B * K, den_p)
    terms.append(term); tol_terms.append(tol + 3 * U * term.abs())
    oh = _onehot(ys, NS).unsqueeze(-1)                                       # (B, K, NS, 1)
    g = oh * (lab.unsqueeze(-1) * e.clamp(-1.0, 1.0) / 3.0 / den_p).unsqueeze(2)
    grads["size_residuals_normalized"] = g
    tols["size_residuals_normalized"] = oh * (lab.unsqueeze(-1) * e_e / 3.0 / den_p).unsqueeze(2) + (2 * U + 3 * U) * g.abs()
    # (the heading_reg / size_reg terms sit at indices 4 and 6: the appends above ran in the order 3, 4, 5, 6)
    add_ce("sem_cls_scores", f("sem_cls_scores"), boxlab("sem_cls_label"))

    total = float(B * K)
    pos, allm = npos / total, msk.sum() / total
    R.update(terms=torch.stack(terms), tol_terms=torch.stack(tol_terms), ratios=torch.stack([pos, allm - pos]),
             tol_ratios=torch.stack([U * pos, U * (allm + pos) + U * (allm - pos).abs()]),
             objectness_label=near.long(), objectness_mask=msk.float(), object_assignment=i1, grads=grads, tol_grads=tols,
             i1=i1, ic=ic, k2=k2, bj=bj, bv=bv, npos=float(npos))
    R["sign_share"] = float(R["sign_contested"].sum()) / R["sign_contested"].numel()
    if check:
        bad = {k: v for k, v in R["contested"].items() if v}
        assert not bad, "contested decisions: %r" % bad
        assert R["sign_share"] <= SIGN_CAP, "contested sign share %.3g" % R["sign_share"]
    return R


@functools.lru_cache(maxsize=None)
def reference_of(name):
    t, cfg = tensors(name)
    return reference(t, cfg)


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def autograd_slack(ref, tw=TW):
    """what torch autograd of the COMPOSITION adds to the two Huber gradients, and the kernel does not: it forms the derivative of
    0.5 q^2 + (a - q) as g0 + (g0 q - g0), each add rounding relative to the upstream g0 = lab / npos (/ 3), not to the result"""
    out = {}
    for n, third in (("heading_residuals_normalized", 1.0), ("size_residuals_normalized", 3.0)):
        g0 = ref["objectness_label"].double() / (ref["npos"] + 1e-6) / third * abs(tw[NAMES.index(n)])
        g0 = g0.unsqueeze(-1) if third == 1.0 else g0.unsqueeze(-1).unsqueeze(-1)
        out[n] = 2 * U * g0 * (ref["grads"][n] != 0)
    return out


def compare(out, ref, tw=TW, slack=None):
    """out: terms (8,), ratios (2,), the three label tensors, grads {name: the gradient of sum_t tw[t] term[t]}.
    -> (worst {output: |err| / tol}, failures [str]): the ONE comparison of the CPU and the GPU module.  slack: autograd_slack(),
    for the torch composition only"""
    worst, fails = {}, []

    def hold(kind, got, want, tol):
        r, msg = excess(got, want, tol)
        worst[kind] = r
        if msg:
            fails.append("%s: %s" % (kind, msg))
    for k in LABELS:
        got = out[k].detach().cpu()
        if got.dtype != ref[k].dtype or not torch.equal(got, ref[k]):
            fails.append("%s differs from the reference at %d places" % (k, int((got.double() != ref[k].double()).sum())))
    hold("terms", out["terms"], ref["terms"], ref["tol_terms"])
    hold("ratios", out["ratios"], ref["ratios"], ref["tol_ratios"])
    for i, n in enumerate(NAMES):
        g, tol = ref["grads"][n] * tw[i], ref["tol_grads"][n] * abs(tw[i])
        tol = tol + U * g.abs() + TINY * (tol > 0)
        if n == "vote_xyz":
            und = ref["sign_contested"]
            g = torch.where(und, torch.zeros_like(g), g)
            tol = torch.where(und, ref["m_over_den"] * abs(tw[i]) * (1 + 4 * U), tol)
        if slack and n in slack:
            tol = tol + slack[n]
        hold("g_" + n, out["grads"][n], g, tol)
    return worst, fails


# ---- fp32 emulation of the kernels' arithmetic and partition ------------------------------------------------------------------------
F32 = torch.float32
DEFECTS = ("drop_A", "drop_B", "drop_C", "batch_mod", "last_i1", "last_k2", "last_vote", "sign0", "labels_via_ic", "skip_padded",
           "huber_unclamped", "no_third", "weights_swapped", "share_div_npos", "partial_left_out", "neg_no_sub", "cl_stride3",
           "seed_i64_as_i32", "wrong_upstream")


def _grid_sum(v, skip_block=None):
    """the sum of the per-item fp32 values v (n,) as the grid forms it: item -> thread (it mod 16384, trips in order) -> wave
    butterfly -> 4 waves in order -> 64 block partials in order"""
    n = v.numel()
    n_t = max(_cdiv(n, DL_ALL), 1)
    buf = torch.zeros(n_t * DL_ALL, dtype=F32)
    buf[:n] = v
    buf = buf.view(n_t, 64, 4, 64)
    acc = torch.zeros(64, 4, 64, dtype=F32)
    for i in range(n_t):
        acc = acc + buf[i]
    w = 64
    while w > 1:
        w //= 2
        acc = acc[..., :w] + acc[..., w:2 * w]
    acc = acc[..., 0]                                                        # (64 blocks, 4 waves)
    part = torch.zeros(64, dtype=F32)
    for k in range(4):
        part = part + acc[:, k]
    tot = torch.zeros((), dtype=F32)
    for b in range(64):
        if b != skip_block:
            tot = tot + part[b]
    return tot


def _argmin32(x, last=False):
    n = x.shape[-1]
    lo = x.amin(-1, keepdim=True)
    ar = torch.arange(n)
    return torch.where(x == lo, ar, -1).amax(-1) if last else torch.where(x == lo, ar, n).amin(-1)


def _ce32(x, y):
    t = x - x.amax(-1, keepdim=True)
    p = t.exp()
    se = torch.zeros_like(p[..., 0])
    for i in range(p.shape[-1]):
        se = se + p[..., i]
    lse, inv = se.log(), 1.0 / se
    return -(t.gather(-1, y.unsqueeze(-1))[..., 0] - lse), p * inv.unsqueeze(-1)


def _huber32(e):
    a = e.abs()
    q = a.clamp(max=1.0)
    return (0.5 * q) * q + (a - q)


def emulate(t, cfg, tw=TW, defect=None):
    """the kernels' results in fp32 on the CPU, in compare()'s form; defect: one of DEFECTS, planted"""
    assert defect is None or defect in DEFECTS
    is_ = lambda n: defect == n
    B, S = t["seed_xyz"].shape[:2]
    VF = t["vote_xyz"].shape[1] // S
    K, G, N = t["center"].shape[1], t["center_label"].shape[1], t["vote_label"].shape[1]
    NH, NS, NC = t["heading_scores"].shape[2], t["size_scores"].shape[2], t["sem_cls_scores"].shape[2]
    one, eps = torch.tensor(1.0, dtype=F32), torch.tensor(1e-6, dtype=F32)
    live = lambda n, on: (torch.arange(n) < DL_ALL) if on else torch.ones(n, dtype=torch.bool)

    # pass A
    it = torch.arange(B * S)
    b = it // S
    if is_("batch_mod"):
        b = torch.where(it >= DL_ALL, (it % DL_ALL) // S, b)
    si = t["seed_inds"].contiguous()
    ind = (si.view(torch.int32).reshape(-1)[:B * S] if is_("seed_i64_as_i32") and si.dtype == torch.int64 else si.reshape(-1)).long()
    m = t["vote_label_mask"].reshape(-1)[b * N + ind].float()
    vl = t["vote_label"].reshape(B * N, 3, 3)[b * N + ind]                  # (BS, j, c)
    T = vl + t["seed_xyz"].reshape(B * S, 1, 3)
    vx = t["vote_xyz"].reshape(B * S, VF, 3)
    e = vx[:, None, :, :] - T[:, :, None, :]                                 # (BS, j, v, c)
    a = e.abs()
    dist = ((a[..., 0] + a[..., 1]) + a[..., 2]).reshape(B * S, 3 * VF)
    pick = _argmin32(dist, last=is_("last_vote"))
    best = dist.gather(1, pick.unsqueeze(1))[:, 0]
    keepA = live(B * S, is_("drop_A")).float()
    s_vote, s_vm = _grid_sum(best * m * keepA), _grid_sum(m * keepA)
    ep = e.reshape(B * S, 3 * VF, 3).gather(1, pick.view(-1, 1, 1).expand(-1, 1, 3))[:, 0]
    sg = torch.sign(ep) if not is_("sign0") else torch.where(ep >= 0, 1.0, -1.0)
    g_vote = torch.nn.functional.one_hot(pick % VF, VF).float().unsqueeze(-1) * (m * keepA).unsqueeze(-1).unsqueeze(-1) * sg.unsqueeze(1)

    # pass B
    cl = t["center_label"]
    if is_("cl_stride3"):
        flat = cl.reshape(-1)
        gt = torch.stack([flat[bb * G * 3:bb * G * 3 + G * 3].view(G, 3) for bb in range(B)])
    else:
        gt = cl[:, :, :3]
    bmask = t["box_label_mask"].float()

    def sqd(p):
        d = p[:, :, None] - gt[:, None]
        d = d * d
        return (d[..., 0] + d[..., 1]) + d[..., 2]
    D1 = sqd(t["aggregated_vote_xyz"])
    D1s = torch.where(bmask[:, None] > 0, D1, torch.full_like(D1, float("inf"))) if is_("skip_padded") else D1
    i1 = _argmin32(D1s, last=is_("last_i1"))
    d1 = D1s.gather(2, i1.unsqueeze(-1))[..., 0]
    eu = (d1 + eps).sqrt()
    near = eu < torch.tensor(NEAR, dtype=F32)
    msk = (near | (eu > torch.tensor(FAR, dtype=F32))).float()
    lab = near.float()
    keepB = live(B * K, is_("drop_B")).view(B, K)
    lab_s, msk_s = lab * keepB, msk * keepB                                 # what reaches the sums and the gradient buffers
    wn, wp = torch.tensor(W_OBJ[0], dtype=F32), torch.tensor(W_OBJ[1], dtype=F32)
    if is_("weights_swapped"):
        wn, wp = wp, wn
    w = torch.where(near, wp, wn)
    c = t["center"]
    D2 = sqd(c)
    ic = _argmin32(D2)
    dc = D2.gather(2, ic.unsqueeze(-1))[..., 0]
    l, p = _ce32(t["objectness_scores"], near.long())
    S_ = {}
    S_["obj"], S_["om"], S_["np"] = _grid_sum(((w * l) * msk_s).reshape(-1)), _grid_sum(msk_s.reshape(-1)), _grid_sum(lab_s.reshape(-1))
    g_obj = (w * msk_s).unsqueeze(-1) * (p - torch.nn.functional.one_hot(near.long(), 2).float())
    S_["c1"] = _grid_sum((dc * lab_s).reshape(-1))
    g_cen = 2.0 * (c - torch.gather(gt, 1, ic.unsqueeze(-1).expand(-1, -1, 3))) * lab_s.unsqueeze(-1)
    via = ic if is_("labels_via_ic") else i1
    yh = torch.gather(t["heading_class_label"], 1, via)
    l, p = _ce32(t["heading_scores"], yh)
    S_["hc"] = _grid_sum((l * lab_s).reshape(-1))
    g_hs = lab_s.unsqueeze(-1) * (p - torch.nn.functional.one_hot(yh, NH).float())
    head_bin = torch.tensor(3.14159265358979323846, dtype=F32) / torch.tensor(float(NH), dtype=F32)
    e = torch.gather(t["heading_residuals_normalized"], 2, yh.unsqueeze(-1))[..., 0] - torch.gather(t["heading_residual_label"], 1, via) / head_bin
    S_["hr"] = _grid_sum((_huber32(e) * lab_s).reshape(-1))
    clampf = (lambda v: v) if is_("huber_unclamped") else (lambda v: v.clamp(-1.0, 1.0))
    g_hr = torch.nn.functional.one_hot(yh, NH).float() * (lab_s * clampf(e)).unsqueeze(-1)
    ys = torch.gather(t["size_class_label"], 1, via)
    l, p = _ce32(t["size_scores"], ys)
    S_["sc"] = _grid_sum((l * lab_s).reshape(-1), skip_block=1 if is_("partial_left_out") else None)
    g_ss = lab_s.unsqueeze(-1) * (p - torch.nn.functional.one_hot(ys, NS).float())
    msz = torch.from_numpy(np.ascontiguousarray(np.asarray(cfg.mean_size_arr, dtype=np.float32)))
    e = (torch.gather(t["size_residuals_normalized"], 2, ys.view(B, K, 1, 1).expand(-1, -1, 1, 3))[:, :, 0]
         - torch.gather(t["size_residual_label"], 1, via.unsqueeze(-1).expand(-1, -1, 3)) / msz[ys])
    h3 = _huber32(e)
    hs = (h3[..., 0] + h3[..., 1]) + h3[..., 2]
    S_["sr"] = _grid_sum(((hs / 3.0) * lab_s).reshape(-1))
    third = one if is_("no_third") else one / 3.0
    g_sr = torch.nn.functional.one_hot(ys, NS).float().unsqueeze(-1) * ((lab_s.unsqueeze(-1) * clampf(e)) * third).unsqueeze(2)
    ysem = torch.gather(t["sem_cls_label"], 1, via)
    l, p = _ce32(t["sem_cls_scores"], ysem)
    S_["sem"] = _grid_sum((l * lab_s).reshape(-1))
    g_sem = lab_s.unsqueeze(-1) * (p - torch.nn.functional.one_hot(ysem, NC).float())

    # pass C
    D2t = D2.transpose(1, 2)                                                 # (B, G, K)
    k2 = _argmin32(D2t, last=is_("last_k2"))
    d2 = D2t.gather(2, k2.unsqueeze(-1))[..., 0]
    keepC = live(B * G, is_("drop_C")).view(B, G)
    S_["c2"], S_["bm"] = _grid_sum((d2 * bmask * keepC).reshape(-1)), _grid_sum((bmask * keepC).reshape(-1))
    k2 = torch.where(keepC, k2, torch.full_like(k2, -1))

    # finish
    inv_vm, inv_om = one / (s_vm + eps), one / (S_["om"] + eps)
    inv_np, inv_bm = one / (S_["np"] + eps), one / (S_["bm"] + eps)
    total = torch.tensor(float(B * K), dtype=F32)
    terms = torch.stack([s_vote * inv_vm, S_["obj"] * inv_om, S_["c1"] * inv_np + S_["c2"] * inv_bm, S_["hc"] * inv_np,
                         S_["hr"] * inv_np, S_["sc"] * inv_np, S_["sr"] * inv_np, S_["sem"] * inv_np])
    pos = S_["np"] / total
    ratios = torch.stack([pos, S_["om"] / total if is_("neg_no_sub") else S_["om"] / total - pos])
    g_cen = g_cen * inv_np
    inv_sh = inv_np if is_("share_div_npos") else inv_bm
    for g in range(G):                                                       # in ground-truth order
        kk = k2[:, g]
        rows = (kk >= 0).nonzero()[:, 0]
        if G > 64 and float(bmask[:, g].abs().sum()) == 0.0:
            continue                                                         # s = 0: adds +-0 (skipped for speed only)
        for bb in rows.tolist():
            k = int(kk[bb])
            s = 2.0 * bmask[bb, g] * inv_sh
            g_cen[bb, k] = g_cen[bb, k] + s * (c[bb, k] - gt[bb, g])
    grads = {"vote_xyz": g_vote.reshape(B, S * VF, 3) * inv_vm, "objectness_scores": g_obj * inv_om, "center": g_cen,
             "heading_scores": g_hs * inv_np, "heading_residuals_normalized": g_hr * inv_np, "size_scores": g_ss * inv_np,
             "size_residuals_normalized": g_sr * inv_np, "sem_cls_scores": g_sem * inv_np}
    up = [torch.tensor(v, dtype=F32) for v in tw]
    if is_("wrong_upstream"):
        up[3], up[4] = up[4], up[3]
    grads = {n: grads[n] * up[i] for i, n in enumerate(NAMES)}
    keepBl = keepB.long()
    return dict(terms=terms, ratios=ratios, objectness_label=near.long() * keepBl, objectness_mask=msk * keepB,
                object_assignment=i1 * keepBl, grads=grads)


def composition(t, cfg, tw=TW, dtype=torch.float32):
    """loss_helper's torch composition on the CPU in `dtype`, in compare()'s form (grads of sum_t tw[t] term[t])"""
    from bridgeqa_amd import loss_helper as lh
    d = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()}
    for n in NAMES:
        d[n] = d[n].detach().clone().requires_grad_(True)
    prev, lh.FUSED_DET_LOSS[0] = lh.FUSED_DET_LOSS[0], False
    try:
        _, dd = lh.get_detection_loss(d, cfg)
    finally:
        lh.FUSED_DET_LOSS[0] = prev
    terms = torch.stack([dd[k] for k in TERMS])
    (terms * torch.tensor(tw, dtype=dtype)).sum().backward()
    return dict(terms=terms.detach(), ratios=torch.stack([dd["pos_ratio"], dd["neg_ratio"]]).detach(),
                objectness_label=dd["objectness_label"], objectness_mask=dd["objectness_mask"].float(),
                object_assignment=dd["object_assignment"], grads={n: d[n].grad for n in NAMES})
