"""Reference, bound, inputs, emulation and case tables of the eval-mode SharedMLP kernel of csrc/mlp_eval.hip (mlp_eval_kernel,
bq_mlp_eval / _ext.mlp_eval) for tests/test_mlp_eval_bound_cpu.py and tests/test_mlp_eval_bound_gpu.py.  Nothing here needs a
GPU or the extension: both test modules hand a `launch(layers, tail, grouped, rows, pool)` callable to the hold_* functions
below -- the CPU module the blocked fp32 emulation of this file, the GPU module _ext.mlp_eval -- so the emulation passes the
very checks the kernel is held to.

REFERENCE.  fp64 from the operands the kernel sees: bf16 weights (n, ldw), bf16 input rows, fp32 BatchNorm tensors.
    fold     s = gamma / sqrt(var + eps), t = beta + (bias - mean) s      (gamma 1, beta 0, bias 0 where absent; eps as fp32)
    layer    acc = x W^T, z = acc s + t, relu?(z); stored bf16, or the max over each run of S rows, or the fp32 tail acc + bias
    grouped  x0 = RNE_bf16(v), v formed in fp32 on the CPU exactly as the kernel forms it: xyz[b, idx] - new_xyz[b, j] (one fp32
             subtract), then one IEEE fp32 divide by fp32(radius) when normalize; features RNE_bf16(feats[b, idx]); zero up to
             the next multiple of 32 channels (group_rows).  The build has -ffp-contract=off and no fast-math, divide and sqrtf
             are correctly rounded, so this composition is bit-exact on the device (test_point_major_and_bf16_grouping_vs_
             oracle_composition relies on the same).

EXACT TIER (single layer).  Dyadic operands: rows / features in {-2..2}, weights in {-1, 0, 1}, eps = 0, var in {16, 64, 256},
gamma in {1, -1, 0.5} or absent, beta a multiple of 1/8 in [-1, 1], mean and bias multiples of 1/8.  exact_layer() asserts its
own conditions: s, bias - mean, (bias - mean) s, t, acc s and z are fp32 numbers, and sum_k |w||x| in units of the input step is
below 2^24 -- then the fp32 accumulation is exact in any order and on any MFMA shape, every later step is exact, and the stored
value RNE_bf16(relu?(z)) is determined bit for bit; it is compared with == on values.  At least 99 % of a case's outputs have
bf16(z) == z (a change of the accumulator by one unit is then visible in the stored value) and at least 30 % are positive.
Two choices inside the issue's classes make the 99 % hold; a bf16 output has 8 significant bits, |acc| reaches ~100 at K = 512
(7 bits), so z = s (acc + (bias - mean)) + beta must not carry more than one further bit:
  * mean and bias share their fractional eighths (without a bias, mean is an integer), so bias - mean is an integer;
  * the grouped coordinates lie on the issue's 1/64 lattice but only at multiples of the radius 0.5 (of 1 without normalize), in
    a room of 4 steps, so v is an integer in -3..3.  Coordinates anywhere on the 1/64 lattice give v five fractional bits:
    measured bf16-exact share 80 % at C = 0 falling to 44 % at C = 509 (B M S = 2 x 37 x 16, width 64), so the 99 % condition
    and the free 1/64 grid cannot both stand; the grid yields.  The subtract and the divide at radii that are no power of two
    are held bit for bit by the identity probes instead.
Measured over the GPU tables: bf16-exact share 100 % in every case, alive 41 .. 53 %.

BOUND TIER (single layer).  u = 2^-24, K32 = the input channels rounded up to 32, A = |x| |W|^T:
    e_acc = 2 K32 u A            fp32 accumulation in any order; 2: an MFMA whose internal adds are not round-to-nearest
                                 (the project's MFMA line, tests/gemm_ref.py)
    e_s   = 8 u |s|              var + eps, sqrtf, 1 / ., gamma * .: four operations of at most 1 ulp = 2 u each
    e_t   = |d| e_s + 4 u |d s| + 2 u |t|,  d = bias - mean: the subtract (2 u |d|, carried through the product), the product
                                 (2 u |d s|) and the add (2 u |t|), each at most 1 ulp, plus the error s came with
    e_z   = |s| e_acc + |acc| e_s + e_t + u |acc s| + u |z|     (covers the contracted and the uncontracted acc s + t)
    ReLU  e = 0 where z < -e_z (the output is exactly 0), else e_z;  bf16 output: tol = 2^-8 (|r| + e) + e
    pooled: r = max over the group, tol = the max of the group's tolerances (max is 1-Lipschitz in the sup norm)
    tail  (fp32): r from the kernel's OWN stored bf16 output of the layer run without the tail -- the fused launch multiplies the
          same bits --, tol = e_acc + u |r| + u |bias| with K32 = the layer's width
    gamma = 0: DECIDED, tolerance 0.  s = 0 * (1 / sqrt(.)) = 0, t = beta + d * 0 = beta, z = acc * 0 + beta = beta whenever
          var + eps > 0 and acc, d are finite, in either form of the multiply-add: the stored value is RNE_bf16(relu?(beta)).
Chains carry no tolerance: every intermediate activation is rounded to bf16 in LDS and the plain epilogue copies the LDS tile,
so a fused 2- or 3-layer launch EQUALS the same layers launched one at a time through HBM rows (hold_chain), and a pooled
launch EQUALS the max over S of the unpooled one.

Against the issue's table: (1) e_t is written out above (the issue leaves it to be derived).  (2) The gamma = 0 channels are
compared against RNE_bf16(relu?(beta)) with tolerance 0 instead of 2^-8 |relu(t)|.  (3) The exact-tier coordinates are
restricted as said above.  Nothing else differs.  No comparison looser than equality was needed for the staged tile: the
kernel's value is RNE_bf16 of the fp32 composition in every element on the device.

MEASURED, worst |err| / tol per form.  Blocked fp32 emulation of this file (32-wide k-steps accumulated in fp32, acc*s + t in
fp32, bf16 stores) over every bound-tier case of the GPU tables:
    rows 0.994   grouped 0.994   pooled 0.992   tail 0.121
On an MI355X (profiles/mlp_eval_bound.md): rows 0.994, grouped 0.994, pooled 0.992, tail 0.070, the first layers of the route
0.995.  The bf16 forms sit just below 1 because a correct round-to-nearest just above a power of two uses the whole 2^-8 |r|;
below that rounding the fp32 part of their bound is as slack as the tail's.  The tail shows it alone: e_acc = 2 K32 u A is the
worst case over all summation orders with every rounding in the same direction, where sums of random signs err like
sqrt(K32) u.  It stays because it is the project's one MFMA line, and what a tail can get wrong -- a zeroed column, a missing
bias, a dropped k-step -- is orders of magnitude above it (the zeroed column is planted in the CPU module).
"""
import zlib

import torch

from ln_ref import excess  # noqa: F401  (the comparison of the test modules)

U = 2.0 ** -24
B8 = 2.0 ** -8
TM = 64                 # rows per workgroup (ME_TM)
OLD_NORMS = dict(emulation=3e-3, fp32=1e-2)     # tests/test_mlp_eval_gpu.py: rel-L2 against its emulation / the fp32 composition
BF16_EXACT_SHARE, ALIVE_SHARE = 0.99, 0.30
# channels 1 .. 5 of every bound-tier layer (widths are >= 32): running mean about 40 with a small variance, var = 0 under
# eps = 1e-5, var = 1e4, gamma = 0, gamma < 0
CH_MEAN40, CH_VAR0, CH_VARBIG, CH_GAMMA0, CH_GAMMA_NEG = 1, 2, 3, 4, 5
SPIKE = 24.0


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7FFFFFFF


def _gen(*key):
    return torch.Generator().manual_seed(_seed(*key))


def _bf(t):
    return t.to(torch.bfloat16)


def ceil32(k):
    return (k + 31) // 32 * 32


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def layer_spec(key, K, n, tier, relu=True, affine=True, bias=False, ldw_gap=False):
    """one BatchNorm layer spec of CPU tensors as _ext.mlp_eval takes it: w bf16 (n, ldw), zero from K to K32 and -- with
    ldw_gap -- NaN beyond K32 (the kernel reads K32 columns); mean, var, eps, relu; gamma / beta (affine) and bias optional"""
    g = _gen("layer", key, K, n, tier)
    K32 = ceil32(K)
    w = torch.zeros(n, K32 + (8 if ldw_gap else 0))
    w[:, K32:] = float("nan")
    if tier == "exact":
        w[:, :K] = torch.randint(-1, 2, (n, K), generator=g).float()
        var = torch.tensor([16.0, 64.0, 256.0])[torch.randint(0, 3, (n,), generator=g)]
        gamma = torch.tensor([1.0, -1.0, 0.5])[torch.randint(0, 3, (n,), generator=g)]
        beta = torch.randint(-8, 9, (n,), generator=g).float() / 8
        frac = torch.randint(0, 8, (n,), generator=g).float() / 8 if bias else torch.zeros(n)
        mean = torch.randint(-3, 4, (n,), generator=g).float() + frac
        cb = torch.randint(-3, 4, (n,), generator=g).float() + frac
        eps = 0.0
    else:
        # pre-activations of a few units, as in tests/test_mlp_eval_gpu.py
        w[:, :K] = torch.randn(n, K, generator=g) * (2.0 / K) ** 0.5 * 4.0
        gamma = torch.rand(n, generator=g) + 0.5
        beta = torch.randn(n, generator=g) * 0.5
        mean = torch.randn(n, generator=g) * 3.0
        var = torch.exp(torch.empty(n).uniform_(-2.3, 2.3, generator=g))
        cb = torch.randn(n, generator=g) * 3.0
        mean[CH_MEAN40], var[CH_MEAN40] = 40.0 + float(torch.randn((), generator=g)), 0.01
        cb[CH_MEAN40] = 39.0
        var[CH_VAR0], var[CH_VARBIG] = 0.0, 1e4
        gamma[CH_GAMMA0], gamma[CH_GAMMA_NEG] = 0.0, -0.75
        beta[CH_GAMMA0] = 0.40625                         # the whole channel is relu?(beta): keep it clear of 0
        if bias:
            mean = mean + cb
        eps = 1e-5
    spec = dict(w=_bf(w), mean=mean, var=var, eps=eps, relu=relu)
    if affine:
        spec.update(gamma=gamma, beta=beta)
    if bias:
        spec["bias"] = cb
    return spec


def tail_spec(key, k, n, bias=True):
    """the last linear layer: w bf16 (n, k), fp32 bias or none"""
    g = _gen("tail", key, k, n)
    spec = dict(w=_bf(torch.randn(n, k, generator=g) * (1.0 / k) ** 0.5))
    if bias:
        spec["bias"] = torch.randn(n, generator=g)
    return spec


def rows_input(key, R, K, tier, ldx_gap=False):
    """bf16 (R, ldx) rows, NaN from K to ldx = K + 8 with ldx_gap.  Bound tier: N(0, 1) with row R / 2 and column K / 3 scaled
    by 24"""
    g = _gen("rows", key, R, K, tier)
    x = torch.full((R, K + (8 if ldx_gap else 0)), float("nan"))
    if tier == "exact":
        x[:, :K] = torch.randint(-2, 3, (R, K), generator=g).float()
    else:
        v = torch.randn(R, K, generator=g)
        v[R // 2] *= SPIKE
        v[:, K // 3] *= SPIKE
        x[:, :K] = v
    return _bf(x)


def grouped_input(key, B, M, S, C, N, tier, radius, normalize):
    """dict(xyz (B, N, 3), new_xyz (B, M, 3), cloud (B, N, 3 + C + 2) -- the features are its strided slice [..., 3:3 + C], the
    two trailing columns hold NaN --, C, idx int32 (B, M, S), radius, normalize).  idx is drawn by hand: uniform, the second
    half of every neighbourhood repeats the first hit (but for one row, below), 0, N - 1 and the spiked point N / 2 are present.  Bound tier: point
    N / 2 and feature column C / 3 scaled by 24"""
    g = _gen("grouped", key, B, M, S, C, N, tier, radius, normalize)
    if tier == "exact":
        step = radius if normalize else 1.0
        xyz = torch.randint(0, 4, (B, N, 3), generator=g).float() * step
        f = torch.randint(-2, 3, (B, N, C), generator=g).float()
    else:
        xyz = torch.rand(B, N, 3, generator=g) * torch.tensor([4.0, 4.0, 2.0])
        f = torch.randn(B, N, C, generator=g)
        f[:, N // 2] *= SPIKE
        if C:
            f[:, :, C // 3] *= SPIKE
    cloud = torch.cat([xyz, f, torch.full((B, N, 2), float("nan"))], -1).contiguous()
    new_xyz = xyz[:, torch.randperm(N, generator=g)[:M]].contiguous()
    idx = torch.randint(0, N, (B, M, S), generator=g)
    idx[..., S // 2:] = idx[..., :1]
    # (N - 1 sits in the LAST row of the last group: the one row of the case that a pool over S - 1 rows would lose)
    idx[0, 0, 1], idx[0, 0, 3], idx[-1, -1, S - 1] = 0, N // 2, N - 1
    return dict(xyz=xyz.contiguous(), new_xyz=new_xyz, cloud=cloud, C=C, idx=idx.int(), radius=radius, normalize=normalize)


def group_rows(gi, idx=None, batch_of=None):
    """the staged input tile of the grouped form: bf16 (B M S, ceil32(3 + C)) -- RNE_bf16 of the fp32 composition, zero beyond
    3 + C.  idx / batch_of (the scene each row reads, (R,)) override the case's: the planted defects of the CPU module"""
    xyz, new_xyz, C = gi["xyz"], gi["new_xyz"], gi["C"]
    idx = gi["idx"] if idx is None else idx
    B, M, S = idx.shape
    R = B * M * S
    pos = torch.arange(R)
    b = pos // (M * S) if batch_of is None else batch_of
    ids = idx.reshape(R).long()
    v = xyz[b, ids] - new_xyz.reshape(B * M, 3)[pos // S]
    if gi["normalize"]:
        v = v / torch.tensor(gi["radius"], dtype=torch.float32)
    out = torch.zeros(R, ceil32(3 + C), dtype=torch.bfloat16)
    out[:, :3] = _bf(v)
    out[:, 3:3 + C] = _bf(gi["cloud"][b, ids, 3:3 + C])
    return out


def case_rows(c):
    """(x bf16 (R, K32) zero-padded, K, the launch's input keywords) of a case dict"""
    if "C" in c:
        gi = grouped_input(c["id"], c["B"], c["M"], c["S"], c["C"], c["N"], c["tier"], c["radius"], c["normalize"])
        return group_rows(gi), 3 + c["C"], dict(grouped=gi)
    xf = rows_input(c["id"], c["R"], c["K"], c["tier"], c.get("ldx_gap", False))
    K = c["K"]
    x = torch.zeros(c["R"], ceil32(K), dtype=torch.bfloat16)
    x[:, :K] = xf[:, :K]
    return x, K, dict(rows=(xf, K))


# ---- references and bounds ------------------------------------------------------------------------------------------------------
def fold(spec):
    """fp64 (s, t, e_s, e_t, d) of a layer spec"""
    n = spec["w"].shape[0]
    one, zero = torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    g = spec["gamma"].double() if spec.get("gamma") is not None else one
    be = spec["beta"].double() if spec.get("beta") is not None else zero
    cb = spec["bias"].double() if spec.get("bias") is not None else zero
    ve = spec["var"].double() + _f32(spec["eps"])
    assert bool((ve > 0).all()), "var + eps must be positive"
    s = g / ve.sqrt()
    d = cb - spec["mean"].double()
    t = be + d * s
    e_s = 8.0 * U * s.abs()
    e_t = d.abs() * e_s + 4.0 * U * (d * s).abs() + 2.0 * U * t.abs()
    return s, t, e_s, e_t, d


def _bf16_tol(r, e):
    return B8 * (r.abs() + e) + e


def layer(x, spec):
    """fp64 reference r and tolerance tol of one layer's bf16 output from its bf16 input rows x (R, K32)"""
    K32 = x.shape[1]
    w = spec["w"][:, :K32].double()
    assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(x.float()).all())
    xd = x.double()
    acc, A = xd @ w.t(), xd.abs() @ w.abs().t()
    s, t, e_s, e_t, _ = fold(spec)
    z = acc * s + t
    e = s.abs() * (2.0 * K32 * U * A) + acc.abs() * e_s + e_t + U * (acc * s).abs() + U * z.abs()
    if spec["relu"]:
        e = torch.where(z < -e, torch.zeros_like(e), e)
        z = z.clamp_min(0.0)
    tol = _bf16_tol(z, e)
    if spec.get("gamma") is not None:
        dec = spec["gamma"] == 0                    # decided channels: RNE_bf16(relu?(beta)), tolerance 0
        be = spec["beta"].double() if spec.get("beta") is not None else torch.zeros_like(s)
        zb = _bf(be.clamp_min(0.0) if spec["relu"] else be).double()
        z = torch.where(dec, zb.expand_as(z), z)
        tol = torch.where(dec, torch.zeros_like(tol), tol)
    return z, tol


def pooled(r, tol, S):
    """the max over each run of S rows and the max of the group's tolerances"""
    n = r.shape[1]
    return r.view(-1, S, n).amax(1), tol.view(-1, S, n).amax(1)


def tail(h, spec):
    """fp64 reference and tolerance of the fp32 tail from the stored bf16 rows h (R, k) of the layer before it"""
    k = h.shape[1]
    w = spec["w"][:, :k].double()
    hd = h.double()
    acc, A = hd @ w.t(), hd.abs() @ w.abs().t()
    b = spec["bias"].double() if spec.get("bias") is not None else torch.zeros(w.shape[0], dtype=torch.float64)
    r = acc + b
    return r, 2.0 * k * U * A + U * r.abs() + U * b.abs()


def _is_f32(v):
    return bool((v.float().double() == v).all())


def exact_layer(x, spec, unit=1.0):
    """(the bf16 output the kernel must store, share of outputs with bf16(z) == z, share of positive outputs) of an exact-tier
    layer; asserts the conditions under which the answer is determined bit for bit"""
    K32 = x.shape[1]
    w = spec["w"][:, :K32].double()
    xd = x.double()
    assert bool((xd / unit == (xd / unit).round()).all()), "input off the grid of `unit`"
    assert float((xd.abs() @ w.abs().t()).max()) / unit < 2.0 ** 24, "sum |w||x| reaches 2^24 units"
    assert _f32(spec["eps"]) == 0.0
    s, t, _, _, d = fold(spec)
    acc = xd @ w.t()
    z = acc * s + t
    for name, v in (("s", s), ("bias - mean", d), ("(bias - mean) s", d * s), ("t", t), ("acc s", acc * s), ("z", z)):
        assert _is_f32(v), "%s is not exactly representable in fp32" % name
    out = _bf(z.clamp_min(0.0) if spec["relu"] else z)
    exact_share = float((_bf(z).double() == z).double().mean())
    alive = float((z > 0).double().mean())
    return out, exact_share, alive


def fp32_composition(x, layers, tail_=None, pool_S=0):
    """the layers in fp32 without any bf16 rounding of the activations (the old norms' second reference)"""
    h = x.float()
    for spec in layers:
        s, t, _, _, _ = fold(spec)
        h = h @ spec["w"][:, :h.shape[1]].float().t() * s.float() + t.float()
        h = h.clamp_min(0.0) if spec["relu"] else h
    if tail_ is not None:
        h = h @ tail_["w"][:, :h.shape[1]].float().t() + (tail_["bias"] if tail_.get("bias") is not None else 0.0)
    return h.view(-1, pool_S, h.shape[1]).amax(1) if pool_S else h


def old_norms_accept(out, emu, ref32):
    """tests/test_mlp_eval_gpu.py: rel-L2 <= 3e-3 against the emulation with the kernel's rounding points and <= 1e-2 against
    the fp32 composition"""
    def rel(a, b):
        return ((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)).item()
    return (bool(torch.isfinite(out.float()).all()) and rel(out, emu) <= OLD_NORMS["emulation"]
            and rel(out, ref32) <= OLD_NORMS["fp32"])


# ---- blocked fp32 emulation of the kernel ---------------------------------------------------------------------------------------
def emulate_fold(spec, defect=None):
    """fp32 (s, t) as the kernel's prologue forms them.  defect ("no_bias", c): t of channel c without the conv bias"""
    n = spec["w"].shape[0]
    f = torch.float32
    g = spec["gamma"] if spec.get("gamma") is not None else torch.ones(n, dtype=f)
    be = spec["beta"] if spec.get("beta") is not None else torch.zeros(n, dtype=f)
    cb = spec["bias"] if spec.get("bias") is not None else torch.zeros(n, dtype=f)
    s = g * (torch.tensor(1.0, dtype=f) / torch.sqrt(spec["var"] + torch.tensor(spec["eps"], dtype=f)))
    if defect and defect[0] == "no_bias":
        cb = cb.clone()
        cb[defect[1]] = 0.0
    return s, be + (cb - spec["mean"]) * s


def _emulate_acc(x, w, defect=None):
    """fp32 (R, n) = x W^T in 32-wide k-steps.  defect ("drop_kstep", rb, ct): rows 16 rb .. and channels 16 ct .. miss the last"""
    K32 = x.shape[1]
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32)
    for k0 in range(0, K32, 32):
        step = x[:, k0:k0 + 32] @ w[:, k0:k0 + 32].t()
        if defect and defect[0] == "drop_kstep" and k0 + 32 >= K32:
            step[16 * defect[1]:16 * defect[1] + 16, 16 * defect[2]:16 * defect[2] + 16] = 0.0
        acc = acc + step
    return acc


def emulate_layer(x, spec, defect=None, keep_f32=False):
    """x bf16 (or fp32 with keep_f32) (R, K32) -> bf16 (R, n), fp32 unrounded with keep_f32 (a planted defect)"""
    s, t = emulate_fold(spec, defect)
    y = _emulate_acc(x.float(), spec["w"][:, :x.shape[1]].float(), defect) * s + t
    y = y.clamp_min(0.0) if spec["relu"] else y
    return y if keep_f32 else _bf(y)


def emulate(layers, tail=None, grouped=None, rows=None, pool=False, defect=None):
    """the launch in torch on the CPU, with _ext.mlp_eval's signature.  defect: None or one of ("neighbour", r),
    ("batch_first_row",), ("drop_kstep", rb, ct), ("no_bias", c), ("pool_short", g), ("pool_from_0", g), ("tail_col", c),
    ("f32_intermediate",) -- see tests/test_mlp_eval_bound_cpu.py"""
    kind = defect[0] if defect else None
    if grouped is not None:
        idx = grouped["idx"]
        B, M, S = idx.shape
        batch_of = None
        if kind == "neighbour":
            flat = idx.reshape(-1).clone()
            flat[defect[1]] = flat[defect[1] + 1]
            idx = flat.view(B, M, S)
        if kind == "batch_first_row":
            pos = torch.arange(B * M * S)
            batch_of = (pos // TM * TM) // (M * S)
        x = group_rows(grouped, idx, batch_of)
    else:
        xf, K = rows
        S = 0
        x = torch.zeros(xf.shape[0], ceil32(K), dtype=torch.bfloat16)
        x[:, :K] = xf[:, :K]
    for i, spec in enumerate(layers):
        x = emulate_layer(x, spec, defect if i == 0 else None, keep_f32=kind == "f32_intermediate" and i + 1 < len(layers))
    if tail is not None:
        y = _emulate_acc(x.float(), tail["w"][:, :x.shape[1]].float())
        if tail.get("bias") is not None:
            y = y + tail["bias"]
        if kind == "tail_col":
            y[:, defect[1]] = 0.0
        return y
    if not pool:
        return x
    v = x.float().view(-1, S, x.shape[1])
    out = v.amax(1)
    if kind == "pool_short":
        out[defect[1]] = v[defect[1], :S - 1].amax(0)
    if kind == "pool_from_0":
        out[defect[1]] = v[defect[1]].amax(0).clamp_min(0.0)
    return _bf(out)


# ---- the checks both test modules run ---------------------------------------------------------------------------------------------
class Hold:
    """collects the failures of one case and the worst |err| / tol per form; assert_ok() reports them all"""

    def __init__(self, name, worst):
        self.name, self.fails, self.worst = name, [], worst

    def __call__(self, kind, out, ref, tol):
        ratio, msg = excess(out, ref, tol)
        self.worst[kind] = max(self.worst.get(kind, 0.0), ratio)
        if msg:
            self.fails.append("%s %s: %s" % (self.name, kind, msg))

    def equal(self, what, a, b):
        a, b = a.detach().cpu(), b.detach().cpu()
        if a.shape != b.shape or a.dtype != b.dtype:
            self.fails.append("%s %s: %s %s against %s %s" % (self.name, what, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
            return
        bad = ~(a.double() == b.double())           # on values; NaN never equals
        if bad.any():
            i = tuple(int(v) for v in bad.nonzero()[0])
            self.fails.append("%s %s: %d of %d elements differ, first at %s: %r against %r" % (
                self.name, what, int(bad.sum()), a.numel(), i, float(a[i]), float(b[i])))

    def true(self, cond, msg):
        if not cond:
            self.fails.append("%s: %s" % (self.name, msg))

    def assert_ok(self):
        assert not self.fails, "\n".join(self.fails)


def hold_single(c, launch, hold):
    """a single-layer case of either tier and either input form; grouped cases run unpooled AND pooled, and the pooled
    output must also EQUAL the max over S of the unpooled one.  Returns (exact share, alive share) on the exact tier"""
    x, K, kw = case_rows(c)
    spec = layer_spec(c["id"], K, c["n"], c["tier"], c["relu"], c["affine"], c["bias"], c["ldw_gap"])
    out = launch([spec], **kw)
    S = c.get("S", 0)
    form = "grouped" if S else "rows"
    hold.true(out.dtype == torch.bfloat16 and tuple(out.shape) == (x.shape[0], c["n"]), "output %s %s" % (tuple(out.shape), out.dtype))
    shares = None
    if c["tier"] == "exact":
        want, share, alive = exact_layer(x, spec)
        shares = (share, alive)
        hold.equal(form + " exact", out, want)
        r, tol = want.double(), torch.zeros(want.shape, dtype=torch.float64)
    else:
        r, tol = layer(x, spec)
        hold(form, out, r, tol)
    if S:
        po = launch([spec], pool=True, **kw)
        hold.equal("pooled against the max of the unpooled launch", po, _bf(out.float().view(-1, S, c["n"]).amax(1)))
        pr, pt = pooled(r, tol, S)
        if c["tier"] == "exact":
            hold.equal("pooled exact", po, _bf(pr))
        else:
            hold("pooled", po, pr, pt)
    return shares


def hold_tail(c, launch, hold):
    """one layer + the fp32 tail against the fp64 tail of the launch's own stored layer output"""
    x, K, kw = case_rows(c)
    spec = layer_spec(c["id"], K, c["n"], "bound", True, True, False, False)
    ts = tail_spec(c["id"], c["n"], c["n_tail"], c["tail_bias"])
    h = launch([spec], **kw)
    out = launch([spec], tail=ts, **kw)
    hold.true(out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], c["n_tail"]), "output %s %s" % (tuple(out.shape), out.dtype))
    r, tol = tail(h.cpu(), ts)
    hold("tail", out, r, tol)


def selection_layers(kin32):
    """identity / selection layers that make the staged input tile observable: W picks columns start .. start + n, var = 1,
    eps = 0, mean = 0, no gamma, beta or bias, no ReLU, so z = x exactly.  [(start, spec)]: two for kin32 up to 512"""
    out = []
    for start in range(0, kin32, 256):
        n = min(256, kin32 - start)
        w = torch.zeros(n, kin32)
        w[torch.arange(n), start + torch.arange(n)] = 1.0
        out.append((start, dict(w=_bf(w), mean=torch.zeros(n), var=torch.ones(n), eps=0.0, relu=False)))
    return out


def hold_probe(c, launch, hold):
    """the staged tile (both gathers, the coordinates, the zero padding; the 16-byte row copies) element for element"""
    x, K, kw = case_rows(c)
    for start, spec in selection_layers(x.shape[1]):
        out = launch([spec], **kw)
        hold.equal("staged columns %d..%d" % (start, start + spec["w"].shape[0]), out, x[:, start:start + spec["w"].shape[0]])
    return x


def chain_specs(c):
    """(layers, tail or None) of a chain case"""
    k = 3 + c["C"] if "C" in c else c["K"]
    layers = []
    for i, n in enumerate(c["widths"]):
        layers.append(layer_spec((c["id"], i), k, n, "bound", relu=not (i == 1 and c["id"] % 2), affine=i != 2, bias=i == 0))
        k = n
    return layers, (tail_spec(c["id"], k, c["n_tail"]) if c.get("n_tail") else None)


def chained(launch, layers, tail_, kw, pool_S=0):
    """the same layers launched one at a time through HBM rows; the tail rides on the last layer's launch"""
    h = launch([layers[0]], tail=tail_ if len(layers) == 1 else None, **kw)
    for i, spec in enumerate(layers[1:], start=1):
        h = launch([spec], tail=tail_ if i + 1 == len(layers) else None, rows=(h, h.shape[1]))
    return _bf(h.float().view(-1, pool_S, h.shape[1]).amax(1)) if pool_S else h


def hold_chain(c, launch, hold):
    """fused equals chained, bit for bit: unpooled (or with the tail), and pooled for grouped cases"""
    _, _, kw = case_rows(c)
    layers, tail_ = chain_specs(c)
    hold.equal("fused against chained", launch(layers, tail=tail_, **kw), chained(launch, layers, tail_, kw))
    if "C" in c and tail_ is None:
        hold.equal("fused pooled against chained", launch(layers, pool=True, **kw), chained(launch, layers, None, kw, c["S"]))


# ---- the cases of tests/test_mlp_eval_bound_gpu.py (the CPU module checks the conditions on the same lists) ------------------------
ROWS_R = (1, 63, 64, 65, 301)
ROWS_K = (8, 40, 256, 512)
WIDTHS = (32, 96, 160, 224, 256)
GROUPED_BMS = ((1, 1, 64), (1, 3, 32), (2, 37, 16), (3, 5, 16))      # the last: 80 rows per scene, tiles that span two scenes
GROUPED_C = (0, 1, 4, 7, 29, 30, 132, 253, 256, 260, 509)             # vector gather: 4, 132, 256; scalar: the rest
GROUPED_N = (50, 173, 700)
TAIL_N = (1, 5, 16, 97, 259, 4096)
CHAIN_WIDTHS = ((64, 64, 128), (128, 128, 256), (128, 128, 128), (256, 256), (32, 64, 96), (160, 224))


def _opts(i):
    """relu on and off, gamma and beta absent, bias present, NaN gaps behind the rows and behind the weight rows: cycled so that
    every option meets every other over a list"""
    return dict(relu=i % 2 == 0, affine=i % 3 != 1, bias=i % 4 >= 2, ldx_gap=i % 5 in (1, 3), ldw_gap=i % 7 in (2, 3, 5))


def _rows_cases():
    out = []
    pairs = [(K, n) for K in ROWS_K for n in WIDTHS]                         # every (K, width); R cycles through its list
    pairs += [(40, 96)] * len(ROWS_R) + [(512, 256)] * len(ROWS_R)           # every R at a small and at the largest shape
    for i, (K, n) in enumerate(pairs):
        for tier in ("bound", "exact"):
            # (R = 1 meets the widest layers: 256 outputs, where the exact tier's alive share is no coin toss)
            out.append(dict(id=len(out), tier=tier, R=ROWS_R[(i + 1) % len(ROWS_R)], K=K, n=n, **_opts(i)))
    return out


def _grouped_cases():
    out = []
    i = 0
    for ci, C in enumerate(GROUPED_C):
        for bi, (B, M, S) in enumerate(GROUPED_BMS):
            for tier in ("bound", "exact"):
                o = _opts(i)
                o.pop("ldx_gap")
                out.append(dict(id=1000 + len(out), tier=tier, B=B, M=M, S=S, C=C, N=GROUPED_N[(ci + bi) % 3],
                                n=WIDTHS[(ci + 2 * bi) % 5], radius=0.5 if tier == "exact" else (0.2, 0.4)[(ci + bi) % 2],
                                normalize=(ci + bi // 2) % 2 == 0, **o))
            i += 1
    return out


ROWS_CASES = _rows_cases()
GROUPED_CASES = _grouped_cases()
TAIL_CASES = [dict(id=2000 + 2 * i + b, tier="bound", R=(65, 301, 63)[i % 3], K=(40, 256, 8)[i % 3], n=WIDTHS[(i + b) % 5],
                   n_tail=nt, tail_bias=bool(b)) for i, nt in enumerate(TAIL_N) for b in (1, 0)]
PROBE_CASES = ([dict(id=3000 + i, tier="bound", R=(65, 301)[i % 2], K=K, ldx_gap=i % 2 == 0) for i, K in enumerate(ROWS_K)]
               + [dict(id=3100 + i, tier="bound", B=B, M=M, S=S, C=C, N=GROUPED_N[i % 3], radius=(0.2, 0.4)[i % 2],
                       normalize=i % 3 != 2)
                  for i, (C, (B, M, S)) in enumerate((C, GROUPED_BMS[(j + k) % 4]) for j, C in enumerate(GROUPED_C) for k in (0, 2))])
# every 2- and 3-layer spec in use; layer 2 wider than the input at (32, 64, 96) / C = 0 and (160, 224) / C = 29 (the LDS buffers
# swap which is the larger), narrower at C = 509
_CHAIN_C = (132, 128, 256, 509, 0, 29)
_CHAIN_K = (256, 128, 512, 256, 8, 40)
CHAIN_CASES = ([dict(id=4000 + i, tier="bound", R=301, K=_CHAIN_K[i], widths=w) for i, w in enumerate(CHAIN_WIDTHS)]
               + [dict(id=4100 + i, tier="bound", R=(301, 65)[i % 2], K=_CHAIN_K[i], widths=w, n_tail=(259, 97, 5)[i % 3])
                  for i, w in enumerate(CHAIN_WIDTHS)]
               + [dict(id=4200 + i, tier="bound", B=B, M=M, S=S, C=_CHAIN_C[i], N=GROUPED_N[i % 3], radius=(0.2, 0.4)[i % 2],
                       normalize=i % 2 == 0, widths=w)
                  for i, (w, (B, M, S)) in enumerate(zip(CHAIN_WIDTHS, (GROUPED_BMS * 2)[1:]))]
               + [dict(id=4300 + i, tier="bound", B=B, M=M, S=S, C=_CHAIN_C[(i + 3) % 6], N=GROUPED_N[i % 3], radius=(0.4, 0.2)[i % 2],
                       normalize=i % 2 == 1, widths=w, n_tail=(5, 259, 97)[i % 3])
                  for i, (w, (B, M, S)) in enumerate(zip(CHAIN_WIDTHS, (GROUPED_BMS * 2)[2:]))])


def case_id(c):
    """the case number, its shape, and one letter per option: r(elu) a(ffine) b(ias) x (NaN behind the rows) w (NaN behind the
    weight rows) t(ail bias)"""
    skip = ("id", "affine", "bias", "ldx_gap", "ldw_gap", "relu", "N", "tail_bias", "tier")
    flags = "".join(l for f, l in (("relu", "r"), ("affine", "a"), ("bias", "b"), ("ldx_gap", "x"), ("ldw_gap", "w"),
                                   ("tail_bias", "t")) if c.get(f))
    shape = "-".join("%s%s" % (k, "x".join(map(str, v)) if isinstance(v, tuple) else v) for k, v in c.items() if k not in skip)
    return "%d-%s-%s%s" % (c["id"], c["tier"], shape, "-" + flags if flags else "")
