"""Every kernel route of the MFMA bf16 GEMM family (bq_gemm_bf16 through _ext.gemm_grouped, bq_wgrad_rows_bf16) held to EXACT
integer results and to the per-element fp64 bound of tests/gemm_ref.py: one wrong, missing or doubled product anywhere fails,
where the whole-tensor norms of tests/test_gemm_gpu.py accept it.  Every case

  * builds its operands as strided views inside NaN buffers (ld wider than the row, NaN slack rows before and behind), with a
    large finite integer where the contract makes the partner zero (contraction rows of P beyond its buffer, Kc longer than Q's rows),
  * writes into a NaN-filled buffer wider and longer than the output and requires everything outside the logical output to
    still be NaN,
  * runs once under torch.profiler and requires the launched GEMM kernel ids to equal gemm_ref.routes(...),
  * is run with small-integer operands (exact tier: == on every output) and with real-valued operands that have a spiked row
    and column (bound tier: |err| <= tol on every output).

At the end every id of gemm_ref.ROUTE_TABLE must have been seen.  The battery runs in a child process under a time limit (a
fault ends the child and the test reports its log; nothing is retried).

    python tests/test_gemm_bound_gpu.py OUT.pt   runs the battery in this process (the test's child)

Battery on an MI355X (elements held, seconds, largest |err| / bound per route): see profiles/gemm_bound.md.
"""
import functools
import math
import os
import subprocess
import sys
import time

import pytest
import torch

import gemm_ref as R
from attn_ref import _Checker
from gemm_ref import (BACKGROUND, EPI_ADD, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_NONE, OUT_F32, P_XC, Q_XC, ROUTE_TABLE)
from load_util import _repeat_under_load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

NAN = math.nan
BIG = 64.0          # the finite poison: an integer, so that the exact tier stays exact if it is multiplied by a zero
MAP_CASES = [(16, 1025, 20, 768, 1536), (3, 130, 7, 256, 512), (2, 64, 64, 128, 256), (5, 20, 300, 192, 320)]
DW = P_XC | Q_XC | OUT_F32
BATTERY_LIMIT = 60    # seconds: the child took 18.4 s in its first run on an MI355X (15.7 s of it in the battery), times 3


def profiled(fn):
    """fn() once under torch.profiler; returns (fn's result, GEMM kernel ids, number of device kernels seen)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type.name != "CPU"]
    return res, R.kernel_ids(names), len(names)


@functools.lru_cache(maxsize=12)
def _dev_operands(Ni, Nj, Kc, exact, tag, dev):
    return tuple(t.to(dev) for t in R.operands(Ni, Nj, Kc, exact, tag))


def _framed(X, dev, pad=8, fill=NAN, slack=1):
    """X (rows, cols) as a view inside a buffer with `pad` gap columns and `slack` rows before and behind, all `fill`"""
    r, c = X.shape
    buf = torch.full((r + 2 * slack, c + pad), fill, dtype=X.dtype, device=dev)
    v = buf[slack:slack + r, :c]
    v.copy_(X)
    return buf, v


def _outside_is_nan(buf, view):
    """every element of buf outside the rows / columns of `view` (a 2-D view made by _framed) is still NaN, none inside"""
    r, c = view.shape
    inner = buf[1:1 + r, :c]
    n_nan = int(torch.isnan(buf).sum())
    return n_nan == buf.numel() - r * c and not bool(torch.isnan(inner).any())


class Battery:
    def __init__(self, dev):
        from bridgeqa_amd import _ext
        self.ext, self.dev = _ext, dev
        self.cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.chk = _Checker()
        self.seen = set()
        self.log = []
        self.exact_checked = 0
        assert _ext._lib.bq_gemm_max_problems() == R.MAX_PROBLEMS

    def fail(self, msg):
        self.chk.failures.append(msg)

    def expect(self, name, want, got, ndev):
        self.seen |= got
        if ndev == 0:
            self.fail("%s: the profiler reported no device kernels at all -- route coverage cannot be proven" % name)
        elif got != want:
            self.fail("%s: launched %s, expected %s" % (name, sorted(got), sorted(want)))

    def exact(self, name, out, want):
        """exact tier: == on every value; the failing indices name the tile (j // 64, i // 64) and the 32-row wave"""
        bad = R.mismatches(out, want)
        self.exact_checked += want.numel()
        if bad.shape[0]:
            idx = tuple(int(v) for v in bad[0])
            self.fail("%s: EXACT tier: %d of %d outputs differ, first at %s (64-tile %s): out %r expected %r" % (
                name, bad.shape[0], want.numel(), idx, tuple(v // 64 for v in idx), float(out[idx]), float(want[idx])))

    # -- one gemm_grouped call, both tiers ------------------------------------------------------------------------------------
    def gemm(self, name, probs, flags=0, epi=EPI_NONE, tile=None, det=False, streamk=0, route=None, tiers=(True, False)):
        """probs: dicts with Ni, Nj, Kc and optionally bias ('f32' / 'bf16'), colsum, ksplit, accum, p_rows (contraction rows of
        a contraction-major P that exist; the rest lie beyond p_bytes), q_cols (columns of a K-contiguous Q row that exist:
        the row runs into the next one, P's rows beyond are zero), p_wide (rows of a K-contiguous P that exist: Ni is wider)"""
        ext, dev = self.ext, self.dev
        pxc, qxc, f32 = bool(flags & P_XC), bool(flags & Q_XC), bool(flags & OUT_F32)
        wgrad = pxc and qxc and f32
        odt = torch.float32 if f32 else torch.bfloat16
        want_ids = R.routes([dict(p, colsum=bool(p.get("colsum"))) for p in probs], flags, epi, tile, self.cus, det, streamk)
        rt = route or "+".join(sorted(want_ids))
        for exact in tiers:
            built = []
            for k, p in enumerate(probs):
                Ni, Nj, Kc = p["Ni"], p["Nj"], p["Kc"]
                P, Q, bias, aux = _dev_operands(Ni, Nj, Kc, exact, p.get("tag", 0), dev)
                d = {}
                if "p_rows" in p:       # contraction-major P whose rows [p_rows, Kc) do not exist: zeros by the bounds check
                    P = P.clone()
                    P[:, p["p_rows"]:] = 0
                    Q = Q.clone()
                    Q[:, p["p_rows"]:] = BIG
                    pbuf, pv = _framed(P[:, :p["p_rows"]].t().contiguous(), dev)
                    d["p_bytes"] = p["p_rows"] * pv.stride(0) * 2
                    d["Kc"] = Kc
                elif "p_wide" in p:     # K-contiguous P with fewer rows than the output has columns
                    P = P.clone()
                    P[p["p_wide"]:] = 0
                    pbuf, pv = _framed(P[:p["p_wide"]], dev)
                    d["p_bytes"] = p["p_wide"] * pv.stride(0) * 2
                    d["Ni"] = Ni
                elif "q_cols" in p:     # the rows of P beyond q_cols are zero; Q's rows are q_cols long and contiguous
                    P = P.clone()
                    P[:, p["q_cols"]:] = 0
                    pbuf, pv = _framed(P.t().contiguous() if pxc else P, dev)
                else:
                    pbuf, pv = _framed(P.t().contiguous() if pxc else P, dev)
                if "q_cols" in p:
                    Q = Q.clone()
                    Q[:, p["q_cols"]:] = 0
                    qv = Q[:, :p["q_cols"]].contiguous()
                    d["q_bytes"] = qv.numel() * 2
                    d["Kc"] = Kc
                else:
                    _, qv = _framed(Q.t().contiguous() if qxc else Q, dev)
                base = None
                if p.get("accum"):
                    base = R.int_tensor((Nj, Ni), -5, 5, "base").to(dev).to(odt)
                elif p.get("ksplit", 1) > 1:
                    base = torch.zeros(Nj, Ni, dtype=odt, device=dev)
                obuf, ov = _framed(base if base is not None else torch.zeros(Nj, Ni, dtype=odt, device=dev), dev,
                                   pad=8 if not f32 else 4)
                if base is None:
                    ov.fill_(NAN)       # (a plain store must overwrite every logical element)
                d.update(P=pv, Q=qv, out=ov)
                use_bias = epi in (EPI_BIAS, EPI_BIAS_GELU)
                if use_bias:
                    d["bias"] = bias.to(torch.bfloat16) if p.get("bias") == "bf16" else bias
                    bias = d["bias"].float()
                if epi in (EPI_DGELU, EPI_ADD):
                    _, d["aux"] = _framed(aux, dev)
                if epi == EPI_BIAS_GELU:
                    d["o2buf"], d["out2"] = _framed(torch.full((Nj, Ni), NAN, dtype=odt, device=dev), dev)
                cs0 = None
                if p.get("colsum"):
                    n_cs = Nj if wgrad else Ni
                    cs0 = 2.0 if (p.get("accum") or not wgrad) else (0.0 if p.get("ksplit", 1) > 1 else NAN)
                    csb = torch.full((n_cs + 16,), NAN, device=dev)
                    csb[8:8 + n_cs] = cs0
                    d["csbuf"], d["colsum"] = csb, csb[8:8 + n_cs]
                for key in ("ksplit", "accum"):
                    if key in p:
                        d[key] = p[key]
                built.append((d, P, Q, bias if use_bias else None, aux, base, obuf, cs0))
            call = [{k_: v for k_, v in b[0].items() if k_ not in ("o2buf", "csbuf")} for b in built]

            def run():
                prev_det = self._set_det(det)
                try:
                    self._streamk(streamk)
                    ext.gemm_grouped(call, flags, epi, tile)
                finally:
                    self._streamk(0)
                    self._set_det(prev_det)
            try:
                if exact:
                    _, got, ndev = profiled(run)
                    self.expect(name, want_ids, got, ndev)
                    self.log.append((name, sorted(got)))
                else:
                    run()
                    torch.cuda.synchronize()
            except RuntimeError as e:       # (a refused launch: the case is reported, the battery goes on)
                self.fail("%s: the launch raised: %s" % (name, e))
                break
            for k, (d, P, Q, bias, aux, base, obuf, cs0) in enumerate(built):
                nm = "%s[%d].%s" % (name, k, "int" if exact else "real")
                out = d["out"]
                if not _outside_is_nan(obuf, out):
                    self.fail("%s: a store left the logical output (a NaN guard element was overwritten) or missed an element" % nm)
                    continue
                lin = epi != EPI_DGELU
                aux_l = aux if epi in (EPI_ADD, EPI_DGELU) else None
                if exact and lin:
                    want = R.expected(P, Q, bias, aux_l if epi == EPI_ADD else None, f32=True)
                    if base is not None:
                        want = want + base.double()
                    self.exact(nm, out, want if f32 else R.rne_bf16(want))
                if not exact or not lin:
                    r, tol = R.bound(P, Q, bias, aux_l, epi, f32)
                    if base is not None:
                        r = r + base.double()
                        tol = tol + R.U * r.abs()
                    self.chk(nm, out, r, tol, route=rt)
                if epi == EPI_BIAS_GELU:
                    if not _outside_is_nan(d["o2buf"], d["out2"]):
                        self.fail("%s: out2 left its logical extent" % nm)
                    r, tol = R.gelu_bound(out)
                    self.chk(nm + ".gelu", d["out2"], r, tol, route=rt + ".gelu")
                if "colsum" in d:
                    cs, csb = d["colsum"], d["csbuf"]
                    if not (torch.isnan(csb[:8]).all() and torch.isnan(csb[8 + cs.numel():]).all()):
                        self.fail("%s: colsum wrote outside its vector" % nm)
                    start = 0.0 if (cs0 is None or cs0 != cs0) else cs0
                    if wgrad:
                        r, tol = R.qsum_bound(Q)
                    else:
                        r, tol = R.colsum_bound(out)
                    r = r + start
                    if exact and lin:
                        self.exact(nm + ".colsum", cs, r)
                    else:
                        self.chk(nm + ".colsum", cs, r, tol + R.U * r.abs() * 2, route=rt + ".colsum")
            del built, call
        return want_ids

    def _set_det(self, on):
        import bridgeqa_amd
        return bridgeqa_amd.set_deterministic(bool(on))

    def _streamk(self, mode):
        self.ext.streamk_enable(bool(mode & 1))
        self.ext.streamk256_enable(bool(mode & 2))

    def refused(self, name, probs, flags, epi, tile, det=False):
        """return code only: the launch must raise"""
        dev = self.dev
        f32 = bool(flags & OUT_F32)
        call = []
        for p in probs:
            P = torch.zeros((p["Kc"], p["Ni"]) if flags & P_XC else (p["Ni"], p["Kc"]), dtype=torch.bfloat16, device=dev)
            Q = torch.zeros((p["Kc"], p["Nj"]) if flags & Q_XC else (p["Nj"], p["Kc"]), dtype=torch.bfloat16, device=dev)
            d = dict(P=P, Q=Q, out=torch.zeros(p["Nj"], p["Ni"], dtype=torch.float32 if f32 else torch.bfloat16, device=dev))
            if p.get("colsum"):
                d["colsum"] = torch.zeros(p["Nj"] if flags & Q_XC else p["Ni"], device=dev)
            if epi in (EPI_DGELU, EPI_ADD):
                d["aux"] = torch.zeros_like(d["out"])
            for key in ("ksplit", "accum"):
                if key in p:
                    d[key] = p[key]
            call.append(d)
        prev = self._set_det(det)
        try:
            self.ext.gemm_grouped(call, flags, epi, tile)
            torch.cuda.synchronize()
            self.fail("%s: the launch was accepted, it must be refused" % name)
        except RuntimeError:
            pass
        finally:
            self._set_det(prev)

    # -- the cases ----------------------------------------------------------------------------------------------------------------
    def instantiations(self):
        """every (form, epilogue, tile, K-step) instantiation on small ragged problems; 13 and 15 K tiles under the 2- and
        4-tile steps, Kc = 64 / 128 under the 1-tile step"""
        forms = [(0, (EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_DGELU, EPI_ADD)), (P_XC, (EPI_NONE, EPI_DGELU, EPI_ADD))]
        for fl, epis in forms:
            for e in epis:
                tag = "f%d.e%d" % (fl, e)
                for Kc in (64, 128, 832, 960):
                    self.gemm("inst.%s.t64.K%d" % (tag, Kc), [dict(Ni=72, Nj=257, Kc=Kc, bias="bf16" if Kc == 128 else "f32")],
                              fl, e, 64)
                    self.gemm("inst.%s.t32.K%d" % (tag, Kc), [dict(Ni=264, Nj=257, Kc=Kc)], fl, e, 32)
                    if Kc >= 128:
                        self.gemm("inst.%s.t128.K%d" % (tag, Kc), [dict(Ni=264, Nj=1000, Kc=Kc)], fl, e, 128)
                    if fl or e not in (EPI_DGELU, EPI_ADD):
                        self.gemm("inst.%s.t256.K%d" % (tag, Kc), [dict(Ni=264, Nj=257, Kc=Kc, bias="bf16")], fl, e, 256)
                for Kc in (832, 960):       # the 2-tile step of the 32-row tile: 513 .. 2048 tiles
                    self.gemm("inst.%s.t32kt2.K%d" % (tag, Kc), [dict(Ni=264, Nj=3300, Kc=Kc)], fl, e, 32)
                if e in (EPI_NONE, EPI_DGELU, EPI_ADD, EPI_BIAS):   # column sums of the bf16 output (not on tile 128)
                    for t in (256, 64, 32):
                        if t == 256 and not fl and e in (EPI_DGELU, EPI_ADD):
                            continue
                        self.gemm("inst.%s.t%d.colsum" % (tag, t), [dict(Ni=264, Nj=1000, Kc=192, colsum=True)], fl, e, t)

    def thresholds(self):
        """both sides of every threshold of the automatic route"""
        for Nj in (1023, 1024):
            self.gemm("thr.rows%d" % Nj, [dict(Ni=256, Nj=Nj, Kc=128)], 0, EPI_BIAS)
        for Ni in (248, 256):
            self.gemm("thr.cols%d" % Ni, [dict(Ni=Ni, Nj=1024, Kc=128)], 0, EPI_BIAS)
        for Nj in (512, 513):
            self.gemm("thr.small%d" % Nj, [dict(Ni=72, Nj=Nj, Kc=128)], 0, EPI_NONE)
        for Kc in (64 * 11, 64 * 12):
            self.gemm("thr.longk%d" % Kc, [dict(Ni=264, Nj=100, Kc=Kc)], 0, EPI_BIAS)
            self.gemm("thr.longk%d.t64" % Kc, [dict(Ni=264, Nj=600, Kc=Kc)], 0, EPI_BIAS)
        for Nj in (16384, 16385):       # 512 / 513 tiles of 64 x 32
            self.gemm("thr.k4tiles%d" % Nj, [dict(Ni=64, Nj=Nj, Kc=768)], 0, EPI_NONE, 32)
        for Nj in (65536, 65537):       # 2048 / 2049
            self.gemm("thr.k2tiles%d" % Nj, [dict(Ni=64, Nj=Nj, Kc=768)], 0, EPI_NONE, 32)
        for Kc in (2240, 2304):
            self.gemm("thr.tile256k%d" % Kc, [dict(Ni=768, Nj=2000, Kc=Kc)], 0, EPI_BIAS)
            self.gemm("thr.tile256k%d.dx" % Kc, [dict(Ni=768, Nj=2000, Kc=Kc)], P_XC, EPI_NONE)   # (P_XC: never promoted)
        for Kc in (64, 128):
            self.gemm("thr.midk%d" % Kc, [dict(Ni=256, Nj=1024, Kc=Kc)], 0, EPI_NONE)

    def product_shapes(self):
        """the automatic route of every product call shape, and each forced onto every other tile class that accepts it"""
        M = 16400
        for t in (None, 256, 128, 64, 32):
            s = ".t%s" % t
            for N, K, e in ((768, 768, EPI_BIAS), (2304, 768, EPI_BIAS), (3072, 768, EPI_BIAS_GELU), (768, 3072, EPI_BIAS)):
                self.gemm("vit.fwd.%dx%d%s" % (N, K, s), [dict(Ni=N, Nj=M, Kc=K)], 0, e, t)
            for Ni, Kc, e in ((768, 2304, EPI_NONE), (768, 768, EPI_ADD), (3072, 768, EPI_ADD), (768, 3072, EPI_DGELU)):
                self.gemm("vit.dx.%dx%d%s" % (Ni, Kc, s), [dict(Ni=Ni, Nj=M, Kc=Kc)], P_XC, e, t)
            if t != 128:
                self.gemm("vit.dx.dgelu.colsum%s" % s, [dict(Ni=3072, Nj=M, Kc=768, colsum=True)], P_XC, EPI_DGELU, t)
        for t in (None, 128, 64):
            for Ni, Nj in ((768, 768), (768, 2304), (768, 3072), (3072, 768)):
                self.gemm("vit.dw.%dx%d.t%s" % (Nj, Ni, t), [dict(Ni=Ni, Nj=Nj, Kc=M, colsum=True)], DW, EPI_NONE, t)
        for Mt in (80, 320, 640):       # the text side: forward, dX on the transposed weight copy with each epilogue, dW
            for t in (None, 256, 128, 64, 32):
                s = ".M%d.t%s" % (Mt, t)
                self.gemm("text.fwd" + s, [dict(Ni=768, Nj=Mt, Kc=768)], 0, EPI_BIAS, t)
                self.gemm("text.fc1" + s, [dict(Ni=3072, Nj=Mt, Kc=768)], 0, EPI_BIAS_GELU, t)
                self.gemm("text.fc2" + s, [dict(Ni=768, Nj=Mt, Kc=3072)], 0, EPI_BIAS, t)
                if t != 256:
                    self.gemm("text.dxT.add" + s, [dict(Ni=768, Nj=Mt, Kc=3072)], 0, EPI_ADD, t)
                    self.gemm("text.dxT.dgelu" + s, [dict(Ni=3072, Nj=Mt, Kc=768)], 0, EPI_DGELU, t)
                self.gemm("text.dxT.none" + s, [dict(Ni=768, Nj=Mt, Kc=2304)], 0, EPI_NONE, t)
                self.gemm("text.dx" + s, [dict(Ni=768, Nj=Mt, Kc=768)], P_XC, EPI_NONE, t)
            for t in (None, 256, 64) + ((128,) if Mt >= 128 else ()):
                self.gemm("text.dw.M%d.t%s" % (Mt, t), [dict(Ni=768, Nj=768, Kc=Mt, colsum=True)], DW, EPI_NONE, t)
        # the grouped decoder K/V launch: several sources through their own weights in one launch
        self.gemm("group.kv", [dict(Ni=1536, Nj=16400, Kc=768), dict(Ni=1536, Nj=320, Kc=768, tag=1),
                               dict(Ni=1536, Nj=80, Kc=768, tag=2)], 0, EPI_BIAS)

    def ragged(self):
        for Nj in (1, 7, 257, 1000, 16400):
            for Ni in (8, 72, 264):
                for t in (None, 256, 128, 64, 32):
                    self.gemm("ragged.%dx%d.t%s" % (Nj, Ni, t), [dict(Ni=Ni, Nj=Nj, Kc=192, bias="bf16" if Ni == 72 else "f32")],
                              0, EPI_BIAS, t, route="ragged")
        for M in (20, 63, 64, 65, 1000, 16400):      # weight-gradient contractions: the ragged last K tile
            for t in (256, 64) + ((128,) if M >= 128 else ()):
                self.gemm("dw.M%d.t%d" % (M, t), [dict(Ni=264, Nj=136, Kc=M, colsum=True)], DW, EPI_NONE, t)
        for t in (256, 128, 64, 32):                 # Ni wider than P (a padded vocabulary), p_bytes
            self.gemm("p_wide.t%d" % t, [dict(Ni=328, Nj=257, Kc=192, p_wide=250)], 0, EPI_BIAS, t)
        # Kc longer than the operand: the LM head's dH (contraction rows of P beyond its buffer, a cut contraction) and
        # rows_linear_f32's dX (rows of Q shorter than Kc, running into the next row, against zero rows of P)
        for t in (64, 32):
            for ks in (1, 5):
                self.gemm("kc_long.p_rows.t%d.ks%d" % (t, ks), [dict(Ni=264, Nj=160, Kc=1024, p_rows=1001, ksplit=ks)],
                          P_XC | OUT_F32, EPI_NONE, t)
        for t in (None, 256, 128, 64, 32):
            self.gemm("kc_long.q_cols.t%s" % t, [dict(Ni=264, Nj=1100, Kc=192, q_cols=136)], P_XC, EPI_NONE, t)

    def fp32_outputs(self):
        """fp32 outputs with cut contractions, accum and column sums, atomic and deterministic (the deterministic forms must
        reach the _det kernels and the fold and be bit-equal to the exact expectation like the atomic ones)"""
        for det in (False, True):
            s = ".det" if det else ""
            for ks in (1, 5, 8, 48):        # 9000 rows = 141 K tiles: 5, 8 and 48 do not divide them
                self.gemm("f32.dw.ks%d%s" % (ks, s), [dict(Ni=136, Nj=264, Kc=9000, ksplit=ks)], DW, EPI_NONE, 64, det=det)
                if not (det and ks > 1):
                    self.gemm("f32.dw.ks%d.colsum%s" % (ks, s), [dict(Ni=136, Nj=264, Kc=9000, ksplit=ks, colsum=True)], DW,
                              EPI_NONE, 64, det=det)
                    self.gemm("f32.dw.ks%d.accum%s" % (ks, s), [dict(Ni=136, Nj=264, Kc=9000, ksplit=ks, colsum=True, accum=True)],
                              DW, EPI_NONE, 64, det=det)
            for t in (64, 32):
                for e in (EPI_NONE, EPI_BIAS):
                    for ks in ((1, 5) if e == EPI_NONE else (1,)):
                        self.gemm("f32.fwd.e%d.t%d.ks%d%s" % (e, t, ks, s), [dict(Ni=264, Nj=257, Kc=832, ksplit=ks)], OUT_F32, e, t,
                                  det=det)
                self.gemm("f32.fwd.accum.t%d%s" % (t, s), [dict(Ni=264, Nj=257, Kc=128, accum=True)], OUT_F32, EPI_NONE, t, det=det)
                for ks in (1, 8):
                    self.gemm("f32.dx.t%d.ks%d%s" % (t, ks, s), [dict(Ni=264, Nj=257, Kc=1024, ksplit=ks)], P_XC | OUT_F32, EPI_NONE,
                              t, det=det)
            # bf16 column sums in the deterministic mode go through the fixed-order column sum
            self.gemm("colsum.bf16%s" % s, [dict(Ni=264, Nj=1000, Kc=192, colsum=True)], P_XC, EPI_DGELU, 64, det=det)
            self.gemm("det.plain%s" % s, [dict(Ni=768, Nj=2000, Kc=768)], 0, EPI_BIAS, None, det=det)

    def groups(self):
        mixed = [dict(Ni=264, Nj=1000, Kc=192), dict(Ni=768, Nj=129, Kc=768, tag=1), dict(Ni=1536, Nj=4416, Kc=768),
                 dict(Ni=8, Nj=70, Kc=128), dict(Ni=72, Nj=1, Kc=256)]
        for t in (None, 256, 128, 64, 32):
            self.gemm("group.mixed.t%s" % t, mixed, 0, EPI_BIAS, t)
        many = [dict(Ni=64 + 8 * (k % 3), Nj=90 + k, Kc=128, tag=k) for k in range(R.MAX_PROBLEMS + 5)]
        for t in (32, 64, 128):
            self.gemm("group.many.t%d" % t, many, 0, EPI_NONE, t)
        # the first launch of 36 takes the four-K-tile form, the remainder of 5 too: both from the same ids
        self.gemm("group.many.longk", [dict(p, Kc=768) for p in many], 0, EPI_NONE, 32)
        # one member cannot take tile 128 (Kc = 64): the group falls to 256 as a whole
        self.gemm("group.fall256", [dict(Ni=768, Nj=2000, Kc=768), dict(Ni=264, Nj=1100, Kc=64)], 0, EPI_NONE)
        self.gemm("group.dw", [dict(Ni=768, Nj=768, Kc=700), dict(Ni=768, Nj=2304, Kc=1000), dict(Ni=3072, Nj=768, Kc=512),
                               dict(Ni=768, Nj=3072, Kc=999)], DW, EPI_NONE)
        self.gemm("group.dw.t64", [dict(Ni=768, Nj=768, Kc=700), dict(Ni=72, Nj=64, Kc=777, ksplit=3)], DW, EPI_NONE, 64)

    def special(self):
        """BQ_GEMM_BACKGROUND; both stream-K forms (bit-equal to the exact expectation: integer slabs add exactly)"""
        self.gemm("bg.fwd", [dict(Ni=1536, Nj=16400, Kc=768)], BACKGROUND, EPI_BIAS)
        self.gemm("bg.dx.add", [dict(Ni=768, Nj=16400, Kc=1536)], P_XC | BACKGROUND, EPI_ADD)
        self.gemm("bg.dw", [dict(Ni=768, Nj=1536, Kc=16400)], DW | BACKGROUND, EPI_NONE, 128)
        self.gemm("bg.cleared", [dict(Ni=264, Nj=300, Kc=128)], BACKGROUND, EPI_NONE)      # (not tile 128: the flag is dropped)
        for M in (16400, 16384):
            for e in (EPI_NONE, EPI_BIAS, EPI_ADD):
                self.gemm("sk128.M%d.e%d" % (M, e), [dict(Ni=768, Nj=M, Kc=3072)], 0, e, 128, streamk=1)
            for e in (EPI_NONE, EPI_BIAS):
                self.gemm("sk256.M%d.e%d" % (M, e), [dict(Ni=768, Nj=M, Kc=3072)], 0, e, 128, streamk=2)
        self.gemm("sk.both.short", [dict(Ni=768, Nj=16400, Kc=768)], 0, EPI_BIAS, 128, streamk=3)   # (12 K tiles: whole tiles)

    def refusals(self):
        self.refused("refuse.colsum128", [dict(Ni=264, Nj=1000, Kc=192, colsum=True)], P_XC, EPI_NONE, 128)
        self.refused("refuse.accum256", [dict(Ni=264, Nj=136, Kc=400, accum=True)], DW, EPI_NONE, 256)
        self.refused("refuse.accum128", [dict(Ni=264, Nj=136, Kc=400, accum=True)], DW, EPI_NONE, 128)
        self.refused("refuse.ksplit.bf16", [dict(Ni=264, Nj=136, Kc=448, ksplit=2)], 0, EPI_NONE, 64)
        self.refused("refuse.f32.t256", [dict(Ni=264, Nj=136, Kc=448)], OUT_F32, EPI_NONE, 256)
        self.refused("refuse.f32.gelu", [dict(Ni=264, Nj=136, Kc=448)], OUT_F32, EPI_DGELU, 64)
        self.refused("refuse.qxc.t32", [dict(Ni=264, Nj=136, Kc=400)], DW, EPI_NONE, 32)
        self.refused("refuse.k64.t128", [dict(Ni=264, Nj=1100, Kc=64)], 0, EPI_NONE, 128)
        self.refused("refuse.k100", [dict(Ni=64, Nj=64, Kc=100)], 0, EPI_NONE, 64)
        self.refused("refuse.kcontig.add.t256", [dict(Ni=264, Nj=300, Kc=128)], 0, EPI_ADD, 256)
        # (every piece of a cut contraction runs the whole epilogue: a bias would be added ksplit times)
        self.refused("refuse.bias.ksplit", [dict(Ni=264, Nj=257, Kc=832, ksplit=5)], OUT_F32, EPI_BIAS, 64)
        self.refused("refuse.det.ksplit.colsum", [dict(Ni=136, Nj=264, Kc=900, ksplit=3, colsum=True)], DW, EPI_NONE, 64, det=True)

    def maps(self):
        """batched-row maps (q_rpb / o_rpb): two row sources through one weight into ONE (B, R1 + R2, N) tensor, the input
        gradient reading its row range in place, the weight gradient over both sources (the second added with accum); the
        other row range of a mapped output untouched"""
        ext, dev = self.ext, self.dev
        for B, R1, R2, K, N in MAP_CASES:
            for exact in (True, False):
                mk = (lambda shape, lo, hi, sc, *key: (R.int_tensor(shape, lo, hi, *key) if exact
                                                       else R.real_tensor(shape, sc, *key)).to(dev))
                xa, xb, w = mk((B * R1, K), -1, 1, 1.0, "xa"), mk((B * R2, K), -1, 1, 1.0, "xb"), mk((N, K), -2, 2, 0.1, "w")
                bias = mk((N,), -3, 3, 1.0, "b").float()
                kind = "int" if exact else "real"
                for t in (None, 128, 64, 32):
                    # forward: both sources in one launch
                    big = torch.full((B + 2, R1 + R2, N + 8), NAN, dtype=torch.bfloat16, device=dev)
                    inner = big[1:-1, :, :N]
                    nm = "map.fwd.%dx%d.t%s.%s" % (B, R1, t, kind)
                    pr = [dict(P=w, Q=xa, out=inner[:, :R1], bias=bias), dict(P=w, Q=xb, out=inner[:, R1:], bias=bias)]
                    meta = [dict(Ni=N, Nj=B * R1, Kc=K, map=True), dict(Ni=N, Nj=B * R2, Kc=K, map=True)]
                    _, got, ndev = profiled(lambda: ext.gemm_grouped(pr, 0, EPI_BIAS, t))
                    want_ids = R.routes(meta, 0, EPI_BIAS, t, self.cus)
                    self.expect(nm, want_ids, got, ndev)
                    rt = "map+" + "+".join(sorted(want_ids))
                    if not (torch.isnan(big[0]).all() and torch.isnan(big[-1]).all() and torch.isnan(big[:, :, N:]).all()):
                        self.fail("%s: a store left the mapped output" % nm)
                    for x, o in ((xa, inner[:, :R1]), (xb, inner[:, R1:])):
                        o2 = o.reshape(-1, N)
                        if exact:
                            self.exact(nm, o2, R.expected(w, x, bias))
                        else:
                            self.chk(nm, o2, *R.bound(w, x, bias, None, EPI_BIAS), route=rt)
                    # one source alone: the other row range stays NaN
                    big.fill_(NAN)
                    ext.gemm_grouped(pr[:1], 0, EPI_BIAS, t)
                    if not torch.isnan(inner[:, R1:]).all() or torch.isnan(inner[:, :R1]).any():
                        self.fail("%s: the other row range of a mapped output was written" % nm)
                    # input gradient: Q = a row range of the (B, R1 + R2, N) gradient read in place, ADD epilogue
                    g = mk((B, R1 + R2, N), -1, 1, 1.0, "g")
                    wk = mk((K, N), -2, 2, 0.1, "wk")          # logical P (Ni = K, Kc = N), stored contraction-major as (N, K)
                    aux = mk((B * R1, K), -4, 4, 1.0, "aux")
                    _, ov = _framed(torch.full((B * R1, K), NAN, dtype=torch.bfloat16, device=dev), dev)
                    _, av = _framed(aux, dev)
                    nm = "map.dx.%dx%d.t%s.%s" % (B, R1, t, kind)
                    meta = [dict(Ni=K, Nj=B * R1, Kc=N, map=True)]
                    _, got, ndev = profiled(lambda: ext.gemm_grouped([dict(P=wk.t().contiguous(), Q=g[:, :R1], out=ov, aux=av)],
                                                                      P_XC, EPI_ADD, t))
                    want_ids = R.routes(meta, P_XC, EPI_ADD, t, self.cus)
                    self.expect(nm, want_ids, got, ndev)
                    q = g[:, :R1].reshape(-1, N)
                    if exact:
                        self.exact(nm, ov, R.expected(wk, q, None, aux))
                    else:
                        self.chk(nm, ov, *R.bound(wk, q, None, aux, EPI_ADD), route="map+" + "+".join(sorted(want_ids)))
                # weight gradient over both sources: out (N, K) = g^T x; P = x stored (rows, K) = contraction-major
                g = mk((B, R1 + R2, N), -1, 1, 1.0, "g")
                for t in ([None, 256, 64] if R1 >= 64 else [None, 64]):
                    nm = "map.dw.%dx%d.t%s.%s" % (B, R1, t, kind)
                    obuf, dw = _framed(torch.full((N, K), NAN, device=dev), dev, pad=4)
                    db = torch.full((N,), NAN, device=dev)
                    meta = [dict(Ni=K, Nj=N, Kc=B * R1, map=True, colsum=True)]
                    _, got, ndev = profiled(lambda: ext.gemm_grouped([dict(P=xa, Q=g[:, :R1], out=dw, colsum=db)], DW, EPI_NONE, t))
                    self.expect(nm, R.routes(meta, DW, EPI_NONE, t, self.cus), got, ndev)
                    ext.gemm_grouped([dict(P=xb, Q=g[:, R1:], out=dw, colsum=db, accum=True)], DW, EPI_NONE, 64)
                    if not _outside_is_nan(obuf, dw):
                        self.fail("%s: a store left the logical output" % nm)
                    qa, qb = g[:, :R1].reshape(-1, N).t(), g[:, R1:].reshape(-1, N).t()     # logical Q (Nj = N, Kc = rows)
                    pa, pb = xa.t(), xb.t()
                    if exact:
                        self.exact(nm, dw, R.expected(pa, qa, f32=True) + R.expected(pb, qb, f32=True))
                        self.exact(nm + ".colsum", db, g.double().sum((0, 1)))
                    else:
                        ra, ta = R.bound(pa, qa, f32=True)
                        rb, tb = R.bound(pb, qb, f32=True)
                        self.chk(nm, dw, ra + rb, ta + tb + R.U * (ra + rb).abs(), route="map.dw")
                        r1, t1 = R.qsum_bound(qa)
                        r2, t2 = R.qsum_bound(qb)
                        self.chk(nm + ".colsum", db, r1 + r2, t1 + t2 + R.U * (r1 + r2).abs(), route="map.dw.colsum")

    def wgrad_rows(self):
        """bq_wgrad_rows_bf16: every supported unit combination, contractions 20 .. 16400 rows, an input row stride wider than its
        channels, the padding columns of out zeroed, NaN rows around out untouched"""
        ext, dev = self.ext, self.dev
        Rs = (20, 63, 64, 65, 1000, 16400)
        n = 0
        for ti in range(1, 6):
            for tj in (1, 2, 4):
                Nj = 64 * tj
                Ni = 64 * ti - (56 if ti > 1 else 0)    # ragged last unit: 72, 136, 200, 264 (and 64)
                if not R.wgrad_rows_supported(Ni, Nj):
                    continue
                assert ext.wgrad_rows_ok(Ni, Nj)
                for rows in (Rs[n % 6], Rs[(n + 3) % 6]):
                    for exact in (True, False):
                        P, Q, _, _ = _dev_operands(Ni, Nj, rows, exact, 7, dev)     # logical P (Ni, rows), Q (Nj, rows)
                        _, xv = _framed(P.t().contiguous(), dev, fill=0.0)            # x (rows, Ni), ld = Ni + 8 (zero padding)
                        _, dyv = _framed(Q.t().contiguous(), dev)
                        obuf = torch.full((Nj + 2, Ni + 8), NAN, device=dev)
                        out = obuf[1:-1]
                        nm = "wgrad_rows.%dx%d.R%d.%s" % (ti, tj, rows, "int" if exact else "real")
                        _, got, ndev = profiled(lambda: ext.wgrad_rows(xv, dyv, out, 7 if n % 2 else 0))
                        self.expect(nm, R.wgrad_rows_routes(Ni, Nj), got, ndev)
                        if not (torch.isnan(obuf[0]).all() and torch.isnan(obuf[-1]).all() and (out[:, Ni:] == 0).all()):
                            self.fail("%s: guard rows overwritten or padding columns not zeroed" % nm)
                        if exact:
                            self.exact(nm, out[:, :Ni], R.expected(P, Q, f32=True))
                        else:
                            r, tol = R.bound(P, Q, f32=True)
                            self.chk(nm, out[:, :Ni], r, tol, route="wgrad_rows<%d,%d>" % (ti, tj))
                n += 1
        if ext.wgrad_rows_ok(328, 128) or ext.wgrad_rows_ok(64, 192) or ext.wgrad_rows_ok(256, 256) or ext.wgrad_rows_ok(320, 64):
            self.fail("wgrad_rows_ok accepts a unit combination that has no kernel")


def battery(dev):
    b = Battery(dev)
    t0 = time.time()
    with torch.no_grad():
        for part in (b.instantiations, b.thresholds, b.ragged, b.fp32_outputs, b.groups, b.special, b.refusals, b.maps,
                     b.wgrad_rows, b.product_shapes):
            t1 = time.time()
            part()
            torch.cuda.synchronize()
            print("%-16s %6.1f s, %d failures so far" % (part.__name__, time.time() - t1, len(b.chk.failures)), flush=True)
    return b, time.time() - t0


def test_every_gemm_route_exact_and_within_the_fp64_bound(tmp_path):
    out = str(tmp_path / "gemm_bound.pt")
    t0 = time.time()
    p = subprocess.run(["timeout", "-k", "10", str(BATTERY_LIMIT), sys.executable, os.path.abspath(__file__), out], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    log = p.stdout.decode(errors="replace")
    assert p.returncode == 0, "battery child exited with %d:\n%s" % (p.returncode, log[-6000:])
    r = torch.load(out)
    lines = ["%-60s %.3f" % (k, v) for k, v in sorted(r["ratios"].items())]
    sys.stdout.write("\nGEMM battery: %d outputs held exactly, %d elements held to the bound, %.1f s (child %.1f s); largest "
                     "|err| / bound per route:\n%s\n" % (r["exact"], r["checked"], time.time() - t0, r["seconds"], "\n".join(lines)))
    missing = [k for k in ROUTE_TABLE if k not in r["seen"]]
    assert not missing, "route table kernels never launched: %s" % missing
    assert not r["failures"], "%d failures:\n%s" % (len(r["failures"]), "\n".join(r["failures"][:40]))


# ---- repeatability under load: routes that have no such test in tests/test_gemm_gpu.py ----------------------------------------
def _ops(Ni, Nj, Kc, dev, tag):
    P, Q, bias, aux = R.operands(Ni, Nj, Kc, False, tag)
    return P.to(dev), Q.to(dev), bias.to(dev), aux.to(dev)


def test_small_tile_long_k_forms_repeatable_under_load(dev):
    """the four-K-tile and two-K-tile forms of the 64 x 32 kernel and the two-K-tile form of the 64 x 64 one"""
    from bridgeqa_amd import _ext
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    fns = []
    for Ni, Nj, Kc, tile in ((768, 320, 3072, 32), (264, 3300, 832, 32), (768, 640, 960, 64)):
        P, Q, bias, _ = _ops(Ni, Nj, Kc, dev, 11)
        out = torch.empty(Nj, Ni, dtype=torch.bfloat16, device=dev)

        def f(P=P, Q=Q, bias=bias, out=out, tile=tile):
            _ext.gemm_grouped([dict(P=P, Q=Q, out=out, bias=bias)], 0, EPI_BIAS, tile)
            return (out,)
        assert profiled(f)[1] == R.routes([dict(Ni=Ni, Nj=Nj, Kc=Kc)], 0, EPI_BIAS, tile, cus)
        fns.append(f)
    assert {next(iter(R.routes([dict(Ni=a, Nj=b, Kc=c)], 0, EPI_BIAS, t, cus))) for a, b, c, t in
            ((768, 320, 3072, 32), (264, 3300, 832, 32), (768, 640, 960, 64))} == {
        "gemm64_kernel<32,0,0,1,0,4,3>", "gemm64_kernel<32,0,0,1,0,2,3>", "gemm64_kernel<64,0,0,1,0,2,3>"}
    _repeat_under_load(dev, fns)


def test_row_mapped_256x128_tile_and_det_fold_repeatable_under_load(dev):
    """tile 128 writing row ranges of one (B, R1 + R2, N) tensor; a cut contraction of the deterministic mode (slabs + fold)"""
    import bridgeqa_amd
    from bridgeqa_amd import _ext
    B, R1, R2, K, N = MAP_CASES[0]
    xa, xb, w = R.real_tensor((B * R1, K), 1.0, "xa").to(dev), R.real_tensor((B * R2, K), 1.0, "xb").to(dev), \
        R.real_tensor((N, K), 0.1, "w").to(dev)
    big = torch.empty(B, R1 + R2, N, dtype=torch.bfloat16, device=dev)

    def mapped():
        _ext.gemm_grouped([dict(P=w, Q=xa, out=big[:, :R1]), dict(P=w, Q=xb, out=big[:, R1:])], 0, EPI_NONE, None)
        return (big,)
    assert profiled(mapped)[1] == {"gemm128_kernel<0,0,0,0,16,0>"}
    x, dy = R.real_tensor((9000, 136), 1.0, "x").to(dev), R.real_tensor((9000, 264), 1.0, "dy").to(dev)
    dw = torch.empty(264, 136, device=dev)

    def fold():
        prev = _ext._det()
        bridgeqa_amd.set_deterministic(True)
        try:
            dw.zero_()
            _ext.gemm_grouped([dict(P=x, Q=dy, out=dw, ksplit=8)], DW, EPI_NONE, 64)
        finally:
            bridgeqa_amd.set_deterministic(prev)
        return (dw,)
    assert {"gemm64_kernel_det<64,1,1,0>", "splitk_fold_det_kernel"} <= profiled(fold)[1]
    _repeat_under_load(dev, [mapped, fold])


if __name__ == "__main__":
    b, secs = battery(torch.device("cuda:0"))
    torch.save(dict(failures=b.chk.failures, checked=b.chk.checked, exact=b.exact_checked, ratios=b.chk.ratios,
                    seen=sorted(b.seen), seconds=secs, log=b.log), sys.argv[1])
    print("GEMM battery: %d exact, %d bounded, %d failures, %.1f s" % (b.exact_checked, b.chk.checked, len(b.chk.failures), secs))
    for f in b.chk.failures[:60]:
        print("  " + f)
