"""The beam-search step of include/bqhip_beam.h restated in numpy, and a whole decode over a model-free logits oracle
(tests/test_beam_device_cpu.py, tests/test_beam_device_gpu.py; the cases are in tests/beam_cases.py).

  candidate score   fp64 log-softmax rounded to fp32, eos -> -inf while cur_len < min_length, then ONE fp32 add of beam_score
  the order         score descending, NaN above every number, -0 == +0, equal scores by ascending flat index r_local V + v
  the heaps         generation.BeamHypotheses restated on Python floats (doubles), lenpow[n] = n ** length_penalty by Python
  state             beam_score f32 (S), tokens i32 (S, max_length), anc i32 (Lmax, S), done (B), heaps, cur_len

Every decision the step takes records its MARGIN in fp64 (log-probability units) when a list is passed: the gaps between
adjacent candidates among ranks 0 .. 2 nb, |score - worst_score| of every add to a full heap, the gap between the two lowest
entries when one is evicted, and |worst_score - best / lenpow| of every is_done on a full heap.  A case whose margins are all
>= 1e-4 is decided the same way by any fp32 log-softmax.

The oracle: logits(position, last token, sample) = A[position, sample] + C[last token % 64], one fp32 add of two seeded fp32
tables (the eos bias is folded into A), so numpy, CPU torch and a device compute the same bits."""
import numpy as np


class Heap(object):
    def __init__(self, nb, lenpow, early_stopping):
        self.nb, self.lenpow, self.early = nb, lenpow, early_stopping
        self.beams = []          # (score, tokens, sum_logprobs fp32) in list order
        self.worst = 1e9

    def add(self, toks, s32, margins=None):
        score = float(s32) / self.lenpow[len(toks)]
        if margins is not None and len(self.beams) >= self.nb:
            margins.append(("add", abs(score - self.worst)))
        if len(self.beams) < self.nb or score > self.worst:
            self.beams.append((score, list(toks), np.float32(s32)))
            if len(self.beams) > self.nb:
                ranked = sorted((s, i) for i, (s, _, _) in enumerate(self.beams))
                if margins is not None:
                    margins.append(("evict", ranked[1][0] - ranked[0][0]))
                del self.beams[ranked[0][1]]
                self.worst = ranked[1][0]
            else:
                self.worst = min(score, self.worst)

    def is_done(self, best32, cur_len, margins=None):
        if len(self.beams) < self.nb:
            return False
        if self.early:
            return True
        rhs = float(best32) / self.lenpow[cur_len]
        if margins is not None:
            # the rank-0 candidate itself, added in this step as the heap's lowest entry, is the SAME quotient on both sides:
            # equal by construction on every route, not a near-tie
            low = min(self.beams, key=lambda e: e[0])
            same = low[0] == rhs and len(low[1]) == cur_len and float(low[2]) == float(best32)
            if not same:
                margins.append(("done", abs(self.worst - rhs)))
        return self.worst >= rhs


def lenpow_table(max_length, length_penalty):
    return [1.0] + [float(n ** length_penalty) for n in range(1, max_length + 1)]


def new_state(p, prompt=1, Lmax=None):
    B, nb, S = p["B"], p["nb"], p["B"] * p["nb"]
    Lmax = p["max_length"] if Lmax is None else Lmax
    bs = np.zeros((B, nb), np.float32)
    bs[:, 1:] = -1e9
    tokens = np.zeros((S, p["max_length"]), np.int32)
    tokens[:, 0] = prompt
    lp = lenpow_table(p["max_length"], p["length_penalty"])
    return dict(beam_score=bs.reshape(-1), tokens=tokens, anc=np.tile(np.arange(S, dtype=np.int32), (Lmax, 1)),
                done=np.zeros(B, bool), heaps=[Heap(nb, lp, p["early_stopping"]) for _ in range(B)], cur_len=1,
                ids=tokens[:, 0].astype(np.int64).copy(), lenpow=lp)


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        m = x.max(axis=-1, keepdims=True)
        return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def candidate_scores(logits, beam_score, cur_len, p):
    """(fp32 scores (S, V) as the step ranks them, the same in fp64 without the two roundings)"""
    lsm = log_softmax64(logits)
    if cur_len < p["min_length"]:
        lsm[:, p["eos"]] = -np.inf
    with np.errstate(all="ignore"):
        s32 = beam_score.astype(np.float32)[:, None] + lsm.astype(np.float32)
        s64 = beam_score.astype(np.float64)[:, None] + lsm
    return s32, s64


def ranked(flat_scores, n):
    """the first n flat indices of THE ORDER"""
    s = np.asarray(flat_scores, np.float32)
    nan = np.isnan(s)
    with np.errstate(all="ignore"):
        neg = np.where(nan, 0.0, -s.astype(np.float64))
    if s.size > 4 * n:      # prefilter: everything that can reach the first n (ties at the threshold included)
        key = np.where(nan, -np.inf, neg)
        thr = np.partition(key, n - 1)[n - 1]
        keep = np.nonzero(key <= thr)[0]
    else:
        keep = np.arange(s.size)
    o = np.lexsort((keep, neg[keep], ~nan[keep]))
    return keep[o][:n]


def step(st, logits, p, margins=None):
    """one iteration on the state, in place; returns what a device step exposes: top_index / top_score (B, 2 nb), src (S)"""
    B, nb, V, eos, pad = p["B"], p["nb"], p["V"], p["eos"], p["pad"]
    K2, cur_len = 2 * nb, st["cur_len"]
    assert 1 <= cur_len < p["max_length"]
    s32, s64 = candidate_scores(logits, st["beam_score"], cur_len, p)
    top_index, top_score = np.zeros((B, K2), np.int32), np.zeros((B, K2), np.float32)
    src = np.arange(B * nb, dtype=np.int32)
    nxt_score, nxt_tok = np.zeros(B * nb, np.float32), np.full(B * nb, pad, np.int64)
    ignored_eos = 0
    for b in range(B):
        rows = slice(b * nb, (b + 1) * nb)
        f32, f64 = s32[rows].reshape(-1), s64[rows].reshape(-1)
        order = ranked(f32, min(K2 + 1, f32.size))
        top_index[b], top_score[b] = order[:K2], f32[order[:K2]]
        if st["done"][b]:
            continue
        if margins is not None:
            with np.errstate(all="ignore"):
                gaps = -np.diff(f64[order])
            margins.extend(("rank", float(g)) for g in gaps if not np.isnan(g))
        n_open = 0
        for j, flat in enumerate(order[:K2]):
            beam, tok = int(flat) // V, int(flat) % V
            if tok == eos:
                if j < nb:
                    st["heaps"][b].add(st["tokens"][b * nb + beam, :cur_len].tolist(), f32[flat], margins)
                else:
                    ignored_eos += 1                     # an eos candidate at rank >= nb is dropped
            elif n_open < nb:
                i = b * nb + n_open
                src[i], nxt_score[i], nxt_tok[i] = b * nb + beam, f32[flat], tok
                n_open += 1
        assert n_open == nb
        st["done"][b] = st["heaps"][b].is_done(f32[order[0]], cur_len, margins)
        if st["done"][b]:
            src[rows], nxt_score[rows], nxt_tok[rows] = np.arange(b * nb, (b + 1) * nb), 0.0, pad
    st["tokens"][:, :cur_len] = st["tokens"][src, :cur_len]
    st["tokens"][:, cur_len] = nxt_tok
    st["anc"][:cur_len] = st["anc"][:cur_len][:, src]
    if cur_len < st["anc"].shape[0]:
        st["anc"][cur_len] = np.arange(B * nb)
    st["beam_score"], st["ids"], st["cur_len"] = nxt_score, nxt_tok.copy(), cur_len + 1
    return dict(top_index=top_index, top_score=top_score, src=src, not_done=int((~st["done"]).sum()),
                ignored_eos=ignored_eos)


def finalize(st, p):
    """the tail of generation.beam_search -> (sequences (B, sent_max) int64, scores (B,) f32)"""
    B, nb, cur_len = p["B"], p["nb"], st["cur_len"]
    best, best_scores = [], []
    for b in range(B):
        h = st["heaps"][b]
        if not st["done"][b]:
            for k in range(nb):
                h.add(st["tokens"][b * nb + k, :cur_len].tolist(), st["beam_score"][b * nb + k])
        score, hyp, _ = sorted(h.beams, key=lambda x: x[0])[-1]
        best.append(hyp)
        best_scores.append(score)
    sent_max = min(max(len(h) for h in best) + 1, p["max_length"])
    out = np.full((B, sent_max), p["pad"], np.int64)
    for b, h in enumerate(best):
        out[b, :len(h)] = h
        if len(h) < p["max_length"]:
            out[b, len(h)] = p["eos"]
    return out, np.asarray(best_scores, np.float32)


# ---- the logits oracle ---------------------------------------------------------------------------------------------------
def make_oracle(p):
    rng = np.random.default_rng(p["seed"])
    A = (rng.standard_normal((p["max_length"], p["B"], p["V"])) * p.get("scale", 2.0)).astype(np.float32)
    C = (rng.standard_normal((64, p["V"])) * p.get("scale", 2.0)).astype(np.float32)
    A[:, :, p["eos"]] += np.float32(p.get("eos_bias", 2.0))
    A[:, :, p["pad"]] -= np.float32(8.0)                     # the search never prefers padding
    return dict(A=A, C=C)


def oracle_logits(orc, pos, last_tokens, nb):
    S = len(last_tokens)
    return orc["A"][pos, np.arange(S) // nb] + orc["C"][np.asarray(last_tokens) % 64]


def decode(p, extra_steps=0, margins=None, orc=None, records=None):
    """a whole decode on the oracle; extra_steps more iterations after every sample is done (None: run to max_length)"""
    orc = make_oracle(p) if orc is None else orc
    st = new_state(p)
    extra = 0
    while True:
        r = step(st, oracle_logits(orc, st["cur_len"] - 1, st["ids"], p["nb"]), p, margins)
        if records is not None:
            records.append(r)
        if st["cur_len"] >= p["max_length"]:
            break
        if st["done"].all():
            if extra_steps is not None and extra >= extra_steps:
                break
            extra += 1
    return finalize(st, p) + (st,)


# ---- the error bound of the candidate scores -----------------------------------------------------------------------------
def emu_scores(logits, beam_score, cur_len, p, threads=512, vec=4, head=0):
    """the row kernel's own fp32 arithmetic and summation order (csrc/beam.hip beam_rows_kernel): a thread adds exp(x - max)
    over its head element, its 16-byte vectors (vector i belongs to thread i % threads) and its tail element, in that order;
    a wave adds its 64 lanes by a butterfly (offsets 32 .. 1); the waves' sums are added in wave order"""
    x = np.asarray(logits, np.float32)
    S, V = x.shape
    out = np.empty((S, V), np.float32)
    owner = np.empty(V, np.int64)
    nvec = (V - head) // vec
    owner[:head] = np.arange(head)
    owner[head:head + nvec * vec] = np.repeat(np.arange(nvec) % threads, vec)
    owner[head + nvec * vec:] = np.arange(V - head - nvec * vec)
    with np.errstate(all="ignore"):
        for r in range(S):
            m = np.float32(np.max(x[r]))
            e = np.exp(x[r] - m, dtype=np.float32)
            part = np.zeros(threads, np.float32)
            # a thread's elements in index order: head < vectors (ascending i) < tail
            for v in range(V):
                part[owner[v]] = np.float32(part[owner[v]] + e[v])
            w = part.reshape(threads // 64, 64).copy()
            for o in (32, 16, 8, 4, 2, 1):
                w = (w + w[:, np.arange(64) ^ o]).astype(np.float32)
            tot = w[0, 0]
            for k in range(1, threads // 64):
                tot = np.float32(tot + w[k, 0])
            lse = np.float32(np.log(tot, dtype=np.float32))
            lp = ((x[r] - m).astype(np.float32) - lse).astype(np.float32)
            if cur_len < p["min_length"]:
                lp[p["eos"]] = -np.inf
            out[r] = np.float32(beam_score[r]) + lp
    return out


def cpu32_scores(logits, beam_score, cur_len, p):
    """torch's CPU fp32 log_softmax plus the add: what generation.beam_search ranks"""
    import torch
    s = torch.log_softmax(torch.from_numpy(np.asarray(logits, np.float32)), dim=-1)
    if cur_len < p["min_length"]:
        s[:, p["eos"]] = -float("inf")
    return (s + torch.from_numpy(np.asarray(beam_score, np.float32))[:, None]).numpy()


def score_errors(got, logits, beam_score, cur_len, p, index=None):
    """(errors of `got` against fp64 at `index` (all elements when None), E32, ULP): E32 the largest error of the CPU fp32 scores
    and ULP one fp32 ulp of the largest magnitude, both over the finite scores of beams that are not closed (|beam_score| < 1e8)"""
    _, s64 = candidate_scores(logits, beam_score, cur_len, p)
    live = np.isfinite(s64) & (np.abs(np.asarray(beam_score, np.float64)) < 1e8)[:, None]
    c32 = cpu32_scores(logits, beam_score, cur_len, p).astype(np.float64)
    with np.errstate(all="ignore"):
        e32 = float(np.abs(c32 - s64)[live].max())
        ulp = float(np.spacing(np.float32(np.abs(s64[live]).max())))
        err = np.abs(np.asarray(got, np.float64) - (s64 if index is None else s64[index]))
    return err, e32, ulp
