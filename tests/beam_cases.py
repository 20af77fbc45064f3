"""The cases of the device beam-search tests (tests/test_beam_device_cpu.py, tests/test_beam_device_gpu.py) with their seeds.

A decode case is a parameter dict for beam_ref.decode: B samples x nb beams over a vocabulary of V on the seeded logits oracle.
Every (nb, V) pair runs under every SETTING (max_length, min_length, length_penalty, early_stopping, eos bias); the larger
eos biases are there because an oracle with bias 2 never finishes a sample early.  The seed of a case is the first of 0, 1, 2, ...
whose decode keeps EVERY decision margin (beam_ref) >= MARGIN; it was found on the CPU by `python tests/beam_cases.py` and is
written down here, and the CPU test asserts the margins of every case again.  No case is skipped.

K (the bound of the candidate scores, err <= K E32 + ULP with beam_ref.score_errors' E32 and ULP): twice the worst ratio
err / E32 that the numpy emulation of the row kernel's summation order (beam_ref.emu_scores) reaches over STEP_CASES, measured
on the CPU by emulation_worst_ratio() before any device run (EMU_WORST; profiles/generate_decode.md)."""
import numpy as np

import beam_ref

MARGIN = 1e-4
EOS, PAD, BOS = 2, 0, 1
SETTINGS = [            # max_length, min_length, length_penalty, early_stopping, eos bias
    (8, 1, 1.0, False, 2.0),
    (8, 0, 0.0, False, 4.0),
    (10, 3, 2.0, False, 6.0),
    (8, 1, 1.0, True, 6.0),
    (12, 1, 1.0, False, 8.0),
]
SHAPES = [(3, 1), (3, 2), (3, 5), (2, 10), (1, 16)]          # (B, nb)
# (nb, V, setting) -> seed
SEEDS = {(5, 50, 2): 1, (5, 200, 0): 2, (5, 200, 1): 1, (10, 21, 2): 3, (10, 50, 0): 2, (10, 50, 2): 1, (10, 200, 2): 2,
         (10, 200, 4): 3, (16, 33, 0): 1, (16, 200, 0): 1, (16, 200, 2): 4, (16, 200, 3): 1}      # every other case: seed 0


def vocabularies(nb):
    return (2 * nb + 1, 50, 200)


def decode_cases():
    out = []
    for B, nb in SHAPES:
        for V in vocabularies(nb):
            for i, (ml, minl, lp, es, bias) in enumerate(SETTINGS):
                out.append(dict(B=B, nb=nb, V=V, max_length=ml, min_length=minl, length_penalty=lp, early_stopping=es,
                                eos_bias=bias, eos=EOS, pad=PAD, seed=SEEDS.get((nb, V, i), 0), setting=i))
    # the shapes of the trial: a larger vocabulary, and 16 beams over 33 tokens
    out.append(dict(B=2, nb=10, V=3000, max_length=8, min_length=1, length_penalty=1.0, early_stopping=False, eos_bias=2.0,
                    eos=EOS, pad=PAD, seed=SEEDS.get((10, 3000, 0), 0), setting=0))
    return out


def case_id(p):
    return "B%d-nb%d-V%d-s%d" % (p["B"], p["nb"], p["V"], p["setting"])


def run_case(p, extra_steps=0):
    """-> dict(seq, scores, state, margins, min_margin, all_done (before max_length), mixed, evicted, ignored_eos)"""
    margins, records = [], []
    seq, scores, st = beam_ref.decode(p, extra_steps=extra_steps, margins=margins, records=records)
    return dict(seq=seq, scores=scores, state=st, margins=margins, min_margin=min([m for _, m in margins] or [np.inf]),
                all_done=bool(st["done"].all()) and st["cur_len"] < p["max_length"],
                mixed=bool(st["done"].any()) and not bool(st["done"].all()), evicted=any(k == "evict" for k, _ in margins),
                ignored_eos=sum(r["ignored_eos"] for r in records) > 0, steps=len(records))


# ---- one step on crafted logits (GPU): (B, nb, V) and what the step's logits look like ------------------------------------------
STEP_SHAPES = [(1, 1, 33), (3, 5, 33), (3, 10, 200), (1, 16, 33), (3, 16, 200), (1, 10, 200), (3, 1, 200)]
STEP_LARGE = [(1, 10, 30523), (3, 5, 30524)]
STEP_MAX_LENGTH = 8
EMU_WORST = 1.1365         # (B, nb, V) = (1, 16, 33) at position 1: 1.91e-06 against E32 = 1.68e-06
K = 2 * EMU_WORST


def step_params(B, nb, V, min_length, length_penalty=1.0, early_stopping=False, seed=0):
    return dict(B=B, nb=nb, V=V, max_length=STEP_MAX_LENGTH, min_length=min_length, length_penalty=length_penalty,
                early_stopping=early_stopping, eos_bias=3.0, eos=EOS, pad=PAD, seed=seed, setting=-1)


def state_at(p, position, done_sample=None):
    """the reference state after `position` oracle steps (cur_len = position + 1), optionally with one sample marked done
    (its beams are then what a done sample's are: score 0, padding) -> (state, the oracle's logits for the next step)"""
    orc = beam_ref.make_oracle(p)
    st = beam_ref.new_state(p)
    for _ in range(position):
        beam_ref.step(st, beam_ref.oracle_logits(orc, st["cur_len"] - 1, st["ids"], p["nb"]), p)
    if done_sample is not None and done_sample < p["B"]:
        rows = slice(done_sample * p["nb"], (done_sample + 1) * p["nb"])
        st["done"][done_sample] = True
        st["beam_score"][rows] = 0.0
    return st, beam_ref.oracle_logits(orc, st["cur_len"] - 1, st["ids"], p["nb"])


STEP_SEEDS = {(1, 16, 33, 6, False, "f32"): 1, (1, 16, 33, 6, True, "f32"): 1, (1, 10, 200, 1, False, "f32"): 1,
              (1, 10, 200, 1, True, "f32"): 1}          # every other step case: seed 0


def step_cases():
    """(B, nb, V, position, min_length on, logits dtype): every shape at positions 0, 1 and max_length - 2 with and without the eos
    suppressed in fp32; two shapes in bf16 too; the two large vocabularies once each (30523: rows that start off a 16-byte
    boundary) and the odd one once more in bf16.  Sample 1 of the B = 3 shapes is done from position 1 on."""
    out = [(B, nb, V, pos, on, "f32") for B, nb, V in STEP_SHAPES for pos in (0, 1, STEP_MAX_LENGTH - 2) for on in (False, True)]
    out += [(B, nb, V, pos, pos == 1, "bf16") for B, nb, V in ((3, 5, 33), (3, 10, 200)) for pos in (0, 1, STEP_MAX_LENGTH - 2)]
    out += [STEP_LARGE[0] + (1, False, "f32"), STEP_LARGE[1] + (STEP_MAX_LENGTH - 2, True, "f32"), STEP_LARGE[0] + (1, False, "bf16")]
    return out


def step_id(c):
    return "B%d-nb%d-V%d-pos%d-%s-%s" % (c[0], c[1], c[2], c[3], "noeos" if c[4] else "eos", c[5])


def to_bf16(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16).float().numpy()


def make_step(c, seed=None):
    """-> (params, reference state before the step, the step's logits as fp32 values)"""
    B, nb, V, pos, on, dtype = c
    p = step_params(B, nb, V, STEP_MAX_LENGTH if on else 0, seed=STEP_SEEDS.get(c, 0) if seed is None else seed)
    st, logits = state_at(p, pos, done_sample=1 if (B == 3 and pos >= 1) else None)
    return p, st, (to_bf16(logits) if dtype == "bf16" else logits)


def step_margin(c, seed=None):
    """the smallest decision margin of the step; bf16 logits repeat inside a row, and equal logits of one row are equal scores
    on every route (the index decides): gaps of exactly 0 are ties by construction, not near-ties"""
    p, st, logits = make_step(c, seed)
    m = []
    beam_ref.step(st, logits, p, m)
    return min([v for _, v in m if not (c[5] == "bf16" and v == 0.0)] or [np.inf])


def emulation_worst_ratio():
    worst, where = 0.0, None
    for B, nb, V in STEP_SHAPES + STEP_LARGE[:1]:
        for position in (0, 1, STEP_MAX_LENGTH - 2):
            for min_length in (0, STEP_MAX_LENGTH):
                p = step_params(B, nb, V, min_length)
                st, logits = state_at(p, position)
                head = 1 if V % 2 else 0
                emu = beam_ref.emu_scores(logits, st["beam_score"], st["cur_len"], p, head=head)
                err, e32, ulp = beam_ref.score_errors(emu, logits, st["beam_score"], st["cur_len"], p)
                live = np.isfinite(err) & (np.abs(st["beam_score"]) < 1e8)[:, None]
                r = float(err[live].max()) / e32
                if r > worst:
                    worst, where = r, (B, nb, V, position, min_length, float(err[live].max()), e32, ulp)
    return worst, where


def find_seeds(tries=40):
    found = {}
    for p in decode_cases():
        for seed in range(tries):
            r = run_case(dict(p, seed=seed))
            if r["min_margin"] >= MARGIN:
                found[(p["nb"], p["V"], p["setting"])] = seed
                break
        else:
            raise RuntimeError("no seed for %s" % case_id(p))
    return found


if __name__ == "__main__":
    import sys
    if "seeds" in sys.argv:
        f = find_seeds()
        print("SEEDS = {%s}" % ", ".join("%r: %d" % kv for kv in sorted(f.items())))
    if "steps" in sys.argv:
        print("STEP_SEEDS = {%s}" % ", ".join("%r: %d" % (c, next(k for k in range(40) if step_margin(c, k) >= MARGIN))
                                              for c in step_cases() if step_margin(c, 0) < MARGIN))
    if "emu" in sys.argv:
        print(emulation_worst_ratio())
