"""generate on the static K/V cache (ops.DecodeCache + csrc/attn_decode.hip), through the modules: the step logits against the
fp32 composition of today's cached path (which carries the reference's semantics: growing cache, index_select reorder, encoder
states fixed to the beam SLOT), the returned score against a cache-free fp32 re-scoring, the route actually taken, the inputs
that must stay on today's path, and the replay of one captured step.

The decoder is BertConfig(num_hidden_layers=2, vocab_size=200, max_position_embeddings=64) at the default hidden 768 / 12 heads
-- the shapes the GEMM family serves -- sharpened as tests/test_generate_cpu.make_decoder does; S = 20 slots (2 samples x 10
beams), 7 encoder tokens with a ragged mask, encoder states that differ per slot half (concat_repeat)."""
import pytest
import torch

from test_generate_cpu import BOS, EOS, PAD, logprobs_of, make_decoder, run_blip_generate

pytestmark = pytest.mark.gpu

V, B, K, LENC = 200, 2, 10, 7
S = B * K


@pytest.fixture(scope="module")
def rig(dev):
    from bridgeqa_amd import med
    from bridgeqa_amd.blip_vqa_3d import concat_repeat
    cfg = med.BertConfig(num_hidden_layers=2, vocab_size=V, max_position_embeddings=64)
    torch.manual_seed(0)
    dec = med.BertLMHeadModel(config=cfg).to(dev).eval()
    with torch.no_grad():
        dec.cls.predictions.bias.copy_(torch.randn(V, device=dev) * 1.5)
        dec.cls.predictions.decoder.weight.mul_(8.0)
    g = torch.Generator().manual_seed(21)
    a, b = torch.randn(B, LENC, 768, generator=g).to(dev), torch.randn(B, LENC, 768, generator=g).to(dev)
    m = torch.ones(B, LENC, dtype=torch.long)
    m[1, 4:] = 0                                        # ragged: sample 1 sees 4 of its 7 encoder tokens
    toks = [torch.full((S, 1), BOS, dtype=torch.long)] + [torch.randint(3, V, (S, 1), generator=g) for _ in range(5)]
    base = (torch.arange(B) * K).unsqueeze(1)
    sched = []
    for _ in range(5):                                  # picks inside each sample, across its two encoder halves
        pick = torch.randint(0, K, (B, K), generator=g)
        pick[:, 0], pick[:, K - 1] = K - 1, 0           # slot 0 continues a hypothesis of the other half, and back
        sched.append((pick + base).reshape(-1).to(dev))
    return dict(dec=dec, a=a, b=b, enc=concat_repeat(a, b, K // 2), enc_same=concat_repeat(a, a, K // 2),
                m=m.to(dev), em=m.repeat_interleave(K, dim=0).to(dev), toks=[t.to(dev) for t in toks], sched=sched)


class _dtype(object):
    def __init__(self, dt):
        self.dt = dt

    def __enter__(self):
        from bridgeqa_amd import fusion_ops as ops
        self.prev = ops.set_compute_dtype(self.dt)

    def __exit__(self, *a):
        from bridgeqa_amd import fusion_ops as ops
        ops.set_compute_dtype(self.prev)


class _switch(object):
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from bridgeqa_amd import med
        self.prev, med._DECODE_CACHE[0] = med._DECODE_CACHE[0], self.on

    def __exit__(self, *a):
        from bridgeqa_amd import med
        med._DECODE_CACHE[0] = self.prev


def _todays_steps(r):
    """six steps on the growing cache, driven as generation.beam_search drives them (prepare_inputs_for_generation, the last
    token once a cache exists, _reorder_cache)"""
    dec, out = r["dec"], []
    cur, past = r["toks"][0], None
    with torch.no_grad():
        for k in range(6):
            inp = dec.prepare_inputs_for_generation(cur, past=past, encoder_hidden_states=r["enc"], encoder_attention_mask=r["em"])
            o = dec(**inp, use_cache=True, return_dict=True)
            out.append(o.logits[:, -1, :].float().clone())
            if k < 5:
                past = dec._reorder_cache(o.past_key_values, r["sched"][k])
                cur = torch.cat([cur[r["sched"][k]], r["toks"][k + 1]], dim=-1)
    return out


def _cache_steps(r, graph=False):
    sess = r["dec"].decode_session(r["toks"][0], 20, r["enc"], r["em"], graph=graph)
    assert sess is not None, "the decode is eligible for the static cache"
    out = []
    for k in range(6):
        out.append(sess.step(r["toks"][k]).clone())
        if k < 5:
            sess.reorder(r["sched"][k])
    return out


def _rel(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


def test_step_logits_follow_the_fp32_composition(rig):
    """a wrong ancestry row, or a slot reading another slot's encoder block, is an O(1) error here"""
    from bridgeqa_amd import _ext
    with _dtype(torch.float32):
        ref = _todays_steps(rig)
    with _dtype(torch.bfloat16):
        with _switch(False):
            parent = _todays_steps(rig)
        calls = list(_ext.DECODE_CALLS)
        with _switch(True):
            cache = _cache_steps(rig)
    assert _ext.DECODE_CALLS[0] == calls[0] + 12 and _ext.DECODE_CALLS[1] == calls[1] + 12      # 6 steps x 2 layers each
    worst = 0.0
    for k in range(6):
        rp, rc = _rel(parent[k], ref[k]), _rel(cache[k].float(), ref[k])
        print("step %d rel-L2 against fp32: today's bf16 path %.3e   cache route %.3e" % (k, rp, rc))
        worst = max(worst, rc)
    assert worst <= 2e-2, worst                       # the repo's bf16 tolerance


def _discrepancy(rig, seq, score):
    """|returned score - teacher-forced fp32 score without any cache| of the returned sequences, the worst sample"""
    worst = 0.0
    with _dtype(torch.float32):
        for i in range(B):
            s = [t for t in seq[i].tolist() if t != PAD]
            lps = logprobs_of(rig["dec"], torch.tensor(s, device=seq.device), rig["a"][i], rig["m"][i])
            n_prefix = len(s) - 1 if s[-1] == EOS else len(s)
            worst = max(worst, abs(sum(lps) / n_prefix - float(score[i])))
    return worst


def test_returned_score_is_the_sequences_own(rig):
    """identical encoder halves make the score checkable by plain teacher forcing; the cache route may be off by at most twice
    what today's bf16 path is off on the same inputs (both are maxima of independent bf16 roundings over a handful of steps),
    plus 1e-3 for the case where today's happens to be near zero"""
    dec = rig["dec"]
    bos = torch.full((B, 1), BOS, dtype=torch.long, device=rig["a"].device)
    kw = dict(max_length=8, min_length=1, num_beams=K, eos_token_id=EOS, pad_token_id=PAD, encoder_hidden_states=rig["enc_same"],
              encoder_attention_mask=rig["em"], return_scores=True)
    from bridgeqa_amd import med
    with _dtype(torch.bfloat16):
        with _switch(False):
            seq_p, score_p = dec.generate(bos, **kw)
        sessions = med._DECODE_STATS["sessions"]
        with _switch(True):
            seq_c, score_c = dec.generate(bos, **kw)
        assert med._DECODE_STATS["sessions"] == sessions + 1
    d_parent, d_cache = _discrepancy(rig, seq_p, score_p), _discrepancy(rig, seq_c, score_c)
    print("score discrepancy against fp32 teacher forcing: today's bf16 path %.3e   cache route %.3e" % (d_parent, d_cache))
    assert seq_c.shape[0] == B and bool((seq_c[:, 0] == BOS).all())
    assert d_cache <= 2.0 * d_parent + 1e-3, (d_cache, d_parent)


def test_blip_generate_takes_the_cache_route_and_is_repeatable(dev):
    from bridgeqa_amd import _ext, med
    calls, sessions = list(_ext.DECODE_CALLS), med._DECODE_STATS["sessions"]
    with _dtype(torch.bfloat16):
        with _switch(True):
            run_blip_generate(dev)                  # two calls, identical answers and fused states (asserted inside)
    assert med._DECODE_STATS["sessions"] == sessions + 2
    assert _ext.DECODE_CALLS[0] > calls[0] and _ext.DECODE_CALLS[1] > calls[1]
    assert _ext.DECODE_CALLS[0] - calls[0] == _ext.DECODE_CALLS[1] - calls[1]


def _both(dec, bos, **kw):
    from bridgeqa_amd import _ext
    with _dtype(torch.bfloat16):
        with _switch(False):
            off = dec.generate(bos, return_scores=True, **kw)
        calls = list(_ext.DECODE_CALLS)
        with _switch(True):
            on = dec.generate(bos, return_scores=True, **kw)
        assert _ext.DECODE_CALLS == calls, "an ineligible decode reached the decode kernel"
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])


def test_ineligible_inputs_stay_on_todays_path(rig, dev):
    kw = dict(max_length=8, min_length=1, num_beams=K, eos_token_id=EOS, pad_token_id=PAD)
    # head size 16
    small = make_decoder(40, dev, seed=2)
    g = torch.Generator().manual_seed(5)
    enc = torch.randn(S, 5, 64, generator=g).to(dev)
    _both(small, torch.full((B, 1), BOS, dtype=torch.long, device=dev), encoder_hidden_states=enc,
          encoder_attention_mask=torch.ones(S, 5, dtype=torch.long, device=dev), **kw)
    # a prompt of two tokens
    dec = rig["dec"]
    two = torch.tensor([[BOS, 7], [BOS, 9]], dtype=torch.long, device=dev)
    _both(dec, two, encoder_hidden_states=rig["enc"], encoder_attention_mask=rig["em"], **kw)
    # a save_attention hook
    hook = dec.bert.encoder.layer[1].crossattention.self
    hook.save_attention = True
    try:
        _both(dec, torch.full((B, 1), BOS, dtype=torch.long, device=dev), encoder_hidden_states=rig["enc"],
              encoder_attention_mask=rig["em"], **kw)
    finally:
        hook.save_attention = False


def test_replayed_steps_are_bitwise_the_eager_cache_route(rig):
    from bridgeqa_amd import med
    with _dtype(torch.bfloat16):
        with _switch(True):
            eager = _cache_steps(rig, graph=False)
            captures = med._DECODE_STATS["captures"]
            replay = _cache_steps(rig, graph=True)
    assert med._DECODE_STATS["captures"] == captures + 1           # exactly one capture, replayed four more times
    for k in range(6):
        assert torch.equal(eager[k].view(torch.int16), replay[k].view(torch.int16)), k
