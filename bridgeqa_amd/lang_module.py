"""`LangModule` of the question branch -- mirror of the reference's models/lang_module.py:14-119 with its constructor signature,
forward contract and state-dict keys (lstm.weight_ih_l0, ..., lstm.bias_hh_l{k}_reverse, lang_cls.1.*).

An nn.LSTM is kept as the parameter holder, so keys and initialisation are the reference's.  What runs it:

  fused route   fp32 CUDA tensors and hidden size in _ext.LSTM_HIDDEN: per (layer, direction) one autograd Function over
                csrc/lstm.hip -- Gx = x W_ih^T + b_ih + b_hh as one GEMM, the recurrence in bq_lstm_fwd (pad rows written as
                zeros by the kernel), bq_lstm_bwd for dGx, then dX / dW_ih / dW_hh / the bias gradients as GEMMs and a column
                sum.  Layers and directions are looped on the host; the inter-layer dropout is a torch op.  W_hh^T is formed
                per call (a 1 MB transpose at H = 256; profiles/lang_branch.md).
  fallback      anything else (CPU, double, other hidden sizes, BQ_LSTM_FUSED=0): the held nn.LSTM on
                pack_padded_sequence(enforce_sorted=False) input, exactly as the reference.

BQ_LSTM_FUSED: "1" / "0" force the choice among eligible inputs; unset = the default recorded in profiles/lang_branch.md.

`lang_len` is read on the HOST (max(len) sizes the outputs; the reference does `.cpu()` on it every step and the loader
delivers it there): a device tensor costs one synchronisation per forward.  A zero length raises ValueError, as
pack_padded_sequence does.  bert_model_name raises NotImplementedError (the package carries no HF encoder for this branch).
"""
import os

import torch
import torch.nn as nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

FUSED_DEFAULT = True   # profiles/lang_branch.md: the measured A/B this default follows


def fused_enabled():
    v = os.environ.get("BQ_LSTM_FUSED")
    return FUSED_DEFAULT if v is None or v == "" else v == "1"


class _LSTMDirection(torch.autograd.Function):
    """one layer, one direction of a packed-sequence LSTM over csrc/lstm.hip.  x (B, t_out, E) -> y (B, t_out, H), h_last (B, H)"""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, lens, t_out, reverse):
        from . import _ext
        x = x.contiguous()
        B, _, E = x.shape
        H = w_hh.shape[1]
        bias = b_ih + b_hh if b_ih is not None else None
        if bias is not None:
            gx = torch.addmm(bias, x.reshape(B * t_out, E), w_ih.t()).view(B, t_out, 4 * H)
        else:
            gx = torch.mm(x.reshape(B * t_out, E), w_ih.t()).view(B, t_out, 4 * H)
        save = any(ctx.needs_input_grad[:5])
        y, h_last, gates, cells = _ext.lstm_fwd(gx, w_hh.t().contiguous(), lens, t_out, reverse, save=save)
        if save:
            ctx.save_for_backward(x, w_ih, w_hh, lens, y, gates, cells)
            ctx.reverse, ctx.has_bias = reverse, b_ih is not None
        return y, h_last

    @staticmethod
    def backward(ctx, dy, dh_last):
        from . import _ext
        x, w_ih, w_hh, lens, y, gates, cells = ctx.saved_tensors
        B, t_out, H = y.shape
        dgx = _ext.lstm_bwd(dy.contiguous() if dy is not None else None, dh_last.contiguous() if dh_last is not None else None,
                            gates, cells, w_hh.contiguous(), lens, ctx.reverse)
        d2 = dgx.view(B * t_out, 4 * H)
        # h of the step before, in the order the direction walks (zero in front of the first step; dgx is zero in the padding)
        hprev = torch.zeros_like(y)
        if t_out > 1:
            if ctx.reverse:
                hprev[:, :-1] = y[:, 1:]
            else:
                hprev[:, 1:] = y[:, :-1]
        need = ctx.needs_input_grad
        dx = torch.mm(d2, w_ih).view(B, t_out, -1) if need[0] else None
        dw_ih = torch.mm(d2.t(), x.reshape(B * t_out, -1)) if need[1] else None
        dw_hh = torch.mm(d2.t(), hprev.view(B * t_out, H)) if need[2] else None
        db = d2.sum(0) if ctx.has_bias and (need[3] or need[4]) else None
        return dx, dw_ih, dw_hh, db if need[3] else None, db if need[4] else None, None, None, None


def lstm_eligible(lstm, x):
    """the fused route's condition (apart from BQ_LSTM_FUSED): fp32 CUDA input and parameters, batch_first, a built hidden size"""
    from . import _ext
    return (x.is_cuda and x.dtype == torch.float32 and lstm.batch_first and lstm.hidden_size in _ext.LSTM_HIDDEN
            and getattr(lstm, "proj_size", 0) == 0 and all(p.is_cuda and p.dtype == torch.float32 for p in lstm.parameters()))


def lstm_fused(lstm, x, lens_host, lens_dev=None):
    """`lstm` (an nn.LSTM, batch_first) over x (B, T, E) with lengths lens_host (a CPU int tensor, all >= 1) on the fused route.
    Returns out (B, max(len), H dirs), zero beyond each length, and h_n (layers dirs, B, H) as nn.LSTM orders it."""
    t_out = int(lens_host.max())
    lens_dev = (lens_host if lens_dev is None else lens_dev).to(device=x.device, dtype=torch.int32).contiguous()
    dirs = 2 if lstm.bidirectional else 1
    h_n, inp = [], x[:, :t_out]
    for layer in range(lstm.num_layers):
        outs = []
        for d in range(dirs):
            sfx = "_l%d%s" % (layer, "_reverse" if d else "")
            w_ih, w_hh = getattr(lstm, "weight_ih" + sfx), getattr(lstm, "weight_hh" + sfx)
            b_ih, b_hh = (getattr(lstm, "bias_ih" + sfx), getattr(lstm, "bias_hh" + sfx)) if lstm.bias else (None, None)
            y, h_last = _LSTMDirection.apply(inp, w_ih, w_hh, b_ih, b_hh, lens_dev, t_out, bool(d))
            outs.append(y)
            h_n.append(h_last)
        inp = outs[0] if dirs == 1 else torch.cat(outs, dim=-1)
        if layer + 1 < lstm.num_layers and lstm.dropout > 0 and lstm.training:
            inp = nn.functional.dropout(inp, lstm.dropout, True)
    return inp, torch.stack(h_n, 0)


class LangModule(nn.Module):
    def __init__(self, num_object_class, use_lang_classifier=True, use_bidir=False, num_layers=1, emb_size=300, hidden_size=256,
                 pdrop=0.1, word_pdrop=0.1, bert_model_name=None, freeze_bert=False, finetune_bert_last_layer=False):
        super().__init__()
        if bert_model_name is not None:
            raise NotImplementedError("LangModule: bert_model_name is not supported (GloVe rows + LSTM only)")
        self.num_object_class = num_object_class
        self.use_lang_classifier = use_lang_classifier
        self.use_bidir = use_bidir
        self.num_layers = num_layers
        self.bert_model_name = bert_model_name
        self.use_bert_model = False
        self.lstm = nn.LSTM(input_size=emb_size, hidden_size=hidden_size, batch_first=True, num_layers=num_layers,
                            bidirectional=use_bidir, dropout=0.1 if num_layers > 1 else 0)
        self.word_drop = nn.Dropout(pdrop)   # (word_pdrop is accepted and unused, as in the reference)
        lang_size = hidden_size * 2 if use_bidir else hidden_size
        if use_lang_classifier:
            self.lang_cls = nn.Sequential(nn.Dropout(p=pdrop), nn.Linear(lang_size, num_object_class))

    def make_mask(self, feature):
        """True where a row is all zeros (= padding: the LSTM output is written as zeros beyond each length)"""
        return torch.sum(torch.abs(feature), dim=-1) == 0

    def forward(self, data_dict):
        """data_dict: lang_feat (B, T, emb) GloVe rows, lang_len (B) -- read on the host: a device tensor costs one
        synchronisation.  Writes lang_out (B, max(len), H dirs), lang_emb (B, H dirs), lang_mask (B, max(len)) with True =
        padding, and lang_scores under use_lang_classifier."""
        word_embs = self.word_drop(data_dict["lang_feat"])
        lang_len = data_dict["lang_len"]
        lens_host = lang_len.cpu()
        if lens_host.numel() and int(lens_host.min()) <= 0:
            raise ValueError("LangModule: every lang_len must be at least 1 (pack_padded_sequence refuses a zero length)")
        if fused_enabled() and lstm_eligible(self.lstm, word_embs):
            lang_output, lang_last = lstm_fused(self.lstm, word_embs, lens_host, lang_len if lang_len.is_cuda else None)
        else:
            packed = pack_padded_sequence(word_embs, lens_host, batch_first=True, enforce_sorted=False)
            packed_output, (lang_last, _) = self.lstm(packed)
            lang_output, _ = pad_packed_sequence(packed_output, batch_first=True)
        data_dict["lang_out"] = lang_output
        _, batch_size, hidden_size = lang_last.size()
        lang_last = lang_last.view(self.num_layers, -1, batch_size, hidden_size)[-1]
        data_dict["lang_emb"] = lang_last.permute(1, 0, 2).contiguous().flatten(start_dim=1)
        data_dict["lang_mask"] = self.make_mask(lang_output)
        if self.use_lang_classifier:
            data_dict["lang_scores"] = self.lang_cls(data_dict["lang_emb"])
        return data_dict
