"""Golden vectors for the stage-1 question branch (LangModule, AttFlat, MCAN_E, MCAN_ED and the branch of ScanQA.forward,
models/qa_module.py:501-587), produced by the REFERENCE's own models/lang_module.py and models/mcan_module.py on the CPU of the
build container.  Both files are imported at run time by path; nothing of them is copied.

TEST INFRASTRUCTURE.  Usage:  python tools/gen_golden_lang.py [reference checkout]   -> tests/golden/lang_branch.npz (data only)

Weights are not stored: tests/golden_util.fill_params seeds every state-dict entry by the crc32 of its NAME, so the reference
module here and the bridgeqa_amd module in the tests hold the same values iff their keys and shapes agree; the key lists are
stored.  ScanQA itself is not instantiated (its module imports the CUDA-only point-cloud extension): the branch's modules are
created from the reference's classes in the order and with the arguments of qa_module.py:252-330 (`Branch`), and run in the
order of :501-587 (`branch_reference`, statements cited).

Sizes: LSTM E = 20, H = 128, lens [1, 9, 7, 2, 9] in T = 12 (unsorted, a length of 1, a tie, max(len) < T); MCAN / AttFlat at
hidden 32, 8 heads, 2 layers; the whole branch at hidden 128 over 16 proposals, 18 classes, B = 3."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.dont_write_bytecode = True
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "lang_branch.npz")
sys.path.insert(0, os.path.join(REPO, "oracle"))
sys.path.insert(0, os.path.join(REPO, "tests"))
from gen_golden_loss import REF as DEFAULT_REF  # noqa: E402
from golden_util import fill_params  # noqa: E402

LENS = [1, 9, 7, 2, 9]


def load(ref, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def keys_of(module, prefix=""):
    return np.array(["%s%s %s" % (prefix, k, "x".join(map(str, v.shape))) for k, v in module.state_dict().items()])


def branch_inputs(seed, B, K, hidden, T, E, lens, num_class=18):
    g = torch.Generator().manual_seed(seed)
    bbox_mask = (torch.rand(B, K, generator=g) > 0.4).float()
    bbox_mask[:, 0] = 1
    return dict(object_feat=torch.randn(B, K, hidden, generator=g), bbox_mask=bbox_mask,
                objectness_scores=torch.randn(B, K, 2, generator=g), lang_feat=torch.randn(B, T, E, generator=g),
                lang_len=torch.tensor(lens))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_REF
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "lib"))
    lm = load(ref, "models/lang_module.py", "ref_lang_module")
    mc = load(ref, "models/mcan_module.py", "ref_mcan_module")
    save = {}

    # ---- LangModule (eval mode: dropout off), one layer forward-only and two layers bidirectional
    g = torch.Generator().manual_seed(11)
    lang_feat = torch.randn(len(LENS), 12, 20, generator=g)
    save["lm_lang_feat"], save["lm_lang_len"] = lang_feat.numpy(), np.array(LENS, dtype=np.int64)
    for tag, kw in (("uni", dict(use_bidir=False, num_layers=1)), ("bi2", dict(use_bidir=True, num_layers=2))):
        m = lm.LangModule(18, use_lang_classifier=True, emb_size=20, hidden_size=128, **kw).eval()
        fill_params(m, "lm_%s." % tag)
        with torch.no_grad():
            d = m({"lang_feat": lang_feat.clone(), "lang_len": torch.tensor(LENS)})
        save["lm_%s_keys" % tag] = keys_of(m)
        for k in ("lang_out", "lang_emb", "lang_mask", "lang_scores"):
            save["lm_%s_%s" % (tag, k)] = d[k].numpy()
        # the reference's own fp32-vs-fp64 gap at this size (the tolerance of the CPU comparison is a multiple of it)
        with torch.no_grad():
            d64 = m.double()({"lang_feat": lang_feat.double(), "lang_len": torch.tensor(LENS)})
        save["lm_%s_gap64" % tag] = np.array(float((d64["lang_out"] - torch.from_numpy(save["lm_%s_lang_out" % tag]).double()).abs().max()))
        print("LangModule", tag, tuple(d["lang_out"].shape), "fp32-vs-fp64 gap %.2e" % save["lm_%s_gap64" % tag])

    # ---- AttFlat / MCAN_E / MCAN_ED at hidden 32, 8 heads, 2 layers, both masks in use
    g = torch.Generator().manual_seed(12)
    x, y = torch.randn(3, 9, 32, generator=g), torch.randn(3, 16, 32, generator=g)
    x_mask = torch.tensor([[t >= n for t in range(9)] for n in (9, 4, 1)]).unsqueeze(1).unsqueeze(2)
    y_mask = (torch.rand(3, 16, generator=g) > 0.6)
    y_mask[:, 0] = False
    y_mask = y_mask.unsqueeze(1).unsqueeze(2)
    save.update(mc_x=x.numpy(), mc_y=y.numpy(), mc_x_mask=x_mask.numpy(), mc_y_mask=y_mask.numpy())
    af = mc.AttFlat(32, flat_mlp_size=48, flat_glimpses=2, flat_out_size=40, pdrop=0.1).eval()
    e = mc.MCAN_E(32, num_heads=8, num_layers=2, pdrop=0.1).eval()
    ed = mc.MCAN_ED(32, num_heads=8, num_layers=2, pdrop=0.1).eval()
    fill_params(af, "af."), fill_params(e, "e."), fill_params(ed, "ed.")
    with torch.no_grad():
        save["af_keys"], save["af_out_x"], save["af_out_y"] = keys_of(af), af(x, x_mask).numpy(), af(y, y_mask).numpy()
        save["af_out_nomask"] = af(x, None).numpy()
        save["e_keys"], save["e_out"] = keys_of(e), e(y, y_mask).numpy()
        ox, oy = ed(x, y, x_mask, y_mask)
        save["ed_keys"], save["ed_out_x"], save["ed_out_y"] = keys_of(ed), ox.numpy(), oy.numpy()
    print("parameters: AttFlat %d, MCAN_E %d, MCAN_ED %d" % tuple(sum(p.numel() for p in m.parameters()) for m in (af, e, ed)))

    # ---- the branch of ScanQA (qa_module.py:252-330 / 501-587) on the reference's classes
    class Branch(nn.Module):
        def __init__(self, num_answers, num_object_class, hidden_size=128, answer_pdrop=0.3, mcan_num_layers=2, mcan_num_heads=8,
                     mcan_pdrop=0.1, mcan_flat_mlp_size=512, mcan_flat_glimpses=1, mcan_flat_out_size=1024, lang_use_bidir=False,
                     lang_num_layers=1, lang_emb_size=300, lang_pdrop=0.1):
            super().__init__()
            lang_size = hidden_size * (1 + lang_use_bidir)                                                          # :153
            self.object_cls = nn.Sequential(nn.Linear(hidden_size, hidden_size), nn.GELU(), nn.Dropout(0.1),
                                            nn.Linear(hidden_size, 1))                                             # :254-259
            self.lang_net = lm.LangModule(num_object_class, use_lang_classifier=False, use_bidir=lang_use_bidir,
                                          num_layers=lang_num_layers, emb_size=lang_emb_size, hidden_size=hidden_size,
                                          pdrop=lang_pdrop, bert_model_name=None, freeze_bert=False,
                                          finetune_bert_last_layer=False)                                          # :269-280
            self.lang_feat_linear = nn.Sequential(nn.Linear(lang_size, hidden_size), nn.GELU())                    # :283-285
            self.lang_cls = nn.Sequential(nn.Linear(mcan_flat_out_size, hidden_size), nn.GELU(), nn.Dropout(0.1),
                                          nn.Linear(hidden_size, num_object_class))                                # :288-293
            self.attflat_visual = mc.AttFlat(hidden_size, mcan_flat_mlp_size, mcan_flat_glimpses, mcan_flat_out_size, 0.1)
            self.attflat_lang = mc.AttFlat(hidden_size, mcan_flat_mlp_size, mcan_flat_glimpses, mcan_flat_out_size, 0.1)
            self.answer_cls = nn.Sequential(nn.Linear(mcan_flat_out_size, hidden_size), nn.GELU(), nn.Dropout(answer_pdrop),
                                            nn.Linear(hidden_size, num_answers))                                   # :302-307
            self.fusion_backbone = mc.MCAN_ED(hidden_size, num_heads=mcan_num_heads, num_layers=mcan_num_layers,
                                              pdrop=mcan_pdrop)                                                    # :324-329
            self.fusion_norm = mc.LayerNorm(mcan_flat_out_size)                                                    # :330

    def branch_reference(self, data_dict, object_feat, object_mask):
        data_dict = self.lang_net(data_dict)                                                                       # :501
        lang_feat, lang_mask = data_dict["lang_out"], data_dict["lang_mask"]                                       # :510-512
        if lang_mask.dim() == 2:
            lang_mask = lang_mask.unsqueeze(1).unsqueeze(2)                                                        # :514-515
        lang_feat = self.lang_feat_linear(lang_feat)                                                               # :518
        lang_feat, object_feat = self.fusion_backbone(lang_feat, object_feat, lang_mask, object_mask)              # :522
        object_conf_feat = object_feat * data_dict["objectness_scores"].max(2)[1].float().unsqueeze(2)             # :543
        data_dict["cluster_ref"] = self.object_cls(object_conf_feat).squeeze(-1)                                   # :546
        lang_feat = self.attflat_lang(lang_feat, lang_mask)                                                        # :548
        object_feat = self.attflat_visual(object_feat, object_mask, 0, 100)                                        # :553
        fuse_feat = self.fusion_norm(lang_feat + object_feat)                                                      # :560
        data_dict["fuse_feat"] = fuse_feat.clone()                                                                 # :564
        data_dict["lang_scores"] = self.lang_cls(fuse_feat)                                                        # :575
        data_dict["answer_scores"] = self.answer_cls(fuse_feat)                                                    # :585
        return data_dict

    # (a) the default-size module tree: key names and shapes only
    save["branch_default_keys"] = keys_of(Branch(num_answers=30, num_object_class=18, hidden_size=256))
    # (b) a small one, run: hidden 128, 16 proposals, E = 20, flat sizes 64 / 1 / 96
    kw = dict(num_answers=30, num_object_class=18, hidden_size=128, mcan_flat_mlp_size=64, mcan_flat_out_size=96,
              lang_emb_size=20)
    br = Branch(**kw).eval()
    fill_params(br, "branch.")
    save["branch_keys"] = keys_of(br)
    inp = branch_inputs(13, 3, 16, 128, 12, 20, [5, 12, 1])
    for k, v in inp.items():
        save["br_in_" + k] = v.numpy()
    object_mask = (~inp["bbox_mask"].bool().detach()).unsqueeze(1).unsqueeze(2)                                    # :467-474
    with torch.no_grad():
        d = branch_reference(br, {k: v.clone() for k, v in inp.items()}, inp["object_feat"], object_mask)
    for k in ("lang_out", "lang_emb", "lang_mask", "fuse_feat", "lang_scores", "cluster_ref", "answer_scores"):
        save["br_out_" + k] = d[k].numpy()
    np.savez_compressed(OUT, **save)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(save), "arrays")


if __name__ == "__main__":
    main()
