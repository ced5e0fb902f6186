"""Shared helpers of the Chinese-branch tests: the config directories a user would point the model at, written to a temp dir."""
import json
import os
import tempfile
from argparse import Namespace

from conftest import ROOT
from hmmc_amd import synth


def bert_config_dir(bdims, **over):
    """<pretrained_text>: a directory with the encoder's config.json (what save_pretrained writes beside the weights)."""
    d = tempfile.mkdtemp(prefix="hmmc_zh_cfg_")
    cfg = bdims.to_config()
    cfg.update(over)
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(cfg, fh)
    return d


def cross_dir(bdims):
    """cross-base with chinese_hidden_size set to the encoder's width (the shipped file says 768)."""
    cfg = json.load(open(os.path.join(ROOT, "hmmc_amd", "cross-base", "cross_config.json")))
    cfg["chinese_hidden_size"] = bdims.hidden_size
    d = tempfile.mkdtemp(prefix="hmmc_zh_cross_")
    with open(os.path.join(d, "cross_config.json"), "w") as fh:
        json.dump(cfg, fh)
    return d


def task_config(bdims, **kw):
    over = {k: kw.pop(k) for k in ("hidden_dropout_prob", "attention_probs_dropout_prob") if k in kw}
    d = dict(local_rank=0, rank=0, use_temp=True, language="chinese", top_frames=2, max_frames=4, n_display=100000,
             logdir=None, use_frame_fea=True, dataset="msrvtt", pretrained_text=bert_config_dir(bdims, **over), lr=1e-4,
             text_lr=3e-5, coef_lr=1e-3, weight_decay=0.2, warmup_proportion=0.1)
    d.update(kw)
    return Namespace(**d)


def build(dims, bdims, sd=None, **tc):
    """BirdModel(language = "chinese") with the synthetic state loaded, fp32 throughout (the reference after model.float())."""
    from hmmc_amd.modeling import BirdModel
    sd = sd if sd is not None else synth.finetune_state_zh(dims, bdims)
    model = BirdModel.from_pretrained(cross_dir(bdims), state_dict=sd, task_config=task_config(bdims, **tc))
    return model.float()
