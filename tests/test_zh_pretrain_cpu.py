"""CPU checks of pre-training with the Chinese text branch: the model constructs from a <pretrained_text> directory that holds
the BertTokenizer's vocab.txt, with the reference's state_dict layout; and the plain-torch restatement tests/zh_pretrain_ref.py
reproduces the reference's own fp32 runs stored in tests/golden/moco_zh*_fp32.npz (tests/golden/make_golden_zh_pretrain.py).

Tolerances are those tests/test_zh_cpu.py applies to the fine-tune fixtures: loss 1e-4, gradient norms 2e-3 relative; for the
sampled weights and queue columns, which the fine-tune fixtures do not have, those tests/test_oracle_golden.py applies to the
English pre-training fixture (1e-5 + 1e-4 relative; 1e-5).  From step 1 on the weights have moved by one fp32 BertAdam update
per step on both sides and the losses are held to test_oracle_golden's multi-step 2e-3."""
import json
import os

import pytest
import torch

import zh_pretrain_ref as R
from conftest import GOLDEN, golden
from hmmc_amd import synth
from test_zh_cpu import close


def test_model_constructs_from_a_directory_with_vocab_txt():
    model = R.build(synth.TINY, synth.ZH_TINY)
    assert (model.PAD_ID, model.CLS_ID, model.MASK_ID, model.VOCAB) == (0, 101, 103, synth.ZH_TINY.vocab_size)
    assert tuple(model.cls.decoder.weight.shape) == (synth.ZH_TINY.vocab_size, 512)
    assert tuple(model.cls.bias.shape) == (synth.ZH_TINY.vocab_size,)
    online, key = dict(model.text_encoder.named_parameters()), dict(model.text_encoder_k.named_parameters())
    assert list(online) == list(key) and any(n.startswith("chinese_encoder.") for n in online)
    for n, p in online.items():
        assert p.requires_grad and not key[n].requires_grad and torch.equal(p, key[n]), n
    for on, k_ in model.model_pairs:
        assert all(not p.requires_grad for p in k_.parameters())
        assert [tuple(p.shape) for p in on.parameters()] == [tuple(p.shape) for p in k_.parameters()]
    # the English model keeps the CLIP tokenizer's constants
    from hmmc_amd.modeling import BirdPreTrainedModel
    assert (BirdPreTrainedModel.PAD_ID, BirdPreTrainedModel.CLS_ID, BirdPreTrainedModel.MASK_ID, BirdPreTrainedModel.VOCAB) == \
        (49407, 49406, 49394, 49408)


def test_vocab_ids_are_read_as_bert_tokenizer_indexes_them():
    """id = line number; a vocabulary shorter than the embedding table is allowed (vocab_size = its lines)."""
    from hmmc_amd.module_cross import bert_tokenizer_constants
    lines = ["[CLS]", "a", "[MASK]", "b c", "[PAD]", "[SEP]", "[UNK]"]
    d = R.text_dir(synth.ZH_TINY, lines)
    assert bert_tokenizer_constants(d) == {"vocab_size": 7, "pad_id": 4, "cls_id": 0, "mask_id": 2}
    with open(os.path.join(d, "vocab.txt"), "w", encoding="utf-8") as fh:      # no newline after the last token
        fh.write("\n".join(lines))
    assert bert_tokenizer_constants(d)["vocab_size"] == 7
    model = R.build(synth.TINY, synth.ZH_TINY, vocab_lines=lines, sd={})
    assert (model.PAD_ID, model.CLS_ID, model.MASK_ID, model.VOCAB) == (4, 0, 2, 7) and model.cls.decoder.weight.shape[0] == 7


@pytest.mark.parametrize("tag,dims,bdims,K,Fr", [("pretrain_zh_tiny", synth.TINY, synth.ZH_TINY, 16, 4),
                                                 ("pretrain_zh_b32", synth.VIT_B32, synth.ZH_BASE, 1024, 2)])
def test_state_dict_layout_equals_the_reference(tag, dims, bdims, K, Fr):
    man = json.load(open(os.path.join(GOLDEN, "statedict_manifest_zh_pretrain.json")))
    model = R.build(dims, bdims, contrast_num_negative=K, max_frames=Fr)
    sd, ref = model.state_dict(), man[tag]
    assert set(sd) == set(ref), sorted(set(sd) ^ set(ref))
    got = {k: [list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in sd.items()}
    assert got == ref, [k for k in ref if got[k] != ref[k]]
    assert sorted(n for n, p in model.named_parameters() if p.requires_grad) == man[tag + ":trainable"]
    src = synth.pretrain_state_zh(dims, bdims, K, Fr)
    assert all(torch.equal(sd[k], src[k]) for k in src), "the synthetic state did not load bit for bit"


def test_bad_vocabularies_are_refused_by_name():
    lines = synth.bert_vocab_lines(synth.ZH_TINY)
    with pytest.raises(ValueError, match=r"\[MASK\]"):
        R.build(synth.TINY, synth.ZH_TINY, vocab_lines=[t for t in lines if t != "[MASK]"], sd={})
    with pytest.raises(ValueError, match="word-embedding table"):
        R.build(synth.TINY, synth.ZH_TINY, vocab_lines=lines + ["extra"], sd={})


def _check_step0(g, sd, queues, loss, parts, tn, ptr, grads, slices=True):
    fam, vtm, ftm, mlm = [float(x) for x in parts]
    close(fam, g["fam0"], 1e-4, what="fam0")
    close(ftm, g["ftm0"], 1e-4, what="ftm0")
    close(mlm, g["mlm0"], 1e-4, what="mlm0")
    close(loss, g["loss0"], 1e-4, what="loss0")
    assert ptr == int(g["ptr0"][0])
    if grads is not None:
        close(tn, g["gnorm0"], 0, 2e-3, "gnorm0")
        ref = dict(zip([str(n) for n in g["grad_norm_names"]], g["grad_norm_values"]))
        assert set(grads) == {("cls.bias" if n == "cls.decoder.bias" else n) for n in ref}
        for n, gr in grads.items():
            if n.endswith("attention.self.key.bias"):
                # exactly zero in exact arithmetic: both values are rounding noise (tests/test_zh_cpu.py)
                wn = ref[n[:-4] + "weight"]
                assert float(gr.norm()) <= 1e-5 * wn and ref[n] <= 1e-5 * wn, f"grad norm {n}"
                continue
            if ref[n] < 1e-6:           # biases in front of BatchNorm: the true gradient is zero, both sides hold noise
                assert float(gr.norm()) < 1e-5, n
                continue
            assert abs(float(gr.norm()) - ref[n]) <= 2e-3 * ref[n] + 1e-7, f"grad norm {n}: {float(gr.norm())} vs {ref[n]}"
    if slices:
        for key in g.files:
            if key.startswith("s0:"):
                close(sd[key[3:]].detach().reshape(-1)[:16], g[key], 1e-5, 1e-4, key)
            if key.startswith("q0:"):
                close(queues[key[3:]][:32, :64], g[key], 1e-5, what=key)


def test_restatement_reproduces_five_reference_steps():
    g = golden("moco_zh_fp32")
    for step, sd, queues, loss, parts, tn, ptr, grads in R.run("moco_zh_fp32", g, synth.TINY, synth.ZH_TINY, "tiny", 5):
        if step == 0:
            _check_step0(g, sd, queues, loss, parts, tn, ptr, grads)
            continue
        fam, vtm, ftm, mlm = [float(x) for x in parts]
        for nm, val in (("fam", fam), ("ftm", ftm), ("mlm", mlm), ("loss", float(loss))):
            close(val, g[f"{nm}{step}"], 2e-3, what=f"{nm}{step}")
        assert ptr == int(g[f"ptr{step}"][0])
    assert ptr == 4                                     # 5 x 4 keys into 16 columns: the pointer wrapped


def test_restatement_reproduces_the_bird_step():
    g = golden("moco_zh_bird_fp32")
    for out in R.run("moco_zh_bird_fp32", g, synth.TINY, synth.ZH_TINY, "tiny", 1, bird=True):
        _check_step0(g, *out[1:])


def test_restatement_reproduces_step_0_at_true_dimensions():
    """ViT-B/32 beside BERT-base, forward only (the CPU suite's time)."""
    name, dims, bdims = "moco_zh_b32_fp32", synth.VIT_B32, synth.ZH_BASE
    g = golden(name)
    K, Fr = int(g["K"]), int(g["F"])
    sd = {k: v.clone() for k, v in synth.pretrain_state_zh(dims, bdims, K, Fr).items()}
    sd["cls.decoder.bias"] = sd["cls.bias"]
    queues = {k: sd[k] for k in sd if k.startswith("queue_") and k != "queue_ptr"}
    with torch.no_grad():
        loss, parts, ptr = R.pretrain_loss(R.batch_of(name, g, dims, bdims, "b32", 0), sd, queues, 0, K, json.loads(str(g["bert"])),
                                           R.draws_of(g, 0))
    _check_step0(g, sd, queues, loss, parts, None, ptr, None)
