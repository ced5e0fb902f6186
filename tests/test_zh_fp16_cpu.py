"""CPU checks of the fp16 regime of the Chinese text encoder: the dtype layout module_cross.convert_bert_weights produces,
module_cross.bert_regime on the layouts it must tell apart, and how far the regime's plain-torch restatement
(tests/bert16_ref.py) is from the fp64 definition (tests/bert_ref.py) on the same fp16-rounded weights."""
import json

import pytest
import torch

import bert16_ref
import bert_ref
from conftest import golden
from hmmc_amd import synth
from zh_common import build


def _encoder():
    return build(synth.TINY, synth.ZH_TINY).text_encoder


def test_convert_bert_weights_layout_per_parameter_name():
    from hmmc_amd.module_cross import bert_regime, convert_bert_weights
    enc = _encoder()
    keys = set(enc.state_dict())
    assert bert_regime(enc) == torch.float32
    assert convert_bert_weights(enc) is enc
    for name, p in enc.named_parameters():
        fixed = "embeddings." in name or "LayerNorm." in name
        assert p.dtype == (torch.float32 if fixed else torch.float16), name
    halves = [n for n, p in enc.named_parameters() if p.dtype == torch.float16]
    per_layer = 6 * 2                                # query, key, value, attention.output.dense, intermediate.dense, output.dense
    assert len(halves) == synth.ZH_TINY.num_hidden_layers * per_layer + 2 + 2       # + pooler.dense + text_proj
    assert "text_proj.weight" in halves and "chinese_encoder.pooler.dense.bias" in halves
    assert set(enc.state_dict()) == keys, "conversion must not change the state_dict's keys"
    assert bert_regime(enc) == torch.float16


def test_bert_regime_refuses_other_layouts_by_naming_the_helper():
    from hmmc_amd.module_cross import bert_regime, convert_bert_weights
    with pytest.raises(TypeError, match="convert_bert_weights"):
        bert_regime(_encoder().half())               # LayerNorms and embeddings halved too
    enc = convert_bert_weights(_encoder())
    lin = enc.chinese_encoder.encoder.layer[1].intermediate.dense
    lin.weight.data = lin.weight.data.float()        # one Linear left behind
    with pytest.raises(TypeError, match="convert_bert_weights"):
        bert_regime(enc)
    with pytest.raises(ValueError, match="chinese"):
        convert_bert_weights(torch.nn.Linear(2, 2))


@pytest.mark.parametrize("want,measured", [("feat", 7.52e-4), ("hidden", 6.65e-4)])
def test_restatement_stays_close_to_fp64_on_the_rounded_weights(want, measured):
    """Relative L2 of bert16_ref's forward against bert_ref in fp64, both on tests/golden/zh_tiny_fp32's inputs and the
    fp16-rounded weights.  Measured on the CPU: feat 7.52e-4, hidden 6.65e-4 (about one fp16 ulp, 4.9e-4, after two layers
    of roundings); the assertion is twice that."""
    g = golden("zh_tiny_fp32")
    B, L = int(g["B"]), int(g["L"])
    cfg = json.loads(str(g["bert"]))
    sd = bert16_ref.convert_state(synth.bert_state(synth.ZH_TINY))
    ids, mask = synth.zh_token_ids("zh_tiny_fp32.query_ids", B, L, synth.ZH_TINY.vocab_size, lens=[int(x) for x in g["lens"]])
    with torch.no_grad():
        ref = bert_ref.text_encoder({k: v.double() for k, v in sd.items()}, ids, mask, cfg, want=want)
    dout = torch.zeros(ref.shape)
    got, _ = bert16_ref.text_encoder(sd, ids, mask, cfg, dout, want=want)
    rel = float((got.double() - ref).norm() / ref.norm())
    print(f"[zh16-cpu] {want}: relative L2 of the restatement against fp64 {rel:.3e}")
    assert rel <= 2.0 * measured, (want, rel)
