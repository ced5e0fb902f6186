"""Names shared by tests/golden/make_golden_zh_pretrain.py (which imports them) and the Chinese pre-training tests: the tensors
sampled after each optimizer step of moco_zh*_fp32.npz and the real-token counts (1 = [CLS] alone) of every step's titles / tags."""
PRETRAIN_SAMPLED = ["text_encoder_k.chinese_encoder.embeddings.word_embeddings.weight",
                    "text_encoder_k.chinese_encoder.embeddings.LayerNorm.weight",
                    "text_encoder_k.chinese_encoder.encoder.layer.0.attention.self.query.weight",
                    "text_encoder_k.chinese_encoder.encoder.layer.1.output.dense.bias",
                    "text_encoder_k.chinese_encoder.pooler.dense.weight",
                    "text_encoder_k.text_proj.weight", "text_encoder_k.text_proj.bias",
                    "visual_encoder_k.visual.conv1.weight", "v_projector_k.linear_out.weight",
                    "v_projector.linear_hidden.2.running_mean", "v_projector.linear_hidden.2.running_var",
                    "v_projector_k.linear_hidden.2.running_mean", "v_predictor.linear_hidden.2.running_var",
                    "text_encoder.chinese_encoder.encoder.layer.0.attention.self.query.weight",
                    "text_encoder.chinese_encoder.encoder.layer.1.output.LayerNorm.weight",
                    "text_encoder.chinese_encoder.embeddings.position_embeddings.weight",
                    "text_encoder.chinese_encoder.pooler.dense.bias", "text_encoder.text_proj.weight"]
PRETRAIN_LENS = {
    "tiny": {"title_len": 16, "tag_len": 9,
             "title": ([16, 1, 9, 5], [4, 16, 11, 7], [3, 16, 8, 13], [10, 2, 16, 6], [5, 12, 9, 16]),
             "tag": ([9, 2, 5, 3], [1, 9, 4, 7], [6, 3, 9, 2], [9, 9, 1, 5], [2, 8, 9, 4])},
    "b32": {"title_len": 45, "tag_len": 25, "title": ([45, 7, 19, 30], [12, 45, 3, 28]), "tag": ([25, 3, 12, 8], [5, 25, 17, 2])},
}
