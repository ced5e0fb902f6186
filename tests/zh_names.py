"""Names shared by tests/golden/make_golden_zh.py (which imports them) and tests/test_gpu_zh.py: the weights sampled after each optimizer step of zh_train_ft_fp32.npz and the real-token counts of its four batches."""
SAMPLED = ["text_encoder.text_proj.weight", "text_encoder.chinese_encoder.pooler.dense.bias",
           "text_encoder.chinese_encoder.encoder.layer.0.attention.self.query.weight",
           "text_encoder.chinese_encoder.encoder.layer.1.output.LayerNorm.weight",
           "text_encoder.chinese_encoder.embeddings.position_embeddings.weight",
           "visual_encoder.visual.conv1.weight", "visual_encoder.temporal_transformer.resblocks.2.attn.in_proj_weight"]
TRAIN_LENS = ([16, 4, 11, 7], [3, 16, 8, 13], [10, 2, 16, 6], [5, 12, 9, 16])
