"""Writes tests/golden/lora_tiny.safetensors: a seeded LoRA adapter for the tiny golden DiT layout (tests/golden/dit_tiny_meta.json),
one entry per kind of key `k5_dit_add_lora` maps (include/k5.h), ranks 1..8, factors in fp32 / bf16 / fp16, some with an alpha.
peft names (`base_model.model.<module>.lora_A.weight`); everything is drawn here from torch's CPU generator.

    python tools/gen_golden_lora.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# module -> (rows, cols) symbols of the tiny config; the order fixes rank, dtype and alpha of every entry
MODULES = [
    "text_transformer_blocks.0.self_attention.to_query", "text_transformer_blocks.0.self_attention.to_key",
    "text_transformer_blocks.0.feed_forward.in_layer", "text_transformer_blocks.0.text_modulation.out_layer",
    "visual_transformer_blocks.0.self_attention.to_query", "visual_transformer_blocks.1.self_attention.to_key",
    "visual_transformer_blocks.1.self_attention.to_value", "visual_transformer_blocks.0.self_attention.out_layer",
    "visual_transformer_blocks.1.cross_attention.to_query", "visual_transformer_blocks.1.cross_attention.to_key",
    "visual_transformer_blocks.0.cross_attention.to_value", "visual_transformer_blocks.0.cross_attention.out_layer",
    "visual_transformer_blocks.1.feed_forward.in_layer", "visual_transformer_blocks.0.feed_forward.out_layer",
    "visual_transformer_blocks.1.visual_modulation.out_layer",
    "text_embeddings.in_layer", "pooled_text_embeddings.in_layer", "visual_embeddings.in_layer",
    "out_layer.out_layer", "out_layer.modulation.out_layer", "time_embeddings.in_layer", "time_embeddings.out_layer",
]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def main():
    from safetensors.torch import load_file, save_file
    shapes = {k[2:]: tuple(v.shape) for k, v in load_file(os.path.join(ROOT, "tests", "golden", "dit_tiny.safetensors")).items()
              if k.startswith("w.")}
    out = {}
    for i, m in enumerate(MODULES):
        rows, cols = shapes[m + ".weight"]
        R = 1 + (i * 3) % 8
        g = torch.Generator().manual_seed(7000 + i)
        dt = DTYPES[i % 3]
        out[f"base_model.model.{m}.lora_A.weight"] = (torch.randn(R, cols, generator=g) * 0.05).to(dt)
        out[f"base_model.model.{m}.lora_B.weight"] = (torch.randn(rows, R, generator=g) * 0.05).to(DTYPES[(i + 1) % 3])
        if i % 2:
            out[f"base_model.model.{m}.alpha"] = torch.tensor(float(R) * (0.5 + 0.25 * (i % 4)))
    path = os.path.join(ROOT, "tests", "golden", "lora_tiny.safetensors")
    save_file(out, path)
    print(json.dumps({"path": path, "tensors": len(out), "bytes": os.path.getsize(path)}))


if __name__ == "__main__":
    main()
