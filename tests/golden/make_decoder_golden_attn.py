#!/usr/bin/env python3
"""Regenerates tests/golden/decoder_attn_tiny.npz from the VENDORED transformers 4.46.0.dev0 under /root/reference (build
container only): the eager attention probabilities (`output_attentions=True`, attn_implementation="eager") of the tiny Llama
and Gemma models of decoder_llama_tiny.npz / decoder_gemma_tiny.npz, on the inputs and weights stored there (not regenerated).
Stored per model: every layer's fp32-run attentions [B, Hq, S, S], and the largest |bf16 run - fp32 run| of each layer and of the
layer-and-head mean (the yardstick of tests/test_gpu_attn_probs.py)."""
import importlib.metadata as md
import os
import sys

import numpy as np

_orig = md.version


def _fake(name):   # the vendored checkout pins older tokenizers / huggingface-hub (dependency_versions_check.py:57)
    n = name.lower().replace("_", "-")
    return {"tokenizers": "0.20.3", "huggingface-hub": "0.26.0"}.get(n) or _orig(name)


md.version = _fake
sys.path.insert(0, "/root/reference/transformers/src")
import torch  # noqa: E402
from transformers import GemmaConfig, GemmaForCausalLM, LlamaConfig, LlamaForCausalLM  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def _configs():
    llama = LlamaConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                        num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=256, rms_norm_eps=1e-5,
                        rope_theta=500000.0, tie_word_embeddings=True, pad_token_id=299, initializer_range=0.05,
                        rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                      "original_max_position_embeddings": 32, "rope_type": "llama3"})
    gemma = GemmaConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=128, max_position_embeddings=256, rms_norm_eps=1e-6, rope_theta=10000.0,
                        pad_token_id=299, initializer_range=0.05, hidden_activation="gelu_pytorch_tanh")
    return {"llama": (llama, LlamaForCausalLM, "decoder_llama_tiny.npz"), "gemma": (gemma, GemmaForCausalLM, "decoder_gemma_tiny.npz")}


def _attentions(cls, cfg, sd, z, dtype):
    cfg._attn_implementation = "eager"
    m = cls(cfg).to(dtype).eval()
    missing, unexpected = m.load_state_dict({k: v.to(dtype) for k, v in sd.items()}, strict=False)
    assert not unexpected and all(k == "lm_head.weight" for k in missing), (missing, unexpected)
    m.tie_weights()
    with torch.no_grad():
        out = m(input_ids=torch.from_numpy(z["input_ids"]), attention_mask=torch.from_numpy(z["attention_mask"]),
                position_ids=torch.from_numpy(z["position_ids"]), output_attentions=True)
    return [a.float() for a in out.attentions]


def main():
    data = {}
    for name, (cfg, cls, src) in _configs().items():
        z = np.load(os.path.join(HERE, src))
        sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
        a32 = _attentions(cls, cfg, sd, z, torch.float32)
        a16 = _attentions(cls, cfg, sd, z, torch.bfloat16)
        for i, (x, y) in enumerate(zip(a32, a16)):
            data[f"{name}/fp32/{i}"] = x.numpy()
            data[f"{name}/bf16_err/{i}"] = np.float32((y - x).abs().max().item())
        m32, m16 = torch.stack(a32).mean(dim=(0, 2)), torch.stack(a16).mean(dim=(0, 2))
        data[f"{name}/bf16_err/mean"] = np.float32((m16 - m32).abs().max().item())
        print(name, "layers", len(a32), "shape", tuple(a32[0].shape), "bf16 err", [float(data[f"{name}/bf16_err/{i}"]) for i in range(len(a32))],
              "mean", float(data[f"{name}/bf16_err/mean"]))
    np.savez_compressed(os.path.join(HERE, "decoder_attn_tiny.npz"), **data)


if __name__ == "__main__":
    main()
