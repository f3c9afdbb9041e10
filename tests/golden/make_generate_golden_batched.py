#!/usr/bin/env python3
"""Regenerates tests/golden/decoder_generate_batched_tiny.npz from the VENDORED transformers under /root/reference
(build container only): greedy `generate` (do_sample=False, use_cache=True, no eos) of the tiny Llama of
make_generate_golden.py (the weights of decoder_llama_tiny.npz, every projection scaled by 4) on two left-padded
batches wide enough for the 9..64-row decode kernels: B = 12 (16 new tokens, generator seed 21) and B = 33 (8 new
tokens, seed 23), prompts of 45 columns, left pads drawn in [0, 40) with row 0 unpadded.  Stored per batch (key suffix
_b12 / _b33): prompts, masks, generated ids, the fp32 scores of every step, and the deviation of the reference's own
bf16 run, teacher-forced on the fp32 greedy path, from them -- exactly as make_generate_golden.py computes it."""
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
from transformers import LlamaConfig, LlamaForCausalLM  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = [(12, 45, 16, 21), (33, 45, 8, 23)]          # B, S0, new tokens, generator seed


def main():
    z = np.load(os.path.join(HERE, "decoder_llama_tiny.npz"))
    cfg = LlamaConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2,
                      num_attention_heads=2, num_key_value_heads=1, max_position_embeddings=256, rms_norm_eps=1e-5,
                      rope_theta=500000.0, tie_word_embeddings=True, pad_token_id=299, initializer_range=0.05,
                      rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                    "original_max_position_embeddings": 32, "rope_type": "llama3"})
    m = LlamaForCausalLM(cfg).eval()
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    sd = {k: (v * 4.0 if "proj" in k else v) for k, v in sd.items()}
    sd["lm_head.weight"] = sd["model.embed_tokens.weight"]
    m.load_state_dict(sd)
    mb = LlamaForCausalLM(cfg).to(torch.bfloat16).eval()
    mb.load_state_dict({k: v.to(torch.bfloat16) for k, v in m.state_dict().items()})
    out = {"pad_token_id": np.int64(299)}
    for B, S0, NEW, seed in BATCHES:
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(0, 299, (B, S0), generator=g)
        pads = torch.randint(0, 40, (B,), generator=g)
        pads[0] = 0
        mask = torch.ones(B, S0, dtype=torch.long)
        for r in range(B):
            mask[r, :int(pads[r])] = 0
            ids[r, :int(pads[r])] = 299
        free = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=NEW, pad_token_id=299, use_cache=True, do_sample=False,
                          output_scores=True, return_dict_in_generate=True)
        scores = torch.stack(free.scores, 1)
        full_mask = torch.cat([mask, torch.ones(B, NEW, dtype=torch.long)], 1)
        pos = (full_mask.cumsum(-1) - 1).masked_fill(full_mask == 0, 1)
        with torch.no_grad():
            lb = mb(input_ids=free.sequences, attention_mask=full_mask, position_ids=pos).logits.float()[:, S0 - 1:-1]
        bf16_dev = (lb - scores).abs().amax(-1).numpy()
        print("B %d: reference bf16-vs-fp32 logit deviation: max %.3f mean %.3f" % (B, bf16_dev.max(), bf16_dev.mean()))
        k = "_b%d" % B
        out.update({"input_ids" + k: ids.numpy(), "attention_mask" + k: mask.numpy(), "max_new_tokens" + k: np.int64(NEW),
                    "sequences" + k: free.sequences.numpy(), "scores" + k: scores.numpy().astype(np.float32),
                    "ref_bf16_deviation" + k: bf16_dev.astype(np.float32)})
    np.savez_compressed(os.path.join(HERE, "decoder_generate_batched_tiny.npz"), **out)


if __name__ == "__main__":
    main()
