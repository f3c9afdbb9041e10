"""Mirrors of ecg_byte/runners/train.py (`trainer`, `validater`), ecg_byte/runners/inference.py (`tester`) and
ecg_byte/runners/interpret.py (`interpreter`, without its plots): same arguments, same return dicts, same checkpoint files.  Differences, all on the device side: the gradient
clip of train.py:26 is folded into `optimizer.step_and_update_lr()` (decoder.HipAdam applies the global-norm
clip to 1.0 inside the Adam kernel), and in a multi-rank run the gradients are exchanged by
`parallel.GradAllReduce` during backward instead of DDP hooks.  wandb logging is not mirrored."""
from __future__ import annotations

import re

import numpy as np
import torch
import torch.distributed as dist

from .model_utils import evaluate_strings
from .tokenizer_utils import decode_text


def _save(checkpoint, path, args):
    if getattr(args, "dis", False):
        dist.barrier()
        if dist.get_rank() == 0:
            torch.save(checkpoint, path)
    else:
        torch.save(checkpoint, path)


def trainer(model, dataloader, optimizer, args, epoch, directory_path, checkpoint_every=50000):
    """train.py:7-73"""
    model.train()
    if getattr(args, "dis", False) and hasattr(getattr(dataloader, "sampler", None), "set_epoch"):
        dataloader.sampler.set_epoch(epoch)
    total_loss, len_of_batch, dev_count = 0.0, 0, 0
    for step, batch in enumerate(dataloader):
        if batch is None:
            print(f"Skipping invalid batch at step {step}")
            continue
        try:
            optimizer.zero_grad()
            out = model(batch)
            loss = out.loss
            loss.backward()
            optimizer.step_and_update_lr()          # clip_grad_norm_(1.0) happens inside
            total_loss += loss.item()
            len_of_batch += 1
            if ((step + 1) % checkpoint_every == 0) and not getattr(args, "toy", False):
                _save({"model": model.state_dict(), "epoch": epoch}, f"{directory_path}/best_train_model_{epoch}_{step}.pth", args)
                print(f"Best model saved at epoch: {epoch+1} {step}")
            if getattr(args, "dev", False):
                dev_count += 1
                if dev_count == 10:
                    break
        except Exception as e:
            print(f"Error during training at step {step}: {e}")
            if getattr(args, "dis", False):
                # train.py:59-61 swallows the error on every rank alike; with a collective inside backward a rank that skips a
                # step leaves the others waiting in all-reduce forever, so a multi-rank run stops instead
                raise
            continue
    if len_of_batch == 0:
        print("No valid batches for training.")
        return {"average_loss": float("inf")}
    return {"average_loss": total_loss / len_of_batch}


def validater(model, dataloader, args, epoch):
    """train.py:75-117.  The loss of a batch is computed with the forward-only path (no activations kept)."""
    model.eval()
    total_loss, len_of_batch, dev_count = 0.0, 0, 0
    with torch.no_grad():
        for step, batch in enumerate(dataloader):
            if batch is None:
                print(f"Skipping invalid batch at step {step}")
                continue
            try:
                out = model(batch)
                total_loss += out.loss.item()
                len_of_batch += 1
                if getattr(args, "dev", False):
                    dev_count += 1
                    if dev_count == 10:
                        break
            except Exception as e:
                print(f"Error during validation at step {step}: {e}")
                continue
    if len_of_batch == 0:
        print("No valid batches for validation.")
        return {"average_loss": float("inf")}
    return {"average_loss": total_loss / len_of_batch}


def tester(model, dataloader, tokenizer, args, extra_metrics=None):
    """inference.py:7-78: batch-1 greedy generation, per-sample metrics, averages over the samples.  A batch that holds several answers (main's --inference_batch) is
    generated in one call (model.generate_batch) and still scored sample by sample, in dataset order; a batch whose generation fails scores zero once per sample."""
    model.eval()
    all_results, gt_answers, gen_answers, questions = [], [], [], []
    dev_count = 0
    with torch.no_grad():
        for batch in dataloader:
            if batch is None:
                print("Skipping invalid batch ")
                continue
            answer = batch["answer"]
            n_samples = len(answer) if isinstance(answer, (list, tuple)) and len(answer) > 1 else 1
            out = None
            try:
                if n_samples > 1:
                    out = list(model.generate_batch(batch, tokenizer))
                    if len(out) != n_samples:
                        raise ValueError(f"generate_batch returned {len(out)} strings for {n_samples} samples")
                    scored = [evaluate_strings([answer[k]], [out[k]], getattr(args, "device", None), extra_metrics) for k in range(n_samples)]
                    all_results.extend(scored)
                    gt_answers.extend(answer)
                    gen_answers.extend(out)
                    questions.extend(batch["question"])
                else:
                    out = [model.generate(batch, tokenizer)]
                    all_results.append(evaluate_strings(answer, out, getattr(args, "device", None), extra_metrics))
                    gt_answers.append(answer[0])
                    gen_answers.append(out[0])
                    questions.append(batch["question"][0])
            except Exception as e:
                print("could not evaluate for some reason:", str(e))
                print(f"Error type: {type(e).__name__}")
                # inference.py:34-36: a failed sample scores zero in EVERY metric, so it pulls all the averages down alike
                for _ in range(n_samples):
                    zero = {"BLEU": 0}
                    if extra_metrics is not None:
                        zero.update({"METEOR": 0, "ROUGE": {"rouge-1": 0, "rouge-2": 0, "rouge-l": 0},
                                     "BERTSCORE": {"hf-prec": [0], "hf-rec": [0], "hf-f1": [0]}})
                    all_results.append(zero)
            if getattr(args, "dev", False):
                dev_count += n_samples
                if dev_count >= 10:
                    break
    sums, counts = {}, {}
    for entry in all_results:
        for key, value in entry.items():
            if isinstance(value, dict):           # ROUGE / BERTSCORE style sub-dicts (inference.py:57-63)
                for sub_key, sub_value in value.items():
                    v = sub_value[0] if isinstance(sub_value, (list, tuple)) else sub_value
                    sums[sub_key] = sums.get(sub_key, 0) + v
                    counts[sub_key] = counts.get(sub_key, 0) + 1
            else:
                sums[key] = sums.get(key, 0) + value
                counts[key] = counts.get(key, 0) + 1
    return {"metrics": {k: sums[k] / counts[k] for k in sums},
            "qa_results": {"questions": questions, "gt_answers": gt_answers, "gen_answers": gen_answers}}


def get_component_indices(batch, tokenizer):
    """interpret.py:9-36: where the signal (after <sig_start>), the question (after <sig_end>) and the answer (first label that is
    neither -100 nor the pad id, searched from the question on) begin in the first sequence of the batch."""
    tokenized_seq = [int(t) for t in batch["tokenized_signal"][0].tolist()]
    labels = [int(t) for t in batch["quantized_signal_ids_input"][0].tolist()] if "quantized_signal_ids_input" in batch else None
    sig_start, sig_end = tokenizer.convert_tokens_to_ids("<sig_start>"), tokenizer.convert_tokens_to_ids("<sig_end>")
    signal_start = 0
    for i, t in enumerate(tokenized_seq):
        if t == sig_start:
            signal_start = i + 1
            break
    question_start = signal_start
    for i in range(signal_start, len(tokenized_seq)):
        if tokenized_seq[i] == sig_end:
            question_start = i + 1
            break
    answer_start = len(tokenized_seq)
    if labels is not None:
        for i in range(question_start, len(labels)):
            if labels[i] != -100 and labels[i] != tokenizer.pad_token_id:
                answer_start = i
                break
    return signal_start, question_start, answer_start


def expand_attention(encoded_ids, attention_sequence, vocab):
    """interpret.py:106-111: each token's attention repeated once per ECG symbol the token stands for."""
    expanded_attention = []
    for token_id, attention_value in zip(encoded_ids, attention_sequence):
        expanded_attention.extend([attention_value] * len(vocab[token_id]))
    return expanded_attention


def interpreter(model, dataloader, tokenizer, vocab, args):
    """interpret.py:38-104 without the plots: batch-1 forwards with the attention map averaged over layers and heads (the model's
    output_attentions="mean" form -- the same [S, S] as the reference's torch.stack(out.attentions).mean(dim=(0, 2))[0]), each component's
    block of it averaged over its query rows.  The reference reshapes the expanded signal attention to (12, 500) and fails on anything
    else; here it is (12, n // 12), and a sample whose n is not a multiple of 12 (a truncated signal) is skipped with a printed reason."""
    model.eval()
    signal_attentions, signal_seqs, signal_decodes = [], [], []
    question_attentions, question_seqs = [], []
    answer_attentions, answer_seqs = [], []
    previous = getattr(model, "output_attentions", False)
    model.output_attentions = "mean"
    try:
        with torch.no_grad():
            for step, batch in enumerate(dataloader):
                if batch is None:
                    continue
                signal_start, question_start, answer_start = get_component_indices(batch, tokenizer)
                out = model(batch)
                attention = torch.stack(out.attentions).mean(dim=(0, 2))[0]
                sequence = batch["tokenized_signal"][0]
                seq_len = len(sequence)
                signal_seq = sequence[signal_start:question_start]
                signal_att = attention[signal_start:question_start, signal_start:question_start].mean(dim=0)
                question_seq = sequence[question_start:answer_start]
                if len(question_seq) == 0:
                    continue
                question_att = attention[question_start:answer_start, question_start:answer_start].mean(dim=0)
                answer_seq = sequence[answer_start:seq_len - 1]
                if len(answer_seq) == 0:
                    continue
                answer_att = attention[answer_start:seq_len - 1, answer_start:seq_len - 1].mean(dim=0)

                signal_att_np = signal_att.cpu().float().numpy()
                signal_decoded = tokenizer.decode(signal_seq.cpu().numpy(), skip_special_tokens=True)
                signal_ids = [int(i) for i in re.findall(r"signal_(\d+)", signal_decoded)]
                n = len(expand_attention(signal_ids, signal_att_np, vocab))
                if n % 12:
                    print(f"Skipping sample {step}: {n} signal symbols are not 12 leads of equal length")
                    continue
                signal_seqs.append(signal_seq.cpu().numpy())
                signal_attentions.append(signal_att_np)
                question_seqs.append(question_seq.cpu().numpy())
                question_attentions.append(question_att.cpu().float().numpy())
                answer_seqs.append(answer_seq.cpu().numpy())
                answer_attentions.append(answer_att.cpu().float().numpy())
                signal_decodes.append(decode_text(signal_ids, vocab))
                if getattr(args, "dev", False) and len(signal_seqs) >= 5:
                    break
    finally:
        model.output_attentions = previous
    return {
        "signal": {"sequences": signal_seqs, "attentions": signal_attentions, "signal": signal_decodes},
        "question": {"sequences": question_seqs, "attentions": question_attentions},
        "answer": {"sequences": answer_seqs, "attentions": answer_attentions},
    }
