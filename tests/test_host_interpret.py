"""CPU tests of the interpretation runner (runners.get_component_indices / expand_attention / interpreter, mirrors of
ecg_byte/runners/interpret.py) and of the interp_analysis CLI's options."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")

SIG_START, SIG_END, PAD = 90, 91, 92


class _Tok:
    """The slice of a HF tokenizer the runner touches: ids >= 100 are signal tokens `signal_{id - 100}`."""
    pad_token_id = PAD

    def convert_tokens_to_ids(self, token):
        return {"<sig_start>": SIG_START, "<sig_end>": SIG_END, "<pad>": PAD}[token]

    def decode(self, ids, skip_special_tokens=False):
        return "".join(f"signal_{int(i) - 100}" for i in ids if int(i) >= 100)


def _batch(seq, labels=None):
    b = {"tokenized_signal": torch.tensor([seq])}
    if labels is not None:
        b["quantized_signal_ids_input"] = torch.tensor([labels])
    return b


def test_component_indices():
    from ecg_byte_amd.runners import get_component_indices
    tok = _Tok()
    seq = [PAD, PAD, 1, SIG_START, 100, 101, 102, SIG_END, 5, 6, 7, 8, 9]
    labels = [-100] * 10 + [8, 9, 2]
    assert get_component_indices(_batch(seq, labels), tok) == (4, 8, 10)
    # no <sig_start>: the signal starts at 0 and the question after <sig_end>
    assert get_component_indices(_batch([1, 100, 101, SIG_END, 5, 6], [-100] * 5 + [6]), tok) == (0, 4, 5)
    # no answer labels: the answer starts at the end of the sequence; no labels at all: the same
    assert get_component_indices(_batch(seq, [-100] * len(seq)), tok) == (4, 8, len(seq))
    assert get_component_indices(_batch(seq), tok) == (4, 8, len(seq))
    # pad labels are not answer tokens
    assert get_component_indices(_batch(seq, [-100] * 9 + [PAD, PAD, 9, 2]), tok) == (4, 8, 11)


def test_expand_attention():
    from ecg_byte_amd.runners import expand_attention
    vocab = {0: "ab", 1: "c", 2: "defg"}
    assert expand_attention([2, 0, 1, 0], [0.5, 0.25, 0.125, 1.0], vocab) == [0.5] * 4 + [0.25] * 2 + [0.125] + [1.0] * 2


class _Stub:
    """A model with LLM's surface: output_attentions set by the runner, attentions from a fixed table keyed by the batch."""

    def __init__(self, table):
        self.table, self.output_attentions, self.seen = table, False, []

    def eval(self):
        return self

    def __call__(self, batch):
        self.seen.append(self.output_attentions)
        return SimpleNamespace(attentions=self.table[int(batch["key"])])


def _numpy_interpret(att_layers, seq, s, q, a, vocab):
    """interpret.py:51-79 restated in numpy (layer-and-head mean, per-component block means over query rows)."""
    att = np.stack([x.numpy() for x in att_layers]).astype(np.float64).mean(axis=(0, 2))[0]
    n = len(seq)
    sig = att[s:q, s:q].mean(axis=0)
    que = att[q:a, q:a].mean(axis=0)
    ans = att[a:n - 1, a:n - 1].mean(axis=0)
    return sig, que, ans


def test_interpreter_matches_the_reference_slicing():
    from ecg_byte_amd.runners import interpreter
    tok = _Tok()
    vocab = {0: "abc", 1: "def", 2: "ghijkl"}           # 3 + 3 + 6 = 12 symbols: one per lead
    g = torch.Generator().manual_seed(0)
    seq = [PAD, SIG_START, 100, 101, 102, SIG_END, 5, 6, 7, 8, 9, 10]
    labels = [-100] * 9 + [9, 10, 2]
    S = len(seq)
    table, batches = [], []
    for k in range(3):
        layers = tuple(torch.rand(1, 4, S, S, generator=g).softmax(-1) for _ in range(2))
        table.append(layers)
        b = _batch(seq, labels)
        b["key"] = k
        batches.append(b)
    table.append((torch.rand(1, 1, S, S, generator=g),))        # the model's "mean" form: a 1-tuple
    b = _batch(seq, labels)
    b["key"] = 3
    batches.append(b)
    bad = _batch([SIG_START, 100, 101, SIG_END, 5, 6, 7], [-100] * 5 + [7, 2])   # 6 symbols: not 12 leads -> skipped
    bad["key"] = 0
    batches.insert(1, bad)
    model = _Stub(table)
    out = interpreter(model, batches, tok, vocab, SimpleNamespace(model="stub", dev=False))
    assert model.seen == ["mean"] * 5 and model.output_attentions is False
    assert len(out["signal"]["attentions"]) == 4
    for n, k in enumerate([0, 1, 2, 3]):
        sig, que, ans = _numpy_interpret(table[k], seq, 2, 6, 9, vocab)
        np.testing.assert_allclose(out["signal"]["attentions"][n], sig, rtol=1e-6, atol=0)
        np.testing.assert_allclose(out["question"]["attentions"][n], que, rtol=1e-6, atol=0)
        np.testing.assert_allclose(out["answer"]["attentions"][n], ans, rtol=1e-6, atol=0)
        assert out["signal"]["sequences"][n].tolist() == [100, 101, 102, SIG_END]   # the reference keeps <sig_end> in the signal block
        assert out["question"]["sequences"][n].tolist() == [5, 6, 7]
        assert out["answer"]["sequences"][n].tolist() == [8, 9]
        assert out["signal"]["signal"][n] == "abcdefghijkl"
    # --dev stops after five kept samples
    model = _Stub(table)
    out = interpreter(model, [batches[0]] * 8, tok, vocab, SimpleNamespace(model="stub", dev=True))
    assert len(model.seen) == 5 and len(out["answer"]["attentions"]) == 5


def test_interp_analysis_takes_the_reference_script_arguments():
    from ecg_byte_amd import interp_analysis
    argv = ["--model=meta-llama/Llama-3.2-1B", "--tokenizer_check=tokenizer_3500_100_mimic2", "--batch_size=1", "--pad_to_max=2046",
            "--device=cuda:3", "--toy", "--peft", "--num_merges=3500", "--bins=100", "--percentiles=./data/mimic_dataset_stats_500_unseg.npy",
            "--checkpoint=meta-llama/Llama-3.2-1B_ptb_qa_0.0001_0.9_0.99_1e-08_0.01_500_2_1_0.99_3500_100_2046_True_True",
            "--dataset=ptb_qa", "--interpret"]
    a = interp_analysis.get_args(argv)
    assert a.model == "meta-llama/Llama-3.2-1B" and a.pad_to_max == 2046 and a.batch_size == 1 and a.toy and a.peft and a.interpret
    assert a.bins == 100 and a.num_merges == 3500 and a.dataset == "ptb_qa" and a.device == "cuda:3"
    assert a.data_root == "./data" and a.runs_root == "./runs" and a.workers == 4


def test_save_result_layout(tmp_path):
    from ecg_byte_amd.interp_analysis import save_result
    res = {"signal": {"sequences": [np.arange(3)], "attentions": [np.ones(3, np.float32)], "signal": ["abc"]},
           "question": {"sequences": [np.arange(2)], "attentions": [np.zeros(2, np.float32)]},
           "answer": {"sequences": [], "attentions": []}}
    z = np.load(save_result(res, str(tmp_path / "x.npz")))
    assert sorted(z.files) == ["question/attentions/0", "question/sequences/0", "signal/attentions/0", "signal/sequences/0", "signal/signal/0"]
    assert z["signal/signal/0"].item() == "abc" and z["signal/attentions/0"].tolist() == [1, 1, 1]
