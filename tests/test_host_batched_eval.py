"""runners.tester over batches that hold several answers (main's --inference_batch): one generate_batch call per batch, every sample scored on its own, a failed
batch scored zero once per sample, --dev counted in samples -- with a stub model, no GPU."""
from types import SimpleNamespace

import pytest


class _Stub:
    def __init__(self, fail_on=()):
        self.calls, self.fail_on = [], set(fail_on)

    def eval(self):
        pass

    def generate(self, batch, tokenizer):
        self.calls.append(("one", len(batch["answer"])))
        return batch["answer"][0]

    def generate_batch(self, batch, tokenizer):
        self.calls.append(("batch", len(batch["answer"])))
        if len(self.calls) in self.fail_on:
            raise RuntimeError("boom")
        # the first answer of a batch is reproduced, the others are missed
        return [a if k == 0 else "nothing in common" for k, a in enumerate(batch["answer"])]


def _batches(sizes):
    out, i = [], 0
    for n in sizes:
        out.append({"answer": [f"sinus rhythm normal ecg number {j}" for j in range(i, i + n)], "question": [f"q{j}" for j in range(i, i + n)]})
        i += n
    return out


def test_tester_scores_every_sample_of_a_batch_on_its_own():
    from ecg_byte_amd.runners import tester
    extra = lambda refs, hyps: {"ROUGE": {"rouge-1": 0.5 if len(refs) == 1 and len(hyps) == 1 else -100.0}}
    m = _Stub()
    out = tester(m, _batches([4, 3]) + [None], None, SimpleNamespace(dev=False, device="cpu"), extra_metrics=extra)
    assert m.calls == [("batch", 4), ("batch", 3)]
    assert out["metrics"]["BLEU"] == pytest.approx(2 * 1.0 / 7)             # the per-sample average: two hits in seven samples
    assert out["metrics"]["rouge-1"] == pytest.approx(0.5)                   # the extra metrics saw one reference and one hypothesis per call
    qa = out["qa_results"]
    assert qa["questions"] == [f"q{j}" for j in range(7)]                    # dataset order
    assert qa["gt_answers"] == [f"sinus rhythm normal ecg number {j}" for j in range(7)]
    assert [g == a for g, a in zip(qa["gen_answers"], qa["gt_answers"])] == [True, False, False, False, True, False, False]


def test_a_failed_batch_scores_zero_once_per_sample():
    from ecg_byte_amd.runners import tester
    extra = lambda refs, hyps: {"ROUGE": {"rouge-1": 0.5}, "BERTSCORE": {"hf-f1": [0.75]}}
    m = _Stub(fail_on=(2,))
    out = tester(m, _batches([2, 3, 1]), None, SimpleNamespace(dev=False, device="cpu"), extra_metrics=extra)
    assert m.calls == [("batch", 2), ("batch", 3), ("one", 1)]               # a one-answer batch still goes through generate
    # six samples: batch 1 scores (1, 0), the failed batch three zeros in EVERY metric, the single sample 1
    assert out["metrics"]["BLEU"] == pytest.approx(2 / 6)
    assert out["metrics"]["rouge-1"] == pytest.approx(3 * 0.5 / 6) and out["metrics"]["hf-f1"] == pytest.approx(3 * 0.75 / 6)
    assert out["metrics"]["METEOR"] == 0
    assert out["qa_results"]["questions"] == ["q0", "q1", "q5"]              # failed samples leave no question / answer pair, as a failed single sample does


def test_dev_stops_after_at_least_ten_samples():
    from ecg_byte_amd.runners import tester
    m = _Stub()
    out = tester(m, _batches([4, 4, 4, 4]), None, SimpleNamespace(dev=True, device="cpu"))
    assert m.calls == [("batch", 4)] * 3 and len(out["qa_results"]["questions"]) == 12
    m = _Stub()
    tester(m, _batches([1] * 12), None, SimpleNamespace(dev=True, device="cpu"))
    assert m.calls == [("one", 1)] * 10                                      # single prompts: ten, as before


def test_a_wrong_number_of_generated_strings_is_a_failed_batch():
    from ecg_byte_amd.runners import tester

    class Short(_Stub):
        def generate_batch(self, batch, tokenizer):
            return ["only one"]
    out = tester(Short(), _batches([3]), None, SimpleNamespace(dev=False, device="cpu"))
    assert out["metrics"]["BLEU"] == 0 and out["qa_results"]["questions"] == []
