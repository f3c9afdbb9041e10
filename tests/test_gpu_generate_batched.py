"""A decode step of 9..64 sequences on the weight-streaming kernels (HipCausalLM.decode_rows, ops.gemm_nt_rows): teacher-forced on the greedy paths of the vendored
transformers (tests/golden/make_generate_golden_batched.py) -- a free-running comparison is nearly empty on this model, most steps are near-ties at bf16 resolution --
and on the model's own recompute path for adapters and Gemma; the replayed graph against the eager loop."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from ecg_byte_amd import decoder_ops
    return decoder_ops


@pytest.fixture(scope="module")
def zb():
    return np.load(os.path.join(GOLDEN, "decoder_generate_batched_tiny.npz"))


def _llama():
    z = np.load(os.path.join(GOLDEN, "decoder_llama_tiny.npz"))
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    cfg = DecoderConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                        num_key_value_heads=1, rms_norm_eps=1e-5, rope_theta=500000.0, pad_token_id=299,
                        rope_scaling={"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                      "original_max_position_embeddings": 32, "rope_type": "llama3"})
    m = HipCausalLM(cfg)
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    m.load_state_dict({k: (v * 4.0 if "proj" in k else v) for k, v in sd.items()})   # as make_generate_golden_batched.py does
    return m.eval()


def _gemma():
    z = np.load(os.path.join(GOLDEN, "decoder_gemma_tiny.npz"))
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    cfg = DecoderConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                        num_key_value_heads=1, head_dim=128, rms_norm_eps=1e-6, rope_theta=10000.0, rope_scaling=None, pad_token_id=299,
                        model_type="gemma")
    m = HipCausalLM(cfg)
    sd = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w:")}
    m.load_state_dict({k: (v * 4.0 if "proj" in k else v) for k, v in sd.items()})   # as make_decoder_golden_gemma.py does for its generate fixture
    return m.eval()


def _walk(m, ops, ids, mask0, seqs, new):
    """Logits [B, new, V] of the cached path fed the tokens of `seqs`: the prompt through _hidden_states, then one _decode_step and the head per given token, as the
    eager loop of generate runs them."""
    B, S0 = ids.shape
    c, V = m.cfg, m.cfg.vocab_size
    cap_rows = -(-(S0 + new) // 128) * 128
    mask = torch.zeros((B, cap_rows), dtype=torch.float32, device="cuda")
    mask[:, :S0] = mask0.float()
    caches = [torch.empty((B, cap_rows, 2 * c.num_key_value_heads * c.head_dim), dtype=torch.bfloat16, device="cuda") for _ in range(c.num_hidden_layers)]

    def positions(mm):
        return (mm.long().cumsum(-1) - 1).masked_fill(mm == 0, 1)

    with torch.no_grad():
        m0 = mask[:, :S0].contiguous()
        hf = m._hidden_states(ids, m0, positions(m0), kv_out=caches)
        out = [ops.gemm_nt(hf.view(B, S0, -1)[:, -1].contiguous(), m.embed.data)[:, :V].float()]
        for t in range(1, new):
            n = S0 + t
            mask[:, n - 1] = 1.0
            last = m._decode_step(seqs[:, n - 1].contiguous(), positions(mask[:, :n])[:, -1], mask, caches, n)
            out.append(m._head_rows(last, rows=m._rows_route(B))[:, :V].float())
    return torch.stack(out, 1)


@pytest.mark.parametrize("decode_rows", [True, False], ids=["rows-kernels", "tile-kernels"])
@pytest.mark.parametrize("B", [12, 33])
def test_batched_decode_teacher_forced_vs_vendored_transformers(ops, zb, B, decode_rows):
    """Every (row, step) logit row within 1.5 x the reference's own bf16 deviation of its fp32 scores (the rule of _check_greedy), on both routes: the tile kernels'
    pass shows the yardstick is fair."""
    k = "_b%d" % B
    m = _llama()
    m.decode_rows = decode_rows
    ids, mask = torch.from_numpy(zb["input_ids" + k]).cuda(), torch.from_numpy(zb["attention_mask" + k]).cuda()
    seqs, new = torch.from_numpy(zb["sequences" + k]).cuda(), int(zb["max_new_tokens" + k])
    assert ids.shape == (B, 45) and seqs.shape == (B, 45 + new)
    before = ops.rows_calls
    got = _walk(m, ops, ids, mask, seqs, new).cpu().numpy()
    ran = ops.rows_calls - before
    assert ran == ((new - 1) * (4 * m.cfg.num_hidden_layers + 1) if decode_rows else 0), ran      # q|k|v, o, gate|up + GLU, down a layer, and the head
    tol = 1.5 * float(zb["ref_bf16_deviation" + k].max())
    err = np.abs(got - zb["scores" + k]).max(-1)                          # [B, new]
    print("B %d decode_rows %s: max deviation %.4f (tolerance %.4f)" % (B, decode_rows, err.max(), tol))
    assert (err < tol).all(), (np.argwhere(err >= tol)[:5].tolist(), float(err.max()), tol)


@pytest.mark.parametrize("which", ["llama-lora", "gemma"])
def test_batched_decode_with_adapters_and_gemma_vs_recompute(ops, zb, which):
    """The same walk against the model's own recompute path (generate(use_cache=False): 12 x 45 rows and more, the tile kernels only) on its greedy sequences."""
    if which == "gemma":
        m = _gemma()
    else:
        m = _llama()
        m.enable_lora(r=16, alpha=32, dropout=0.05, seed=3)
        g = torch.Generator(device="cuda").manual_seed(4)
        with torch.no_grad():
            for layer in m.lora:
                for site in layer.values():
                    site.B.copy_((torch.randn(site.B.shape, device="cuda", generator=g) * 0.05).to(torch.bfloat16) * site.bmask)
        m.eval()
    ids, mask = torch.from_numpy(zb["input_ids_b12"]).cuda(), torch.from_numpy(zb["attention_mask_b12"]).cuda()
    new = 16
    before = ops.rows_calls
    seqs, want = m.generate(input_ids=ids, attention_mask=mask, max_new_tokens=new, pad_token_id=299, use_cache=False, return_logits=True)
    assert ops.rows_calls == before                                      # the yardstick ran none of the kernels under test
    got = _walk(m, ops, ids, mask, seqs, new)
    assert ops.rows_calls - before >= (new - 1) * (4 * m.cfg.num_hidden_layers + 1)
    tol = 1.5 * float(zb["ref_bf16_deviation_b12"].max())
    err = (got - want).abs().amax(-1)
    print("%s: max deviation %.4f (tolerance %.4f)" % (which, float(err.max()), tol))
    assert bool((err < tol).all()), (float(err.max()), tol)


def test_batched_generate_graph_replay_equals_the_eager_loop(ops, zb):
    m = _llama()
    ids, mask = torch.from_numpy(zb["input_ids_b12"]).cuda(), torch.from_numpy(zb["attention_mask_b12"]).cuda()
    kw = dict(input_ids=ids, attention_mask=mask, max_new_tokens=16, pad_token_id=299)
    before = ops.rows_calls
    a = m.generate(use_graph=True, **kw)
    assert ops.rows_calls > before                                        # the captured step holds the rows kernels
    b = m.generate(use_graph=False, **kw)
    assert a.shape == (12, 45 + 16) and torch.equal(a, b)
    assert len(m._gen_graphs) == 1
    (key, st), = m._gen_graphs.items()
    assert key[-1] is True                                               # decode_rows is part of the key
    captured = ops.rows_calls
    assert torch.equal(m.generate(use_graph=True, **kw), a)
    assert len(m._gen_graphs) == 1 and next(iter(m._gen_graphs.values())) is st and ops.rows_calls == captured      # replayed, not captured again
    m.decode_rows = False
    c = m.generate(use_graph=True, **kw)
    assert len(m._gen_graphs) == 2 and ops.rows_calls == captured and c.shape == a.shape


def test_few_sequences_keep_their_kernels(ops):
    zg = np.load(os.path.join(GOLDEN, "decoder_generate_tiny.npz"))
    m = _llama()
    before = ops.rows_calls
    seq = m.generate(input_ids=torch.from_numpy(zg["input_ids"]).cuda(), attention_mask=torch.from_numpy(zg["attention_mask"]).cuda(), max_new_tokens=24,
                     pad_token_id=299, use_graph=False)
    assert ops.rows_calls == before and seq.shape == zg["sequences_no_eos"].shape


# ---- left-padded inference batches: assembler, loader, tester and the CLI (the small helpers of tests/test_gpu_pipeline.py, with six test records)
REPORTS = ["sinus rhythm normal ecg", "atrial fibrillation with rapid ventricular response", "sinus bradycardia otherwise normal ecg",
           "left bundle branch block", "sinus rhythm with premature ventricular complexes", "normal ecg"]
QUESTION = "Could you please help me explain my ECG?"


@pytest.fixture()
def ptb_test_dir(tmp_path):
    import json
    import pickle
    from helpers import load_tokenizer
    from ecg_byte_amd import file_utils as F
    from ecg_byte_amd import synth
    vocab, merges, pc = load_tokenizer("c1")
    x = synth.synth_ecg(6, 1000, seed=5)
    os.makedirs(tmp_path / "ecg" / "test"); os.makedirs(tmp_path / "text" / "test")
    for i in range(6):
        np.save(tmp_path / "ecg" / "test" / f"ecg_{i}_0.npy", x[i])
        (tmp_path / "text" / "test" / f"text_{i}_0.json").write_text(json.dumps(REPORTS[i]))
    F.save_percentiles(tmp_path / "percentiles.npy", pc["percentile_1"], pc["percentile_99"])
    with open(tmp_path / "tok.pkl", "wb") as f:
        pickle.dump((vocab, merges), f)
    return tmp_path


def _tokenizer(vocab):
    from helpers import WordTokenizer
    tok = WordTokenizer(QUESTION.split() + " ".join(REPORTS).split())
    tok.add_tokens([f"signal_{k}" for k in vocab.keys()])
    tok.add_tokens(["<sig_start>"], special_tokens=True)
    tok.add_tokens(["<sig_end>"], special_tokens=True)
    tok.add_special_tokens({"pad_token": "<pad>"})
    return tok


def _dataset(root):
    from types import SimpleNamespace
    from ecg_byte_amd import file_utils as F
    from ecg_byte_amd.data_loader import ECGTokenDataset
    vocab, merges = F.load_vocab_and_merges(str(root / "tok.pkl"))
    tok = _tokenizer(vocab)
    sig, txt = F.align_signal_text_files(str(root / "ecg" / "test"), str(root / "text" / "test"))
    args = SimpleNamespace(percentiles=str(root / "percentiles.npy"), dataset="ptb_500", inference=True, pad_to_max=124, dis=False, dev=False, toy=True,
                           device="cuda")
    return ECGTokenDataset(sig, txt, vocab, merges, tokenizer=tok, args=args), tok, args


def test_loader_yields_left_padded_inference_batches(ptb_test_dir):
    from ecg_byte_amd.data_loader import DeviceBatchLoader
    ds, tok, args = _dataset(ptb_test_dir)
    items = [ds[i] for i in range(len(ds))]
    assert len(items) == 6 and len({it["tokenized_signal"].numel() for it in items}) > 1      # prompts of different lengths: some rows are padded
    batches = list(DeviceBatchLoader(ds, batch_size=4))
    assert [b["tokenized_signal"].shape[0] for b in batches] == [4, 2] and len(DeviceBatchLoader(ds, batch_size=4)) == 2
    i = 0
    for b in batches:
        assert set(b) == {"answer", "question", "tokenized_signal", "attn_mask"}
        ids, am = b["tokenized_signal"].cpu(), b["attn_mask"].cpu()
        assert ids.is_cuda is False and b["tokenized_signal"].is_cuda and ids.dtype == torch.int64 and am.dtype == torch.float32 and ids.shape == am.shape
        S, longest = ids.shape[1], 0
        for k in range(ids.shape[0]):
            it = items[i]
            n = it["tokenized_signal"].numel()
            assert torch.equal(ids[k, S - n:], it["tokenized_signal"]) and torch.equal(am[k, S - n:], it["attn_mask"]), (i, k)
            assert bool((ids[k, :S - n] == tok.pad_token_id).all()) and bool((am[k, :S - n] == 0).all())
            assert b["answer"][k] == it["answer"] and b["question"][k] == it["question"]
            longest = max(longest, n)
            i += 1
        assert longest == S                                              # the longest prompt has no pad column
    for i, b in enumerate(DeviceBatchLoader(ds, batch_size=1)):           # single prompts: the dict of before, unpadded
        it = items[i]
        assert set(b) == {"answer", "question", "tokenized_signal", "attn_mask"} and b["answer"] == [it["answer"]] and b["question"] == [it["question"]]
        assert torch.equal(b["tokenized_signal"].cpu(), it["tokenized_signal"][None]) and torch.equal(b["attn_mask"].cpu(), it["attn_mask"][None])


def test_tester_over_batches_of_four(ptb_test_dir):
    from ecg_byte_amd.data_loader import DeviceBatchLoader
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    from ecg_byte_amd.llm import LLM
    from ecg_byte_amd.runners import tester
    ds, tok, args = _dataset(ptb_test_dir)
    cfg = DecoderConfig(vocab_size=len(tok), hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                        num_key_value_heads=1, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None, pad_token_id=tok.pad_token_id)
    model = LLM(HipCausalLM(cfg, seed=0), args)
    out = tester(model, DeviceBatchLoader(ds, batch_size=4), tok, args)
    want = [ds.load_host(i)[4] for i in range(len(ds))]
    assert out["qa_results"]["gt_answers"] == want and out["qa_results"]["questions"] == [QUESTION] * 6      # dataset order, one answer per sample
    assert len(out["qa_results"]["gen_answers"]) == 6 and all(isinstance(g, str) for g in out["qa_results"]["gen_answers"])
    assert set(out["metrics"]) == {"BLEU"} and 0.0 <= out["metrics"]["BLEU"] <= 1.0


def test_main_cli_inference_batch(ptb_test_dir, tmp_path):
    pytest.importorskip("transformers")
    import json
    from tokenizers import Tokenizer
    from tokenizers.models import WordLevel
    from tokenizers.pre_tokenizers import Whitespace
    from ecg_byte_amd import file_utils as F
    from ecg_byte_amd import main as M
    from ecg_byte_amd.decoder import DecoderConfig, HipCausalLM
    root = ptb_test_dir
    data = tmp_path / "data"
    os.makedirs(data / "ptb_500")
    os.rename(root / "ecg", data / "ptb_500" / "ecg")
    os.rename(root / "text", data / "ptb_500" / "text")
    os.rename(root / "tok.pkl", data / "tokenizer_c1.pkl")
    model_dir = str(tmp_path / "tiny-llama")
    words = ["<unk>", "<bos>", "<eos>"] + sorted(set("Could you please help me explain my ECG ?".split() + " ".join(REPORTS).split()))
    t = Tokenizer(WordLevel({w: i for i, w in enumerate(words)}, unk_token="<unk>"))
    t.pre_tokenizer = Whitespace()
    os.makedirs(model_dir)
    t.save(os.path.join(model_dir, "tokenizer.json"))
    with open(os.path.join(model_dir, "tokenizer_config.json"), "w") as f:
        json.dump({"tokenizer_class": "PreTrainedTokenizerFast", "bos_token": "<bos>", "eos_token": "<eos>", "unk_token": "<unk>"}, f)
    HipCausalLM(DecoderConfig(vocab_size=len(words), hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2,
                              num_key_value_heads=1, rms_norm_eps=1e-5, rope_theta=10000.0, rope_scaling=None), seed=4).save_pretrained(model_dir)
    argv = ["--device", "cuda:0", "--model", model_dir, "--dataset", "ptb_500", "--tokenizer_check", "tokenizer_c1", "--percentiles", str(root / "percentiles.npy"),
            "--pad_to_max", "124", "--data_root", str(data), "--runs_root", str(tmp_path / "runs"), "--num_merges", "1000", "--inference", "--checkpoint", "ck",
            "--inference_batch", "4"]
    args = M.get_args(argv)
    assert args.inference_batch == 4 and M.get_args(argv[:-2]).inference_batch == 1
    vocab, _ = F.load_vocab_and_merges(str(data / "tokenizer_c1.pkl"))
    model, _tok = M.build_model_and_tokenizer(args, vocab, torch.device("cuda:0"))
    ck_dir = tmp_path / "runs" / "0" / "ck"
    os.makedirs(ck_dir)
    torch.save({"model": model.state_dict(), "epoch": 0}, ck_dir / "best_model.pth")
    stats = M.main(argv)
    assert set(stats) == {"BLEU"} and len(stats["BLEU"]["raw_values"]) == 5
    files = os.listdir(ck_dir)
    assert sorted(f for f in files if f.startswith("seed_")) == sorted(f"seed_{s}_results_ptb_500.json" for s in (0, 42, 123, 456, 789))
    one = json.load(open(ck_dir / "seed_0_results_ptb_500.json"))
    assert len(one["qa_results"]["gen_answers"]) == len(one["qa_results"]["gt_answers"]) >= 1
