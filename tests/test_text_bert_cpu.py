"""Bert / SentenceBert, PhraseEmbedder and the two phrase-embedding tools without a GPU: the restatement tests/text_bert_ref.py
against the fixture made from the real transformers BertModel, the state-dict surface, loading local directories, every limit
raising ValueError before any launch, the bucketing and order restoration of PhraseEmbedder and both tools end to end with a stub
encoder."""
import importlib.util
import json
import os
import pickle

import numpy as np
import pytest
import torch

from tests import text_bert_ref as R
from texttoaudiogrounding_amd.models.text_encoder import Bert, SentenceBert  # noqa: F401  (the feature: without it nothing here runs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG, FX = R.TINY, R.FIXTURE
VOCAB = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", "a", "dog", "barks", "rain", "falls", "car", "passes", "by"]


def _fixture(golden_dir):
    out = dict(np.load(f"{golden_dir}/text_bert.npz"))
    for case in ("mean_norm", "mean"):
        out.update({k: v for k, v in np.load(f"{golden_dir}/text_bert_{case}.npz").items() if k.startswith(case + "_f")})
    return out


@pytest.mark.parametrize("case", list(R.CASES))
def test_restatement_reproduces_the_fixture_fp64(golden_dir, case):
    fx = _fixture(golden_dir)
    ids, tps, mask = (torch.from_numpy(fx[k].astype(np.int64)) for k in ("input_ids", "token_type_ids", "attention_mask"))
    assert torch.equal(ids, R.draw_inputs(FX["R"], FX["L"], FX["input_seed"])[0])
    assert int(mask.sum(-1).min()) == 2 and int(mask[0].sum()) == FX["L"] and int(tps.max()) == 1
    mode, norm = R.CASES[case]
    st = R.draw_state(CFG, FX["state_seed"])
    mine = R.results(st, ids, tps, mask, CFG["num_attention_heads"], mode, norm, torch.float64, seed=FX["objective_seed"])
    quantities = fx["quantities"].tolist()
    assert sorted(k for k in mine if "pooler" not in k) == quantities
    for k in quantities:
        assert R.quantity_err(mine, {q: torch.from_numpy(fx[f"{case}_f64_{q}"]) for q in quantities}, k) < 1e-12, k
    assert float(mine["dmodel.pooler.dense.weight"].abs().max()) == 0.0


def test_kernel_restatements_equal_autograd_fp64():
    g = torch.Generator().manual_seed(3)
    B, L, V, D, P, T = 4, 6, 30, 16, 9, 3
    ids, tps, _ = R.draw_inputs(B, L, 2, V, T)
    leaves = [t.double().requires_grad_(True) for t in (torch.randn(V, D, generator=g), torch.randn(T, D, generator=g),
                                                         torch.randn(P, D, generator=g), torch.randn(D, generator=g),
                                                         torch.randn(D, generator=g))]
    dh = torch.randn(B * L, D, generator=g).double()
    h, xhat, rstd = R.embed_forward(ids, tps, *leaves, 1e-12)
    (h * dh).sum().backward()
    got = R.embed_backward(dh, xhat.detach(), rstd.detach(), leaves[3].detach(), ids, tps, V, T, P, -1)
    for a, leaf in zip(got, leaves):
        assert R.rel_err(a, leaf.grad) < 1e-12
    assert float(got[2][L:].abs().max()) == 0.0
    skipped = R.embed_backward(dh, xhat.detach(), rstd.detach(), leaves[3].detach(), ids, tps, V, T, P, 0)
    assert float(skipped[0][0].abs().max()) == 0.0


def test_state_dict_surface_and_strict_load(tmp_path):
    from transformers import BertConfig, BertModel
    from texttoaudiogrounding_amd.models.text_encoder import BERT_DEFAULTS, MINILM_DEFAULTS, Bert, SentenceBert
    hf = BertModel(BertConfig(**CFG))
    want = {"model." + k for k in hf.state_dict()} | {"dummy_param"}
    for enc in (Bert(None, CFG), SentenceBert(None, CFG)):
        assert set(enc.state_dict()) == want
        assert enc.embed_dim == CFG["hidden_size"] and [n for n in enc._names if "pooler" in n] == []
    assert Bert(None, dict(num_hidden_layers=1)).config["hidden_size"] == BERT_DEFAULTS["hidden_size"] == 768
    mini = SentenceBert(None, dict(num_hidden_layers=1))
    assert (mini.embed_dim, mini.config["intermediate_size"], mini.config["vocab_size"]) == (384, 1536, 30522)
    assert MINILM_DEFAULTS["num_hidden_layers"] == 6 and mini.pooling == "mean" and mini.normalize
    # a BertModel.save_pretrained directory: configuration and weights are copied, strict load
    hf.save_pretrained(tmp_path / "bert")
    enc = Bert(str(tmp_path / "bert"))
    assert enc.config["hidden_size"] == 64 and enc.config["type_vocab_size"] == 2
    for k, v in hf.state_dict().items():
        assert torch.equal(enc.state_dict()["model." + k], v), k
    # a reference checkpoint (with or without the index buffers) loads strictly; load_pretrained is a no-op
    st = {"model." + k: v for k, v in hf.state_dict().items()}
    st["dummy_param"] = torch.zeros(1)
    fresh = Bert(None, CFG)
    fresh.load_state_dict(dict(st, **{"model.embeddings.position_ids": torch.arange(72)[None]}), strict=True)
    assert fresh.load_pretrained("x", print) is None
    with pytest.warns(UserWarning, match="no/such/model-anywhere.*RANDOMLY"):                 # does not resolve locally: says so
        assert Bert("no/such/model-anywhere", CFG).config["hidden_size"] == 64
    with pytest.warns(UserWarning, match="not a local sentence-transformers directory"):
        SentenceBert("all-MiniLM-L6-v2", CFG)
    # built from a configuration: BertPreTrainedModel's initialisation
    w = Bert(None, CFG).model
    assert 0.015 < float(w.encoder.layer[0].intermediate.dense.weight.detach().std()) < 0.025
    assert float(w.embeddings.word_embeddings.weight[0].abs().max()) == 0.0 and float(w.pooler.dense.bias.abs().max()) == 0.0
    assert torch.equal(w.embeddings.LayerNorm.weight, torch.ones(64))
    # through a parent module, strictly, with the index buffers in the checkpoint (the load pre-hook runs under any prefix)
    parent = torch.nn.Module()
    parent.text_encoder, parent.proj = Bert(None, CFG), torch.nn.Linear(2, 2)
    whole = {"text_encoder." + k: v for k, v in st.items()}
    whole.update({"text_encoder.model.embeddings.position_ids": torch.arange(72)[None],
                  "text_encoder.model.embeddings.token_type_ids": torch.zeros(1, 72, dtype=torch.long)})
    whole.update({"proj." + k: v for k, v in parent.proj.state_dict().items()})
    res = parent.load_state_dict(whole, strict=True)
    assert not res.missing_keys and not res.unexpected_keys and len(whole) == len(st) + 4      # (the caller's dict is not touched)
    assert torch.equal(parent.text_encoder.model.pooler.dense.weight, st["model.pooler.dense.weight"])


def _sbert_dir(tmp_path, pooling, normalize=True, nested=False):
    from transformers import BertConfig, BertModel, BertTokenizerFast
    d = tmp_path / f"sbert_{sorted(pooling.items())}_{normalize}_{nested}".replace(" ", "").replace("'", "")[:80]
    root = d / "0_Transformer" if nested else d
    os.makedirs(root, exist_ok=True)
    BertModel(BertConfig(**dict(CFG, vocab_size=len(VOCAB)))).save_pretrained(root)
    (root / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    BertTokenizerFast(str(root / "vocab.txt")).save_pretrained(root)
    mods = [{"idx": 0, "name": "0", "path": "0_Transformer" if nested else "", "type": "sentence_transformers.models.Transformer"},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
    if normalize:
        mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
    (d / "modules.json").write_text(json.dumps(mods))
    os.makedirs(d / "1_Pooling", exist_ok=True)
    base = dict(word_embedding_dimension=64, pooling_mode_cls_token=False, pooling_mode_mean_tokens=False,
                pooling_mode_max_tokens=False, pooling_mode_mean_sqrt_len_tokens=False)
    (d / "1_Pooling" / "config.json").write_text(json.dumps(dict(base, **pooling)))
    (root / "sentence_bert_config.json").write_text(json.dumps({"max_seq_length": 7, "do_lower_case": False}))
    return str(d)


def test_sentence_bert_reads_a_local_directory(tmp_path):
    from texttoaudiogrounding_amd.models.text_encoder import SentenceBert
    a = SentenceBert(_sbert_dir(tmp_path, {"pooling_mode_mean_tokens": True}))
    assert (a.pooling, a.normalize, a.max_seq_length, a.config["vocab_size"]) == ("mean", True, 7, len(VOCAB))
    b = SentenceBert(_sbert_dir(tmp_path, {"pooling_mode_cls_token": True}, normalize=False, nested=True))
    assert (b.pooling, b.normalize, b.max_seq_length) == ("cls", False, 7)
    tok = b._tokenize(["a dog barks", "rain falls a dog barks a car passes by"])
    assert tok["input_ids"].shape == (2, 7) and tok["attention_mask"][0].tolist() == [1, 1, 1, 1, 1, 0, 0]
    for bad in ({"pooling_mode_max_tokens": True}, {"pooling_mode_mean_tokens": True, "pooling_mode_cls_token": True}, {}):
        with pytest.raises(ValueError, match="pooling modes"):
            SentenceBert(_sbert_dir(tmp_path, bad))
    with pytest.raises(ValueError, match="'mean' and 'cls'"):
        SentenceBert(None, CFG, pooling="max")
    with pytest.raises(RuntimeError, match="tokenizer"):
        SentenceBert(None, CFG)(["a dog"])


def test_limits_raise_value_error_before_any_launch():
    from texttoaudiogrounding_amd import ops
    from texttoaudiogrounding_amd.models.text_encoder import Bert, SentenceBert
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder, RetrievalTextEncoder
    enc = Bert(None, CFG)                                          # CPU parameters: nothing below may reach a launch
    ones = lambda *s: torch.ones(*s, dtype=torch.long)             # noqa: E731
    for L in (1, 65):
        with pytest.raises(ValueError, match="2 ... 64 tokens"):
            enc({"input_ids": ones(2, L), "token_type_ids": ones(2, L) * 0, "attention_mask": ones(2, L)})
    small = Bert(None, dict(CFG, max_position_embeddings=8))
    with pytest.raises(ValueError, match="max_position_embeddings is 8"):
        small({"input_ids": ones(2, 9), "token_type_ids": ones(2, 9) * 0, "attention_mask": ones(2, 9)})
    with pytest.raises(ValueError, match="right-padded prefix"):
        enc({"input_ids": ones(2, 4), "token_type_ids": ones(2, 4) * 0, "attention_mask": torch.tensor([[1, 1, 1, 0], [1, 0, 1, 0]])})
    with pytest.raises(ValueError, match="differ in shape"):
        enc({"input_ids": ones(2, 4), "token_type_ids": ones(2, 5), "attention_mask": ones(2, 4)})
    with pytest.raises(ValueError, match="token_type_ids span"):
        enc({"input_ids": ones(2, 4), "token_type_ids": ones(2, 4) * 2, "attention_mask": ones(2, 4)})
    for bad in (dict(hidden_size=60, num_attention_heads=4), dict(hidden_size=96, num_attention_heads=2),
                dict(hidden_size=2048, num_attention_heads=32), dict(type_vocab_size=17), dict(num_hidden_layers=0)):
        for cls in (Bert, SentenceBert):
            with pytest.raises(ValueError):
                cls(None, dict(CFG, **bad))
    with pytest.raises(ValueError, match="2 ... 64 tokens"):
        ops.text_bert_check(64, 4, 65)
    with pytest.raises(ValueError, match="max_position_embeddings"):
        ops.text_bert_check(64, 4, 12, P=10)
    with pytest.raises(ValueError, match="pooling mode"):
        ops.text_bert_check(64, 4, pool_mode=2)
    with pytest.raises(ValueError, match="normalisation"):
        ops.text_bert_check(64, 4, norm=3)
    with pytest.raises(ValueError, match="forward-only"):
        ops.text_bert_check(64, 4, norm=2, need_grad=True)
    with pytest.raises(ValueError, match="5 \\+ 16 per layer"):
        ops.text_bert_layers(12)
    assert ops.text_bert_layers(5 + 32) == (2, False) and ops.text_bert_layers(5 + 32 + 2) == (2, True)
    assert ops.text_bert_param_names(2, pooler=False) == R.param_names(2)
    assert ops.text_bert_param_names(2) == R.param_names(2, pooler=True)
    with pytest.raises(ValueError):
        PhraseEmbedder(None, None, max_length=65)
    with pytest.raises(ValueError, match="1024"):
        RetrievalTextEncoder(CFG, shared_dim=2048)
    # the host-resident inputs are refused by the device check, not computed on the CPU
    ids, tps, mask = R.draw_inputs(3, 5, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc({"input_ids": ids, "token_type_ids": tps, "attention_mask": mask})


def test_operators_symbols_and_runner_key():
    import texttoaudiogrounding_amd.torch_ops as T
    from torch._subclasses.fake_tensor import FakeTensorMode
    from texttoaudiogrounding_amd import lib, ops, runner
    for name in ("text_bert", "text_bert_backward"):
        assert name in T.OP_NAMES
        assert str(getattr(torch.ops.tag, name).default._schema).startswith(f"tag::{name}(")
    for name in ("tag_text_bert_embed_forward", "tag_text_bert_embed_backward", "tag_text_bert_embed_backward_ws_bytes",
                 "tag_text_bert_pool_forward", "tag_text_bert_pool_backward"):
        assert name in lib.declared_symbols(), name
    for name in ("TextBertFunction", "text_bert_forward", "text_bert_backward", "text_bert_embed_forward", "text_bert_embed_backward",
                 "text_bert_pool_forward", "text_bert_pool_backward", "text_bert_check", "text_bert_param_names"):
        assert hasattr(ops, name), name
    assert "token_type_ids" in runner._INT64_KEYS
    R_, L, D, H = 6, 5, CFG["hidden_size"], CFG["num_attention_heads"]
    with FakeTensorMode():
        ps = [torch.empty(*s, requires_grad=True) for s in R.param_shapes(CFG)]
        ids = torch.empty(R_, L, dtype=torch.long)
        for tps in (ids, None):
            tok, seq, saved = torch.ops.tag.text_bert(ids, tps, ids, ps, H, 1e-12, 0, 1, 1, 0.1, 0.1, 3, True)
            assert tok.shape == (R_, L, D) and seq.shape == (R_, D) and len(saved) == 4 + 11 * 2
            (tok.sum() + seq.sum()).backward()
            assert all(p.grad.shape == p.shape for p in ps)
        out = torch.ops.tag.text_bert(ids, None, ids, [p.detach() for p in ps], H, 1e-12, 0, 0, 2, 0.0, 0.0, 0, False)
        assert out[2] == [] and out[1].shape == (R_, D)


def test_library_argument_checks():
    from texttoaudiogrounding_amd import lib
    h = lib.load()
    one = 16                                                      # any non-null pointer value: the checks come before any use
    err = lambda: b"argument check failed" in h.tag_last_error()  # noqa: E731
    ok = dict(ids=one, tps=None, word=one, typ=one, pos=one, g=one, b=one, h=one, xhat=one, rstd=one, B=2, L=5, D=64, V=120, T=2, P=72)

    def fwd(**kw):
        a = dict(ok, **kw)
        return h.tag_text_bert_embed_forward(a["ids"], a["tps"], a["word"], a["typ"], a["pos"], a["g"], a["b"], 1e-12, a["h"],
                                             a["xhat"], a["rstd"], a["B"], a["L"], a["D"], a["V"], a["T"], a["P"], None)
    for bad in (dict(ids=None), dict(word=None), dict(typ=None), dict(pos=None), dict(g=None), dict(b=None), dict(h=None),
                dict(xhat=None), dict(B=0), dict(L=0), dict(D=0), dict(D=1025), dict(V=0), dict(T=0), dict(P=4)):
        assert fwd(**bad) == -1 and err(), bad
    okb = dict(dh=one, xhat=one, rstd=one, g=one, ids=one, tps=None, dword=one, dtype=one, dpos=one, dg=one, db=one, B=2, L=5, D=64,
               V=120, T=2, P=72, pad=0, ws=one)

    def bwd(**kw):
        a = dict(okb, **kw)
        return h.tag_text_bert_embed_backward(a["dh"], a["xhat"], a["rstd"], a["g"], a["ids"], a["tps"], a["dword"], a["dtype"],
                                              a["dpos"], a["dg"], a["db"], a["B"], a["L"], a["D"], a["V"], a["T"], a["P"], a["pad"],
                                              a["ws"], None)
    for bad in (dict(dh=None), dict(xhat=None), dict(rstd=None), dict(g=None), dict(ids=None), dict(ws=None),
                dict(dword=None, dtype=None, dpos=None, dg=None, db=None), dict(B=0), dict(L=0), dict(D=1025), dict(V=0), dict(T=0),
                dict(T=17), dict(P=4)):
        assert bwd(**bad) == -1 and err(), bad
    ws = h.tag_text_bert_embed_backward_ws_bytes
    assert ws(0, 5, 64, 2) == 0 and ws(2, 5, 1025, 2) == 0 and ws(2, 5, 64, 17) == 0 and ws(2, 5, 64, 2) > 0
    for bad in ((None, one, 1, 0, one, one, 3, 4, 64), (one, None, 1, 0, one, one, 3, 4, 64), (one, one, 2, 0, one, one, 3, 4, 64),
                (one, one, 1, 3, one, one, 3, 4, 64), (one, one, 1, 0, one, None, 3, 4, 64), (one, one, 1, 0, one, one, 0, 4, 64),
                (one, one, 1, 0, one, one, 3, 4, 1025)):
        assert h.tag_text_bert_pool_forward(*bad, None) == -1 and err(), bad
    for bad in ((None, None, one, one, 1, 0, one, 3, 4, 64), (one, one, None, one, 1, 1, one, 3, 4, 64),
                (one, one, one, one, 1, 2, one, 3, 4, 64), (one, one, one, None, 1, 0, one, 3, 4, 64),
                (one, one, one, one, 1, 0, None, 3, 4, 64), (one, one, one, one, 1, 0, one, 3, 0, 64)):
        assert h.tag_text_bert_pool_backward(*bad, None) == -1 and err(), bad
    src = os.path.join(ROOT, "texttoaudiogrounding_amd", "csrc")
    for f in ("text_bert.hip", "text_rows.h"):
        assert "atomic" not in open(os.path.join(src, f)).read().replace("no atomics", "")
    assert "tc_scatter_rows_kernel" not in open(os.path.join(src, "text_clap.hip")).read().split("extern \"C\"")[0]


# ---------------------------------------------------------------------------------------------- phrase embeddings
class StubEncoder:
    """seq_emb = [number of valid tokens, sum of valid ids, padded length, batch size]: shows what each batch looked like."""
    embed_dim = 4

    def __init__(self):
        self.shapes = []

    def __call__(self, batch):
        assert not torch.is_grad_enabled()
        ids, mask = batch["input_ids"], batch["attention_mask"]
        assert batch["token_type_ids"].shape == ids.shape
        self.shapes.append(tuple(ids.shape))
        B, L = ids.shape
        return {"seq_emb": torch.stack([mask.sum(-1), (ids * mask).sum(-1), torch.full((B,), L), torch.full((B,), B)], -1).float()}


def _tokenizer(tmp_path):
    from transformers import BertTokenizerFast
    (tmp_path / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    return BertTokenizerFast(str(tmp_path / "vocab.txt"), do_lower_case=True)


def test_phrase_embedder_buckets_and_restores_order(tmp_path):
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    tok = _tokenizer(tmp_path)
    phrases = ["a dog barks", "rain", "a car passes by a dog", "rain falls", "a dog barks a car passes by rain falls", "dog"]
    lens = [len(tok(p)["input_ids"]) for p in phrases]
    assert lens == [5, 3, 8, 4, 11, 3]
    assert PhraseEmbedder.plan(lens, 16) == [[1, 5, 3], [0, 2], [4]]
    assert PhraseEmbedder.plan(lens, 1000) == [[1, 5, 3, 0, 2, 4]]
    assert PhraseEmbedder.plan([], 16) == []
    enc = StubEncoder()
    out = PhraseEmbedder(enc, tok, batch_tokens=16).encode(phrases)
    assert out.dtype == np.float32 and out.shape == (6, 4)
    assert enc.shapes == [(3, 4), (2, 8), (1, 11)]            # padded to each batch's own longest phrase
    assert out[:, 0].tolist() == lens and out[:, 2].tolist() == [8, 4, 8, 4, 11, 4] and out[:, 3].tolist() == [2, 3, 2, 3, 1, 3]
    assert out[:, 1].tolist() == [float(sum(tok(p)["input_ids"])) for p in phrases]
    cut = PhraseEmbedder(StubEncoder(), tok, batch_tokens=64, max_length=6).encode(phrases)
    assert cut[:, 0].tolist() == [5, 3, 6, 4, 6, 3]
    assert PhraseEmbedder(StubEncoder(), tok).encode([]).shape == (0, 4)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name + "_tool", os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


class _LabelEncoder:
    classes_ = np.array(["Dog", "Rain", "Car passing by"])


LABEL_JSON = [{"audio_id": "a.wav", "phrases": [{"phrase": "a dog barks", "segments": [[0.0, 1.0]]}, {"phrase": "rain falls"}]},
              {"audio_id": "b.wav", "phrases": [{"phrase": "rain falls"}, {"phrase": "a car passes by"}]},
              {"audio_id": "c.wav", "phrases": [{"phrase": "a dog barks"}, {"phrase": "dog"}]}]


def _check_table(path, keys):
    with open(path, "rb") as f:
        table = pickle.load(f)
    assert list(table) == keys
    assert all(v.dtype == np.float32 and v.shape == (4,) for v in table.values())
    return table


def test_both_tools_end_to_end_with_a_stub_encoder(tmp_path):
    from texttoaudiogrounding_amd.utils.text_embed import PhraseEmbedder
    tok = _tokenizer(tmp_path)
    emb = PhraseEmbedder(StubEncoder(), tok, batch_tokens=16)
    label_json, enc_pkl = str(tmp_path / "label.json"), str(tmp_path / "label_encoder.pkl")
    with open(label_json, "w") as f:
        json.dump(LABEL_JSON, f)
    with open(enc_pkl, "wb") as f:
        pickle.dump(_LabelEncoder(), f)
    phrases = ["a dog barks", "rain falls", "a car passes by", "dog"]
    # sentence-transformers tool
    sb = _tool("prepare_phrase_sbert")
    out = str(tmp_path / "sbert_phrase.pkl")
    sb.main(sb.build_parser().parse_args(["phrase", "--input", label_json, "--output", out]), emb)
    table = _check_table(out, phrases)
    assert table["dog"].tolist()[0] == 3.0 and table["a car passes by"].tolist()[0] == 6.0
    with open(out, "wb") as f:
        pickle.dump({k: table[k] for k in phrases[:2]}, f)
    sb.main(sb.build_parser().parse_args(["check_add_missing", "--label", label_json, "--phrase_emb", out]), emb)
    again = _check_table(out, phrases)
    assert all(np.array_equal(again[k][:2], table[k][:2]) for k in phrases)
    lab = str(tmp_path / "sbert_label.pkl")
    sb.main(sb.build_parser().parse_args(["label", "--input", enc_pkl, "--output", lab]), emb)
    _check_table(lab, ["Dog", "Rain", "Car passing by"])
    args = sb.build_parser().parse_args(["phrase", "--input", "i", "--output", "o"])
    assert (args.model_type, args.device, args.debug) == ("all-MiniLM-L6-v2", "cuda:0", False)
    # retrieval-model tool
    cl = _tool("prepare_phrase_clap")
    out2 = str(tmp_path / "clap_phrase.pkl")
    cl.main(cl.build_parser().parse_args(["phrase", "--experiment_path", "e", "--phrase_input", label_json, "--output", out2]), emb)
    _check_table(out2, phrases)
    extra = tmp_path / "extra.txt"
    extra.write_text("rain\na dog\n")
    out3 = str(tmp_path / "clap_more.pkl")
    cl.main(cl.build_parser().parse_args(["add_phrase", "--experiment_path", "e", "--extra_phrase", str(extra), "--phrase_emb", out2,
                                          "--output", out3]), emb)
    _check_table(out3, phrases + ["rain", "a dog"])
    lab2 = str(tmp_path / "clap_label.pkl")
    cl.main(cl.build_parser().parse_args(["label", "--experiment_path", "e", "--label_encoder_input", enc_pkl, "--output", lab2]), emb)
    labels = _check_table(lab2, ["Dog", "Rain", "Car passing by"])
    args = cl.build_parser().parse_args(["phrase", "--experiment_path", "e", "--phrase_input", "i", "--output", "o", "--with_proj",
                                         "--batch_size", "32"])
    assert args.with_proj and args.batch_size == 32
    # the pickles are what tools/map_phrase_to_event.py reads: its own host-side loading (utils.label_map.stack_embeddings, called
    # by its phrase_table) accepts them as they are.  The device half of that tool on these pickles: tests/test_gpu_text_bert.py
    from texttoaudiogrounding_amd.utils.label_map import stack_embeddings
    mp = _tool("map_phrase_to_event")
    margs = mp.build_parser().parse_args(["--phrase_emb", out3, "--label_emb", lab2, "--output", str(tmp_path / "o.tsv")])
    with open(margs.phrase_emb, "rb") as f:
        x = stack_embeddings(pickle.load(f))
    with open(margs.label_emb, "rb") as f:
        e = stack_embeddings(pickle.load(f))
    assert x.shape == (6, 4) and e.shape == (3, 4) and x.dtype == e.dtype == np.float32
    assert np.array_equal(e, np.stack(list(labels.values())))


def test_retrieval_text_encoder_loads_only_the_text_side(tmp_path):
    from texttoaudiogrounding_amd.utils.text_embed import RetrievalTextEncoder, _bert_config_from_state
    st = R.draw_state(CFG, 3)
    ckpt = {"text_encoder." + k: v for k, v in st.items()}
    ckpt.update({"text_proj.weight": torch.randn(48, 64), "text_proj.bias": torch.zeros(48), "audio_encoder.fc.weight": torch.zeros(3),
                 "audio_proj.weight": torch.zeros(2), "audio_proj.bias": torch.zeros(2), "logit_scale": torch.zeros(())})
    got = _bert_config_from_state(ckpt, "text_encoder.model.")
    assert got == {k: CFG[k] for k in got} and "num_attention_heads" not in got
    enc = RetrievalTextEncoder(CFG, 48, with_proj=True)
    assert enc.load_retrieval_state_dict(ckpt) == 4 and enc.embed_dim == 48
    assert torch.equal(enc.text_encoder.model.pooler.dense.weight, st["model.pooler.dense.weight"])
    with pytest.raises(RuntimeError, match="Missing key"):
        enc.load_retrieval_state_dict({k: v for k, v in ckpt.items() if k != "text_proj.bias"})


def test_retrieval_text_encoder_from_experiment(tmp_path, capsys):
    from transformers import BertConfig, BertTokenizerFast
    from texttoaudiogrounding_amd.utils.text_embed import RetrievalTextEncoder
    tok_dir, bert_dir = tmp_path / "tok", tmp_path / "bert"
    os.makedirs(tok_dir)
    (tok_dir / "vocab.txt").write_text("\n".join(VOCAB) + "\n")
    BertTokenizerFast(str(tok_dir / "vocab.txt")).save_pretrained(tok_dir)
    BertConfig(**CFG).save_pretrained(bert_dir)
    st = R.draw_state(CFG, 3)
    ckpt = {"text_encoder." + k: v for k, v in st.items()}
    ckpt.update({"text_proj.weight": torch.randn(48, 64), "text_proj.bias": torch.zeros(48), "audio_encoder.fc.weight": torch.zeros(3),
                 "logit_scale": torch.zeros(())})
    os.makedirs(tmp_path / "exp" / "models")
    torch.save({"state_dict": ckpt}, tmp_path / "exp" / "models" / "trained_model.pth")
    config = {"model": {"text_encoder": {"type": "Bert", "args": {"model_type": str(bert_dir)}}},
              "data_loader": {"collate_fn": {"args": {"tokenizer_type": str(tok_dir), "max_text_length": 30}}}}
    (tmp_path / "exp" / "models" / "config.json").write_text(json.dumps(config))
    enc, tok, got = RetrievalTextEncoder.from_experiment(str(tmp_path / "exp"), with_proj=True, device="cpu")
    assert "dropped 2 audio-side keys of" in capsys.readouterr().out and enc.dropped_keys == 2
    assert got == config and not enc.training and enc.with_proj and enc.embed_dim == 48
    assert enc.text_encoder.config["num_attention_heads"] == 4 and enc.text_encoder.config["num_hidden_layers"] == 2
    assert tok(["a dog"])["input_ids"] == [[2, 5, 6, 3]]
    # the model_type does not resolve: BERT's head_dim 64
    config["model"]["text_encoder"]["args"]["model_type"] = "no/such/model"
    (tmp_path / "exp" / "models" / "config.json").write_text(json.dumps(config))
    enc, _, _ = RetrievalTextEncoder.from_experiment(str(tmp_path / "exp"), device="cpu")
    assert enc.text_encoder.config["num_attention_heads"] == 1 and enc.embed_dim == 64
