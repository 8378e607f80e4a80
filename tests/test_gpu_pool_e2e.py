"""GPU: sub-token pooling and layer selection of FROZEN TransformerWordEmbeddings in the stacked tagger, end to end, on two tiny
encoders: A (sentencepiece-style tokenizer) with pooling_operation='mean', layers='-1,-2'; B (BERT-style tokenizer, which drops
control-character words) with pooling_operation='first_last', layers='all', use_scalar_mix=True.

  (a) each block of _stack_input's X equals tests/poolref.py applied to that encoder's own hidden states (read back from enc.acts)
      through the host tables, under poolref.check; padding rows are zero; and every one of those buffers IS the hidden state of its
      layer: compared with the torch oracle encoder (oracle/encoder.py) on the same weights and ids;
  (b) a tagger with 'first' / '-1' issues exactly the library calls of the producers' composition written out (encoder_forward +
      kbner_gather_rows_ld) and never kbner_pool_rows_layers;
  (c) with the feature store open ("gpu") a second visit returns X bit for bit and launches no producer;
  (d) forward_backward on the pooled features: a finite loss, and the head's gradient against float64 autograd of the same head on the
      same X passes selftest.TRAIN_TOL["delta_cos_min"] (the comparison of tests/test_gpu_stack_train.py);
  (e) ModelFinetuner, one epoch, from a YAML with pooling_operation: mean and layers: -1,-2: trains, writes stack-model.pt, and
      train.py --test reloads it."""
import os

import numpy as np
import pytest
import torch

import lstmbwdref as R
import poolref as pr
import selftest

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


class Calls:
    """records the name of every library call, and counts the encoder passes"""

    def __init__(self, monkeypatch):
        from kbner import engine
        from kbner import lib as L
        self.names, self.encoders = [], 0
        call, enc = L.call, engine.Tagger.encoder_forward

        def spy(name, *a):
            self.names.append(name)
            return call(name, *a)

        def encoder_forward(this, *a, **k):
            self.encoders += 1
            return enc(this, *a, **k)
        monkeypatch.setattr(L, "call", spy)
        monkeypatch.setattr(engine.Tagger, "encoder_forward", encoder_forward)

    def count(self, name):
        return sum(n == name for n in self.names)


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    import tiny_assets
    from flair.custom_data_loader import BatchedData
    from flair.data import Dictionary, Sentence
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    d = tmp_path_factory.mktemp("pool_e2e")
    tiny_assets.build_model_dir(str(d / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(d / "enc_b"), seed=3, tokenizer="wordpiece")
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)
    POOLED = (dict(layers="-1,-2", pooling_operation="mean"), dict(layers="all", pooling_operation="first_last", use_scalar_mix=True))
    PLAIN = (dict(layers="-1", pooling_operation="first"), dict(layers="-1", pooling_operation="first"))

    def make(specs=POOLED, **kw):
        torch.manual_seed(99)
        embs = [TransformerWordEmbeddings(model=str(d / "enc_a"), **specs[0]), TransformerWordEmbeddings(model=str(d / "enc_b"), **specs[1])]
        args = dict(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=True,
                    dropout=0.0, word_dropout=0.0, locked_dropout=0.0, sentence_loss=True)
        args.update(kw)
        return FastSequenceTagger(**args)

    sents = []
    for toks, tags in [("alice zalandoresearchuniversitycambridge \x01 berlin wikipedia", "S-PER O O B-LOC E-LOC"), ("bob", "S-PER"),
                       ("\x01 museum population", "O O S-PER")]:
        s = Sentence(toks)
        assert len(s) == len(tags.split())
        for t, v in zip(s, tags.split()):
            t.add_tag("ner", v)
        s.ner_tags = [td.get_idx_for_item(v) for v in tags.split()]
        sents.append(s)
    return make, BatchedData(sents), sents, PLAIN


def _states_are_the_hidden_states(enc, states, hb):
    """The buffers the pooled path reads after a forward-only pass, enc.acts(R, S).x[i], against an INDEPENDENT encoder: the torch
    restatement of oracle/encoder.py on the same weights (GEMM weights rounded through bf16, as selftest.oracle_params does) and the
    same ids / mask, at the real sub-token positions.  x[i] must be hidden state i -- within selftest.STEP_TOL["emissions_rel"], the
    project's margin for what this tiny encoder's forward differs from float32 by -- and must NOT be within it of any other state."""
    from oracle import encoder as oenc
    sd = {k: v.detach().float().cpu() for k, v in enc.hf_state_dict().items()}
    for k in list(sd):
        if k.endswith(("dense.weight", "query.weight", "key.weight", "value.weight")):
            sd[k] = sd[k].to(BF16).float()
    R, S, H = hb["R"], hb["S"], enc.cfg.hidden_size
    with torch.no_grad():
        _, hs = oenc.encoder_forward(sd, enc.cfg, torch.from_numpy(hb["input_ids"]), torch.from_numpy(hb["attention_mask"]), return_all=True)
    assert len(states) == len(hs) == enc.cfg.num_hidden_layers + 1
    real = torch.from_numpy(hb["attention_mask"].astype(bool))
    tol = selftest.STEP_TOL["emissions_rel"]
    for i, st in enumerate(states):
        mine = st[:R * S].float().cpu().view(R, S, H)[real]
        rels = [float((mine - h[real]).norm() / h[real].norm()) for h in hs]
        print("[pool] x[%d] against the oracle's hidden states 0..%d: %s" % (i, len(hs) - 1, ", ".join("%.3e" % r for r in rels)))
        assert rels[i] < tol, (i, rels)
        assert all(r > tol for j, r in enumerate(rels) if j != i), (i, rels)


def test_a_blocks_equal_the_reference_on_the_encoders_own_hidden_states(assets):
    from kbner import batch as kb
    make, batch, sents, _ = assets
    tagger = make()
    tagger.eval()
    X, lengths, B, n = tagger._stack_input(batch)
    torch.cuda.synchronize()
    head = tagger.stack_head
    assert (B, n) == (3, 5) and head.blocks == [256, 256] and X.dtype == BF16
    assert not bool(X[B * n:].any()), "rows behind the batch must be zero"
    Xh = X.float().cpu().numpy().astype(np.float64)
    seen_multi = seen_dropped = 0
    for slot, emb in enumerate(tagger._stack_embs):
        ids, am, lens, span_ptr, span_loc = emb.prepare_pool_batch(batch)
        hb = kb.assemble(ids, am, np.full((B, n), -1, np.int64), np.zeros((B, n), np.int64), lens, None)
        enc = tagger._encoder_for(emb)
        states = enc.acts(hb["R"], hb["S"]).x
        _states_are_the_hidden_states(enc, states, hb)
        xs = [states[li].float().cpu().numpy().astype(np.float64) for li in emb.layer_indexes]
        flat = span_loc[:, 0] * hb["S"] + span_loc[:, 1]
        col, W = head.cols[slot], emb.embedding_length
        pr.check(Xh[:B * n, col:col + W], xs, span_ptr, flat, emb.pooling_operation, emb.use_scalar_mix)
        m = pr.span_lengths(span_ptr).reshape(B, n)
        for b, s in enumerate(sents):
            assert not m[b, len(s):].any() and not Xh[b * n + len(s):(b + 1) * n, col:col + W].any()       # padding rows
            seen_dropped += int((m[b, :len(s)] == 0).sum())
        seen_multi += int((m > 1).sum())
        assert bool(Xh[:B * n, col:col + W].any())
    assert seen_multi >= 2 and seen_dropped >= 2                 # multi-piece words in both blocks, the dropped tokens in B's


def test_b_first_of_the_last_layer_issues_the_old_launches_only(assets, monkeypatch):
    import flair
    from kbner import batch as kb
    from kbner import ops
    make, batch, _, PLAIN = assets
    tagger = make(PLAIN)
    tagger.eval()
    calls = Calls(monkeypatch)
    tagger._stack_input(batch)          # (a first pass: whatever an encoder does once is behind us)
    # the producers' composition, written out: what _stack_compute did before the pooling kernel existed
    head = tagger.stack_head
    B, n = 3, 5
    want = head.new_input(B, n)
    torch.cuda.synchronize()
    calls.names.clear()
    for slot, emb in enumerate(tagger._stack_embs):
        ids, am, first, lens, first_row = emb.prepare_stack_batch(batch)
        db = kb.to_device(kb.assemble(ids, am, first, np.zeros(first.shape, np.int64), lens, None, first_row=first_row), flair.device)
        enc = tagger._encoder_for(emb)
        hidden = enc.encoder_forward(db["ids"], db["pos_ids"], db["maskbias"], db["R"], db["S"], need_grad=False)
        ops.gather_rows_into(hidden, db["row_idx"], want, head.cols[slot], enc.cfg.hidden_size)
    old = list(calls.names)
    calls.names.clear()
    X = tagger._stack_input(batch)[0]
    assert calls.names == old and calls.count("kbner_gather_rows_ld") == 2 and calls.count("kbner_pool_rows_layers") == 0
    assert torch.equal(_bits(X), _bits(want))
    # and the pooled tagger: one launch of the new kernel per encoder, none of the old gather
    pooled = make()
    pooled.eval()
    calls.names.clear()
    before = calls.encoders
    pooled._stack_input(batch)
    assert calls.count("kbner_pool_rows_layers") == 2 and calls.count("kbner_gather_rows_ld") == 0 and calls.encoders == before + 2


def test_c_a_second_visit_reads_the_store_bit_for_bit(assets, monkeypatch):
    make, batch, _, _ = assets
    tagger = make()
    tagger.eval()
    calls = Calls(monkeypatch)
    store = tagger.open_feature_store("gpu")
    X0 = tagger._stack_input(batch)[0].clone()
    assert calls.encoders == 2 and calls.count("kbner_pool_rows_layers") == 2 and len(store) == 3
    calls.names.clear()
    X1 = tagger._stack_input(batch)[0]
    assert calls.encoders == 2 and calls.count("kbner_pool_rows_layers") == 0 and calls.count("kbner_gather_rows_blocks_drop") == 1
    assert torch.equal(_bits(X1), _bits(X0))
    tagger.close_feature_store()


def test_d_forward_backward_on_pooled_features_against_float64_autograd(assets):
    make, batch, sents, _ = assets
    tagger = make()
    tagger.train()
    loss = float(tagger.forward_backward(batch))
    torch.cuda.synchronize()
    assert np.isfinite(loss)
    head = tagger.stack_head
    X, lengths, B, n = tagger._stack_input(batch)
    x = np.zeros((B * n, head.D))
    ref = 0
    for w, c in zip(head.blocks, head.cols):
        x[:, ref:ref + w] = X[:B * n, c:c + w].float().cpu().numpy()
        ref += w
    tags = np.zeros((B, n), np.int64)
    for b, s in enumerate(sents):
        tags[b, :len(s)] = [tagger.tag_dictionary.get_idx_for_item(t.get_tag("ner").value) for t in s]
    st = tagger._stack_state
    stn = {"rnn": {k: v.numpy() for k, v in st["rnn"].items()}, "linear.weight": st["linear.weight"].numpy(),
           "linear.bias": st["linear.bias"].numpy(), "transitions": st["transitions"].numpy()}
    ref_loss, ref_grads, _ = R.head_reference64(x.reshape(B, n, head.D), lengths, tags, stn, tagger.start_idx, tagger.stop_idx)
    g = head.state_of(head.g)
    got = {"rnn." + k: v for k, v in g["rnn"].items()}
    got.update({k: g[k] for k in ("linear.weight", "linear.bias", "transitions")})
    got = {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float64) for k, v in got.items()}
    keys = sorted(ref_grads)
    c = cos(np.concatenate([got[k].ravel() for k in keys]), np.concatenate([np.asarray(ref_grads[k], np.float64).ravel() for k in keys]))
    print("[pool] loss %.6f (float64 %.6f), head gradient cosine %.9f" % (loss, ref_loss, c))
    assert c > selftest.TRAIN_TOL["delta_cos_min"]


def test_e_model_finetuner_trains_from_an_ace_style_yaml_and_test_reloads(tmp_path):
    import subprocess
    import sys
    import yaml
    import tiny_assets
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    tiny_assets.build_model_dir(str(tmp_path / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(tmp_path / "enc_b"), seed=5)
    tiny_assets.write_conll_corpus(str(tmp_path / "data"), n_train=6, n_dev=3, n_test=3, seed=3)
    cfg = {"ModelFinetuner": {"distill_mode": False, "optimizer": "AdamW", "sentence_level_batch": True},
           "embeddings": {"TransformerWordEmbeddings-0": {"layers": "-1,-2", "model": str(tmp_path / "enc_a"), "pooling_operation": "mean"},
                          "TransformerWordEmbeddings-1": {"layers": "-1", "model": str(tmp_path / "enc_b"), "pooling_operation": "mean"}},
           "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40, "use_rnn": True,
                                            "sentence_loss": True, "use_crf": True}},
           "model_name": "pool_tiny", "target_dir": str(tmp_path / "out"), "targets": "ner", "trainer": "ModelFinetuner",
           "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(tmp_path / "tags.pkl"),
                   "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                         "data_folder": str(tmp_path / "data"), "tag_to_bioes": "ner"}},
           "train": {"learning_rate": 2e-3, "lr_rate": 2.0, "max_epochs": 1, "mini_batch_size": 2, "gradient_accumulation_steps": 1,
                     "monitor_test": False, "train_with_dev": False, "shuffle": True, "embeddings_storage_mode": "gpu"}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    cp = ConfigParser(Params.from_file(str(tmp_path / "cfg.yaml")))
    student = cp.create_student()
    assert student.use_rnn and student._stack_blocks == [256, 128]
    assert [e.pooling_operation for e in student._stack_embs] == ["mean", "mean"] and student._stack_embs[0].layer_indexes == [-1, -2]
    trainer = flair.trainers.ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    losses = []
    trainer.stack_step_hook = lambda batches, ls: losses.extend(float(x) for x in ls)
    base = cp.get_target_path
    res = trainer.train(base, **cp.config["train"])
    assert len(res["dev_score_history"]) == 1 and len(losses) == 3 and np.isfinite(losses).all()
    assert (base / "stack-model.pt").exists()
    best = torch.load(str(base / "stack-model.pt"), map_location="cpu", weights_only=False)
    assert tuple(best["rnn"]["weight_ih_l0"].shape) == (160, 384)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "--config", str(tmp_path / "cfg.yaml"), "--test"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
