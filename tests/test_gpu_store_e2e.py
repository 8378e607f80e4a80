"""GPU: the feature store of the stacked tagger end to end (kbner.stack.FeatureStore, FastSequenceTagger.open_feature_store,
BiLSTMHead.loss_backward(source=...), ModelFinetuner's embeddings_storage_mode), on the tiny two-encoder stack of
tests/test_gpu_stack_train.py (tiny_assets, 6 / 3 / 3 sentences, 2 epochs).

  (a) store open in "gpu" and in "cpu" mode: the second _stack_input of a batch returns X bit-equal to the first and launches no
      feature producer (calls of kbner.engine.Tagger.encoder_forward and kbner.stack.CharLMGroup.run are counted); over a whole trainer
      run every batch is computed once -- the count stays flat across epoch 2, its dev evaluation and the trainer's hook -- and with
      "none" it grows with every visit;
  (b) forward_backward reading the store gives last_emissions and a loss BIT-equal to the X path for the same drawn dropout sites
      (WordDropout, element and locked dropout before the BiLSTM, both after it) and gradients within selftest.TRAIN_TOL (the
      weight-gradient GEMMs accumulate with fp32 atomics: gradients are not run-to-run exact without a store either);
  (c) a trainer run with "gpu" (and "cpu") against one with "none" from the same initial state and seed: the losses of the first
      optimizer step are identical, all later losses and the total update of stack-model.pt agree within selftest.TRAIN_TOL
      (loss_rel_max, delta_cos_min), dev_score_history has the same length;
  (d) a selection that switches a stored block off zeroes exactly that block's columns without computing anything; one that needs a
      block the store lacks refills it;
  (e) with no store open _stack_input gives the bytes of the producers' composition (encoder_forward + gather_rows_ld into a zeroed
      X) and nothing launches the new kernel.

Figures of the MI355X run that accompanied this module (8 tests, 6.6 s): trainer runs with "gpu" and with "cpu" against "none": worst
relative loss difference 0.0, cosine of the total update 1.000000000 (the bounds are 1.5e-3 and 0.9985); encoder launches 10 against
18 over the two epochs, dev evaluations and the final test."""
import numpy as np
import pytest
import torch

import selftest

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


class Counter:
    """counts the feature producers' launches and the store kernel's"""

    def __init__(self, monkeypatch):
        from kbner import engine, ops, stack
        self.producers = self.store_reads = 0
        enc, lm, rd = engine.Tagger.encoder_forward, stack.CharLMGroup.run, ops.gather_rows_blocks_drop

        def encoder_forward(this, *a, **k):
            self.producers += 1
            return enc(this, *a, **k)

        def run(this, *a, **k):
            self.producers += 1
            return lm(this, *a, **k)

        def read(*a, **k):
            self.store_reads += 1
            return rd(*a, **k)
        monkeypatch.setattr(engine.Tagger, "encoder_forward", encoder_forward)
        monkeypatch.setattr(stack.CharLMGroup, "run", run)
        monkeypatch.setattr(ops, "gather_rows_blocks_drop", read)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


# ====================================================================== the tagger
@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    import tiny_assets
    from flair.custom_data_loader import BatchedData
    from flair.data import Dictionary, Sentence
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    d = tmp_path_factory.mktemp("store")
    tiny_assets.build_model_dir(str(d / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(d / "enc_b"), seed=5)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)

    def make(**kw):
        torch.manual_seed(99)
        embs = [TransformerWordEmbeddings(model=str(d / "enc_a"), layers="-1", pooling_operation="first"),
                TransformerWordEmbeddings(model=str(d / "enc_b"), layers="-1", pooling_operation="first")]
        args = dict(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=True,
                    dropout=0.0, word_dropout=0.0, locked_dropout=0.0, sentence_loss=True)
        args.update(kw)
        return FastSequenceTagger(**args)

    def batch(texts):
        sents = []
        for toks, tags in texts:
            s = Sentence(toks)
            for t, v in zip(s, tags.split()):
                t.add_tag("ner", v)
            s.ner_tags = [td.get_idx_for_item(v) for v in tags.split()]
            sents.append(s)
        return BatchedData(sents)
    one = batch([("a b c d e", "O S-PER O B-LOC E-LOC"), ("f", "S-PER"), ("g h i", "O O S-PER")])
    two = batch([("j k", "O O"), ("l m n o", "B-LOC E-LOC O S-PER")])
    return make, one, two


@pytest.mark.parametrize("mode", ["gpu", "cpu"], ids=["device_store", "host_store"])
def test_a_second_visit_reads_the_store_bit_for_bit_and_launches_no_producer(assets, mode, monkeypatch):
    make, one, two = assets
    tagger = make()
    tagger.eval()
    count = Counter(monkeypatch)
    store = tagger.open_feature_store(mode)
    assert store is not None and store.mode == mode and len(store) == 0
    first = {}
    for name, b in (("one", one), ("two", two)):
        X, lengths, B, n = tagger._stack_input(b)
        first[name] = (X.clone(), lengths, B, n)
    assert count.producers == 4 and count.store_reads == 0 and len(store) == 5 and store.rows == 9 + 6
    for name, b in (("one", one), ("two", two), ("one", one)):
        X, lengths, B, n = tagger._stack_input(b)
        X0, l0, B0, n0 = first[name]
        assert X.shape == X0.shape and X.dtype == BF16 and (B, n) == (B0, n0) and np.array_equal(lengths, l0)
        assert torch.equal(_bits(X), _bits(X0)), name
    assert count.producers == 4 and count.store_reads == 3 and (store.hits, store.misses) == (3, 2)
    # sentences of two batches in a third: served from the store, each sentence's own rows, zero rows at the padding
    from flair.custom_data_loader import BatchedData
    mix = BatchedData([two[1], one[2]])
    X, lengths, B, n = tagger._stack_input(mix)
    assert count.producers == 4 and (B, n) == (2, 4)
    assert torch.equal(_bits(X[0:4]), _bits(first["two"][0][4:8])) and torch.equal(_bits(X[4:7]), _bits(first["one"][0][10:13]))
    assert not bool(X[7:].any())
    # the emissions of an evaluation forward are those of the computed features
    em_store = tagger.forward(one).clone()
    tagger.close_feature_store()
    assert tagger._feature_store is None and store.chunks == [] and len(store) == 0
    em_plain = tagger.forward(one)
    assert count.producers == 6 and torch.equal(_bits(em_store), _bits(em_plain))
    # "none": no store
    assert tagger.open_feature_store("none") is None
    tagger._stack_input(one)
    tagger._stack_input(one)
    assert count.producers == 10 and count.store_reads == 5


def _word_seed(n, p):
    """a dropout seed whose first draw drops some positions of n and keeps some (the head's stream: _draw_dropout)"""
    for seed in range(100):
        w = np.random.default_rng(seed).random(n) < p
        if 0 < int(w.sum()) < n:
            return seed
    raise AssertionError


def test_b_forward_backward_from_the_store_equals_the_x_path(assets, monkeypatch):
    make, one, _ = assets
    tagger = make(dropout=0.1, word_dropout=0.3, locked_dropout=0.5)
    tagger.train()
    count = Counter(monkeypatch)
    head = tagger.enable_stack_training()
    seed = _word_seed(5, 0.3)
    head.seed_dropout(seed)
    loss_x = tagger.forward_backward(one)
    em_x, g_x, drop_x = head.last_emissions.clone(), head.g.clone(), head.last_drop
    assert count.store_reads == 0 and drop_x[0].any() and drop_x[1][0][1] and drop_x[1][1][1]
    for mode in ("gpu", "cpu"):
        tagger.zero_grad()
        tagger.open_feature_store(mode)
        tagger._stack_input(one)                                    # the first visit fills the store
        before = (count.producers, count.store_reads)
        head.seed_dropout(seed)
        loss_s = tagger.forward_backward(one)
        torch.cuda.synchronize()
        assert (count.producers, count.store_reads) == (before[0], before[1] + 1)      # ONE launch replaces the first stage
        assert repr(head.last_drop) == repr(drop_x)
        assert torch.equal(_bits(head.last_emissions), _bits(em_x)), mode
        assert float(loss_s) == float(loss_x), (mode, float(loss_s), float(loss_x))
        c = cos(head.g.cpu().numpy(), g_x.cpu().numpy())
        rel = float((head.g - g_x).norm() / g_x.norm())
        print("[store] %s: gradient cosine %.9f, relative L2 %.3e against the X path" % (mode, c, rel))
        assert c > selftest.TRAIN_TOL["delta_cos_min"]
        tagger.close_feature_store()


def test_d_selection_subset_is_served_and_a_missing_block_refills(assets, monkeypatch):
    make, one, _ = assets
    tagger = make()
    tagger.eval()
    count = Counter(monkeypatch)
    head = tagger.stack_head
    c0, c1 = head.cols
    full = tagger._stack_input(one)[0].clone()
    assert bool(full[:, c0:c1].any()) and bool(full[:, c1:].any()) and count.producers == 2
    store = tagger.open_feature_store("gpu")
    tagger._stack_input(one)
    assert store.have == [True, True] and count.producers == 4
    # one stored block switched off: exactly its columns are zero, nothing is computed
    tagger.embedding_selector, tagger.selection = True, torch.tensor([1.0, 0.0])
    X = tagger._stack_input(one)[0]
    assert count.producers == 4 and len(store) == 3
    assert torch.equal(_bits(X[:, :c1]), _bits(full[:, :c1])) and not bool(X[:, c1:].any())
    tagger.selection = torch.tensor([0.0, 1.0])
    X = tagger._stack_input(one)[0]
    assert count.producers == 4 and torch.equal(_bits(X[:, c1:]), _bits(full[:, c1:])) and not bool(X[:, :c1].any())
    # a store filled under the narrower selection lacks block 0: a selection that needs it empties and refills the store
    tagger.close_feature_store()
    store = tagger.open_feature_store("gpu")
    X = tagger._stack_input(one)[0]
    assert count.producers == 5 and store.have == [False, True] and not bool(X[:, :c1].any())     # the deselected encoder did not run
    tagger._stack_input(one)
    assert count.producers == 5
    tagger.selection = torch.tensor([1.0, 1.0])
    X = tagger._stack_input(one)[0]
    assert count.producers == 7 and store.have == [True, True] and len(store) == 3 and torch.equal(_bits(X), _bits(full))
    X = tagger._stack_input(one)[0]
    assert count.producers == 7 and torch.equal(_bits(X), _bits(full))
    tagger.close_feature_store()


def test_e_without_a_store_nothing_changed(assets, monkeypatch):
    from kbner import batch as kb
    from kbner import ops
    import flair
    make, one, _ = assets
    tagger = make(dropout=0.1, word_dropout=0.3, locked_dropout=0.5)
    tagger.eval()
    count = Counter(monkeypatch)
    assert tagger.__dict__.get("_feature_store") is None
    X, lengths, B, n = tagger._stack_input(one)
    # the producers' composition, written out
    head = tagger.stack_head
    want = head.new_input(B, n)
    for slot, emb in enumerate(tagger._stack_embs):
        ids, am, first, lens, first_row = emb.prepare_stack_batch(one)
        db = kb.to_device(kb.assemble(ids, am, first, np.zeros(first.shape, np.int64), lens, None, first_row=first_row), flair.device)
        enc = tagger._encoder_for(emb)
        hidden = enc.encoder_forward(db["ids"], db["pos_ids"], db["maskbias"], db["R"], db["S"], need_grad=False)
        ops.gather_rows_into(hidden, db["row_idx"], want, head.cols[slot], enc.cfg.hidden_size)
    assert torch.equal(_bits(X), _bits(want)) and not bool(X[B * n:].any())
    # forward_backward outside the trainer: the X path, the loss of loss_backward on that X with the same sites
    tagger.train()
    head = tagger.enable_stack_training()
    head.seed_dropout(3)
    loss = float(tagger.forward_backward(one))
    sites, em = head.last_drop, head.last_emissions.clone()
    tagger.zero_grad()
    direct = float(head.loss_backward(X, lengths, B, n, tagger._last[1], tagger.start_idx, tagger.stop_idx, drop=sites))
    assert direct == loss and torch.equal(_bits(head.last_emissions), _bits(em))
    assert count.store_reads == 0


# ====================================================================== the trainer
N_TRAIN, N_DEV, N_TEST, MBS, EPOCHS = 6, 3, 3, 2, 2


def _np_state(st):
    return np.concatenate([np.asarray(st["rnn"][k], np.float64).ravel() for k in sorted(st["rnn"])] +
                          [np.asarray(st[k], np.float64).ravel() for k in ("linear.weight", "linear.bias", "transitions")])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """ModelFinetuner.train on the tiny corpus with embeddings_storage_mode none / gpu / cpu, each from the same seed -> per mode:
    the producer launches counted at every hook call and at the end, the losses of every optimizer step, stack-model.pt, the result"""
    import yaml
    import tiny_assets
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    from kbner import engine
    root = tmp_path_factory.mktemp("storetrain")
    tiny_assets.build_model_dir(str(root / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(root / "enc_b"), seed=5)
    tiny_assets.write_conll_corpus(str(root / "data"), n_train=N_TRAIN, n_dev=N_DEV, n_test=N_TEST, seed=3)
    out = {}
    mp = pytest.MonkeyPatch()
    try:
        calls = [0]
        enc = engine.Tagger.encoder_forward

        def encoder_forward(this, *a, **k):
            calls[0] += 1
            return enc(this, *a, **k)
        mp.setattr(engine.Tagger, "encoder_forward", encoder_forward)
        for mode in ("none", "gpu", "cpu"):
            cfg = {"ModelFinetuner": {"distill_mode": False, "optimizer": "AdamW", "sentence_level_batch": True},
                   "embeddings": {"TransformerWordEmbeddings-0": {"layers": "-1", "model": str(root / "enc_a"), "pooling_operation": "first"},
                                  "TransformerWordEmbeddings-1": {"layers": "-1", "model": str(root / "enc_b"), "pooling_operation": "first"}},
                   "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40,
                                                    "use_rnn": True, "sentence_loss": True, "use_crf": True}},
                   "model_name": "store_" + mode, "target_dir": str(root / "out"), "targets": "ner", "trainer": "ModelFinetuner",
                   "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(root / "tags.pkl"),
                           "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                                 "data_folder": str(root / "data"), "tag_to_bioes": "ner"}},
                   "train": {"learning_rate": 2e-3, "lr_rate": 2.0, "max_epochs": EPOCHS, "mini_batch_size": MBS,
                             "gradient_accumulation_steps": 1, "monitor_test": False, "train_with_dev": False, "shuffle": True,
                             "embeddings_storage_mode": mode}}
            with open(root / ("cfg_%s.yaml" % mode), "w") as f:
                yaml.safe_dump(cfg, f)
            torch.manual_seed(2024)
            cp = ConfigParser(Params.from_file(str(root / ("cfg_%s.yaml" % mode))))
            student = cp.create_student()
            trainer = flair.trainers.ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
            start = _np_state(student._stack_state)
            calls[0] = 0
            losses, at_step = [], []

            def hook(batches, ls):
                losses.append([float(x) for x in ls])
                at_step.append(calls[0])
            trainer.stack_step_hook = hook
            res = trainer.train(cp.get_target_path, **cp.config["train"])
            best = torch.load(str(cp.get_target_path / "stack-model.pt"), map_location="cpu", weights_only=False)
            out[mode] = dict(losses=losses, at_step=at_step, total=calls[0], res=res, start=start, best=_np_state(best),
                             store_open_after=student.__dict__.get("_feature_store") is not None,
                             log=open(str(cp.get_target_path / "training.log")).read())
    finally:
        mp.undo()
    return out


def test_a_trainer_computes_every_batch_once(runs):
    enc = 2                                              # frozen encoders, one encoder_forward each per computed batch
    train_b, dev_b, test_b = N_TRAIN // MBS, 1, 1        # eval batches hold up to 32 sentences
    steps = train_b                                      # gradient_accumulation_steps 1: one optimizer step per batch
    none = runs["none"]
    assert len(none["at_step"]) == EPOCHS * steps
    # "none": every visit computes -- epoch 2, its dev evaluation and the final test included
    assert none["at_step"] == [enc * (k + 1 + dev_b * (k // steps)) for k in range(EPOCHS * steps)]
    assert none["total"] == enc * (EPOCHS * (train_b + dev_b) + test_b)
    for mode in ("gpu", "cpu"):
        r = runs[mode]
        first = [enc * (k + 1) for k in range(steps)]
        assert r["at_step"][:steps] == first
        flat = enc * (train_b + dev_b)
        assert r["at_step"][steps:] == [flat] * steps, (mode, r["at_step"])      # flat across epoch 2
        assert r["total"] == flat + enc * test_b                                 # epoch 2's dev evaluation computed nothing; the test
        assert not r["store_open_after"]                                          # set is visited once; the store is closed at the end
        assert r["log"].count("feature store (%s):" % mode) == EPOCHS
    assert "feature store" not in none["log"]


@pytest.mark.parametrize("mode", ["gpu", "cpu"], ids=["device_store", "host_store"])
def test_c_trainer_with_a_store_follows_the_run_without(runs, mode):
    a, b = runs["none"], runs[mode]
    assert a["losses"][0] == b["losses"][0], "the first optimizer step sees the same features and the same weights"
    assert len(a["losses"]) == len(b["losses"]) == EPOCHS * (N_TRAIN // MBS)
    worst = max(abs(x - y) / abs(x) for la, lb in zip(a["losses"], b["losses"]) for x, y in zip(la, lb))
    assert np.array_equal(a["start"], b["start"])
    c = cos(a["best"] - a["start"], b["best"] - b["start"])
    print("[store] %s against none: worst relative loss difference %.3e, cosine of the total update %.9f" % (mode, worst, c))
    assert worst < selftest.TRAIN_TOL["loss_rel_max"] and c > selftest.TRAIN_TOL["delta_cos_min"]
    assert len(a["res"]["dev_score_history"]) == len(b["res"]["dev_score_history"]) == EPOCHS
