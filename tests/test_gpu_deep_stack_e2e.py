"""GPU: FastSequenceTagger(use_rnn=True, rnn_layers=2, train_initial_hidden_state=True) end to end on the tiny assets.

  (a) ModelFinetuner.train from a YAML, two epochs, embeddings_storage_mode gpu and none: every new parameter (rnn.*_l1, lstm_init_h,
      lstm_init_c) changes, the loss falls, the two storage modes agree;
  (b) stack-model.pt carries rnn_layers, train_initial_hidden_state and the new tensors; a fresh tagger that loads it reproduces the
      emissions bit for bit; a one-layer tagger refuses it; final_test runs;
  (c) one ReinforcementTrainer episode runs;
  (d) with a FastCharacterEmbeddings in the stack the character gradients -- whose window of dXt comes from layer 0 -- and every
      other gradient still match float64 autograd of the whole step (bounds: selftest.STEP_TOL, as tests/test_gpu_char_e2e.py);
  (e) without use_rnn both switches build the fine-tuning tagger unchanged and travel through its state file."""
import numpy as np
import pytest
import torch

import charref as C
import deepref as DR
import selftest

pytestmark = pytest.mark.gpu
N_TRAIN, N_DEV, N_TEST, MBS, EPOCHS = 6, 3, 3, 2, 2
NEW = ("lstm_init_h", "lstm_init_c")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def _np_state(st):
    out = {"rnn." + k: np.asarray(v, np.float64) for k, v in st["rnn"].items()}
    out.update({k: np.asarray(st[k], np.float64) for k in ("linear.weight", "linear.bias", "transitions") + NEW if k in st})
    return out


def _config(root, name, trainer, storage, optimizer, **train):
    import yaml
    tblock = {"distill_mode": False, "optimizer": optimizer, "sentence_level_batch": True}
    if trainer == "ReinforcementTrainer":
        tblock.update(controller_optimizer="SGD", controller_learning_rate=0.1)
    cfg = {trainer: tblock, "Controller": {"model_structure": None},
           "embeddings": {"TransformerWordEmbeddings-0": {"layers": "-1", "model": str(root / "enc_a"), "pooling_operation": "first"},
                          "TransformerWordEmbeddings-1": {"layers": "-1", "model": str(root / "enc_b"), "pooling_operation": "first"}},
           "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40, "use_rnn": True,
                                            "sentence_loss": True, "use_crf": True, "rnn_layers": 2, "train_initial_hidden_state": True}},
           "model_name": name, "target_dir": str(root / "out"), "targets": "ner", "trainer": trainer,
           "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(root / "tags.pkl"),
                   "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                         "data_folder": str(root / "data"), "tag_to_bioes": "ner"}},
           "train": dict({"learning_rate": 0.05 if optimizer == "SGD" else 2e-3, "lr_rate": 2.0, "max_epochs": EPOCHS, "mini_batch_size": MBS,
                          "gradient_accumulation_steps": 1, "monitor_test": False, "train_with_dev": False, "shuffle": True,
                          "embeddings_storage_mode": storage}, **train)}
    if trainer == "ReinforcementTrainer":
        cfg["train"].update(controller_momentum=0.9, discount=0.5)
    path = root / ("%s.yaml" % name)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


def _run(root, name, tname, storage, optimizer, **train):
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    path = _config(root, name, tname, storage, optimizer, **train)
    torch.manual_seed(2024)
    cp = ConfigParser(Params.from_file(str(path)))
    student = cp.create_student()
    assert student.use_rnn and student.nlayers == 2 and student.train_initial_hidden_state and student.stack_head.L == 2
    trainer = getattr(flair.trainers, tname)(student, None, cp.corpus, config=cp.config, **cp.config[tname])
    start = _np_state(student._stack_state)
    steps = []
    trainer.stack_step_hook = lambda batches, ls: steps.append(dict(losses=[float(x) for x in ls], state=_np_state(student._stack_state)))
    res = trainer.train(cp.get_target_path, **cp.config["train"])
    return dict(steps=steps, res=res, start=start, base=cp.get_target_path, student=student, cp=cp, trainer=trainer, path=path)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import tiny_assets
    root = tmp_path_factory.mktemp("deep_train")
    tiny_assets.build_model_dir(str(root / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(root / "enc_b"), seed=5)
    tiny_assets.write_conll_corpus(str(root / "data"), n_train=N_TRAIN, n_dev=N_DEV, n_test=N_TEST, seed=3)
    out = {"root": root}
    for mode in ("none", "gpu"):
        out[mode] = _run(root, "deep_" + mode, "ModelFinetuner", mode, "AdamW")
    return out


def test_a_finetuner_trains_every_new_parameter_in_both_storage_modes(runs):
    none = runs["none"]
    steps = none["steps"]
    per = N_TRAIN // MBS
    assert len(steps) == EPOCHS * per
    first, last = np.mean([np.mean(s["losses"]) for s in steps[:per]]), np.mean([np.mean(s["losses"]) for s in steps[-per:]])
    print("[deepe2e] mean loss of the first epoch %.4f, of the last %.4f" % (first, last))
    assert last < first
    new = [k for k in none["start"] if "_l1" in k] + list(NEW)
    assert len(new) == 8 + 2
    for k in new:
        moved = np.abs(steps[-1]["state"][k] - none["start"][k])
        assert moved.max() > 1e-4 and (moved > 0).mean() > 0.5, k
    gpu = runs["gpu"]
    assert all(np.array_equal(gpu["start"][k], none["start"][k]) for k in none["start"])
    worst = max(abs(x - y) / abs(x) for a, b in zip(steps, gpu["steps"]) for x, y in zip(a["losses"], b["losses"]))
    flat = lambda st: np.concatenate([st[k].ravel() for k in sorted(st)])                      # noqa: E731
    c = cos(flat(steps[-1]["state"]) - flat(none["start"]), flat(gpu["steps"][-1]["state"]) - flat(none["start"]))
    print("[deepe2e] gpu against none: worst relative loss difference %.3e, update cosine %.9f" % (worst, c))
    assert worst < selftest.TRAIN_TOL["loss_rel_max"] and c > selftest.TRAIN_TOL["delta_cos_min"]


def test_b_stack_model_file_reloads_bit_for_bit_and_final_test_runs(runs):
    from flair.custom_data_loader import BatchedData
    r = runs["none"]
    student = r["student"]
    student.eval()
    batch = BatchedData([r["cp"].corpus.train[i] for i in range(3)])
    state = torch.load(str(r["base"] / "stack-model.pt"), map_location="cpu", weights_only=False)
    assert state["rnn_layers"] == 2 and state["train_initial_hidden_state"] is True
    assert {"weight_ih_l1", "weight_hh_l1_reverse", "bias_hh_l1"} <= set(state["rnn"]) and tuple(state["lstm_init_h"].shape) == (4, 40)
    student.load_stack_state(state)                      # (the trainer left the LAST weights in place; the file holds the best)
    want = student.forward(batch).clone()
    torch.manual_seed(7)                                 # another initialisation: everything must come from the file
    fresh = r["cp"].create_student()
    fresh.eval()
    assert not torch.equal(_bits(fresh.forward(batch)), _bits(want))
    fresh.load_stack_state(state)
    assert fresh.stack_head.arena is None and torch.equal(_bits(fresh.forward(batch)), _bits(want))
    # the initial state matters to the emissions: zeroing it changes them
    fresh.load_stack_state(dict(state, lstm_init_h=torch.zeros(4, 40), lstm_init_c=torch.zeros(4, 40)))
    assert not torch.equal(_bits(fresh.forward(batch)), _bits(want))
    res = r["trainer"].final_test(r["base"], MBS)
    assert res is not None and np.isfinite(float(res))


def test_c_one_reinforcement_episode_runs(runs):
    r = _run(runs["root"], "deep_ace", "ReinforcementTrainer", "gpu", "SGD", max_episodes=1)
    assert len(r["steps"]) >= 1 and all(np.isfinite(s["losses"]).all() for s in r["steps"])
    assert np.abs(r["steps"][-1]["state"]["lstm_init_c"] - r["start"]["lstm_init_c"]).max() > 0
    assert (r["base"] / "stack-model.pt").exists()
    best = torch.load(str(r["base"] / "stack-model.pt"), map_location="cpu", weights_only=False)
    assert best["rnn_layers"] == 2 and "lstm_init_h" in best


def test_d_character_gradients_still_match_float64_autograd(tmp_path, monkeypatch):
    """the window of dXt the character BiLSTM receives is layer 0's dgx . Wih, whatever sits above layer 0"""
    import tiny_assets
    from flair.custom_data_loader import BatchedData
    from flair.data import Dictionary, Sentence
    from flair.embeddings import FastCharacterEmbeddings, StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    from kbner import stack as K
    tiny_assets.build_model_dir(str(tmp_path / "enc_a"), seed=0)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)
    texts = [("alice zalandoresearchuniversitycambridge x berlin wikipedia", "S-PER O O B-LOC E-LOC"), ("bob", "S-PER"),
             ("alice museum population", "O O S-PER")]
    torch.manual_seed(99)
    embs = [TransformerWordEmbeddings(model=str(tmp_path / "enc_a"), layers="-1", pooling_operation="first"),
            FastCharacterEmbeddings(vocab=[w for t, _ in texts for w in t.split() if w != "museum"])]
    tagger = FastSequenceTagger(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=td, tag_type="ner", use_crf=True,
                                use_rnn=True, dropout=0.0, word_dropout=0.0, locked_dropout=0.0, sentence_loss=True, rnn_layers=2,
                                train_initial_hidden_state=True)
    sents = []
    for toks, tags in texts:
        s = Sentence(toks)
        for t, v in zip(s, tags.split()):
            t.add_tag("ner", v)
        s.ner_tags = [td.get_idx_for_item(v) for v in tags.split()]
        sents.append(s)
    batch = BatchedData(sents)
    tagger.train()
    head = tagger.enable_stack_training()
    head.rnn_dropout = 0.0                       # (the float64 model below has no mask between the layers)
    seen = {}
    fwd = K.CharStep.forward

    def forward(this, Xt, sites, n, save=True):
        seen["before"] = Xt.clone()
        fwd(this, Xt, sites, n, save)
    monkeypatch.setattr(K.CharStep, "forward", forward)
    loss = float(tagger.forward_backward(batch))
    torch.cuda.synchronize()
    net, slot = tagger._char_net(), tagger._char_slot
    B, n = len(sents), max(len(s) for s in sents)
    W2 = 2 * net.Hc
    # the frozen columns as the input GEMM saw them, in the reference's column order
    x = np.zeros((B * n, head.D))
    ref = 0
    for w, c in zip(head.blocks, head.cols):
        x[:, ref:ref + w] = seen["before"][:B * n, c:c + w].float().cpu().numpy()
        ref += w
    c0 = sum(head.blocks[:slot])
    assert not x[:, c0:c0 + W2].any()
    chars, lens, rows = tagger._stack_embs[slot].char_batch(batch, n)
    st = tagger._stack_state
    cstate = {k: v.numpy() for k, v in st["char"].items()}
    # float64 autograd: Embedding -> BiLSTM over each word's characters -> hidden[0] placed into the block, then the two-layer head
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))                                  # noqa: E731
    emb = torch.nn.Embedding(net.V, net.E).double()
    crnn = torch.nn.LSTM(net.E, net.Hc, num_layers=1, bidirectional=True).double()
    with torch.no_grad():
        emb.weight.copy_(t64(cstate["char_embedding.weight"]))
        for k, p in crnn.named_parameters():
            p.copy_(t64(cstate["char_layer." + k]))
    ce = emb(torch.from_numpy(chars.astype(np.int64)).t())
    packed = torch.nn.utils.rnn.pack_padded_sequence(ce, torch.from_numpy(lens.astype(np.int64)), enforce_sorted=False)
    _, (hidden, _) = crnn(packed)
    block = torch.cat([hidden[0], hidden[1]], 1)
    place = torch.zeros((B * n, head.D), dtype=torch.float64)
    place = place.index_put((torch.from_numpy(rows.astype(np.int64))[:, None], torch.arange(c0, c0 + W2)[None, :]), block)
    xin = t64(x).view(B, n, head.D) + place.view(B, n, head.D)
    tags = np.zeros((B, n), np.int64)
    for b, s in enumerate(sents):
        tags[b, :len(s)] = s.ner_tags
    stn = {"rnn": {k: v.numpy() for k, v in st["rnn"].items()}}
    stn.update({k: st[k].numpy() for k in ("linear.weight", "linear.bias", "transitions") + NEW})
    ref_loss, ref_g, _ = DR.head_torch(xin, np.asarray([len(s) for s in sents]), tags, stn, 2, tagger.start_idx, tagger.stop_idx)
    ref_c = {"char_embedding.weight": emb.weight.grad.numpy()}
    ref_c.update({"char_layer." + k: p.grad.numpy() for k, p in crnn.named_parameters()})
    g = head.grad_state()
    got = {"rnn." + k: v.numpy() for k, v in g["rnn"].items()}
    got.update({k: g[k].numpy() for k in ("linear.weight", "linear.bias", "transitions") + NEW})
    got_c = {k: v.numpy() for k, v in net.state(net.g).items()}
    assert sorted(got) == sorted(ref_g) and sorted(got_c) == sorted(ref_c)
    print("[deepe2e] loss %.6f (float64 %.6f)" % (loss, ref_loss))
    rows_ = []
    for name, a, b in [(k, got[k], ref_g[k]) for k in sorted(ref_g)] + [(k, got_c[k], ref_c[k]) for k in sorted(ref_c)]:
        rows_.append((name, rel(a, b), cos(a, b)))
        print("[deepe2e]   %-36s rel %.3e  cos %.6f" % rows_[-1])
    assert abs(loss - ref_loss) / abs(ref_loss) < selftest.STEP_TOL["loss_rel"]
    bad = [r for r in rows_ if not (r[1] < selftest.STEP_TOL["grad_worst_rel"] and r[2] > selftest.STEP_TOL["grad_min_cos"])]
    assert not bad, bad
    assert hasattr(C, "stack_reference64")        # (the one-layer form of the model restated above)


def test_e_without_use_rnn_both_switches_select_nothing(tmp_path):
    import tiny_assets
    from flair.data import Dictionary
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    tiny_assets.build_model_dir(str(tmp_path / "enc_a"), seed=0)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)

    def make(**kw):
        torch.manual_seed(5)
        emb = TransformerWordEmbeddings(model=str(tmp_path / "enc_a"), layers="-1", pooling_operation="first", fine_tune=True)
        return FastSequenceTagger(hidden_size=40, embeddings=StackedEmbeddings([emb]), tag_dictionary=td, tag_type="ner", use_crf=True,
                                  use_rnn=False, **kw)
    a, b = make(), make(rnn_layers=2, train_initial_hidden_state=True)
    na, nb = dict(a.named_parameters()), dict(b.named_parameters())
    assert list(na) == list(nb) and "lstm_init_h" not in nb and not any(k.startswith("rnn.") for k in nb)
    assert all(torch.equal(na[k], nb[k]) for k in ("linear.weight", "linear.bias", "transitions"))
    assert b.stack_head is None and b.nlayers == 2 and b.train_initial_hidden_state is True
    st = b._get_state_dict()
    assert st["rnn_layers"] == 2 and st["train_initial_hidden_state"] is True and st["use_rnn"] is False
    b.save(tmp_path / "model.pt")
    back = FastSequenceTagger.load(tmp_path / "model.pt")
    assert back.nlayers == 2 and back.train_initial_hidden_state is True and not back.use_rnn
    old = a._get_state_dict()
    del old["rnn_layers"], old["train_initial_hidden_state"]          # a file from before the switches
    plain = FastSequenceTagger._init_model_with_state_dict(old)
    assert plain.nlayers == 1 and plain.train_initial_hidden_state is False
