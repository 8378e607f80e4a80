"""GPU: FastCharacterEmbeddings in the stacked tagger, end to end, on one tiny frozen TransformerWordEmbeddings plus the character
embedding (the encoders of tests/test_gpu_pool_e2e.py).

  (a) one training step with the pre-RNN dropouts on (element, locked and WordDropout): the loss, the head's gradients and the
      character gradients against float64 autograd of the whole step (charref.stack_reference64: lstmbwdref.head_reference64's model
      extended by the character model), both sides under the masks the step drew -- the frozen columns as gather_rows_drop leaves them,
      the character block times charref.block_mask --, within selftest.STEP_TOL's loss and gradient bounds; the block the input GEMM
      read is the character kernel's, the frozen columns are untouched by it;
  (b) a forward-only pass writes the block into X itself, unmasked, and _stack_compute never holds it;
  (c) a stack WITHOUT the embedding issues exactly the library calls it issued before the character step existed: the training step's
      sequence written out from the head's stages, none of the three new entry points among them;
  (d) ModelFinetuner with embeddings_storage_mode none / gpu / cpu, seeded alike: the loss falls, the character parameters move,
      the three trajectories agree within selftest.TRAIN_TOL (the rule of tests/test_gpu_store_e2e.py), the store never holds the
      block; stack-model.pt carries the character state and a fresh tagger that loads it reproduces the emissions bit for bit;
  (e) one ReinforcementTrainer run of two episodes, the embedding selected, then deselected by the curriculum: deselected, neither
      kernel is launched and the character parameters stay bit for bit what episode 1 left (SGD without momentum, zero gradient)."""
import json

import numpy as np
import pytest
import torch

import charref as C
import selftest

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
CHAR_CALLS = ("kbner_char_lstm_fwd", "kbner_char_lstm_bwd")
N_TRAIN, N_DEV, N_TEST, MBS, EPOCHS = 6, 3, 3, 2, 3


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


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


class Calls:
    def __init__(self, monkeypatch):
        from kbner import lib as L
        self.names = []
        call = L.call

        def spy(name, *a):
            self.names.append(name)
            return call(name, *a)
        monkeypatch.setattr(L, "call", spy)

    def count(self, *names):
        return sum(n in names for n in self.names)


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    import tiny_assets
    from flair.custom_data_loader import BatchedData
    from flair.data import Dictionary, Sentence
    from flair.embeddings import FastCharacterEmbeddings, StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    d = tmp_path_factory.mktemp("char_e2e")
    tiny_assets.build_model_dir(str(d / "enc_a"), seed=0)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)
    texts = [("alice zalandoresearchuniversitycambridge x berlin wikipedia", "S-PER O O B-LOC E-LOC"), ("bob", "S-PER"),
             ("alice museum population", "O O S-PER")]

    def make(with_char=True, **kw):
        torch.manual_seed(99)
        embs = [TransformerWordEmbeddings(model=str(d / "enc_a"), layers="-1", pooling_operation="first")]
        if with_char:
            embs.append(FastCharacterEmbeddings(vocab=[w for t, _ in texts for w in t.split() if w != "museum"]))   # 'm' is unknown
        args = dict(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=True,
                    dropout=0.0, word_dropout=0.0, locked_dropout=0.0, sentence_loss=True)
        args.update(kw)
        return FastSequenceTagger(**args)

    sents = []
    for toks, tags in texts:
        s = Sentence(toks)
        for t, v in zip(s, tags.split()):
            t.add_tag("ner", v)
        s.ner_tags = [td.get_idx_for_item(v) for v in tags.split()]
        sents.append(s)
    return make, BatchedData(sents), sents


def _ref_layout(head, M, B, n):
    """a matrix in the head's padded column layout -> the reference's [B, n, D] (float64)"""
    x = np.zeros((B * n, head.D))
    ref = 0
    for w, c in zip(head.blocks, head.cols):
        x[:, ref:ref + w] = M[:B * n, c:c + w].float().cpu().numpy()
        ref += w
    return x.reshape(B, n, head.D)


def _np_head_state(st):
    return {"rnn": {k: v.numpy() for k, v in st["rnn"].items()}, "linear.weight": st["linear.weight"].numpy(),
            "linear.bias": st["linear.bias"].numpy(), "transitions": st["transitions"].numpy()}


def test_a_one_step_against_float64_autograd_of_the_whole_step(assets, monkeypatch):
    from kbner import ops
    from kbner import stack as K
    make, batch, sents = assets
    tagger = make(dropout=0.25, locked_dropout=0.5, word_dropout=0.3)
    tagger.train()
    # the sites of this step, fixed: both pre-RNN masks, WordDropout at position 1 of every sentence; the post-RNN sites off (the
    # float64 model has none)
    fixed = (np.array([False, True, False, False, False]), ((111, ops.drop_thresh(0.25)), (222, ops.drop_thresh(0.5))),
             (ops.NO_DROP, ops.NO_DROP))
    tagger.enable_stack_training()._draw_dropout = lambda n: fixed
    slot = tagger._char_slot
    cemb = tagger._stack_embs[slot]
    seen = {}
    fwd = K.CharStep.forward

    def forward(this, Xt, sites, n, save=True):
        before = Xt.clone()
        fwd(this, Xt, sites, n, save)
        seen.update(before=before, after=Xt.clone(), step=this)
    monkeypatch.setattr(K.CharStep, "forward", forward)
    loss = float(tagger.forward_backward(batch))
    torch.cuda.synchronize()
    head, net = tagger.stack_head, tagger._char_net()
    word, pre, post = head.last_drop
    assert word.any() and not word.all() and pre[0][1] and pre[1][1]
    B, n = len(sents), max(len(s) for s in sents)
    col, W2 = head.cols[slot], 2 * net.Hc
    # the matrix the input GEMM read: the character block arrived as zeros, nothing else was touched
    before, after = seen["before"], seen["after"]
    assert not bool(before[:, col:col + 64].any())
    keep = torch.ones(after.shape[1], dtype=torch.bool)
    keep[col:col + W2] = False
    assert torch.equal(_bits(after[:, keep]), _bits(before[:, keep])) and not bool(after[:, col + W2:col + 64].any())
    step = seen["step"]
    chars, lens, rows = cemb.char_batch(batch, n)
    dropped = np.tile(word, B)[rows]
    assert (step.tab.rows.cpu().numpy() == np.where(dropped, -1, rows)).all() and dropped.any()
    cmask = C.block_mask(np.where(dropped, -1, rows), n, col, net.Hc, pre[0], pre[1])
    p = C.NS(emb=net.param("emb").cpu().numpy().astype(np.float64), wih=net.param("wih").cpu().numpy().astype(np.float64),
             whh=net.param("whh").cpu().numpy().astype(np.float64), bih=net.param("bias_ih").cpu().numpy().astype(np.float64),
             bhh=net.param("bias_hh").cpu().numpy().astype(np.float64))
    r64 = C.evaluate(p, chars, lens, np.where(dropped, -1, rows))
    got_block = after[:B * n, col:col + W2].float().cpu().numpy()
    live = ~dropped
    assert (got_block[rows[live]] == C.stored(C.stored(r64.h[live]), cmask[live])).mean() > 0.99      # (a rounding boundary may flip)
    assert not got_block[np.setdiff1d(np.arange(B * n), rows[live])].any()
    # float64 autograd of the whole step on what the GEMM saw in the frozen columns
    x = _ref_layout(head, before, B, n)
    c0 = sum(head.blocks[:slot])
    tags = np.zeros((B, n), np.int64)
    for b, s in enumerate(sents):
        tags[b, :len(s)] = s.ner_tags
    st = tagger._stack_state
    ref_loss, ref_g, ref_c, _ = C.stack_reference64(x, (c0, c0 + W2), {k: v.numpy() for k, v in st["char"].items()}, chars, lens,
                                                    np.where(dropped, -1, rows), cmask, np.asarray([len(s) for s in sents]), tags,
                                                    _np_head_state(st), tagger.start_idx, tagger.stop_idx)
    g = head.state_of(head.g)
    got = {"rnn." + k: v.numpy() for k, v in g["rnn"].items()}
    got.update({k: g[k].numpy() for k in ("linear.weight", "linear.bias", "transitions")})
    got_c = {k: v.numpy() for k, v in net.state(net.g).items()}
    print("[char] loss %.6f (float64 %.6f)" % (loss, ref_loss))
    rows_ = []
    for name, a, b in [(k, got[k], ref_g[k]) for k in sorted(ref_g)] + [(k, got_c[k], ref_c[k]) for k in sorted(ref_c)]:
        rows_.append((name, rel(a, b), cos(a, b)))
        print("[char]   %-36s rel %.3e  cos %.6f" % rows_[-1])
    assert abs(loss - ref_loss) / abs(ref_loss) < selftest.STEP_TOL["loss_rel"]
    bad = [r for r in rows_ if not (r[1] < selftest.STEP_TOL["grad_worst_rel"] and r[2] > selftest.STEP_TOL["grad_min_cos"])]
    assert not bad, bad
    assert np.array_equal(got_c["char_layer.bias_ih_l0"], got_c["char_layer.bias_hh_l0"])
    # the gradient of a character no live word holds is exactly zero; ONE clip norm covers both arenas
    unused = np.setdiff1d(np.arange(net.V), np.unique(np.concatenate([chars[w, :lens[w]] for w in np.nonzero(live)[0]])))
    assert len(unused) and not got_c["char_embedding.weight"][unused].any()
    opt = K.StackOptimizer(head, name="SGD", lr=0.1)
    want = float((head.g.double() ** 2).sum() + (net.g.double() ** 2).sum())
    nsq = float(opt.step()[0])
    assert abs(nsq - want) / want < 1e-5 and not bool(net.g.any()) and not bool(head.g.any())


def test_b_a_forward_only_pass_writes_the_block_into_x(assets, monkeypatch):
    make, batch, sents = assets
    tagger = make()
    tagger.eval()
    calls = Calls(monkeypatch)
    Xc = tagger._stack_compute(batch)[0]
    assert calls.count(*CHAR_CALLS) == 0
    X, lengths, B, n = tagger._stack_input(batch)
    assert calls.count("kbner_char_lstm_fwd") == 1 and calls.count("kbner_char_lstm_bwd") == 0
    head, net, slot = tagger.stack_head, tagger._char_net(), tagger._char_slot
    col, W2 = head.cols[slot], 2 * net.Hc
    assert not bool(Xc[:, col:col + 64].any())
    keep = torch.ones(X.shape[1], dtype=torch.bool)
    keep[col:col + W2] = False
    assert torch.equal(_bits(X[:, keep]), _bits(Xc[:, keep]))
    chars, lens, rows = tagger._stack_embs[slot].char_batch(batch, n)
    p = C.NS(emb=net.param("emb").cpu().numpy(), wih=net.param("wih").cpu().numpy(), whh=net.param("whh").cpu().numpy(),
             bih=net.param("bias_ih").cpu().numpy(), bhh=net.param("bias_hh").cpu().numpy())
    r64, r32 = C.evaluate(p, chars, lens, rows), C.evaluate(p, chars, lens, rows, f32=True)
    C.check({"h": X[:B * n, col:col + W2].float().cpu().numpy()[rows]}, r64, r32, what="forward-only block")
    em = tagger.forward(batch)
    assert bool(torch.isfinite(em).all())


def test_c_a_stack_without_the_embedding_issues_the_calls_it_always_issued(assets, monkeypatch):
    """the training step's library calls, written out from the stages of BiLSTMHead.loss_backward as they stood before the character
    step: producers, dropout gather, input GEMM, recurrence, head, CRF, their backwards, the weight-gradient GEMMs, the column sums"""
    make, batch, sents = assets
    tagger = make(with_char=False, dropout=0.25, locked_dropout=0.5, word_dropout=0.3)
    tagger.train()
    tagger.forward_backward(batch)                # (whatever happens once is behind us)
    calls = Calls(monkeypatch)
    tagger.forward_backward(batch)
    steps = int(max(len(s) for s in sents))
    T = tagger.tagset_size
    names = list(calls.names)
    assert calls.count(*CHAR_CALLS, "kbner_char_lstm_ws_bytes") == 0
    i = names.index("kbner_gather_rows_drop")
    head_part = names[i:]
    gemm = [n for n in head_part if n.startswith("kbner_gemm")]
    expect = ["kbner_gather_rows_drop", gemm[0], "kbner_lstm_seq_train", "kbner_gather_rows_drop", "kbner_head_fwd", "kbner_gather_rows_f32",
              "kbner_crf_nll_fwd", "kbner_wdiff_sum", "kbner_crf_nll_bwd", "kbner_scatter_rows_f32" if T % 4 == 0 else "kbner_scatter_add_rows_f32",
              "kbner_head_bwd_dx", "kbner_head_bwd_dw", "kbner_scatter_rows_drop", "kbner_lstm_seq_bwd", gemm[1], gemm[2], "kbner_colsum", "kbner_colsum"]
    print("[char] the head's calls without the embedding: %s" % " ".join(head_part))
    assert head_part == expect
    assert len(gemm) == 3 and steps >= 2                                  # no fourth GEMM: the dXt window belongs to the character step
    # ... and the forward-only pass: the producers, nothing after them
    tagger.eval()
    calls.names.clear()
    tagger._stack_input(batch)
    assert calls.names[-1] == "kbner_gather_rows_ld"
    assert calls.count(*CHAR_CALLS) == 0


def _np_all(st):
    head = np.concatenate([np.asarray(st["rnn"][k], np.float64).ravel() for k in sorted(st["rnn"])] +
                          [np.asarray(st[k], np.float64).ravel() for k in ("linear.weight", "linear.bias", "transitions")])
    char = np.concatenate([np.asarray(st["char"][k], np.float64).ravel() for k in sorted(st["char"])])
    return head, char


def _config(root, name, trainer, storage, optimizer, **train):
    import yaml
    tblock = {"distill_mode": False, "optimizer": optimizer, "sentence_level_batch": True}
    if trainer == "ReinforcementTrainer":
        tblock.update(controller_optimizer="SGD", controller_learning_rate=0.1)
    cfg = {trainer: tblock, "Controller": {"model_structure": None},
           "embeddings": {"TransformerWordEmbeddings-0": {"layers": "-1", "model": str(root / "enc_a"), "pooling_operation": "first"},
                          "FastCharacterEmbeddings": {"char_embedding_dim": 25, "hidden_size_char": 25}},
           "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40, "use_rnn": True,
                                            "sentence_loss": True, "use_crf": True}},
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
    from kbner import lib as L
    path = _config(root, name, tname, storage, optimizer, **train)
    torch.manual_seed(2024)
    cp = ConfigParser(Params.from_file(str(path)))
    student = cp.create_student()
    assert student.char_map is student._stack_embs[student._char_slot].char_dictionary
    trainer = getattr(flair.trainers, tname)(student, None, cp.corpus, config=cp.config, **cp.config[tname])
    start = _np_all(student._stack_state)
    steps, names = [], []
    call = L.call
    mp = pytest.MonkeyPatch()

    def spy(nm, *a):
        names.append(nm)
        return call(nm, *a)
    mp.setattr(L, "call", spy)

    def hook(batches, ls):
        store = student.__dict__.get("_feature_store")
        steps.append(dict(losses=[float(x) for x in ls], char=_np_all(student._stack_state)[1], fwd=names.count(CHAR_CALLS[0]),
                          bwd=names.count(CHAR_CALLS[1]), selection=None if student.selection is None else [float(x) for x in student.selection],
                          store_want=None if store is None else list(store.want)))
    trainer.stack_step_hook = hook
    try:
        res = trainer.train(cp.get_target_path, **cp.config["train"])
    finally:
        mp.undo()
    return dict(steps=steps, res=res, start=start, base=cp.get_target_path, student=student, cp=cp)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    import tiny_assets
    root = tmp_path_factory.mktemp("char_train")
    tiny_assets.build_model_dir(str(root / "enc_a"), seed=0)
    tiny_assets.write_conll_corpus(str(root / "data"), n_train=N_TRAIN, n_dev=N_DEV, n_test=N_TEST, seed=3)
    out = {"root": root}
    for mode in ("none", "gpu", "cpu"):
        out[mode] = _run(root, "char_" + mode, "ModelFinetuner", mode, "AdamW")
    return out


def test_d_finetuner_trains_the_character_parameters_in_every_storage_mode(runs):
    none = runs["none"]
    steps = none["steps"]
    assert len(steps) == EPOCHS * (N_TRAIN // MBS)
    first, last = np.mean([np.mean(s["losses"]) for s in steps[:N_TRAIN // MBS]]), np.mean([np.mean(s["losses"]) for s in steps[-(N_TRAIN // MBS):]])
    print("[char] mean loss of the first epoch %.4f, of the last %.4f" % (first, last))
    assert last < first
    moved = np.abs(steps[-1]["char"] - none["start"][1])
    assert moved.max() > 1e-3 and (moved > 0).mean() > 0.5                       # the character parameters move
    assert [s["fwd"] for s in steps] == sorted(s["fwd"] for s in steps) and steps[-1]["bwd"] == len(steps)
    best = torch.load(str(none["base"] / "stack-model.pt"), map_location="cpu", weights_only=False)
    assert set(best) >= {"char", "char_dictionary"} and best["char_dictionary"] == none["student"].char_map
    for mode in ("gpu", "cpu"):
        r = runs[mode]
        assert np.array_equal(r["start"][0], none["start"][0]) and np.array_equal(r["start"][1], none["start"][1])
        worst = max(abs(x - y) / abs(x) for a, b in zip(steps, r["steps"]) for x, y in zip(a["losses"], b["losses"]))
        b_ = torch.load(str(r["base"] / "stack-model.pt"), map_location="cpu", weights_only=False)
        (ha, ca), (hb, cb) = _np_all(best), _np_all(b_)
        c_head, c_char = cos(ha - none["start"][0], hb - none["start"][0]), cos(ca - none["start"][1], cb - none["start"][1])
        print("[char] %s against none: worst relative loss difference %.3e, update cosine head %.9f char %.9f" % (mode, worst, c_head, c_char))
        assert worst < selftest.TRAIN_TOL["loss_rel_max"]
        assert c_head > selftest.TRAIN_TOL["delta_cos_min"] and c_char > selftest.TRAIN_TOL["delta_cos_min"]
        slot = r["student"]._char_slot
        assert all(s["store_want"] is not None and s["store_want"][slot] is False for s in r["steps"])       # never read from the store


def test_d_save_then_load_reproduces_the_emissions_bit_for_bit(runs, assets):
    import flair
    from flair.custom_data_loader import BatchedData
    r = runs["none"]
    student = r["student"]
    student.eval()
    batch = BatchedData([r["cp"].corpus.train[i] for i in range(3)])
    state = torch.load(str(r["base"] / "stack-model.pt"), map_location="cpu", weights_only=False)
    student.load_stack_state(state)                      # (the trainer left the LAST weights in place; the file holds the best)
    want = student.forward(batch).clone()
    torch.manual_seed(7)                                 # another initialisation: everything must come from the file
    fresh = r["cp"].create_student()
    fresh.eval()
    assert not torch.equal(_bits(fresh.forward(batch)), _bits(want))
    fresh.load_stack_state(state)
    assert torch.equal(_bits(fresh.forward(batch)), _bits(want))
    assert fresh._stack_embs[fresh._char_slot].char_dictionary == state["char_dictionary"]


def test_e_a_deselected_character_embedding_launches_nothing_and_keeps_its_parameters(runs):
    root = runs["root"]
    with open(root / "forced.json", "w") as f:
        f.write(json.dumps([[1.0, 1.0], [1.0, 0.0]]))      # slots in sorted-name order: [encoder, Char]
    r = _run(root, "char_ace", "ReinforcementTrainer", "gpu", "SGD", max_episodes=2, curriculum_file=str(root / "forced.json"))
    assert r["student"]._char_slot == 1
    steps = r["steps"]
    per = EPOCHS * (N_TRAIN // MBS)
    ep1 = [s for s in steps if s["selection"] == [1.0, 1.0]]
    ep2 = [s for s in steps if s["selection"] == [1.0, 0.0]]
    assert len(ep1) >= 1 and len(ep2) >= 1 and len(ep1) + len(ep2) == len(steps) <= 2 * per and steps.index(ep2[0]) == len(ep1)
    assert ep1[-1]["bwd"] == len(ep1) and np.abs(ep1[-1]["char"] - r["start"][1]).max() > 0
    # deselected: zero launches of the two kernels (dev evaluations included), parameters bit for bit what episode 1 left
    assert all(s["fwd"] == ep2[0]["fwd"] and s["bwd"] == ep1[-1]["bwd"] for s in ep2)
    assert all(np.array_equal(s["char"], ep1[-1]["char"]) for s in ep2)
