"""GPU: training of the stacked tagger's BiLSTM -> linear -> CRF head on frozen features (kbner.stack.BiLSTMHead.loss_backward,
StackOptimizer, FastSequenceTagger(use_rnn=True).forward_backward).

Head gradients: the loss and every parameter's gradient, un-padded through state() layouts, against float64 autograd
(torch.nn.LSTM + linear + oracle.train_step.crf_nll_torch; lstmbwdref.head_reference64).  Bound per tensor: relative L2 <= 3 x the
relative L2 of lstmbwdref.emulate (the same computation with values rounded at the implementation's storage points, another
summation order, one draw of the rounding noise; 3 x is the project's margin, selftest.STEP_TOL) against float64 on the same inputs,
computed here on the CPU, and in no case looser than STEP_TOL's loss_rel, grad_linear.weight and grad_transitions; cosine >=
STEP_TOL["grad_min_cos"]; padded arena entries receive exactly 0.  Dropout: each of the five sites on its own.  Tagger:
forward_backward returns forward_loss's value, its gradients under the same bound, refusals by name.  Trainer: ModelFinetuner.train
on a six-sentence corpus, 2 epochs, AdamW and SGD: after every optimizer step the update against a float64 oracle trainer fed the
same batches (selftest.TRAIN_TOL), stack-model.pt reloaded bit for bit, train.py --test.

Figures of the MI355X run that accompanied this module (16 tests, 21 s; -s prints every tensor): the kernel path's relative L2
against float64 equals the emulation's to two or three digits everywhere (worst gradient 6.0e-3, rnn.weight_hh_l0 of the tagger case,
emulation 6.0e-3, bound 1.8e-2; worst cosine 0.999982); loss 5e-6 to 8e-5.  Trainer: update cosine >= 0.999913 (AdamW, step 1) and
>= 0.999995 (SGD) against the bound 0.9985."""
import numpy as np
import pytest
import torch

import lstmbwdref as R
import rowref
import selftest

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SFX = ("", "_reverse")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def problem(B, n, D, H, T, seed):
    """a random head in the reference's layout, bf16-valued features with ragged lengths (one of them n, one 1), tags"""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    st = {"rnn": {}}
    for s in SFX:
        st["rnn"]["weight_ih_l0" + s] = rng.uniform(-k, k, (4 * H, D)).astype(np.float32)
        st["rnn"]["weight_hh_l0" + s] = rng.uniform(-k, k, (4 * H, H)).astype(np.float32)
        st["rnn"]["bias_ih_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
        st["rnn"]["bias_hh_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
    st["linear.weight"] = rng.uniform(-1, 1, (T, 2 * H)).astype(np.float32) / np.float32(np.sqrt(2 * H)) * 4
    st["linear.bias"] = rng.standard_normal(T).astype(np.float32)
    tr = rng.standard_normal((T, T)).astype(np.float32)
    tr[T - 2, :] = -1e12
    tr[:, T - 1] = -1e12
    st["transitions"] = tr
    lengths = rng.integers(1, n + 1, size=B)
    lengths[0] = n
    if B > 1:
        lengths[1] = 1
    x = rowref.bf16_round(rng.standard_normal((B, n, D))).astype(np.float64)
    for b in range(B):
        x[b, lengths[b]:] = 0
    tags = rng.integers(0, T - 2, (B, n))
    blocks = [D - 8, 8] if D > 8 else [D]
    return R.NS(st=st, lengths=lengths, x=x, tags=tags, blocks=blocks, B=B, n=n, D=D, H=H, T=T, start=T - 2, stop=T - 1)


def build_head(p, trainable=True):
    from kbner import stack as K
    st = p.st
    return K.BiLSTMHead({k: torch.from_numpy(v) for k, v in st["rnn"].items()}, st["linear.weight"], st["linear.bias"], p.blocks, p.H,
                        "cuda", transitions=st["transitions"], trainable=trainable)


def device_input(p, head):
    from kbner import batch as kb
    X = head.new_input(p.B, p.n)
    xb = torch.from_numpy(p.x).to(BF16).view(p.B * p.n, p.D)
    ref = 0
    for w, c in zip(p.blocks, head.cols):
        X[:p.B * p.n, c:c + w] = xb[:, ref:ref + w].cuda()
        ref += w
    hb = kb.assemble(np.zeros((p.B, 1), np.int64), np.ones((p.B, 1), np.int64), np.full((p.B, p.n), -1, np.int64), p.tags.astype(np.int64),
                     p.lengths.astype(np.int64), None)
    return X, kb.to_device(hb, "cuda")


def flat_grads(g):
    out = {"rnn." + k: v for k, v in g["rnn"].items()}
    out.update({k: g[k] for k in ("linear.weight", "linear.bias", "transitions")})
    return {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float64) for k, v in out.items()}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


CAP = {"loss": selftest.STEP_TOL["loss_rel"], "linear.weight": selftest.STEP_TOL["grad_linear.weight"],
       "transitions": selftest.STEP_TOL["grad_transitions"]}


def compare(what, loss, grads, ref_loss, ref_grads, emu_loss, emu_grads):
    fails = []
    rows = [("loss", abs(loss - ref_loss) / abs(ref_loss), abs(emu_loss - ref_loss) / abs(ref_loss), 1.0)]
    for k in sorted(ref_grads):
        rows.append((k, rel(grads[k], ref_grads[k]), rel(emu_grads[k], ref_grads[k]), cos(grads[k], ref_grads[k])))
    for k, got, emu, c in rows:
        bound = min(3.0 * emu, CAP.get(k, np.inf))
        print("[stacktrain] %s %-26s rel %.3e  emulation %.3e  bound %.3e  cos %.6f" % (what, k, got, emu, bound, c))
        if not got <= bound or not c >= selftest.STEP_TOL["grad_min_cos"]:
            fails.append((k, got, bound, c))
    assert not fails, (what, fails)


@pytest.mark.parametrize("B,n,D,H,T", [(3, 7, 40, 24, 9), (5, 19, 96, 100, 9), (33, 12, 64, 32, 9), (4, 9, 128, 1000, 9), (3, 7, 40, 24, 77)])
def test_head_loss_and_gradients_against_float64_autograd(B, n, D, H, T):
    p = problem(B, n, D, H, T, seed=B + H + T)
    head = build_head(p)
    X, db = device_input(p, head)
    loss = float(head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop))
    torch.cuda.synchronize()
    grads = flat_grads(head.state_of(head.g))
    ref_loss, ref_grads, ref_em = R.head_reference64(p.x, p.lengths, p.tags, p.st, p.start, p.stop)
    emu_loss, emu_grads = R.emulate(p.x, p.lengths, p.tags, p.st, p.start, p.stop)
    compare("B%d n%d D%d H%d T%d" % (B, n, D, H, T), loss, grads, ref_loss, ref_grads, emu_loss, emu_grads)
    # the forward alone (emissions(), inference kernels) gives the same emissions bit for bit
    em = head.emissions(X, p.lengths, B, n)
    assert torch.equal(em.view(torch.int32), head.last_emissions.view(torch.int32))
    # padded arena entries: gradient exactly 0
    g = head.g.clone()
    ones = {"rnn": {k: np.ones_like(v) for k, v in p.st["rnn"].items()}, "linear.weight": np.ones_like(p.st["linear.weight"]),
            "linear.bias": np.ones_like(p.st["linear.bias"]), "transitions": np.ones_like(p.st["transitions"])}
    head.load_state(ones)
    pad = head.arena == 0
    assert bool(pad.any()) and not bool(g[pad].any()), "a padded arena entry received a gradient"
    # a second micro-batch accumulates; loss_scale scales the gradient
    head.load_state(p.st)
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop, loss_scale=0.5)
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop, loss_scale=0.5)
    g2 = flat_grads(head.state_of(head.g))
    assert all(rel(g2[k], grads[k]) < 2e-3 for k in grads)       # (fp32 atomics in another order, 0.5 x exact in bf16)


def test_state_round_trip_and_optimizer_steps():
    from kbner import stack as K
    p = problem(5, 9, 72, 100, 9, seed=3)
    head = build_head(p)
    back = head.state()
    for k, v in flat_grads(back).items():
        want = p.st["rnn"][k[4:]] if k.startswith("rnn.") else p.st[k]
        assert np.array_equal(v, np.asarray(want, np.float64)), k
    X, db = device_input(p, head)
    ref_loss, ref_grads, _ = R.head_reference64(p.x, p.lengths, p.tags, p.st, p.start, p.stop)
    gnorm = float(np.sqrt(sum((v ** 2).sum() for v in ref_grads.values())))
    for name in ("SGD", "AdamW"):
        head.load_state(p.st)
        opt = K.StackOptimizer(head, name=name, lr=0.1 if name == "SGD" else 1e-3, lr_rate=0.5, max_norm=gnorm / 2)
        head.loss_backward(X, p.lengths, p.B, p.n, db, p.start, p.stop)
        nsq = float(opt.step()[0])
        torch.cuda.synchronize()
        assert abs(np.sqrt(nsq) - gnorm) / gnorm < 1e-2 and not bool(head.g.any())
        new = flat_grads(head.state())
        clip = (gnorm / 2) / (gnorm + 1e-6)
        for k, g in ref_grads.items():
            old = np.asarray(p.st["rnn"][k[4:]] if k.startswith("rnn.") else p.st[k], np.float64)
            lr = opt.lr * (1.0 if k.startswith("linear.") else opt.lr_rate)
            if name == "SGD":
                want = -lr * clip * g
            else:     # first AdamW step: m / (sqrt(v) + eps) = g / (|g| + eps'), step size lr
                gc = clip * g
                want = -lr * gc / (np.abs(gc) + 1e-6 / np.sqrt(1 - 0.999))
            delta = new[k] - old
            live = np.abs(g) > 1e-3 * np.abs(g).max()
            c = cos(delta[live], want[live])
            print("[stacktrain] %s first step %-26s update cosine %.6f" % (name, k, c))
            assert c > selftest.TRAIN_TOL["delta_cos_min"], (name, k, c)
        # the shadow the next forward reads is the bf16 rounding of the arena
        assert torch.equal(head.shadow, head.arena[:head.n_shadow].to(BF16))
        assert torch.equal(head.grp.whh.reshape(-1), head.param("whh").to(BF16).reshape(-1))


SITES = ["pre_dropout", "word_dropout", "pre_locked", "post_dropout", "post_locked"]


@pytest.mark.parametrize("site", SITES)
def test_each_dropout_site_on_its_own(site):
    from kbner import ops
    p = problem(5, 9, 72, 40, 9, seed=11)
    head = build_head(p)
    X, db = device_input(p, head)
    B, n, R_, Hp = p.B, p.n, p.B * p.n, head.Hp
    th = ops.drop_thresh(0.4)
    word = None
    pre, post = [ops.NO_DROP, ops.NO_DROP], [ops.NO_DROP, ops.NO_DROP]
    if site == "pre_dropout":
        pre[0] = (1234567, th)
    elif site == "pre_locked":
        pre[1] = (7654321, th)
    elif site == "post_dropout":
        post[0] = (2222, th)
    elif site == "post_locked":
        post[1] = (3333, th)
    else:
        word = np.zeros(n, bool)
        word[[1, n - 1]] = True
    sites = (word, tuple(pre), tuple(post))
    head.train(True)
    loss_d = float(head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop, drop=sites))
    g_d = head.g.clone()
    feat_d, out_d = head.last_feat.clone(), head.last_out.clone()
    head.g.zero_()

    def mask(pair, width):
        e = ops.dropout_mask(1, R_, width, pair[0][0], pair[0][1])[0] if pair[0][1] else torch.ones((R_, width), device="cuda")
        l = ops.dropout_mask(1, B, width, pair[1][0], pair[1][1])[0] if pair[1][1] else torch.ones((B, width), device="cuda")
        return e * l.repeat_interleave(n, dim=0)

    if site in ("post_dropout", "post_locked"):
        m = mask(post, 2 * Hp)
        assert 0.3 < float((m == 0).float().mean()) < 0.5
        assert torch.equal(feat_d, (out_d[:R_].float() * m).to(BF16)), "the post-RNN features are not the masked BiLSTM output"
        # against float64 autograd with the same masks on the BiLSTM output
        mh = m.cpu().numpy().reshape(B, n, 2 * Hp)
        pm = np.concatenate([mh[:, :, :p.H], mh[:, :, Hp:Hp + p.H]], 2)
        ref_loss, ref_grads, _ = R.head_reference64(p.x, p.lengths, p.tags, p.st, p.start, p.stop, post_mask=pm)
        grads = flat_grads(head.state_of(g_d))
        assert abs(loss_d - ref_loss) / abs(ref_loss) < selftest.STEP_TOL["loss_rel"]
        for k in ref_grads:
            assert rel(grads[k], ref_grads[k]) < selftest.STEP_TOL["grad_worst_rel"] and cos(grads[k], ref_grads[k]) > selftest.STEP_TOL["grad_min_cos"], k
        return
    # pre-RNN sites: the run equals the run without dropout on the masked input
    m = mask(pre, head.Dp)
    if word is not None:
        m = m * torch.from_numpy(np.tile(~word, B)).cuda()[:, None].float()
        assert set(np.unique(m.cpu().numpy())) == {0.0, 1.0}                    # whole positions, every sentence, no rescaling
        assert not bool(m.view(B, n, -1)[:, 1].any()) and not bool(m.view(B, n, -1)[:, n - 1].any())
    Xm = X.clone()
    Xm[:R_] = (X[:R_].float() * m).to(BF16)
    loss_m = float(head.loss_backward(Xm, p.lengths, B, n, db, p.start, p.stop, drop=None))
    assert loss_m == loss_d and loss_m != float(head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop, drop=None))
    head.g.zero_()
    head.loss_backward(Xm, p.lengths, B, n, db, p.start, p.stop, drop=None)
    assert torch.equal(head.last_out, out_d)
    a, b = flat_grads(head.state_of(head.g)), flat_grads(head.state_of(g_d))
    assert all(rel(a[k], b[k]) < 1e-5 for k in a)                                # (fp32 atomics in another order)


def test_eval_mode_draws_nothing_and_default_head_allocates_nothing():
    p = problem(3, 5, 40, 24, 9, seed=2)
    plain = build_head(p, trainable=False)
    assert plain.arena is None and not hasattr(plain, "g")
    X, db = device_input(p, plain)
    with pytest.raises(Exception):
        plain.loss_backward(X, p.lengths, p.B, p.n, db, p.start, p.stop)
    head = build_head(p)
    head.dropout = head.word_dropout = head.locked_dropout = 0.3
    head.train(False)
    head.loss_backward(X, p.lengths, p.B, p.n, db, p.start, p.stop)
    assert head.last_drop is None
    head.train(True)
    head.loss_backward(X, p.lengths, p.B, p.n, db, p.start, p.stop)
    word, pre, post = head.last_drop
    assert word.shape == (p.n,) and pre[0][1] == pre[1][1] == post[0][1] == post[1][1] > 0 and len({pre[0][0], pre[1][0], post[0][0], post[1][0]}) == 4
    assert torch.equal(plain.emissions(X, p.lengths, p.B, p.n), head.emissions(X, p.lengths, p.B, p.n))


# ====================================================================== the tagger
@pytest.fixture(scope="module")
def tagger_and_batch(tmp_path_factory):
    import tiny_assets
    from flair.custom_data_loader import BatchedData
    from flair.data import Dictionary, Sentence
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    d = tmp_path_factory.mktemp("stacktrain")
    tiny_assets.build_model_dir(str(d / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(d / "enc_b"), seed=5)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)

    def make(**kw):
        embs = [TransformerWordEmbeddings(model=str(d / "enc_a"), layers="-1", pooling_operation="first"),
                TransformerWordEmbeddings(model=str(d / "enc_b"), layers="-1", pooling_operation="first")]
        args = dict(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=True,
                    dropout=0.0, word_dropout=0.0, locked_dropout=0.0, sentence_loss=True)
        args.update(kw)
        return FastSequenceTagger(**args), embs
    texts = [("a b c d e", "O S-PER O B-LOC E-LOC"), ("f", "S-PER"), ("g h i", "O O S-PER")]
    sents = []
    for toks, tags in texts:
        s = Sentence(toks)
        for t, v in zip(s, tags.split()):
            t.add_tag("ner", v)
        s.ner_tags = [td.get_idx_for_item(v) for v in tags.split()]       # what ColumnDataLoader.assign_tags leaves on a sentence
        sents.append(s)
    return make, BatchedData(sents), sents


def test_tagger_forward_backward_returns_forward_loss_and_the_reference_gradients(tagger_and_batch):
    make, batch, sents = tagger_and_batch
    tagger, _ = make()
    tagger.train()
    want = float(tagger.forward_loss(batch))
    assert tagger.stack_head.arena is None                                   # nothing allocated until a training step asks
    loss = float(tagger.forward_backward(batch))
    torch.cuda.synchronize()
    assert abs(loss - want) <= 1e-6 * abs(want), (loss, want)
    head = tagger.stack_head
    assert head.arena is not None and head.training
    # the same features, in the reference's layout, through float64 autograd
    X, lengths, B, n = tagger._stack_input(batch)
    D = head.D
    x = np.zeros((B * n, D))
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
    args = (x.reshape(B, n, D), lengths, tags, stn, tagger.start_idx, tagger.stop_idx)
    ref_loss, ref_grads, _ = R.head_reference64(*args)
    emu_loss, emu_grads = R.emulate(*args)
    compare("tagger", loss, flat_grads(head.state_of(head.g)), ref_loss, ref_grads, emu_loss, emu_grads)
    names = dict(tagger.named_parameters())
    assert set(names) == {"transitions", "linear.weight", "linear.bias"} | {"rnn." + k for k in st["rnn"]}
    tagger.zero_grad()
    assert not bool(head.g.any())
    # load_stack_state refreshes the arena
    st2 = {"rnn": {k: v * 0.5 for k, v in st["rnn"].items()}, "linear.weight": st["linear.weight"], "linear.bias": st["linear.bias"],
           "transitions": st["transitions"]}
    tagger.load_stack_state(st2)
    assert tagger.stack_head is head and torch.equal(tagger._stack_state["rnn"]["weight_hh_l0"], st2["rnn"]["weight_hh_l0"])
    tagger.eval()
    assert not head.training


def test_tagger_refusals_by_name(tagger_and_batch):
    make, batch, _ = tagger_and_batch
    tagger, embs = make(dropout=0.1, locked_dropout=0.5, word_dropout=0.05)
    assert tagger.use_dropout == 0.1
    for kw, name in (({"multi_view": ([0], [1.0])}, "multi_view"), ({"distill_interpolation": 0.5}, "distill_interpolation"),
                     ({"grad_ready": lambda lo, hi: None}, "grad_ready")):
        with pytest.raises(NotImplementedError, match=name):
            tagger.forward_backward(batch, **kw)
    embs[0].fine_tune = True
    with pytest.raises(NotImplementedError, match="fine_tune"):
        tagger.forward_backward(batch)
    embs[0].fine_tune = False
    tagger.train()
    assert np.isfinite(float(tagger.forward_backward(batch)))
    assert tagger.stack_head.last_drop is not None and tagger.stack_head.dropout == 0.1


# ====================================================================== the trainer
def _features(tagger, batch):
    """the frozen features of a batch in the reference's layout [B, n, D] (float64 of the bf16 values), lengths, tags"""
    head = tagger.stack_head
    X, lengths, B, n = tagger._stack_input(batch)
    x = np.zeros((B * n, head.D))
    ref = 0
    for w, c in zip(head.blocks, head.cols):
        x[:, ref:ref + w] = X[:B * n, c:c + w].float().cpu().numpy()
        ref += w
    tags = np.zeros((B, n), np.int64)
    for b, s in enumerate(batch):
        tags[b, :len(s)] = [tagger.tag_dictionary.get_idx_for_item(t.get_tag(tagger.tag_type).value) for t in s]
    return x.reshape(B, n, head.D), np.asarray(lengths), tags


def _np_state(st):
    return {"rnn": {k: np.asarray(v, np.float64) for k, v in st["rnn"].items()}, "linear.weight": np.asarray(st["linear.weight"], np.float64),
            "linear.bias": np.asarray(st["linear.bias"], np.float64), "transitions": np.asarray(st["transitions"], np.float64)}


def _flat(st):
    return np.concatenate([st["rnn"][k].ravel() for k in sorted(st["rnn"])] + [st[k].ravel() for k in ("linear.weight", "linear.bias", "transitions")])


@pytest.mark.parametrize("optimizer", ["AdamW", "SGD"])
def test_model_finetuner_trains_the_stack_like_a_float64_oracle_trainer(optimizer, tmp_path):
    import subprocess
    import sys
    import os
    import yaml
    import tiny_assets
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    tiny_assets.build_model_dir(str(tmp_path / "enc_a"), seed=0)
    tiny_assets.build_model_dir(str(tmp_path / "enc_b"), seed=5)
    tiny_assets.write_conll_corpus(str(tmp_path / "data"), n_train=6, n_dev=3, n_test=3, seed=3)
    lr, lr_rate = (0.05, 2.0) if optimizer == "SGD" else (2e-3, 2.0)
    cfg = {"ModelFinetuner": {"distill_mode": False, "optimizer": optimizer, "sentence_level_batch": True},
           "embeddings": {"TransformerWordEmbeddings-0": {"layers": "-1", "model": str(tmp_path / "enc_a"), "pooling_operation": "first"},
                          "TransformerWordEmbeddings-1": {"layers": "-1", "model": str(tmp_path / "enc_b"), "pooling_operation": "first"}},
           "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40, "use_rnn": True,
                                            "sentence_loss": True, "use_crf": True}},
           "model_name": "stack_tiny", "target_dir": str(tmp_path / "out"), "targets": "ner", "trainer": "ModelFinetuner",
           "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(tmp_path / "tags.pkl"),
                   "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                         "data_folder": str(tmp_path / "data"), "tag_to_bioes": "ner"}},
           "train": {"learning_rate": lr, "lr_rate": lr_rate, "max_epochs": 2, "mini_batch_size": 2, "gradient_accumulation_steps": 2,
                     "monitor_test": False, "train_with_dev": False, "shuffle": True}}
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    cp = ConfigParser(Params.from_file(str(tmp_path / "cfg.yaml")))
    student = cp.create_student()
    assert student.use_rnn
    trainer = flair.trainers.ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    start = _np_state(student._stack_state)
    record = []

    def hook(batches, losses):
        record.append(([_features(student, b) for b in batches], [float(l) for l in losses], _np_state(student._stack_state)))
    trainer.stack_step_hook = hook
    base = cp.get_target_path
    res = trainer.train(base, **cp.config["train"])
    assert len(res["dev_score_history"]) == 2 and len(record) == 2 * 2          # 3 batches of 2 -> 2 optimizer steps per epoch
    for name in ("stack-model.pt", "training.log", "loss.tsv"):
        assert (base / name).exists(), name
    # ---- the float64 oracle trainer on the same batches: autograd + HF AdamW / plain SGD behind the same clip
    from oracle import optim as ooptim
    st = start
    m = v = None
    for t, (feats, losses, got) in enumerate(record, 1):
        grads, ref_losses = None, []
        for x, lengths, tags in feats:
            l, g, _ = R.head_reference64(x, lengths, tags, st, student.start_idx, student.stop_idx)
            ref_losses.append(l)
            g = {k: v_ / len(feats) for k, v_ in g.items()}
            grads = g if grads is None else {k: grads[k] + g[k] for k in g}
        for a, b in zip(losses, ref_losses):
            assert abs(a - b) / abs(b) < selftest.TRAIN_TOL["loss_rel_max"], (t, a, b)
        gn = np.sqrt(sum((g ** 2).sum() for g in grads.values()))
        clip = min(1.0, 5.0 / (gn + 1e-6))
        new = {"rnn": {}}
        for k, g in grads.items():
            old = st["rnn"][k[4:]] if k.startswith("rnn.") else st[k]
            rate = lr * (1.0 if k.startswith("linear.") else lr_rate)
            if optimizer == "SGD":
                upd = old - rate * clip * g
            else:
                m = {} if m is None else m
                v = {} if v is None else v
                mk = 0.9 * m.get(k, 0.0) + 0.1 * clip * g
                vk = 0.999 * v.get(k, 0.0) + 0.001 * (clip * g) ** 2
                m[k], v[k] = mk, vk
                upd = old - rate * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * mk / (np.sqrt(vk) + 1e-6)
            if k.startswith("rnn."):
                new["rnn"][k[4:]] = upd
            else:
                new[k] = upd
        d_ref, d_got = _flat(new) - _flat(st), _flat(got) - _flat(st)
        live = np.abs(d_ref) > 0
        c = cos(d_got[live], d_ref[live])
        print("[stacktrain] %s step %d: update cosine %.6f, losses %s" % (optimizer, t, c, losses))
        assert c > selftest.TRAIN_TOL["delta_cos_min"], (optimizer, t, c)
        st = got                                   # the next step starts from the trained parameters: errors do not compound
    assert hasattr(ooptim, "adamw_hf_step")         # (the update above is that function's formula, written out per tensor)
    # ---- stack-model.pt: a fresh tagger loading it reproduces the trained tagger's emissions bit for bit
    student.eval()
    batch = record[0][0] and [s for s in cp.corpus.dev_list[0]][:3]
    from flair.custom_data_loader import BatchedData
    dev = BatchedData(batch)
    best = torch.load(str(base / "stack-model.pt"), map_location="cpu", weights_only=False)
    student.load_stack_state(best)
    want = student.forward(dev).clone()
    fresh = ConfigParser(Params.from_file(str(tmp_path / "cfg.yaml"))).create_student()
    fresh.load_stack_state(best)
    fresh.eval()
    assert fresh.stack_head.arena is None
    assert torch.equal(fresh.forward(dev).view(torch.int32), want.view(torch.int32))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "train.py"), "--config", str(tmp_path / "cfg.yaml"), "--test"],
                       cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
