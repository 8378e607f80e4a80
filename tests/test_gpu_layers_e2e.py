"""GPU: the encoder layer selection end to end.
  - one forward + backward of kbner.engine.Tagger on the tiny model of tests/selftest.py (L2, H128, S64, B2) for the selections
    (-1,-2), (-2,), (0,1,2) and the mean of (-1,-2,-3), against tests/layersref.py's autograd restatement: loss, emissions, the head's
    and the transitions' gradients and every encoder parameter's gradient under selftest.STEP_TOL, unchanged.  With (-2,) the top
    layer takes no part: its gradients are exactly zero here and absent in the oracle.  (-1,) through the same code reproduces
    selftest.check_step().
  - a FastSequenceTagger over TransformerWordEmbeddings(layers="-1,-2") on the tiny assets: two optimizer steps, evaluate, predict,
    Viterbi parity, the captured inference graph against eager launches, the state-dict round trip, one training step with head and
    locked dropout whose pooled rows are checked against the reference gather, one multi-view step."""
import os

import numpy as np
import pytest
import torch

import headdropref as hd
import layersref as lr
import selftest

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _run_step(layers, mean):
    """selftest.check_step's comparison for a layer selection -> (result dict, tagger)"""
    from kbner import batch as kb
    from kbner import engine
    from oracle import crf as ocrf
    from oracle import encoder as oenc
    cfg, tg, b, (start, stop, x_idx) = lr.tiny_setup_layers(layers, mean)
    bd = kb.to_device(b, DEV)
    loss = tg.forward_loss(bd, loss_scale=1.0, backward=True)
    torch.cuda.synchronize()
    ocfg = oenc.EncoderConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                              num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                              max_position_embeddings=cfg.max_position_embeddings)
    params = {k: v.clone().requires_grad_(True) for k, v in selftest.oracle_params(tg).items()}
    ob = dict(input_ids=torch.from_numpy(b["input_ids"]), attention_mask=torch.from_numpy(b["attention_mask"]),
              first_idx=torch.from_numpy(b["first_idx"]), tags=torch.from_numpy(b["tags"].astype(np.int64)),
              lengths=torch.from_numpy(b["lengths"].astype(np.int64)))
    oloss, oem = lr.tagger_forward_loss_layers(params, ocfg, ob, start, stop, x_idx, layers=layers, mean=mean)
    oloss.backward()
    oloss_f = float(oloss.detach())
    res = {"loss_hip": float(loss), "loss_oracle": oloss_f, "loss_rel": abs(float(loss) - oloss_f) / abs(oloss_f)}
    em = tg.forward_features(bd)
    torch.cuda.synchronize()
    valid = torch.from_numpy(b["first_idx"] >= 0)
    res["emissions_rel"] = selftest.rel_l2(em.cpu()[valid], oem.detach()[valid])
    gscale = max(float(v.grad.abs().max()) for v in params.values() if v.grad is not None)
    worst, worst_name, coss, unused = 0.0, "", 1.0, []
    for hf, (mine, sl) in engine.hf_name_map(cfg).items():
        gh = tg.arena.grad(mine)
        gh = (gh[sl[0]:sl[1]] if sl is not None else gh).cpu()
        go = params[hf].grad
        if go is None or float(go.abs().max()) == 0.0:
            unused.append((hf, float(gh.abs().max())))          # a parameter the loss does not depend on
            continue
        if hf.endswith("key.bias") or float(go.abs().max()) < 1e-7 * gscale:      # (selftest.check_step: only roundoff on both sides)
            continue
        e, c = selftest.rel_l2(gh, go), selftest.cosine(gh, go)
        coss = min(coss, c)
        if e > worst:
            worst, worst_name = e, hf
    res["grad_worst_rel"], res["grad_worst_name"], res["grad_min_cos"], res["unused"] = worst, worst_name, coss, unused
    for k in ("linear.weight", "linear.bias", "transitions"):
        assert float(params[k].grad.abs().max()) > 0
        res["grad_" + k] = selftest.rel_l2(tg.arena.grad(k).cpu(), params[k].grad)
    lens = torch.from_numpy(b["lengths"]).to(DEV)
    vt, vc = tg.viterbi(em, lens)
    torch.cuda.synchronize()
    rt, rc = ocrf.viterbi_batch(em.cpu().numpy(), b["lengths"], tg.arena.param("transitions").cpu().numpy(), start, stop)
    res["viterbi_equal"] = bool(np.array_equal(vt.cpu().numpy(), rt))
    return res, tg


def _assert_step(r):
    tol = selftest.STEP_TOL
    assert r["loss_rel"] < tol["loss_rel"], r
    assert r["emissions_rel"] < tol["emissions_rel"], r
    assert r["grad_min_cos"] > tol["grad_min_cos"] and r["grad_worst_rel"] < tol["grad_worst_rel"], r
    # linear.bias has no entry of its own in the table and takes linear.weight's (tests/test_gpu_widetags_e2e.py: one factor less)
    assert r["grad_linear.weight"] < tol["grad_linear.weight"] and r["grad_linear.bias"] < tol["grad_linear.weight"], r
    assert r["grad_transitions"] < tol["grad_transitions"], r
    assert r["viterbi_equal"], r


@pytest.mark.parametrize("layers,mean", [((-1, -2), False), ((-2,), False), ((0, 1, 2), False), ((-1, -2, -3), True)])
def test_step_vs_oracle_autograd(layers, mean):
    r, tg = _run_step(layers, mean)
    print("[layers] step %s%s: %s" % (layers, " mean" if mean else "", r))
    H = tg.cfg.hidden_size
    assert tg.W == (H if mean else len(layers) * H) and tuple(tg.arena.param("linear.weight").shape) == (tg.T, tg.W)
    _assert_step(r)
    if layers == (-2,):
        # the top layer feeds nothing the loss reads: all 16 of its tensors, exactly zero here (the pass still ran through it: a
        # layer left out would keep the previous step's weight gradients), None in the oracle
        top = [(n, g) for n, g in r["unused"] if n.startswith("encoder.layer.1.")]
        assert len(top) == 16 and all(g == 0.0 for _, g in top), top
        assert len(r["unused"]) == 16
    else:
        assert r["unused"] == [], r["unused"]


def test_last_layer_alone_reproduces_check_step():
    """(-1,) through this module's code path is selftest.check_step(): the forward is deterministic (equal to the bit), the gradient
    figures agree up to the order of the float32 atomics of the embedding backward"""
    r, tg = _run_step((-1,), False)
    ref = selftest.check_step()
    assert tg._last_layer_only and tg.W == tg.cfg.hidden_size
    for k in ("loss_hip", "loss_oracle", "emissions_rel", "viterbi_equal"):
        assert r[k] == ref[k], (k, r[k], ref[k])
    for k in ("grad_worst_rel", "grad_linear.weight", "grad_transitions"):
        assert abs(r[k] - ref[k]) <= 0.02 * ref[k], (k, r[k], ref[k])
    assert abs(r["grad_min_cos"] - ref["grad_min_cos"]) < 1e-5 and r["grad_worst_name"] == ref["grad_worst_name"]
    _assert_step(r)


def test_second_step_overwrites_every_weight_gradient():
    """Arena.wgrad_stale: after an optimizer step the GEMM-weight gradients are overwritten, not zeroed.  With (-2,) the top layer's
    must be overwritten with zeros: a second step after an optimizer step leaves them exactly zero again"""
    from kbner import batch as kb
    from kbner.engine import FusedAdamW
    cfg, tg, b, _ = lr.tiny_setup_layers((-2,), False, H=256, A=4, F_=256)     # (multiples of 256: the overwriting launch is taken)
    assert tg.arena.wgrad_overwrite_ok
    bd = kb.to_device(b, DEV)
    opt = FusedAdamW(tg.arena, lr=1e-3, lr_rate=50.0, t_total=10)
    tg.forward_loss(bd, backward=True)
    opt.step()                                                   # (where the weight gradients are left stale: made visibly so)
    assert tg.arena.wgrad_stale == tg.arena.wgrad_overwrite_ok
    if tg.arena.wgrad_stale:
        tg.arena.grad("l1.ffn1.weight").fill_(3.0)
    tg.forward_loss(bd, backward=True)
    torch.cuda.synchronize()
    for nm in ("qkv", "o", "ffn1", "ffn2"):
        assert float(tg.arena.grad("l1.%s.weight" % nm).abs().max()) == 0.0, nm
        assert float(tg.arena.grad("l0.%s.weight" % nm).abs().max()) > 0.0, nm


# ---------------------------------------------------------------------- the flair surface
@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("layers_e2e")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


TYPES = ("PER", "LOC", "ORG")


def _dictionary():
    from flair.data import Dictionary
    td = Dictionary(add_unk=True)
    td.add_item("O")
    for t in TYPES:
        td.add_item("S-" + t)
    for t in ("S-X", "<START>", "<STOP>"):
        td.add_item(t)
    return td


def _sentences(n_sent, seed, with_orig=False):
    """tiny KB-NER-style sentences: 4 to 8 words tagged O or S-<type>, then <EOS> + context tagged S-X; with_orig: the bare sentence
    (the other view of multi-view training) hangs on each as `orig_sent`"""
    import tiny_assets
    from flair.data import Sentence
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sent):
        n, nctx = int(rng.integers(4, 9)), int(rng.integers(3, 8))
        words = [str(w) for w in rng.choice(tiny_assets.WORDS, size=n + nctx)]
        tags = [("S-" + TYPES[int(rng.integers(0, 3))]) if rng.random() < 0.4 else "O" for _ in range(n)]
        s = Sentence(" ".join(words[:n] + ["<EOS>"] + words[n:]))
        assert len(s) == n + 1 + nctx
        for i, tok in enumerate(s):
            tok.add_tag("ner", tags[i] if i < n else "S-X")
        if with_orig:
            o = Sentence(" ".join(words[:n]))
            for i, tok in enumerate(o):
                tok.add_tag("ner", tags[i])
            s.orig_sent = o
        out.append(s)
    return out


def _tagger(tiny_dir, layers="-1,-2", mix=False, **kw):
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    emb = TransformerWordEmbeddings(model=tiny_dir, layers=layers, use_scalar_mix=mix, pooling_operation="first", fine_tune=True)
    args = dict(hidden_size=256, embeddings=StackedEmbeddings([emb]), tag_dictionary=_dictionary(), tag_type="ner", use_crf=True,
                use_rnn=False, remove_x=True, sentence_loss=True, word_dropout=0.0, dropout=0.0, locked_dropout=0.0)
    args.update(kw)
    return FastSequenceTagger(**args)


def test_fast_sequence_tagger_with_two_layers(tiny_dir):
    from flair.custom_data_loader import BatchedData, ColumnDataLoader
    from flair.models import FastSequenceTagger
    from kbner.engine import FusedAdamW
    from oracle import crf as ocrf
    torch.manual_seed(4)
    tagger = _tagger(tiny_dir)
    eng = tagger.engine
    H, L = eng.cfg.hidden_size, eng.cfg.num_hidden_layers
    assert eng.layer_sel == (L, L - 1) and eng.W == 2 * H == tagger.embeddings.embedding_length
    td = tagger.tag_dictionary
    train = _sentences(4, 1)
    # ---- two optimizer steps on the same four sentences: finite, decreasing loss
    tagger.train()
    opt = FusedAdamW(eng.arena, lr=1e-3, lr_rate=50.0, eps=1e-6, weight_decay=0.0, max_norm=5.0, t_total=10, warmup=0)
    losses = []
    for _ in range(2):
        losses.append(float(tagger.forward_backward(BatchedData(train), loss_scale=1.0)))
        opt.step()
    tagger.eval()
    losses.append(float(tagger.forward_loss(BatchedData(train))))
    torch.cuda.synchronize()
    print("[layers] losses", losses)
    assert all(np.isfinite(x) and x > 0 for x in losses) and losses[0] > losses[1] > losses[2], losses
    assert tuple(eng.last_pooled.shape)[-1] == 2 * H
    # ---- evaluate and predict; predicted tags = oracle Viterbi on the model's own emissions
    test = _sentences(6, 2)
    dl = ColumnDataLoader(test, 3, sentence_level_batch=True)
    dl.assign_tags("ner", td)
    res, eval_loss = tagger.evaluate(dl, embeddings_storage_mode="none")
    assert np.isfinite(eval_loss) and isinstance(res.main_score, float)
    batch = BatchedData(_sentences(5, 3))
    tagger.predict(batch, mini_batch_size=5)
    feats = tagger.forward(batch)
    torch.cuda.synchronize()
    lens = np.asarray([len(s) for s in batch], np.int32)
    rt, _ = ocrf.viterbi_batch(feats.cpu().numpy(), lens, eng.arena.param("transitions").cpu().numpy(), tagger.start_idx, tagger.stop_idx)
    items = td.get_items()
    for b, s in enumerate(batch):
        assert [tok.get_tag("ner").value for tok in s] == [items[int(t)] for t in rt[b, :len(s)]], b
    # ---- the captured forward-only graph (from the third pass over a shape on) against eager launches, bit for bit
    for _ in range(4):
        replayed = tagger.forward(batch).clone()
    hb = tagger._last[0]
    st = eng.acts(hb.get("R", hb["B"]), hb["S"]).infer_graph
    assert st is not None and st["graph"] not in (None, False), "the forward-only pass was not captured"
    eng.INFER_GRAPH = False
    try:
        eager = tagger.forward(batch).clone()
    finally:
        del eng.INFER_GRAPH
    torch.cuda.synchronize()
    assert torch.equal(replayed, eager) and torch.equal(replayed, feats)
    # ---- state-dict round trip: the selection and the 2H-wide head come back, and with them the emissions
    state = tagger._get_state_dict()
    assert state["embedding_layers"] == "-1,-2" and tuple(state["linear.weight"].shape) == (len(td), 2 * H)
    back = FastSequenceTagger._init_model_with_state_dict(state)
    assert back.engine.layer_sel == eng.layer_sel and back.engine.W == 2 * H
    back.eval()
    assert torch.equal(back.forward(batch), feats)


def test_training_step_with_head_and_locked_dropout(tiny_dir):
    """dropout=0.1, locked_dropout=0.5: what the head read (engine.last_pooled) is the reference gather of the two layers' rows under
    the seeds this step drew, masks keyed by the column of the 2H-wide row, within headdropref.real_bound (a concatenation)"""
    from flair.custom_data_loader import BatchedData
    from kbner import ops
    torch.manual_seed(5)
    tagger = _tagger(tiny_dir, dropout=0.1, locked_dropout=0.5)
    eng = tagger.engine
    L = eng.cfg.num_hidden_layers
    tagger.train()
    drawn = []
    draw = eng._head_drop
    eng._head_drop = lambda: drawn.append(draw()) or drawn[-1]
    loss = tagger.forward_backward(BatchedData(_sentences(3, 7)), loss_scale=1.0)
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and len(drawn) == 1 and drawn[0] is not None
    de, dl = drawn[0]
    assert de[1] == ops.drop_thresh(0.1) and dl[1] == ops.drop_thresh(0.5)
    hb = tagger._last[0]
    B, S, nc = hb["B"], hb["S"], hb["ctags"].shape[1]
    ac = eng.acts(hb.get("R", B), S)
    xs = [ac.x[i].float().cpu().numpy().astype(np.float64) for i in (L, L - 1)]
    crow = hb["crow_idx"].astype(np.int64)
    ref = lr.gather_layers(xs, crow, nc, False, de, dl)
    got = eng.last_pooled.float().cpu().numpy().astype(np.float64).reshape(B * nc, -1)
    assert got.shape == ref.shape
    ke, kl = hd.keep(B * nc, ref.shape[1], nc, de, dl)
    dead = ~(ke & kl & (crow >= 0)[:, None])
    assert dead.any() and (got[dead] == 0).all() and (got[~dead] != 0).mean() > 0.99
    bound = hd.real_bound(ref)
    diff = np.abs(got - ref)
    print("[layers] last_pooled: worst share of the bound %.3f" % float((diff[bound > 0] / bound[bound > 0]).max()))
    assert (diff <= bound).all()
    assert float(eng.arena.grad("linear.weight").abs().max()) > 0 and bool(torch.isfinite(eng.arena.g).all())


def test_multi_view_step(tiny_dir):
    """multi_view_training + distill_posterior + calculate_l2_loss with remove_x: the context view's NLL step, then the bare
    sentences' distillation step with the l2 term on the 2H-wide rows; finite loss, a head gradient"""
    from flair.custom_data_loader import BatchedData
    torch.manual_seed(6)
    tagger = _tagger(tiny_dir, multi_view_training=True, distill_posterior=True, calculate_l2_loss=True, temperature=2.0)
    eng = tagger.engine
    tagger.train()
    sents = _sentences(3, 11, with_orig=True)
    B = len(sents)
    loss = tagger.forward_backward(BatchedData(sents), loss_scale=1.0, multi_view=(list(range(B)), [1.0 / B] * B))
    torch.cuda.synchronize()
    nll, kd = tagger.last_loss_parts
    assert np.isfinite(float(loss)) and np.isfinite(float(nll)) and kd is not None and np.isfinite(float(kd)) and float(kd) >= 0
    assert tuple(eng.last_pooled.shape)[-1] == 2 * eng.cfg.hidden_size
    g = eng.arena.grad("linear.weight")
    assert bool(torch.isfinite(eng.arena.g).all()) and float(g.abs().max()) > 0
    assert float(g[:, :eng.cfg.hidden_size].abs().max()) > 0 and float(g[:, eng.cfg.hidden_size:].abs().max()) > 0


@pytest.mark.parametrize("layers,mix", [("-1,-2", False), ("-1,-2,-3", True)])
def test_yaml_keys_train_save_and_reload(tmp_path, layers, mix):
    """`layers` / `use_scalar_mix` in the YAML, through the config parser and ModelFinetuner as train.py drives them: one epoch trains
    with a finite loss, best-model.pt carries the selection, the reloaded model computes the saved model's emissions"""
    import yaml
    import tiny_assets
    from flair.config_parser import ConfigParser
    from flair.custom_data_loader import BatchedData
    from flair.models import FastSequenceTagger
    from flair.trainers import ModelFinetuner
    from flair.utils.from_params import Params
    torch.manual_seed(8)
    cfg = tiny_assets.e2e_config(str(tmp_path), word_dropout=0.05, max_epochs=1, n_train=8, n_dev=4, n_test=4)
    cfg["embeddings"]["TransformerWordEmbeddings-0"].update(layers=layers, use_scalar_mix=mix)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    cp = ConfigParser(Params.from_file(str(tmp_path / "cfg.yaml")))
    student = cp.create_student()
    k = len(layers.split(","))
    H = student.engine.cfg.hidden_size
    assert student.engine.layer_mean is mix and len(student.engine.layer_sel) == k and student.engine.W == (H if mix else k * H)
    trainer = ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    out = trainer.train(cp.get_target_path, **cp.config["train"])
    hist = out["train_loss_history"]
    assert len(hist) == 1 and np.isfinite(hist[0]) and hist[0] > 0, hist
    again = FastSequenceTagger.load(cp.get_target_path / "best-model.pt")
    assert again.engine.layer_sel == student.engine.layer_sel and again.engine.layer_mean is mix
    emb = again.embeddings.embeddings[0]
    assert emb.layers == layers and emb.use_scalar_mix is mix and emb.embedding_length == student.engine.W
    best = FastSequenceTagger.load(cp.get_target_path / "best-model.pt")
    batch = BatchedData(_sentences(3, 5))
    again.eval(), best.eval()
    assert torch.equal(again.forward(batch), best.forward(batch))
    again.predict(batch, mini_batch_size=3)
    assert all(tok.get_tag("ner").value for s in batch for tok in s)
