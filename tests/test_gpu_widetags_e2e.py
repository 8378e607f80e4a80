"""GPU: tag sets wider than 64 tags end to end on the tiny model (L2, H128, S64, V512).

  - one forward + backward of kbner.engine.Tagger at T = 137 (a 33-type BIOES dictionary) and T = 77 (18 types) against the oracle's
    autograd (oracle.train_step.tagger_forward_loss), following selftest.check_step: loss, emissions, the gradients of
    linear.weight, linear.bias and transitions, and Viterbi on the HIP emissions == oracle.crf.viterbi_batch on the same emissions.
    The bounds are selftest.STEP_TOL's; linear.bias has no entry of its own there and takes linear.weight's: its gradient is the
    column sum of the same d loss / d emissions whose product with the bf16 token features is the weight gradient, so it carries
    the error of one factor less.
  - a FastSequenceTagger over a 137-item dictionary on the tiny assets: two optimizer steps with finite, decreasing loss; evaluate
    and predict run; the predicted tags equal oracle Viterbi on the model's own emissions; predict_posterior's marginals sum to 1
    (within the float32 rounding of their exponents and of a sum of 137 terms, bound stated at the assertion); state dict round trip.
"""
import os

import numpy as np
import pytest
import torch

import selftest

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.mark.parametrize("T", [137, 77])
def test_step_vs_oracle_autograd(T):
    from kbner import batch as kb
    from oracle import crf as ocrf
    from oracle import encoder as oenc
    from oracle import train_step as ots
    cfg, tg, b, (start, stop, x_idx) = selftest.tiny_setup(T=T)
    assert tg.T == T and start < T and stop < T
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
    oloss, oem = ots.tagger_forward_loss(params, ocfg, ob, start, stop, x_idx)
    oloss.backward()
    r = {"loss_rel": abs(float(loss) - float(oloss.detach())) / abs(float(oloss.detach()))}
    em = tg.forward_features(bd)
    torch.cuda.synchronize()
    valid = torch.from_numpy(b["first_idx"] >= 0)
    r["emissions_rel"] = selftest.rel_l2(em.cpu()[valid], oem.detach()[valid])
    for k in ("linear.weight", "linear.bias", "transitions"):
        assert float(params[k].grad.abs().max()) > 0
        r["grad_" + k] = selftest.rel_l2(tg.arena.grad(k).cpu(), params[k].grad)
    print("[widetags] T=%d: %s" % (T, r))
    tol = selftest.STEP_TOL
    assert r["loss_rel"] < tol["loss_rel"], r
    assert r["emissions_rel"] < tol["emissions_rel"], r
    assert r["grad_linear.weight"] < tol["grad_linear.weight"] and r["grad_linear.bias"] < tol["grad_linear.weight"], r
    assert r["grad_transitions"] < tol["grad_transitions"], r
    lens = torch.from_numpy(b["lengths"]).to(DEV)
    vt, vc = tg.viterbi(em, lens)
    torch.cuda.synchronize()
    rt, rc = ocrf.viterbi_batch(em.cpu().numpy(), b["lengths"], tg.arena.param("transitions").cpu().numpy(), start, stop)
    assert np.array_equal(vt.cpu().numpy(), rt)


# ---------------------------------------------------------------------- the flair surface
N_TYPES = 33


def _dictionary():
    from flair.data import Dictionary
    td = Dictionary(add_unk=True)
    td.add_item("O")
    for k in range(N_TYPES):
        for p in "BIES":
            td.add_item("%s-T%02d" % (p, k))
    for t in ("S-X", "<START>", "<STOP>"):
        td.add_item(t)
    assert len(td) == 137
    return td


def _sentences(n_sent, seed):
    """tiny KB-NER-style sentences: 4 to 8 words tagged O or S-T<k> (k over all 33 types), then <EOS> + context tagged S-X"""
    import tiny_assets
    from flair.data import Sentence
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_sent):
        n, nctx = int(rng.integers(4, 9)), int(rng.integers(3, 8))
        words = [str(w) for w in rng.choice(tiny_assets.WORDS, size=n + nctx)]
        s = Sentence(" ".join(words[:n] + ["<EOS>"] + words[n:]))
        assert len(s) == n + 1 + nctx
        for i, tok in enumerate(s):
            if i >= n:
                tok.add_tag("ner", "S-X")
            else:
                tok.add_tag("ner", "S-T%02d" % int(rng.integers(0, N_TYPES)) if rng.random() < 0.4 else "O")
        out.append(s)
    return out


@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("widetags")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def test_fast_sequence_tagger_over_137_tags(tiny_dir):
    from flair.custom_data_loader import BatchedData, ColumnDataLoader
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    from kbner.engine import FusedAdamW
    from oracle import crf as ocrf
    torch.manual_seed(4)
    td = _dictionary()
    emb = TransformerWordEmbeddings(model=tiny_dir, layers="-1", pooling_operation="first", fine_tune=True)
    tagger = FastSequenceTagger(hidden_size=256, embeddings=StackedEmbeddings([emb]), tag_dictionary=td, tag_type="ner", use_crf=True,
                                use_rnn=False, remove_x=True, sentence_loss=True, word_dropout=0.0, dropout=0.0, locked_dropout=0.0)
    assert tagger.tagset_size == 137 and tagger.engine.T == 137
    train = _sentences(4, 1)
    # ---- two optimizer steps on the same four sentences: finite, decreasing loss
    tagger.train()
    opt = FusedAdamW(tagger.engine.arena, lr=1e-3, lr_rate=50.0, eps=1e-6, weight_decay=0.0, max_norm=5.0, t_total=10, warmup=0)
    losses = []
    for _ in range(2):
        losses.append(float(tagger.forward_backward(BatchedData(train), loss_scale=1.0)))
        opt.step()
    tagger.eval()
    losses.append(float(tagger.forward_loss(BatchedData(train))))
    torch.cuda.synchronize()
    print("[widetags] losses", losses)
    assert all(np.isfinite(x) and x > 0 for x in losses) and losses[0] > losses[1] > losses[2], losses
    # ---- evaluate and predict
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
    rt, _ = ocrf.viterbi_batch(feats.cpu().numpy(), lens, tagger.engine.arena.param("transitions").cpu().numpy(), tagger.start_idx,
                               tagger.stop_idx)
    items = td.get_items()
    for b, s in enumerate(batch):
        got = [tok.get_tag("ner").value for tok in s]
        assert got == [items[int(t)] for t in rt[b, :len(s)]], b
    # ---- posterior decoding: a distribution over the 137 tags at every token
    from kbner import ops
    marg = ops.crf_posterior(feats.contiguous(), tagger.engine.arena.param("transitions"), torch.from_numpy(lens).to(feats.device),
                             tagger.start_idx, tagger.stop_idx).cpu().numpy().astype(np.float64)
    below = np.arange(marg.shape[1])[None, :] < lens[:, None]
    # a marginal is exp(alpha + beta - logz): three scores of at most (n + 1) steps of |emission| + |transition| + log T each, so
    # its exponent carries 2^-24 of 3 (n + 1) m; 137 of them are added.  Times rowref.tolerance's factor 8.
    tr = tagger.engine.arena.param("transitions").cpu().numpy().astype(np.float64)
    m = float(np.abs(feats.cpu().numpy()).max()) + float(np.abs(tr[np.abs(tr) < 1e3]).max()) + np.log(137.0)
    bound = 8 * 2.0 ** -24 * (3 * (marg.shape[1] + 1) * m + 137)
    worst = float(np.abs(marg.sum(2)[below] - 1.0).max())
    print("[widetags] posterior row sums - 1: worst %.2e, bound %.2e" % (worst, bound))
    assert (marg >= 0).all() and worst <= bound
    assert (marg[~below] == 0).all()
    tagger.predict_posterior = True
    try:
        labels, _ = tagger._obtain_labels(feats, batch)
    finally:
        tagger.predict_posterior = False
    assert [len(x) for x in labels] == [len(s) for s in batch] and all(0.0 < lab.score <= 1.0 for row in labels for lab in row)
    # ---- state dict round trip: same parameters, same predictions
    again = FastSequenceTagger._init_model_with_state_dict(tagger._get_state_dict())
    assert again.tagset_size == 137
    for k in ("linear.weight", "linear.bias", "transitions"):
        assert torch.equal(again.engine.arena.param(k), tagger.engine.arena.param(k)), k
    again.eval()
    assert torch.equal(again.forward(batch), feats)
