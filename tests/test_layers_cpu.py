"""CPU: the encoder layer selection (TransformerWordEmbeddings(layers=..., use_scalar_mix=...)) without a GPU.
  - tests/layersref.py's references against torch autograd in float64, and its bounds against a plain float32 evaluation of the
    GPU case list (tests/test_gpu_layers_kernels.py imports the same list);
  - the constructors: widths, the state-dict round trip, every refusal with its named message;
  - dispatch: the default selection calls only the ops it called before the selection existed; another one calls the new ops."""
import os
import types

import numpy as np
import pytest
import torch

import headdropref as hd
import layersref as lr

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32

from layersref import DROPS, GATHER_CASES, SCATTER_CASES, WIDTHS, gather_inputs, scatter_inputs, sites


def test_case_list_covers_the_grid():
    assert len(GATHER_CASES) <= 64
    for ax, vals in ((0, {1, 6, 70}), (2, set(WIDTHS)), (3, {1, 2, 3, 4}), (4, {False, True}), (5, set(DROPS))):
        assert {c[ax] for c in GATHER_CASES} == vals
    assert any(c[2] == 520 and c[3] == 3 and c[5] == "both" and c[4] for c in GATHER_CASES)
    assert any(c[2] == 520 and c[3] == 3 and c[5] == "both" and not c[4] for c in GATHER_CASES)
    assert any(c[0] == 1 for c in GATHER_CASES)


# ---------------------------------------------------------------------- references against autograd
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("drop", ["none", "both"])
def test_gather_reference_is_concat_or_mean_times_mask(mean, drop):
    R, n, H, k = 6, 3, 16, 4          # (1 / k is a float32 number: the reference takes `scale` as the float32 the kernel is handed)
    xs, idx = gather_inputs(R, n, H, k)
    de, dl = sites(drop, 5)
    W = H if mean else k * H
    M = torch.from_numpy(hd.mult(R, W, n, de, dl).astype(np.float64))
    xt = [torch.from_numpy(x).requires_grad_(True) for x in xs]
    safe = torch.from_numpy(np.maximum(idx, 0))
    rows = [x[safe] for x in xt]
    feat = torch.stack(rows, 0).mean(0) if mean else torch.cat(rows, 1)
    y = feat * M * torch.from_numpy((idx >= 0).astype(np.float64))[:, None]
    ref = lr.gather_layers(xs, idx, n, mean, de, dl)
    np.testing.assert_allclose(ref, y.detach().numpy(), rtol=1e-14, atol=0)
    # scatter_add_ld is the vector-Jacobian product: every source's gradient = its block (mean: the whole row / k) scattered back
    g = np.random.default_rng(3).standard_normal((R, W))
    y.backward(torch.from_numpy(g))
    for j in range(k):
        got, _ = lr.scatter_add_ld(np.zeros_like(xs[j]), g, W, 0 if mean else j * H, idx, 1.0 / k if mean else 1.0, n, de, dl)
        np.testing.assert_allclose(got, xt[j].grad.numpy(), rtol=1e-12, atol=1e-15)
    # adding to a pre-filled matrix: rows idx does not name keep their values
    start = np.random.default_rng(4).standard_normal(xs[0].shape)
    got, mag = lr.scatter_add_ld(start, g, W, 0, idx, 1.0, n, de, dl)
    untouched = np.setdiff1d(np.arange(start.shape[0]), idx[idx >= 0])
    assert np.array_equal(got[untouched], start[untouched]) and (mag >= np.abs(start)).all()


# ---------------------------------------------------------------------- the bounds hold for a float32 evaluation of the GPU cases
@pytest.mark.parametrize("R,n,H,k,mean,drop", [c for c in GATHER_CASES if c[4]])
def test_mean_bound_covers_a_float32_evaluation(R, n, H, k, mean, drop):
    xs, idx = gather_inputs(R, n, H, k)
    de, dl = sites(drop, R + H)
    ref = lr.gather_layers(xs, idx, n, True, de, dl)
    mag = lr.gather_abs(xs, idx, n, True, de, dl)
    bound = lr.gather_mean_bound(ref, mag, k)
    got = lr.round_bf16(lr.gather_mean_f32(xs, idx, n, de, dl))
    assert (np.abs(got - ref) <= bound).all()
    assert (bound[mag == 0] == 0).all() and (got[mag == 0] == 0).all()       # dropped elements and -1 rows: exactly 0


@pytest.mark.parametrize("R,n,H,c,scale,drop", SCATTER_CASES)
def test_scatter_add_bound_covers_a_float32_evaluation(R, n, H, c, scale, drop):
    dst, d, idx = scatter_inputs(R, n, H)
    de, dl = sites(drop, R + H)
    ref, mag = lr.scatter_add_ld(dst, d, 4 * H, c * H, idx, scale, n, de, dl)
    got = lr.round_bf16(lr.scatter_add_f32(dst, d, 4 * H, c * H, idx, scale, n, de, dl))
    named = idx[idx >= 0]
    assert (np.abs(got - ref)[named] <= lr.scatter_add_bound(ref, mag)[named]).all()
    untouched = np.setdiff1d(np.arange(dst.shape[0]), named)
    assert np.array_equal(got[untouched], dst[untouched])


# ---------------------------------------------------------------------- the flair surface
@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("layers_cpu")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def _dictionary():
    from flair.data import Dictionary
    td = Dictionary(add_unk=True)
    for t in ("O", "S-PER", "S-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(t)
    return td


def _cpu_tagger(monkeypatch, tiny_dir, layers="-1", use_scalar_mix=False, pooling_operation="first", **kw):
    import flair
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    from kbner import ops
    monkeypatch.setattr(flair, "device", torch.device("cpu"))
    monkeypatch.setattr(ops, "f32_to_bf16", lambda x, y: y.copy_(x.to(BF16)))
    monkeypatch.setattr(ops, "bf16_to_f32", lambda x, y: y.copy_(x.float()))
    emb = TransformerWordEmbeddings(model=tiny_dir, layers=layers, use_scalar_mix=use_scalar_mix, pooling_operation=pooling_operation,
                                    fine_tune=True)
    args = dict(hidden_size=256, embeddings=StackedEmbeddings([emb]), tag_dictionary=_dictionary(), tag_type="ner", use_crf=True,
                use_rnn=False, remove_x=True, sentence_loss=True, dropout=0.0, locked_dropout=0.0)
    args.update(kw)
    return FastSequenceTagger(**args)


def test_constructor_takes_a_layer_selection(monkeypatch, tiny_dir, caplog):
    import logging
    from flair.embeddings import TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    H, L = 128, 2                                               # tests/tiny_assets.py build_model_dir
    flog = logging.getLogger("flair")                           # (the package's logger does not propagate to the root)
    flog.addHandler(caplog.handler)
    try:
        with caplog.at_level(logging.INFO, logger="flair"):
            tg = _cpu_tagger(monkeypatch, tiny_dir, layers="-1,-2")
    finally:
        flog.removeHandler(caplog.handler)
    assert any("-1,-2" in r.getMessage() and str(2 * H) in r.getMessage() for r in caplog.records)
    T = tg.tagset_size
    emb = tg.embeddings.embeddings[0]
    assert emb.layer_indexes == [-1, -2] and emb.use_scalar_mix is False and emb.embedding_length == 2 * H
    assert tg.embeddings.embedding_length == 2 * H
    assert tg.engine.layer_sel == (L, L - 1) and tg.engine.layer_mean is False and tg.engine.W == 2 * H
    w = tg.engine.arena.param("linear.weight")
    assert tuple(w.shape) == (T, 2 * H)
    assert float(w.abs().max()) <= 1.0 / (2 * H) ** 0.5 and float(w.abs().max()) > 0.9 / (2 * H) ** 0.5     # nn.Linear's rule on in_features
    # 'all' with the mean: every hidden state, width H, no parameter
    mix = _cpu_tagger(monkeypatch, tiny_dir, layers="all", use_scalar_mix=True)
    e2 = mix.embeddings.embeddings[0]
    assert e2.layer_indexes == [0, 1, 2] and e2.use_scalar_mix is True and e2.embedding_length == H
    assert mix.engine.layer_sel == (0, 1, 2) and mix.engine.layer_mean is True
    assert tuple(mix.engine.arena.param("linear.weight").shape) == (T, H)
    # order and duplicates are kept
    dup = TransformerWordEmbeddings(model=tiny_dir, layers="0,-1,0", fine_tune=True)
    assert dup.layer_indexes == [0, -1, 0] and dup.embedding_length == 3 * H
    # the signature default stays the last layer alone
    dflt = TransformerWordEmbeddings(model=tiny_dir, fine_tune=True)
    assert dflt.layer_indexes == [-1] and dflt.embedding_length == H
    # state dict round trip keeps the selection; a state from before the keys existed loads as '-1'
    state = tg._get_state_dict()
    assert state["embedding_layers"] == "-1,-2" and state["embedding_scalar_mix"] is False
    back = FastSequenceTagger._init_model_with_state_dict(state)
    assert back.embeddings.embeddings[0].layer_indexes == [-1, -2] and back.engine.layer_sel == (L, L - 1)
    assert torch.equal(back.engine.arena.param("linear.weight"), w)
    ms = mix._get_state_dict()
    assert ms["embedding_layers"] == "0,1,2" and ms["embedding_scalar_mix"] is True
    mback = FastSequenceTagger._init_model_with_state_dict(ms)
    assert mback.engine.layer_sel == (0, 1, 2) and mback.engine.layer_mean is True
    plain = _cpu_tagger(monkeypatch, tiny_dir)
    old = {k: v for k, v in plain._get_state_dict().items() if k not in ("embedding_layers", "embedding_scalar_mix")}
    oback = FastSequenceTagger._init_model_with_state_dict(old)
    assert oback.embeddings.embeddings[0].layer_indexes == [-1] and oback.engine.layer_sel == (L,) and oback.engine.W == H


def test_constructor_refusals_are_named(monkeypatch, tiny_dir):
    from flair.embeddings import TransformerWordEmbeddings
    for bad in ("3", "-4", "-1,7"):
        with pytest.raises(ValueError, match=r"outside the 3 hidden states"):
            TransformerWordEmbeddings(model=tiny_dir, layers=bad, fine_tune=True)
    with pytest.raises(ValueError, match="comma-separated"):
        TransformerWordEmbeddings(model=tiny_dir, layers="last", fine_tune=True)
    with pytest.raises(ValueError, match="1 to 32 hidden states"):
        TransformerWordEmbeddings(model=tiny_dir, layers=",".join(["-1"] * 33), fine_tune=True)
    wide = ",".join(["-1", "-2"] * 16)                          # 32 layers: inside the count limit
    assert TransformerWordEmbeddings(model=tiny_dir, layers=wide, fine_tune=True).embedding_length == 32 * 128
    with pytest.raises(NotImplementedError, match="pooling_operation='mean'"):
        TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation="mean", fine_tune=True)
    for kw in (dict(document_extraction=True), dict(ext_doc=True), dict(sentence_feat=True)):
        with pytest.raises(NotImplementedError, match="document_extraction / ext_doc / sentence_feat"):
            TransformerWordEmbeddings(model=tiny_dir, fine_tune=True, **kw)
    with pytest.raises(NotImplementedError, match=r"use_rnn: true.*layers='-1,-2'"):
        _cpu_tagger(monkeypatch, tiny_dir, layers="-1,-2", use_rnn=True, locked_dropout=0.0)


def test_width_limit_is_refused_by_name(monkeypatch, tiny_dir):
    """a concatenation wider than 8192 columns: NotImplementedError naming the width, the limit and use_scalar_mix ('all' on
    XLM-R-large is 25 600 wide).  On the tiny model (H = 128) the limit is reached through the engine's constant."""
    import flair.embeddings as FE
    from flair.embeddings import TransformerWordEmbeddings
    monkeypatch.setattr(FE, "MAX_EMBEDDING_WIDTH", 256)
    with pytest.raises(NotImplementedError) as ei:
        TransformerWordEmbeddings(model=tiny_dir, layers="all", fine_tune=True)
    msg = str(ei.value)
    assert "384" in msg and "256" in msg and "use_scalar_mix" in msg
    assert TransformerWordEmbeddings(model=tiny_dir, layers="all", use_scalar_mix=True, fine_tune=True).embedding_length == 128
    from kbner import engine as E
    assert E.HEAD_MAX_WIDTH == 8192
    cfg = E.EncoderConfig(vocab_size=64, hidden_size=1024, num_hidden_layers=24, num_attention_heads=16, intermediate_size=4096)
    with pytest.raises(ValueError, match="25600"):
        E.Tagger(cfg, 5, 3, 4, device="cpu", layers=tuple(range(25)))          # (raised before anything is allocated)
    with pytest.raises(ValueError, match="outside the 25 hidden states"):
        E.normalize_layers((25,), 24)
    assert E.normalize_layers((-1, -25, 0, 24), 24) == (24, 0, 0, 24)


# ---------------------------------------------------------------------- dispatch
class _Spy:
    """torch stand-ins for the row / head ops on the engine's module, recording every call"""
    NAMES = ("gather_rows", "gather_rows_drop", "scatter_rows", "scatter_rows_drop", "gather_rows_layers", "scatter_add_rows_ld",
             "head_fwd", "head_bwd")

    def __init__(self, monkeypatch, eng_mod):
        self.calls = []
        for name in self.NAMES:
            monkeypatch.setattr(eng_mod.ops, name, getattr(self, name))

    @staticmethod
    def _take(src, idx):
        out = src[idx.long().clamp(min=0)].clone()
        out[idx < 0] = 0
        return out

    def gather_rows(self, src, idx, out=None):
        self.calls.append(("gather_rows",))
        return self._take(src, idx)

    def gather_rows_drop(self, src, idx, n, drop_e=(0, 0), drop_l=(0, 0), out=None):
        self.calls.append(("gather_rows_drop", n, tuple(drop_e), tuple(drop_l)))
        return self._take(src, idx)

    def scatter_rows(self, dout, idx, dsrc):
        self.calls.append(("scatter_rows",))

    def scatter_rows_drop(self, dout, idx, dsrc, n, drop_e=(0, 0), drop_l=(0, 0)):
        self.calls.append(("scatter_rows_drop", n, tuple(drop_e), tuple(drop_l)))

    def gather_rows_layers(self, srcs, idx, n, mean=False, drop_e=(0, 0), drop_l=(0, 0), out=None):
        self.calls.append(("gather_rows_layers", [int(s[0, 0]) for s in srcs], n, bool(mean), tuple(drop_e), tuple(drop_l)))
        rows = [self._take(s, idx).float() for s in srcs]
        return (torch.stack(rows, 0).mean(0) if mean else torch.cat(rows, 1)).to(BF16)

    def scatter_add_rows_ld(self, dout, col0, idx, dst, n, scale=1.0, drop_e=(0, 0), drop_l=(0, 0)):
        self.calls.append(("scatter_add_rows_ld", col0, n, float(scale), tuple(drop_e), tuple(drop_l), tuple(dout.shape)))

    def head_fwd(self, x, w, bias):
        return x.float() @ w.t() + bias

    def head_bwd(self, de, x, w, dw, db):
        return (de @ w).to(BF16)

    def names(self):
        return [c[0] for c in self.calls]


B_, NC_, S_, NPOS_ = 2, 3, 8, 5


def _stub_engine(monkeypatch, tiny_dir, layers, mix=False, **rates):
    import kbner.engine as E
    tg = _cpu_tagger(monkeypatch, tiny_dir, layers=layers, use_scalar_mix=mix, dropout=rates.get("dropout", 0.0),
                     locked_dropout=rates.get("locked_dropout", 0.0), word_dropout=rates.get("word_dropout", 0.0))
    eng = tg.engine
    H, L = eng.cfg.hidden_size, eng.cfg.num_hidden_layers
    xs = [torch.full((B_ * S_, H), float(i), dtype=BF16) for i in range(L + 1)]      # x[i] is filled with i: the spy reads the order
    ac = types.SimpleNamespace(dx=torch.zeros(B_ * S_, H, dtype=BF16), x=xs)
    seen = {}
    monkeypatch.setattr(eng, "encoder_forward", lambda ids, pos_ids, maskbias, R, S, **kw: xs[L])
    monkeypatch.setattr(eng, "acts", lambda R, S: ac)
    monkeypatch.setattr(eng, "encoder_backward", lambda dx, grad_ready=None, **kw: seen.update(kw))
    spy = _Spy(monkeypatch, E)
    crow = torch.tensor([1, 2, 3, 9, 10, -1], dtype=I32)
    batch = {"B": B_, "S": S_, "ids": None, "pos_ids": None, "maskbias": None, "ctags": torch.zeros(B_, NC_, dtype=I32),
             "crow_idx": crow, "cpos": torch.tensor([0, 1, 2, 0, 1, -1], dtype=I32), "n_tokens": NPOS_,
             "row_idx": torch.arange(B_ * NPOS_, dtype=I32)}
    return eng, spy, batch, seen


def _step(eng, batch):
    em, pooled, crow_idx, B, nc, R, S, drop = eng._emit(batch)
    eng._backprop_emissions(torch.ones(B, nc, eng.T), pooled, crow_idx, B, nc, R, S, None, drop=drop)
    return pooled, drop


def test_default_selection_calls_only_the_ops_it_called_before(monkeypatch, tiny_dir):
    eng, spy, batch, seen = _stub_engine(monkeypatch, tiny_dir, "-1", word_dropout=0.1)
    eng.train()
    eng.seed_dropout(77)
    _step(eng, batch)
    assert spy.names() == ["gather_rows", "scatter_rows"] and seen == {}          # (no inject keyword either)
    expect = np.random.default_rng(77)
    expect.random(NPOS_)
    assert eng._drop_rng.bit_generator.state == expect.bit_generator.state         # no extra draw from the engine's stream
    eng.head_dropout, eng.locked_dropout = 0.1, 0.5
    spy.calls.clear()
    _step(eng, batch)
    assert spy.names() == ["gather_rows_drop", "scatter_rows_drop"] and seen == {}
    eng.eval()
    spy.calls.clear()
    eng.forward_features(batch)
    assert spy.names() == ["gather_rows"]


def test_a_selection_calls_the_layer_ops(monkeypatch, tiny_dir):
    from kbner import ops
    eng, spy, batch, seen = _stub_engine(monkeypatch, tiny_dir, "-1,-2", dropout=0.1, locked_dropout=0.5)
    H = eng.cfg.hidden_size
    eng.train()
    eng.seed_dropout(5)
    pooled, drop = _step(eng, batch)
    assert tuple(pooled.shape) == (B_ * NC_, 2 * H) and tuple(eng.arena.param("linear.weight").shape) == (eng.T, 2 * H)
    assert spy.names() == ["gather_rows_layers", "scatter_add_rows_ld"]
    g, s = spy.calls
    assert g[1] == [2, 1] and g[2] == NC_ and g[3] is False and g[4] == drop[0] and g[5] == drop[1]
    assert drop[0][1] == ops.drop_thresh(0.1) and drop[1][1] == ops.drop_thresh(0.5)
    assert s[1:] == (0, NC_, 1.0, drop[0], drop[1], (B_ * NC_, 2 * H))              # the last layer's block goes in at once ...
    inj = seen["inject"]
    assert sorted(inj) == [1] and len(inj[1]) == 1                                  # ... layer 1's inside the encoder backward
    dout, col0, idx, n_, scale, de_, dl_ = inj[1][0]
    assert (col0, n_, scale, de_, dl_) == (H, NC_, 1.0, drop[0], drop[1]) and tuple(dout.shape) == (B_ * NC_, 2 * H)
    # without the last layer: nothing is scattered before the pass, which still starts at the top
    eng2, spy2, batch2, seen2 = _stub_engine(monkeypatch, tiny_dir, "0,1,2", mix=True)
    pooled2, drop2 = _step(eng2, batch2)
    assert drop2 is None and tuple(pooled2.shape) == (B_ * NC_, H)
    assert spy2.calls[0][:4] == ("gather_rows_layers", [0, 1, 2], NC_, True)
    assert spy2.names() == ["gather_rows_layers", "scatter_add_rows_ld"] and spy2.calls[1][1:4] == (0, NC_, 1.0 / 3)
    assert sorted(seen2["inject"]) == [0, 1] and all(v[0][1] == 0 and v[0][4] == 1.0 / 3 for v in seen2["inject"].values())
    eng3, spy3, batch3, seen3 = _stub_engine(monkeypatch, tiny_dir, "-2")
    _step(eng3, batch3)
    assert spy3.names() == ["gather_rows_layers"] and sorted(seen3["inject"]) == [1]
