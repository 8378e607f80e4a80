"""CPU: the head-dropout reference (tests/headdropref.py) against torch.autograd, the structure and keep rates of its masks, and the
host side of the feature -- FastSequenceTagger(dropout=..., locked_dropout=..., use_rnn=False) constructs, keeps both rates through
a state dict, and the engine hands every backward the (seed, thresh) pairs of ITS forward.

The engine is built on the CPU device with the tiny model of tests/tiny_assets.py; the one device call of the constructor (the bf16
shadow of the weights) and the row / head ops the checks watch are replaced by torch stand-ins, the encoder by a stub: what is
tested is the plumbing in kbner/engine.py, not a kernel (tests/test_gpu_headdrop_kernels.py, tests/test_gpu_headdrop_e2e.py)."""
import os
import types

import numpy as np
import pytest
import torch

import headdropref as hd
import mmaref

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _idx(rng, R, rows_src):
    idx = rng.permutation(rows_src)[:R].astype(np.int64)
    idx[rng.random(R) < 0.25] = -1
    return idx


# ---------------------------------------------------------------------- the reference
@pytest.mark.parametrize("p_e,p_l", [(0.1, 0.0), (0.0, 0.3), (0.1, 0.3), (0.5, 0.75), (0.0, 0.0)])
def test_reference_equals_autograd(p_e, p_l):
    """gather is y = x[idx] * M with idx = -1 rows zero; scatter of a cotangent is x.grad (float64, exact up to the product's rounding)"""
    rng = np.random.default_rng(11)
    R, n, H, rows_src = 12, 4, 24, 20
    de, dl = (123457, mmaref.dropout_thresh(p_e)), (7654321, mmaref.dropout_thresh(p_l))
    idx = _idx(rng, R, rows_src)
    x = torch.from_numpy(rng.standard_normal((rows_src, H))).requires_grad_(True)
    M = torch.from_numpy(hd.mult(R, H, n, de, dl).astype(np.float64))
    ok = torch.from_numpy(idx >= 0)
    y = torch.where(ok[:, None], x[torch.from_numpy(np.maximum(idx, 0))] * M, torch.zeros((), dtype=torch.float64))
    d = torch.from_numpy(rng.standard_normal((R, H)))
    y.backward(d)
    np.testing.assert_array_equal(hd.gather(x.detach().numpy(), idx, n, de, dl), y.detach().numpy())
    np.testing.assert_array_equal(hd.scatter(d.numpy(), idx, rows_src, n, de, dl), x.grad.numpy())
    if p_e == 0.0 and p_l == 0.0:
        assert (M == 1.0).all()


def test_locked_mask_is_per_sentence():
    """B = 8, n = 5, H = 64, p = 0.5, seed 424242: the locked factor is one value per (sentence, column) -- constant over the 5 rows
    of a sentence -- and the 8 sentences do not share one mask (all 8 rows of the per-sentence table differ for this seed)"""
    B, n, H = 8, 5, 64
    M = hd.mult(B * n, H, n, hd.NO_DROP, (424242, mmaref.dropout_thresh(0.5))).reshape(B, n, H)
    assert set(np.unique(M).tolist()) == {0.0, 2.0}
    assert (M == M[:, :1, :]).all()
    per_sentence = M[:, 0, :]
    assert len({row.tobytes() for row in per_sentence}) == B
    # and the element site of the same seed is NOT constant over a sentence's rows
    E = hd.mult(B * n, H, n, (424242, mmaref.dropout_thresh(0.5)), hd.NO_DROP).reshape(B, n, H)
    assert not (E == E[:, :1, :]).all()


def test_keep_rates():
    """R = 64, n = 4, H = 512, (p_e, p_l) = (0.1, 0.5), seeds (20220711, 20220712): both keep rates within 5 binomial standard
    deviations sqrt(p (1 - p) / N) of 1 - p, N = R * H = 32768 and (R / n) * H = 8192.  The masks are a fixed function of the seed;
    for these seeds the reference gives 0.90067 (0.40 sigma from 0.9) and 0.49927 (0.13 sigma from 0.5)."""
    R, n, H = 64, 4, 512
    p_e, p_l = 0.1, 0.5
    ke, kl = hd.keep(R, H, n, (20220711, mmaref.dropout_thresh(p_e)), (20220712, mmaref.dropout_thresh(p_l)))
    rate_e = ke.mean()
    rate_l = kl[::n].mean()
    assert (kl.reshape(R // n, n, H) == kl[::n][:, None, :]).all()
    for rate, p, N in ((rate_e, p_e, R * H), (rate_l, p_l, (R // n) * H)):
        sd = np.sqrt(p * (1 - p) / N)
        print("[headdrop] keep rate %.5f, expected %.2f, %.2f sigma" % (rate, 1 - p, abs(rate - (1 - p)) / sd))
        assert abs(rate - (1 - p)) <= 5 * sd
    # the survivors' scale: 1 / (1 - p) in float32
    M = hd.mult(R, H, n, (20220711, mmaref.dropout_thresh(p_e)), (20220712, mmaref.dropout_thresh(p_l)))
    assert abs(float(M.max()) - (1 / 0.9) * 2.0) <= 2.0 ** -22 and float(M.min()) == 0.0


# ---------------------------------------------------------------------- the flair surface and the engine's plumbing, on the CPU
@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("headdrop")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def _cpu_tagger(monkeypatch, tiny_dir, **kw):
    """FastSequenceTagger on the tiny model, its engine on the CPU device (the weights' bf16 shadow by torch instead of the kernel)"""
    import flair
    from flair.data import Dictionary
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    from kbner import ops
    monkeypatch.setattr(flair, "device", torch.device("cpu"))
    monkeypatch.setattr(ops, "f32_to_bf16", lambda x, y: y.copy_(x.to(BF16)))
    monkeypatch.setattr(ops, "bf16_to_f32", lambda x, y: y.copy_(x.float()))
    td = Dictionary(add_unk=False)
    for t in ("O", "B-PER", "E-PER", "S-X", "<START>", "<STOP>"):
        td.add_item(t)
    emb = TransformerWordEmbeddings(model=tiny_dir, layers="-1", pooling_operation="first", fine_tune=True)
    return FastSequenceTagger(hidden_size=256, embeddings=StackedEmbeddings([emb]), tag_dictionary=td, tag_type="ner", use_crf=True,
                              use_rnn=False, remove_x=True, sentence_loss=True, **kw)


def test_constructor_accepts_head_and_locked_dropout(monkeypatch, tiny_dir):
    tg = _cpu_tagger(monkeypatch, tiny_dir, dropout=0.1, locked_dropout=0.5, word_dropout=0.05)
    assert (tg.use_dropout, tg.use_locked_dropout) == (0.1, 0.5)
    assert (tg.engine.head_dropout, tg.engine.locked_dropout, tg.engine.word_dropout) == (0.1, 0.5, 0.05)
    # the constructor's own defaults (dropout 0.0, locked_dropout 0.5) are accepted too: a YAML may omit the keys
    tg = _cpu_tagger(monkeypatch, tiny_dir)
    assert (tg.engine.head_dropout, tg.engine.locked_dropout) == (0.0, 0.5)
    for bad in (dict(dropout=1.0), dict(locked_dropout=-0.1), dict(locked_dropout=1.5)):
        with pytest.raises(ValueError, match=r"in \[0, 1\)"):
            _cpu_tagger(monkeypatch, tiny_dir, **bad)


def test_state_dict_round_trip_keeps_the_rates(monkeypatch, tiny_dir):
    from flair.models import FastSequenceTagger
    tg = _cpu_tagger(monkeypatch, tiny_dir, dropout=0.1, locked_dropout=0.5, word_dropout=0.0)
    state = tg._get_state_dict()
    assert (state["dropout"], state["locked_dropout"]) == (0.1, 0.5)
    back = FastSequenceTagger._init_model_with_state_dict(state)
    assert (back.use_dropout, back.use_locked_dropout) == (0.1, 0.5)
    assert (back.engine.head_dropout, back.engine.locked_dropout) == (0.1, 0.5)
    assert torch.equal(back.engine.arena.param("linear.weight"), tg.engine.arena.param("linear.weight"))
    old = {k: v for k, v in state.items() if k not in ("dropout", "locked_dropout")}     # a checkpoint from before the feature
    back = FastSequenceTagger._init_model_with_state_dict(old)
    assert (back.use_dropout, back.use_locked_dropout, back.engine.head_dropout, back.engine.locked_dropout) == (0.0, 0.0, 0.0, 0.0)


class _Spy:
    """torch stand-ins for the row / head ops of kbner.ops on the engine's module, recording every call"""

    def __init__(self, monkeypatch, eng_mod):
        self.calls = []
        for name in ("gather_rows", "gather_rows_drop", "scatter_rows", "scatter_rows_drop", "head_fwd", "head_bwd"):
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

    def head_fwd(self, x, w, bias):
        return x.float() @ w.t() + bias

    def head_bwd(self, de, x, w, dw, db):
        return (de @ w).to(BF16)

    def names(self):
        return [c[0] for c in self.calls]


B_, NC_, S_, NPOS_ = 2, 3, 8, 5


def _stub_engine(monkeypatch, tiny_dir, **rates):
    import kbner.engine as E
    tg = _cpu_tagger(monkeypatch, tiny_dir, dropout=rates.get("dropout", 0.0), locked_dropout=rates.get("locked_dropout", 0.0),
                     word_dropout=rates.get("word_dropout", 0.0))
    eng = tg.engine
    H = eng.cfg.hidden_size
    g = torch.Generator().manual_seed(3)
    hidden = torch.randn(B_ * S_, H, generator=g).to(BF16)
    monkeypatch.setattr(eng, "encoder_forward", lambda ids, pos_ids, maskbias, R, S, **kw: hidden)
    monkeypatch.setattr(eng, "acts", lambda R, S: types.SimpleNamespace(dx=torch.zeros(B_ * S_, H, dtype=BF16)))
    monkeypatch.setattr(eng, "encoder_backward", lambda dx, grad_ready=None: None)
    spy = _Spy(monkeypatch, E)
    crow = torch.tensor([1, 2, 3, 9, 10, -1], dtype=I32)
    batch = {"B": B_, "S": S_, "ids": None, "pos_ids": None, "maskbias": None, "ctags": torch.zeros(B_, NC_, dtype=I32),
             "crow_idx": crow, "cpos": torch.tensor([0, 1, 2, 0, 1, -1], dtype=I32), "n_tokens": NPOS_,
             "row_idx": torch.arange(B_ * NPOS_, dtype=I32)}
    return eng, spy, batch


def _back(eng, fwd, T):
    em, pooled, crow_idx, B, nc, R, S, drop = fwd
    eng._backprop_emissions(torch.ones(B, nc, T), pooled, crow_idx, B, nc, R, S, None, drop=drop)


def test_rates_zero_take_the_plain_ops_and_draw_nothing_more(monkeypatch, tiny_dir):
    """both rates 0, training: the plain gather / scatter run, the _drop ops never, and the engine's stream advances by the
    word-dropout draw alone -- what it did before head dropout existed"""
    eng, spy, batch = _stub_engine(monkeypatch, tiny_dir, word_dropout=0.1)
    eng.train()
    eng.seed_dropout(77)
    fwd = eng._emit(batch)
    assert fwd[-1] is None
    _back(eng, fwd, eng.T)
    assert spy.names() == ["gather_rows", "scatter_rows"]
    expect = np.random.default_rng(77)
    expect.random(NPOS_)
    assert eng._drop_rng.bit_generator.state == expect.bit_generator.state


def test_each_backward_replays_its_own_forward(monkeypatch, tiny_dir):
    """two forwards, then their two backwards (a multi-view step's order): every scatter gets the (seed, thresh) pairs of the gather of
    ITS forward; the seeds are the stream's next two 32-bit draws after that forward's word-dropout draw"""
    from kbner import ops
    eng, spy, batch = _stub_engine(monkeypatch, tiny_dir, dropout=0.1, locked_dropout=0.5, word_dropout=0.1)
    eng.train()
    eng.seed_dropout(77)
    f1 = eng._emit(batch)
    f2 = eng._emit(batch)
    _back(eng, f1, eng.T)
    _back(eng, f2, eng.T)
    assert spy.names() == ["gather_rows_drop", "gather_rows_drop", "scatter_rows_drop", "scatter_rows_drop"]
    g1, g2, s1, s2 = spy.calls
    assert g1[1:] == s1[1:] and g2[1:] == s2[1:] and g1[2][0] != g2[2][0] and g1[3][0] != g2[3][0]
    rng = np.random.default_rng(77)
    for g in (g1, g2):
        rng.random(NPOS_)
        sd = rng.integers(0, 2 ** 32, size=2, dtype="uint64")
        assert g[1] == NC_
        assert g[2] == (int(sd[0]), ops.drop_thresh(0.1)) and g[3] == (int(sd[1]), ops.drop_thresh(0.5))
    assert eng._drop_rng.bit_generator.state == rng.bit_generator.state
    # one rate alone: the other site is disabled by its threshold, the seeds are drawn all the same
    eng.head_dropout = 0.0
    f3 = eng._emit(batch)
    assert f3[-1][0][1] == 0 and f3[-1][1][1] == ops.drop_thresh(0.5)


def test_kd_path_carries_the_pair_and_eval_takes_the_plain_ops(monkeypatch, tiny_dir):
    eng, spy, batch = _stub_engine(monkeypatch, tiny_dir, dropout=0.1, locked_dropout=0.5)
    monkeypatch.setattr(eng, "kd_crf_terms", lambda em, *a, **k: (em.sum(), torch.ones_like(em)))
    eng.train()
    eng.seed_dropout(5)
    eng._kd_loss(batch, {}, 0.5, 1.0, 1.0, True, None, None)
    (g, s) = spy.calls
    assert g[0] == "gather_rows_drop" and s[0] == "scatter_rows_drop" and g[1:] == s[1:] and g[1] == NPOS_
    # eval mode: nothing drawn, the plain ops
    eng.eval()
    state = eng._drop_rng.bit_generator.state
    del spy.calls[:]
    fwd = eng._emit(batch)
    _back(eng, fwd, eng.T)
    eng._kd_loss(batch, {}, 0.5, 1.0, 1.0, True, None, None)
    assert spy.names() == ["gather_rows", "scatter_rows", "gather_rows", "scatter_rows"]
    assert eng._drop_rng.bit_generator.state == state
