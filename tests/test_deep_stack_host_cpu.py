"""CPU: the host surface of rnn_layers > 1 and train_initial_hidden_state in the stacked tagger -- the constructor switches and their
refusals, the reference's parameter names, the parameter blocks of kbner.stack.BiLSTMHead (state -> arenas -> state bit for bit, padding
exactly zero, a one-layer head unchanged), the optimizer's groups, the refusals of load_stack_state, and the binding of the new entry
point.  Nothing is launched: there is no GPU here."""
import numpy as np
import pytest
import torch

SFX = ("", "_reverse")


def _td():
    from flair.data import Dictionary
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)
    return td


@pytest.fixture(scope="module")
def make(tmp_path_factory):
    import tiny_assets
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    d = tmp_path_factory.mktemp("deep_host")
    tiny_assets.build_model_dir(str(d / "enc"), seed=0)

    def _make(**kw):
        torch.manual_seed(3)
        embs = [TransformerWordEmbeddings(model=str(d / "enc"), layers="-1", pooling_operation="first", fine_tune=not kw.get("use_rnn", True))]
        args = dict(hidden_size=40, embeddings=StackedEmbeddings(embs), tag_dictionary=_td(), tag_type="ner", use_crf=True, use_rnn=True)
        args.update(kw)
        return FastSequenceTagger(**args)
    return _make


# ====================================================================== the constructor
def test_constructor_accepts_the_switches_and_refuses_zero_layers(make):
    from flair.models.sequence_tagger_model import _UNSUPPORTED_TRUE
    assert "train_initial_hidden_state" not in _UNSUPPORTED_TRUE and "relearn_embeddings" in _UNSUPPORTED_TRUE
    t = make(rnn_layers=2, train_initial_hidden_state=True)              # (both raised NotImplementedError before)
    assert t.nlayers == 2 and t.train_initial_hidden_state is True
    head = t.stack_head
    assert head.L == 2 and len(head.upper) == 1 and head.init is not None and head.rnn_dropout == 0.5
    assert make(rnn_layers=3).stack_head.L == 3 and make(rnn_layers=3).stack_head.init is None
    plain = make()
    assert plain.nlayers == 1 and plain.stack_head.L == 1 and plain.stack_head.upper == [] and plain.stack_head.init is None
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="rnn_layers"):
            make(rnn_layers=bad)
    with pytest.raises(ValueError, match="rnn_layers"):
        make(rnn_layers=0, use_rnn=False)                                 # (refused before the engine is built)
    # what stays refused, by name
    with pytest.raises(NotImplementedError, match="relearn_embeddings"):
        make(rnn_layers=2, relearn_embeddings=True)
    with pytest.raises(NotImplementedError, match="use_crf=False"):
        make(rnn_layers=2, use_crf=False)


def test_a_one_layer_tagger_draws_the_weights_it_always_drew(make):
    """the layers above the first and the initial state are drawn after everything else: layer 0, linear and transitions of a deeper
    tagger are the one-layer tagger's"""
    a, b = make()._stack_state, make(rnn_layers=2, train_initial_hidden_state=True)._stack_state
    assert all(torch.equal(a["rnn"][k], b["rnn"][k]) for k in a["rnn"])
    assert all(torch.equal(a[k], b[k]) for k in ("linear.weight", "linear.bias", "transitions"))
    assert set(a) == {"rnn", "linear.weight", "linear.bias", "transitions"}
    assert set(b) == set(a) | {"lstm_init_h", "lstm_init_c", "rnn_layers", "train_initial_hidden_state"}
    k = 1.0 / 40 ** 0.5
    assert float(b["rnn"]["weight_ih_l1"].abs().max()) <= k and float(b["lstm_init_h"].abs().max()) > 1.0       # uniform(+-k) / randn


def test_named_parameters_are_the_references(make):
    """the names torch gives FastSequenceTagger's modules in the reference: rnn = torch.nn.LSTM(num_layers=L, bidirectional=True),
    lstm_init_h / lstm_init_c Parameters, linear, transitions"""
    L = 2
    t = make(rnn_layers=L, train_initial_hidden_state=True)
    ref = torch.nn.LSTM(128, 40, num_layers=L, bidirectional=True)
    want = {"rnn." + k for k, _ in ref.named_parameters()} | {"lstm_init_h", "lstm_init_c", "linear.weight", "linear.bias", "transitions"}
    got = dict(t.named_parameters())
    assert set(got) == want
    for k, p in ref.named_parameters():
        assert tuple(got["rnn." + k].shape) == tuple(p.shape), k
    assert tuple(got["lstm_init_h"].shape) == tuple(got["lstm_init_c"].shape) == (2 * L, 40)
    assert [k for k in got if k.startswith("rnn.")] == ["rnn." + k for k, _ in ref.named_parameters()]       # torch's order too
    assert set(dict(make().named_parameters())) == {"rnn." + k for k, _ in torch.nn.LSTM(128, 40, 1, bidirectional=True).named_parameters()} | {
        "linear.weight", "linear.bias", "transitions"}
    # after enable_stack_training the same names, read from the arenas
    t.enable_stack_training()
    assert set(dict(t.named_parameters())) == want


def test_without_use_rnn_both_switches_are_accepted_and_select_nothing(make, monkeypatch):
    """(the fine-tuning tagger's engine needs a GPU: its construction is stubbed here; tests/test_gpu_deep_stack_e2e.py builds it)"""
    from flair.models import sequence_tagger_model as M
    monkeypatch.setattr(M.SequenceTagger, "_build_engine", lambda self: None)
    M._LOGGED_ONCE.clear()
    lines = []
    monkeypatch.setattr(M.log, "info", lambda msg, *a, **k: lines.append(msg % a))
    t = make(use_rnn=False, rnn_layers=2, train_initial_hidden_state=True)
    make(use_rnn=False, rnn_layers=3)
    said = [m for m in lines if "no effect without use_rnn" in m]
    assert len(said) == 1                                                  # logged once
    assert t.stack_head is None and t.nlayers == 2 and t.train_initial_hidden_state is True and "_stack_state_host" not in t.__dict__


# ====================================================================== the head's parameter blocks
def _state(D, H, T, L, init, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnn = {}
    for k in range(L):
        for s in SFX:
            rnn["weight_ih_l%d%s" % (k, s)] = torch.randn(4 * H, D if k == 0 else 2 * H, generator=g)
            rnn["weight_hh_l%d%s" % (k, s)] = torch.randn(4 * H, H, generator=g)
            rnn["bias_ih_l%d%s" % (k, s)] = torch.randn(4 * H, generator=g)
            rnn["bias_hh_l%d%s" % (k, s)] = torch.randn(4 * H, generator=g)
    st = {"rnn": rnn, "linear.weight": torch.randn(T, 2 * H, generator=g), "linear.bias": torch.randn(T, generator=g),
          "transitions": torch.randn(T, T, generator=g)}
    if init:
        st["lstm_init_h"], st["lstm_init_c"] = torch.randn(2 * L, H, generator=g), torch.randn(2 * L, H, generator=g)
    return st


def _head(st, D, H, L, trainable=True):
    from kbner import stack as K
    ini = {k: st[k] for k in ("lstm_init_h", "lstm_init_c")} if "lstm_init_h" in st else None
    return K.BiLSTMHead(st["rnn"], st["linear.weight"], st["linear.bias"], [D - 8, 8], H, "cpu", transitions=st["transitions"],
                        trainable=trainable, rnn_layers=L, init_state=ini)


def _same(a, b):
    assert set(a) == set(b) and set(a["rnn"]) == set(b["rnn"])
    for k in a["rnn"]:
        assert torch.equal(a["rnn"][k], b["rnn"][k]), k
    for k in a:
        if k != "rnn":
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("L", [2, 3])
def test_state_to_arenas_to_state_is_bit_for_bit_and_padding_is_zero(L, init):
    D, H, T = 72, 40, 9
    st = _state(D, H, T, L, init)
    head = _head(st, D, H, L)
    Hp = head.Hp
    assert Hp == 64 and len(head.upper) == L - 1 and (head.init is not None) == init
    _same(head.state(), st)
    assert list(head.state()["rnn"]) == [k for k, _ in torch.nn.LSTM(D, H, L, bidirectional=True).named_parameters()]
    for lay in head.upper:
        assert lay.n == 8 * Hp * 2 * Hp + 2 * 4 * Hp * Hp + 16 * Hp and lay.n_shadow == 8 * Hp * 2 * Hp + 2 * 4 * Hp * Hp
        assert lay.g.numel() == lay.n and not bool(lay.g.any())
        assert torch.equal(lay.shadow, lay.arena[:lay.n_shadow].to(torch.bfloat16))
        w = lay.param("wih").view(2, 4, Hp, 2 * Hp)
        assert not bool(w[:, :, H:].any()) and not bool(w[..., H:Hp].any()) and not bool(w[..., Hp + H:].any())      # rows and columns
        assert bool(w[:, :, :H, :H].all()) and bool(w[:, :, :H, Hp:Hp + H].all())                                    # [0, H) and [Hp, Hp + H)
        hh = lay.param("whh").view(2, 4, Hp, Hp)
        assert not bool(hh[:, :, H:].any()) and not bool(hh[..., H:].any())
        for b in ("bias_ih", "bias_hh"):
            assert not bool(lay.param(b).view(2, 4, Hp)[..., H:].any())
        src = st["rnn"]["weight_ih_l%d_reverse" % lay.k]
        assert torch.equal(w[1, 2, :H, Hp:Hp + H], src[2 * H:3 * H, H:])
    if init:
        assert head.init.n == 2 * 2 * L * Hp and head.init.shadow is None
        assert not bool(head.init.param("h")[:, H:].any()) and not bool(head.init.param("c")[:, H:].any())
        assert torch.equal(head.init.param("h")[:, :H], st["lstm_init_h"]) and torch.equal(head.init.h16, head.init.param("h").to(torch.bfloat16))
        assert torch.equal(head.init.of_layer(L - 1)[1][1, :H], st["lstm_init_c"][2 * (L - 1) + 1])                 # row 2k + d
    # a second state through load_state, and back
    other = _state(D, H, T, L, init, seed=1)
    head.load_state(other)
    _same(head.state(), other)
    # gradients come back in the same layout
    gs = head.grad_state()
    assert set(gs["rnn"]) == set(st["rnn"]) and ("lstm_init_h" in gs) == init
    # the inference head (not trainable) holds the same operands and allocates no gradient
    plain = _head(st, D, H, L, trainable=False)
    assert plain.arena is None and all(blk.g is None for blk in plain.blocks_extra())
    head.load_state(st)
    assert all(torch.equal(a.shadow, b.shadow) for a, b in zip(plain.upper, head.upper))


def test_a_one_layer_head_is_what_it_was():
    """n, offsets, n_shadow and split by the formulae tests/test_stack_train_cpu.py reads, no block beside the arena"""
    D, H, T = 72, 40, 9
    st = _state(D, H, T, 1, False)
    head = _head(st, D, H, 1)
    Hp, Dq = head.Hp, head.Dq
    assert head.upper == [] and head.init is None and head.blocks_extra() == [] and head.L == 1 and head.rnn_dropout == 0.0
    assert head._FIELDS == ("wih", "whh", "bias_ih", "bias_hh", "transitions", "linear.weight", "linear.bias")
    r4 = lambda x: (x + 3) // 4 * 4                                                   # noqa: E731
    sizes = [8 * Hp * Dq, 2 * 4 * Hp * Hp, 8 * Hp, 8 * Hp, T * T, T * 2 * Hp, T]
    offs = np.concatenate([[0], np.cumsum([r4(s) for s in sizes])])
    assert [head.offsets[k] for k in head._FIELDS] == offs[:-1].tolist() and head.n == offs[-1]
    assert head.n_shadow == head.offsets["bias_ih"] and head.split == head.offsets["linear.weight"]
    assert head.Dp == 128 and Dq == 128 and Hp == 64 and head.n % 4 == 0 and head.n_shadow < head.split < head.n
    assert set(head.state()) == {"rnn", "linear.weight", "linear.bias", "transitions"} and len(head.state()["rnn"]) == 8
    # a deeper head keeps exactly this arena
    deep = _head(_state(D, H, T, 3, True), D, H, 3)
    assert deep.n == head.n and deep.offsets == head.offsets and deep.n_shadow == head.n_shadow and deep.split == head.split
    # ... and the layer count of the state must be the head's
    from kbner import stack as K
    with pytest.raises(ValueError, match="2 layer"):
        K.BiLSTMHead(_state(D, H, T, 2, False)["rnn"], st["linear.weight"], st["linear.bias"], [D - 8, 8], H, "cpu")
    with pytest.raises(ValueError, match="at least 1"):
        _head(st, D, H, 0)
    with pytest.raises(ValueError, match="initial state"):
        head.load_state(_state(D, H, T, 1, True))


def test_the_optimizer_places_every_new_tensor_in_the_lr_rate_group(monkeypatch):
    from kbner import lib as L_
    from kbner import stack as K
    D, H, T = 72, 40, 9
    head = _head(_state(D, H, T, 3, True), D, H, 3)
    monkeypatch.setattr(L_, "load", lambda: type("Lib", (), {"kbner_sqnorm_ws_floats": staticmethod(lambda: 64)})())
    opt = K.StackOptimizer(head, name="AdamW", lr=0.1, lr_rate=0.25)
    opt.lr_scale = 0.5
    groups = opt.groups()
    assert [g[0] for g in groups] == ["rnn+transitions", "linear", "rnn layer 1", "rnn layer 2", "lstm_init"]
    assert [g[1] for g in groups] == [head.split, head.n - head.split, head.upper[0].n, head.upper[1].n, head.init.n]
    slow, plain = 0.1 * 0.25 * 0.5, 0.1 * 0.5
    assert [g[2] for g in groups] == [slow, plain, slow, slow, slow]
    assert [m.numel() for m in opt.xm] == [b.n for b in head.blocks_extra()] == [v.numel() for v in opt.xv]
    one = K.StackOptimizer(_head(_state(D, H, T, 1, False), D, H, 1), name="SGD")
    assert [g[0] for g in one.groups()] == ["rnn+transitions", "linear"] and one.xm == []


# ====================================================================== state files
def test_load_stack_state_refuses_another_layer_count_or_initial_state_with_both_sides_named(make):
    deep, plain = make(rnn_layers=2, train_initial_hidden_state=True), make()
    st2, st1 = deep._stack_state, plain._stack_state
    assert st2["rnn_layers"] == 2 and st2["train_initial_hidden_state"] is True and "rnn_layers" not in st1
    with pytest.raises(ValueError, match=r"rnn_layers=2.*rnn_layers=1"):
        plain.load_stack_state(st2)
    with pytest.raises(ValueError, match=r"rnn_layers=1.*rnn_layers=2"):
        deep.load_stack_state(st1)
    no_init = make(rnn_layers=2)
    with pytest.raises(ValueError, match=r"train_initial_hidden_state=True.*train_initial_hidden_state=False"):
        no_init.load_stack_state(st2)
    with pytest.raises(ValueError, match=r"train_initial_hidden_state=False.*train_initial_hidden_state=True"):
        deep.load_stack_state(no_init._stack_state)
    with pytest.raises(ValueError, match="holds 2 BiLSTM layer"):             # keys and tensors that disagree
        deep.load_stack_state(dict(st2, rnn_layers=3))
    # nothing was replaced by the refused calls; its own state loads, through the inference head and through the arenas
    before = deep._stack_state
    deep.load_stack_state(before)
    twin = make(rnn_layers=2, train_initial_hidden_state=True)
    twin.load_stack_state(st2)
    twin.enable_stack_training()
    twin.load_stack_state(st2)
    after = twin._stack_state
    assert all(torch.equal(after["rnn"][k], st2["rnn"][k]) for k in st2["rnn"]) and torch.equal(after["lstm_init_c"], st2["lstm_init_c"])
    # the keys are optional: the tensors decide (a state written without them)
    twin.load_stack_state({k: v for k, v in st2.items() if k not in ("rnn_layers", "train_initial_hidden_state")})


def test_a_state_from_before_the_switches_loads_as_one_layer_without_initial_state(make, tmp_path):
    plain = make()
    old = {k: v for k, v in plain._stack_state.items()}
    assert "rnn_layers" not in old and "lstm_init_h" not in old
    torch.save(old, str(tmp_path / "stack-model.pt"))
    fresh = make()
    fresh.load_stack_state(torch.load(str(tmp_path / "stack-model.pt"), map_location="cpu", weights_only=False))
    assert fresh.nlayers == 1 and fresh.train_initial_hidden_state is False and fresh.stack_head.L == 1 and fresh.stack_head.init is None


def test_the_binding_holds_the_new_entry_point():
    from ctypes import c_int
    from kbner import lib
    res, args = lib.SIGNATURES["kbner_lstm_seq_bwd_init"]
    old = lib.SIGNATURES["kbner_lstm_seq_bwd"][1]
    assert res is c_int and len(args) == len(old) + 2 == 18
    assert args[8] is lib.P and args[12] is lib.P and [a for i, a in enumerate(args) if i not in (8, 12)] == old       # c0 and dh0
    assert hasattr(lib.load(), "kbner_lstm_seq_bwd_init")
