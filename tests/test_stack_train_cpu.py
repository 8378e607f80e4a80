"""CPU: the host side of stacked-tagger training -- the prefix-active check of the LSTM training wrapper, the new entry points in
the binding, the constructor accepting dropout with use_rnn, and the parameter layout of the trainable head (no kernel runs)."""
import numpy as np
import pytest


def test_new_entry_points_are_bound():
    from kbner import lib
    for name, nargs in (("kbner_lstm_seq_train", 18), ("kbner_lstm_seq_bwd", 16), ("kbner_sgd", 11)):
        assert name in lib.SIGNATURES and len(lib.SIGNATURES[name][1]) == nargs, name
    from kbner import ops, stack
    assert callable(ops.sgd) and callable(stack.StackOptimizer) and callable(stack.BiLSTMHead.loss_backward)


def test_prefix_active_check_of_the_host_wrapper():
    from kbner.lib import KbnerError
    from kbner.stack import check_prefix_active, step_tables
    tab = step_tables([4, 1, 3, 0], 5)
    out = check_prefix_active(tab, 20, 2, 4)
    assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and np.array_equal(out, tab)
    assert check_prefix_active(np.zeros((0, 2, 4), np.int32), 20, 2, 4).shape == (0, 2, 4)
    bad = tab.copy()
    bad[3, 0, 1] = 7                                  # active again after it finished
    with pytest.raises(KbnerError, match="prefix-active"):
        check_prefix_active(bad, 20, 2, 4)
    bad = tab.copy()
    bad[1, 1, 0] = bad[0, 1, 0]                       # one direction consumes a row twice
    with pytest.raises(KbnerError, match="twice"):
        check_prefix_active(bad, 20, 2, 4)
    dup = tab.copy()
    dup[0, 1, 2] = dup[0, 0, 0]                       # two DIRECTIONS may share a row: their column blocks differ
    if len(np.unique(dup[:, 1][dup[:, 1] >= 0])) == (dup[:, 1] >= 0).sum():
        check_prefix_active(dup, 20, 2, 4)
    with pytest.raises(KbnerError, match="below"):
        check_prefix_active(tab, 10, 2, 4)            # a row past the buffer
    bad = tab.copy()
    bad[0, 0, 0] = -2
    with pytest.raises(KbnerError):
        check_prefix_active(bad, 20, 2, 4)
    with pytest.raises(KbnerError):
        check_prefix_active(tab, 20, 1, 4)            # wrong shape
    with pytest.raises(KbnerError):
        check_prefix_active(tab.astype(np.float32), 20, 2, 4)


def test_stack_optimizer_refuses_unknown_names_and_untrainable_heads():
    from kbner import stack as K
    from kbner.lib import KbnerError

    class Head:
        arena = None
    with pytest.raises(NotImplementedError, match="Adagrad"):
        K.StackOptimizer(Head(), name="Adagrad")
    with pytest.raises(KbnerError):
        K.StackOptimizer(Head(), name="SGD")


def test_tagger_constructor_accepts_dropout_with_use_rnn(tmp_path):
    """dropout > 0 with use_rnn used to be refused; it is a rate of the trainable head now, validated like the fine-tuning tagger's.
    The default construction allocates no arena; train() / eval() no longer warn that the mode has no effect."""
    import logging
    import tiny_assets
    from flair.data import Dictionary
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    tiny_assets.build_model_dir(str(tmp_path / "enc"), seed=0)
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "<START>", "<STOP>"):
        td.add_item(it)
    emb = TransformerWordEmbeddings(model=str(tmp_path / "enc"), layers="-1", pooling_operation="first")
    kw = dict(hidden_size=32, embeddings=StackedEmbeddings([emb]), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=True)
    t = FastSequenceTagger(dropout=0.2, locked_dropout=0.5, word_dropout=0.05, **kw)
    assert (t.use_dropout, t.use_locked_dropout, t.use_word_dropout) == (0.2, 0.5, 0.05) and t.stack_head.arena is None
    for bad in ({"dropout": 1.5}, {"locked_dropout": -0.1}, {"word_dropout": 1.0}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            FastSequenceTagger(**dict(kw, **bad))
    seen = []
    h = logging.Handler()
    h.emit = lambda rec: seen.append(rec.getMessage())
    logging.getLogger("flair").addHandler(h)
    try:
        t.train()
        t.eval()
    finally:
        logging.getLogger("flair").removeHandler(h)
    assert not any("no effect" in m for m in seen)
    assert {n for n, _ in t.named_parameters()} >= {"transitions", "linear.weight", "linear.bias", "rnn.weight_hh_l0_reverse"}
    for name in ("multi_view", "distill_interpolation", "grad_ready"):          # refused by name before anything runs
        with pytest.raises(NotImplementedError, match=name):
            t.forward_backward([], **{name: 1})


def _state(rng, D, H, T):
    k = 1.0 / np.sqrt(H)
    st = {"rnn": {}}
    for s in ("", "_reverse"):
        st["rnn"]["weight_ih_l0" + s] = rng.uniform(-k, k, (4 * H, D)).astype(np.float32)
        st["rnn"]["weight_hh_l0" + s] = rng.uniform(-k, k, (4 * H, H)).astype(np.float32)
        st["rnn"]["bias_ih_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
        st["rnn"]["bias_hh_l0" + s] = rng.uniform(-k, k, 4 * H).astype(np.float32)
    st["linear.weight"] = rng.standard_normal((T, 2 * H)).astype(np.float32)
    st["linear.bias"] = rng.standard_normal(T).astype(np.float32)
    st["transitions"] = rng.standard_normal((T, T)).astype(np.float32)
    return st


def test_arena_and_state_dict_round_trip_exactly():
    """the reference-layout dict -> padded arena -> dict: every value bit for bit, padding exactly zero, the default head untouched"""
    import torch
    from kbner import stack as K
    rng = np.random.default_rng(0)
    D, H, T = 72, 100, 9                      # Dp 128 (blocks 64 + 8 at 32-aligned columns), Hp 128, T odd
    st = _state(rng, D, H, T)
    rnn = {k: torch.from_numpy(v) for k, v in st["rnn"].items()}
    plain = K.BiLSTMHead(rnn, st["linear.weight"], st["linear.bias"], [D - 8, 8], H, "cpu")
    assert plain.arena is None and not plain.training and not hasattr(plain, "g") and not hasattr(plain, "shadow")
    head = K.BiLSTMHead(rnn, st["linear.weight"], st["linear.bias"], [D - 8, 8], H, "cpu", transitions=st["transitions"], trainable=True)
    assert head.Dp == plain.Dp and head.Hp == plain.Hp == 128 and head.Dq % 128 == 0 and head.n % 4 == 0 and head.n_shadow % 4 == 0
    assert head.split % 4 == 0 and head.n_shadow < head.split < head.n
    back = head.state()
    for k, v in st["rnn"].items():
        assert np.array_equal(back["rnn"][k].numpy(), v), k
    for k in ("linear.weight", "linear.bias", "transitions"):
        assert np.array_equal(back[k].numpy(), st[k]), k
    before = head.arena.clone()
    head.load_state(back)
    assert torch.equal(before, head.arena)
    # what inference reads is the bf16 rounding of the same weights the default head holds
    assert torch.equal(head.wih[:, :plain.Dp], plain.wih) and torch.equal(head.grp.whh, plain.grp.whh)
    assert torch.equal(head.bias, plain.bias) and torch.equal(head.lin_w, plain.lin_w) and torch.equal(head.lin_b, plain.lin_b)
    # the two biases are two parameters; padded entries are zero: real entries = the state's element count
    assert not torch.equal(head.param("bias_ih"), head.param("bias_hh"))
    n_real = sum(v.size for v in st["rnn"].values()) + st["linear.weight"].size + T + T * T
    assert int((head.arena != 0).sum()) == n_real
    # the gradient buffer reads back through the same layout
    head.g.copy_(head.arena * 2)
    g = head.state_of(head.g)
    assert np.array_equal(g["rnn"]["weight_hh_l0_reverse"].numpy(), 2 * st["rnn"]["weight_hh_l0_reverse"])


def test_trainer_refusals_of_the_stack_branch():
    """ModelFinetuner.train with a use_rnn model: what the single-process loop does not do is refused by name, before any work"""
    from flair.trainers import ModelFinetuner

    class Model:
        use_rnn = True
        multi_view_training = False

    class Corpus:
        targets = []
    base = dict(learning_rate=0.1, mini_batch_size=2, eval_mini_batch_size=None, max_epochs=1, gradient_accumulation_steps=1, lr_rate=1,
                shuffle=False, sort_data=True, checkpoint=False, train_with_dev=False, use_amp=False, use_autocast=False, rootschedule=False,
                freezing=False, use_unlabeled_data=False, unlabeled_data_for_zeroshot=False, gold_reward=False,
                language_attention_warmup=False, language_attention_warmup_and_fix=False)
    import tempfile
    from pathlib import Path
    tr = ModelFinetuner(Model(), None, Corpus(), optimizer="SGD")
    assert tr.optimizer_name == "SGD"
    with tempfile.TemporaryDirectory() as d:
        for kw, name in (({"checkpoint": True}, "checkpoint"), ({"train_with_dev": True}, "train_with_dev"), ({"use_amp": True}, "use_amp")):
            with pytest.raises(NotImplementedError, match=name):
                tr._train_stack(Path(d), dict(base, **kw), {})
        tr.distill_mode = True
        with pytest.raises(NotImplementedError, match="distill_mode"):
            tr._train_stack(Path(d), dict(base), {})
        tr.distill_mode = False
        import os
        old = os.environ.get("WORLD_SIZE")
        os.environ["WORLD_SIZE"] = "2"
        try:
            from kbner import dp
            if dp.world_size() > 1:
                with pytest.raises(NotImplementedError, match="WORLD_SIZE"):
                    tr._train_stack(Path(d), dict(base), {})
        finally:
            if old is None:
                os.environ.pop("WORLD_SIZE", None)
            else:
                os.environ["WORLD_SIZE"] = old
        assert not os.listdir(d)                # nothing was written by a refused run
