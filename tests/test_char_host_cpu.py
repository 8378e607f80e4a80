"""CPU: the host surface of FastCharacterEmbeddings in the stacked tagger -- the constructor and its refusals, char_batch, ConfigParser
building an `embeddings:` block with the class (with and without kwargs) and returning char_map, the stack's block widths and columns,
every refusal of the ops wrappers' table checks (nothing is launched: there is no GPU here), the optimizer's groups, and the save /
load refusals of stack-model.pt's state."""
import numpy as np
import pytest
import torch


def _td():
    from flair.data import Dictionary
    td = Dictionary(add_unk=False)
    for it in ("<unk>", "O", "S-PER", "B-LOC", "E-LOC", "S-X", "<START>", "<STOP>"):
        td.add_item(it)
    return td


# ====================================================================== the class
def test_constructor_dictionary_and_refusals():
    from flair.embeddings import FastCharacterEmbeddings
    e = FastCharacterEmbeddings(vocab=["ab", "bca", "ab"])
    assert e.name == "Char" and e.static_embeddings is False and e.embedding_length == 50
    assert e.char_dictionary == {"<u>": 0, "a": 1, "b": 2, "c": 3, " ": 4, "\n": 5}      # first-seen order, then ' ' and '\\n' 
    assert FastCharacterEmbeddings(vocab=["x"], embedding_name="C2").name == "C2"
    assert FastCharacterEmbeddings(vocab=["x"]).char_dictionary == {"<u>": 0, "x": 1, " ": 2, "\n": 3}
    sd = e.state_dict()
    assert set(sd) == {"char_embedding.weight"} | {"char_layer.%s_l0%s" % (k, s) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")
                                                    for s in ("", "_reverse")}
    assert tuple(sd["char_embedding.weight"].shape) == (6, 25) and tuple(sd["char_layer.weight_hh_l0_reverse"].shape) == (100, 25)
    e8 = FastCharacterEmbeddings(vocab=["x"], char_embedding_dim=8, hidden_size_char=8)
    assert e8.embedding_length == 16
    with pytest.raises(NotImplementedError, match="char_cnn"):
        FastCharacterEmbeddings(vocab=["x"], char_cnn=True)
    with pytest.raises(ValueError, match=r"char_embedding_dim=25, hidden_size_char=30"):
        FastCharacterEmbeddings(vocab=["x"], hidden_size_char=30)
    with pytest.raises(ValueError, match=r"outside \[1, 32\]"):
        FastCharacterEmbeddings(vocab=["x"], char_embedding_dim=40, hidden_size_char=40)
    with pytest.raises(ValueError, match="vocab"):
        FastCharacterEmbeddings()
    # torch's generator decides the initial values
    torch.manual_seed(5)
    a = FastCharacterEmbeddings(vocab=["xy"]).state_dict()
    torch.manual_seed(5)
    b = FastCharacterEmbeddings(vocab=["xy"]).state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    k = 1.0 / 25 ** 0.5
    assert float(a["char_layer.weight_ih_l0"].abs().max()) <= k and float(a["char_embedding.weight"].abs().max()) > k


def test_char_batch_follows_get_char_idx():
    from flair.data import Sentence
    from flair.embeddings import FastCharacterEmbeddings
    e = FastCharacterEmbeddings(vocab=["abc", "d"])
    sents = [Sentence("abc d zz"), Sentence("a")]
    chars, lens, rows = e.char_batch(sents, 4)
    assert chars.dtype == lens.dtype == rows.dtype == np.int32
    assert lens.tolist() == [3, 1, 2, 1] and rows.tolist() == [0, 1, 2, 4]             # only real words; row b * n + token
    assert chars.tolist() == [[1, 2, 3], [4, 0, 0], [0, 0, 0], [1, 0, 0]]               # unknown 'z' and the padding are '<u>' = 0


# ====================================================================== ConfigParser
@pytest.fixture()
def parser(tmp_path):
    import tiny_assets
    from flair.config_parser import ConfigParser
    tiny_assets.write_conll_corpus(str(tmp_path / "data"), n_train=5, n_dev=2, n_test=2, seed=1)
    cfg = {"targets": "ner", "train": {"mini_batch_size": 2},
           "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(tmp_path / "tags.pkl"),
                   "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                         "data_folder": str(tmp_path / "data"), "tag_to_bioes": "ner"}}}
    return ConfigParser(cfg)


def test_config_parser_builds_the_class_with_and_without_kwargs(parser):
    """(fails before this class existed: 'embedding class FastCharacterEmbeddings is outside the hot path')"""
    from collections import Counter
    from flair.embeddings import FastCharacterEmbeddings
    for block in ({"FastCharacterEmbeddings": None}, {"FastCharacterEmbeddings-0": {"char_embedding_dim": 25, "hidden_size_char": 25}}):
        stacked, word_map, char_map, lemma_map, postag_map = parser.create_embeddings(block)
        emb = stacked.embeddings[0]
        assert isinstance(emb, FastCharacterEmbeddings) and char_map is emb.char_dictionary
        assert word_map is None and lemma_map is None and postag_map is None
        # vocab = the tokens of train + dev + test by falling frequency (the reference's self.tokens[1])
        full = [t for t, _ in Counter(tok.text for s in parser.corpus.get_all_sentences() for tok in s.tokens).most_common()]
        assert parser.tokens[1] == full and set(parser.tokens[0]) <= set(full)
        want = {"<u>": 0}
        for w in full:
            for c in w:
                want.setdefault(c, len(want))
        want[" "] = len(want)
        want["\n"] = len(want)
        assert char_map == want and list(char_map) == list(want)
    with pytest.raises(NotImplementedError, match="outside the hot path"):
        parser.create_embeddings({"LemmaEmbeddings": None})


# ====================================================================== the stack
@pytest.fixture()
def taggers(tmp_path):
    import tiny_assets
    from flair.embeddings import FastCharacterEmbeddings, StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    tiny_assets.build_model_dir(str(tmp_path / "enc"), seed=0)

    def make(with_char=True, **kw):
        torch.manual_seed(3)
        embs = [TransformerWordEmbeddings(model=str(tmp_path / "enc"), layers="-1", pooling_operation="first")]
        if with_char:
            embs.insert(0, FastCharacterEmbeddings(vocab=["alice", "bob", "berlin"]))
        args = dict(hidden_size=32, embeddings=StackedEmbeddings(embs), tag_dictionary=_td(), tag_type="ner", use_crf=True, use_rnn=True)
        args.update(kw)
        return FastSequenceTagger(**args)
    return make


def test_stack_blocks_columns_and_refusals(taggers):
    from flair.embeddings import FastCharacterEmbeddings, StackedEmbeddings
    t = taggers()
    names = [e.name for e in t._stack_embs]
    assert names == sorted(names) and names[1] == "Char" and t._char_slot == 1           # (the encoder's name is its path: '/' < 'C')
    head = t.stack_head
    assert head.blocks == [128, 50] and head.cols == [0, 128] and head.Dp == 192        # 50 columns padded to 64, at a multiple of 32
    assert tuple(t._stack_state["rnn"]["weight_ih_l0"].shape) == (128, 178)
    cemb = t._stack_embs[1]
    head = t.enable_stack_training()                                                   # the fine_tune refusal does not trip on it
    assert head.char is t._char_net() and head.char.V == len(cemb.char_dictionary) and head.char.g.numel() == head.char.n
    assert {n for n, _ in t.named_parameters()} >= {"embeddings.list_embedding_0.char_embedding.weight",
                                                     "embeddings.list_embedding_0.char_layer.weight_hh_l0_reverse"}
    assert taggers(with_char=False).enable_stack_training().char is None
    with pytest.raises(NotImplementedError, match="at most one FastCharacterEmbeddings"):
        taggers(embeddings=StackedEmbeddings([FastCharacterEmbeddings(vocab=["a"]), FastCharacterEmbeddings(vocab=["a"], embedding_name="C2")]))
    with pytest.raises(NotImplementedError, match="exactly one TransformerWordEmbeddings"):
        taggers(use_rnn=False)                                  # [encoder, Char] without the BiLSTM: the existing refusal
    # deselected: no step object, so neither kernel can be launched
    from flair.data import Sentence
    t.embedding_selector, t.selection = True, [1, 0]
    assert t._char_step([Sentence("alice bob")], 2) is None
    t.selection = [1, 1]
    step = t._char_step([Sentence("alice bob")], 2)
    assert step.col == 128 and step.rows.tolist() == [0, 1] and step.net is head.char


def test_char_arena_round_trip_and_optimizer_groups(taggers):
    from kbner import stack as K
    t = taggers()
    head = t.enable_stack_training()
    net = head.char
    sd = t._stack_embs[t._char_slot].state_dict()
    back = net.state()
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)       # the host modules' values, bit for bit
    before = net.arena.clone()
    net.load_state(back)
    assert torch.equal(net.arena, before) and net.n % 4 == 0
    assert net.param("wih").shape == (2, 100, 25) and net.grad("emb").shape == net.param("emb").shape
    opt = K.StackOptimizer(head, name="SGD", lr=0.1, lr_rate=0.5)
    assert opt.groups() == [("rnn+transitions", head.split, 0.05), ("linear", head.n - head.split, 0.1), ("char", net.n, 0.1)]
    assert opt.cm is None
    opt = K.StackOptimizer(head, name="AdamW", lr=0.1, lr_rate=0.5)
    assert opt.cm.numel() == net.n and opt.cv.numel() == net.n
    plain = taggers(with_char=False).enable_stack_training()
    assert [g[0] for g in K.StackOptimizer(plain, name="SGD").groups()] == ["rnn+transitions", "linear"]


def test_save_and_load_carry_the_character_state_or_refuse(taggers):
    t, plain = taggers(), taggers(with_char=False)
    st, st_plain = t._stack_state, plain._stack_state
    assert set(st) == {"rnn", "linear.weight", "linear.bias", "transitions", "char", "char_dictionary"}
    assert set(st_plain) == {"rnn", "linear.weight", "linear.bias", "transitions"}
    assert st["char_dictionary"] == t._stack_embs[t._char_slot].char_dictionary
    # a state without them into a tagger that has the embedding, and the other way round: refused, saying which side lacks it
    with pytest.raises(ValueError, match="state carries no character"):
        t.load_stack_state({k: v for k, v in st.items() if k not in ("char", "char_dictionary")})
    wide = dict(st_plain, char=st["char"], char_dictionary=st["char_dictionary"])
    with pytest.raises(ValueError, match="no FastCharacterEmbeddings"):
        plain.load_stack_state(wide)
    # restores both, also a dictionary of another size
    other = taggers()
    new = {k: (v + 1.0) for k, v in st["char"].items()}
    new["char_embedding.weight"] = torch.cat([new["char_embedding.weight"], torch.ones(1, 25)])
    other.load_stack_state(dict(st, char=new, char_dictionary=dict(st["char_dictionary"], **{"~": len(st["char_dictionary"])})))
    got = other._stack_state
    assert all(torch.equal(got["char"][k], new[k]) for k in new) and got["char_dictionary"]["~"] == len(st["char_dictionary"])
    assert other._stack_embs[other._char_slot].char_dictionary == got["char_dictionary"]
    with pytest.raises(ValueError, match="disagree"):
        other.load_stack_state(dict(st, char=new))


# ====================================================================== ops refusals (before any launch)
def test_table_checks_refuse_before_upload():
    from kbner import ops
    from kbner.lib import KbnerError
    chars, lens, rows = np.array([[1, 2, 0], [3, 0, 0]], np.int32), np.array([2, 1], np.int32), np.array([4, -1], np.int32)
    ch, ln, rw = ops.check_char_tables(chars, lens, rows, 4, 8)
    assert ch.dtype == ln.dtype == rw.dtype == torch.int32 and not ch.is_cuda
    bad = [("character ids", dict(chars=np.array([[1, 4, 0], [3, 0, 0]], np.int32))),
           ("character ids", dict(chars=np.array([[1, -1, 0], [3, 0, 0]], np.int32))),
           ("lengths", dict(lens=np.array([2, 0], np.int32))), ("lengths", dict(lens=np.array([4, 1], np.int32))),
           ("more than one word", dict(rows=np.array([4, 4], np.int32))), ("rows must be -1", dict(rows=np.array([8, -1], np.int32))),
           ("rows must be -1", dict(rows=np.array([4, -2], np.int32))), ("HOST", dict(lens=np.array([2.0, 1.0]))),
           ("chars \\[W, Lmax", dict(rows=np.array([4], np.int32)))]
    for match, kw in bad:
        args = dict(chars=chars, lens=lens, rows=rows)
        args.update(kw)
        with pytest.raises(KbnerError, match=match):
            ops.check_char_tables(args["chars"], args["lens"], args["rows"], 4, 8)
    assert ops.check_char_tables(chars, lens, np.array([-1, -1], np.int32), 4, 8)[2].tolist() == [-1, -1]       # -1 may repeat


def test_block_and_parameter_checks_refuse_before_any_launch(monkeypatch):
    from kbner import lib as L
    from kbner import ops
    monkeypatch.setattr(L, "call", lambda *a: pytest.fail("a refused call reached the library"))
    tab = ops.CharTables(np.zeros((0, 1), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 6, 8, "cpu")
    f = lambda *s: torch.zeros(*s)      # noqa: E731
    par = [f(6, 25), f(2, 100, 25), f(2, 100, 25), f(2, 100), f(2, 100)]
    m = torch.zeros((8, 128), dtype=torch.bfloat16)
    for col, match in ((4, "multiple of 8"), (96, "lie inside"), (-8, "multiple of 8")):
        with pytest.raises(L.KbnerError, match=match):
            ops.char_lstm_fwd(*par, tab, m, col, 4)
    with pytest.raises(L.KbnerError, match="16-byte"):
        ops.char_lstm_fwd(*par, tab, torch.zeros((8 * 128 + 8,), dtype=torch.bfloat16)[4:4 + 8 * 128].view(8, 128), 0, 4)
    with pytest.raises(L.KbnerError, match="bfloat16"):
        ops.char_lstm_fwd(*par, tab, m.float(), 0, 4)
    with pytest.raises(L.KbnerError, match="-22"):
        ops.char_lstm_fwd(f(6, 40), f(2, 160, 40), f(2, 160, 40), f(2, 160), f(2, 160), tab, m, 0, 4)
    with pytest.raises(L.KbnerError, match="wih \\[2, 4Hc, E\\]"):
        ops.char_lstm_fwd(par[0], f(2, 100, 24), *par[2:], tab, m, 0, 4)
    with pytest.raises(L.KbnerError, match="emb \\[V = 6"):
        ops.char_lstm_fwd(f(7, 25), *par[1:], tab, m, 0, 4)
    with pytest.raises(L.KbnerError, match="rows"):
        ops.char_lstm_fwd(*par, tab, m[:4], 0, 4)
    with pytest.raises(L.KbnerError, match="cuda"):                                       # host tensors: dtypes and devices last
        ops.char_lstm_fwd(*par, tab, m, 0, 4)
