"""CPU: the host side of the sub-token pooling of frozen TransformerWordEmbeddings in the stacked tagger.
  - the constructor takes first / last / first_last / mean when frozen, doubles the width for first_last, and keeps its named refusals;
  - prepare_pool_batch agrees with prepare_stack_batch (the first entry of every span is the old first sub-token; empty spans where it
    has -1) and, on a sentence longer than one window with a word astride the seam, pooling through the tables equals pooling the
    sequence stitched by the reference's rule (flair/embeddings.py:3292-3299);
  - kbner.ops.pool_rows_layers refuses every malformed table or shape before anything is launched;
  - FastSequenceTagger._build_stack accepts and sizes the blocks; load_stack_state refuses a width mismatch by name;
  - the tagger on the transformer's own features (use_rnn: false) refuses a frozen embedding with another pooling than 'first'."""
import os

import numpy as np
import pytest
import torch

import poolref as pr

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("pool_host")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def _dictionary():
    from flair.data import Dictionary
    td = Dictionary(add_unk=False)
    for t in ("<unk>", "O", "S-PER", "S-LOC", "<START>", "<STOP>"):
        td.add_item(t)
    return td


# ---------------------------------------------------------------------- constructor
def test_constructor_takes_the_four_poolings_when_frozen(tiny_dir):
    from flair.embeddings import TransformerWordEmbeddings
    H = 128
    for op in pr.OPS:
        e = TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation=op)
        assert e.pooling_operation == op and e.embedding_length == (4 * H if op == "first_last" else 2 * H)
        m = TransformerWordEmbeddings(model=tiny_dir, layers="all", pooling_operation=op, use_scalar_mix=True)
        assert m.embedding_length == (2 * H if op == "first_last" else H)
    with pytest.raises(ValueError) as ei:
        TransformerWordEmbeddings(model=tiny_dir, pooling_operation="max")
    assert all(repr(o) in str(ei.value) for o in pr.OPS)
    for op in ("last", "first_last", "mean"):                   # the fine-tuning path keeps refusing, and says who does take it
        with pytest.raises(NotImplementedError, match="pooling_operation='%s'.*[Ff]rozen.*stacked tagger" % op):
            TransformerWordEmbeddings(model=tiny_dir, pooling_operation=op, fine_tune=True)
    assert TransformerWordEmbeddings(model=tiny_dir, fine_tune=True).pooling_operation == "first"
    import inspect
    par = inspect.signature(TransformerWordEmbeddings.__init__).parameters
    assert par["pooling_operation"].default == "first" and par["layers"].default == "-1"


def test_width_limit_applies_to_the_doubled_width(monkeypatch, tiny_dir):
    import flair.embeddings as FE
    monkeypatch.setattr(FE, "MAX_EMBEDDING_WIDTH", 256)
    assert FE.TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation="mean").embedding_length == 256
    with pytest.raises(NotImplementedError, match="512"):
        FE.TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation="first_last")
    assert FE.TransformerWordEmbeddings(model=tiny_dir, layers="all", pooling_operation="first_last", use_scalar_mix=True).embedding_length == 256


# ---------------------------------------------------------------------- tables
TEXTS = ["alice visited \x01 berlin <EOS> the museum of art", "\x01 zalandoresearchuniversitycambridge is located in berlin \x02",
         "bob <EOS> wikipedia"]


@pytest.fixture(scope="module")
def wp_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("pool_host_wp")
    return tiny_assets.build_model_dir(os.path.join(str(d), "bert-tiny"), tokenizer="wordpiece", seed=3)


@pytest.mark.parametrize("kind", ["sp", "wp"])
def test_pool_batch_agrees_with_stack_batch(tiny_dir, wp_dir, kind):
    tiny_dir = tiny_dir if kind == "sp" else wp_dir
    from flair.data import Sentence
    from flair.embeddings import TransformerWordEmbeddings
    emb = TransformerWordEmbeddings(model=tiny_dir, pooling_operation="mean", maximum_subtoken_length=3)
    sents = [Sentence(t) for t in TEXTS]
    ids, am, first, lens, first_row = emb.prepare_stack_batch(sents)
    ids2, am2, lens2, span_ptr, span_loc = emb.prepare_pool_batch(sents)
    assert np.array_equal(ids, ids2) and np.array_equal(am, am2) and np.array_equal(lens, lens2)
    B, n = first.shape
    assert span_ptr.shape == (B * n + 1,) and span_ptr[0] == 0 and span_ptr[-1] == len(span_loc) and (np.diff(span_ptr) >= 0).all()
    m = np.diff(span_ptr).reshape(B, n)
    assert np.array_equal(m == 0, first < 0)
    if kind == "wp":                                                            # control-character words receive no sub-token
        assert [(first[b, :lens[b]] < 0).sum() for b in range(B)] == [1, 2, 0]
    assert m.max() == 3 and (m > 1).sum() >= 2                                  # multi-piece words, the long one clamped to 3
    for b in range(B):
        for t in range(n):
            if m[b, t]:
                lo = span_ptr[b * n + t]
                assert tuple(span_loc[lo]) == (first_row[b, t], first[b, t])
                row = span_loc[lo:lo + m[b, t]]
                assert (row[:, 0] == row[0, 0]).all() and np.array_equal(row[:, 1], row[0, 1] + np.arange(m[b, t]))   # one window: consecutive
    assert (am[span_loc[:, 0], span_loc[:, 1]] == 1).all()                      # every entry is a real sub-token
    # use_internal_doc: the encoder reads doc_sent, only the chunked sentence's tokens are pooled
    emb.use_internal_doc = True
    short = Sentence("alice visited berlin")
    short.doc_sent = Sentence("alice visited berlin <EOS> the museum of art")
    a = emb.prepare_stack_batch([short])
    b_ = emb.prepare_pool_batch([short])
    assert np.array_equal(a[0], b_[0]) and b_[3].shape == (4,) and np.array_equal(b_[4][b_[3][:-1], 1], a[2][0])


def test_pool_batch_takes_the_v2_doc_window(tiny_dir):
    """v2_doc: the same document window as prepare_stack_batch, spans of consecutive positions starting at its first sub-tokens"""
    from flair.data import Sentence
    from flair.embeddings import TransformerWordEmbeddings
    emb = TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation="last", v2_doc=True)
    doc = [Sentence(t) for t in ("alice visited zalandoresearch berlin", "the museum of art", "bob lives near cambridgeuniversity")]
    for i, s in enumerate(doc):
        s.doc, s.doc_pos = doc, i
    ids, am, first, lens, first_row = emb.prepare_stack_batch(doc)
    ids2, am2, lens2, span_ptr, span_loc = emb.prepare_pool_batch(doc)
    assert np.array_equal(ids, ids2) and np.array_equal(am, am2) and np.array_equal(lens, lens2)
    B, n = first.shape
    m = np.diff(span_ptr).reshape(B, n)
    assert np.array_equal(m == 0, first < 0) and (m > 1).any()
    for b in range(B):
        pos = None
        for t in range(int(lens[b])):
            row = span_loc[span_ptr[b * n + t]:span_ptr[b * n + t + 1]]
            assert (row[:, 0] == b).all() and row[0, 1] == first[b, t] and np.array_equal(row[:, 1], first[b, t] + np.arange(m[b, t]))
            assert pos is None or row[0, 1] == pos                               # the words tile the sentence's stretch of the window
            pos = row[-1, 1] + 1
    assert (am[span_loc[:, 0], span_loc[:, 1]] == 1).all()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_spans_astride_a_seam_equal_the_stitched_sequence(tiny_dir, seed):
    """hidden states that are random numbers: pooling them through the tables == pooling the reference's stitched sequence"""
    import tiny_assets
    from flair.data import Sentence
    from flair.embeddings import TransformerWordEmbeddings
    emb = TransformerWordEmbeddings(model=tiny_dir, pooling_operation="mean")
    emb.max_subtokens_sequence_length, emb.stride = 64, 32
    rng = np.random.default_rng(seed)
    words = ["".join(str(w) for w in rng.choice(tiny_assets.WORDS, size=2)) for _ in range(60)]      # two-word compounds: many pieces each
    s = Sentence(" ".join(words))
    ids, am, lens, span_ptr, span_loc = emb.prepare_pool_batch([Sentence("bob"), s])
    R, S0 = ids.shape
    assert R >= 3                                                               # 'bob' + at least two windows
    n = len(s)
    Hh = 8
    hidden = rng.standard_normal((2, R, S0, Hh))                                # two "layers"
    # the reference's stitching of the windows of sentence 1 (rows 1 .. R - 1), :3292-3299
    st = emb.stride
    row_len = am.sum(1)
    stitched = [hidden[:, 1, :row_len[1]]]
    for r in range(2, R):
        stitched = [np.concatenate([stitched[0][:, :-1 - st // 2], hidden[:, r, :row_len[r]][:, 1 + st // 2:]], axis=1)]
    stitched = stitched[0]
    pieces = emb.tokenizer.tokenize(" ".join(words))
    counts = emb.reconstruct_tokens_from_subtokens(list(s), pieces)
    assert stitched.shape[1] == sum(counts) + 2
    flat = span_loc[:, 0] * S0 + span_loc[:, 1]
    xs = [hidden[j].reshape(R * S0, Hh) for j in range(2)]
    astride = 0
    for op in pr.OPS:
        mine = pr.pool_layers(xs, span_ptr, flat, op, False)[n:2 * n]           # sentence 1's rows of the token-major matrix
        start = 1
        for t, c in enumerate(counts):
            cur = stitched[:, start:start + c]                                  # [layer, c, H]
            if op == "first":
                want = [l[0] for l in cur]
            elif op == "last":
                want = [l[-1] for l in cur]
            elif op == "first_last":
                want = [np.concatenate([l[0], l[-1]]) for l in cur]
            else:
                want = [l.mean(0) for l in cur]
            np.testing.assert_allclose(mine[t], np.concatenate(want), rtol=1e-12, atol=0, err_msg="%s word %d" % (op, t))
            start += c
    for t in range(n):
        rows = span_loc[span_ptr[n + t]:span_ptr[n + t + 1], 0]
        astride += len(set(rows.tolist())) > 1
    assert astride >= 1, "no word of this sentence lies astride a window seam"


# ---------------------------------------------------------------------- ops refusals
def test_ops_refuse_malformed_tables_before_any_launch(monkeypatch):
    from kbner import lib as L
    from kbner import ops

    def reached(*a, **k):
        raise AssertionError("a refused call reached the library")

    monkeypatch.setattr(L, "call", reached)
    srcs = [torch.zeros(20, 16, dtype=BF16), torch.zeros(24, 16, dtype=BF16)]
    out = torch.zeros(4, 64, dtype=BF16)
    sp, sr = np.asarray([0, 0, 2, 3, 3]), np.asarray([5, 19, 0])
    good = dict(srcs=srcs, span_ptr=sp, span_rows=sr, out2d=out, col=8, op="mean", layer_mean=False)

    def refused(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(L.KbnerError, match=match):
            ops.pool_rows_layers(a["srcs"], a["span_ptr"], a["span_rows"], a["out2d"], a["col"], a["op"], layer_mean=a["layer_mean"])

    refused("non-decreasing", span_ptr=np.asarray([0, 2, 1, 3, 3]))
    refused("non-decreasing", span_ptr=np.asarray([1, 1, 2, 3, 3]))
    refused("ends at", span_ptr=np.asarray([0, 0, 2, 3, 4]))
    refused("ends at", span_rows=np.asarray([5, 19]))
    refused(r"\[0, 20\)", span_rows=np.asarray([5, 20, 0]))                     # a row of the LONGER source only
    refused(r"\[0, 20\)", span_rows=np.asarray([5, -1, 0]))
    refused("HOST 1-d integer", span_ptr=sp.astype(np.float32))
    refused("HOST 1-d integer", span_rows=sr.reshape(1, 3))
    refused("out2d holds 4 rows", span_ptr=np.asarray([0, 0, 2, 3, 3, 3]))
    refused("multiple of 8", col=4)
    refused("multiple of 8", col=40)                                            # 40 + 32 > 64
    refused("multiple of 8", col=0, op="first_last", srcs=srcs + srcs[:1], layer_mean=False)      # 3 * 32 > 64
    refused("multiple of 8", out2d=torch.zeros(4, 60, dtype=BF16))
    refused("one of", op="max")
    refused("1 to 32", srcs=[])
    refused("1 to 32", srcs=srcs[:1] * 33)
    refused("bfloat16", srcs=[srcs[0], srcs[1].float()])
    refused("bfloat16", out2d=out.float())
    refused("bfloat16", srcs=[srcs[0], srcs[1][:, :8]])                         # not contiguous
    refused("one H", srcs=[srcs[0], torch.zeros(24, 24, dtype=BF16)])
    refused("one H", srcs=[torch.zeros(20, 12, dtype=BF16)])
    refused("cuda tensor")                                                      # well-formed, but host tensors: still no launch
    assert ops.pool_width("first_last", 4, 16) == 128 and ops.pool_width("mean", 4, 16, True) == 16


# ---------------------------------------------------------------------- the stacked tagger
def _stack_tagger(tiny_dir, specs, hidden_size=32):
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    embs = [TransformerWordEmbeddings(model=tiny_dir, embedding_name="e%d" % i, **kw) for i, kw in enumerate(specs)]
    return FastSequenceTagger(hidden_size=hidden_size, embeddings=StackedEmbeddings(embs), tag_dictionary=_dictionary(), tag_type="ner",
                              use_crf=True, use_rnn=True)


def test_build_stack_sizes_the_blocks_and_load_state_names_a_mismatch(tiny_dir):
    from flair.models import FastSequenceTagger
    H = 128
    tg = _stack_tagger(tiny_dir, [dict(layers="-1,-2", pooling_operation="mean"),
                                  dict(layers="all", pooling_operation="first_last", use_scalar_mix=True), dict()])
    assert tg._stack_blocks == [2 * H, 2 * H, H] and tg.stack_head.Dp >= 5 * H
    assert [FastSequenceTagger._plain_first(e) for e in tg._stack_embs] == [False, False, True]
    assert tuple(tg._stack_state["rnn"]["weight_ih_l0"].shape) == (4 * 32, 5 * H)
    # a state trained under another pooling / layer setting: refused by name, both widths in the message
    other = _stack_tagger(tiny_dir, [dict(layers="-1", pooling_operation="mean"), dict()])
    st = {k: v for k, v in other._stack_state.items()}
    with pytest.raises(ValueError, match=r"weight_ih_l0.*256.*640"):
        tg.load_stack_state(st)
    tg.load_stack_state({k: v for k, v in tg._stack_state.items()})             # its own state loads
    # fine_tune: true keeps the refusal of a layer selection under use_rnn
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    e = TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", fine_tune=True)
    with pytest.raises(NotImplementedError, match=r"use_rnn: true.*layers='-1,-2'"):
        FastSequenceTagger(hidden_size=32, embeddings=StackedEmbeddings([e]), tag_dictionary=_dictionary(), tag_type="ner", use_crf=True,
                           use_rnn=True)


def test_use_rnn_false_refuses_a_frozen_embedding_with_another_pooling(tiny_dir):
    """its engine pools the first sub-token and sizes the head k * H: a frozen embedding (a teacher, say) that asks for another pooling
    is refused by name before anything is built, never quietly pooled 'first'"""
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    for op in ("last", "first_last", "mean"):
        e = TransformerWordEmbeddings(model=tiny_dir, layers="-1,-2", pooling_operation=op)
        for embeddings in (StackedEmbeddings([e]), e):
            with pytest.raises(NotImplementedError, match=r"use_rnn: false.*pooling_operation='%s'.*stacked tagger" % op):
                FastSequenceTagger(hidden_size=32, embeddings=embeddings, tag_dictionary=_dictionary(), tag_type="ner", use_crf=True,
                                   use_rnn=False)
