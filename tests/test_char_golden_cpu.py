"""CPU: FastCharacterEmbeddings' host code and tests/charref.py against tests/golden/char_embeddings.npz, which tools/gen_golden_char.py
captured by running the REFERENCE's FastCharacterEmbeddings and ColumnDataLoader._get_char_idx: the dictionary, the character tables of
a batch, the features and the gradient of a fixed weighted sum with respect to every parameter."""
import os

import numpy as np
import pytest

import charref as C

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "char_embeddings.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def mine(gold):
    from flair.data import Sentence
    from flair.embeddings import FastCharacterEmbeddings
    emb = FastCharacterEmbeddings(vocab=[str(w) for w in gold["vocab"]])
    sents = [Sentence(str(t)) for t in gold["texts"]]
    n = max(len(s) for s in sents)
    return emb, sents, n, emb.char_batch(sents, n)


def test_dictionary_name_and_width(gold, mine):
    emb = mine[0]
    assert list(emb.char_dictionary.keys()) == [str(c) for c in gold["dict_items"]]
    assert list(emb.char_dictionary.values()) == gold["dict_ids"].tolist()
    assert emb.name == str(gold["name"]) and emb.embedding_length == int(gold["embedding_length"]) == 50
    assert {k: tuple(v.shape) for k, v in emb.state_dict().items()} == {k[6:]: gold[k].shape for k in gold.files if k.startswith("state/")}


def test_char_batch_is_get_char_idx_at_the_real_words(gold, mine):
    emb, sents, n, (chars, lens, rows) = mine
    seqs, lengths = gold["char_seqs"], gold["char_lengths"]                 # [Lmax, B * n], [B * n]
    assert chars.shape[1] == seqs.shape[0] and rows.tolist() == [b * n + k for b, s in enumerate(sents) for k in range(len(s))]
    assert (chars == seqs[:, rows].T).all() and (lens == lengths[rows]).all()
    assert (chars == 0).any() and (lens == 1).any()                          # unknown characters, a one-character word
    pad = np.setdiff1d(np.arange(len(sents) * n), rows)                     # the reference feeds '<u>' with length 1 at the padding;
    assert len(pad) and (lengths[pad] == 1).all() and not seqs[:, pad].any()  # this stack gives those positions no entry: zero rows


def test_reference_features_and_gradients(gold, mine):
    emb, sents, n, (chars, lens, rows) = mine
    st = {k[6:]: gold[k].astype(np.float64) for k in gold.files if k.startswith("state/")}
    p = C.NS(emb=st["char_embedding.weight"], wih=np.stack([st["char_layer.weight_ih_l0" + s] for s in C.SFX]),
             whh=np.stack([st["char_layer.weight_hh_l0" + s] for s in C.SFX]), bih=np.stack([st["char_layer.bias_ih_l0" + s] for s in C.SFX]),
             bhh=np.stack([st["char_layer.bias_hh_l0" + s] for s in C.SFX]))
    B = len(sents)
    feats, G = gold["features"].reshape(B * n, -1), gold["G"].reshape(B * n, -1)
    r = C.evaluate(p, chars, lens, rows, dout=G[rows])
    assert np.abs(r.h - feats[rows]).max() < 2e-6                            # (the golden features are float32)
    want = {"d_emb": gold["grad/char_embedding.weight"]}
    for name, key in (("d_wih", "weight_ih_l0"), ("d_whh", "weight_hh_l0"), ("d_bih", "bias_ih_l0"), ("d_bhh", "bias_hh_l0")):
        want[name] = np.stack([gold["grad/char_layer." + key + s] for s in C.SFX])
    for name, g in want.items():
        assert np.abs(getattr(r, name) - g).max() < 2e-6 * max(1.0, np.abs(g).max()), name
    # the class's own state dict has the golden's names: loading it into the device arena's layout is name for name
    from kbner.stack import CharBiLSTM
    net = CharBiLSTM({k: gold["state/" + k] for k in st}, "cpu")
    assert np.array_equal(net.param("wih").numpy(), p.wih.astype(np.float32)) and np.array_equal(net.param("emb").numpy(), p.emb.astype(np.float32))
    assert all(np.array_equal(v.numpy(), gold["state/" + k]) for k, v in net.state().items())
