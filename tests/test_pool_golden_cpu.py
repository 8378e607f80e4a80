"""CPU: the host half of the sub-token pooling against the RUNNING reference (tests/golden/pooling_ops.npz, captured by
tools/gen_golden_pooling_ops.py): for a sentencepiece-style and a BERT-style tokenizer, on the crafted texts of G7 (word tokens the
tokenizer drops, a long word clamped by maximum_subtoken_length, <EOS>), the mirror's ids / mask equal the reference's, and
tests/poolref.py applied to the reference's own hidden states through the mirror's span tables reproduces the reference's features
-- first / last / first_last / mean, layers='-1,-2', use_scalar_mix off and on -- to float32 rounding, zero vectors included.

THE BOUND GOES BEYOND rtol 1e-6 for `mean` and `use_scalar_mix`, and only for them.  The reference adds in float32 there, so its own
value carries up to (m + k + 4) * 2^-24 of the pooled |x| (the float32 term of poolref.bound, derived there); where the sum cancels,
that error is not small against the RESULT and rtol of the result alone cannot hold.  With rtol 1e-6 alone 7 (sp mean), 8 (sp mean +
mix) and 1 (wp mean) elements miss, by at most 9e-9 (largest absolute error 1.6e-7 on values of order 1); a wrong table would be off
by O(1).  first / last / first_last without the mix keep the pure rtol 1e-6 (they are in fact exact)."""
import os

import numpy as np
import pytest

import poolref as pr

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def model_dirs(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("pool_golden")
    return {"sp": tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny")),
            "wp": tiny_assets.build_model_dir(os.path.join(str(d), "bert-tiny"), tokenizer="wordpiece", seed=3)}


@pytest.mark.parametrize("mix", [False, True], ids=["cat", "mix"])
@pytest.mark.parametrize("op", pr.OPS)
@pytest.mark.parametrize("kind", ["sp", "wp"])
def test_tables_reproduce_the_reference_features(model_dirs, kind, op, mix):
    from flair.data import Sentence
    from flair.embeddings import TransformerWordEmbeddings
    z = np.load(os.path.join(GOLD, "pooling_ops.npz"))
    g = {k[3:]: z[k] for k in z.files if k.startswith(kind + "/")}
    feats = g["feat/%s/%s" % (op, "mix" if mix else "cat")]
    emb = TransformerWordEmbeddings(model=model_dirs[kind], layers="-1,-2", pooling_operation=op, use_scalar_mix=mix,
                                    maximum_subtoken_length=int(g["maximum_subtoken_length"]))
    sents = [Sentence(str(t)) for t in g["texts"]]
    assert [len(s) for s in sents] == g["n_tokens"].tolist()
    ids, am, lengths, span_ptr, span_loc = emb.prepare_pool_batch(sents)
    np.testing.assert_array_equal(ids, g["ids"])
    np.testing.assert_array_equal(am, g["mask"])
    hidden = g["hidden"].astype(np.float64)                      # [L + 1, B, S, H]
    Lp1, B, S, H = hidden.shape
    n = feats.shape[1]
    assert feats.shape == (B, n, emb.embedding_length) and span_ptr.size == B * n + 1
    xs = [hidden[li].reshape(B * S, H) for li in emb.layer_indexes]
    mine = pr.pool_layers(xs, span_ptr, span_loc[:, 0] * S + span_loc[:, 1], op, mix).reshape(B, n, -1)
    # float32 rounding: rtol 1e-6 of the feature; where the reference ADDS in float32 (mean, use_scalar_mix) its own value carries up
    # to (m + k + 4) * 2^-24 of the pooled |x| (poolref.bound's float32 term), which a sum that cancels does not hide behind rtol
    flat_rows = span_loc[:, 0] * S + span_loc[:, 1]
    slack = 0.0 if pr.is_copy(op, mix) else (pr.bound(0 * mine.reshape(B * n, -1), pr.pool_abs(xs, span_ptr, flat_rows, op, mix), span_ptr,
                                                      len(xs))).reshape(mine.shape)
    err = np.abs(mine - feats.astype(np.float64))
    assert (err <= 1e-6 * np.abs(feats) + slack).all(), float((err - 1e-6 * np.abs(feats) - slack).max())
    m = pr.span_lengths(span_ptr).reshape(B, n)
    zero = np.abs(feats).sum(-1) == 0
    assert np.array_equal(zero, m == 0)                          # zero vectors exactly where a span is empty (dropped words, padding)
    dropped = [int((m[b, :int(lengths[b])] == 0).sum()) for b in range(B)]
    # (sp: the soft-hyphen word is deleted by the normaliser but keeps a lone metaspace piece; wp: control characters leave nothing)
    assert dropped == ([0, 0, 0] if kind == "sp" else [1, 2, 0])
    assert m.max() == int(g["maximum_subtoken_length"])          # the clamped long word is in there
