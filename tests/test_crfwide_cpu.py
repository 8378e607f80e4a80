"""CPU: what the wide-tag-set feature (65 to 192 tags) rests on without a GPU.

  - the case list of tests/crfwide_cases.py: on every case with n > 1 the tie inputs do tie (>= 25 % of the Viterbi cells and at
    least one terminal), and on every case float32 and float64 Viterbi agree on tags and popped, for the real and for the tie
    inputs -- so the bit-exact comparison of tests/test_gpu_crf_wide_kernels.py is neither vacuous nor a coin toss;
  - kbner.ops dispatches on the tag count: T <= 64 calls the single-wave entry points, T > 64 the kbner_crf_wide_* ones (recorded
    from a stub of lib.call; no kernel runs);
  - FastSequenceTagger accepts a CRF tagger over 137 and 192 tags, and refuses by name, in the constructor, what has single-wave
    kernels only (softmax head, multi-view training, the distill_* switches), more than 192 tags, and teacher labelling by a wide
    teacher.  The constructor is reached the way tests/test_headdrop_cpu.py reaches it (tiny model, engine on the CPU device).
"""
import os
import types

import numpy as np
import pytest
import torch

import crfref
import crfwide_cases

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


# ---------------------------------------------------------------------- the case list
def test_case_list_is_the_issue_s():
    assert len(crfwide_cases.WIDE) == 29 and len(set(crfwide_cases.WIDE)) == 29
    assert sorted({c[0] for c in crfwide_cases.WIDE}) == [65, 96, 127, 128, 129, 137, 160, 191, 192]
    assert all(65 <= c[0] <= 192 and 0 <= c[1] < c[0] and 0 <= c[2] < c[0] and c[1] != c[2] for c in crfwide_cases.WIDE)
    assert not any(crfref.grid_id(c) in crfref.TIE_SALT for c in crfwide_cases.WIDE)
    assert [c[0] for c in crfwide_cases.NARROW] == [3, 29, 33, 64]


@pytest.mark.parametrize("case", crfwide_cases.WIDE, ids=crfref.grid_id)
def test_case_ties_and_float32_agrees_with_float64(case):
    x = crfref.grid_inputs(case)
    s = (x["start"], x["stop"])
    sets = [("real", x["emit"], x["trans"], x["lens"])]
    if x["n"] > 1:
        assert x["tie_emit"] is not None
        share, terminal = crfref.tie_stats(x["tie_emit"], x["tie_trans"], x["tie_lens"], *s)
        print("[crfwide] %s: tied cells %.3f, tied terminals %d" % (crfref.grid_id(case), share, terminal))
        assert share >= 0.25 and terminal >= 1
        sets.append(("tie", x["tie_emit"], x["tie_trans"], x["tie_lens"]))
    for name, emit, trans, lens in sets:
        t32, _, p32 = crfref._oracle_viterbi(emit, trans, lens, *s)
        t64, _, p64 = crfref.viterbi(emit, trans, lens, *s, dtype=np.float64)
        assert np.array_equal(t32, t64) and np.array_equal(p32, p64), name


# ---------------------------------------------------------------------- ops: dispatch on the tag count
def test_ops_dispatch_by_tag_count(monkeypatch):
    from kbner import ops
    calls = []
    monkeypatch.setattr(ops.L, "call", lambda name, *a: calls.append((name, len(a))))
    monkeypatch.setattr(ops, "_chk", lambda t, dtype, name: None)
    monkeypatch.setattr(ops, "stream_ptr", lambda: None)
    B, n = 2, 3
    for T, pre in ((64, "kbner_crf_"), (65, "kbner_crf_wide_"), (192, "kbner_crf_wide_"), (29, "kbner_crf_")):
        del calls[:]
        emit, trans = torch.zeros(B, n, T), torch.zeros(T, T)
        tags, lens = torch.zeros(B, n, dtype=I32), torch.full((B,), n, dtype=I32)
        ops.crf_viterbi(emit, trans, lens, 0, 1, want_popped=True)
        logz, gold, alpha = ops.crf_nll_fwd(emit, trans, tags, lens, 0, 1)
        ops.crf_nll_bwd(emit, trans, tags, lens, alpha, logz, torch.ones(B), 0, 1, torch.zeros(T, T))
        ops.crf_posterior(emit, trans, lens, 0, 1)
        wide = pre.endswith("wide_")
        assert calls == [(pre + "viterbi", 13 if wide else 12), (pre + "nll_fwd", 13), (pre + "nll_bwd", 15),
                         (pre + "nll_fwd", 13), (pre + "posterior", 12)], (T, calls)
    assert (ops.CRF_NARROW_MAXT, ops.CRF_WIDE_MAXT) == (64, 192)


def test_wide_workspace_size_is_a_host_function():
    from kbner import lib
    f = lib.load().kbner_crf_wide_viterbi_ws_bytes
    assert f(0, 7, 137) == 0 and f(3, 0, 137) == 0
    assert f(2, 300, 192) >= 2 * 300 * 192 * 5 and f(2, 300, 192) % 16 == 0


# ---------------------------------------------------------------------- the flair surface
@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("crfwide")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def wide_dictionary(n_types):
    """<unk>, O, the BIES tags of n_types entity types, S-X, <START>, <STOP>: 4 * n_types + 5 items (33 types: 137)"""
    from flair.data import Dictionary
    td = Dictionary(add_unk=True)
    td.add_item("O")
    for k in range(n_types):
        for p in "BIES":
            td.add_item("%s-T%02d" % (p, k))
    for t in ("S-X", "<START>", "<STOP>"):
        td.add_item(t)
    assert len(td) == 4 * n_types + 5
    return td


def _cpu_tagger(monkeypatch, tiny_dir, td, **kw):
    import flair
    from flair.embeddings import StackedEmbeddings, TransformerWordEmbeddings
    from flair.models import FastSequenceTagger
    from kbner import ops
    monkeypatch.setattr(flair, "device", torch.device("cpu"))
    monkeypatch.setattr(ops, "f32_to_bf16", lambda x, y: y.copy_(x.to(BF16)))
    monkeypatch.setattr(ops, "bf16_to_f32", lambda x, y: y.copy_(x.float()))
    emb = TransformerWordEmbeddings(model=tiny_dir, layers="-1", pooling_operation="first", fine_tune=True)
    args = dict(hidden_size=256, embeddings=StackedEmbeddings([emb]), tag_dictionary=td, tag_type="ner", use_crf=True, use_rnn=False,
                remove_x=True, sentence_loss=True)
    args.update(kw)
    return FastSequenceTagger(**args)


def test_constructor_accepts_wide_crf_taggers(monkeypatch, tiny_dir):
    for n_types, kw in ((33, {}), (33, dict(predict_posterior=True)), (18, {}), (15, {})):
        td = wide_dictionary(n_types)
        tg = _cpu_tagger(monkeypatch, tiny_dir, td, **kw)
        assert tg.tagset_size == len(td) == tg.engine.T
        assert tuple(tg.engine.arena.param("transitions").shape) == (len(td), len(td))
        assert tuple(tg.engine.arena.param("linear.weight").shape)[0] == len(td)
    from flair.data import Dictionary
    td = Dictionary(add_unk=False)
    for k in range(190):
        td.add_item("t%d" % k)
    td.add_item("<START>")
    td.add_item("<STOP>")
    assert _cpu_tagger(monkeypatch, tiny_dir, td, remove_x=False).tagset_size == 192      # the limit itself


@pytest.mark.parametrize("switch,kw,limit", [
    ("use_crf=False", dict(use_crf=False), 64),
    ("multi_view_training", dict(multi_view_training=True, distill_posterior=True, temperature=2.0), 32),
    ("distill_crf", dict(distill_crf=True), 32),
    ("distill_posterior", dict(distill_posterior=True), 32),
    ("distill_exact", dict(distill_exact=True), 32),
    ("distill_emission", dict(distill_emission=True), 64),
])
def test_constructor_refuses_the_narrow_paths_by_name(monkeypatch, tiny_dir, switch, kw, limit):
    import re
    with pytest.raises(NotImplementedError, match=r"%s with a tag dictionary of 137 items.* %d tags" % (re.escape(switch), limit)):
        _cpu_tagger(monkeypatch, tiny_dir, wide_dictionary(33), **kw)
    # the same switch on 61 tags is none of this feature's business: whatever the constructor did before, it does now
    try:
        _cpu_tagger(monkeypatch, tiny_dir, wide_dictionary(14), **kw)
    except NotImplementedError as e:
        assert "tag dictionary of" not in str(e)


def test_constructor_refuses_more_than_192_tags(monkeypatch, tiny_dir):
    with pytest.raises(NotImplementedError, match=r"197 items.*192"):
        _cpu_tagger(monkeypatch, tiny_dir, wide_dictionary(48))


def test_teacher_labelling_refuses_a_wide_teacher():
    from flair.trainers.finetune_trainer import ModelFinetuner
    td = wide_dictionary(33)
    teacher = types.SimpleNamespace(tag_dictionary=td, eval=lambda: None)
    me = types.SimpleNamespace(corpus=types.SimpleNamespace(targets=["x"]), model=types.SimpleNamespace(tag_dictionary=td))
    with pytest.raises(NotImplementedError, match=r"137 items.*64 tags"):
        ModelFinetuner.assign_pretrained_teacher_targets(me, [[]], [teacher])
