"""GPU: head dropout (`dropout`) and locked dropout (`locked_dropout`) of the fine-tuning tagger end to end, on the tiny assets of
tests/tiny_assets.py: the engine in eval and training mode (masks replayable from the seed, applied to what the head reads, replayed
by the backward), the linear head's weight gradient, ModelFinetuner with both rates in the YAML, checkpoint round trip, one
multi-view run.  The kernels themselves: tests/test_gpu_headdrop_kernels.py; the host plumbing: tests/test_headdrop_cpu.py."""
import os

import numpy as np
import pytest
import torch
import yaml

import headdropref as hd
import rowref

pytestmark = pytest.mark.gpu

T_, START_, STOP_, X_ = 8, 6, 7, 3


@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    import tiny_assets
    d = tmp_path_factory.mktemp("headdrop_e2e")
    return tiny_assets.build_model_dir(os.path.join(str(d), "xlmr-tiny"))


def _engine(tiny_dir, rates=(0.0, 0.0), use_crf=True):
    """kbner.engine.Tagger with the tiny model's encoder weights and a seeded head; rates = (head_dropout, locked_dropout)"""
    import json
    from safetensors.torch import load_file
    from kbner import engine
    hc = json.load(open(os.path.join(tiny_dir, "config.json")))
    cfg = engine.EncoderConfig(vocab_size=hc["vocab_size"], hidden_size=hc["hidden_size"], num_hidden_layers=hc["num_hidden_layers"],
                               num_attention_heads=hc["num_attention_heads"], intermediate_size=hc["intermediate_size"],
                               max_position_embeddings=hc["max_position_embeddings"], hidden_dropout_prob=0.0,
                               attention_probs_dropout_prob=0.0)
    tg = engine.Tagger(cfg, T_, START_, STOP_)
    tg.init_random(seed=5)
    tg.load_hf_state_dict(load_file(os.path.join(tiny_dir, "model.safetensors")))
    tg.use_crf = use_crf
    tg.head_dropout, tg.locked_dropout = rates
    return tg


@pytest.fixture(scope="module")
def batch(tiny_dir):
    import json
    from kbner import batch as kb
    V = json.load(open(os.path.join(tiny_dir, "config.json")))["vocab_size"]
    hb = kb.synthetic_batch(3, 64, vocab=V, T=T_, x_idx=X_, start=START_, stop=STOP_, n_real=5, seed=9)
    return hb, kb.to_device(hb)


def test_eval_mode_is_unaffected(tiny_dir, batch):
    hb, db = batch
    a, b = _engine(tiny_dir, (0.1, 0.5)), _engine(tiny_dir, (0.0, 0.0))
    assert torch.equal(a.arena.p, b.arena.p)
    state = a._drop_rng.bit_generator.state
    ea, eb = a.eval().forward_features(db), b.eval().forward_features(db)
    la, lb = a.forward_loss(db, backward=False), b.forward_loss(db, backward=False)
    torch.cuda.synchronize()
    assert torch.equal(ea, eb) and torch.equal(la, lb) and torch.equal(a.last_emissions, b.last_emissions)
    assert a._drop_rng.bit_generator.state == state


def _one_sentence_batch(tiny_dir):
    """one 64-position sentence whose sub-tokens are all different ids: no two rows of the batch add into the same embedding row and
    the padded tail of the token dimension is zero, so every gradient of the step is a sum with ONE order -- the fp32 atomics of the
    embedding backward and of the split weight-gradient GEMMs cannot reorder anything, and arena.g is reproducible to the bit"""
    import json
    from kbner import batch as kb
    V = json.load(open(os.path.join(tiny_dir, "config.json")))["vocab_size"]
    S = 64
    assert V >= S + 3
    rng = np.random.default_rng(21)
    ids = np.concatenate([[0], 5 + rng.permutation(V - 5)[:S - 2], [2]])[None, :]
    n = S - 2
    first_idx = np.arange(1, S - 1)[None, :]
    tags = np.full((1, n), X_, np.int64)
    tags[0, :7] = rng.choice([0, 1, 2, 4, 5], size=7)
    hb = kb.assemble(ids, np.ones((1, S), np.int64), first_idx, tags, np.asarray([n]), X_)
    return hb, kb.to_device(hb)


def test_training_step_is_replayable_from_the_seed(tiny_dir, batch):
    """two forward_loss(backward=True) steps after the same seed_dropout(s): bit-identical loss and arena.g; another seed, another
    loss.  The whole arena on the one-sentence batch (see there); on the three-sentence batch the loss and the head's gradients
    (the sums that have one order whatever the batch)."""
    tg = _engine(tiny_dir, (0.1, 0.5)).train()
    tg.word_dropout = 0.1

    def step(db, seed):
        tg.seed_dropout(seed)
        tg.arena.g.zero_()
        loss = tg.forward_loss(db, backward=True)
        torch.cuda.synchronize()
        return loss.clone(), tg.arena.g.clone()

    hb1, db1 = _one_sentence_batch(tiny_dir)
    l1, g1 = step(db1, 31)
    l2, g2 = step(db1, 31)
    l3, _ = step(db1, 32)
    assert torch.isfinite(l1) and torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    assert float(l3) != float(l1)
    hb, db = batch
    l1, g1 = step(db, 41)
    l2, g2 = step(db, 41)
    l3, _ = step(db, 42)
    assert torch.equal(l1, l2) and float(l3) != float(l1)
    for name in ("linear.weight", "linear.bias"):
        k = tg.arena.offsets[name]
        m = int(np.prod(tg.arena.shapes[name]))
        assert torch.equal(g1[k:k + m], g2[k:k + m]) and float(g1[k:k + m].abs().max()) > 0, name


def _expected_stream(seed, n_pos, word_dropout):
    """what one training forward draws from the engine's stream, in the documented order (HF dropout off): word dropout, then
    the two head-dropout seeds"""
    rng = np.random.default_rng(seed)
    dropped = rng.random(n_pos) < word_dropout if word_dropout > 0 else np.zeros(n_pos, bool)
    sd = rng.integers(0, 2 ** 32, size=2, dtype="uint64")
    return dropped, int(sd[0]), int(sd[1])


def test_masks_reach_the_head(tiny_dir, batch):
    """training mode: engine.last_pooled == the reference gather of the encoder output under the seeds the engine drew (word dropout
    first: its rows are index -1), within the bound of the REAL kernel cases"""
    from kbner import ops
    hb, db = batch
    tg = _engine(tiny_dir, (0.1, 0.5)).train()
    tg.word_dropout = 0.2
    tg.seed_dropout(77)
    tg.forward_loss(db, backward=False)
    torch.cuda.synchronize()
    B, S, nc = hb["B"], hb["S"], hb["ctags"].shape[1]
    L = tg.cfg.num_hidden_layers
    hidden = tg.acts(B, S).x[L].float().cpu().numpy().astype(np.float64)
    dropped, se, sl = _expected_stream(77, int(hb["n_tokens"]), 0.2)
    assert np.array_equal(dropped, tg._last_word_dropped) and dropped.any()
    crow, cpos = hb["crow_idx"].astype(np.int64), hb["cpos"].astype(np.int64)
    crow = np.where((cpos >= 0) & dropped[np.maximum(cpos, 0)], -1, crow)
    de, dl = (se, ops.drop_thresh(0.1)), (sl, ops.drop_thresh(0.5))
    ref = hd.gather(hidden, crow, nc, de, dl)
    got = tg.last_pooled.float().cpu().numpy().astype(np.float64).reshape(B * nc, -1)
    ke, kl = hd.keep(B * nc, ref.shape[1], nc, de, dl)
    dead = ~(ke & kl & (crow >= 0)[:, None])
    assert (got[dead] == 0).all() and (got[~dead] != 0).mean() > 0.99
    bound = hd.real_bound(ref)
    diff = np.abs(got - ref)
    print("[headdrop] last_pooled: worst share of the bound %.3f" % float((diff[bound > 0] / bound[bound > 0]).max()))
    assert (diff <= bound).all()
    # the locked mask really is shared by a sentence's rows: a column dead in one live row of a sentence is dead in all of them
    assert (kl.reshape(B, nc, -1) == kl.reshape(B, nc, -1)[:, :1]).all()


def test_linear_weight_gradient_and_replayed_scatter(tiny_dir, batch):
    """a hand-built d loss / d emissions through _backprop_emissions: linear.weight's gradient is demit^T . last_pooled (the masked
    rows the head read) within rowref.tolerance for head_bwd_dw, and the gradient that reaches the encoder rows is the reference
    scatter of the head's dX under the SAME seeds (compared through the kernel's own dX)"""
    from kbner import ops
    hb, db = batch
    tg = _engine(tiny_dir, (0.1, 0.5), use_crf=False).train()
    tg.seed_dropout(13)
    em, pooled, crow_idx, B, nc, R, S, drop = tg._emit(db)
    assert drop is not None and drop[0][1] == ops.drop_thresh(0.1) and drop[1][1] == ops.drop_thresh(0.5)
    rng = np.random.default_rng(4)
    demit = (0.1 * rng.standard_normal((B, nc, T_))).astype(np.float32)
    seen = {}
    monkey = tg.encoder_backward
    tg.encoder_backward = lambda dx, grad_ready=None: seen.setdefault("dx", dx.clone())
    try:
        tg.arena.g.zero_()
        tg._backprop_emissions(torch.from_numpy(demit).cuda(), pooled, crow_idx, B, nc, R, S, None, drop=drop)
    finally:
        tg.encoder_backward = monkey
    torch.cuda.synchronize()
    x64 = pooled.float().cpu().numpy().astype(np.float64)
    de = demit.reshape(B * nc, T_)
    ref = de.astype(np.float64).T @ x64
    tol, err32 = rowref.tolerance(ref, rowref.seq_dot32(de.T, x64.T), np.abs(de.astype(np.float64)).T @ np.abs(x64))
    got = tg.arena.grad("linear.weight").cpu().numpy().astype(np.float64)
    diff = np.abs(got - ref)
    print("[headdrop] d linear.weight: worst error %.3e, share of the tolerance %.3f" % (float(diff.max()), float((diff / tol).max())))
    assert (diff <= tol).all()
    # the scatter replays the forward's masks: rows of dx = reference scatter of the head's dX
    w = tg.arena.param("linear.weight")
    dpooled = ops.head_bwd(torch.from_numpy(de).cuda(), pooled, w, torch.zeros_like(w), torch.zeros(T_, device="cuda"))
    dref = hd.scatter(dpooled.float().cpu().numpy().astype(np.float64), crow_idx.cpu().numpy(), seen["dx"].shape[0], nc, drop[0], drop[1])
    dgot = seen["dx"].float().cpu().numpy().astype(np.float64)
    assert (np.abs(dgot - dref) <= hd.real_bound(dref)).all() and np.abs(dref).max() > 0


def _yaml_student(tmp_path, cfg):
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    cp = ConfigParser(Params.from_file(str(tmp_path / "cfg.yaml")))
    return cp, cp.create_student()


def test_finetuner_trains_saves_and_resumes(tmp_path):
    """dropout: 0.1, locked_dropout: 0.5 in the YAML: ModelFinetuner trains 2 epochs with finite losses; best-model.pt and
    checkpoint.pt carry both rates; a restart from the checkpoint continues (the dropout stream is part of it) for a third epoch"""
    import tiny_assets
    from flair.models import FastSequenceTagger
    from flair.trainers import ModelFinetuner
    torch.manual_seed(2)
    cfg = tiny_assets.e2e_config(str(tmp_path), word_dropout=0.05, max_epochs=2, n_train=16, n_dev=4, n_test=4)
    cfg["model"]["FastSequenceTagger"].update(dropout=0.1, locked_dropout=0.5)
    cp, student = _yaml_student(tmp_path, cfg)
    assert (student.engine.head_dropout, student.engine.locked_dropout) == (0.1, 0.5)
    drawn = []
    hd_draw = student.engine._head_drop
    student.engine._head_drop = lambda: drawn.append(hd_draw()) or drawn[-1]
    trainer = ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    train_kw = dict(cp.config["train"], checkpoint=True)
    out = trainer.train(cp.get_target_path, **train_kw)
    hist = out["train_loss_history"]
    assert len(hist) == 2 and all(np.isfinite(x) and x > 0 for x in hist), hist
    assert drawn and all(d is not None for d in drawn)                 # every training forward took the dropout gather
    base = cp.get_target_path
    again = FastSequenceTagger.load(base / "best-model.pt")
    assert (again.use_dropout, again.use_locked_dropout, again.engine.head_dropout, again.engine.locked_dropout) == (0.1, 0.5, 0.1, 0.5)
    ck = FastSequenceTagger.load_checkpoint(base / "checkpoint.pt")
    assert ck["epoch"] == 2
    m = ck["model"]
    assert (m.engine.head_dropout, m.engine.locked_dropout) == (0.1, 0.5)
    tr2 = ModelFinetuner.load_from_checkpoint(ck, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    out2 = tr2.train(base, **dict(train_kw, max_epochs=3))
    assert m.engine._drop_rng.bit_generator.state != np.random.default_rng(0).bit_generator.state
    h2 = out2["train_loss_history"]
    assert len(h2) == 1 and np.isfinite(h2[0]) and h2[0] > 0, h2


def test_multiview_run_with_both_rates(tmp_path):
    """multi_view_training + distill_posterior with remove_x and both rates on: two forwards and two backwards per step, each
    backward replaying its own forward's masks; every NLL and every second-view term is finite"""
    import tiny_assets
    from flair.trainers import ModelFinetuner
    torch.manual_seed(3)
    cfg = tiny_assets.multiview_config(str(tmp_path), max_epochs=1, accum=1, mini_batch_size=2, temperature=2.0, n_train=6, n_dev=2,
                                       n_test=2)
    cfg["model"]["FastSequenceTagger"].update(dropout=0.1, locked_dropout=0.5)
    cp, student = _yaml_student(tmp_path, cfg)
    assert student.multi_view_training and student.remove_x and student.engine.locked_dropout == 0.5
    trainer = ModelFinetuner(student, None, cp.corpus, config=cp.config, **cp.config["ModelFinetuner"])
    parts = []
    fb = student.forward_backward

    def spy(data_points, *a, **k):
        out = fb(data_points, *a, **k)
        nll, kd = student.last_loss_parts
        parts.append((float(nll), None if kd is None else float(kd)))
        return out

    student.forward_backward = spy
    out = trainer.train(cp.get_target_path, **cp.config["train"])
    kds = [kd for _, kd in parts if kd is not None]
    assert kds and all(np.isfinite(x) and x >= 0 for x in kds) and all(np.isfinite(n) for n, _ in parts), parts
    assert all(np.isfinite(x) for x in out["train_loss_history"])
