"""GPU, end to end: Tagger.HEAD_ROWS_ONLY -- the last encoder layer computed on the rows the tagger head reads -- against the full
path.  Two taggers with the same seed, the switch on and off, run the same micro-batch (uneven kept counts per sentence, with and
without WordDropout, hidden / attention dropout 0 and 0.1: the same stream of draws, hence the same masks on both paths).

The yardstick is the full path's OWN distance to the oracle (fp32 autograd, fed the masks the kernels drew) for the same tensor:
for the loss, the emissions, the pooled rows and every gradient tensor the distance new-vs-full must not exceed full-vs-oracle --
no extra margin.  The two paths round the same values (the few-query kernels take the maxima, the probability arithmetic and the
softmax correction D exactly as the full kernels of the shape do) and differ in the order of fp32 sums: inside one attention call
and in the last layer's weight gradients.  Ratios on the MI355X run that accompanied this module (printed, run with -s): below
1e-4 at H = 128 without dropout (no bf16 value differs), 0.02 - 0.16 with it, worst 0.50 at H = 1024 (layer 0's query / key
weights).  selftest.check_step
itself must pass at its existing thresholds with the switch at its default (on), dropout included: that pins the masks."""
import numpy as np
import pytest
import torch

import selftest
from kbner import batch as kb
from kbner import engine, ops
from selftest import DEV, rel_l2

pytestmark = pytest.mark.gpu

T, START, STOP, X_IDX = 29, 27, 28, 9
SMALL = dict(L=2, H=128, A=2, F_=256, S=128, B=3, V=512)
LARGE = dict(L=2, H=1024, A=16, F_=4096, S=512, B=2, V=512)
# enough heads (B * A = 512 at S = 256) for the full path to take its 32-row attention kernels, as the benchmark shape does: the
# few-query kernels then run their two-part forward and their fused backward arithmetic (csrc/attn_rows.hip)
ROUTES = dict(L=2, H=512, A=8, F_=1024, S=256, B=64, V=512)
CONFIGS = {"small": SMALL, "large": LARGE, "routes": ROUTES}


def uneven_batch(B, S, V, n_real=7, seed=5):
    """synthetic sentences whose kept (non-X) token counts differ: sentence b has some of its real tokens re-tagged X"""
    ids, am, first_idx, tags, lengths = kb.synthetic_sentences(B, S, vocab=V, T=T, x_idx=X_IDX, start=START, stop=STOP, n_real=n_real, seed=seed)
    for b in range(B):
        tags[b, 1:1 + (2 * b + 1) % n_real:2] = X_IDX
    b_ = kb.assemble(ids, am, first_idx, tags, lengths, X_IDX)
    assert len(set(int(c) for c in b_["clens"])) > 1
    return b_


def make_tagger(c, head_rows_only, **kw):
    cfg = engine.EncoderConfig(vocab_size=c["V"], hidden_size=c["H"], num_hidden_layers=c["L"], num_attention_heads=c["A"],
                               intermediate_size=c["F_"], max_position_embeddings=c["S"] + 2)
    tg = engine.Tagger(cfg, T, START, STOP, device=DEV, head_rows_only=head_rows_only, **kw)
    tg.init_random(seed=5, std=0.08 if c["H"] == 128 else 0.02)
    return cfg, tg


def run_step(tg, bd, dropout, word_dropout):
    if dropout or word_dropout:
        tg.train(True)
        tg.word_dropout = word_dropout
        if not dropout:
            tg.cfg.hidden_dropout_prob = tg.cfg.attention_probs_dropout_prob = 0.0
        tg.seed_dropout(7)
    loss = tg.forward_loss(bd, loss_scale=1.0, backward=True)
    torch.cuda.synchronize()
    return float(loss)


def oracle_step(cfg, tg_full, b, dropout, word_dropout):
    """loss, kept-token emissions, pooled rows and gradients of the fp32 autograd oracle under the masks tg_full's step drew"""
    from oracle import encoder as oenc
    from oracle import train_step as ots
    masks = selftest.dropout_masks_of(tg_full, b["B"], b["S"]) if dropout else None
    word_keep = torch.from_numpy(~tg_full._last_word_dropped) if word_dropout else None
    ocfg = oenc.EncoderConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                              num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                              max_position_embeddings=cfg.max_position_embeddings)
    params = {k: v.clone().requires_grad_(True) for k, v in selftest.oracle_params(tg_full).items()}
    ob = dict(input_ids=torch.from_numpy(b["input_ids"]), attention_mask=torch.from_numpy(b["attention_mask"]),
              first_idx=torch.from_numpy(b["first_idx"]), tags=torch.from_numpy(b["tags"].astype(np.int64)),
              lengths=torch.from_numpy(b["lengths"].astype(np.int64)))
    oloss, oem = ots.tagger_forward_loss(params, ocfg, ob, START, STOP, X_IDX, masks=masks, word_keep=word_keep)
    oloss.backward()
    with torch.no_grad():
        hid = oenc.encoder_forward(params, ocfg, ob["input_ids"], ob["attention_mask"], masks=masks)
    B, nc = b["B"], b["ctags"].shape[1]
    em = torch.zeros(B, nc, T)
    pooled = torch.zeros(B, nc, cfg.hidden_size)
    crow, cpos = b["crow_idx"].reshape(B, nc), b["cpos"].reshape(B, nc)
    for r in range(B):
        for j in range(int(b["clens"][r])):
            em[r, j] = oem.detach()[r, cpos[r, j]]
            if word_keep is None or bool(word_keep[cpos[r, j]]):
                pooled[r, j] = hid[r, crow[r, j] - r * b["S"]]
    return float(oloss.detach()), em, pooled, params


def valid_rows(b):
    B, nc = b["B"], b["ctags"].shape[1]
    return torch.from_numpy(np.arange(nc)[None, :] < b["clens"][:, None])


@pytest.mark.parametrize("cfgname,dropout,word_dropout",
                         [(c, d, w) for c in ("small", "large") for d, w in ((False, 0.0), (True, 0.0), (True, 0.3), (False, 0.3))]
                         + [("routes", False, 0.0), ("routes", True, 0.3)])
def test_head_rows_step_is_the_full_step(cfgname, dropout, word_dropout):
    import mmaref
    c = CONFIGS[cfgname]
    assert (mmaref.pick_rpw(c["B"], c["S"], c["A"]) % 256 == 0) == (cfgname == "routes")
    b = uneven_batch(c["B"], c["S"], c["V"])
    bd = kb.to_device(b, DEV)
    cfg, tg_new = make_tagger(c, True)
    _, tg_full = make_tagger(c, False)
    loss_new = run_step(tg_new, bd, dropout, word_dropout)
    loss_full = run_step(tg_full, bd, dropout, word_dropout)
    assert tg_new.last_path == "head_rows" and tg_full.last_path == "full"
    if word_dropout:
        assert np.array_equal(tg_new._last_word_dropped, tg_full._last_word_dropped)
    L, B, S, nc = c["L"], c["B"], c["S"], b["ctags"].shape[1]
    # ac.x[L] at the head's rows holds the undropped pooled rows exactly (head dropout is off: last_pooled IS the gathered rows)
    crow = tg_new._rows_saved[0].row_ids[:B * nc].long()     # the rows the step read (WordDropout's -1 entries included)
    assert bool((crow >= 0).any()) and bool(((crow < 0) | (crow == bd["crow_idx"].long())).all())
    xl = tg_new.acts(B, S).x[L]
    live = crow >= 0
    assert torch.equal(xl[crow[live]], tg_new.last_pooled.reshape(B * nc, -1)[live])
    assert not tg_new.last_pooled.reshape(B * nc, -1)[~live].any()
    oloss, oem, opooled, oparams = oracle_step(cfg, tg_full, b, dropout, word_dropout)
    v = valid_rows(b)
    rows = []

    def compare(name, new, full, orc):
        d_nf, d_fo = rel_l2(new, full), rel_l2(full, orc)
        rows.append((d_nf / d_fo if d_fo > 0 else (0.0 if d_nf == 0 else float("inf")), d_nf, d_fo, name))

    rows.append((abs(loss_new - loss_full) / abs(loss_full) / max(abs(loss_full - oloss) / abs(oloss), 1e-300),
                 abs(loss_new - loss_full) / abs(loss_full), abs(loss_full - oloss) / abs(oloss), "loss"))
    compare("last_emissions", tg_new.last_emissions.cpu()[v], tg_full.last_emissions.cpu()[v], oem[v])
    compare("last_pooled", tg_new.last_pooled.float().cpu()[v], tg_full.last_pooled.float().cpu()[v], opooled[v])
    # every gradient tensor check_step compares: attention key biases are excluded (softmax is invariant to a per-query constant:
    # the gradient is 0 in exact arithmetic and all three sides hold roundoff noise), as are tensors with no gradient to speak of
    gscale = max(float(p.grad.abs().max()) for p in oparams.values() if p.grad is not None)
    for hf, (mine, sl) in engine.hf_name_map(cfg).items():
        go = oparams[hf].grad
        if go is None or hf.endswith("key.bias") or float(go.abs().max()) < 1e-7 * gscale:
            continue
        gn, gf = tg_new.arena.grad(mine), tg_full.arena.grad(mine)
        if sl is not None:
            gn, gf = gn[sl[0]:sl[1]], gf[sl[0]:sl[1]]
        compare("grad " + hf, gn.cpu(), gf.cpu(), go)
    for k in ("linear.weight", "linear.bias", "transitions"):
        compare("grad " + k, tg_new.arena.grad(k).cpu(), tg_full.arena.grad(k).cpu(), oparams[k].grad)
    rows.sort(reverse=True)
    print("\n[head_rows] %s dropout=%s word_dropout=%g: new-vs-full / full-vs-oracle, worst first" % (cfgname, dropout, word_dropout))
    for ratio, d_nf, d_fo, name in rows[:8]:
        print("[head_rows]   ratio %.4f  new-vs-full %.3e  full-vs-oracle %.3e  %s" % (ratio, d_nf, d_fo, name))
    bad = [(name, ratio) for ratio, _, _, name in rows if not ratio <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("cfgname", ["small", "large"])
def test_check_step_passes_through_the_head_rows_path(monkeypatch, cfgname, dropout):
    calls = []
    fwd = ops.attn_rows_fwd
    monkeypatch.setattr(ops, "attn_rows_fwd", lambda *a, **k: (calls.append(1), fwd(*a, **k))[1])
    assert engine.Tagger.HEAD_ROWS_ONLY is True
    c = SMALL if cfgname == "small" else LARGE
    r = selftest.check_step(dropout=dropout, H=c["H"], A=c["A"], F_=c["F_"], L=c["L"], S=c["S"], V=c["V"],
                            std=0.08 if cfgname == "small" else 0.02)
    print("[head_rows] check_step %s dropout=%s: %s" % (cfgname, dropout, {k: v for k, v in r.items() if "table" not in k}))
    assert calls, "check_step did not take the head-rows path"
    if not dropout:
        selftest.assert_step(r)
    else:   # the thresholds tests/test_gpu_kernels.py test_full_step_with_dropout_vs_oracle applies to check_step(dropout=True)
        assert r["n_sites"] == 1 + 3 * c["L"], r
        assert r["loss_rel"] < 3e-2 and r["emissions_rel"] < 3e-2, r
        assert r["grad_min_cos"] > 0.97 and r["grad_worst_rel"] < 0.2, r
        assert r["grad_linear.weight"] < 5e-2 and r["grad_transitions"] < 5e-2, r


def test_old_path_where_the_preconditions_fail():
    c = SMALL
    # a layer selection
    _, tg = make_tagger(c, True, layers=(-1, -2))
    b = uneven_batch(c["B"], c["S"], c["V"])
    tg.forward_loss(kb.to_device(b, DEV), backward=True)
    assert tg.last_path == "full"
    # 4 * nc > S
    _, tg = make_tagger(c, True)
    b = kb.synthetic_batch(c["B"], c["S"], vocab=c["V"], T=T, x_idx=X_IDX, start=START, stop=STOP, n_real=c["S"] // 4 + 1, seed=3)
    assert 4 * b["ctags"].shape[1] > c["S"]
    tg.forward_loss(kb.to_device(b, DEV), backward=True)
    assert tg.last_path == "full"
    b = kb.synthetic_batch(c["B"], c["S"], vocab=c["V"], T=T, x_idx=X_IDX, start=START, stop=STOP, n_real=c["S"] // 4, seed=3)
    tg.forward_loss(kb.to_device(b, DEV), backward=True)
    assert tg.last_path == "head_rows"
    # a windowed batch: sentence 0 spans encoder rows 0 and 1 (R = B + 1)
    ids, am, first_idx, tags, lengths = kb.synthetic_sentences(2, 64, vocab=c["V"], T=T, x_idx=X_IDX, start=START, stop=STOP, n_real=5, seed=9)
    ids3, am3 = np.concatenate([ids[:1], ids]), np.concatenate([am[:1], am])
    first_row = np.zeros_like(first_idx)
    first_row[0, 3:] = 1
    first_row[1] = 2
    b = kb.assemble(ids3, am3, first_idx, tags, lengths, X_IDX, first_row=first_row)
    assert b["R"] == 3 and b["B"] == 2
    torch.cuda.synchronize()
    tg.forward_loss(kb.to_device(b, DEV), backward=True)
    torch.cuda.synchronize()
    assert tg.last_path == "full"
    # the switch off
    _, tg = make_tagger(c, False)
    tg.forward_loss(kb.to_device(uneven_batch(c["B"], c["S"], c["V"]), DEV), backward=True)
    assert tg.last_path == "full"
