"""CPU: tests/crfref.py (the float64 references of tests/test_gpu_crf_kernels.py) proved without a GPU -- against brute-force
enumeration of every path, against torch.autograd in float64, against oracle/crf.py on the golden files' own inputs -- plus
the two conditions the GPU module relies on: its tie inputs really tie, and its check (crfref.check_grid) refuses a float32
evaluation with any of eight defects switched on, each on a named case of the GPU module's own list."""
import contextlib
import io
import itertools
import os

import numpy as np
import pytest
import torch

import crfref
from oracle import crf as ocrf

F64 = np.float64


# ====================================================================== brute force: every path, float64
def _paths(T, n):
    return np.array(list(itertools.product(range(T), repeat=n)), np.int64)             # [T^n, n]


def _path_scores(e, tr, paths, start, stop):
    """score of each path under transitions[to, from]: emissions + trans[p_0, START] + trans[p_k, p_{k-1}] + trans[STOP, p_last]"""
    n = paths.shape[1]
    s = e[np.arange(n)[None, :], paths].sum(1) + tr[paths[:, 0], start] + tr[stop, paths[:, -1]]
    for k in range(1, n):
        s = s + tr[paths[:, k], paths[:, k - 1]]
    return s


BRUTE = [(T, n, st, sp) for T in (3, 4, 5) for n in (1, 2, 3, 4)
         for st, sp in ((T - 2, T - 1), (0, 1), (1, 0), (T - 1, 0), (T // 2, (T // 2 + 1) % T))]


@pytest.mark.parametrize("T,n,start,stop", BRUTE)
def test_forward_marginals_viterbi_equal_path_enumeration(T, n, start, stop):
    rng = np.random.default_rng(T * 100 + n * 10 + start)
    B = 3
    emit, trans, tags, _ = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    lens = np.full(B, n, np.int32)
    paths = _paths(T, n)
    logz, alpha = crfref.forward(emit, trans, lens, start, stop)
    marg = crfref.marginals(emit, trans, lens, start, stop)
    vt, conf, popped = crfref.viterbi(emit, trans, lens, start, stop)
    gold = crfref.gold(emit, trans, tags, lens, start, stop)
    for b in range(B):
        s = _path_scores(emit[b].astype(F64), trans.astype(F64), paths, start, stop)
        m = s.max()
        z = m + np.log(np.exp(s - m).sum())
        assert abs(logz[b] - z) <= 1e-12 * max(1.0, abs(z))
        p = np.exp(s - z)
        for i in range(n):
            want = np.bincount(paths[:, i], weights=p, minlength=T)
            assert np.abs(marg[b, i] - want).max() <= 1e-12
        assert np.array_equal(vt[b], paths[int(s.argmax())])                       # Gaussian inputs: no tie
        assert popped[b] == start
        k = int(np.nonzero((paths == tags[b][None, :]).all(1))[0][0])
        assert abs(gold[b] - s[k]) <= 1e-12 * max(1.0, abs(s[k]))
    assert np.abs(marg.sum(2) - 1.0).max() <= 1e-12


def test_shorter_sentences_are_the_prefix_problem():
    """lens < n: every function equals itself on the sentence cut to its length, and pads as documented"""
    rng = np.random.default_rng(5)
    B, n, T, start, stop = 4, 6, 5, 1, 3
    emit, trans, tags, lens = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    assert sorted(lens.tolist())[:2] == [0, 1] and lens.max() == n
    w = crfref.dloss_mix(rng, B)
    logz, alpha = crfref.forward(emit, trans, lens, start, stop)
    marg = crfref.marginals(emit, trans, lens, start, stop)
    de, dtr = crfref.nll_grads(emit, trans, tags, lens, w, start, stop)
    vt, conf, popped = crfref.viterbi(emit, trans, lens, start, stop)
    acc = np.zeros((T, T))
    for b in range(B):
        L = int(lens[b])
        one = np.array([L], np.int32)
        z1, a1 = crfref.forward(emit[b:b + 1, :L], trans, one, start, stop)
        assert z1[0] == logz[b] and np.array_equal(a1[0], alpha[b, :L + 1])
        assert np.array_equal(marg[b, :L], crfref.marginals(emit[b:b + 1, :L], trans, one, start, stop)[0]) and (marg[b, L:] == 0).all()
        d1, t1 = crfref.nll_grads(emit[b:b + 1, :L], trans, tags[b:b + 1, :L], one, w[b:b + 1], start, stop)
        assert np.array_equal(de[b, :L], d1[0]) and (de[b, L:] == 0).all()
        acc += t1
        assert (vt[b, L:] == -1).all() and (conf[b, L:] == 0).all()
    assert np.abs(acc - dtr).max() <= 1e-12
    b0 = int(np.nonzero(lens == 0)[0][0])
    assert popped[b0] == start and logz[b0] == pytest.approx(float(trans[stop, start]), abs=1e-9)
    assert crfref.gold(emit, trans, tags, lens, start, stop)[b0] == float(trans[stop, start])


@pytest.mark.parametrize("T,n,start,stop", [c for c in BRUTE if c[1] >= 2])
def test_oracle_nbest_equals_path_enumeration(T, n, start, stop):
    """oracle.crf.viterbi_nbest on full-length sentences: the nbest best paths and the softmax of their scores, in its [from, to]
    indexing (score = emissions + trans[START, first] + trans[prev, cur] + trans[last, STOP]).  n = 1 is left out: the decoder
    starts from `nbest` copies of the first partition, so its n = 1 answer is the best tag `nbest` times (a reproduced defect)."""
    rng = np.random.default_rng(T * 100 + n * 10 + stop)
    B = 2
    emit = (rng.standard_normal((B, n, T)) * 2).astype(np.float32)
    trans = rng.standard_normal((T, T)).astype(np.float32)
    paths = _paths(T, n)
    for nbest in sorted({1, 2, T}):
        ps, dec = ocrf.viterbi_nbest(emit, np.full(B, n), trans, start, stop, nbest)
        for b in range(B):
            s = _path_scores(emit[b].astype(F64), trans.astype(F64).T, paths, start, stop)   # [from, to] = transposed [to, from]
            order = np.argsort(-s, kind="stable")[:nbest]
            assert np.array_equal(dec[b].T, paths[order])
            p = np.exp(s[order] - s[order].max())
            assert np.abs(ps[b] - p / p.sum()).max() <= 2e-6


# ====================================================================== autograd, float64
def _nll_torch(emit, trans, tags, lens, dloss, start, stop):
    total = emit.new_zeros(())
    T = emit.shape[2]
    for b in range(emit.shape[0]):
        L = int(lens[b])
        a = torch.full((T,), -1e12, dtype=emit.dtype)
        a[start] = 0.0
        g = emit.new_zeros(())
        prev = start
        for i in range(L):
            a = torch.logsumexp(emit[b, i][:, None] + trans + a[None, :], dim=1)
            t = int(tags[b, i])
            g = g + emit[b, i, t] + trans[t, prev]
            prev = t
        logz = torch.logsumexp(a + trans[stop], dim=0)
        total = total + float(dloss[b]) * (logz - (g + trans[stop, prev]))
    return total


@pytest.mark.parametrize("T,start,stop,B,n", [(5, 1, 0, 4, 6), (33, 32, 0, 4, 9), (64, 17, 5, 5, 7), (33, 0, 32, 3, 5)])
def test_nll_grads_equal_autograd(T, start, stop, B, n):
    rng = np.random.default_rng(T + B)
    emit, trans, tags, lens = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    w = crfref.dloss_mix(rng, B)
    assert (w > 0).any() and (w == 0).any() and (w < 0).any()
    e = torch.from_numpy(emit).double().requires_grad_(True)
    tr = torch.from_numpy(trans).double().requires_grad_(True)
    _nll_torch(e, tr, tags, lens, w, start, stop).backward()
    de, dtr = crfref.nll_grads(emit, trans, tags, lens, w, start, stop)
    assert np.abs(de - e.grad.numpy()).max() <= 1e-12
    assert np.abs(dtr - tr.grad.numpy()).max() <= 1e-11


# ====================================================================== what is already pinned: oracle/crf.py on the golden inputs
def _g(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def test_agrees_with_oracle_on_golden_inputs(golden_dir):
    g = _g(golden_dir, "crf_forward_score.npz")
    start, stop = int(g["start"]), int(g["stop"])
    for c in range(int(g["n_cases"])):
        feats, lens, tags, trans = (g["c%d_%s" % (c, k)] for k in ("feats", "lens", "tags", "trans"))
        logz, alpha = crfref.forward(feats, trans, lens, start, stop)
        np.testing.assert_allclose(ocrf.forward_alg(feats, lens, trans, start, stop), logz, rtol=2e-6, atol=2e-5)
        np.testing.assert_allclose(ocrf.score_sentence(feats, tags, lens, trans, start, stop),
                                   crfref.gold(feats, trans, tags, lens, start, stop), rtol=2e-6, atol=2e-5)
        B = feats.shape[0]
        w = np.linspace(-1.0, 1.0, B) if B > 1 else np.ones(1)
        de, dtr = crfref.nll_grads(feats, trans, tags, lens, w, start, stop)
        ode, odtr = ocrf.crf_nll_grads(feats, tags, lens, trans, start, stop, dloss=w)
        assert np.abs(de - ode).max() <= 1e-10 and np.abs(dtr - odtr).max() <= 1e-10
    g = _g(golden_dir, "viterbi.npz")
    start, stop = int(g["start"]), int(g["stop"])
    for c in range(int(g["n_cases"])):
        feats, trans = g["c%d_feats" % c][None], g["c%d_trans" % c]
        lens = np.array([feats.shape[1]], np.int32)
        ot, oc = ocrf.viterbi_batch(feats, lens, trans, start, stop)
        for dt in (np.float32, F64):
            vt, conf, popped, sc = crfref.viterbi(feats, trans, lens, start, stop, dtype=dt, with_scores=True)
            assert np.array_equal(vt, ot) and popped[0] == start
            # the oracle's float32 scores carry up to half an ulp of |score| per step into the exponent of its confidence
            tol = 1e-6 if dt == np.float32 else 1e-6 + 4 * 2.0 ** -24 * crfref.fin(sc).max()
            assert np.abs(conf - oc).max() <= tol
    g = _g(golden_dir, "posterior.npz")
    trans, start, stop = g["trans"], int(g["start"]), int(g["stop"])
    for c in range(int(g["n_cases"])):
        feats, lens = g["c%d_feats" % c], g["c%d_lens" % c]
        dist, _ = ocrf.posterior(feats, lens, trans, start, stop)
        marg = crfref.marginals(feats, trans, lens, start, stop)
        valid = np.arange(feats.shape[1])[None, :] < lens[:, None]
        assert np.abs(dist[valid] - marg[valid]).max() < 2e-5
        assert (marg[~valid] == 0).all()


# ====================================================================== the inputs of the GPU module
def test_grid_covers_what_the_gpu_module_promises():
    by_T = {}
    for T, start, stop, B, n, scale, big in crfref.GRID:
        by_T.setdefault(T, set()).add((start, stop))
        assert 0 <= start < T and 0 <= stop < T and start != stop
    assert sorted(by_T) == [3, 5, 29, 31, 32, 33, 48, 63, 64]
    assert all(len(v) >= 2 for v in by_T.values())
    for wide in (False, True):                                                  # every placement on both kernel widths
        seen = set()
        for T, start, stop, *_ in crfref.GRID:
            if (T > 32) == wide:
                seen |= {k for k, v in crfref._placements(T).items() if v == (start, stop)}
        assert seen == {"last2", "first2", "swapped", "ends", "middle"}
    assert {(c[3], c[4]) for c in crfref.GRID} == {(1, 1), (5, 1), (3, 7), (16, 48), (2, 130)}
    assert {c[0] > 32 for c in crfref.GRID if c[6]} == {False, True}
    for case in crfref.GRID:
        x = crfref.grid_inputs(case)
        lens, B, n = x["lens"], x["B"], x["n"]
        assert lens[0] == n and (B < 2 or 1 in lens) and (B < 3 or 0 in lens)
        assert not np.isin(x["tags"], (x["start"], x["stop"])).any()
        if B > 1:
            assert (x["dloss"] > 0).any() and (x["dloss"] == 0).any() and (B < 3 or (x["dloss"] < 0).any())
        assert (x["pattern"] != 0).all() and (x["pattern"] == np.round(x["pattern"])).all()


@pytest.mark.parametrize("case", [c for c in crfref.GRID if c[4] > 1], ids=crfref.grid_id)
def test_tie_inputs_tie(case):
    """a condition on the inputs: every tie case is exact in float32 (float32 and float64 Viterbi agree bit for bit), and at
    T >= 32 at least a quarter of its (step, to) cells hold tied maximal candidates and one sentence has a tied terminal"""
    x = crfref.grid_inputs(case)
    a = (x["tie_emit"], x["tie_trans"], x["tie_lens"], x["start"], x["stop"])
    share, terminal = crfref.tie_stats(*a)
    if x["T"] >= 32:
        assert share >= 0.25 and terminal >= 1, (share, terminal)
    t32 = crfref.viterbi(*a, dtype=np.float32, with_scores=True)
    t64 = crfref.viterbi(*a, dtype=F64, with_scores=True)
    assert np.array_equal(t32[0], t64[0]) and np.array_equal(t32[2], t64[2])
    finite = np.abs(t64[3]) < crfref.BIG
    assert np.array_equal(np.abs(t32[3]) < crfref.BIG, finite)
    assert np.array_equal(t32[3].astype(F64)[finite], t64[3][finite])           # every finite score is a small integer, exact in float32
    assert (t64[3][finite] == np.round(t64[3][finite])).all() and np.abs(t64[3][finite]).max() <= 3 * x["n"]
    ot, oc = ocrf.viterbi_batch(a[0], a[2], a[1], a[3], a[4])
    assert np.array_equal(ot, t64[0])


def test_issue_tie_table():
    """the four (T, START, STOP) points at B = 6, n = 24: ties are everywhere at T >= 32"""
    for T, start, stop, low in ((33, 0, 32, 0.25), (64, 17, 5, 0.25), (32, 30, 31, 0.25), (5, 1, 0, 0.05)):
        e, tr, lens = crfref.tie_case(np.random.default_rng(T), 6, 24, T, start, stop)
        share, terminal = crfref.tie_stats(e, tr, lens, start, stop)
        assert share >= low, (T, share)


# ====================================================================== discriminating power: float32 evaluations with a defect
DEFECTS = ["transposed", "stop_is_last", "start_is_T_minus_2", "padding_zero", "lens_minus_one", "dloss_of_sentence_0",
           "dtrans_overwritten", "last_index_tie_break"]


def _lse32(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return (np.squeeze(m, axis) + np.log(np.exp(x - m).sum(axis=axis, dtype=np.float32))).astype(np.float32)


def evaluate32(x, defect=None):
    """Every output of the shared grid in float32, at the padded tag width TT = 32 / 64 the kernels use (padding lanes hold
    -1e12 scores and -inf transitions), with one switchable defect.  -> the `got` dictionary of crfref.check_grid"""
    f = np.float32
    T, start, stop, n, B = x["T"], x["start"], x["stop"], x["n"], x["B"]
    TT = 32 if T <= 32 else 64
    pad_tr, pad_lane = (f(0.0), f(0.0)) if defect == "padding_zero" else (f(-np.inf), f(crfref.NEG))
    stop_row = T - 1 if defect == "stop_is_last" else stop
    start_lane = T - 2 if defect == "start_is_T_minus_2" else start

    def padded_trans(trans):
        tr = np.asarray(trans, f)
        tr = tr.T if defect == "transposed" else tr
        P = np.full((TT, TT), pad_tr, f)
        P[:T, :T] = tr
        return tr, P

    def lane0():
        a = np.full(TT, pad_lane, f)
        a[:T] = f(crfref.NEG)
        a[start_lane] = 0.0
        return a

    def cut(lens):
        return np.maximum(np.asarray(lens) - 1, 0) if defect == "lens_minus_one" else np.asarray(lens)

    def vit(emit, trans, lens):
        tr, P = padded_trans(trans)
        tags, conf, popped = np.full((B, n), -1, np.int32), np.zeros((B, n), f), np.full(B, start, np.int32)
        for b in range(B):
            L = int(cut(lens)[b])
            v = lane0()
            bps = np.zeros((L, TT), np.int64)                   # a back-pointer into the padding shows as a wrong tag
            for i in range(L):
                cand = v[None, :] + P[:T]
                bp = TT - 1 - cand[:, ::-1].argmax(1) if defect == "last_index_tie_break" else cand.argmax(1)
                v[:T] = cand[np.arange(T), bp] + emit[b, i]
                bps[i, :T] = bp
                conf[b, i] = f(1.0) / np.exp(v[:T] - v[:T].max()).sum(dtype=f)
            term = v[:T] + tr[stop_row]
            term[stop] = term[start] = f(crfref.NEG)
            best = T - 1 - int(term[::-1].argmax()) if defect == "last_index_tie_break" else int(term.argmax())
            for i in range(L - 1, -1, -1):
                tags[b, i] = best
                best = int(bps[i, best])
            if L:
                popped[b] = best
        return tags, conf, popped

    got = {}
    got["vtags"], got["vconf"], got["vpopped"] = vit(x["emit"], x["trans"], x["lens"])
    if x["tie_emit"] is not None:
        got["tie_tags"], got["tie_conf"], got["tie_popped"] = vit(x["tie_emit"], x["tie_trans"], x["tie_lens"])
    emit, lens, tags = x["emit"], cut(x["lens"]), x["tags"]
    tr, P = padded_trans(x["trans"])
    w = np.full(B, x["dloss"][0], f) if defect == "dloss_of_sentence_0" else x["dloss"]
    logz, gold = np.zeros(B, f), np.zeros(B, f)
    alpha = np.full((B, n + 1, T), np.nan, f)
    marg, demit, dtrans = np.zeros((B, n, T), f), np.zeros((B, n, T), f), np.zeros((T, T), f)
    for b in range(B):
        L = int(lens[b])
        a = lane0()
        rows = [a.copy()]
        for i in range(L):
            a[:T] = _lse32((emit[b, i][:, None] + P[:T]) + a[None, :], 1)
            rows.append(a.copy())
        alpha[b, :L + 1] = np.array(rows)[:, :T]
        logz[b] = _lse32(a[:T] + tr[stop_row], 0)
        prev, g = start_lane, f(0.0)
        for k in range(L):
            g = f(g + (emit[b, k, tags[b, k]] + tr[tags[b, k], prev]))
            prev = int(tags[b, k])
        gold[b] = g + tr[stop_row, prev]
        beta = np.full(TT, pad_lane, f)
        beta[:T] = tr[stop_row]
        dtrans[stop_row] += w[b] * np.exp(rows[L][:T] + beta[:T] - logz[b])
        for i in range(L - 1, -1, -1):
            q = np.exp(((emit[b, i] + beta[:T] - logz[b])[:, None] + P[:T]) + rows[i][None, :])   # [to, from over TT]
            marg[b, i] = q.sum(1, dtype=f)
            demit[b, i] = w[b] * marg[b, i]
            demit[b, i, tags[b, i]] -= w[b]
            dtrans += w[b] * q[:, :T]
            ep = np.full(TT, f(0.0), f)
            ep[:T] = emit[b, i]
            beta[:T] = _lse32((ep[:, None] + P[:, :T]) + beta[:, None], 0)
        prev = start_lane
        for k in range(L):
            dtrans[tags[b, k], prev] -= w[b]
            prev = int(tags[b, k])
        dtrans[stop_row, prev] -= w[b]
    got.update(logz=logz, gold=gold, alpha=alpha, marg=marg, demit=demit,
               dtrans=dtrans if defect == "dtrans_overwritten" else x["pattern"] + dtrans)
    return got


def _passes(case, defect):
    try:
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            crfref.check_grid(case, evaluate32(crfref.grid_inputs(case), defect), crfref.Stats("cpu"))
    except AssertionError:
        return False
    return True


def _case(name):
    return next(c for c in crfref.GRID if crfref.grid_id(c) == name)


@pytest.mark.parametrize("case", crfref.GRID, ids=crfref.grid_id)
def test_check_accepts_the_sound_float32_evaluation(case):
    """the check the GPU module applies is passable: a plain float32 evaluation at the kernels' padded width passes every case"""
    crfref.check_grid(case, evaluate32(crfref.grid_inputs(case)), crfref.Stats("cpu"))


# defect -> the cases of the GPU module's list on which crfref.check_grid must refuse it
CAUGHT_BY = {
    "transposed": ["T5-s0-e1-B16-n48", "T64-s62-e63-B16-n48"],
    "stop_is_last": ["T32-s0-e1-B2-n130", "T33-s32-e0-B16-n48", "T64-s17-e5-B16-n48-big"],
    "start_is_T_minus_2": ["T29-s28-e0-B3-n7", "T33-s32-e0-B16-n48", "T64-s1-e0-B2-n130"],
    "padding_zero": ["T3-s1-e2-B3-n7", "T29-s27-e28-B16-n48", "T31-s29-e30-B2-n130", "T33-s31-e32-B3-n7", "T63-s1-e0-B16-n48"],
    "lens_minus_one": ["T3-s2-e0-B1-n1", "T32-s1-e0-B3-n7", "T64-s1-e0-B2-n130"],
    "dloss_of_sentence_0": ["T5-s2-e3-B2-n130", "T64-s63-e0-B5-n1"],
    "dtrans_overwritten": ["T3-s2-e0-B1-n1", "T64-s32-e33-B1-n1"],
    "last_index_tie_break": ["T32-s30-e31-B16-n48", "T33-s0-e1-B2-n130", "T64-s0-e1-B3-n7"],
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_check_refuses_each_defect(defect):
    for name in CAUGHT_BY[defect]:
        assert not _passes(_case(name), defect), "%s is not caught by %s" % (defect, name)


def test_defects_that_a_case_cannot_show_pass_it():
    """the mutants are real: where a defect coincides with the sound evaluation (START / STOP are the last two ids, no padding
    lane at T = 32 / 64, one sentence) the check passes, so a refusal above is the defect's doing"""
    assert _passes(_case("T29-s27-e28-B16-n48"), "stop_is_last") and _passes(_case("T64-s62-e63-B16-n48"), "start_is_T_minus_2")
    assert _passes(_case("T32-s30-e31-B16-n48"), "padding_zero") and _passes(_case("T64-s1-e0-B2-n130"), "padding_zero")
    assert _passes(_case("T64-s32-e33-B1-n1"), "dloss_of_sentence_0")
