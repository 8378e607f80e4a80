"""CPU: proves tests/lstmbwdref.py -- the float64 references of the LSTM training kernels against float64 torch.nn.LSTM autograd
(packed, bidirectional, kbner.stack.step_tables, hidden sizes that pad, ragged lengths including 1), the conditions of the EXACT
cases, the case list, and the power of the comparison tests/test_gpu_lstm_train_kernels.py uses (lstmbwdref.check_bwd_case): ten
defective evaluations of the backward step are refused at the smallest case that can show them."""
import numpy as np
import pytest
import torch

import lstmbwdref as R
import rowref

F64 = np.float64


# ====================================================================== against torch.nn.LSTM autograd
def _pad_gate_rows(w, H, Hp):
    """[4H, ...] -> [4Hp, ...], every gate block zero-padded (kbner.stack.LSTMGroup.pad_gates)"""
    out = np.zeros((4 * Hp,) + w.shape[1:])
    for q in range(4):
        out[q * Hp:q * Hp + H] = w[q * H:(q + 1) * H]
    return out


def _unpad_gate_rows(w, H, Hp):
    return np.concatenate([w[q * Hp:q * Hp + H] for q in range(4)], 0)


def torch_problem(B, n, D, H, lengths, seed):
    """a packed bidirectional float64 torch.nn.LSTM, a linear loss sum(y * G), and its autograd gradients"""
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    rnn = torch.nn.LSTM(D, H, 1, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.mul_(2.0)
    x = rng.standard_normal((B, n, D))
    for b in range(B):
        x[b, lengths[b]:] = 0.0
    xt = torch.from_numpy(x).requires_grad_(True)
    packed = torch.nn.utils.rnn.pack_padded_sequence(xt, torch.from_numpy(np.asarray(lengths)), batch_first=True, enforce_sorted=False)
    y, _ = rnn(packed)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)
    G = rng.standard_normal((B, n, 2 * H))
    (y * torch.from_numpy(G)).sum().backward()
    sd = {k: v.detach().numpy() for k, v in rnn.state_dict().items()}
    grads = {k: p.grad.numpy() for k, p in rnn.named_parameters()}
    return NS(x=x, y=y.detach().numpy(), G=G, sd=sd, grads=grads, dx=xt.grad.numpy())


NS = R.NS


@pytest.mark.parametrize("B,n,D,H,lengths", [(6, 9, 5, 24, [9, 1, 4, 9, 2, 7]), (3, 4, 7, 100, [1, 4, 3])])
def test_references_equal_torch_autograd_packed_bidirectional_padded(B, n, D, H, lengths):
    from kbner.stack import check_prefix_active, step_tables
    Hp = (H + 63) // 64 * 64
    t = torch_problem(B, n, D, H, lengths, seed=B + H)
    sfx = ("", "_reverse")
    X = t.x.reshape(B * n, D)
    gx = np.concatenate([X @ _pad_gate_rows(t.sd["weight_ih_l0" + s], H, Hp).T
                         + _pad_gate_rows(t.sd["bias_ih_l0" + s] + t.sd["bias_hh_l0" + s], H, Hp) for s in sfx], 1)
    whh = np.zeros((2, 4 * Hp, Hp))
    for d, s in enumerate(sfx):
        whh[d, :, :H] = _pad_gate_rows(t.sd["weight_hh_l0" + s], H, Hp)
    tab = check_prefix_active(step_tables(lengths, n), B * n, 2, B)
    cols = [0, Hp]
    fw = R.train_fwd(gx, tab, whh, tab, np.zeros((B * n, 2 * Hp)), cols, round_h=False)
    y = np.concatenate([fw.out[:, :H], fw.out[:, Hp:Hp + H]], 1).reshape(B, n, 2 * H)
    assert np.abs(y - t.y).max() < 1e-12
    assert not fw.out[:, H:Hp].any() and not fw.out[:, Hp + H:].any()               # padded units stay exactly 0
    dout = np.zeros((B * n, 2 * Hp))
    dout[:, :H], dout[:, Hp:Hp + H] = t.G.reshape(B * n, 2 * H)[:, :H], t.G.reshape(B * n, 2 * H)[:, H:]
    d = NS(gxi=tab, outi=tab, whh=whh, gates=fw.gates, cs=fw.cs, dout=dout, out_cols=cols, Hp=Hp, ndir=2, rows_gx=B * n,
           carry0=np.zeros((2, B, Hp)))
    bw = R.bwd_seq(d)
    dgx = np.nan_to_num(bw.dgx)                                                       # rows no step consumes: the caller's zeros
    dwih, dwhh, db = R.weight_grads(X, dgx, np.nan_to_num(fw.hprev), 2, Hp)
    for dd, s in enumerate(sfx):
        blk = slice(dd * 4 * Hp, (dd + 1) * 4 * Hp)
        assert np.abs(_unpad_gate_rows(dwih[blk], H, Hp) - t.grads["weight_ih_l0" + s]).max() < 1e-10
        assert np.abs(_unpad_gate_rows(dwhh[dd], H, Hp)[:, :H] - t.grads["weight_hh_l0" + s]).max() < 1e-10
        assert np.abs(_unpad_gate_rows(db[blk], H, Hp) - t.grads["bias_ih_l0" + s]).max() < 1e-10
        assert np.abs(t.grads["bias_ih_l0" + s] - t.grads["bias_hh_l0" + s]).max() < 1e-14  # the two biases receive one gradient
        pad = np.ones(4 * Hp, bool)
        for q in range(4):
            pad[q * Hp:q * Hp + H] = False
        assert not dwih[blk][pad].any() and not dwhh[dd][pad].any() and not dwhh[dd][:, H:].any() and not db[blk][pad].any()
    wih = np.concatenate([_pad_gate_rows(t.sd["weight_ih_l0" + s], H, Hp) for s in sfx], 0)
    assert np.abs((dgx @ wih).reshape(B, n, D) - t.dx).max() < 1e-10
    # the float32 evaluation is the same formula
    st64, st32 = R.bwd_step(d, 0, bw.dgx, bw.carry_after[1]), R.bwd_step(d, 0, bw.dgx, bw.carry_after[1], f32=True)
    assert st32.val[0].dtype == np.float32 and 0 < np.abs(st32.val[1] - st64.val[1]).max() < 1e-4
    assert all((sa >= np.abs(v) * (1 - 1e-12)).all() for sa, v in zip(st64.sa_dgx, st64.val))


# ====================================================================== the case list
def test_case_list_covers_what_it_says():
    for kind, cases in (("real", R.REAL_CASES), ("exact", R.EXACT_CASES)):
        shapes = {(c[1], c[2]) for c in cases}
        assert all((hp, b) in shapes for hp in (64, 128, 192, 320) for b in (17, 33))
        assert all((hp, b) in shapes for b in (1, 16, 17, 33, 65, 70) for hp in (64, 320))
        assert {c[3] for c in cases} == {1, 2} and all(c[0] == kind for c in cases)
    assert {c[4] for c in R.REAL_CASES} == {1, 2, 5, 8, 9} and {c[4] for c in R.EXACT_CASES} == {1, 2}
    assert ("real", 1024, 4, 2, 9) in R.REAL_CASES and all(c[4] == 0 for c in R.ZERO_STEP_CASES)
    assert len(set(R.CASES)) == len(R.CASES)


@pytest.mark.parametrize("case", R.CASES + R.ZERO_STEP_CASES, ids=R.case_id)
def test_row_tables_are_inside_the_training_contract(case):
    from kbner.stack import check_prefix_active
    d = R.build_case(case)
    check_prefix_active(d.gxi, d.rows_gx, d.ndir, d.B)
    act = d.gxi >= 0
    assert not (~act & (d.outi >= 0)).any() and d.outi.max(initial=-1) < d.rows_out
    used = R._consumed(d.gxi, d.rows_gx, d.ndir)
    assert (~used).any()                                                       # rows no step consumes
    if d.steps and d.B >= 3:
        assert not act[:, :, d.dead].any() and act[:, :, d.mute].all() and (d.outi[:, :, d.mute] == -1).all()
        assert (d.carry0[:, d.dead] == R.CARRY_GUARD).all()
    if d.steps >= 2 and d.B >= 16:
        assert len(set(d.lengths.tolist())) >= 3
    if d.steps >= 2:
        b = int(np.argmax(d.lengths))
        rows = d.gxi[:, 0, b]
        assert not np.array_equal(rows, rows[0] + np.arange(d.steps))          # permuted, not b * n + t
    if d.ndir == 2 and d.steps >= 2:
        b = [b for b in range(d.B) if b != d.mute and d.lengths[b] >= 2][0]
        n = d.lengths[b]
        assert np.array_equal(d.outi[:n, 1, b], d.outi[:n, 0, b][::-1])
    assert np.isnan(d.gates[~np.repeat(used, 4 * d.Hp, axis=1)]).all() and not np.isnan(d.gates[np.repeat(used, 4 * d.Hp, axis=1)]).any()


@pytest.mark.parametrize("case", R.EXACT_CASES + R.ZERO_STEP_CASES, ids=R.case_id)
def test_exact_conditions(case):
    d = R.build_case(case)
    used = R._consumed(d.gxi, d.rows_gx, d.ndir)
    u1, u4 = np.repeat(used, d.Hp, axis=1), np.repeat(used, 4 * d.Hp, axis=1)
    assert (d.gates[u4] == 0.5).all() and (d.cs[u1] == 0).all()
    assert np.array_equal(d.whh, np.rint(d.whh)) and np.abs(d.whh).max() <= 2
    assert ((d.whh != 0).sum(axis=1) <= 3).all() and ((d.whh[:, :d.Hp] != 0).sum(axis=1) <= 1).all()      # per column j
    read = ~np.isnan(d.dout)
    assert np.isin(d.dout[read], (-16.0, 0.0, 16.0)).all()
    ever = (d.gxi >= 0).any(axis=0) if d.steps else np.zeros((d.ndir, d.B), bool)
    assert not d.carry0[ever].any()
    ref = d.ref
    v = ref.dgx[u4]
    assert np.array_equal(rowref.bf16_round(v).astype(F64), v), "a reference dgx value is no bf16 value"
    assert np.array_equal(v * 16, np.rint(v * 16))
    for c in ref.carry_after:
        assert np.array_equal(c.astype(np.float32).astype(F64), c) and np.array_equal(c * 16, np.rint(c * 16))
    # every partial sum of every step, in any order, is a multiple of 1/16 below 2^24 / 16: float32 adds exactly
    for s in range(d.steps):
        st = R.bwd_step(d, s, ref.dgx, ref.carry_after[s + 1])
        assert all(float(sa.max(initial=0.0)) * 16 < 2 ** 24 for sa in st.sa_dgx)
        for dd in range(d.ndir):                                               # do = df = 0: t = 0 and c_prev = 0
            blk = st.val[dd].reshape(-1, 4, d.Hp)
            assert not blk[:, 1].any() and not blk[:, 3].any()
    if d.steps == 2:                                                           # the recurrent term and the carry both act
        st = R.bwd_step(d, 0, ref.dgx, ref.carry_after[1])
        no_rec = R.bwd_step(d, 0, ref.dgx, ref.carry_after[1], defect="no_recurrent")
        assert any((a != b).mean() > 0.05 for a, b in zip(st.val, no_rec.val))


# ====================================================================== the check's power
def evaluate(d, defect=None):
    """the walk of case d as a kernel would leave it in memory (dgx bf16, carry float32), with one defect"""
    return R.as_stored(R.bwd_seq(d, round_store=True, defect=defect))


CAN_SHOW = {    # defect -> (a REAL case can show it, an EXACT case can show it or None)
    "no_dc_carry": (lambda d: d.steps >= 2, lambda d: d.steps >= 2),
    "c_for_c_prev": (lambda d: d.steps >= 1, None),                     # EXACT: c = 0 everywhere
    "no_recurrent": (lambda d: d.steps >= 2, lambda d: d.steps >= 2),
    "whh_not_transposed": (lambda d: d.steps >= 2, lambda d: d.steps >= 2),
    "other_direction_whh": (lambda d: d.steps >= 2 and d.ndir >= 2, lambda d: d.steps >= 2 and d.ndir >= 2),
    "no_1_minus_g2": (lambda d: d.steps >= 1, lambda d: d.steps >= 1),
    "swap_i_f_derivatives": (lambda d: d.steps >= 1, None),             # EXACT: i = f and c_prev = 0
    "finished_updated": (lambda d: d.steps >= 1 and d.B >= 3, lambda d: d.steps >= 1 and d.B >= 3),
    "dout_wrong_step_reverse": (lambda d: d.steps >= 2 and d.ndir >= 2, lambda d: d.steps >= 2 and d.ndir >= 2),
    "next_from_prev": (lambda d: d.steps >= 2, lambda d: d.steps >= 2),
}


def test_the_ten_defects_are_the_references():
    assert sorted(CAN_SHOW) == sorted(R.DEFECTS) and len(R.DEFECTS) == 10


def _smallest(kind, can_show):
    cs = sorted((c for c in R.CASES if c[0] == kind), key=lambda c: (c[1] * c[2] * c[3] * c[4], c))
    for c in cs:
        if can_show(R.build_case(c)):
            return c
    raise AssertionError("no %s case can show this defect" % kind)


@pytest.mark.parametrize("kind", ["real", "exact"])
@pytest.mark.parametrize("defect", sorted(CAN_SHOW))
def test_the_check_refuses_a_defective_evaluation(defect, kind):
    can = CAN_SHOW[defect][kind == "exact"]
    if can is None:
        return                                                  # (the table above says why an EXACT case cannot show it)
    case = _smallest(kind, can)
    d = R.build_case(case)
    R.check_bwd_case(d, evaluate(d), R.case_id(case))           # the sound evaluation passes ...
    with pytest.raises(AssertionError) as e:                    # ... the defective one does not
        R.check_bwd_case(d, evaluate(d, defect), R.case_id(case))
    print("[lstmbwdref] %s at %s refused: %s" % (defect, R.case_id(case), str(e.value)[:150]))


@pytest.mark.parametrize("case", [c for i, c in enumerate(R.CASES) if i % 5 == 0], ids=R.case_id)
def test_the_check_accepts_the_sound_evaluation(case):
    d = R.build_case(case)
    stats = {}
    R.check_bwd_case(d, evaluate(d), R.case_id(case), stats)
    if d.kind == "real":
        assert stats["lstm_seq_bwd (dc_carry)"][1] < 1.0 and 0.3 < stats["lstm_seq_bwd (dgx, bf16)"][1] <= 1.0


def test_the_forward_check_accepts_the_reference_and_refuses_a_wrong_gate_order():
    case = ("real", 64, 17, 2, 5)
    d = R.build_case(case)
    fw = d.fwd
    used = np.repeat(R._consumed(d.gxi, d.rows_gx, d.ndir), d.Hp, axis=1)
    nanr = lambda a: np.where(np.isnan(a), np.float32("nan"), rowref.bf16_round(np.nan_to_num(a)))     # noqa: E731
    out = np.full(d.out0.shape, np.nan, np.float32)
    out[fw.written] = rowref.bf16_round(fw.out[fw.written])
    got = NS(out=out, gates=nanr(fw.gates), cs=fw.cs.astype(np.float32), hprev=nanr(fw.hprev))
    assert used.any()
    R.check_saved(d, got, "sound")
    bad = NS(**vars(got))
    g = got.gates.reshape(d.rows_gx, d.ndir, 4, d.Hp).copy()
    g[:, :, [1, 2]] = g[:, :, [2, 1]]
    bad.gates = g.reshape(got.gates.shape)
    with pytest.raises(AssertionError):
        R.check_saved(d, bad, "f and g swapped")
    bad = NS(**vars(got))
    bad.hprev = np.where(np.isnan(got.hprev), got.hprev, np.float32(0))
    with pytest.raises(AssertionError):
        R.check_saved(d, bad, "hprev all zero")


def test_sgd_references():
    rng = np.random.default_rng(5)
    p, g = rng.standard_normal(64), 10 * rng.standard_normal(64)
    gn = rowref.sqnorm(g)
    a, sh = R.sgd(p, g, 0.1, gn, 5.0, 0.5, n_shadow=32)
    norm = np.sqrt(gn) * 0.5
    assert norm > 5.0 and np.allclose(a, p - 0.1 * g * 0.5 * 5.0 / (norm + 1e-6), rtol=0, atol=1e-15)
    assert np.array_equal(sh, rowref.bf16_round(a.astype(np.float32)[:32]))
    b, _ = R.sgd(p, g, 0.1, None, 5.0, 0.5)
    assert np.allclose(b, p - 0.05 * g, rtol=0, atol=1e-15)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    tp.grad = torch.from_numpy(g * 0.5)
    torch.nn.utils.clip_grad_norm_([tp], 5.0)
    torch.optim.SGD([tp], lr=0.1).step()
    assert np.abs(tp.detach().numpy() - a).max() < 1e-12
    e = R.sgd32(p, g, 0.1, gn, 5.0, 0.5)
    assert e.dtype == np.float32 and 0 < np.abs(e - a).max() < 1e-5
