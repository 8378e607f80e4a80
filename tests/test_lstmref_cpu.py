"""CPU: proves tests/lstmref.py -- the float64 LSTM references against torch.nn.LSTM, the conditions of the EXACT (switchboard)
inputs for every case tests/test_gpu_lstm_kernels.py runs, and the power of the comparison that module uses
(lstmref.check_case): eleven defective evaluations of the reference, each the kind of mistake one wrong tile, wave or branch of
csrc/lstm.hip would make, are refused by the EXACT and by the REAL check at the smallest case that can show them.

Switchboard shares reached over the 46 EXACT cases (asserted below: >= 1/4 and both sides in every tile): the product h Whh^T
decides the gate's side in 56.7 % to 72.5 % of the pre-activations of a case (gx decides the rest, so a wrong gx row or column
flips gates too); within every 16-unit x 16-sequence tile of every direction at least 13 product-decided gates fall on the rarer
side (printed per case with -s).
"""
import numpy as np
import pytest
import torch

import lstmref as R
import rowref

F64 = np.float64


# ====================================================================== the references against torch.nn.LSTM (float64)
def _torch_lstm(D, H, bidirectional, seed):
    torch.manual_seed(seed)
    rnn = torch.nn.LSTM(D, H, 1, bidirectional=bidirectional, batch_first=True).double()
    with torch.no_grad():
        for p in rnn.parameters():
            p.mul_(3.0)                      # out of the linear range of the gates
    return rnn


def _gx_of(rnn, x, sfxs):
    """pre-activations Wih x + bih + bhh of every row of x [rows, D], direction d at column d * 4H"""
    sd = {k: v.detach().numpy() for k, v in rnn.state_dict().items()}
    return np.concatenate([x @ sd["weight_ih_l0" + s].T + sd["bias_ih_l0" + s] + sd["bias_hh_l0" + s] for s in sfxs], 1), sd


def test_step_and_seq_equal_torch_unidirectional_with_initial_state():
    B, n, D, H = 5, 7, 6, 12
    rng = np.random.default_rng(1)
    rnn = _torch_lstm(D, H, False, 1)
    x, h0, c0 = rng.standard_normal((B, n, D)), rng.standard_normal((1, B, H)), rng.standard_normal((1, B, H))
    with torch.no_grad():
        y, (hn, cn) = rnn(torch.from_numpy(x), (torch.from_numpy(h0), torch.from_numpy(c0)))
    gx, sd = _gx_of(rnn, x.reshape(B * n, D), [""])
    tab = (np.arange(B)[None, :] * n + np.arange(n)[:, None])[:, None, :]          # row b * n + t at step t
    whh = sd["weight_hh_l0"][None]
    r = R.seq(gx, tab, whh, h0, c0, tab, np.zeros((B * n, H)), [0])
    assert np.abs(r.out.reshape(B, n, H) - y.numpy()).max() < 1e-12
    assert np.abs(r.h - hn.numpy()).max() < 1e-12 and np.abs(r.c - cn.numpy()).max() < 1e-12
    assert r.written.all()
    one = R.step(gx, tab[0], whh, h0, c0, tab[0], np.zeros((B * n, H)), [0])       # a single step, on its own
    assert np.abs(one.h[0] - y.numpy()[:, 0]).max() < 1e-12
    assert np.array_equal(one.written.reshape(B, n, H)[:, 1:], np.zeros((B, n - 1, H), bool))
    assert (one.sum_abs >= np.abs(one.pre)).all() and (one.sum_abs_h >= one.sum_abs_c).all()


def test_seq_equals_torch_bidirectional_packed_with_step_tables():
    from kbner.stack import step_tables
    B, n, D, H = 6, 9, 5, 8
    rng = np.random.default_rng(2)
    rnn = _torch_lstm(D, H, True, 2)
    lengths = np.array([9, 1, 4, 9, 2, 7])
    x = rng.standard_normal((B, n, D))
    for b in range(B):
        x[b, lengths[b]:] = 0.0
    packed = torch.nn.utils.rnn.pack_padded_sequence(torch.from_numpy(x), torch.from_numpy(lengths), batch_first=True, enforce_sorted=False)
    with torch.no_grad():
        y, (hn, cn) = rnn(packed)
    y, _ = torch.nn.utils.rnn.pad_packed_sequence(y, batch_first=True, total_length=n)
    gx, sd = _gx_of(rnn, x.reshape(B * n, D), ["", "_reverse"])
    tab = step_tables(lengths, n)
    assert tab.shape == (n, 2, B) and (tab[0] >= 0).all() and (tab[-1, :, 1] == -1).all()
    whh = np.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]])
    z = np.zeros((2, B, H))
    r = R.seq(gx, tab, whh, z, z, tab, np.zeros((B * n, 2 * H + 3)), [0, H + 3])
    got = np.concatenate([r.out[:, :H], r.out[:, H + 3:]], 1).reshape(B, n, 2 * H)
    assert np.abs(got - y.numpy()).max() < 1e-12                                   # padded positions: zero in both
    assert np.abs(r.h - hn.numpy()).max() < 1e-12 and np.abs(r.c - cn.numpy()).max() < 1e-12
    assert not r.written[:, H:H + 3].any()
    for b in range(B):
        assert not r.written.reshape(B, n, -1)[b, lengths[b]:].any()


def test_padded_hidden_units_stay_zero():
    """hidden 12 padded to 64 the way kbner.stack.LSTMGroup pads Whh and the gate blocks: units 12 .. 63 stay exactly 0"""
    from kbner.stack import LSTMGroup
    B, n, D, H = 4, 6, 5, 12
    rng = np.random.default_rng(3)
    rnn = _torch_lstm(D, H, False, 3)
    x = rng.standard_normal((B, n, D))
    with torch.no_grad():
        y, (hn, cn) = rnn(torch.from_numpy(x))
    gx, sd = _gx_of(rnn, x.reshape(B * n, D), [""])
    grp = LSTMGroup.__new__(LSTMGroup)
    grp.H, grp.Hp = H, 64
    Hp = grp.Hp
    gxp = grp.pad_gates(torch.from_numpy(gx.T.copy())).numpy().T.astype(F64)                     # [rows, 4Hp]
    whh = np.zeros((1, 4 * Hp, Hp))
    whh[0, :, :H] = grp.pad_gates(torch.from_numpy(sd["weight_hh_l0"])).numpy()
    tab = (np.arange(B)[None, :] * n + np.arange(n)[:, None])[:, None, :]
    z = np.zeros((1, B, Hp))
    r = R.seq(gxp.astype(np.float32).astype(F64), tab, whh.astype(np.float32).astype(F64), z, z, tab, np.zeros((B * n, Hp)), [0])
    assert np.abs(r.out.reshape(B, n, Hp)[:, :, :H] - y.numpy()).max() < 1e-5      # (pad_gates is float32)
    assert np.abs(r.c[0, :, :H] - cn.numpy()[0]).max() < 1e-5
    assert not r.out[:, H:].any() and not r.h[:, :, H:].any() and not r.c[:, :, H:].any()


def test_rounded_run_differs_from_the_mathematical_one_only_by_the_rounding():
    d = R.build_case(("seq", "real", 64, 17, 3, 5))
    a = R.seq(d.gx, d.gxi, d.whh, d.h0, d.c0, d.outi, d.out0, d.out_cols, round_h=False)
    b = R.seq(d.gx, d.gxi, d.whh, d.h0, d.c0, d.outi, d.out0, d.out_cols, round_h=True)
    assert np.array_equal(b.h, rowref.bf16_round(b.h)) and not np.array_equal(a.h, rowref.bf16_round(a.h))
    assert np.array_equal(a.written, b.written) and 0 < np.abs(a.h - b.h).max() < 0.05


def test_eval32_is_the_step_formula_in_float32():
    d = R.build_case(("step", "real", 96, 17, 3, 1))
    r = R.step(d.gx, d.gxi[0], d.whh, d.h0, d.c0, d.outi[0], d.out0, d.out_cols)
    h32, c32 = R.eval32(d.gx, d.gxi[0], d.whh, d.h0, d.c0)
    assert h32.dtype == c32.dtype == np.float32
    assert 0 < np.abs(c32 - r.c).max() < 1e-5 and 0 < np.abs(h32 - r.h).max() < 1e-5
    dead = ~r.act
    assert dead.any() and np.array_equal(h32[dead], d.h0[dead]) and np.array_equal(c32[dead], d.c0[dead])


# ====================================================================== the case list
def test_case_list_covers_what_it_says():
    for entry, hps, bs in (("step", (32, 64, 96, 160), (1, 15, 16, 17, 33)), ("seq", (64, 128, 192, 256, 320, 576), (1, 16, 17, 32, 33, 48, 49, 64, 65, 70))):
        for kind in ("exact", "real"):
            cs = [c for c in R.CASES if c[0] == entry and c[1] == kind]
            shapes = {(c[2], c[3]) for c in cs}
            assert all((hp, b) in shapes for hp in hps for b in (17, 49)), (entry, kind)
            assert all((hp, b) in shapes for b in bs for hp in (64, 320)), (entry, kind)
            assert {c[4] for c in cs} == {1, 2, 3}
        assert {c[5] for c in R.CASES if c[0] == "seq" and c[1] == "real"} == {1, 2, 5, 8}
        assert {c[5] for c in R.CASES if c[0] == "seq" and c[1] == "exact"} == {1, 2, 5, 8}
    assert len(set(R.CASES)) == len(R.CASES) and all(c[5] == 0 for c in R.ZERO_STEP_CASES)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_row_tables_hold_what_the_cases_need(case):
    d = R.build_case(case)
    act = d.gxi >= 0
    assert d.gxi.shape == d.outi.shape == (d.steps, d.ndir, d.B) and d.gxi.dtype == d.outi.dtype == np.int32
    assert d.gxi.max() < d.rows_gx and d.outi.max() < d.rows_out and max(d.out_cols) + d.Hp <= d.ldo
    assert all(c % 4 == 0 for c in d.out_cols) and d.ldo % 4 == 0
    assert not (~act & (d.outi >= 0)).any()                                    # a finished sequence stores nothing
    assert act[0].any(axis=0).all() or d.B >= 3
    if d.B >= 3:
        assert not act[:, :, d.dead].any()                                     # inactive from step 0
        if d.mute is not None:
            assert act[:, :, d.mute].all() and (d.outi[:, :, d.mute] == -1).all()
        assert (d.mute is not None) == (d.kind == "exact" or d.steps == 1)
    if d.steps >= 2 and d.B >= 15:
        assert len(set(d.lengths.tolist())) >= 3                               # sequences finish at different steps
    named = d.gxi[act]
    assert len(named) > len(np.unique(named)) or d.B * d.steps <= 2            # several sequences consume one gx row
    rows = d.outi[d.outi >= 0]
    for dd in range(d.ndir):                                                   # every step's h has an out row of its own
        r = d.outi[:, dd][d.outi[:, dd] >= 0]
        assert len(r) == len(np.unique(r))
    if d.ndir >= 2 and d.steps >= 2:                                           # the reversed order of the backward direction
        b = int(np.argmax(d.lengths))
        assert np.array_equal(d.outi[:d.lengths[b], 1, b], d.outi[:d.lengths[b], 0, b][::-1]) or b == d.mute
    assert np.isnan(d.gx).any() and len(rows) <= d.rows_out * d.ndir
    assert np.abs(d.h0).max() > 0 and np.abs(d.c0).max() > 0
    if d.entry == "seq" and d.ndir == 3:
        assert d.out_cols[2] - d.out_cols[1] != d.out_cols[1] - d.out_cols[0]
    if d.entry == "step":
        assert d.out_dir_stride != d.Hp and d.out_dir_stride % 4 == 0 and d.out_cols[0] > 0


# ====================================================================== the switchboard's conditions, every EXACT case
def _tiles(mask):
    """[ndir, B, 4, Hp] -> per (direction, sequence tile of 16, unit tile of 16) the number of True"""
    ndir, B, _, Hp = mask.shape
    Bp = (B + 15) // 16 * 16
    m = np.zeros((ndir, Bp, 4, Hp), np.int64)
    m[:, :B] = mask
    return m.reshape(ndir, Bp // 16, 16, 4, Hp // 16, 16).sum(axis=(2, 3, 5))


@pytest.mark.parametrize("case", R.EXACT_CASES + R.ZERO_STEP_CASES, ids=R.case_id)
def test_switchboard_conditions(case):
    d = R.build_case(case)
    assert np.array_equal(d.whh % 65536, np.zeros_like(d.whh)) and np.abs(d.whh).max() <= 65536 * R.SWITCH_M and (d.whh == 0).any()
    assert np.array_equal(rowref.bf16_round(d.whh), d.whh) and np.array_equal(rowref.bf16_round(d.h0), d.h0)
    read = ~np.isnan(d.gx)
    assert np.array_equal(np.abs(d.gx[read]) % 256, np.full(read.sum(), 128.0)) and np.array_equal(rowref.bf16_round(d.gx[read]), d.gx[read])
    assert np.array_equal(d.c0, np.rint(d.c0)) and np.isin(np.abs(d.h0) * 256, R.H_VALUES * 256).all()
    assert d.ref.c_snap < 1e-50 and np.array_equal(d.ref.c, np.rint(d.ref.c))
    if d.steps == 0:
        assert np.array_equal(d.ref.h, d.h0) and np.array_equal(d.ref.c, d.c0) and not d.ref.written.any()
        return
    h_in = d.h0
    decided = total = 0
    pos = np.zeros((d.ndir, (d.B + 15) // 16, d.Hp // 16), np.int64)
    neg = np.zeros_like(pos)
    for s, r in enumerate(d.ref.steps):
        a = r.act[:, :, None, None] & np.ones(r.pre.shape, bool)
        assert np.array_equal(h_in * 256, np.rint(h_in * 256))                 # h = j / 256: every product w h is a multiple of 256
        assert r.sum_abs.max() < 2 ** 31                                       # every partial sum, in any order, is below 2^31 < 2^32
        assert (np.abs(r.pre[a]) >= 128).all() and np.array_equal(np.abs(r.pre[a]) % 256, np.full(a.sum(), 128.0))
        g, _ = R._gather_gx(d.gx, d.gxi[s], d.Hp)
        g = g.reshape(r.pre.shape)
        prod = r.pre - g
        assert np.array_equal(prod % 256, np.zeros_like(prod))
        by_product = a & (np.abs(prod) > np.abs(g))
        decided += int(by_product.sum())
        total += int(a.sum())
        pos += _tiles(by_product & (r.pre > 0))
        neg += _tiles(by_product & (r.pre < 0))
        # tanh(c') of the states that are rounded: at least 2^-12 (relative) from a bf16 rounding midpoint
        c1 = np.rint(r.c[r.act])
        assert np.abs(c1 - r.c[r.act]).max() < 1e-50
        t = np.abs(np.tanh(c1[c1 != 0]))
        ulp = 2.0 ** (np.floor(np.log2(t)) - 7)
        assert ((ulp / 2 - np.abs(t - rowref.bf16_round(t))) >= 2.0 ** -12 * t).all()
        h_in = rowref.bf16_round(r.h).astype(F64)
    share = decided / total
    live = _tiles((d.gxi >= 0).any(axis=0)[:, :, None, None] & np.ones((d.ndir, d.B, 4, d.Hp), bool)) > 0
    rarer = np.minimum(pos, neg)[live]
    print("[lstmref] %s: product decides %.3f of %d gates; rarer side per tile >= %d" % (R.case_id(case), share, total, rarer.min()))
    assert share >= 0.25
    assert rarer.min() >= 1


# ====================================================================== the check's power
def _first_row(gxi, dd):
    r = gxi[:, dd]
    return int(r[r >= 0][0])


def evaluate(d, defect=None):
    """The reference run of case d as a kernel would leave it in memory (ping-pong h, c float32, h bf16), with one defect."""
    gx, whh, gxi, outi, cols = d.gx, d.whh, d.gxi, d.outi, list(d.out_cols)
    Hp, B, ndir, steps = d.Hp, d.B, d.ndir, d.steps
    if defect == "drop_k_slice":             # one 64-wide K slice of one wave, in one 16-unit tile of one direction
        whh = whh.copy()
        for q in range(4):
            whh[ndir - 1, q * Hp + Hp - 16:q * Hp + Hp, Hp - 64:Hp] = 0
    elif defect == "three_partials":         # wave 3's partial sums (k slices 3, 7, ...) never added
        whh = whh.copy()
        whh[:, :, (np.arange(Hp) // 64) % 4 == 3] = 0
    elif defect == "swap_f_g":
        gx, whh = gx.copy(), whh.copy()
        for dd in range(ndir):
            o = dd * 4 * Hp
            gx[:, o + Hp:o + 2 * Hp], gx[:, o + 2 * Hp:o + 3 * Hp] = d.gx[:, o + 2 * Hp:o + 3 * Hp], d.gx[:, o + Hp:o + 2 * Hp]
        whh[:, Hp:2 * Hp], whh[:, 2 * Hp:3 * Hp] = d.whh[:, 2 * Hp:3 * Hp], d.whh[:, Hp:2 * Hp]
    elif defect == "gx_direction_0":
        gx = np.concatenate([d.gx[:, :4 * Hp]] * ndir, 1)
    elif defect == "out_col_equidistant":
        cols[1] = cols[0] + Hp
    elif defect == "mute_frozen":
        gxi = np.where(outi < 0, -1, gxi).astype(np.int32)
    hbuf = [d.h0.copy(), np.full(d.h0.shape, np.nan)]
    c, out = d.c0.copy(), d.out0.copy()
    written = np.zeros(out.shape, bool)
    for s in range(steps):
        h_in = hbuf[s & 1]
        h_mm = h_in.copy()
        if defect == "tile1_reads_tile0":
            h_mm[:, 16:min(B, 32)] = h_in[:, :min(B, 32) - 16]
        elif defect == "clamp_row_15":
            h_mm[:, 16:] = h_in[:, 15:16]
        r = R.step(gx, gxi[s], whh, h_in, c, outi[s], out, cols, h_mm=h_mm)
        h_new = rowref.bf16_round(r.h).astype(F64)
        out = r.out
        out[r.written] = rowref.bf16_round(out[r.written])
        written |= r.written
        c_new = r.c
        if defect == "finished_c_updated":
            rows = np.stack([np.where(gxi[s, dd] < 0, _first_row(d.gxi, dd), gxi[s, dd]) for dd in range(ndir)])
            c_new = np.where(r.act[:, :, None], r.c, R.step(gx, rows, whh, h_in, c, outi[s], out, cols).c)
        if defect == "finished_h_not_copied":
            h_new[~r.act] = hbuf[(s + 1) & 1][~r.act]
        hbuf[(s + 1) & 1], c = h_new, c_new
    h = hbuf[(steps + 1) & 1] if defect == "final_from_other_half" else hbuf[steps & 1]
    got = R.as_stored(np.nan_to_num(h, nan=0.0), c, out, written)
    got.h[np.isnan(h)] = np.nan
    return got


def _stale_half_shows(d):
    """a finished (or never active) sequence whose last copy lands in the half that is not read at the end"""
    return bool(((d.steps - d.lengths) % 2 == 1).any())


# defect -> which cases can show it
DEFECTS = {
    "drop_k_slice": lambda d: d.entry == "seq",
    "three_partials": lambda d: d.entry == "seq" and d.Hp >= 256,
    "swap_f_g": lambda d: True,
    "tile1_reads_tile0": lambda d: d.entry == "seq" and d.B >= 17,
    "clamp_row_15": lambda d: d.B >= 17,
    "finished_c_updated": lambda d: d.B >= 3,
    "finished_h_not_copied": lambda d: d.entry == "seq" and _stale_half_shows(d),
    "final_from_other_half": lambda d: d.entry == "seq",
    "out_col_equidistant": lambda d: d.entry == "seq" and d.ndir >= 2,
    "gx_direction_0": lambda d: d.ndir >= 2,
    "mute_frozen": lambda d: d.mute is not None,
}


def _smallest(kind, can_show):
    cs = sorted((c for c in R.CASES if c[1] == kind), key=lambda c: (c[2] * c[3] * c[4] * c[5], c))
    for c in cs:
        if can_show(R.build_case(c)):
            return c
    raise AssertionError("no %s case can show this defect" % kind)


def test_there_are_eleven_defects():
    assert len(DEFECTS) == 11


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_the_check_refuses_a_defective_evaluation(defect, kind):
    case = _smallest(kind, DEFECTS[defect])
    d = R.build_case(case)
    R.check_case(d, evaluate(d), R.case_id(case))               # the sound evaluation passes ...
    with pytest.raises(AssertionError) as e:                    # ... the defective one does not
        R.check_case(d, evaluate(d, defect), R.case_id(case))
    print("[lstmref] %s at %s refused: %s" % (defect, R.case_id(case), str(e.value)[:150]))


@pytest.mark.parametrize("case", [c for i, c in enumerate(R.CASES) if i % 7 == 0], ids=R.case_id)
def test_the_check_accepts_the_sound_evaluation(case):
    d = R.build_case(case)
    stats = {}
    R.check_case(d, evaluate(d), R.case_id(case), stats)
    if d.kind == "real":           # a float64 evaluation rounded once for storage: float32's half ulp of c, bf16's half ulp of h
        (ck,) = [k for k in stats if k.startswith("lstm_%s (c" % d.entry)]
        assert stats[ck][1] < 1.0 and 0.3 < stats["lstm_%s (h_t, bf16)" % d.entry][1] <= 1.0
