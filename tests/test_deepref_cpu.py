"""CPU: proves tests/deepref.py -- the references of the BiLSTM head with more than one layer and a trained initial state -- against
float64 torch autograd, and proves that the comparisons refuse nine defective evaluations.

The pin is torch: the reference's forward() calls .cuda() (flair/models/sequence_tagger_model.py:1028) and cannot run here, and its
recurrence is exactly torch.nn.LSTM(num_layers=L, bidirectional=True) over pack_padded_sequence(enforce_sorted=False), started from
lstm_init_h / lstm_init_c repeated over the batch (:317-357, 969-994).  Without masks the pin is that one module (dropout=0); with
masks between the layers it is single-layer torch.nn.LSTMs stacked by hand with the same masks, which is shown here to equal the
module when there is no mask."""
import numpy as np
import pytest
import torch

import deepref as DR
import lstmbwdref as R
import rowref

F64 = np.float64
LENGTHS = (7, 1, 4)
B, n, D, H = 3, 7, 5, 6


def problem(L, seed, init=True):
    rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    mod = torch.nn.LSTM(D, H, L, bidirectional=True).double()
    rnn = {k: 2.0 * v.detach().numpy() for k, v in mod.state_dict().items()}
    x = rng.standard_normal((B, n, D))
    for b in range(B):
        x[b, LENGTHS[b]:] = 0.0
    h0 = rng.standard_normal((2 * L, H)) if init else None
    c0 = rng.standard_normal((2 * L, H)) if init else None
    G = rng.standard_normal((B, n, 2 * H))
    keep = rng.random((max(L - 1, 1), B, n, 2 * H)) >= 0.5
    masks = [keep[k] * 2.0 for k in range(L - 1)]
    return R.NS(rnn=rnn, x=x, h0=h0, c0=c0, G=G, masks=masks, L=L)


def autograd(p, masks=None, module=False):
    y, params, h0, c0, x = DR.torch_stack(p.x, LENGTHS, p.rnn, p.L, p.h0, p.c0, masks, module=module)
    (y * torch.from_numpy(p.G)).sum().backward()
    g = {k: v.grad.numpy() for k, v in params.items()}
    return R.NS(y=y.detach().numpy(), g=g, dh0=None if h0 is None else h0.grad.numpy(), dc0=None if c0 is None else c0.grad.numpy(),
                dx=x.grad.numpy())


def agrees(res, t, L, tol=1e-10):
    """THE comparison of a deep_lstm evaluation with the autograd pin: output, every weight gradient, d h_0 and d c_0 summed over the
    batch, dx"""
    assert np.abs(res.y - t.y).max() < tol, "y"
    g = DR.rnn_grads(res, L)
    assert sorted(g) == sorted(t.g)
    for k in sorted(g):
        assert np.abs(g[k] - t.g[k]).max() < tol, k
    if t.dh0 is not None:
        assert np.abs(res.dh0 - t.dh0).max() < tol, "dh0"
        assert np.abs(res.dc0 - t.dc0).max() < tol, "dc0"
    assert np.abs(res.dx - t.dx).max() < tol, "dx"


@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_deep_lstm_equals_torch_lstm_autograd(L, init):
    p = problem(L, seed=10 * L + init, init=init)
    t = autograd(p, module=True)
    res = DR.deep_lstm(p.x, LENGTHS, DR.layer_weights(p.rnn, L), p.h0, p.c0, dy=p.G)
    agrees(res, t, L)
    # padded positions: zero output, no gradient
    for b in range(B):
        assert not res.y[b, LENGTHS[b]:].any() and not res.dx[b, LENGTHS[b]:].any()
    # the hand-stacked single-layer modules are the same function
    t2 = autograd(p, module=False)
    assert np.abs(t2.y - t.y).max() < 1e-12 and all(np.abs(t2.g[k] - t.g[k]).max() < 1e-12 for k in t.g)
    # the float32 restatement is the same formula
    r32 = DR.deep_lstm(p.x, LENGTHS, DR.layer_weights(p.rnn, L), p.h0, p.c0, dy=p.G, f=np.float32)
    assert r32.y.dtype == np.float32 and 0 < np.abs(r32.y - res.y).max() < 1e-4
    assert r32.dh0.dtype == np.float32 and np.abs(r32.dW[0][0][0] - res.dW[0][0][0]).max() < 1e-3 * np.abs(res.dW[0][0][0]).max()


@pytest.mark.parametrize("L", [2, 3])
def test_deep_lstm_with_masks_equals_hand_stacked_torch_lstms(L):
    p = problem(L, seed=20 + L)
    t = autograd(p, masks=p.masks)
    res = DR.deep_lstm(p.x, LENGTHS, DR.layer_weights(p.rnn, L), p.h0, p.c0, p.masks, dy=p.G)
    agrees(res, t, L)
    plain = autograd(p)
    assert np.abs(plain.y - t.y).max() > 1e-2           # the masks act
    # the last layer's output is unmasked: every element of a live position is non-zero
    assert (res.y[0] != 0).all()


@pytest.mark.parametrize("L", [2, 3])
def test_padded_operands_are_the_same_function(L):
    """hidden 6 on operands padded to 64 units: gate blocks, the initial state and an upper layer's input columns [0, H), [Hp, Hp + H)"""
    Hp = 64
    p = problem(L, seed=30 + L)
    t = autograd(p, masks=p.masks)
    W = DR.padded_weights(p.rnn, L, H, Hp)
    res = DR.deep_lstm(p.x, LENGTHS, W, DR.pad_init(p.h0, H, Hp), DR.pad_init(p.c0, H, Hp), [DR.pad_cols(m, H, Hp) for m in p.masks],
                       dy=DR.pad_cols(p.G, H, Hp))
    assert not res.y[..., H:Hp].any() and not res.y[..., Hp + H:].any() and not res.dh0[:, H:].any() and not res.dc0[:, H:].any()
    un = unpadded(res, L, Hp)
    agrees(un, t, L)


def unpadded(res, L, Hp):
    dW = []
    for k in range(L):
        row = []
        for d in range(2):
            dwih, dwhh, db = res.dW[k][d]
            dwih = DR.unpad_gates(dwih, H, Hp)
            if k > 0:
                dwih = DR.unpad_cols(dwih, H, Hp)
            row.append((dwih, DR.unpad_gates(dwhh, H, Hp)[:, :H], DR.unpad_gates(db, H, Hp)))
        dW.append(row)
    return R.NS(y=DR.unpad_cols(res.y, H, Hp), dW=dW, dh0=res.dh0[:, :H], dc0=res.dc0[:, :H], dx=res.dx)


# ====================================================================== the comparisons' power
def test_the_defect_list():
    assert len(DR.DEFECTS) == 9 and len(set(DR.DEFECTS)) == 9


@pytest.mark.parametrize("defect", ["init_index_dL_plus_k", "c0_ignored_in_df", "dh0_without_recurrent_product", "dc0_one_direction_only",
                                    "mask_on_last_layer", "mask_not_rescaled", "upper_reads_unmasked"])
def test_the_autograd_comparison_refuses_a_defective_evaluation(defect):
    L = 2
    p = problem(L, seed=40)
    t = autograd(p, masks=p.masks)
    W = DR.layer_weights(p.rnn, L)
    agrees(DR.deep_lstm(p.x, LENGTHS, W, p.h0, p.c0, p.masks, dy=p.G), t, L)                    # the sound evaluation passes ...
    with pytest.raises(AssertionError) as e:                                                     # ... the defective one does not
        agrees(DR.deep_lstm(p.x, LENGTHS, W, p.h0, p.c0, p.masks, dy=p.G, defect=defect), t, L)
    print("[deepref] %s refused at %s" % (defect, str(e.value)[:60]))


def test_the_autograd_comparison_refuses_upper_wih_columns_at_H_2H():
    L, Hp = 2, 64
    p = problem(L, seed=41)
    t = autograd(p, masks=p.masks)
    args = (DR.pad_init(p.h0, H, Hp), DR.pad_init(p.c0, H, Hp), [DR.pad_cols(m, H, Hp) for m in p.masks])
    agrees(unpadded(DR.deep_lstm(p.x, LENGTHS, DR.padded_weights(p.rnn, L, H, Hp), *args, dy=DR.pad_cols(p.G, H, Hp)), L, Hp), t, L)
    bad = DR.padded_weights(p.rnn, L, H, Hp, defect="upper_wih_cols_H_2H")
    with pytest.raises(AssertionError):
        agrees(unpadded(DR.deep_lstm(p.x, LENGTHS, bad, *args, dy=DR.pad_cols(p.G, H, Hp)), L, Hp), t, L)


def test_the_saved_state_comparison_refuses_an_unrounded_h0():
    """the device's recurrence starts from bf16(lstm_init_h): the emulation rounds there, and the forward kernel test compares the hprev
    rows of step 0 with bf16(h_0) bit for bit (deepref.check_h0_saved)"""
    L = 2
    p = problem(L, seed=42)
    W = DR.layer_weights(p.rnn, L)
    sound = DR.deep_lstm(p.x, LENGTHS, W, p.h0, p.c0, dy=p.G, store=DR.STORE)
    bad = DR.deep_lstm(p.x, LENGTHS, W, p.h0, p.c0, dy=p.G, store=DR.STORE, defect="h0_not_rounded")
    for k in range(L):
        for d in range(2):
            want = np.repeat(p.h0[2 * k + d][None], B, 0)
            DR.check_h0_saved(sound.hprev0[k][d], want)
            with pytest.raises(AssertionError):
                DR.check_h0_saved(bad.hprev0[k][d], want)


# ====================================================================== the emulation
@pytest.mark.parametrize("L", [1, 2, 3])
def test_the_emulation_is_the_reference_with_rounding_noise(L):
    p = problem(L, seed=50 + L)
    W = DR.layer_weights(p.rnn, L)
    bfx = DR.bf(p.x)
    ref = DR.deep_lstm(bfx, LENGTHS, W, p.h0, p.c0, p.masks or None, dy=p.G)
    emu = DR.deep_lstm(bfx, LENGTHS, W, p.h0, p.c0, p.masks or None, dy=DR.bf(p.G), store=DR.STORE)
    rel = lambda a, b: float(np.linalg.norm(a - b) / np.linalg.norm(b))          # noqa: E731
    assert 1e-4 < rel(emu.y, ref.y) < 2e-2
    assert np.array_equal(DR.bf(emu.y), emu.y)                                   # stored as bf16
    for a, b in ((emu.dh0, ref.dh0), (emu.dc0, ref.dc0), (emu.dW[L - 1][1][1], ref.dW[L - 1][1][1])):
        assert 1e-5 < rel(a, b) < 5e-2


def test_the_one_layer_emulation_without_initial_state_is_lstmbwdrefs():
    """deepref.head with L = 1 and no initial state rounds where lstmbwdref.emulate rounds: the two agree to summation order"""
    rng = np.random.default_rng(3)
    T = 6
    p = problem(1, seed=60, init=False)
    st = {"rnn": p.rnn, "linear.weight": rng.standard_normal((T, 2 * H)), "linear.bias": rng.standard_normal(T),
          "transitions": rng.standard_normal((T, T))}
    st["transitions"][T - 2, :] = -1e12
    st["transitions"][:, T - 1] = -1e12
    tags = rng.integers(0, T - 2, (B, n))
    x = DR.bf(p.x)
    la, ga = R.emulate(x, LENGTHS, tags, st, T - 2, T - 1)
    lb, gb, _ = DR.head(x, LENGTHS, tags, st, 1, T - 2, T - 1, store=DR.STORE)
    assert abs(la - lb) < 1e-6 * abs(la)
    for k in ga:
        assert np.linalg.norm(ga[k] - gb[k]) <= 2e-2 * np.linalg.norm(ga[k]), k
    l64, g64, _ = R.head_reference64(x, LENGTHS, tags, st, T - 2, T - 1)
    l2, g2, _ = DR.head_torch(x, LENGTHS, tags, st, 1, T - 2, T - 1)
    l3, g3, _ = DR.head(x, LENGTHS, tags, st, 1, T - 2, T - 1)
    assert abs(l64 - l2) < 1e-12 * abs(l64) and abs(l64 - l3) < 1e-10 * abs(l64)
    assert all(np.abs(g64[k] - g2[k]).max() < 1e-12 and np.abs(g64[k] - g3[k]).max() < 1e-9 for k in g64)


# ====================================================================== kbner_lstm_seq_bwd_init: cases and comparison
def test_init_case_list_covers_what_the_kernel_can_get_wrong():
    cases = DR.REAL_CASES + DR.EXACT_CASES
    assert {c[1] for c in cases} == {64, 128, 320} and {c[2] for c in DR.REAL_CASES} == {1, 17, 48, 65}
    assert {c[3] for c in cases} == {1, 2} and {c[4] for c in DR.REAL_CASES} == {1, 2, 5} and len(DR.EXACT_CASES) >= 1
    assert all((hp, b) in {(c[1], c[2]) for c in DR.REAL_CASES} for hp in (64, 128, 320) for b in (17, 48, 65))
    one = dead = False
    for c in cases:
        d = R.build_case(c)
        one |= bool(d.steps >= 2 and (d.lengths == 1).any())
        dead |= d.dead is not None
    assert one and dead


@pytest.mark.parametrize("case", DR.REAL_CASES + DR.EXACT_CASES + DR.ZERO_STEP_CASES, ids=R.case_id)
def test_init_check_accepts_the_sound_evaluation(case):
    ic = DR.init_case(case)
    stats = {}
    DR.check_init_case(ic, DR.evaluate_init(ic), R.case_id(case), stats)
    if ic.d.kind == "exact" and ic.d.steps:
        assert set(np.unique(ic.c0)) <= {-4.0, 0.0, 4.0} and (ic.c0 != 0).any()
        # c_0 acts: without it the f block of step 0 is zero, with it it is not
        got = DR.evaluate_init(ic)
        rows = ic.d.gxi[0, 0][ic.d.gxi[0, 0] >= 0]
        assert got.dgx[rows, ic.d.Hp:2 * ic.d.Hp].any()
    if ic.d.kind == "real":
        assert stats["lstm_seq_bwd_init (dh0)"][1] < 1.0 and stats["lstm_seq_bwd_init (dc_carry)"][1] < 1.0


@pytest.mark.parametrize("case", [("real", 64, 17, 1, 2), ("exact", 64, 17, 2, 2)], ids=R.case_id)
@pytest.mark.parametrize("defect", ["c0_ignored_in_df", "dh0_without_recurrent_product", "dh0_at_finished"])
def test_init_check_refuses_a_defective_evaluation(defect, case):
    ic = DR.init_case(case)
    with pytest.raises(AssertionError) as e:
        DR.check_init_case(ic, DR.evaluate_init(ic, defect), R.case_id(case))
    print("[deepref] %s at %s refused: %s" % (defect, R.case_id(case), str(e.value)[:120]))


def test_exact_init_cases_are_exact():
    for case in DR.EXACT_CASES:
        ic = DR.init_case(case)
        got = DR.evaluate_init(ic)
        used = ~np.isnan(got.dgx)
        assert np.array_equal(got.dgx[used] * 16, np.rint(got.dgx[used] * 16))
        first = ic.d.gxi[0] >= 0
        v = got.dh0[first].astype(F64)
        assert np.array_equal(v * 16, np.rint(v * 16)) and np.abs(v).max() * 16 < 2 ** 24
        # unrounded: the float64 walk with c_0 holds the same values (nothing was lost to the storage types)
        a = ic.aug
        dgx = np.full((a.rows_gx, ic.d.ndir * 4 * ic.d.Hp), np.nan)
        carry = ic.d.carry0.copy()
        for s in range(ic.d.steps - 1, -1, -1):
            stp = R.bwd_step(a, s + 1, dgx, carry)
            R._put(dgx, ic.d.Hp, stp, False)
            carry = stp.carry
        assert np.array_equal(np.nan_to_num(dgx[:ic.d.rows_gx]), np.nan_to_num(got.dgx.astype(F64)))
        assert np.array_equal(rowref.bf16_round(np.nan_to_num(dgx)).astype(F64), np.nan_to_num(dgx))
