"""GPU: kbner_lstm_seq_bwd_init (csrc/lstm_train.hip) -- the backward walk of a recurrence that started from a state -- through the C
ABI with test-owned, NaN-guarded buffers, against tests/deepref.py (check_init_case: lstmbwdref.bwd_step on a table with one virtual
step in front whose saved c is c_0; rowref.tolerance: float64 value, float32 restatement, sum_abs), and the forward kernels started
from a non-zero h[0] / c.

Cases (deepref.REAL_CASES / EXACT_CASES): Hp 64 / 128 / 320; B 1 / 17 / 48 / 65 (NT = 1, 2, 3, 4 and a second batch chunk); 1 and 2
directions; 1, 2 and 5 steps with sequences of length 1 (step 0 is also their last), one sequence that is never active (its dh0 and
carry come back bit for bit) and one that never stores; EXACT cases with c_0 in {0, +-4}.  Structure: c0 = dh0 = NULL is
kbner_lstm_seq_bwd bit for bit, steps = 0 writes nothing, rejected calls return EINVAL and write nothing.  Forward: kbner_lstm_seq_train
from a non-zero state against lstmref's reference (its cases carry h0 / c0), bit-equal to kbner_lstm_seq, hprev of step 0 = h_0.

Worst figures of the MI355X run that accompanied this module (29 tests, all passing, 4 s on its own; run with -s): `ratio` = kernel
error / float32 evaluation error (of which the rule allows 8), `share` = the largest fraction of its tolerance any element used.

    lstm_seq_bwd_init (dc_carry)       ratio 1.51   share 0.19       lstm_seq_bwd_init (dh0)          ratio 0.34   share 0.04
    lstm_seq_bwd_init (dgx, bf16)      -            share 0.992      lstm_seq_train (c_1 from c_0)    ratio 1.57   share 0.13
"""
import ctypes

import numpy as np
import pytest
import torch

import deepref as DR
import lstmbwdref as R
import lstmref

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
GUARD = 64
EINVAL = -22
WORST = {}


@pytest.fixture(scope="module")
def L():
    from kbner import lib as _L
    _L.load()
    yield _L
    print("\n[lstminit] worst per output (error ratio kernel / float32 evaluation, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[lstminit]   %-34s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def dev2d(a, dtype, pad_cols=0, extra_rows=2):
    a = np.asarray(a)
    full = torch.full((a.shape[0] + extra_rows, a.shape[1] + pad_cols), NAN, dtype=dtype, device=DEV)
    full[:a.shape[0], :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)
    return full


def flat(a, dtype, copies=1):
    a = np.asarray(a)
    full = torch.full((copies * a.size + GUARD,), NAN, dtype=dtype, device=DEV)
    full[:a.size] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV).reshape(-1)
    return full


def host(t):
    return t.detach().float().cpu().numpy()


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32).clone()


def tables(d):
    tab = (max(d.steps, 1), d.ndir, d.B)
    gxi = torch.full(tab, -1, dtype=I32, device=DEV)
    outi = torch.full(tab, -1, dtype=I32, device=DEV)
    gxi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.gxi)).to(DEV)
    outi[:d.steps] = torch.from_numpy(np.ascontiguousarray(d.outi)).to(DEV)
    # what the kernels index stays inside what they were given
    assert d.gxi.max(initial=-1) < d.rows_gx and d.outi.max(initial=-1) < d.rows_out
    assert all(c % 4 == 0 and c + d.Hp <= d.ldo for c in d.out_cols) and d.ldo % 4 == 0
    return gxi, outi, torch.tensor(d.out_cols, dtype=I32, device=DEV)


NAMES = ["dout", "ldo", "out_col", "outi", "gxi", "whht", "gates", "cs", "c0", "dc_carry", "dgx", "ld_dgx", "dh0", "steps", "B", "Hp", "ndir",
         "stream"]


class Bwd:
    """the device buffers of one kbner_lstm_seq_bwd_init case"""

    def __init__(self, ic):
        d = self.d = ic.d
        self.ic = ic
        K = d.ndir * 4 * d.Hp
        self.n = d.ndir * d.B * d.Hp
        self.gxi, self.outi, self.out_col = tables(d)
        self.dout = dev2d(d.dout, BF16)
        self.whht = flat(np.ascontiguousarray(d.whh.transpose(0, 2, 1)), BF16)
        self.gates = dev2d(d.gates, BF16, extra_rows=1)
        self.cs = dev2d(d.cs, F32, extra_rows=1)
        self.c0 = flat(ic.c0, F32)
        self.carry = flat(d.carry0, F32)
        self.dh0 = flat(ic.dh0_0, F32)
        self.dgx = torch.full((d.rows_gx + 2, K + 8), NAN, dtype=BF16, device=DEV)
        assert d.gates.shape == (d.rows_gx, K) and d.cs.shape == (d.rows_gx, d.ndir * d.Hp) and self.dgx.shape[1] % 8 == 0
        assert ic.c0.shape == ic.dh0_0.shape == d.carry0.shape == (d.ndir, d.B, d.Hp)

    def outputs(self):
        return [self.carry, self.dgx, self.dh0]

    def args(self, L, s0=0, carry_t=None, dgx_t=None, init=True, **kw):
        d = self.d
        off = 4 * s0 * d.ndir * d.B
        a = dict(dout=L.ptr(self.dout), ldo=self.dout.shape[1], out_col=L.ptr(self.out_col),
                 outi=ctypes.c_void_p(self.outi.data_ptr() + off), gxi=ctypes.c_void_p(self.gxi.data_ptr() + off), whht=L.ptr(self.whht),
                 gates=L.ptr(self.gates), cs=L.ptr(self.cs), c0=L.ptr(self.c0) if init else None,
                 dc_carry=L.ptr(self.carry if carry_t is None else carry_t), dgx=L.ptr(self.dgx if dgx_t is None else dgx_t),
                 ld_dgx=self.dgx.shape[1], dh0=L.ptr(self.dh0) if init else None, steps=d.steps - s0, B=d.B, Hp=d.Hp, ndir=d.ndir,
                 stream=L.stream_ptr())
        a.update(kw)
        assert list(a) == NAMES
        return list(a.values())

    def run(self, L):
        """-> got for deepref.check_init_case.  The carry every step started from is observed by running the tail of the walk (steps
        s .. steps - 1) on copies: a tail does not contain step 0, so it runs without c0 and dh0."""
        d, n = self.d, self.n
        after = [None] * d.steps + [host(self.carry[:n]).reshape(d.ndir, d.B, d.Hp)]
        for s0 in range(d.steps - 1, 0, -1):
            carry, dgx = self.carry.clone(), self.dgx.clone()
            L.call("kbner_lstm_seq_bwd_init", *self.args(L, s0=s0, carry_t=carry, dgx_t=dgx, init=False))
            after[s0] = host(carry[:n]).reshape(d.ndir, d.B, d.Hp)
        L.call("kbner_lstm_seq_bwd_init", *self.args(L))
        torch.cuda.synchronize()
        if d.steps:
            after[0] = host(self.carry[:n]).reshape(d.ndir, d.B, d.Hp)
        K = d.ndir * 4 * d.Hp
        assert bool(torch.isnan(self.carry[n:]).all()) and bool(torch.isnan(self.dh0[n:]).all()), "wrote behind dc_carry or dh0"
        assert bool(torch.isnan(self.dgx[d.rows_gx:]).all()) and bool(torch.isnan(self.dgx[:, K:]).all()), "wrote beside dgx"
        assert torch.equal(bits(self.c0[:n]), bits(flat(self.ic.c0, F32)[:n])), "c0 was written"
        return R.NS(dgx=host(self.dgx[:d.rows_gx, :K]), carry_after=after, dh0=host(self.dh0[:n]).reshape(d.ndir, d.B, d.Hp))


@pytest.mark.parametrize("case", DR.EXACT_CASES, ids=R.case_id)
def test_bwd_init_exact(L, case):
    ic = DR.init_case(case)
    DR.check_init_case(ic, Bwd(ic).run(L), R.case_id(case))


@pytest.mark.parametrize("case", DR.REAL_CASES, ids=R.case_id)
def test_bwd_init_real(L, case):
    ic = DR.init_case(case)
    got = Bwd(ic).run(L)
    DR.check_init_case(ic, got, R.case_id(case), WORST, print)
    d = ic.d
    if d.dead is not None:       # the never-active sequence: dh0 and the carry bit for bit
        assert (got.dh0[:, d.dead] == DR.DH0_GUARD).all() and (got.carry_after[0][:, d.dead] == R.CARRY_GUARD).all()


@pytest.mark.parametrize("case", [("real", 64, 17, 1, 2), ("real", 128, 65, 2, 2), ("real", 320, 48, 2, 5), ("exact", 64, 17, 2, 2)], ids=R.case_id)
def test_null_c0_and_dh0_is_kbner_lstm_seq_bwd_bit_for_bit(L, case):
    ic = DR.init_case(case)
    a, b = Bwd(ic), Bwd(ic)
    old = a.args(L, init=False)
    del old[NAMES.index("dh0")], old[NAMES.index("c0")]
    L.call("kbner_lstm_seq_bwd", *old)
    L.call("kbner_lstm_seq_bwd_init", *b.args(L, init=False))
    torch.cuda.synchronize()
    assert torch.equal(bits(a.dgx), bits(b.dgx)) and torch.equal(bits(a.carry), bits(b.carry))
    assert torch.equal(bits(b.dh0), bits(flat(ic.dh0_0, F32)))
    # and the plain walk is lstmbwdref's
    K = ic.d.ndir * 4 * ic.d.Hp
    assert np.isfinite(host(b.dgx[:ic.d.rows_gx, :K])[np.repeat(R._consumed(ic.d.gxi, ic.d.rows_gx, ic.d.ndir), 4 * ic.d.Hp, axis=1)]).all()


@pytest.mark.parametrize("case", DR.ZERO_STEP_CASES, ids=R.case_id)
def test_zero_steps_writes_nothing(L, case):
    ic = DR.init_case(case)
    buf = Bwd(ic)
    before = [bits(t) for t in buf.outputs()]
    got = buf.run(L)
    assert all(torch.equal(x, bits(t)) for x, t in zip(before, buf.outputs()))
    DR.check_init_case(ic, got, R.case_id(case))


def test_rejects_bad_arguments(L):
    ic = DR.init_case(("exact", 64, 17, 2, 2))
    buf = Bwd(ic)
    good = buf.args(L)
    ldo, ld = good[NAMES.index("ldo")], good[NAMES.index("ld_dgx")]
    bad = [({n: None}, "null " + n) for n in NAMES if isinstance(good[NAMES.index(n)], ctypes.c_void_p) and n not in ("stream", "c0", "dh0")]
    assert len(bad) == 9
    bad += [({"B": 0}, "B = 0"), ({"ndir": 0}, "ndir = 0"), ({"ldo": ldo + 2}, "ldo % 4"), ({"ld_dgx": ld + 4}, "ld_dgx % 8"),
            ({"ld_dgx": 2 * 4 * 64 - 8}, "ld_dgx < ndir * 4Hp"), ({"Hp": 96}, "Hp = 96"), ({"Hp": 32}, "Hp = 32"), ({"steps": -1}, "steps < 0")]
    for kw, what in bad:
        before = [bits(t) for t in buf.outputs()]
        rc = L.load().kbner_lstm_seq_bwd_init(*buf.args(L, **kw))
        torch.cuda.synchronize()
        assert rc == EINVAL, (what, rc)
        assert all(torch.equal(x, bits(t)) for x, t in zip(before, buf.outputs())), what
    DR.check_init_case(ic, buf.run(L), "after the rejected calls")


# ====================================================================== the forward kernels from a non-zero state
class Fwd:
    def __init__(self, d, h0, c0, rows_gx):
        self.d = d
        self.n = d.ndir * d.B * d.Hp
        self.gxi, self.outi, self.out_col = tables(d)
        self.gx = dev2d(d.gx, BF16, pad_cols=8)
        self.whh = flat(d.whh, BF16)
        self.h, self.c = flat(h0, BF16, copies=2), flat(c0, F32)
        self.out = torch.full((d.rows_out + 3, d.ldo), NAN, dtype=BF16, device=DEV)
        self.gates = torch.full((rows_gx + 1, d.ndir * 4 * d.Hp), NAN, dtype=BF16, device=DEV)
        self.cs = torch.full((rows_gx + 1, d.ndir * d.Hp), NAN, dtype=F32, device=DEV)
        self.hprev = torch.full((rows_gx + 1, d.ndir * d.Hp), NAN, dtype=BF16, device=DEV)

    def seq_args(self, L):
        d = self.d
        return [L.ptr(self.gx), self.gx.shape[1], L.ptr(self.gxi), L.ptr(self.whh), L.ptr(self.h), L.ptr(self.c), L.ptr(self.out), d.ldo,
                L.ptr(self.out_col), L.ptr(self.outi), d.steps, d.B, d.Hp, d.ndir]

    def run(self, L, train):
        if train:
            L.call("kbner_lstm_seq_train", *(self.seq_args(L) + [L.ptr(self.gates), L.ptr(self.cs), L.ptr(self.hprev), L.stream_ptr()]))
        else:
            L.call("kbner_lstm_seq", *(self.seq_args(L) + [L.stream_ptr()]))
        torch.cuda.synchronize()

    def got(self):
        d, n = self.d, self.n
        assert bool(torch.isnan(self.h[2 * n:]).all()) and bool(torch.isnan(self.c[n:]).all()) and bool(torch.isnan(self.out[d.rows_out:]).all())
        half = d.steps & 1
        return R.NS(h=host(self.h[half * n:(half + 1) * n]).reshape(d.ndir, d.B, d.Hp), c=host(self.c[:n]).reshape(d.ndir, d.B, d.Hp),
                    out=host(self.out[:d.rows_out]))


@pytest.mark.parametrize("case", [("seq", "real", 64, 17, 2, 5), ("seq", "real", 128, 49, 2, 2), ("seq", "real", 320, 65, 1, 1),
                                  ("seq", "exact", 64, 17, 2, 2), ("seq", "exact", 320, 33, 1, 5)], ids=lstmref.case_id)
def test_training_forward_from_a_nonzero_state_matches_the_reference(L, case):
    """lstmref's cases start from non-zero h0 / c0: kbner_lstm_seq_train gives what the reference gives, and what kbner_lstm_seq gives
    bit for bit (the row tables of these cases consume a gx row more than once: the saved state is not looked at here)"""
    d = lstmref.build_case(case)
    trn, inf = Fwd(d, d.h0, d.c0, d.rows_gx), Fwd(d, d.h0, d.c0, d.rows_gx)
    trn.run(L, True)
    inf.run(L, False)
    lstmref.check_case(d, trn.got(), lstmref.case_id(case), WORST, print)
    for a, b in ((trn.h, inf.h), (trn.c, inf.c), (trn.out, inf.out)):
        assert torch.equal(bits(a), bits(b))


@pytest.mark.parametrize("case", [("real", 64, 17, 2, 5), ("real", 128, 65, 2, 2), ("real", 320, 48, 1, 5), ("real", 64, 1, 2, 1)], ids=R.case_id)
def test_training_forward_saves_h0_as_hprev_of_step_0(L, case):
    """on tables inside the training contract (lstmbwdref's: every row consumed once): hprev of the row step 0 consumes is h_0 bit for
    bit -- so dWhh = dgx^T hprev holds the h_0 term --, hprev of a later step is the h the sequence emitted, the final c is the c_t
    saved at the sequence's last step, and a sequence that is never active keeps h_0 and c_0"""
    d = R.build_case(case)
    rng = np.random.default_rng([11, d.Hp, d.B])
    h0 = DR.bf(rng.uniform(-1, 1, size=(d.ndir, d.B, d.Hp)))
    c0 = DR.f32(rng.standard_normal((d.ndir, d.B, d.Hp)))
    buf = Fwd(d, h0, c0, d.rows_gx)
    buf.run(L, True)
    got = buf.got()
    hprev, cs, Hp = host(buf.hprev[:d.rows_gx]), host(buf.cs[:d.rows_gx]), d.Hp
    assert bool(torch.isnan(buf.hprev[d.rows_gx:]).all()) and bool(torch.isnan(buf.cs[d.rows_gx:]).all()) and bool(torch.isnan(buf.gates[d.rows_gx:]).all())
    used = np.repeat(R._consumed(d.gxi, d.rows_gx, d.ndir), Hp, axis=1)
    assert np.isnan(hprev[~used]).all() and np.isfinite(hprev[used]).all()
    for dd in range(d.ndir):
        a = np.nonzero(d.gxi[0, dd] >= 0)[0]
        DR.check_h0_saved(hprev[d.gxi[0, dd, a], dd * Hp:(dd + 1) * Hp], h0[dd, a], R.case_id(case))
        for s in range(1, d.steps):
            a = np.nonzero((d.gxi[s, dd] >= 0) & (d.outi[s - 1, dd] >= 0))[0]
            seen = got.out[d.outi[s - 1, dd, a], d.out_cols[dd]:d.out_cols[dd] + Hp]
            assert R._bits_equal(hprev[d.gxi[s, dd, a], dd * Hp:(dd + 1) * Hp], seen)
        for b in range(d.B):
            if d.lengths[b]:
                assert R._bits_equal(got.c[dd, b], cs[d.gxi[d.lengths[b] - 1, dd, b], dd * Hp:(dd + 1) * Hp])
            else:
                assert R._bits_equal(got.h[dd, b], h0[dd, b]) and R._bits_equal(got.c[dd, b], c0[dd, b])
    # the first step against the one-step reference started from (h_0, c_0): c_1 under the single-step rule
    import rowref
    r = lstmref.step(np.nan_to_num(d.gx), d.gxi[0], d.whh, h0, c0, d.outi[0], np.full((d.rows_out, d.ldo), NAN), d.out_cols)
    h32, c32 = lstmref.eval32(np.nan_to_num(d.gx), d.gxi[0], d.whh, h0, c0)
    act = d.gxi[0] >= 0
    c1 = np.stack([np.stack([cs[max(d.gxi[0, dd, b], 0), dd * Hp:(dd + 1) * Hp] for b in range(d.B)]) for dd in range(d.ndir)])
    tol, err32 = rowref.tolerance(r.c[act], c32[act], r.sum_abs_c[act])
    lstmref._share("lstm_seq_train (c_1 from c_0)", R.case_id(case), np.abs(c1 - r.c)[act], tol, err32, False, WORST, print)
