"""GPU: the character BiLSTM kernels (csrc/char_lstm.hip: kbner_char_lstm_fwd, kbner_char_lstm_bwd) against the float64 restatement
of tests/charref.py (which tests/test_charref_cpu.py proves against torch autograd), under rowref.tolerance, in test-owned NaN-guarded
buffers.

Per case: the UNMASKED forward (null workspace: forward only) against charref under the tolerance with the bf16 term; the MASKED forward
(with a workspace) bit-equal to bf16(unmasked * mask) with charref's mask -- the kernel rounds h once and the masks multiply the rounded
value, so a second tolerance would only hide a wrong key -- and bit-equal to ops.gather_rows_drop over the unmasked matrix (the parity
the placement rule of the stacked tagger rests on); everything around the block (its pad columns, rows no word names, the rows behind the
matrix) stays NaN; the backward ADDS to pre-filled gradient buffers and is compared under the tolerance (fp32 atomics: no bit compare).
Cases: every (E, Hc) of {(25, 25), (8, 8), (32, 32), (16, 24)}, W of {1, 5, 67, 300}, Lmax of {1, 5, 33} (lengths 1 and Lmax present),
V = 3 (every id collides) and 97, rows non-contiguous with some -1, masks off / element / locked / both; W = 1030 and 530 make a wave
walk more than one word in the forward and in the backward launch.  Rejected calls return -22 and write nothing.
The module prints, under -s, the worst error ratio (kernel / float32 evaluation) and tolerance share per output.
"""
import ctypes

import numpy as np
import pytest
import torch

import charref as C
import mmaref
import rowref

pytestmark = pytest.mark.gpu

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
DEV = "cuda"
NAN = float("nan")
GUARD = 64
EINVAL = -22
G0 = 0.5              # what the gradient buffers hold before the backward adds to them
WORST = {}

SITES = {"off": ((0, 0), (0, 0)), "element": ((21, mmaref.dropout_thresh(0.25)), (0, 0)),
         "locked": ((0, 0), (22, mmaref.dropout_thresh(0.5))), "both": ((23, mmaref.dropout_thresh(0.25)), (24, mmaref.dropout_thresh(0.5)))}
# (E, Hc, W, Lmax, V, sites)
CASES = [(25, 25, 300, 33, 97, "both"), (25, 25, 67, 5, 3, "off"), (25, 25, 1, 5, 97, "element"), (25, 25, 5, 1, 3, "locked"),
         (8, 8, 1, 1, 3, "element"), (8, 8, 5, 5, 97, "locked"), (8, 8, 300, 1, 97, "off"), (8, 8, 67, 33, 3, "both"),
         (32, 32, 67, 33, 3, "both"), (32, 32, 300, 5, 97, "off"), (32, 32, 1, 33, 97, "locked"), (32, 32, 5, 1, 3, "element"),
         (16, 24, 5, 33, 97, "element"), (16, 24, 67, 1, 3, "locked"), (16, 24, 300, 5, 3, "both"), (16, 24, 1, 5, 97, "off"),
         (8, 8, 1030, 2, 3, "both"), (4, 5, 530, 3, 97, "element")]


def test_case_list_covers_what_it_says():
    assert {(c[0], c[1]) for c in CASES} >= {(25, 25), (8, 8), (32, 32), (16, 24)}
    for dims in ((25, 25), (8, 8), (32, 32), (16, 24)):
        mine = [c for c in CASES if (c[0], c[1]) == dims]
        assert {c[2] for c in mine} >= {1, 5, 67, 300} and {c[3] for c in mine} >= {1, 5, 33} and {c[4] for c in mine} == {3, 97}
        assert {c[5] for c in mine} == set(SITES)
    assert any(c[2] > 4 * 256 for c in CASES) and any(c[2] > 4 * 128 for c in CASES)      # a second word per wave, fwd and bwd


@pytest.fixture(scope="module")
def L():
    from kbner import lib as _L
    _L.load()
    yield _L
    print("\n[chark] worst per output (error ratio kernel / float32 evaluation, largest share of the tolerance used):")
    for k in sorted(WORST):
        print("[chark]   %-8s ratio %8.3f   share %6.3f" % (k, WORST[k][0], WORST[k][1]))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def dev(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)


def flat(a, fill=None):
    """f32 device buffer holding `a` (or `fill` in its shape) with a NaN guard behind it"""
    a = np.asarray(a)
    full = torch.full((a.size + GUARD,), NAN, dtype=F32, device=DEV)
    full[:a.size] = dev(a).reshape(-1) if fill is None else fill
    return full


def bits(t):
    return t.contiguous().view(torch.int16)


class Case:
    def __init__(self, case, seed=0):
        from kbner import ops
        self.E, self.Hc, self.W, self.Lmax, self.V, self.sites = case
        rng = np.random.default_rng(seed + 1000 * self.W + self.Lmax)
        self.n = 5
        self.R = (2 * self.W + 3 + self.n - 1) // self.n * self.n                      # rows of the matrix: [B, n]
        self.col = 32
        self.ld = self.col + (2 * self.Hc + 31) // 32 * 32 + 8
        self.p = C.params(rng, self.V, self.E, self.Hc)
        self.chars, self.lens, self.rows = C.tables(rng, self.W, self.Lmax, self.V, self.R, dropped=0.2 if self.W >= 5 else 0.0)
        self.de, self.dl = SITES[self.sites]
        self.mask = C.block_mask(self.rows, self.n, self.col, self.Hc, self.de, self.dl)
        self.dout = rowref.bf16_round(rng.standard_normal((self.W, 2 * self.Hc)).astype(np.float32))
        self.tab = ops.CharTables(self.chars, self.lens, self.rows, self.V, self.R, DEV)
        self.par = [dev(a) for a in (self.p.emb, self.p.wih, self.p.whh, self.p.bih, self.p.bhh)]
        self.blk = slice(self.col, self.col + 2 * self.Hc)
        self.live = self.rows >= 0

    def matrix(self, fill):
        """[R + 2, ld] bf16; the ops see the first R rows"""
        return torch.full((self.R + 2, self.ld), fill, dtype=BF16, device=DEV)

    def fwd(self, fill, masked, ws=None):
        from kbner import ops
        m = self.matrix(fill)
        de, dl = (self.de, self.dl) if masked else ((0, 0), (0, 0))
        ops.char_lstm_fwd(*self.par, self.tab, m[:self.R], self.col, self.n, de, dl, ws=ws)
        return m

    def block_of(self, m):
        """float32 [W, 2Hc]: word w's block, NaN for a dropped word"""
        out = np.full((self.W, 2 * self.Hc), np.nan, np.float32)
        out[self.live] = m[:self.R].float().cpu().numpy()[self.rows[self.live], self.blk]
        return out

    def untouched(self, m):
        """everything but the named rows' block columns still holds NaN"""
        hit = torch.zeros(m.shape, dtype=torch.bool, device=DEV)
        rows = torch.from_numpy(self.rows[self.live].astype(np.int64)).to(DEV)
        hit[rows, self.blk] = True
        return bool(torch.isnan(m.float()[~hit]).all()) and not bool(torch.isnan(m.float()[hit]).any())


@pytest.mark.parametrize("case", CASES, ids=lambda c: "E%d-H%d-W%d-L%d-V%d-%s" % c)
def test_forward_and_backward_against_the_reference(L, case):
    from kbner import ops
    c = Case(case)
    ref64 = C.evaluate(c.p, c.chars, c.lens, c.rows, c.dout, c.mask)
    ref32 = C.evaluate(c.p, c.chars, c.lens, c.rows, c.dout, c.mask, f32=True)
    # forward only, no masks, NaN all around
    plain = c.fwd(NAN, masked=False)
    assert c.untouched(plain), "the unmasked forward wrote outside the named rows' block, or left a named element unwritten"
    h = c.block_of(plain)
    C.check({"h": h}, ref64, ref32, what="forward", stats=WORST)
    # masked, saving for the backward: exactly the mask of charref on the stored value
    ws = ops.char_lstm_ws(c.tab, c.Hc, DEV)
    ws_guarded = torch.full((ws.numel() + GUARD,), NAN, dtype=F32, device=DEV)
    masked = c.fwd(NAN, masked=True, ws=ws_guarded[:ws.numel()])
    assert c.untouched(masked) and bool(torch.isnan(ws_guarded[ws.numel():]).all())
    exp = C.stored(h[c.live], c.mask[c.live])
    got = c.block_of(masked)[c.live]
    assert (got.view(np.int32) == exp.view(np.int32)).all(), "masked block != bf16(bf16(h) * mask) with the (row, col0 + c) keys"
    # ... and exactly gather_rows_drop over the unmasked matrix (zeros around the block on both sides)
    plain0, masked0 = c.fwd(0.0, masked=False), c.fwd(0.0, masked=True)
    idx = torch.arange(c.R, dtype=I32, device=DEV)
    via_rows = ops.gather_rows_drop(plain0[:c.R].contiguous(), idx, c.n, c.de, c.dl)
    assert torch.equal(bits(via_rows), bits(masked0[:c.R]))
    # backward: ADDS to what the buffers hold
    dmat = c.matrix(NAN)
    rows = torch.from_numpy(c.rows[c.live].astype(np.int64)).to(DEV)
    dmat[rows, c.blk] = dev(c.dout[c.live], BF16)
    grads = [flat(a, fill=G0) for a in (c.p.emb, c.p.wih, c.p.whh, c.p.bih, c.p.bhh)]
    ops.char_lstm_bwd(dmat[:c.R], c.col, *c.par[:3], c.tab, ws_guarded[:ws.numel()], *[g[:g.numel() - GUARD] for g in grads], c.n,
                      c.de, c.dl)
    torch.cuda.synchronize()
    got = {}
    for (name, sa), g, a in zip(C.GRADS, grads, (c.p.emb, c.p.wih, c.p.whh, c.p.bih, c.p.bhh)):
        assert bool(torch.isnan(g[a.size:]).all()), "wrote behind " + name
        got[name] = g[:a.size].cpu().numpy().astype(np.float64).reshape(a.shape) - G0
    for sa in {sa for _, sa in C.GRADS}:
        setattr(ref64, sa, getattr(ref64, sa) + G0)                      # the start value is a term of the sum
    C.check(got, ref64, ref32, what="backward", stats=WORST)
    if not c.live.all():                                                  # a dropped word's characters receive nothing from it
        only_dropped = np.setdiff1d(np.unique(c.chars[~c.live]), np.unique(np.concatenate(
            [c.chars[w, :c.lens[w]] for w in np.nonzero(c.live)[0]] or [np.zeros(0, np.int32)])))
        only_dropped = only_dropped[only_dropped != 0]
        assert (got["d_emb"][only_dropped] == 0).all()


def test_no_word_no_launch(L):
    from kbner import ops
    tab = ops.CharTables(np.zeros((0, 4), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), 5, 8, DEV)
    rng = np.random.default_rng(0)
    p = C.params(rng, 5, 8, 8)
    par = [dev(a) for a in (p.emb, p.wih, p.whh, p.bih, p.bhh)]
    m = torch.full((8, 32), NAN, dtype=BF16, device=DEV)
    seen = []
    real = L.call
    try:
        L.call = lambda name, *a: seen.append(name) or real(name, *a)
        ops.char_lstm_fwd(*par, tab, m, 8, 4)
        grads = [torch.zeros_like(t) for t in par]
        ops.char_lstm_bwd(m, 8, *par[:3], tab, None, *grads, 4)
    finally:
        L.call = real
    assert seen == [] and bool(torch.isnan(m.float()).all())


def _raw_args(L, c, m, **kw):
    a = dict(emb=L.ptr(c.par[0]), wih=L.ptr(c.par[1]), whh=L.ptr(c.par[2]), bih=L.ptr(c.par[3]), bhh=L.ptr(c.par[4]),
             chars=L.ptr(c.tab.chars), lens=L.ptr(c.tab.lens), rows=L.ptr(c.tab.rows), out=ctypes.c_void_p(m.data_ptr() + 2 * c.col),
             ld_out=c.ld, col0=c.col, ws=None, W=c.W, Lmax=c.Lmax, V=c.V, E=c.E, Hc=c.Hc, n=c.n, se=0, te=0, sl=0, tl=0,
             stream=L.stream_ptr())
    a.update(kw)
    return list(a.values())


@pytest.mark.parametrize("bad", [dict(E=0), dict(E=33), dict(Hc=0), dict(Hc=33), dict(ld_out=44), dict(col0=4), dict(n=0), dict(Lmax=0),
                                 dict(V=0), dict(W=-1), dict(out="odd"), dict(ld_out=40, col0=32), dict(ld_out=8, col0=0)],
                         ids=lambda b: ",".join("%s=%s" % kv for kv in b.items()))
def test_limits_return_einval_and_write_nothing(L, bad):
    c = Case((8, 8, 5, 5, 97, "off"))
    m = c.matrix(NAN)
    if bad.get("out") == "odd":
        bad = dict(out=ctypes.c_void_p(m.data_ptr() + 2 * c.col + 2))
    lib = L.load()
    assert lib.kbner_char_lstm_fwd(*_raw_args(L, c, m, **bad)) == EINVAL
    fwd = _raw_args(L, c, m, **bad)
    names = ["emb", "wih", "whh", "bih", "bhh", "chars", "lens", "rows", "out", "ld_out", "col0", "ws", "W", "Lmax", "V", "E", "Hc", "n",
             "se", "te", "sl", "tl", "stream"]
    a = dict(zip(names, fwd))
    grads = [flat(x, fill=G0) for x in (c.p.emb, c.p.wih, c.p.whh, c.p.bih, c.p.bhh)]
    ws = torch.zeros(max(lib.kbner_char_lstm_ws_bytes(c.W, c.Lmax, c.Hc) // 4, 1), dtype=F32, device=DEV)
    fwd_only = "out" in bad or bad == dict(ld_out=40, col0=32)            # the backward has no alignment rule of its own, and its
    if not fwd_only:                                                      # col0 is a mask key: the block need not lie at col0 of dout
        rc = lib.kbner_char_lstm_bwd(a["out"], a["ld_out"], a["col0"], a["emb"], a["wih"], a["whh"], a["chars"], a["lens"], a["rows"],
                                     L.ptr(ws), *[L.ptr(g) for g in grads], a["W"], a["Lmax"], a["V"], a["E"], a["Hc"], a["n"], 0, 0, 0, 0,
                                     a["stream"])
        assert rc == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(m.float()).all())
    for g, x in zip(grads, (c.p.emb, c.p.wih, c.p.whh, c.p.bih, c.p.bhh)):
        assert bool((g[:x.size] == G0).all())
    assert lib.kbner_char_lstm_ws_bytes(5, 0, 8) == 0 and lib.kbner_char_lstm_ws_bytes(5, 5, 33) == 0
    assert lib.kbner_char_lstm_ws_bytes(5, 5, 8) > 0
