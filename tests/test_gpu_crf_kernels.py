"""GPU: direct parity tests of the linear-chain CRF kernels (csrc/crf.hip, csrc/crf_nbest.hip, the distillation scans and
kbner_softmax_decode of csrc/crf_kd.hip), each through the C ABI with test-owned buffers, at every tag width where the
launchers change kernel (T <= 32 -> <32>, 33 <= T <= 64 -> <64>) and with the START / STOP ids anywhere in the tag range.

Shared grid (crfref.GRID: T in {3, 5, 29, 31, 32, 33, 48, 63, 64} x five START / STOP placements x (B, n) in {(1, 1), (5, 1),
(3, 7), (16, 48), (2, 130)}): kbner_crf_viterbi, _nll_fwd, _nll_bwd and _posterior against tests/crfref.py.  Viterbi tags and
the popped start tag equal oracle.crf's float32 decoder bit for bit, on Gaussian inputs and on integer inputs where ties are
everywhere (tests/test_crfref_cpu.py asserts that they are); every smooth output is compared with the float64 reference under
rowref.tolerance: 8 x the worst error of the same formula in plain float32 numpy, with a floor of 2 * 2^-24 * sum|terms|.
Every output buffer is pre-filled with NaN (or an int sentinel) and has guard elements behind it; dtrans is pre-filled with an
integer pattern the gradient has to be ADDED to.  tests/test_crfref_cpu.py shows that this check refuses eight kinds of
subtly wrong kernel, each on a named case of this list.

Every check prints the kernel's worst error, the float32-numpy evaluation's worst error, their ratio and the largest share of
the tolerance any element used (run with -s).  Worst figures per kernel output of the MI355X run that accompanied this module
(122 cases of this module, all passing, 5.2 s; the shared grid is 32 of them, each of which also decodes its tie inputs):
`ratio` = kernel error / float32-numpy error, of which the rule allows 8, taken over the cases where that term is the
tolerance; where the float32 evaluation comes out (nearly) exact the tolerance is its floor and the ratio says nothing (the
gold sum of 130 terms happened to round to 1.5e-7 in sequential float32 numpy; the kernel's 64-lane strided sum gave 4.0e-6,
0.11 of the floor) -- those lines are printed as floor-bound and left out of the ratio column.  `share` = the largest fraction
of its tolerance any element used.

    kernel (output)           kernel err   float32-numpy err   ratio   share
    nll_fwd (logz)            3.56e-04     3.56e-04            1.00    0.125
    nll_fwd (gold)            1.07e-05     1.22e-05            2.20    0.275
    nll_fwd (alpha)           4.04e-04     4.04e-04            1.23    0.154
    posterior                 4.26e-04     4.15e-04            2.48    0.310
    nll_bwd (demit)           2.86e-04     2.41e-04            2.50    0.312
    nll_bwd (dtrans)          3.94e-03     2.91e-03            1.36    0.354
    viterbi (conf)            8.76e-05     8.76e-05            -       0.125
    viterbi (conf, ties)      1.09e-07     1.09e-07            -       0.099

The worst errors come from the scale-8 case with +-30 outliers at T = 64, n = 48 (scores in the thousands) and, for conf, n = 511.  The
Viterbi confidences equal the float32 evaluation to every printed digit on every case (ratio 1.000, all floor-bound): the
kernel does the same float32 adds.  Posterior rows below lens sum to 1 within 4.3e-4 and demit rows to 0 within 3.1e-4 at
worst (same case).  No output needed scale > 1: the factor 8 stands, at most 2.5 of it is used, and no element used more
than 0.36 of its tolerance; __expf's argument scaling does not show, because every exponent the kernels hand it is a
log-probability (<= 0, small) formed after the large terms have cancelled.

The n-best decoder (bit-exact decode against oracle.crf.viterbi_nbest at T in {5, 29, 32, 33, 64}, nbest on both sides of
each <4>/<8>/<16> switch, ragged lens), the Viterbi LDS limit (n = 160 and n = 511 at T = 64 decode bit-exactly, n = 512 is
refused), argument rejection, softmax_decode ties and the distillation scans are further down.  Nothing here found a defect
in csrc/.
"""
import ctypes

import numpy as np
import pytest
import torch

import crfref
from oracle import crf as ocrf

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
DEV = "cuda"
GUARD = 96            # elements behind every output buffer that no kernel may touch
ISENT = -7777         # int sentinel
EINVAL = -22
STATS = crfref.Stats("crfk")


@pytest.fixture(scope="module")
def lib():
    from kbner import lib as L
    yield L.load()
    STATS.table()


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def dev(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


class Out:
    """a test-owned output buffer: `shape` elements pre-filled with NaN (float) / ISENT (int) or with `init`, GUARD more behind"""

    def __init__(self, shape, dtype=F32, init=None):
        self.shape, self.dtype = tuple(shape), dtype
        self.size = int(np.prod(self.shape)) if len(self.shape) else 1
        self.fill = float("nan") if dtype == F32 else ISENT
        self.full = torch.full((self.size + GUARD,), self.fill, dtype=dtype, device=DEV)
        if init is not None:
            self.full[:self.size] = dev(init, np.float32 if dtype == F32 else np.int32).reshape(-1)
        self.ptr = P(self.full)

    def _untouched(self, part):
        return bool(torch.isnan(part).all()) if self.dtype == F32 else bool((part == ISENT).all())

    def get(self):
        """the written part as numpy, after asserting that the guard behind it is as it was"""
        assert self._untouched(self.full[self.size:]), "wrote behind the buffer"
        return self.full[:self.size].cpu().numpy().reshape(self.shape)

    def untouched(self):
        return self._untouched(self.full)


def no_sentinel(a):
    return not np.isnan(a).any() if a.dtype.kind == "f" else not (a == ISENT).any()


# ====================================================================== the shared grid
def _viterbi(lib, emit, trans, lens, start, stop):
    B, n, T = emit.shape
    tags, conf, popped = Out((B, n), I32), Out((B, n)), Out((B,), I32)
    d_emit, d_trans, d_lens = dev(emit), dev(trans), dev(lens, np.int32)     # held until the kernel has run
    rc = lib.kbner_crf_viterbi(P(d_emit), P(d_trans), P(d_lens), B, n, T, start, stop, tags.ptr, conf.ptr, popped.ptr,
                               _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    out = tags.get(), conf.get(), popped.get()
    assert all(no_sentinel(a) for a in out), "kbner_crf_viterbi left an output element unwritten"
    return out


@pytest.mark.parametrize("case", crfref.GRID, ids=crfref.grid_id)
def test_crf_grid(lib, case):
    x = crfref.grid_inputs(case)
    B, n, T, start, stop = x["B"], x["n"], x["T"], x["start"], x["stop"]
    got = {}
    got["vtags"], got["vconf"], got["vpopped"] = _viterbi(lib, x["emit"], x["trans"], x["lens"], start, stop)
    if x["tie_emit"] is not None:
        got["tie_tags"], got["tie_conf"], got["tie_popped"] = _viterbi(lib, x["tie_emit"], x["tie_trans"], x["tie_lens"], start, stop)
    emit, trans, tags, lens, dloss = dev(x["emit"]), dev(x["trans"]), dev(x["tags"], np.int32), dev(x["lens"], np.int32), dev(x["dloss"])
    logz, gold, alpha = Out((B,)), Out((B,)), Out((B, n + 1, T))
    rc = lib.kbner_crf_nll_fwd(P(emit), P(trans), P(tags), P(lens), B, n, T, start, stop, logz.ptr, gold.ptr, alpha.ptr, _stream())
    assert rc == 0, rc
    demit, dtrans, marg = Out((B, n, T)), Out((T, T), init=x["pattern"]), Out((B, n, T))
    rc = lib.kbner_crf_nll_bwd(P(emit), P(trans), P(tags), P(lens), alpha.ptr, logz.ptr, P(dloss), B, n, T, start, stop, demit.ptr,
                               dtrans.ptr, _stream())
    assert rc == 0, rc
    rc = lib.kbner_crf_posterior(P(emit), P(trans), P(lens), alpha.ptr, logz.ptr, B, n, T, start, stop, marg.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for k, o in (("logz", logz), ("gold", gold), ("alpha", alpha), ("demit", demit), ("dtrans", dtrans), ("marg", marg)):
        got[k] = o.get()
        if k != "alpha":                                                          # alpha rows above lens[b] are unspecified
            assert no_sentinel(got[k]), "%s: an element was left unwritten" % k
    crfref.check_grid(case, got, STATS)


# ====================================================================== the Viterbi LDS limit
@pytest.mark.parametrize("n", [160, 511])
def test_viterbi_dynamic_lds(lib, n):
    """T = 64: n = 160 needs 51 216 B, the first launch through the raised dynamic-LDS limit; n = 511 needs 163 536 B, the
    largest the 160 KiB the header promises admit"""
    B, T, start, stop = 2, 64, 17, 5
    lds = int(lib.kbner_crf_viterbi_lds_bytes(n, T))
    assert lds == n * T * 5 + 16 and 48 * 1024 < lds <= 160 * 1024
    rng = np.random.default_rng(n)
    emit, trans, _, lens = crfref.real_case(rng, B, n, T, start, stop, 2.0)
    tags, conf, popped = _viterbi(lib, emit, trans, lens, start, stop)
    rt, rc, rp = crfref._oracle_viterbi(emit, trans, lens, start, stop)
    assert np.array_equal(tags, rt) and np.array_equal(popped, rp)
    r64 = crfref.viterbi(emit, trans, lens, start, stop, np.float64, with_scores=True)
    r32 = crfref.viterbi(emit, trans, lens, start, stop, np.float32)
    step = np.abs(emit.astype(np.float64)).max(axis=2) + crfref.fin(trans).max()
    crfref.check_close(STATS, "viterbi conf", "T64-lds-n%d" % n, conf, r64[1], r32[1], 2.0 * np.cumsum(step, axis=1))


def test_viterbi_lds_limit_is_refused_before_any_launch(lib):
    B, T, n = 2, 64, 512
    assert int(lib.kbner_crf_viterbi_lds_bytes(n, T)) == 163856 > 160 * 1024
    emit, trans, lens = torch.zeros((B, n, T), device=DEV), torch.zeros((T, T), device=DEV), torch.full((B,), n, dtype=I32, device=DEV)
    tags, conf, popped = Out((B, n), I32), Out((B, n)), Out((B,), I32)
    rc = lib.kbner_crf_viterbi(P(emit), P(trans), P(lens), B, n, T, 17, 5, tags.ptr, conf.ptr, popped.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert tags.untouched() and conf.untouched() and popped.untouched()


# ====================================================================== argument rejection: -22, nothing launched, nothing written
def _crf_entry_points(lib, B, n, T, start, stop, TA):
    """the four CRF entry points with buffers sized for tag count TA (>= 1); -> [(name, rc, outputs)]"""
    z = lambda *s: torch.zeros(s, device=DEV)
    zi = lambda *s: torch.zeros(s, dtype=I32, device=DEV)
    emit, trans, tags, lens, dloss = z(B, n, TA), z(TA, TA), zi(B, n), zi(B) + n, z(B) + 1.0
    alpha, logz = z(B, n + 1, TA), z(B)
    res = []
    o = [Out((B, n), I32), Out((B, n)), Out((B,), I32)]
    res.append(("viterbi", lib.kbner_crf_viterbi(P(emit), P(trans), P(lens), B, n, T, start, stop, o[0].ptr, o[1].ptr, o[2].ptr, _stream()), o))
    o = [Out((B,)), Out((B,)), Out((B, n + 1, TA))]
    res.append(("nll_fwd", lib.kbner_crf_nll_fwd(P(emit), P(trans), P(tags), P(lens), B, n, T, start, stop, o[0].ptr, o[1].ptr, o[2].ptr,
                                                 _stream()), o))
    o = [Out((B, n, TA)), Out((TA, TA))]
    res.append(("nll_bwd", lib.kbner_crf_nll_bwd(P(emit), P(trans), P(tags), P(lens), P(alpha), P(logz), P(dloss), B, n, T, start, stop,
                                                 o[0].ptr, o[1].ptr, _stream()), o))
    o = [Out((B, n, TA))]
    res.append(("posterior", lib.kbner_crf_posterior(P(emit), P(trans), P(lens), P(alpha), P(logz), B, n, T, start, stop, o[0].ptr,
                                                     _stream()), o))
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("T,start,stop", [(0, 0, 0), (65, 63, 64), (29, 29, 28), (29, -1, 28), (29, 27, 29), (29, 27, -1),
                                          (64, 64, 0), (64, 0, 64), (33, -1, 0), (33, 0, -1)])
def test_crf_entry_points_reject_bad_tag_arguments(lib, T, start, stop):
    for name, rc, outs in _crf_entry_points(lib, 2, 3, T, start, stop, max(T, 1)):
        assert rc == EINVAL, (name, rc)
        assert all(o.untouched() for o in outs), name


def test_nbest_rejects_bad_arguments(lib):
    B, n, T = 2, 3, 5
    emit, trans, lens = torch.zeros((B, n, T), device=DEV), torch.zeros((T, T), device=DEV), torch.full((B,), n, dtype=I32, device=DEV)
    ws = torch.zeros(B * n * T * 32, dtype=torch.int16, device=DEV)
    for nn, nbest in ((n, 0), (n, 17), (n, T + 1), (0, 2)):
        dec, score = Out((B, max(nn, 1), max(nbest, 1)), I32), Out((B, max(nbest, 1)))
        rc = lib.kbner_crf_viterbi_nbest(P(emit), P(trans), P(lens), B, nn, T, 3, 4, nbest, P(ws), dec.ptr, score.ptr, _stream())
        torch.cuda.synchronize()
        assert rc == EINVAL, (nn, nbest, rc)
        assert dec.untouched() and score.untouched()
    T = 64                                               # nbest = 17 where T would allow it
    emit, trans = torch.zeros((B, n, T), device=DEV), torch.zeros((T, T), device=DEV)
    ws = torch.zeros(B * n * T * 32, dtype=torch.int16, device=DEV)
    dec, score = Out((B, n, 17), I32), Out((B, 17))
    assert lib.kbner_crf_viterbi_nbest(P(emit), P(trans), P(lens), B, n, T, 3, 4, 17, P(ws), dec.ptr, score.ptr, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert dec.untouched() and score.untouched()


def test_narrow_kernels_reject_wider_tag_sets(lib):
    """T = 33 for the distillation scans (T <= 32), T = 65 for the softmax head and the emission KL (T <= 64)"""
    z = lambda *s: torch.zeros(s, device=DEV)
    B, n, T = 2, 3, 33
    emit, trans, lens, wgt = z(B, n, T), z(T, T), torch.full((B,), n, dtype=I32, device=DEV), z(B) + 1.0
    ws = z(B * 4 * n * T + 16)
    pair, sc = z(B, n - 1, T * T), z(B, T)
    st = _stream()
    o = [Out((B, n, T))]
    assert lib.kbner_crf_fb_score(P(emit), P(trans), P(lens), 0, B, n, T, 0, 1, o[0].ptr, st) == EINVAL and o[0].untouched()
    for fn in (lib.kbner_crf_posterior_kl, lib.kbner_crf_posterior_kl_scores):
        o = [Out((B,)), Out((B, n, T)), Out((T, T))]
        assert fn(P(emit), P(emit), P(trans), P(lens), P(wgt), 2.0, B, n, T, 0, 1, o[0].ptr, o[1].ptr, o[2].ptr, P(ws), st) == EINVAL
        assert all(x.untouched() for x in o)
    o = [Out((B, n - 1, T * T)), Out((B, T)), Out((B, T))]
    assert lib.kbner_crf_pair_posterior(P(emit), P(trans), P(lens), 0, 2.0, B, n, T, 0, 1, o[0].ptr, o[1].ptr, o[2].ptr, P(ws), st) == EINVAL
    assert all(x.untouched() for x in o)
    o = [Out((B,)), Out((B, n, T)), Out((T, T))]
    assert lib.kbner_crf_exact_kd(P(emit), P(trans), P(lens), P(pair), P(sc), P(sc), P(wgt), 2.0, B, n, T, 0, 1, o[0].ptr, o[1].ptr, o[2].ptr,
                                  P(ws), st) == EINVAL
    assert all(x.untouched() for x in o)
    T = 65
    emit, tags = z(B, n, T), torch.zeros((B, n), dtype=I32, device=DEV)
    o = [Out((B,)), Out((B, n, T))]
    assert lib.kbner_softmax_ce(P(emit), P(tags), P(lens), P(wgt), B, n, T, o[0].ptr, o[1].ptr, st) == EINVAL and all(x.untouched() for x in o)
    o = [Out((B, n), I32), Out((B, n)), Out((B, n, T))]
    assert lib.kbner_softmax_decode(P(emit), P(lens), B, n, T, o[0].ptr, o[1].ptr, o[2].ptr, st) == EINVAL and all(x.untouched() for x in o)
    o = [Out((B,)), Out((B, n, T))]
    assert lib.kbner_emission_kl(P(emit), P(emit), P(lens), P(wgt), 2.0, 0, B, n, T, o[0].ptr, o[1].ptr, st) == EINVAL
    assert all(x.untouched() for x in o)
    torch.cuda.synchronize()


# ====================================================================== n-best Viterbi
def _nbest(lib, emit, trans, lens, start, stop, nbest):
    B, n, T = emit.shape
    ws = torch.zeros(max(1, int(lib.kbner_crf_viterbi_nbest_ws_bytes(B, n, T, nbest)) // 2) + GUARD, dtype=torch.int16, device=DEV)
    dec, score = Out((B, n, nbest), I32), Out((B, nbest))
    d_emit, d_trans, d_lens = dev(emit), dev(trans), dev(lens, np.int32)
    rc = lib.kbner_crf_viterbi_nbest(P(d_emit), P(d_trans), P(d_lens), B, n, T, start, stop, nbest, P(ws), dec.ptr,
                                     score.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    d, s = dec.get(), score.get()
    assert no_sentinel(d) and no_sentinel(s)
    return d, s


def _nbest_lens(rng, B, n):
    lens = rng.integers(1, n + 1, size=B).astype(np.int32)            # >= 1; sentences shorter than the batch maximum
    lens[0] = n
    lens[1] = 1
    return lens


NBEST_PLACE = ["last2", "first2", "swapped", "ends", "middle"]
NBEST_CASES = [(T, nb, B, n, NBEST_PLACE[(k + j) % 5])
               for k, T in enumerate((5, 29, 32, 33, 64))
               for j, (nb, (B, n)) in enumerate(zip((1, 4, 5, 8, 9, 16), ((4, 1), (4, 2), (7, 3), (8, 40), (4, 2), (7, 3)))) if nb <= T]
NBEST_CASES += [(29, 16, 8, 40, "ends"), (64, 16, 8, 40, "middle"), (33, 4, 8, 40, "first2"), (5, 5, 8, 40, "swapped"), (64, 9, 4, 1, "last2")]


@pytest.mark.parametrize("T,nbest,B,n,place", NBEST_CASES)
def test_viterbi_nbest(lib, T, nbest, B, n, place):
    start, stop = crfref._placements(T)[place]
    rng = np.random.default_rng(T * 1000 + nbest * 10 + n)
    emit = (rng.standard_normal((B, n, T)) * 2).astype(np.float32)
    trans = rng.standard_normal((T, T)).astype(np.float32)
    lens = _nbest_lens(rng, B, n)
    dec, score = _nbest(lib, emit, trans, lens, start, stop, nbest)
    ps, want = ocrf.viterbi_nbest(emit, lens, trans, start, stop, nbest)
    np.testing.assert_array_equal(dec, want)
    np.testing.assert_allclose(score, ps, rtol=2e-5, atol=1e-7)


@pytest.mark.parametrize("T,start,stop,nbest", [(33, 0, 32, 5), (64, 17, 5, 16), (33, 32, 0, 9), (64, 62, 63, 4)])
def test_viterbi_nbest_tie_order(lib, T, start, stop, nbest):
    """Among equal candidates the lower flat index (from * nbest + k) comes first: the kernel's comment and the docstring of
    oracle.crf.viterbi_nbest both promise it.  The reference's torch.topk leaves the order among equal values open, so this
    pins the project's own convention, not the reference's.  The decoder reads transitions[from, to]: crfref.tie_case's matrix
    is given as it is (START row forbidden: every score sits on the -1e12 level and everything ties) and transposed (small
    integer scores, ties among the real candidates)."""
    B, n = 4, 40
    emit, trans, _ = crfref.tie_case(np.random.default_rng(T + nbest), B, n, T, start, stop)
    lens = _nbest_lens(np.random.default_rng(T), B, n)
    for tr in (trans, np.ascontiguousarray(trans.T)):
        dec, score = _nbest(lib, emit, tr, lens, start, stop, nbest)
        ps, want = ocrf.viterbi_nbest(emit, lens, tr, start, stop, nbest)
        np.testing.assert_array_equal(dec, want)
        np.testing.assert_allclose(score, ps, rtol=2e-5, atol=1e-7)


# ====================================================================== softmax decode: first index among equal maxima
@pytest.mark.parametrize("T", [2, 33, 64])
def test_softmax_decode_ties(lib, T):
    rng = np.random.default_rng(T)
    B, n = 3, 9
    emit = rng.integers(-3, 4, size=(B, n, T)).astype(np.float32)
    emit[:, 0, :] = 1.0                                              # all values equal
    emit[:, 1, :] = np.minimum(emit[:, 1, :], 2.0)
    emit[:, 1, 0] = emit[:, 1, T - 1] = 3.0                          # the maximum on lane 0 and lane T - 1
    emit[:, 2, :] = -2.0
    emit[:, 2, T - 1] = 0.0                                          # the maximum on the last lane alone
    emit[:, 3, :] = 0.0
    emit[:, 3, T // 2:] = 2.0                                        # the upper half ties
    lens = np.array([n, 5, 0], np.int32)
    tags, conf, dist = Out((B, n), I32), Out((B, n)), Out((B, n, T))
    d_emit, d_lens = dev(emit), dev(lens, np.int32)
    rc = lib.kbner_softmax_decode(P(d_emit), P(d_lens), B, n, T, tags.ptr, conf.ptr, dist.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0
    tg, cf, ds = tags.get(), conf.get(), dist.get()
    assert no_sentinel(tg) and no_sentinel(cf) and no_sentinel(ds)
    e = emit.astype(np.float64)
    p = np.exp(e - e.max(2, keepdims=True))
    p /= p.sum(2, keepdims=True)
    below = np.arange(n)[None, :] < lens[:, None]
    first = e.argmax(2)                                              # numpy: the first maximal index
    assert (first[:, 0] == 0).all() and (first[:, 1] == 0).all() and (first[:, 2] == T - 1).all() and (first[:, 3] == T // 2).all()
    assert np.array_equal(tg[below], first[below])
    assert np.abs(cf[below] - np.take_along_axis(p, first[:, :, None], 2)[:, :, 0][below]).max() <= 2e-6
    assert np.abs(ds[below] - p[below]).max() <= 2e-6
    assert (tg[~below] == 0).all() and (cf[~below] == 0).all() and (ds[~below] == 0).all()


# ====================================================================== distillation scans (csrc/crf_kd.hip), T <= 32
KD_CASES = [(T, place, B, n) for T in (3, 5, 31, 32) for place in ("last2", "first2", "swapped") for B, n in ((4, 1), (4, 2), (6, 9))]


def _valid(n, lens):
    return np.arange(n)[None, :] < np.asarray(lens)[:, None]


@pytest.mark.parametrize("T,place,B,n", KD_CASES)
def test_kd_scans(lib, T, place, B, n):
    """fb_score, pair_posterior, posterior_kl, posterior_kl_scores and exact_kd against the float64 torch-autograd restatements
    of oracle/kd.py and oracle/multiview.py, with START / STOP moved and the suppressed set following them; bounds as in
    test_kd_loss_vs_oracle and test_multiview_posterior_kl_vs_oracle"""
    from oracle import kd as okd
    from oracle import multiview as omv
    start, stop = crfref._placements(T)[place]
    rng = np.random.default_rng(T * 100 + B * 10 + n + start)
    unk = [t for t in range(T) if t not in (start, stop)][0]
    sup = (stop, start) if T == 3 else (stop, start, unk)
    bits = sum(1 << t for t in sup)
    tau = 2.0
    trans = ocrf.init_transitions(T, start, stop, rng).astype(np.float32)
    trans_t = rng.standard_normal((T, T)).astype(np.float32)
    es = (rng.standard_normal((B, n, T)) * 2.0).astype(np.float32)
    et = (es + rng.standard_normal((B, n, T))).astype(np.float32)
    lens = crfref.ragged_lens(rng, B, n, low=1)
    wts = rng.uniform(0.1, 1.0, size=B).astype(np.float32)
    pattern = crfref.dtrans_pattern(T)
    valid = _valid(n, lens)
    d_es, d_et, d_tr, d_trt, d_lens, d_w = dev(es), dev(et), dev(trans), dev(trans_t), dev(lens, np.int32), dev(wts)
    T64 = lambda a: torch.from_numpy(np.asarray(a)).double()
    tol = 1e-4 * max(1.0, n / 20.0)

    def close(got, ref, t, floor, f32_floor=None):
        assert np.isfinite(got).all()
        big = np.abs(ref).max(initial=0.0)
        bound = t * max(floor, big)
        if f32_floor is not None and big < floor:          # the reference (all but) vanishes: see f_e below
            bound = max(bound, f32_floor)
        assert np.abs(got - ref).max(initial=0.0) <= bound, (np.abs(got - ref).max(), bound)

    # ---- teacher side: fb scores and pair posteriors
    score = Out((B, n, T))
    assert lib.kbner_crf_fb_score(P(d_et), P(d_trt), P(d_lens), bits, B, n, T, start, stop, score.ptr, _stream()) == 0
    ws = torch.zeros(max(1, int(lib.kbner_crf_pair_ws_floats(B, n, T))) + GUARD, device=DEV)
    pair, s_sc, e_sc = Out((B, max(n - 1, 1), T * T)), Out((B, T)), Out((B, T))
    assert lib.kbner_crf_pair_posterior(P(d_et), P(d_trt), P(d_lens), bits, tau, B, n, T, start, stop, pair.ptr if n > 1 else None,
                                        s_sc.ptr, e_sc.ptr, P(ws), _stream()) == 0
    torch.cuda.synchronize()
    g_score = score.get()
    assert no_sentinel(g_score) and (g_score[~valid] == 0).all()
    o_score = okd.teacher_fb_score(T64(et), T64(trans_t), lens, start, stop, sup).numpy()
    fin = valid[:, :, None] & (o_score > -1e10)
    assert (g_score[valid[:, :, None] & ~(o_score > -1e10)] < -1e10).all()
    assert np.abs(g_score[fin] - o_score[fin]).max() <= 2e-5 * max(1.0, np.abs(o_score[fin]).max())
    o_pair, o_s, o_e = okd.teacher_pair_posterior(T64(et), T64(trans_t), lens, start, stop, sup, tau)
    g_s, g_e = s_sc.get(), e_sc.get()
    assert no_sentinel(g_s) and no_sentinel(g_e)
    for g, o in ((g_s, o_s.numpy()), (g_e, o_e.numpy())):
        f = o > -1e10
        assert (g[~f] < -1e10).all()
        assert np.abs(g[f] - o[f]).max() <= 2e-5 * max(1.0, np.abs(o[f]).max())
    if n > 1:
        g_pair = pair.get()
        pv = np.arange(n - 1)[None, :] < (lens - 1)[:, None]
        assert no_sentinel(g_pair) and (g_pair[~pv] == 0).all()
        assert np.abs(g_pair[pv] - o_pair.numpy()[pv]).max(initial=0.0) < 5e-6
        p_in = g_pair
    else:
        p_in = np.zeros((B, 0, T * T), np.float32)

    # ---- student side: the three losses, each with demit written into NaN and dtrans added to the pattern
    def student(fn, *front):
        loss, demit, dtr = Out((B,)), Out((B, n, T)), Out((T, T), init=pattern)
        w = torch.zeros(max(1, int(lib.kbner_crf_posterior_kl_ws_floats(B, n, T))) + GUARD, device=DEV)
        rc = fn(*front, B, n, T, start, stop, loss.ptr, demit.ptr, dtr.ptr, P(w), _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        out = loss.get(), demit.get(), dtr.get() - pattern
        assert all(no_sentinel(a) for a in out) and (out[1][~valid] == 0).all()
        return out

    # Where the reference gradient (all but) vanishes the relative bound has nothing to be relative to: at T = 3 one tag is
    # left, the path is forced, the float64 gradient is exactly 0 and tol * max(1e-3, 0) = 1e-7 asks for less than one rounding
    # of a float32 exponent.  There, and only there (largest |reference| below the bound's own 1e-3), the bound is the
    # project's floor rule 2 * 2^-24 * sum|terms|: a gradient is w tau (q - p), two probabilities whose exponents
    # alpha + beta - normaliser, of size S, carry 2^-24 S each; a transition gradient sums that over the tokens.
    with torch.no_grad():
        gs0 = (omv.forward_vars(T64(es), T64(trans), start) + omv.backward_vars(T64(es), lens, T64(trans), stop)).numpy()
    S = 2.0 * crfref.fin(gs0[valid]).max()
    f_e = 2.0 * 2.0 ** -24 * float(wts.max()) * tau * S
    f_t = f_e * int(lens.sum())

    def compare(out, per, es_t, tr_t):
        (per * T64(wts)).sum().backward()
        close(out[0], per.detach().numpy(), tol, 1.0)
        close(out[1], es_t.grad.numpy(), tol, 1e-3, f_e)
        close(out[2], tr_t.grad.numpy(), 3 * tol, 1e-3, f_t)

    def leaves():
        return T64(es).requires_grad_(True), T64(trans).requires_grad_(True)

    es_t, tr_t = leaves()
    compare(student(lib.kbner_crf_posterior_kl, P(d_es), P(d_et), P(d_tr), P(d_lens), P(d_w), tau),
            omv.posterior_kl(es_t, T64(et), tr_t, lens, tau, start, stop), es_t, tr_t)
    # teacher given as its fb scores (the device's own, so both sides see the same numbers)
    es_t, tr_t = leaves()
    mask = T64(valid.astype(np.float64))
    gs = (omv.forward_vars(es_t, tr_t, start) + omv.backward_vars(es_t, lens, tr_t, stop)) * mask[:, :, None]
    kd = torch.nn.functional.kl_div(torch.log_softmax(gs / tau, dim=-1), torch.softmax(T64(g_score) / tau, dim=-1), reduction="none")
    d_score, d_s, d_e = dev(g_score), dev(g_s), dev(g_e)
    compare(student(lib.kbner_crf_posterior_kl_scores, P(d_es), P(d_score), P(d_tr), P(d_lens), P(d_w), tau),
            (kd * mask[:, :, None]).sum((1, 2)) * tau * tau, es_t, tr_t)
    es_t, tr_t = leaves()
    d_pair = dev(p_in) if n > 1 else None
    compare(student(lib.kbner_crf_exact_kd, P(d_es), P(d_tr), P(d_lens), P(d_pair), P(d_s), P(d_e), P(d_w), tau),
            okd.exact_per_sentence(es_t, tr_t, lens, T64(p_in), T64(g_s), T64(g_e), tau, start, stop), es_t, tr_t)
