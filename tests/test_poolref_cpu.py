"""CPU: the reference of kbner_pool_rows_layers (tests/poolref.py) is what the GPU test trusts, so it is checked here:
  - against a direct transcription of the reference's loop in torch float64 (flair/embeddings.py:3303-3345: slice, [0] / [-1] / cat /
    torch.mean, cat over the layers, torch.mean(torch.stack(..., 1), 1));
  - its float32 restatement in the kernel's order of operations stays inside the bound on the whole case list, with and without a
    fused multiply-add of the scale, and reproduces the exact cases bit for bit;
  - the check REFUSES a list of defective evaluations, each on at least one case."""
import numpy as np
import pytest
import torch

import poolref as pr


def _loop_torch(xs64, span_ptr, span_rows, op, layer_mean):
    """the reference's per-token loop on hidden states [k][rows, H], float64"""
    hs = [torch.from_numpy(np.asarray(x, np.float64)) for x in xs64]
    R = len(span_ptr) - 1
    W = pr.width(op, len(hs), hs[0].shape[1], layer_mean)
    out = torch.zeros(R, W, dtype=torch.float64)
    for r in range(R):
        rows = torch.from_numpy(np.asarray(span_rows[span_ptr[r]:span_ptr[r + 1]], np.int64))
        if rows.numel() == 0:
            continue                                           # torch.zeros(self.embedding_length)
        subtoken_embeddings = []
        for layer in hs:
            current = layer[rows]
            if op == "first":
                final = current[0]
            if op == "last":
                final = current[-1]
            if op == "first_last":
                final = torch.cat([current[0], current[-1]])
            if op == "mean":
                final = torch.mean(torch.cat([e.unsqueeze(0) for e in current], dim=0), dim=0)
            subtoken_embeddings.append(final)
        if layer_mean:
            subtoken_embeddings = [torch.mean(torch.stack(subtoken_embeddings, dim=1), dim=1)]
        out[r] = torch.cat(subtoken_embeddings)
    return out.numpy()


def test_case_list_covers_every_axis_value():
    cs = pr.POOL_CASES
    assert {c[0] for c in cs} == set(pr.ROWS) and {c[1] for c in cs} == set(pr.WIDTHS) and {c[2] for c in cs} == set(pr.KS)
    assert {c[3] for c in cs} == set(pr.OPS) and {c[4] for c in cs} == {False, True}
    assert {(c[3], c[4]) for c in cs if c[1] == 520} == {(o, l) for o in pr.OPS for l in (False, True)}
    assert len(cs) <= 80
    _, sp, sr = pr.pool_inputs(70, 8, 1)
    m = pr.span_lengths(sp)
    assert m[0] == 0 and m[-1] == 0 and {1, 2, 3, 17} <= set(m.tolist())
    seam = sr[sp[2]:sp[3]]
    assert seam[1] < seam[0] - 1                                # non-consecutive, non-monotone
    assert sr[sp[3]] == sr[sp[1]]                               # one source row, two words


@pytest.mark.parametrize("case", pr.POOL_CASES, ids=lambda c: "R%d-H%d-k%d-%s-%s" % (c[0], c[1], c[2], c[3], "lm" if c[4] else "cat"))
def test_reference_is_the_reference_loop_and_f32_is_inside_the_bound(case):
    R, H, k, op, lm = case
    xs, sp, sr = pr.pool_inputs(R, H, k)
    ref = pr.pool_layers(xs, sp, sr, op, lm)
    np.testing.assert_allclose(ref, _loop_torch(xs, sp, sr, op, lm), rtol=1e-14, atol=0)
    for fma in (False, True):
        got = pr.round_bf16(pr.pool_layers_f32(xs, sp, sr, op, lm, fma=fma))
        pr.check(got, xs, sp, sr, op, lm)
    m = pr.span_lengths(sp)
    if op == "mean" and not lm:                                 # a span of one row: the mean is the copy
        one = np.nonzero(m == 1)[0]
        got = pr.round_bf16(pr.pool_layers_f32(xs, sp, sr, op, lm))
        first = pr.pool_layers(xs, sp, sr, "first", False)
        assert np.array_equal(got[one], first[one])


@pytest.mark.parametrize("op,lm", pr.EXACT_CASES)
def test_exact_inputs_are_exact_in_float32(op, lm):
    xs, sp, sr = pr.exact_inputs()
    ref = pr.pool_layers(xs, sp, sr, op, lm)
    for fma in (False, True):
        f32 = pr.pool_layers_f32(xs, sp, sr, op, lm, fma=fma)
        assert np.array_equal(f32.astype(np.float64), ref)     # no float32 rounding anywhere
        pr.check(pr.round_bf16(f32), xs, sp, sr, op, lm, exact=True)
    for x in xs:
        assert np.array_equal(pr.round_bf16(x), x)             # the inputs are bf16 numbers


def test_tie_case_pins_round_to_nearest_even():
    xs, sp, sr, want = pr.tie_inputs()
    assert np.array_equal(pr.round_bf16(xs[0]), xs[0])
    f32 = pr.pool_layers_f32(xs, sp, sr, "mean", False)
    assert np.array_equal(f32.astype(np.float64), pr.pool_layers(xs, sp, sr, "mean", False))
    assert np.array_equal(pr.round_bf16(f32), want)
    pr.check(want, xs, sp, sr, "mean", False, exact=True)
    up = want.copy()
    up[0, 0] = 258.0                                            # round-half-up / away from zero gives 258
    with pytest.raises(AssertionError):
        pr.check(up, xs, sp, sr, "mean", False, exact=True)


# ---------------------------------------------------------------------- defective evaluations the check must refuse
def _extended(sp, sr):
    """every span extended by the next non-empty word's first piece"""
    spans = [list(sr[sp[r]:sp[r + 1]]) for r in range(len(sp) - 1)]
    out = []
    for r, s in enumerate(spans):
        nxt = next((t[0] for t in spans[r + 1:] if t), None)
        out.append(s + [nxt] if s and nxt is not None else s)
    return np.concatenate([[0], np.cumsum([len(s) for s in out])]).astype(np.int64), np.asarray([x for s in out for x in s], np.int64)


def _defect(kind, xs, sp, sr, op, lm):
    """-> the defective block (float64, rounded to bf16), or None where the defect does not apply to the case"""
    k, H = len(xs), xs[0].shape[1]
    m = pr.span_lengths(sp).astype(np.float64)[:, None]
    good = pr.pool_layers(xs, sp, sr, op, lm)
    if kind == "first_for_last" and op == "last":
        out = pr.pool_layers(xs, sp, sr, "first", lm)
    elif kind == "halves_swapped" and op == "first_last":
        out = good.reshape(good.shape[0], -1, 2, H)[:, :, ::-1, :].reshape(good.shape)
    elif kind == "layers_reversed" and k > 1 and not lm:
        out = pr.pool_layers(xs[::-1], sp, sr, op, lm)
    elif kind == "span_extended" and op in ("last", "first_last", "mean"):
        sp2, sr2 = _extended(sp, sr)
        out = pr.pool_layers(xs, sp2, sr2, op, lm)
    elif kind == "mean_over_m_plus_1" and op == "mean":
        out = good * m / (m + 1)
    elif kind == "sum_undivided" and op == "mean":
        out = good * np.maximum(m, 1)
    elif kind == "layer_mean_over_k_minus_1" and lm and k > 1:
        out = good * k / (k - 1)
    elif kind == "empty_row_keeps_sentinel" and (m == 0).any():
        out = good.copy()
        out[(m == 0)[:, 0]] = pr.SENTINEL
    else:
        return None
    return pr.round_bf16(out)


DEFECTS = ["first_for_last", "halves_swapped", "layers_reversed", "span_extended", "mean_over_m_plus_1", "sum_undivided",
           "layer_mean_over_k_minus_1", "empty_row_keeps_sentinel"]


@pytest.mark.parametrize("kind", DEFECTS)
def test_check_refuses_defective_evaluations(kind):
    applied = refused = 0
    for R, H, k, op, lm in pr.POOL_CASES:
        xs, sp, sr = pr.pool_inputs(R, H, k)
        bad = _defect(kind, xs, sp, sr, op, lm)
        if bad is None:
            continue
        applied += 1
        try:
            pr.check(bad, xs, sp, sr, op, lm)
        except AssertionError:
            refused += 1
    assert applied >= 1 and refused >= 1, (kind, applied, refused)
    multi = [c for c in pr.POOL_CASES if c[0] > 1 and _defect(kind, *pr.pool_inputs(*c[:3]), c[3], c[4]) is not None]
    for R, H, k, op, lm in multi:                               # on every multi-row case it applies to, in fact
        xs, sp, sr = pr.pool_inputs(R, H, k)
        with pytest.raises(AssertionError):
            pr.check(_defect(kind, xs, sp, sr, op, lm), xs, sp, sr, op, lm)


def test_check_refuses_a_write_past_the_block():
    R, H, k, op, lm = 6, 128, 2, "mean", False
    xs, sp, sr = pr.pool_inputs(R, H, k)
    W, col, ld = pr.width(op, k, H, lm), 16, 16 + 2 * 128 + 24
    full = np.full((R + 3, ld), pr.SENTINEL)
    full[:R, col:col + W] = pr.round_bf16(pr.pool_layers_f32(xs, sp, sr, op, lm))
    pr.check_matrix(full, R, col, xs, sp, sr, op, lm)
    for where in ((slice(0, 1), slice(col + W, col + W + 8)), (slice(0, 1), slice(col - 8, col)), (slice(R, R + 1), slice(col, col + 8))):
        bad = full.copy()
        bad[where] = 0.0                                        # one 8-column group past the block / before it / a row behind R
        with pytest.raises(AssertionError, match="outside its block"):
            pr.check_matrix(bad, R, col, xs, sp, sr, op, lm)
