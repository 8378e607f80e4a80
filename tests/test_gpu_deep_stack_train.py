"""GPU: kbner.stack.BiLSTMHead with rnn_layers > 1 and a trained initial state (lstm_init_h / lstm_init_c), and StackOptimizer over the
parameter blocks they add.

Head: (D, H, T) = (72, 100, 9) and (72, 40, 5), B = 3, n = 7, lengths (7, 1, 4), L = 2 and 3.  The loss, the emissions and every
parameter's gradient -- every layer's rnn.*, lstm_init_h, lstm_init_c, linear.*, transitions -- un-padded through the state()
layouts, against float64 torch autograd (deepref.head_torch: torch.nn.LSTMs over pack_padded_sequence started from the initial state,
linear, oracle.train_step.crf_nll_torch).  The bound is the rule of tests/test_gpu_stack_train.py with its factor: relative L2 <= 3 x
the relative L2 of the emulation (deepref.head(store=STORE): the same computation rounded at the device's storage points -- every
layer's bf16 gx, out and dgx, the bf16 h_0, the bf16 masked matrix between two layers) against float64 on the same inputs, in no case
looser than selftest.STEP_TOL's loss_rel, grad_linear.weight and grad_transitions; cosine >= STEP_TOL["grad_min_cos"]; padded entries
of every block receive exactly 0.  With rnn_dropout = 0.5 the masks are restated on the host from the sites the head drew
(mmaref.dropout_mult) and fed to the reference; the last layer's output is unmasked.  A one-layer head without an initial state issues
the library calls it always issued and draws what it always drew; with an all-zero initial state it gives the same loss and
gradients bit for bit.  StackOptimizer: SGD and AdamW move every new tensor as a float64 restatement does, at lr * lr_rate.

Figures of the MI355X run that accompanied this module are in DESIGN.md section 3."""
import numpy as np
import pytest
import torch

import deepref as DR
import lstmbwdref as R
import mmaref
import rowref
import selftest

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
SFX = ("", "_reverse")
LENGTHS = np.array([7, 1, 4])
B, n = 3, 7
SHAPES = [(72, 100, 9), (72, 40, 5)]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(WORST):
        print("[deepstack] worst %-40s rel / emulation %.3f   (rel %.3e, emulation %.3e)" % ((k,) + WORST[k]))


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def problem(D, H, T, L, seed, init=True):
    """a random head in the reference's layout, bf16-valued features, lengths (7, 1, 4), tags"""
    rng = np.random.default_rng(seed)
    k = 1.0 / np.sqrt(H)
    st = {"rnn": {}}
    for layer in range(L):
        for s in SFX:
            st["rnn"]["weight_ih_l%d%s" % (layer, s)] = rng.uniform(-k, k, (4 * H, D if layer == 0 else 2 * H)).astype(np.float32)
            st["rnn"]["weight_hh_l%d%s" % (layer, s)] = rng.uniform(-k, k, (4 * H, H)).astype(np.float32)
            st["rnn"]["bias_ih_l%d%s" % (layer, s)] = rng.uniform(-k, k, 4 * H).astype(np.float32)
            st["rnn"]["bias_hh_l%d%s" % (layer, s)] = rng.uniform(-k, k, 4 * H).astype(np.float32)
    st["linear.weight"] = rng.uniform(-1, 1, (T, 2 * H)).astype(np.float32) / np.float32(np.sqrt(2 * H)) * 4
    st["linear.bias"] = rng.standard_normal(T).astype(np.float32)
    tr = rng.standard_normal((T, T)).astype(np.float32)
    tr[T - 2, :] = -1e12
    tr[:, T - 1] = -1e12
    st["transitions"] = tr
    if init:       # torch.randn, as the reference draws them
        st["lstm_init_h"] = rng.standard_normal((2 * L, H)).astype(np.float32)
        st["lstm_init_c"] = rng.standard_normal((2 * L, H)).astype(np.float32)
    x = rowref.bf16_round(rng.standard_normal((B, n, D))).astype(np.float64)
    for b in range(B):
        x[b, LENGTHS[b]:] = 0
    tags = rng.integers(0, T - 2, (B, n))
    return R.NS(st=st, lengths=LENGTHS, x=x, tags=tags, blocks=[D - 8, 8], B=B, n=n, D=D, H=H, T=T, L=L, start=T - 2, stop=T - 1)


def build_head(p, trainable=True, init="state"):
    """init: "state" (the problem's, if it has one), "zero" (an all-zero initial state), None"""
    from kbner import stack as K
    st = p.st
    ini = None
    if init == "state" and "lstm_init_h" in st:
        ini = {k: torch.from_numpy(st[k]) for k in ("lstm_init_h", "lstm_init_c")}
    elif init == "zero":
        ini = {k: torch.zeros((2 * p.L, p.H)) for k in ("lstm_init_h", "lstm_init_c")}
    return K.BiLSTMHead({k: torch.from_numpy(v) for k, v in st["rnn"].items()}, st["linear.weight"], st["linear.bias"], p.blocks, p.H,
                        "cuda", transitions=st["transitions"], trainable=trainable, rnn_layers=p.L, init_state=ini)


def device_input(p, head):
    from kbner import batch as kb
    X = head.new_input(p.B, p.n)
    xb = torch.from_numpy(p.x).to(BF16).view(p.B * p.n, p.D)
    ref = 0
    for w, c in zip(p.blocks, head.cols):
        X[:p.B * p.n, c:c + w] = xb[:, ref:ref + w].cuda()
        ref += w
    hb = kb.assemble(np.zeros((p.B, 1), np.int64), np.ones((p.B, 1), np.int64), np.full((p.B, p.n), -1, np.int64), p.tags.astype(np.int64),
                     p.lengths.astype(np.int64), None)
    return X, kb.to_device(hb, "cuda")


def flat_state(g):
    out = {"rnn." + k: v for k, v in g["rnn"].items()}
    out.update({k: g[k] for k in g if k != "rnn"})
    return {k: np.asarray(v.numpy() if hasattr(v, "numpy") else v, np.float64) for k, v in out.items()}


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


def cos(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


CAP = {"loss": selftest.STEP_TOL["loss_rel"], "linear.weight": selftest.STEP_TOL["grad_linear.weight"],
       "transitions": selftest.STEP_TOL["grad_transitions"]}


def compare(what, loss, em, grads, ref, emu):
    """the rule of tests/test_gpu_stack_train.py (compare) with the emissions as one more row"""
    (ref_loss, ref_grads, ref_em), (emu_loss, emu_grads, emu_em) = ref, emu
    assert sorted(grads) == sorted(ref_grads) == sorted(emu_grads)
    fails = []
    rows = [("loss", abs(loss - ref_loss) / abs(ref_loss), abs(emu_loss - ref_loss) / abs(ref_loss), 1.0),
            ("emissions", rel(em, ref_em), rel(emu_em, ref_em), cos(em, ref_em))]
    for k in sorted(ref_grads):
        rows.append((k, rel(grads[k], ref_grads[k]), rel(emu_grads[k], ref_grads[k]), cos(grads[k], ref_grads[k])))
    for k, got, emu_, c in rows:
        bound = min(3.0 * emu_, CAP.get(k, np.inf))
        print("[deepstack] %s %-30s rel %.3e  emulation %.3e  bound %.3e  cos %.6f" % (what, k, got, emu_, bound, c))
        if got / emu_ > WORST.get(k, (0.0,))[0]:
            WORST[k] = (got / emu_, got, emu_)
        if not got <= bound or not c >= selftest.STEP_TOL["grad_min_cos"]:
            fails.append((k, got, bound, c))
    assert not fails, (what, fails)


def references(p, masks=None):
    args = (p.x, p.lengths, p.tags, p.st, p.L, p.start, p.stop)
    return DR.head_torch(*args, masks=masks), DR.head(*args, masks=masks, store=DR.STORE)


def padding_receives_no_gradient(head, p):
    """every block's padded entries: gradient exactly 0 (found by loading an all-ones state: what stays 0 is padding)"""
    g = [head.g.clone()] + [blk.g.clone() for blk in head.blocks_extra()]
    ones = {k: (np.ones_like(v) if k != "rnn" else {kk: np.ones_like(vv) for kk, vv in v.items()}) for k, v in p.st.items()}
    head.load_state(ones)
    for buf, arena in zip(g, [head.arena] + [blk.arena for blk in head.blocks_extra()]):
        pad = arena == 0
        assert bool(pad.any()) and not bool(buf[pad].any()), "a padded entry received a gradient"
    head.load_state(p.st)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("D,H,T", SHAPES)
def test_loss_emissions_and_every_gradient_against_float64_autograd(D, H, T, L):
    p = problem(D, H, T, L, seed=H + T + L)
    head = build_head(p)
    assert head.rnn_dropout == 0.5 and len(head.upper) == L - 1 and head.init is not None
    head.rnn_dropout = 0.0
    head.train(True)
    X, db = device_input(p, head)
    loss = float(head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop))
    torch.cuda.synchronize()
    grads = flat_state(head.grad_state())
    em = head.last_emissions.cpu().numpy().astype(np.float64)
    ref, emu = references(p)
    compare("D%d H%d T%d L%d" % (D, H, T, L), loss, em, grads, ref, emu)
    assert {"lstm_init_h", "lstm_init_c", "rnn.weight_ih_l%d_reverse" % (L - 1)} <= set(grads)
    # emissions(): the inference kernels, no dropout between the layers, the same emissions bit for bit
    assert torch.equal(head.emissions(X, p.lengths, B, n).view(torch.int32), head.last_emissions.view(torch.int32))
    padding_receives_no_gradient(head, p)


@pytest.mark.parametrize("L", [2, 3])
@pytest.mark.parametrize("D,H,T", SHAPES)
def test_dropout_between_the_layers(D, H, T, L):
    p = problem(D, H, T, L, seed=7 * H + L)
    head = build_head(p)
    X, db = device_input(p, head)
    Hp, R_ = head.Hp, B * n
    head.seed_dropout(1234 + L)
    # eval(): nothing is drawn, and emissions() is the training forward with every rate 0
    head.train(False)
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    assert head.last_drop is None
    plain = head.last_emissions.clone()
    assert torch.equal(head.emissions(X, p.lengths, B, n).view(torch.int32), plain.view(torch.int32))
    head.zero_grad()
    head.train(True)
    loss = float(head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop))
    torch.cuda.synchronize()
    word, pre, post, inter = head.last_drop
    assert word is None and pre[0][1] == pre[1][1] == post[0][1] == post[1][1] == 0           # only the sites between the layers act
    assert len(inter) == L - 1 and len({s for s, _ in inter}) == L - 1 and all(t == mmaref.dropout_thresh(0.5) for _, t in inter)
    masks = []
    for seed, th in inter:     # the element site of the [B * n, 2Hp] matrix, restated on the host
        m = mmaref.dropout_mult(1, R_, 2 * Hp, seed, th)[0].astype(np.float64).reshape(B, n, 2 * Hp)
        assert set(np.unique(m)) == {0.0, 2.0} and 0.4 < float((m == 0).mean()) < 0.6
        masks.append(DR.unpad_cols(m, H, Hp))
    assert not torch.equal(head.last_emissions, plain)
    # the last layer's output is unmasked: no live element of it is an exact zero
    out = head.last_out[:R_].float().cpu().numpy().reshape(B, n, 2 * Hp)
    assert (DR.unpad_cols(out, H, Hp)[0] != 0).all() and not out[1, 1:].any()
    ref, emu = references(p, masks)
    compare("D%d H%d T%d L%d dropout" % (D, H, T, L), loss, head.last_emissions.cpu().numpy().astype(np.float64),
            flat_state(head.grad_state()), ref, emu)


class Calls:
    def __init__(self, monkeypatch):
        from kbner import lib as L_
        self.names = []
        call = L_.call

        def spy(name, *a):
            self.names.append(name)
            return call(name, *a)
        monkeypatch.setattr(L_, "call", spy)


def test_a_one_layer_head_without_initial_state_issues_the_calls_and_draws_it_always_did(monkeypatch):
    """the literal list: the stages of BiLSTMHead.loss_backward as they stood before layers and the initial state"""
    D, H, T = SHAPES[0]
    p = problem(D, H, T, 1, seed=5, init=False)
    head = build_head(p)
    assert head.upper == [] and head.init is None and head.blocks_extra() == [] and head.rnn_dropout == 0.0
    X, db = device_input(p, head)
    head.dropout, head.locked_dropout, head.word_dropout = 0.25, 0.5, 0.3
    head.seed_dropout(99)
    head.train(True)
    calls = Calls(monkeypatch)
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    torch.cuda.synchronize()
    assert calls.names == ["kbner_gather_rows_drop", "kbner_gemm_bf16", "kbner_lstm_seq_train", "kbner_gather_rows_drop", "kbner_head_fwd",
                           "kbner_gather_rows_f32", "kbner_crf_nll_fwd", "kbner_wdiff_sum", "kbner_crf_nll_bwd", "kbner_scatter_add_rows_f32",
                           "kbner_head_bwd_dx", "kbner_head_bwd_dw", "kbner_scatter_rows_drop", "kbner_lstm_seq_bwd", "kbner_gemm_bf16",
                           "kbner_gemm_bf16", "kbner_colsum", "kbner_colsum"]
    # the draws: WordDropout's n uniforms, then four seeds -- and nothing after them
    from kbner import ops
    rng = np.random.default_rng(99)
    word = rng.random(n) < 0.3
    sd = rng.integers(0, 2 ** 32, size=4, dtype="uint64")
    te, tl = ops.drop_thresh(0.25), ops.drop_thresh(0.5)
    assert len(head.last_drop) == 3 and np.array_equal(head.last_drop[0], word)
    assert head.last_drop[1:] == (((int(sd[0]), te), (int(sd[1]), tl)), ((int(sd[2]), te), (int(sd[3]), tl)))
    assert head._drop_rng.random() == rng.random()
    # all rates 0: nothing is drawn at all
    head.dropout = head.locked_dropout = head.word_dropout = 0.0
    calls.names.clear()
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    assert head.last_drop is None and calls.names == [
        "kbner_gemm_bf16", "kbner_lstm_seq_train", "kbner_head_fwd", "kbner_gather_rows_f32", "kbner_crf_nll_fwd", "kbner_wdiff_sum",
        "kbner_crf_nll_bwd", "kbner_scatter_add_rows_f32", "kbner_head_bwd_dx", "kbner_head_bwd_dw", "kbner_lstm_seq_bwd", "kbner_gemm_bf16",
        "kbner_gemm_bf16", "kbner_colsum", "kbner_colsum"]
    calls.names.clear()
    head.emissions(X, p.lengths, B, n)
    assert calls.names == ["kbner_gemm_bf16", "kbner_lstm_seq", "kbner_head_fwd"]


def test_a_two_layer_head_with_initial_state_walks_every_layer_through_the_new_entry(monkeypatch):
    D, H, T = SHAPES[1]
    p = problem(D, H, T, 2, seed=6)
    head = build_head(p)
    X, db = device_input(p, head)
    head.train(True)
    calls = Calls(monkeypatch)
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    torch.cuda.synchronize()
    c = calls.names.count
    assert c("kbner_lstm_seq_train") == 2 and c("kbner_lstm_seq_bwd_init") == 2 and c("kbner_lstm_seq_bwd") == 0
    assert c("kbner_gather_rows_drop") == 2 and c("kbner_scatter_rows_drop") == 1        # (pre-RNN sites with rate 0, one site between)
    assert c("kbner_colsum") == 4 and c("kbner_colsum_rows_f32") == 8 and c("kbner_gemm_bf16") + c("kbner_gemm_bf16_grouped") == 7


@pytest.mark.parametrize("D,H,T", SHAPES)
def test_a_one_layer_head_with_an_all_zero_initial_state_is_the_plain_head_bit_for_bit(D, H, T):
    p = problem(D, H, T, 1, seed=H, init=False)
    plain, zero = build_head(p, init=None), build_head(p, init="zero")
    assert plain.init is None and zero.init is not None and not bool(zero.init.arena.any())
    X, db = device_input(p, plain)
    la = plain.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    lb = zero.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    torch.cuda.synchronize()
    assert torch.equal(la.view(torch.int32), lb.view(torch.int32))
    assert torch.equal(plain.last_emissions.view(torch.int32), zero.last_emissions.view(torch.int32))
    assert torch.equal(plain.g.view(torch.int32), zero.g.view(torch.int32))
    assert bool(zero.init.g.any())                       # ... and the zero state receives its gradient
    assert torch.equal(plain.emissions(X, p.lengths, B, n).view(torch.int32), zero.emissions(X, p.lengths, B, n).view(torch.int32))


@pytest.mark.parametrize("name", ["SGD", "AdamW"])
def test_optimizer_steps_move_every_new_tensor_as_a_float64_restatement_does(name):
    from kbner import stack as K
    D, H, T = SHAPES[0]
    p = problem(D, H, T, 2, seed=17)
    head = build_head(p)
    head.rnn_dropout = 0.0
    back = flat_state(head.state())
    want_st = flat_state(p.st)
    assert sorted(back) == sorted(want_st) and all(np.array_equal(back[k], want_st[k]) for k in back)        # state() is the inverse
    X, db = device_input(p, head)
    ref_loss, ref_grads, _ = DR.head_torch(p.x, p.lengths, p.tags, p.st, p.L, p.start, p.stop)
    gnorm = float(np.sqrt(sum((v ** 2).sum() for v in ref_grads.values())))
    opt = K.StackOptimizer(head, name=name, lr=0.1 if name == "SGD" else 1e-3, lr_rate=0.5, max_norm=gnorm / 2)
    rates = {g[0]: g[2] for g in opt.groups()}
    assert rates["rnn layer 1"] == rates["lstm_init"] == rates["rnn+transitions"] == opt.lr * 0.5 and rates["linear"] == opt.lr
    head.loss_backward(X, p.lengths, B, n, db, p.start, p.stop)
    nsq = float(opt.step()[0])
    torch.cuda.synchronize()
    assert abs(np.sqrt(nsq) - gnorm) / gnorm < 1e-2, "the clip norm does not cover every block"
    assert not bool(head.g.any()) and all(not bool(blk.g.any()) for blk in head.blocks_extra())
    new = flat_state(head.state())
    clip = (gnorm / 2) / (gnorm + 1e-6)
    for k, g in ref_grads.items():
        lr = opt.lr * (1.0 if k.startswith("linear.") else opt.lr_rate)
        if name == "SGD":
            want = -lr * clip * g
        else:     # first AdamW step: m / (sqrt(v) + eps) = g / (|g| + eps'), step size lr
            gc = clip * g
            want = -lr * gc / (np.abs(gc) + 1e-6 / np.sqrt(1 - 0.999))
        delta = new[k] - want_st[k]
        live = np.abs(g) > 1e-3 * np.abs(g).max()
        c = cos(delta[live], want[live])
        print("[deepstack] %s first step %-30s update cosine %.6f" % (name, k, c))
        assert c > selftest.TRAIN_TOL["delta_cos_min"], (name, k, c)
    # what the next forward reads is the bf16 rounding of the new values
    lay = head.upper[0]
    assert torch.equal(lay.shadow, lay.arena[:lay.n_shadow].to(BF16)) and torch.equal(lay.wih.reshape(-1), lay.param("wih").to(BF16).reshape(-1))
    assert torch.equal(lay.grp.whh.reshape(-1), lay.param("whh").to(BF16).reshape(-1))
    assert torch.equal(head.init.h16, head.init.param("h").to(BF16))
    assert not bool(head.init.param("h")[:, H:].any()) and not bool(head.init.param("c")[:, H:].any())      # padding stays 0
