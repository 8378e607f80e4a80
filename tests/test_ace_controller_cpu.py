"""CPU: the ACE controller and ReinforcementTrainer's episode loop (flair.models.controller.EmbedController,
flair.trainers.reinforcement_trainer) -- no kernel runs: the controller is host arithmetic, and the episode loop is driven through a
stub of the stacked tagger's epoch run whose dev scores are scripted.

The float64 reference is tests/aceref.py.  Bound of the float32 update against it: 64 * 2^-23 * max(1, max|lr * R|) absolute -- the
update is a handful of float32 operations (a sum of a few products, a sigmoid, a multiply-add) on values of that size."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import aceref

EPS = 2.0 ** -23


def bound(lr, *rewards):
    return 64 * EPS * max(1.0, max(float(np.max(np.abs(lr * np.asarray(R, np.float64)))) for R in rewards))


def _sgd(controller, lr=0.1, momentum=0.9):
    return torch.optim.SGD(controller.parameters(), lr=lr, momentum=momentum)


# ====================================================================== the update
def test_worked_example():
    """3 actions, selector zeros, {(1,1,1): [60], (1,0,1): [62]}, the episode trained (0,0,1) to 61, discount 0.5, SGD lr 0.1
    momentum 0.9, first step.  By hand: against (1,1,1) r = 1, two positions differ -> 1 * 0.5^1 on positions 0 and 1; against (1,0,1)
    r = -1, one position differs -> -1 * 0.5^0 on position 0: R = (-0.5, 0.5, 0).  dloss/ds_k = -R_k (a_k - 0.5) = (-0.25, 0.25, 0):
    selector (0.025, -0.025, 0)."""
    from flair.models.controller import EmbedController
    from flair.trainers.reinforcement_trainer import ace_reward, controller_step
    c = EmbedController(3)
    assert c.selector.dtype == torch.float32 and c.selector.device.type == "cpu" and not bool(c.selector.any())
    action = torch.tensor([0.0, 0.0, 1.0])
    table = {(1.0, 1.0, 1.0): {"counts": 1, "scores": [60]}, (1.0, 0.0, 1.0): {"counts": 1, "scores": [62]}}
    R = ace_reward(action, 61, table, discount=0.5)
    assert R.dtype == torch.float32 and R.tolist() == [-0.5, 0.5, 0.0]
    assert np.array_equal(aceref.reward([0, 0, 1], 61, table, discount=0.5), [-0.5, 0.5, 0.0])
    controller_step(_sgd(c), c.log_prob(c.get_value(), action), R)
    got = c.selector.detach().numpy().astype(np.float64)
    assert np.max(np.abs(got - np.array([0.025, -0.025, 0.0]))) <= bound(0.1, R.numpy())
    assert float(got[2]) == 0.0


def _random_table(rng, n, k):
    table, k = {}, min(k, 2 ** n - 1)     # there are no more non-zero actions than that
    while len(table) < k:
        a = tuple(float(x) for x in rng.integers(0, 2, n))
        if sum(a) > 0:
            table[a] = {"counts": 1, "scores": [float(x) for x in rng.uniform(40, 95, rng.integers(1, 4))]}
    return table


@pytest.mark.parametrize("opts", [{}, {"log_reward": True}, {"sqrt_reward": True}, {"log_reward": True, "sqrt_reward": True},
                                  {"old_reward": True}], ids=["plain", "log", "sqrt", "log_sqrt", "old"])
def test_update_parity_with_the_float64_reference(opts):
    """two consecutive steps (the second with the momentum buffer of the first) over random action tables; each step is compared
    from the mirror's own float32 state, so the bound is one step's"""
    from flair.models.controller import EmbedController
    from flair.trainers.reinforcement_trainer import ace_reward, controller_step
    rng = np.random.default_rng(7)
    lr, mu = 0.1, 0.9
    for case in range(40):
        n = int(rng.integers(2, 10))
        discount = float(rng.choice([0.3, 0.5, 1.0]))
        c = EmbedController(n)
        with torch.no_grad():
            c.selector.copy_(torch.from_numpy(rng.uniform(-2, 2, n).astype(np.float32)))
        opt = _sgd(c, lr, mu)
        buf, seen = None, []
        for step in range(2):
            table = _random_table(rng, n, int(rng.integers(1, 7)))
            action = list(table)[0] if case % 5 == 0 else tuple(float(x) for x in np.maximum(rng.integers(0, 2, n), np.eye(n)[0]))
            best, base = float(rng.uniform(40, 95)), float(rng.uniform(40, 95))
            s0 = c.selector.detach().numpy().astype(np.float64)
            R = ace_reward(torch.tensor(action), best, table, baseline_score=base, discount=discount, **opts)
            R64 = aceref.reward(action, best, table, baseline_score=base, discount=discount, **opts)
            seen.append(R64)
            tol = bound(lr, *seen)
            assert np.max(np.abs(lr * (R.numpy().astype(np.float64) - R64))) <= tol
            opt.zero_grad()
            a = torch.tensor(action)
            lp = c.log_prob(c.get_value(), a)
            assert np.max(np.abs(lp.detach().numpy() - aceref.log_prob(s0, action))) <= 64 * EPS
            controller_step(opt, lp, R)
            want, buf = aceref.sgd_step(s0, action, R64, lr, mu, buf)
            got = c.selector.detach().numpy().astype(np.float64)
            assert np.max(np.abs(got - want)) <= tol, (case, step, got, want, tol)
            buf = opt.state[c.selector]["momentum_buffer"].numpy().astype(np.float64)    # step 2 starts from the mirror's float32 state


def test_reward_options_by_hand():
    from flair.trainers.reinforcement_trainer import ace_reward
    table = {(1.0, 1.0, 1.0): {"counts": 1, "scores": [60, 52]}, (1.0, 0.0, 1.0): {"counts": 2, "scores": [45, 64]}}
    action = torch.tensor([0.0, 1.0, 1.0])
    # against (1,1,1): r = 69 - 60 = 9, one position differs (0) -> 9; against (1,0,1): r = 69 - 64 = 5, two differ (0, 1) -> 5 d
    assert ace_reward(action, 69, table, discount=0.5).tolist() == [11.5, 2.5, 0.0]
    assert ace_reward(action, 69, table, discount=1.0).tolist() == [14.0, 5.0, 0.0]
    got = ace_reward(action, 69, table, discount=0.5, sqrt_reward=True).numpy()
    assert np.allclose(got, [3.0 + 0.5 * 5 ** 0.5, 0.5 * 5 ** 0.5, 0.0], rtol=0, atol=8 * EPS * 4)
    got = ace_reward(action, 69, table, discount=0.5, log_reward=True).numpy()
    assert np.allclose(got, [np.log(10.0) + 0.5 * np.log(6.0), 0.5 * np.log(6.0), 0.0], rtol=0, atol=8 * EPS * 4)
    # a worse episode is punished: the sign survives log and sqrt
    got = ace_reward(action, 51, table, discount=0.5, sqrt_reward=True).numpy()
    assert np.allclose(got, [-3.0 - 0.5 * 13 ** 0.5, -0.5 * 13 ** 0.5, 0.0], rtol=0, atol=8 * EPS * 8)
    assert ace_reward(action, 69, table, baseline_score=64.5, old_reward=True).tolist() == [4.5, 4.5, 4.5]
    # the same action as one tried before: nothing differs, the division by the discount (ham - 1 = -1) multiplies zeros
    assert ace_reward(torch.tensor([1.0, 1.0, 1.0]), 70, {(1.0, 1.0, 1.0): {"counts": 1, "scores": [60]}}, discount=0.5).tolist() == [0, 0, 0]


# ====================================================================== sampling
def test_sampling_from_a_fixed_seed():
    from flair.models.controller import EmbedController
    c = EmbedController(3)
    twin = EmbedController(3)
    prev, seq = None, []
    for _ in range(300):      # p = 1/2 each: an unconstrained draw is all zero 1 time in 8 and repeats the last one 1 time in 8
        a, lp = c.sample()
        assert a.dtype == torch.float32 and set(a.tolist()) <= {0.0, 1.0}
        assert float(a.sum()) > 0
        assert prev is None or not torch.equal(a, prev)
        assert torch.equal(c.previous_selection, a)
        assert np.max(np.abs(lp.detach().numpy() - aceref.log_prob(np.zeros(3), a.tolist()))) <= 64 * EPS
        assert lp.requires_grad
        prev = a.clone()
        seq.append(a.tolist())
    assert seq == [twin.sample()[0].tolist() for _ in range(300)], "two controllers of one configuration draw the same curriculum"
    # the frequencies: one logit at +20 rules the all-zero draw out and previous_selection = None the other rejection, so every
    # other position is a plain Bernoulli(sigmoid(selector)) draw
    c = EmbedController(5)
    logits = [20.0, -1.0, 0.5, 0.0, 2.0]
    with torch.no_grad():
        c.selector.copy_(torch.tensor(logits))
    N, count = 4000, np.zeros(5)
    for _ in range(N):
        c.previous_selection = None
        a, lp = c.sample()
        assert bool(torch.isfinite(lp).all())
        count += a.numpy()
    p = aceref.sigmoid(logits)
    for k in range(1, 5):
        assert abs(count[k] / N - p[k]) <= 4 * np.sqrt(p[k] * (1 - p[k]) / N), (k, count[k] / N, p[k])
    assert count[0] == N


def test_controller_round_trip(tmp_path):
    from flair.models.controller import EmbedController
    c = EmbedController(4, state_size=20)
    with torch.no_grad():
        c.selector.copy_(torch.tensor([0.25, -1.5, 0.0, 3.0]))
    c.sample()
    c.best_action = torch.tensor([1.0, 0.0, 0.0, 1.0])
    c.save(tmp_path / "controller.pt")
    raw = torch.load(str(tmp_path / "controller.pt"), map_location="cpu", weights_only=False)
    assert {"state_dict", "num_actions", "model_structure", "state_size"} <= set(raw)
    assert raw["num_actions"] == 4 and raw["model_structure"] is None and raw["state_size"] == 20
    assert list(raw["state_dict"]) == ["selector"]
    back = EmbedController.load(tmp_path / "controller.pt")
    assert torch.equal(back.selector, c.selector) and back.selector.requires_grad
    assert torch.equal(back.previous_selection, c.previous_selection) and torch.equal(back.best_action, c.best_action)
    assert [back.sample()[0].tolist() for _ in range(20)] == [c.sample()[0].tolist() for _ in range(20)]
    with pytest.raises(NotImplementedError, match="Controller.model_structure"):
        EmbedController(4, model_structure="sentence")


# ====================================================================== the episode loop
NAMES = ["a", "b", "c", "d"]
WEIGHT = {"a": 3.0, "b": -2.0, "c": 1.5, "d": 0.25}


def scripted_score(action, epoch):
    """the dev score of an epoch under an action: what the stub 'trains' to.  Best at epoch 1 of 3; b hurts, a / c / d help"""
    return 60.0 + sum(WEIGHT[n] * x for n, x in zip(NAMES, action)) + [0.0, 1.0, 0.5][epoch]


class StubModel:
    use_rnn = True
    multi_view_training = False

    def __init__(self):
        self.embeddings = SimpleNamespace(embeddings=[SimpleNamespace(name=n) for n in reversed(NAMES)])   # the trainer sorts names
        self.selection = None
        self.loaded = []

    def load_stack_state(self, st):
        self.loaded.append(st)


class StubRun:
    """finetune_trainer._StackRun's interface with scripted scores; records what the loop did"""

    def __init__(self, trainer, base_path, a):
        base_path.mkdir(parents=True, exist_ok=True)
        self.model, self.a, self.eval_bs = trainer.model, a, 2
        self.dev_score_history, self.dev_loss_history, self.train_loss_history = [], [], []
        self.episodes, self.prefills, self.saved, self.closed = [], 0, [], False
        self.stop_after = None

    def prefill(self):
        assert not self.episodes
        self.prefills += 1

    def new_optimizer(self):
        self.episodes.append({"action": None, "epochs": 0, "min_lr": None})

    def epoch(self, epoch):
        ep = self.episodes[-1]
        action = tuple(float(x) for x in self.model.selection)
        assert ep["action"] in (None, action)
        ep["action"], ep["epochs"] = action, ep["epochs"] + 1
        score = scripted_score(action, epoch)
        self.dev_score_history.append(score)
        return score

    def track(self, score):
        return True

    def anneal(self, min_learning_rate=None):
        self.episodes[-1]["min_lr"] = min_learning_rate
        return False

    def save_model(self, path):
        self.saved.append((len(self.episodes) - 1, self.dev_score_history[-1]))
        torch.save({"episode": len(self.episodes) - 1, "score": self.dev_score_history[-1]}, str(path))

    def log_store(self):
        pass

    def close(self):
        self.closed = True


def _trainer(config=None, model=None, **kw):
    from flair.trainers import ReinforcementTrainer

    class Trainer(ReinforcementTrainer):
        def _open_stack_run(self, base_path, a):
            self.run = StubRun(self, base_path, a)
            return self.run
    corpus = SimpleNamespace(targets=[], test=None)
    return Trainer(model or StubModel(), None, corpus, optimizer="SGD", controller_optimizer="SGD", controller_learning_rate=0.1,
                   config=config if config is not None else {"Controller": {"model_structure": None}}, **kw)


TRAIN = dict(learning_rate=0.1, mini_batch_size=2, max_epochs=3, controller_momentum=0.9, discount=0.5, embeddings_storage_mode="none")


def _expected(curriculum, lr=0.1, mu=0.9, discount=0.5):
    """the bookkeeping of the search restated from the issue, from a curriculum and the scripted scores -> per episode (action_dict,
    baseline_score, best_action), and the float64 selector after the last one"""
    table, baseline, best_action, out = {}, 0.0, None, []
    s, buf = np.zeros(len(NAMES)), None
    for e, action in enumerate(curriculum):
        action = tuple(action)
        best = max(scripted_score(action, k) for k in range(3))
        if e == 0:
            baseline, best_action = best, action
        else:
            R = aceref.reward(action, best, table, discount=discount)
            s, buf = aceref.sgd_step(s, action, R, lr, mu, buf)
            if best >= baseline:
                baseline, best_action = best, action
        ent = table.setdefault(action, {"counts": 0, "scores": []})
        ent["counts"] += 1
        ent["scores"].append(best)
        out.append(({k: {"counts": v["counts"], "scores": list(v["scores"])} for k, v in table.items()}, baseline, best_action))
    return out, s


def test_episode_loop_bookkeeping_and_files(tmp_path):
    EP = 5
    full = _trainer()
    res = full.train(tmp_path / "full", max_episodes=EP, **TRAIN)
    assert set(res) == {"test_score", "dev_score_history", "test_score_history", "train_loss_history", "dev_loss_history",
                        "test_loss_history"} and res["test_score"] == 0.0 and len(res["dev_score_history"]) == 3 * EP
    run = full.run
    assert run.closed and run.prefills == 1 and len(run.episodes) == EP and all(e["epochs"] == 3 for e in run.episodes)
    assert all(e["min_lr"] == pytest.approx(0.1 / 1000) for e in run.episodes)           # learning_rate / 1000, whatever is passed
    curriculum = json.loads((tmp_path / "full" / "curriculum.json").read_text())
    assert len(curriculum) == EP and curriculum[0] == [1.0] * 4                          # episode 1 trains every embedding
    assert [list(e["action"]) for e in run.episodes] == curriculum
    assert all(x != y for x, y in zip(curriculum, curriculum[1:])) and all(sum(x) > 0 for x in curriculum)
    want, s64 = _expected(curriculum)
    # after each episode: a run of k episodes ends in the state the full run passed through
    for k in range(1, EP + 1):
        t = _trainer()
        t.train(tmp_path / ("k%d" % k), max_episodes=k, **TRAIN)
        st = torch.load(str(tmp_path / ("k%d" % k) / "training_state.pt"), map_location="cpu", weights_only=False)
        assert set(st) == {"episode", "best_action", "baseline_score", "action_dict"}
        assert type(st["episode"]) is int and st["episode"] == k - 1
        assert isinstance(st["best_action"], torch.Tensor) and st["best_action"].dtype == torch.float32
        assert isinstance(st["baseline_score"], float) and isinstance(st["action_dict"], dict)
        table, baseline, best_action = want[k - 1]
        assert tuple(st["best_action"].tolist()) == best_action and st["baseline_score"] == baseline
        got = st["action_dict"]
        assert all(type(key) is tuple and all(type(x) is float for x in key) for key in got)
        assert list(got) == list(table)
        for key in table:      # training_state.pt is written before the averages exist; train() adds them to its own dict at the end
            assert got[key]["counts"] == table[key]["counts"] and got[key]["scores"] == table[key]["scores"]
            assert t.action_dict[key]["average"] == sum(table[key]["scores"]) / table[key]["counts"]
        assert torch.equal(t.best_action, st["best_action"]) and torch.equal(t.controller.best_action, st["best_action"])
        assert tuple(float(x) for x in t.model.selection) == best_action                # the model is left at the best action ...
        assert t.model.loaded and t.model.loaded[-1]["score"] == baseline               # ... with the head that reached the baseline
        assert json.loads((tmp_path / ("k%d" % k) / "curriculum.json").read_text()) == curriculum[:k]
        for f in ("controller.pt", "controller_optimizer_state.pt", "stack-model.pt"):
            assert (tmp_path / ("k%d" % k) / f).exists()
    # the selector against the float64 replay of the same curriculum (EP - 1 updates, each within one step's bound)
    rewards = [aceref.reward(tuple(curriculum[e]), max(scripted_score(curriculum[e], k) for k in range(3)), want[e - 1][0], discount=0.5)
               for e in range(1, EP)]
    got = full.controller.selector.detach().numpy().astype(np.float64)
    assert np.max(np.abs(got - s64)) <= (EP - 1) * bound(0.1, *rewards), (got, s64)
    assert np.any(got != 0)
    # stack-model.pt is written whenever an epoch's score reaches the baseline, the last time by the episode best_action names
    assert run.saved[-1][1] == want[-1][1]
    assert list(run.episodes[run.saved[-1][0]]["action"]) == list(want[-1][2])


def test_random_search_leaves_the_selector_untouched(tmp_path):
    t = _trainer()
    t.train(tmp_path / "rs", max_episodes=4, random_search=True, **TRAIN)
    assert not bool(t.controller.selector.any())
    curriculum = json.loads((tmp_path / "rs" / "curriculum.json").read_text())
    assert len(curriculum) == 4 and [list(e["action"]) for e in t.run.episodes] == curriculum
    # old_reward: the baseline has been raised by the episode's own epochs, so the reward is best - baseline <= 0 everywhere
    t = _trainer()
    t.train(tmp_path / "old", max_episodes=3, old_reward=True, **TRAIN)
    assert bool(torch.isfinite(t.controller.selector).all())


def test_curriculum_file_replays_the_recorded_actions(tmp_path):
    a = _trainer()
    a.train(tmp_path / "a", max_episodes=4, **TRAIN)
    b = _trainer()
    b.train(tmp_path / "b", max_episodes=4, curriculum_file=str(tmp_path / "a" / "curriculum.json"), **TRAIN)
    assert [e["action"] for e in b.run.episodes] == [e["action"] for e in a.run.episodes]
    assert b.action_dict == a.action_dict and torch.equal(b.controller.selector, a.controller.selector)
    assert (tmp_path / "b" / "curriculum.json").read_text() == (tmp_path / "a" / "curriculum.json").read_text()
    # a curriculum of its own choosing, starting at a subset: applied as written
    forced = [[1.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]]
    (tmp_path / "forced.json").write_text(json.dumps(forced))
    c = _trainer()
    c.train(tmp_path / "c", max_episodes=3, curriculum_file=str(tmp_path / "forced.json"), **TRAIN)
    assert [list(e["action"]) for e in c.run.episodes] == forced
    assert tuple(c.best_action.tolist()) == max((tuple(x) for x in forced), key=lambda x: scripted_score(x, 1))


def test_continue_training_goes_on_where_the_search_stopped(tmp_path):
    EP, K = 6, 3
    a = _trainer()
    a.train(tmp_path / "a", max_episodes=EP, **TRAIN)
    b = _trainer()
    b.train(tmp_path / "b", max_episodes=K, **TRAIN)
    c = _trainer()                                # a new process: nothing but the files
    c.train(tmp_path / "b", max_episodes=EP, continue_training=True, **TRAIN)
    assert len(c.run.episodes) == EP - K          # resumes at the saved episode + 1
    assert c.model.loaded[0]["episode"] <= K - 1  # stack-model.pt of the interrupted run was loaded first
    assert (tmp_path / "b" / "curriculum.json").read_text() == (tmp_path / "a" / "curriculum.json").read_text()
    assert [e["action"] for e in c.run.episodes] == [e["action"] for e in a.run.episodes[K:]]
    assert torch.equal(c.controller.selector, a.controller.selector)
    assert c.action_dict == a.action_dict and torch.equal(c.best_action, a.best_action)
    sa = torch.load(str(tmp_path / "a" / "training_state.pt"), map_location="cpu", weights_only=False)
    sb = torch.load(str(tmp_path / "b" / "training_state.pt"), map_location="cpu", weights_only=False)
    assert sa["episode"] == sb["episode"] == EP - 1 and sa["baseline_score"] == sb["baseline_score"]


# ====================================================================== refusals
def test_refusals_by_name(tmp_path):
    from flair.embeddings import ELMoEmbeddings, FastWordEmbeddings
    d = tmp_path / "refused"

    def refused(exc, match, trainer=None, **kw):
        t = trainer or _trainer()
        with pytest.raises(exc, match=match):
            t.train(d, max_episodes=2, **dict(TRAIN, **kw))
        assert not d.exists(), "a refused search writes nothing"
        assert getattr(t, "run", None) is None
    # everything the stacked tagger's loop refuses
    refused(NotImplementedError, "checkpoint", checkpoint=True)
    refused(NotImplementedError, "train_with_dev", train_with_dev=True)
    for flag in ("use_amp", "rootschedule", "freezing"):
        refused(NotImplementedError, flag, **{flag: True})
    t = _trainer()
    t.distill_mode = True
    refused(NotImplementedError, "distill_mode", trainer=t)
    refused(NotImplementedError, "checkpoint", trainer=_trainer(optimizer_state={"t": 1}))
    # the search's own
    m = StubModel()
    m.use_rnn = False
    refused(NotImplementedError, "use_rnn", trainer=_trainer(model=m))
    refused(NotImplementedError, r"Controller\.model_structure", trainer=_trainer(config={"Controller": {"model_structure": "sentence"}}))
    refused(NotImplementedError, "monitor_train", monitor_train=True)
    for emb in (ELMoEmbeddings(options_file="elmo_2x4096_512_2048cnn_2xhighway_options.json"), FastWordEmbeddings(embeddings="en")):
        m = StubModel()
        m.embeddings.embeddings.append(emb)
        t = _trainer(model=m)
        refused(NotImplementedError, "out of scope", trainer=t)
        with pytest.raises(NotImplementedError, match="embeddings:") as e:
            t.train(d, **TRAIN)
        assert emb.name in str(e.value)
    for bad in (0.0, -0.5, 1.5):
        refused(ValueError, "discount", discount=bad)
    # accepted and without effect, as in the reference's loop
    t = _trainer()
    t.train(tmp_path / "inert", max_episodes=2, one_by_one=True, select_model_by_macro=True, **TRAIN)
    assert t.run.a["select_model_by_macro"] is False and len(t.run.episodes) == 2
    # no Controller block at all: the embedding-level controller over len(embeddings) actions
    t = _trainer(config={})
    assert t.controller.num_actions == 4 and t.model.use_rl and t.model.embedding_selector and t.model.selection == [1] * 4
