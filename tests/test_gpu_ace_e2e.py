"""GPU: ReinforcementTrainer.train, the ACE controller's search, end to end on a tiny stack of three frozen encoders (tiny_assets
seeds 0, 5, 9; hidden_size 40, mini_batch_size 2, 6 / 3 / 3 sentences, 3 episodes of 2 epochs, SGD for the head and the controller).

  (a) one episode is plain stack training: with max_episodes 1 the losses of the first optimizer step equal those of
      ModelFinetuner.train on the same YAML values bit for bit, the later ones and the total update of stack-model.pt agree within
      selftest.TRAIN_TOL (the rule of test_gpu_store_e2e.py: weight gradients accumulate with fp32 atomics);
  (b) the selection is applied: a curriculum forces (1, 0, 1) in episode 2, whose first loss is forward_backward of a fresh tagger
      holding episode 1's final weights with selection [1, 0, 1] -- and not that of the full selection;
  (c) between episodes the optimizer is new (t = 1 at its first step, lr scale 1) while the weights carry over (that is (b));
  (d) with embeddings_storage_mode "gpu" the feature producers run once per batch for the WHOLE search: the encoder_forward count
      stays at the prefill's from the first optimizer step to the last, for the sampled run and for a curriculum that starts at a
      subset; with "none" every episode launches exactly the encoders its action selects;
  (e) the files, and best_action = the action of the episode that reached baseline_score;
  (f) the command line: train.py --config trains (twice: the same curriculum.json), --test then evaluates with that selection."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import selftest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N_TRAIN, N_DEV, N_TEST, MBS, EPOCHS, EPISODES, ENC = 6, 3, 3, 2, 2, 3, 3
STEPS = N_TRAIN // MBS                     # optimizer steps per epoch (gradient_accumulation_steps 1)
FORCED = [[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]]


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error after a test; nothing more is launched: %s" % e, returncode=3)


def _np_state(st):
    return np.concatenate([np.asarray(st["rnn"][k], np.float64).ravel() for k in sorted(st["rnn"])] +
                          [np.asarray(st[k], np.float64).ravel() for k in ("linear.weight", "linear.bias", "transitions")])


def cos(a, b):
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


def _config(root, name, trainer, storage, **train):
    import yaml
    tblock = {"distill_mode": False, "optimizer": "SGD", "sentence_level_batch": True}
    if trainer == "ReinforcementTrainer":
        tblock.update(controller_optimizer="SGD", controller_learning_rate=0.1)
    cfg = {trainer: tblock, "Controller": {"model_structure": None},
           "embeddings": {"TransformerWordEmbeddings-%d" % i: {"layers": "-1", "model": str(root / d), "pooling_operation": "first"}
                          for i, d in enumerate(("enc_a", "enc_b", "enc_c"))},
           "model": {"FastSequenceTagger": {"dropout": 0.0, "word_dropout": 0.0, "locked_dropout": 0.0, "hidden_size": 40,
                                            "use_rnn": True, "sentence_loss": True, "use_crf": True}},
           "model_name": name, "target_dir": str(root / "out"), "targets": "ner", "trainer": trainer,
           "ner": {"Corpus": "ColumnCorpus-TINY", "tag_dictionary": str(root / "tags.pkl"),
                   "ColumnCorpus-TINY": {"column_format": {0: "text", 1: "pos", 2: "upos", 3: "ner"}, "comment_symbol": "# id",
                                         "data_folder": str(root / "data"), "tag_to_bioes": "ner"}},
           "train": dict({"learning_rate": 0.05, "lr_rate": 2.0, "max_epochs": EPOCHS, "mini_batch_size": MBS,
                          "gradient_accumulation_steps": 1, "monitor_test": False, "train_with_dev": False, "shuffle": True,
                          "embeddings_storage_mode": storage}, **train)}
    if trainer == "ReinforcementTrainer":
        cfg["train"].update(controller_momentum=0.9, discount=0.5)
    path = root / ("%s.yaml" % name)
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the trainer runs every test below reads, each from the same seed -> per run: the losses and batches of every optimizer step,
    which encoder ran when, the optimizer at every step, the head's weights after every step, the files"""
    import tiny_assets
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    from kbner import engine
    root = tmp_path_factory.mktemp("ace")
    for d, seed in (("enc_a", 0), ("enc_b", 5), ("enc_c", 9)):
        tiny_assets.build_model_dir(str(root / d), seed=seed)
    tiny_assets.write_conll_corpus(str(root / "data"), n_train=N_TRAIN, n_dev=N_DEV, n_test=N_TEST, seed=3)
    with open(root / "forced.json", "w") as f:
        f.write(json.dumps(FORCED))
    out = {"root": root}
    mp = pytest.MonkeyPatch()
    try:
        calls = []
        enc = engine.Tagger.encoder_forward

        def encoder_forward(this, *a, **k):
            calls.append(id(this))
            return enc(this, *a, **k)
        mp.setattr(engine.Tagger, "encoder_forward", encoder_forward)
        plan = (("plain", "ModelFinetuner", "gpu", {}),
                ("one", "ReinforcementTrainer", "gpu", {"max_episodes": 1}),
                ("sampled", "ReinforcementTrainer", "gpu", {"max_episodes": EPISODES}),
                ("forced", "ReinforcementTrainer", "gpu", {"max_episodes": EPISODES, "curriculum_file": str(root / "forced.json")}),
                ("forced_none", "ReinforcementTrainer", "none", {"max_episodes": EPISODES, "curriculum_file": str(root / "forced.json")}))
        for name, tname, storage, train in plan:
            path = _config(root, name, tname, storage, **train)
            torch.manual_seed(2024)
            cp = ConfigParser(Params.from_file(str(path)))
            student = cp.create_student()
            trainer = getattr(flair.trainers, tname)(student, None, cp.corpus, config=cp.config, **cp.config[tname])
            start = _np_state(student._stack_state)
            del calls[:]
            steps, episode_at = [], []

            def hook(batches, ls, steps=steps, trainer=trainer, student=student):
                opt = trainer.optimizer
                steps.append(dict(losses=[float(x) for x in ls], calls=len(calls), opt=id(opt), t=opt.t, lr=opt.lr, lr_scale=opt.lr_scale,
                                  batches=batches, state=student._stack_state, selection=[float(x) for x in student.selection]
                                  if student.selection is not None else None))
            trainer.stack_step_hook = hook
            if tname == "ReinforcementTrainer":
                sample = trainer.controller.sample

                def counted(*a, sample=sample, episode_at=episode_at, **k):
                    episode_at.append(len(calls))
                    return sample(*a, **k)
                trainer.controller.sample = counted
            res = trainer.train(cp.get_target_path, **cp.config["train"])
            encoders = [id(student._encoder_for(e)) for e in student._stack_embs]
            out[name] = dict(steps=steps, calls=list(calls), episode_at=episode_at, res=res, start=start, base=cp.get_target_path,
                             encoders=encoders, student=student, trainer=trainer, cfg=path, cp=cp,
                             store_open_after=student.__dict__.get("_feature_store") is not None)
    finally:
        mp.undo()
    return out


def test_a_one_episode_is_plain_stack_training(runs):
    a, b = runs["plain"], runs["one"]
    la, lb = [s["losses"] for s in a["steps"]], [s["losses"] for s in b["steps"]]
    assert len(la) == len(lb) == EPOCHS * STEPS
    assert la[0] == lb[0], "the first optimizer step sees the same features and the same weights"
    worst = max(abs(x - y) / abs(x) for p, q in zip(la, lb) for x, y in zip(p, q))
    assert np.array_equal(a["start"], b["start"])
    best_a = _np_state(torch.load(str(a["base"] / "stack-model.pt"), map_location="cpu", weights_only=False))
    best_b = _np_state(torch.load(str(b["base"] / "stack-model.pt"), map_location="cpu", weights_only=False))
    c = cos(best_a - a["start"], best_b - b["start"])
    print("[ace] one episode against ModelFinetuner.train: worst relative loss difference %.3e, cosine of the total update %.9f" % (worst, c))
    assert worst < selftest.TRAIN_TOL["loss_rel_max"] and c > selftest.TRAIN_TOL["delta_cos_min"]
    assert len(b["res"]["dev_score_history"]) == len(a["res"]["dev_score_history"]) == EPOCHS
    assert [float(x) for x in b["student"].selection] == [1.0] * ENC          # episode 1 trains every embedding


def test_b_the_selection_is_applied_and_the_weights_carry_over(runs):
    import flair
    from flair.config_parser import ConfigParser
    from flair.utils.from_params import Params
    r = runs["forced"]
    per = EPOCHS * STEPS
    assert [s["selection"] for s in r["steps"]] == [FORCED[e] for e in range(EPISODES) for _ in range(per)]
    end_of_1, first_of_2 = r["steps"][per - 1], r["steps"][per]
    torch.manual_seed(2024)
    twin = ConfigParser(Params.from_file(str(r["cfg"]))).create_student()
    twin.load_stack_state(end_of_1["state"])
    twin.embedding_selector = True
    twin.train()
    twin.enable_stack_training()
    batch = first_of_2["batches"][0]
    twin.selection = FORCED[1]
    want = float(twin.forward_backward(batch))
    twin.zero_grad()
    twin.selection = [1.0] * ENC
    full = float(twin.forward_backward(batch))
    print("[ace] episode 2, first loss %r; a tagger in episode 1's final state gives %r under (1,0,1), %r under (1,1,1)"
          % (first_of_2["losses"][0], want, full))
    assert first_of_2["losses"][0] == want and want != full


def test_c_between_episodes_the_optimizer_is_new(runs):
    per = EPOCHS * STEPS
    for name in ("sampled", "forced"):
        steps = runs[name]["steps"]
        assert len(steps) == EPISODES * per
        assert [s["t"] for s in steps] == list(range(1, per + 1)) * EPISODES           # the step count restarts with every episode
        assert len({s["opt"] for s in steps[::per]}) >= 1 and all(s["lr"] == 0.05 and s["lr_scale"] == 1.0 for s in steps)
        opt = runs[name]["trainer"].optimizer
        assert opt.m is None and opt.v is None                                        # SGD keeps no moments; t above is its state
        # the weights are not reset: episode 2 starts from what episode 1 left (a reset would give episode 1's first loss again)
        assert not np.array_equal(_np_state(steps[per - 1]["state"]), runs[name]["start"])


def test_d_producers_run_once_per_batch_for_the_whole_search(runs):
    train_b, dev_b, test_b = N_TRAIN // MBS, 1, 1
    prefill = ENC * (train_b + dev_b)
    for name in ("sampled", "forced"):
        r = runs[name]
        assert [s["calls"] for s in r["steps"]] == [prefill] * (EPISODES * EPOCHS * STEPS), name
        best = [float(x) for x in r["student"].selection]
        assert len(r["calls"]) == prefill + int(sum(best)) * test_b          # the test set is visited once, under the best action
        assert not r["store_open_after"]
        log = open(str(r["base"] / "training.log")).read()
        assert log.count("filled under the full selection") == 1 and "the store refills" not in log
        assert log.count("feature store (gpu):") == EPISODES * (EPOCHS + 1)
    # "none": every episode launches the encoders its action selects, and no other
    r = runs["forced_none"]
    assert len(r["episode_at"]) == EPISODES
    bounds = r["episode_at"] + [len(r["calls"]) - int(sum(float(x) for x in r["student"].selection)) * test_b]
    for e in range(EPISODES):
        ran = r["calls"][bounds[e]:bounds[e + 1]]
        want = [enc for enc, on in zip(r["encoders"], FORCED[e]) if on]
        assert set(ran) == set(want) and len(ran) == len(want) * EPOCHS * (train_b + dev_b), (e, len(ran))
    assert "feature store" not in open(str(r["base"] / "training.log")).read()


def test_e_files_and_best_action(runs):
    for name in ("sampled", "forced"):
        r = runs[name]
        base = r["base"]
        for f in ("training.log", "loss.tsv", "stack-model.pt", "controller.pt", "controller_optimizer_state.pt", "training_state.pt",
                  "curriculum.json"):
            assert (base / f).exists(), f
        st = torch.load(str(base / "training_state.pt"), map_location="cpu", weights_only=False)
        curriculum = json.loads(open(str(base / "curriculum.json")).read())
        assert len(curriculum) == EPISODES and st["episode"] == EPISODES - 1
        assert curriculum[0] == ([1.0] * ENC if name == "sampled" else FORCED[0])
        hist = r["res"]["dev_score_history"]
        assert len(hist) == EPISODES * EPOCHS
        baseline, at = 0.0, None
        for e in range(EPISODES):
            best = max([0.0] + hist[e * EPOCHS:(e + 1) * EPOCHS])
            if e == 0 or best >= baseline:
                baseline, at = max(baseline, best) if e else best, e
        assert st["baseline_score"] == baseline and st["best_action"].tolist() == curriculum[at]
        assert sum(v["counts"] for v in st["action_dict"].values()) == EPISODES
        log = open(str(base / "training.log")).read()
        assert log.count("Start episode") == EPISODES and log.count("controller probabilities") == EPISODES
        from flair.models import EmbedController
        c = EmbedController.load(base / "controller.pt")
        assert c.num_actions == ENC and torch.equal(c.selector, r["trainer"].controller.selector)


def test_f_command_line(runs):
    root = runs["root"]
    cfg = _config(root, "cli", "ReinforcementTrainer", "gpu", max_episodes=EPISODES)
    train_py = os.path.join(os.path.dirname(HERE), "train.py")
    seen = []
    for _ in range(2):
        r = subprocess.run([sys.executable, train_py, "--config", str(cfg)], cwd=str(root), stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
        seen.append(open(str(root / "out" / "cli" / "curriculum.json")).read())
    assert seen[0] == seen[1] and len(json.loads(seen[0])) == EPISODES, "two runs of one configuration give the same curriculum"
    r = subprocess.run([sys.executable, train_py, "--config", str(cfg), "--test"], cwd=str(root), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    tsv = root / "out" / "cli" / "ColumnCorpus-TINY-test.tsv"
    assert tsv.exists() and len([l for l in open(str(tsv)).read().split("\n") if l]) > 0
