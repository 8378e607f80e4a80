"""ReinforcementTrainer for BASELINE config 5 (ACE: automated concatenation of embeddings): the controller's search over
embedding subsets, every episode one training run of the stacked tagger's BiLSTM-CRF head on frozen features.

Behavioural reference (restated): flair/trainers/reinforcement_trainer.py -- constructor keywords (:61-84) and what it does to
the model (:97-101: `use_rl`, `embedding_selector`, the EmbedController over len(embeddings) actions), train() keywords
(:273-322) and the episode loop (:521-1075):

    start of an episode   a fresh tagger optimizer and scheduler (:521-575); action, log_prob = controller.sample(); episode 1
                          trains with every embedding on (:595-598); the action is appended to the curriculum or replaced by the
                          curriculum file's (:600-603); model.selection = action (:607)
    every epoch           train, evaluate on dev; a score >= the overall `baseline_score` saves the tagger and the controller and
                          raises the baseline (:921-932)
    end of an episode     reward per position from every action tried so far (:998-1018, `ace_reward` below), controller_loss =
                          -sum(log_prob * reward), one controller_optimizer step (:1018-1032); best_action follows the baseline
                          (:976-982, :1040-1045); action_dict, training_state.pt, controller_optimizer_state.pt (:1059-1075)
    after the search      action_dict averages, curriculum.json, model.selection = best_action, final_test (:1090-1122)

What runs on the device is ModelFinetuner's stacked-tagger epoch (finetune_trainer._StackRun, the one copy both trainers share):
the head's optimizer step over stored rows and the dev decode, all HIP.  The controller is len(embeddings) numbers updated once per
episode: it stays on the host (torch.optim on a CPU parameter) and this module launches nothing of its own.  With
embeddings_storage_mode "gpu" / "cpu" the feature store is filled ONCE, with every embedding on, before the first episode
(FastSequenceTagger.fill_feature_store; the reference's gpu_friendly_assign_embedding, :512-517); every episode's selection is then
the store's block_on switch and no feature producer runs again for the whole search.  With "none" every batch is computed under the
episode's selection and deselected embeddings are not launched.

Deviations from the reference, recorded in DESIGN.md: the controller samples from its own seeded generator (one configuration, one
curriculum); `continue_training` resumes at the saved episode + 1 (the reference re-runs the saved index) and controller.pt /
curriculum.json are also written at every episode's end so that the resumed search goes on exactly; the tagger's file is
stack-model.pt (the head's weights; the reference pickles the whole model into best-model.pt).

Refused by name: what _train_stack refuses, `use_rnn: false`, `Controller.model_structure` (the sentence-level controller),
`monitor_train`, and an embedding list with a placeholder (ELMo / fastText, whose weights are not available offline): episode 1
selects every embedding.  `one_by_one` and `select_model_by_macro` are accepted and unused, as in the reference's loop.

Note: the shipped ACE YAML passes `assign_doc_for_ext_context` and string optimiser names to this constructor, which the
reference's own signature does not accept (its **kwargs is commented out, :83) -- the mirror accepts them."""
import json
import logging
import math
from pathlib import Path

import torch

from flair.training_utils import log_line
from .finetune_trainer import ModelFinetuner, _StackRun, _warn_unknown

log = logging.getLogger("flair")


def ace_reward(action, best_score, action_dict, baseline_score=0.0, discount=0.5, log_reward=False, sqrt_reward=False,
               old_reward=False):
    """The reward at each position for an episode that trained `action` to `best_score` (reinforcement_trainer.py:991-1010):
    for every action a_p tried before, r = best_score - max(scores[a_p]) (optionally sign(r) log(|r| + 1) / sign(r) sqrt(|r|)),
    discounted by discount ** (hamming(action, a_p) - 1), credited to the positions where the two actions differ.
    old_reward: best_score - baseline_score at every position.  -> f32 [num_actions]"""
    action = torch.as_tensor(action, dtype=torch.float32)
    R = torch.zeros_like(action)
    if old_reward:
        return R + float(best_score - baseline_score)
    for prev, entry in action_dict.items():
        r = float(best_score) - float(max(entry["scores"]))
        if log_reward:
            r = math.copysign(math.log(abs(r) + 1.0), r)
        if sqrt_reward:
            r = math.copysign(math.sqrt(abs(r)), r)
        change = torch.abs(action - torch.tensor(prev, dtype=torch.float32))
        r = r * float(discount) ** (float(change.sum()) - 1.0)
        R += r * change
    return R


def controller_step(controller_optimizer, log_prob, reward):
    """controller_loss = -sum_k log_prob_k * reward_k, backward, one optimizer step (:1018-1032) -> the loss"""
    controller_loss = -(log_prob * reward).sum()
    controller_loss.backward()
    controller_optimizer.step()
    return controller_loss.detach()


class ReinforcementTrainer(ModelFinetuner):
    def __init__(self, model, teachers, corpus, optimizer=None, controller_optimizer=None, controller_learning_rate: float = 0.1,
                 epoch: int = 0, distill_mode=False, optimizer_state: dict = None, scheduler_state: dict = None,
                 use_tensorboard: bool = False, language_resample=False, config=None, is_test: bool = False,
                 direct_upsample_rate: int = -1, down_sample_amount: int = -1, sentence_level_batch: bool = False,
                 dev_sample: bool = False, assign_doc_id: bool = False, train_with_doc: bool = False,
                 pretrained_file_dict: dict = None, sentence_level_pretrained_data: bool = False,
                 assign_doc_for_ext_context: bool = False, **kwargs):
        _warn_unknown("ReinforcementTrainer", kwargs)
        super().__init__(model, teachers, corpus, optimizer=optimizer, epoch=epoch, optimizer_state=optimizer_state,
                         scheduler_state=scheduler_state, use_tensorboard=use_tensorboard, distill_mode=distill_mode, config=config,
                         is_test=is_test, language_resample=language_resample, direct_upsample_rate=direct_upsample_rate,
                         down_sample_amount=down_sample_amount, sentence_level_batch=sentence_level_batch,
                         assign_doc_id=assign_doc_id, train_with_doc=train_with_doc, pretrained_file_dict=pretrained_file_dict,
                         sentence_level_pretrained_data=sentence_level_pretrained_data,
                         assign_doc_for_ext_context=assign_doc_for_ext_context)
        self.controller_learning_rate = controller_learning_rate
        self.controller_optimizer = controller_optimizer if controller_optimizer is not None else "SGD"
        # reinforcement_trainer.py:97-101: the tagger multiplies every embedding's features by `selection[idx]` in forward()
        self.model.use_rl = True
        self.model.embedding_selector = True
        n = len(self.model.embeddings.embeddings) if hasattr(self.model.embeddings, "embeddings") else 1
        if getattr(self.model, "selection", None) is None:
            self.model.selection = [1] * n   # all embeddings on until a search (train) or train.py (best_action) sets it
        # the controller over the embeddings (:101); a Controller block that selects the sentence-level one is refused by train()
        from flair.models.controller import EmbedController
        ccfg = config.get("Controller", None) if config is not None else None
        self.controller_config = dict(ccfg) if ccfg else {}
        self.controller = None
        if self.controller_config.get("model_structure") is None:
            self.controller = EmbedController(num_actions=n, **self.controller_config)
        self.best_action = None
        self.action_dict = {}

    def _ace_refusals(self, a, kwargs):
        """what the search does not do, by name, before any work (after everything the stacked tagger's loop refuses)"""
        self._stack_refusals(a, kwargs)
        if not getattr(self.model, "use_rnn", False):
            raise NotImplementedError("use_rnn: false: ReinforcementTrainer searches over the frozen embeddings of the stacked tagger "
                                      "(use_rnn: true); a fine-tuned encoder has no embedding list to select from")
        if self.controller is None:
            raise NotImplementedError("Controller.model_structure=%r selects the sentence-level controller (assign_embedding_masks, "
                                      "use_embedding_masks); only the embedding-level controller is implemented"
                                      % (self.controller_config.get("model_structure"),))
        if a["monitor_train"]:
            raise NotImplementedError("monitor_train is not supported by ReinforcementTrainer (the reference asserts on it)")
        from flair.embeddings import _NeedsExternalWeights
        held = [e.name for e in self.model.embeddings.embeddings if isinstance(e, _NeedsExternalWeights)]
        if held:
            raise NotImplementedError("ACE controller training with the placeholder embedding(s) %s is out of scope: their weights are "
                                      "not available offline and episode 1 selects every embedding -- drop them from the YAML's "
                                      "`embeddings:` block (they still work deselected for --test / --parse)" % ", ".join(held))
        if not 0.0 < float(a["discount"]) <= 1.0:
            raise ValueError("discount must lie in (0, 1] (got %r): the reward is scaled by discount ** (hamming distance - 1)"
                             % (a["discount"],))

    def _open_stack_run(self, base_path, a):
        return _StackRun(self, base_path, a)

    def train(self, base_path, learning_rate: float = 5e-5, mini_batch_size: int = 32, eval_mini_batch_size: int = None,
              max_epochs: int = 100, max_episodes: int = 10, anneal_factor: float = 0.5, patience: int = 10,
              min_learning_rate: float = 5e-9, train_with_dev: bool = False, macro_avg: bool = True, monitor_train: bool = False,
              monitor_test: bool = False, embeddings_storage_mode: str = "cpu", checkpoint: bool = False,
              save_final_model: bool = True, anneal_with_restarts: bool = False, shuffle: bool = True,
              true_reshuffle: bool = False, param_selection_mode: bool = False, num_workers: int = 4, sampler=None,
              use_amp: bool = False, amp_opt_level: str = "O1", max_epochs_without_improvement=30, warmup_steps: int = 0,
              use_warmup: bool = True, gradient_accumulation_steps: int = 1, lr_rate: int = 1, decay: float = 0.75,
              decay_steps: int = 5000, sort_data: bool = True, fine_tune_mode: bool = False, debug: bool = False,
              min_freq: int = -1, min_lemma_freq: int = -1, min_pos_freq: int = -1, rootschedule: bool = False,
              freezing: bool = False, log_reward: bool = False, sqrt_reward: bool = False, controller_momentum: float = 0.0,
              discount: float = 0.5, curriculum_file=None, random_search=False, continue_training=False, old_reward=False,
              one_by_one: bool = False, select_model_by_macro: bool = False, **kwargs):
        """Keywords are the reference's (:273-322).  -> {"test_score", "dev_score_history", "test_score_history",
        "train_loss_history", "dev_loss_history", "test_loss_history"} (:1115-1122)"""
        a = dict(locals())
        for k in ("self", "kwargs", "base_path"):
            a.pop(k)
        a["warmup_epochs"] = 1                  # use_warmup: one epoch of warm-up (:568-569), read with fine_tune_mode only
        a["select_model_by_macro"] = False      # accepted, unused: the reference's loop never reads it (nor one_by_one)
        base_path = Path(base_path)
        self._ace_refusals(a, kwargs)
        controller = self.controller
        controller_optimizer = getattr(torch.optim, str(self.controller_optimizer))(
            controller.parameters(), lr=self.controller_learning_rate, momentum=controller_momentum)    # host tensors only (:429-431)
        min_lr = float(learning_rate) / 1000.0  # (:504) whatever min_learning_rate says: an episode ends after three annealings
        names = sorted(e.name for e in self.model.embeddings.embeddings)
        run = self._open_stack_run(base_path, a)
        try:
            start_episode, baseline_score, curriculum = 0, 0, []
            self.action_dict = {}
            if continue_training:               # (:433-444)
                if (base_path / "stack-model.pt").exists():
                    self.model.load_stack_state(torch.load(str(base_path / "stack-model.pt"), map_location="cpu", weights_only=False))
                controller = self.controller = type(controller).load(base_path / "controller.pt")
                controller_optimizer = getattr(torch.optim, str(self.controller_optimizer))(
                    controller.parameters(), lr=self.controller_learning_rate, momentum=controller_momentum)
                if (base_path / "controller_optimizer_state.pt").exists():
                    controller_optimizer.load_state_dict(torch.load(str(base_path / "controller_optimizer_state.pt"),
                                                                    map_location="cpu", weights_only=False))
                state = torch.load(str(base_path / "training_state.pt"), map_location="cpu", weights_only=False)
                start_episode = int(state["episode"]) + 1        # the saved episode is complete: go on with the next one
                self.best_action = controller.best_action = state["best_action"]
                self.action_dict = state["action_dict"]
                baseline_score = state["baseline_score"]
                if curriculum_file is None and (base_path / "curriculum.json").exists():
                    with open(base_path / "curriculum.json") as f:
                        curriculum = json.loads(f.read())[:start_episode]
                log.info("continue_training: episode %d on, baseline score %s, %d actions tried", start_episode + 1, baseline_score,
                         len(self.action_dict))
            if curriculum_file is not None:
                with open(curriculum_file) as f:
                    curriculum = json.loads(f.read())
            # every embedding of every training and dev sentence, once, before the first episode (:512-517)
            run.prefill()
            try:
                for episode in range(start_episode, int(max_episodes)):
                    best_score = 0
                    run.new_optimizer()         # moments and step count cleared, default learning rate, no bad epochs (:521-560)
                    log.info("================================== Start episode %d ==================================", episode + 1)
                    action, log_prob = controller.sample()
                    if episode == 0 and not random_search:        # (:595-598)
                        log_prob = torch.log(torch.sigmoid(controller.get_value()))
                        action = torch.ones_like(action)
                        controller.previous_selection = action
                    if curriculum_file is None:
                        curriculum.append(action.tolist())
                    else:
                        action = torch.tensor(curriculum[episode], dtype=action.dtype)
                    self.model.selection = action
                    for epoch in range(self.epoch, int(max_epochs) + self.epoch):
                        score = run.epoch(epoch)
                        run.track(score)
                        if score > best_score:
                            best_score = score
                        if score >= baseline_score:               # (:921-932)
                            log.info("==================Saving the current overall best model: %s==================", score)
                            run.save_model(base_path / "stack-model.pt")
                            controller.save(base_path / "controller.pt")
                            baseline_score = score
                        if run.anneal(min_lr):
                            break
                    log.info("================================== End episode %d ==================================", episode + 1)
                    controller_optimizer.zero_grad()
                    controller.zero_grad()
                    reward = torch.zeros_like(action)
                    if episode == 0:                              # (:976-982)
                        baseline_score = best_score
                        self.best_action = controller.best_action = action
                    else:                                         # (:983-1045)
                        reward = ace_reward(action, best_score, self.action_dict, baseline_score=baseline_score, discount=discount,
                                            log_reward=log_reward, sqrt_reward=sqrt_reward, old_reward=old_reward)
                        if random_search:
                            log.info("================= Doing random search, stop updating the controller =================")
                        else:
                            controller_step(controller_optimizer, log_prob, reward)
                        if best_score >= baseline_score:
                            baseline_score = best_score
                            self.best_action = controller.best_action = action
                    log.info("episode %d: action %s - best score %s - reward at each position %s - controller probabilities %s",
                             episode + 1, ", ".join("%s=%d" % (n, int(x)) for n, x in zip(names, action.tolist())), best_score,
                             [round(float(x), 6) for x in reward], [round(float(x), 6) for x in controller().detach()])
                    log.info("overall best action %s - overall best score %s",
                             None if self.best_action is None else [int(x) for x in self.best_action], baseline_score)
                    run.log_store()
                    key = tuple(action.tolist())                  # (:1059-1066)
                    entry = self.action_dict.setdefault(key, {"counts": 0, "scores": []})
                    entry["counts"] += 1
                    entry["scores"].append(best_score)
                    torch.save({"episode": episode, "best_action": self.best_action, "baseline_score": baseline_score,
                                "action_dict": self.action_dict}, str(base_path / "training_state.pt"))     # (:1068-1075)
                    torch.save(controller_optimizer.state_dict(), str(base_path / "controller_optimizer_state.pt"))
                    # (not in the reference) what continue_training goes on from: the updated controller with its generator, and
                    # the actions so far
                    controller.save(base_path / "controller.pt")
                    with open(base_path / "curriculum.json", "w") as f:
                        f.write(json.dumps(curriculum))
            except KeyboardInterrupt:
                log_line(log)
                log.info("Exiting from training early.")
            # (:1090-1099)
            for entry in self.action_dict.values():
                entry["average"] = sum(entry["scores"]) / entry["counts"]
            log.info("Final State dictionary: %s", self.action_dict)
            with open(base_path / "curriculum.json", "w") as f:
                f.write(json.dumps(curriculum))
            if self.best_action is not None:
                self.model.selection = self.best_action
            if (base_path / "stack-model.pt").exists():   # final_test reads best_action's head (its own loading is ModelFinetuner's)
                self.model.load_stack_state(torch.load(str(base_path / "stack-model.pt"), map_location="cpu", weights_only=False))
                log.info("Testing using stack-model.pt with the best action ...")
            final_score = 0.0
            if self.corpus.test is not None and len(self.corpus.test) > 0:
                final_score = self.final_test(base_path, run.eval_bs, quiet_mode=False)
            else:
                log.info("Test data not provided setting final score to 0")
        finally:
            run.close()
        return {"test_score": final_score, "dev_score_history": run.dev_score_history, "test_score_history": [],
                "train_loss_history": run.train_loss_history, "dev_loss_history": run.dev_loss_history, "test_loss_history": []}
