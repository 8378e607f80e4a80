"""EmbedController: the ACE controller, one logit per embedding of the stacked tagger (BASELINE config 5).

Behavioural reference (restated): flair/models/controller.py -- `selector`, a float32 [num_actions] parameter of zeros (:47-51);
`get_value` / `forward` = sigmoid of it (:103-114); `sample` = one Bernoulli(sigmoid(selector)) draw per embedding, repeated
while nothing is selected or the draw equals the previous one (:85-102); controller.pt = {state_dict, num_actions,
model_structure, state_size} (:67-84).

The controller lives on the HOST: it is `num_actions` numbers (9 in the shipped YAML) updated once per episode by torch.optim,
and nothing of it is ever read by a kernel -- the tagger takes the sampled 0/1 action as `selection`.

Two deviations from the reference, both so that one configuration gives one curriculum:
  * the draws come from a torch.Generator the controller owns, seeded with SEED (the reference draws from the global generator);
  * controller.pt also carries that generator's state, `previous_selection` and `best_action`, which `continue_training` needs to
    go on where the search stopped (the reference's four keys are all there, with the reference's types).
A `model_structure` (the sentence-level controller of :52-62, a Linear over sentence states) is refused by name."""
import torch
from torch.nn.parameter import Parameter

import flair.nn

SEED = 20220711     # the stack trainer's shuffle seed (ModelFinetuner._train_stack)


class EmbedController(flair.nn.Model):
    def __init__(self, num_actions, model_structure=None, state_size=20, hidden_size=100):
        super().__init__()
        if model_structure is not None:
            raise NotImplementedError("Controller.model_structure=%r selects the sentence-level controller (one action per sentence "
                                      "from a Linear over sentence states); only the embedding-level controller "
                                      "(model_structure: null) is implemented" % (model_structure,))
        self.previous_selection = None
        self.best_action = None
        self.num_actions = int(num_actions)
        self.model_structure = model_structure
        self.state_size = state_size
        self.selector = Parameter(torch.zeros(self.num_actions), requires_grad=True)     # host memory, whatever flair.device is
        self.generator = torch.Generator().manual_seed(SEED)

    @classmethod
    def _init_model_with_state_dict(cls, state):
        model = cls(num_actions=state["num_actions"], model_structure=state["model_structure"], state_size=state["state_size"])
        model.load_state_dict(state["state_dict"])
        if state.get("generator_state") is not None:
            model.generator.set_state(state["generator_state"])
        for k in ("previous_selection", "best_action"):
            v = state.get(k)
            setattr(model, k, None if v is None else torch.as_tensor(v, dtype=torch.float32).clone())
        return model

    def _get_state_dict(self):
        return {"state_dict": self.state_dict(), "num_actions": self.num_actions, "model_structure": self.model_structure,
                "state_size": self.state_size, "generator_state": self.generator.get_state(),
                "previous_selection": None if self.previous_selection is None else self.previous_selection.clone(),
                "best_action": None if self.best_action is None else torch.as_tensor(self.best_action, dtype=torch.float32).clone()}

    def get_value(self, states=None, mask=None):
        return self.selector

    def forward(self, states=None, mask=None):
        return torch.sigmoid(self.get_value(states, mask))

    @staticmethod
    def log_prob(value, selection):
        """log Bernoulli(selection; sigmoid(value)) per position, from the logits as torch.distributions.Bernoulli.log_prob
        computes it: finite also where sigmoid(value) rounds to 0 or 1"""
        return -torch.nn.functional.binary_cross_entropy_with_logits(value, selection, reduction="none")

    def sample(self, states=None, mask=None):
        """-> (selection f32 [num_actions] of 0/1, log_prob [num_actions] with the selector's graph)"""
        value = self.get_value(states, mask)
        p = torch.sigmoid(value).detach()
        selection = torch.bernoulli(p, generator=self.generator)
        # never nothing, and never the previous episode's action again
        while selection.sum() == 0 or (self.previous_selection is not None and bool((self.previous_selection == selection).all())):
            selection = torch.bernoulli(p, generator=self.generator)
        self.previous_selection = selection.clone()
        return selection, self.log_prob(value, selection)
