"""Float64 restatement of the ACE controller's arithmetic, written from the formulas (not from the trainer's code): the reward at
each position of an episode and one optimizer step of the selector.

    R_k     = sum over every action a_p tried before of  f(best_score - max(scores[a_p])) * discount ** (ham(a, a_p) - 1) * |a_k - a_p,k|
              f = identity, sign(r) log(|r| + 1) (log_reward) or sign(r) sqrt(|r|) (sqrt_reward; after the log when both are set)
              old_reward: R_k = best_score - baseline_score for every k
    loss    = - sum_k log Bernoulli(a_k; sigmoid(s_k)) * R_k
    dloss/ds_k = - R_k * (a_k - sigmoid(s_k))
    SGD with momentum mu (torch.optim.SGD, dampening 0): buf = g on the first step, mu * buf + g later; s -= lr * buf"""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def log_prob(selector, action):
    p, a = sigmoid(selector), np.asarray(action, np.float64)
    return a * np.log(p) + (1.0 - a) * np.log1p(-p)


def reward(action, best_score, action_dict, baseline_score=0.0, discount=0.5, log_reward=False, sqrt_reward=False, old_reward=False):
    a = np.asarray(action, np.float64)
    if old_reward:
        return np.full(a.shape, float(best_score) - float(baseline_score))
    R = np.zeros(a.shape, np.float64)
    for prev, entry in action_dict.items():
        r = float(best_score) - max(float(x) for x in entry["scores"])
        if log_reward:
            r = np.sign(r) * np.log(abs(r) + 1.0)
        if sqrt_reward:
            r = np.sign(r) * np.sqrt(abs(r))
        change = np.abs(a - np.asarray(prev, np.float64))
        R += r * discount ** (change.sum() - 1.0) * change
    return R


def sgd_step(selector, action, R, lr, momentum=0.0, buf=None):
    """-> (the selector after one step, the momentum buffer)"""
    s = np.asarray(selector, np.float64)
    g = -np.asarray(R, np.float64) * (np.asarray(action, np.float64) - sigmoid(s))
    buf = g if buf is None else momentum * np.asarray(buf, np.float64) + g
    return s - lr * buf, buf
