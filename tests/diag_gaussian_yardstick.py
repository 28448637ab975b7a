"""What belongs to the diagonal-Gaussian head with a learnable log_std alone (include/rlppo.h, "[diag]"): Normal(mean, exp(log_std))
in closed form -- log p, and the entropy = sum over the action dimensions of Normal.entropy(), no division by k -- checked against
torch.distributions, a float64 sampler, the batch's advantage statistics, and the CPU-side assertions that keep a test's inputs clear
of discrete decisions: no ratio near a clip edge, no hidden pre-activation within its float32 rounding bound of 0.  The PPO
minibatch, learn() and the tolerance rule built on these are tests/ppo_yardstick.py."""
import math

import numpy as np
import torch

from oracle import nets, ppo

U32 = 2.0 ** -24
ENT_C = 0.5 + 0.5 * math.log(2 * math.pi)   # 1.4189385332046727
HALF_LOG_2PI = math.log(math.sqrt(2 * math.pi))


def _t(x, dtype):
    return x.detach().to(dtype).clone() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x), dtype=dtype).clone()


def logp_terms(acts, mean, log_std):
    """Normal.log_prob's three terms in its order, closed form."""
    var = torch.exp(log_std) ** 2
    return -((acts - mean) ** 2) / (2 * var) - log_std - HALF_LOG_2PI


def row_entropy(log_std):
    return (ENT_C + log_std).sum()


def check_closed_form(mean, log_std, acts):
    """float64: the closed forms above equal torch.distributions.Normal's to 1e-12."""
    mean, log_std, acts = _t(mean, torch.float64), _t(log_std, torch.float64), _t(acts, torch.float64)
    dist = torch.distributions.Normal(mean, torch.exp(log_std).expand_as(mean))
    e_lp = (logp_terms(acts, mean, log_std) - dist.log_prob(acts)).abs().max().item()
    e_ent = (row_entropy(log_std) - dist.entropy().sum(-1)).abs().max().item()
    assert e_lp <= 1e-12 and e_ent <= 1e-12, (e_lp, e_ent)
    return e_lp, e_ent


def sample64(pol, log_std, obs, eps):
    """float64: (mean, actions = mean + exp(log_std) eps, log p of those actions)."""
    p64 = [(_t(w, torch.float64), _t(b, torch.float64)) for w, b in pol]
    mean = nets.mlp(p64, _t(obs, torch.float64))
    ls = _t(log_std, torch.float64)
    act = mean + torch.exp(ls) * _t(eps, torch.float64)
    return mean.numpy(), act.numpy(), logp_terms(act, mean, ls).sum(-1).numpy()


def adv_stats(adv):
    """(mean, 1 / (std + 1e-8)) of a batch's advantages, unbiased std: rlppo_adv_stats."""
    a = np.asarray(adv, np.float64)
    return float(a.mean()), float(1.0 / (a.std(ddof=1) + 1e-8))


def assert_clear_of_clip_edges(ratio, clip, margin=1e-4):
    """No ratio of the float64 run within `margin` of a clip edge (float32 carries ~1e-6 of rounding in a ratio), and rows on both
    sides of both edges."""
    r = np.asarray(ratio, np.float64)
    d = np.minimum(np.abs(r - (1.0 - clip)), np.abs(r - (1.0 + clip)))
    assert d.min() > margin, ("a ratio sits near a clip edge: regenerate the seed", float(d.min()))


def assert_relu_clear(params, obs, who=""):
    """No hidden pre-activation of the float64 forward within its float32 rounding bound of 0 (the bound of tests/fp64_gate.py,
    with its factor 2 of slack): B_l = (K_l + 2) u (sum_k |h_k w_jk| + |b_j|) + |W_l| B_(l-1).  A seed that trips it is replaced."""
    p64 = [(np.asarray(w, np.float64), np.asarray(b, np.float64)) for w, b in params]
    det = {}
    ppo._fwd64(p64, np.asarray(obs, np.float64), detail=det)
    prev = None
    for l, (pre, scale) in enumerate(zip(det.get("pre", []), det.get("scale", []))):
        w = np.abs(p64[l][0])
        bound = (w.shape[1] + 2) * U32 * scale
        if prev is not None:
            bound = bound + prev @ w.T
        prev = bound
        worst = float((np.abs(pre) / bound).min())
        assert worst > 2.0, (who, "a hidden pre-activation sits within float32 rounding of 0: regenerate the seed", l, worst)
