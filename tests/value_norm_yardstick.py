"""The yardstick of value normalisation (the critic trained on standardised value targets): plain numpy float64, no import of the
product.

  * the running statistic: Chan's merge of a batch (n_b, mean_b, M2_b) into {count, mean, M2} and the published four numbers
    {mu, 1/sigma, sigma, 0} with sigma = sqrt(M2 / count + 1e-5) -- population variance and epsilon of rl_games' RunningMeanStd;
  * GAE on values denormalised in float64, V = v^ sigma + mu, through the per-trajectory recurrence of
    tests/gae_bootstrap_yardstick.py (imported: the project's CPU oracle per segment);
  * the normalised value loss and its gradient with respect to the critic's output, with and without clipping."""
import math

import numpy as np

import gae_bootstrap_yardstick as GY

EPS = 1e-5


# ---------------------------------------------------------------------------------------------------------- statistic
def batch_moments(x):
    """(n_b, mean_b, M2_b) of one batch with exact summation (math.fsum) -- the truth of the kernel's shifted double sums."""
    a = np.asarray(x, np.float32).astype(np.float64).reshape(-1)
    n = a.size
    mean = math.fsum(a.tolist()) / n
    dev = a - mean
    m2 = math.fsum((dev * dev).tolist()) - math.fsum(dev.tolist()) ** 2 / n
    return float(n), mean, max(m2, 0.0)


def merge(state, batch):
    """Chan's formula: state = (count, mean, M2), batch = (n_b, mean_b, M2_b) -> the merged state."""
    count, mean, m2 = (float(v) for v in state)
    nb, mean_b, m2_b = (float(v) for v in batch)
    delta = mean_b - mean
    tot = count + nb
    return tot, mean + delta * nb / tot, m2 + m2_b + delta * delta * count * nb / tot


def update(state, x):
    """The statistic after one more batch; a batch with a non-finite entry leaves it as it is (the caller counts it)."""
    if not np.isfinite(np.asarray(x, np.float64)).all():
        return tuple(float(v) for v in state)
    return merge(state, batch_moments(x))


def scale64(state):
    """{mu, 1/sigma, sigma, 0} in float64; count == 0: {0, 1, 1, 0}."""
    count, mean, m2 = (float(v) for v in state)
    if count <= 0:
        return np.array([0.0, 1.0, 1.0, 0.0])
    sd = math.sqrt(m2 / count + EPS)
    return np.array([mean, 1.0 / sd, sd, 0.0])


def scale32(state):
    """... each entry rounded once to float32."""
    return scale64(state).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- GAE
def gae(rews, dones, trunc, vhat, boot_hat, mu, sigma, gamma, lmbda, std):
    """GAE per trajectory on V = v^ sigma + mu formed in float64 (boot values likewise; None: the plain scan).  The recurrence is
    gae_bootstrap_yardstick.per_segment's.  -> (value_targets, advantages, returns)."""
    f = lambda x: np.asarray(x, np.float32).astype(np.float64)
    v = f(vhat) * float(sigma) + float(mu)
    n = len(rews)
    boot = np.full(n, np.nan) if boot_hat is None else f(boot_hat) * float(sigma) + float(mu)
    if boot_hat is None:   # the plain scan bootstraps a truncated step from the next entry of the values
        idx = GY.boot_steps(dones, trunc)
        boot[idx] = v[idx + 1]
    return GY.per_segment(rews, dones, trunc, v, boot, gamma, lmbda, std)


def gae_value_rounding(vmax, gamma, lmbda):
    """What one float32 rounding of every V (relative 2^-24) can move an advantage or a value target by:
    delta_t = r + gamma V_{t+1} - V_t moves by at most (1 + gamma) max|V| 2^-24 and A_t = sum_k (gamma lambda)^k delta_{t+k} by at
    most that over (1 - gamma lambda); the target V_t + A_t is covered by the same bound with the relative tolerance on V_t."""
    return (1.0 + gamma) / (1.0 - gamma * lmbda) * float(vmax) * 2.0 ** -24


# --------------------------------------------------------------------------------------------------------- value loss
def normalise_targets32(t, mu, inv_sd):
    """t^ as the kernel forms it: a float32 subtraction, then a float32 multiplication."""
    t, mu, inv_sd = np.asarray(t, np.float32), np.float32(mu), np.float32(inv_sd)
    return ((t - mu).astype(np.float32) * inv_sd).astype(np.float32)


def value_loss64(vhat, t, adv, mu, inv_sd, vclip=0.0, mb_ratio=1.0):
    """float64: loss = mean((v_pred - t^)^2) and mb_ratio d loss / d v^ per row, with t^ = (t - mu) inv_sd and, vclip > 0,
    v_pred = v^_old + clamp(v^ - v^_old, -c, c) around v^_old = (fl32(t - A) - mu) inv_sd (gradient where |v^ - v^_old| <= c)."""
    v = np.asarray(vhat, np.float64)
    t32, a32 = np.asarray(t, np.float32), np.asarray(adv, np.float32)
    mu, inv_sd = float(mu), float(inv_sd)
    tn = (t32.astype(np.float64) - mu) * inv_sd
    n = v.size
    if vclip > 0:
        v_old = ((t32 - a32).astype(np.float32).astype(np.float64) - mu) * inv_sd
        dv = v - v_old
        d = v_old + np.clip(dv, -vclip, vclip) - tn
        g = mb_ratio * 2.0 * d / n * (np.abs(dv) <= vclip)
    else:
        d = v - tn
        g = mb_ratio * 2.0 * d / n
    return float((d * d).mean()), g
