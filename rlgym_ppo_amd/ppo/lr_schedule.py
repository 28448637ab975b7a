"""Learning-rate schedules of PPOLearner / Learner (host side).

  "constant"  the rate the learner was built with (the reference's behaviour; `Learner.update_learning_rate` changes it by hand);
  "adaptive"  rsl_rl's / rl_games' KL-adaptive rule, once per optimiser step, decided and applied on the device
              (rlppo_kl_gate_lr -> rlppo_clip_adam_pack2_lr): `adapt_lr` below is its float64 restatement, the yardstick of the tests;
  "linear"    CleanRL's anneal_lr / SB3's linear_schedule over the run's timestep budget: `linear_lr`, set by `Learner` before every
              learn() -- a bare PPOLearner has no horizon and refuses it.

Nothing here needs the GPU."""
import math

SCHEDULES = ("constant", "adaptive", "linear")
ADAPT_FACTOR = 1.5   # rsl_rl's and rl_games' factor, both directions


def check_schedule(lr_schedule, desired_kl, lr_bounds, policy_lr=None, critic_lr=None, allow_linear=True):
    """Validates the three options (and, under "adaptive", the initial rates against the bounds); returns them normalised as
    (lr_schedule, float(desired_kl), (float(lr_min), float(lr_max)))."""
    if lr_schedule not in SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {SCHEDULES}, got {lr_schedule!r}")
    if lr_schedule == "linear" and not allow_linear:
        raise ValueError("lr_schedule='linear' anneals over a run's timestep budget, which a bare PPOLearner does not have: it is an option "
                         "of Learner (ppo_lr_schedule='linear', over timestep_limit); lr_schedule.linear_lr is the formula")
    try:
        d = float(desired_kl)
    except (TypeError, ValueError):
        raise ValueError(f"desired_kl must be a finite number > 0, got {desired_kl!r}") from None
    if not (math.isfinite(d) and d > 0):
        raise ValueError(f"desired_kl must be a finite number > 0, got {desired_kl!r}")
    try:
        lo, hi = (float(x) for x in lr_bounds)
    except (TypeError, ValueError):
        raise ValueError(f"lr_bounds must be a pair (lr_min, lr_max), got {lr_bounds!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi):
        raise ValueError(f"lr_bounds must satisfy 0 < lr_min <= lr_max (finite), got {lr_bounds!r}")
    if lr_schedule == "adaptive":
        check_rates_in_bounds((lo, hi), policy_lr=policy_lr, critic_lr=critic_lr)
    return lr_schedule, d, (lo, hi)


def check_rates_in_bounds(lr_bounds, **rates):
    """The adaptive rule moves a rate inside [lr_min, lr_max]; one that starts outside is a configuration error."""
    lo, hi = lr_bounds
    for name, lr in rates.items():
        if lr is None:
            continue
        if not (math.isfinite(float(lr)) and lo <= float(lr) <= hi):
            raise ValueError(f"lr_schedule='adaptive': {name}={lr!r} lies outside lr_bounds=({lo!r}, {hi!r})")


def linear_lr(lr0, T, limit):
    """CleanRL's anneal_lr: lr0 * max(0, 1 - T / limit), T the cumulative timesteps before the iteration."""
    return float(lr0) * max(0.0, 1.0 - float(T) / float(limit))


def adapt_lr(lr, kl, desired_kl, lo, hi, factor=ADAPT_FACTOR):
    """The device rule of rlppo_kl_gate_lr in Python floats (IEEE doubles, the same operations in the same order): strict
    inequalities, so a KL exactly on a threshold, a KL of 0 and a NaN KL leave the rate alone."""
    lr, kl, desired_kl, lo, hi, factor = (float(x) for x in (lr, kl, desired_kl, lo, hi, factor))
    if kl > 2.0 * desired_kl:
        v = lr / factor
        return lo if v < lo else v
    if kl > 0.0 and kl < desired_kl / 2.0:
        v = lr * factor
        return hi if v > hi else v
    return lr
