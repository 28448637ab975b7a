"""The yardstick of the bootstrap form of the GAE scan: the project's CPU oracle (oracle.gae.gae, mode "f64"), unmodified, applied
per trajectory.  The concatenated arrays are cut after every step with done or truncated, and each segment is run with
values = V[segment] ++ [b]: b is the segment's bootstrap value when its last step is truncated and not done, V[next] for the open
tail of the data, and V[next] (irrelevant: nd = 0) when the last step is done.  Same recurrence as the whole-array oracle, so the
tolerance of test_gae_matches_oracle holds: rtol 2e-6, atol 2e-6 (tests/test_gae_bootstrap_host.py checks that this construction
reproduces the whole-array oracle when b = V[next] everywhere)."""
import numpy as np

from oracle import gae as ogae

RTOL = ATOL = 2e-6


def per_segment(rews, dones, trunc, values, boot, gamma, lmbda, std):
    """-> (value_targets f32[n], advantages f32[n], returns f64[n]).  `boot` is read at truncated-and-not-done steps only."""
    rews, dones, trunc, values = (np.asarray(x, np.float32) for x in (rews, dones, trunc, values))
    n = len(rews)
    stops = list(np.flatnonzero((dones != 0) | (trunc != 0)) + 1)
    if not stops or stops[-1] != n:
        stops.append(n)
    vt, adv, ret = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
    start = 0
    for stop in stops:
        last = stop - 1
        b = boot[last] if (trunc[last] != 0 and dones[last] == 0) else values[stop]
        v = np.concatenate([values[start:stop], np.asarray([b], np.float32)])
        vt[start:stop], adv[start:stop], ret[start:stop] = ogae.gae(rews[start:stop], dones[start:stop], trunc[start:stop], v,
                                                                    gamma, lmbda, std, "f64")
        start = stop
    return vt, adv, ret


def boot_steps(dones, trunc):
    return np.flatnonzero((np.asarray(trunc) != 0) & (np.asarray(dones) == 0))


def make_case(n, seed, p_done=0.01, p_trunc=0.02):
    """Random rewards / values, mixed done and truncated ends (independent draws: some steps carry both flags, and one is forced
    to), forced truncated-not-done ends on both sides of the first chunk edge, inside the next chunk's look-ahead window and at
    the last step.  boot: a value at every truncated-and-not-done step, NaN at every other entry."""
    rs = np.random.RandomState(seed)
    rews = rs.randn(n).astype(np.float32)
    values = rs.randn(n + 1).astype(np.float32)
    dones = (rs.rand(n) < p_done).astype(np.float32)
    trunc = (rs.rand(n) < p_trunc).astype(np.float32)
    if n > 2:
        dones[n // 2] = trunc[n // 2] = 1.0               # both flags: done wins
    for t in (2047, 2048, 2048 + 100, n - 1):
        if 0 <= t < n:
            dones[t], trunc[t] = 0.0, 1.0
    boot = np.full(n, np.nan, np.float32)
    idx = boot_steps(dones, trunc)
    boot[idx] = rs.randn(idx.size).astype(np.float32)
    return rews, dones, trunc, values, boot


def assert_close(got, want, what=""):
    for k, name in enumerate(("value_targets", "advantages", "returns")):
        g = np.asarray(got[k])
        assert np.isfinite(g).all(), f"{what}: {name} not finite"
        np.testing.assert_allclose(g, np.asarray(want[k], np.float32), rtol=RTOL, atol=ATOL, err_msg=f"{what}: {name}")
