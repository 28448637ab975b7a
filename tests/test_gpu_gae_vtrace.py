"""rlppo_gae_vtrace -- the V-trace scan -- against a plain float64 backward loop, per element, and Learner(gae_vtrace=True) end to end.

The allowance is a running bound carried backwards along the recurrence (`truth`): what the device does differently from float64 is
(1) the ratio: a float32 subtraction (<= 2^-24 |x| on the exponent) and expf (<= 1 ulp, the HIP math API's documented bound);
(2) with a value scale, one float32 fma per value (<= ulp/2); (3) float64 roundings in ANOTHER association order -- the affine maps
are composed over lanes, waves, workgroups -- bounded by DEPTH u64 S_t, S_t = |delta_t| + a_t S_{t+1} the recurrence on magnitudes
and DEPTH the longest chain of compositions (8 + 6 + 2 + the chunks + 8, rounded up); (4) one rounding to float32 at the store.
Against rlppo_gae_boot (equal log-probabilities, both clips 1): the per-step coefficients are the same numbers, the carries are
composed in another order, so the outputs agree within the allowance (each side's own) and NOT bit for bit.
Achieved (printed per test): the worst element uses 0.91 of its allowance (short trajectories under a value scale), 0.87 in the Learner's buffer, 0.55 elsewhere."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from hip_pass import L, P, check, dev, stream  # noqa: E402,F401

GAMMA, LMBDA = 0.99, 0.95
U32, U64, EXPF_ULPS = 2.0 ** -24, 2.0 ** -53, 1
SCALE = np.array([0.3, 1 / 1.7, 1.7, 0.0], np.float32)   # {mu, 1/sigma, sigma, 0}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def truth(rews, dones, trunc, values, boot, lpn, lpo, rho_bar, c_bar, scale=None, gamma=GAMMA, lmbda=LMBDA, g=2048):
    """-> (advantages, value_targets, their allowances), float64."""
    r, d, tr, v, ln, lo = (np.asarray(x, np.float64) for x in (rews, dones, trunc, values, lpn, lpo))
    n, depth = len(r), 64 + len(r) // g
    mu, sd = (0.0, 1.0) if scale is None else (float(scale[0]), float(scale[2]))
    V, B = v * sd + mu, None if boot is None else np.asarray(boot, np.float64) * sd + mu
    eV, eB = (np.zeros(n + 1), np.zeros(n)) if scale is None else (0.5 * ulp32(V), 0.5 * ulp32(np.nan_to_num(B)) if boot is not None else None)
    adv, tol, A, bound, S = np.zeros(n), np.zeros(n), 0.0, 0.0, 0.0
    for t in range(n - 1, -1, -1):
        nd, m = 1.0 - d[t], (1.0 - d[t]) * (1.0 - tr[t])
        v1, e1 = (B[t], eB[t]) if (boot is not None and tr[t] != 0 and d[t] == 0) else (V[t + 1], eV[t + 1])
        x = ln[t] - lo[t]
        ratio = np.exp(x)
        e_ratio = ratio * (EXPF_ULPS * 2.0 ** -23 + U32 * abs(x)) * (1 + 1e-6)
        rho, a = min(rho_bar, ratio), gamma * lmbda * min(c_bar, ratio) * m
        inner = r[t] + gamma * v1 * nd - V[t]
        e_inner = eV[t] + gamma * nd * e1
        delta = rho * inner
        e_step = e_ratio * (abs(inner) + e_inner) + rho * e_inner + gamma * lmbda * m * e_ratio * (abs(A) + bound)
        S = abs(delta) + a * S
        bound = e_step + a * bound
        A = delta + a * A
        adv[t], tol[t] = A, bound + depth * U64 * S
    vt = V[:n] + adv
    return adv, vt, tol + 0.5 * ulp32(adv), tol + eV[:n] + 0.5 * ulp32(vt)


def spans(L):
    return tuple(int(L.rlppo_gae_vtrace_span(k)) for k in range(3))   # steps per lane, wave, workgroup


def make_case(name, s, w, g, seed=0):
    """-> dict of float32 inputs.  Ends sit where a carry changes hands: lane, wave and workgroup boundaries."""
    rs = np.random.RandomState(seed)
    single = {"one": 1, "s-1": s - 1, "s": s, "s+1": s + 1, "w+1": w + 1, "g-1": g - 1, "g": g, "g+1": g + 1, "3g+5": 3 * g + 5}
    done_at, trunc_at = [], []
    if name in single:
        n = single[name]
    elif name.startswith("done@"):                      # a done on the last step of a workgroup's range and on the first of the next
        n = single[name[5:]]
        done_at = [k for c in (1, 2, 3) for k in (c * g - 1, c * g) if k < n]
    elif name == "short":                               # many trajectories of 1 to 3 steps, ends done and truncated in turn
        n = g + w + s + 3
        ends = np.cumsum(rs.randint(1, 4, size=n))
        ends = ends[ends < n]
        done_at, trunc_at = list(ends[::2]), list(ends[1::2])
    else:                                               # "boot": truncated-not-done steps with their own values at a workgroup boundary
        n = 2 * g + 5
        trunc_at, done_at = [g - 1, g, 2 * g - 1, 2 * g - 2], [2 * g - 2]   # (2g - 2: done wins over truncated)
    c = dict(rews=rs.randn(n), values=rs.randn(n + 1), dones=np.zeros(n), trunc=np.zeros(n), lpo=-1.5 + 0.5 * rs.randn(n))
    c["dones"][done_at], c["trunc"][trunc_at] = 1.0, 1.0
    c["lpn"] = c["lpo"] + rs.uniform(np.log(0.2), np.log(5.0), size=n)          # ratios on both sides of both clips
    c["boot"] = np.where((c["trunc"] != 0) & (c["dones"] == 0), rs.randn(n), np.nan)   # NaN where it must never be used
    return {k: np.asarray(x, np.float32) for k, x in c.items()}


def run(L, c, rho_bar, c_bar, scale=None, st=None, keep=None):
    """-> (advantages, value_targets, workspace, keep); keep: an earlier call's device tensors, reused as they are (a captured call)."""
    n = len(c["rews"])
    if keep is None:
        keep = dict({k: dev(x) for k, x in c.items()}, scale=None if scale is None else dev(scale), vt=torch.full((n,), 7.0, device="cuda"),
                    adv=torch.full((n,), 7.0, device="cuda"), ws=torch.zeros(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda"))
    t = keep
    check(L, L.rlppo_gae_vtrace(st or stream(), P(t["rews"]), P(t["dones"]), P(t["trunc"]), P(t["values"]), P(t["boot"]), P(t["scale"]),
                                P(t["lpn"]), P(t["lpo"]), n, GAMMA, LMBDA, rho_bar, c_bar, float("nan"), P(t["vt"]), P(t["adv"]), P(t["ws"]),
                                t["ws"].numel()))
    return t["adv"], t["vt"], t["ws"], t


def assert_within(got, want, tol, what):
    frac = np.abs(np.asarray(got, np.float64) - want) / tol
    print(f"{what}: worst element uses {frac.max():.3f} of its allowance")
    assert np.isfinite(got).all() and frac.max() <= 1.0, (what, int(frac.argmax()), frac.max())


CASES = ["one", "s-1", "s", "s+1", "w+1", "g-1", "g", "g+1", "3g+5", "done@g", "done@g+1", "done@3g+5", "short", "boot"]


@pytest.mark.parametrize("scale", [None, SCALE], ids=["real", "scaled"])
@pytest.mark.parametrize("clips", [(1.0, 1.0), (2.0, 0.5)], ids=["1-1", "2-0.5"])
@pytest.mark.parametrize("name", CASES)
def test_scan_matches_float64(L, name, clips, scale):
    s, w, g = spans(L)
    c = make_case(name, s, w, g, seed=len(name))
    adv, vt, ws, _ = run(L, c, *clips, scale=scale)
    assert int(ws[4:8].view(torch.int32).item()) == 0, "a look-back wait timed out in a clean run"
    a64, v64, ta, tv = truth(c["rews"], c["dones"], c["trunc"], c["values"], c["boot"], c["lpn"], c["lpo"], *clips, scale=scale, g=g)
    assert_within(adv.cpu().numpy(), a64, ta, f"{name} advantages")
    assert_within(vt.cpu().numpy(), v64, tv, f"{name} value_targets")


@pytest.mark.parametrize("name", ["s+1", "done@3g+5", "boot"])
def test_equal_log_probabilities_give_the_bootstrap_scan(L, name):
    """Each side within its allowance of the same float64 truth (see the module docstring: not bit for bit)."""
    s, w, g = spans(L)
    c = make_case(name, s, w, g, seed=7)
    c["lpn"] = c["lpo"].copy()
    adv, vt, _, t = run(L, c, 1.0, 1.0)
    n = len(c["rews"])
    bvt, badv, bret = (torch.empty(n, device="cuda") for _ in range(3))
    ws = torch.zeros(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    check(L, L.rlppo_gae_boot(stream(), P(t["rews"]), P(t["dones"]), P(t["trunc"]), P(t["values"]), P(t["boot"]), n, GAMMA, LMBDA, float("nan"),
                              P(bvt), P(badv), P(bret), P(ws), ws.numel()))
    a64, v64, ta, tv = truth(c["rews"], c["dones"], c["trunc"], c["values"], c["boot"], c["lpn"], c["lpo"], 1.0, 1.0, g=g)
    for got, want, tol, what in ((adv, a64, ta, "vtrace adv"), (badv, a64, ta, "boot adv"), (vt, v64, tv, "vtrace vt"), (bvt, v64, tv, "boot vt")):
        assert_within(got.cpu().numpy(), want, tol, f"{name} {what}")


def test_same_bits_run_to_run_and_under_capture(L):
    """Two eager calls, the two-launch form and three replays of a captured call: one set of bits (open chunks chain three look-backs)."""
    s, w, g = spans(L)
    c = make_case("3g+5", s, w, g, seed=11)
    first = run(L, c, 2.0, 0.5, scale=SCALE)
    again = run(L, c, 2.0, 0.5, scale=SCALE)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    check(L, L.rlppo_dbg_set(1, 0))                     # the stateless two-launch form, eager
    try:
        two = run(L, c, 2.0, 0.5, scale=SCALE)
    finally:
        check(L, L.rlppo_dbg_set(1, 1))
    assert torch.equal(first[0], two[0]) and torch.equal(first[1], two[1])
    keep, side = again[3], torch.cuda.Stream()          # the captured call works on the second call's tensors
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
            run(L, c, 2.0, 0.5, st=ctypes.c_void_p(side.cuda_stream), keep=keep)
    for _ in range(3):
        keep["adv"].zero_(), keep["vt"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(keep["adv"], first[0]) and torch.equal(keep["vt"], first[1])


# ------------------------------------------------------------------------------------------------ the option, end to end
NA, T = 8, 16


def learner_of(**kw):
    import synthetic_env
    from rlgym_ppo_amd import Learner
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        return Learner(lambda: synthetic_env.SyntheticVectorEnv(obs_dim=13, n_actions=7, n_agents=NA, seed=0), vector_env=True, n_proc=1,
                       timestep_limit=10 ** 9, exp_buffer_size=3 * NA * T, ts_per_iteration=NA * T, ppo_epochs=2, ppo_batch_size=NA * T,
                       ppo_minibatch_size=NA * T, policy_layer_sizes=(32, 32), critic_layer_sizes=(32, 32), checkpoints_save_folder=None,
                       checkpoint_load_folder=None, save_every_ts=10 ** 12, log_to_wandb=False, random_seed=5, standardize_returns=False, **kw)


@pytest.mark.parametrize("on", [True, False], ids=["vtrace", "off"])
def test_learner_recomputes_the_whole_buffer(on, monkeypatch):
    learner = learner_of(gae_vtrace=on, gae_vtrace_rho_bar=1.0, gae_vtrace_c_bar=1.0)
    buf, n = learner.experience_buffer, NA * T
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            for it in range(2):
                before = (buf.values.clone(), buf.advantages.clone())
                exp = learner.agent.collect_timesteps(n)[0]
                learner.add_new_experience(exp)
                if it == 0:
                    learner.ppo_learner.learn(buf)      # policy and critic move: the first iteration's rows are off-policy now
        older = (buf.values[:n], buf.advantages[:n])
        if not on:                                      # the library as it was: the older rows keep what they were submitted with
            assert torch.equal(older[0], before[0]) and torch.equal(older[1], before[1]) and learner._vtrace_host is None
            return
        assert not torch.equal(older[1], before[1])
        pol, vn = learner.ppo_learner.policy, learner.ppo_learner.value_net
        values = torch.cat((vn(buf.states).reshape(-1), vn.forward_padded(learner.agent.value_input_rows)[n:])).cpu().numpy()
        lpn = pol.get_backprop_data(buf.states, buf.actions)[0].detach().reshape(-1).cpu().numpy()
        host = lambda x: x.reshape(-1).cpu().numpy()
        a64, v64, ta, tv = truth(host(buf.rewards), host(buf.dones), host(buf.truncated), values, None, lpn, host(buf.log_probs), 1.0, 1.0,
                                 gamma=learner.gae_gamma, lmbda=learner.gae_lambda)
        assert_within(host(buf.advantages), a64, ta, "buffer advantages")
        assert_within(host(buf.values), v64, tv, "buffer value_targets")
        from rlgym_ppo_amd import learner as LM
        reports = []
        monkeypatch.setattr(LM.reporting, "report_metrics", lambda loggable_metrics, **kw: reports.append(loggable_metrics))
        learner.timestep_limit = learner.agent.cumulative_timesteps + n
        with contextlib.redirect_stdout(io.StringIO()):
            learner._learn()                            # one more iteration through the loop that builds the report
        assert 0.0 < reports[0]["V-trace Mean Rho"] <= 1.0 and 0.0 <= reports[0]["V-trace Clipped Fraction"] <= 1.0
    finally:
        learner.cleanup()
