"""The categorical critic on the GPU (include/rlppo.h, "[vbins]"; ppo.ValueBins, Learner(ppo_value_head=...)): the loss and readout
kernels, one whole pass and the Learner loop against a plain float64 torch restatement (cross_entropy below).

Tolerance of the kernel tests: the same restatement runs in float32; the HIP result may miss float64 by K times what that misses it
by in the same case, plus one float32 ulp of the row's largest magnitude.  K = 5 comes from the references alone and was fixed
from their first comparison: a second float32 implementation of the restatement (torch's, on the device) missed float64 by up to
4.97 times what the host's does (beyond the same one ulp), rounded up.  (On the present cases that comparison has one outlier -- the
one-row two-hot case whose target is a bin centre, where the two float32 runs take floor(u) to different sides -- and is at most 2.3
otherwise; K stayed what it was.)  What the kernels reach of it stands in DESIGN.md section 4."""
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ppo_yardstick as A  # noqa: E402
import synthetic_env  # noqa: E402
from hip_pass import L, P, check, dev, stream  # noqa: E402,F401

K = 5.0
NS, ROWS, KINDS = (2, 8, 9, 101, 128, 129, 256), (1, 17, 259), ("hl_gauss", "two_hot")
ulp = lambda x: float(np.spacing(np.float32(np.abs(x).max())))
quiet = lambda: contextlib.redirect_stdout(io.StringIO())


def cross_entropy(z, tgt, b, vs=None):
    """Rows' cross-entropy of logits z against the histogram of tgt over the bins b, and the bin centres: in z's dtype, differentiable."""
    t = torch.as_tensor(tgt).to(z)
    if vs is not None:
        t = (t - float(vs[0])) * float(vs[1])
    n, (lo, hi) = b.n, b.value_range
    w = (hi - lo) / n
    t = t.clamp(lo, hi)[:, None]
    edges = lo + w * torch.arange(n + 1, dtype=z.dtype, device=z.device)
    if b.kind == "hl_gauss":
        cdf = 0.5 * (1 + torch.special.erf((edges - t) / (b.sigma_ratio * w * 2 ** 0.5)))
        p = (cdf[:, 1:] - cdf[:, :-1]) / (cdf[:, -1:] - cdf[:, :1])
    else:
        u = ((t - (lo + w / 2)) / w).clamp(0, n - 1)
        k = u.floor().clamp(max=n - 2)
        p = torch.zeros(len(t), n, dtype=z.dtype, device=z.device).scatter_(1, k.long(), 1 - (u - k)).scatter_(1, k.long() + 1, u - k)
    return -(p * torch.log_softmax(z, 1)).sum(1), edges[:-1] + w / 2


def restate(logits, tgt, b, scale, vs, dtype):
    """-> (row losses, d(scale * their sum) / d logits, values = sum softmax * centres) of the restatement in `dtype`, as float64 arrays."""
    z = torch.as_tensor(logits).to(dtype).requires_grad_(True)
    ce, centres = cross_entropy(z, tgt, b, vs)
    (ce.sum() * scale).backward()
    return ce.detach().double().numpy(), z.grad.double().numpy(), (torch.softmax(z.detach(), 1) * centres).sum(1).double().numpy()


def case(kind, n, rows):
    """Peaked logits (scale 4) and targets.  The first six targets of every case of 17 or 259 rows are vmin, vmax, a bin edge, a bin
    centre, one below vmin and one above vmax (rotated by n, so the one-row cases take different ones: n = 2, 8, 128 the edge, 9 and
    129 the centre, 101 the one above vmax, 256 the one below vmin); uniform draws follow.  Every other case along kind, n and rows
    has its targets in real units behind a value scale {mu, 1/sigma, sigma} = {1.5, 1/4, 4}, whose arithmetic is exact for the six,
    so that they arrive at vmin, vmax, the edge and the centre behind it too (the edge is hit exactly for even n, where it is the middle of the
    range, and to float32's rounding for odd n); every (kind, n) has a case of 17 or 259 rows without the scale."""
    from rlgym_ppo_amd.ppo import ValueBins
    b = ValueBins(n, (-10.0, 10.0) if kind == "hl_gauss" else (-3.0, 7.0), kind)
    rs = np.random.RandomState(1000 * n + rows)
    (lo, hi), w = b.value_range, (b.value_range[1] - b.value_range[0]) / n
    vs = np.array([1.5, 0.25, 4.0, 0.0], np.float32) if (KINDS.index(kind) + NS.index(n) + ROWS.index(rows)) % 2 else None
    special = np.roll([lo, hi, lo + w * (n // 2), lo + w * (n // 2 + 0.5), lo - 1.0, hi + 2.5], -(n % 6))
    t = np.concatenate([special, rs.uniform(lo, hi, rows)])[:rows]
    return b, (4 * rs.randn(rows, n)).astype(np.float32), (t * 4.0 + 1.5 if vs is not None else t).astype(np.float32), vs


def padded(L, logits):
    """Device rows of the library's padded width + one guard row of 7s; the padding holds NaN (it must never reach a sum)."""
    rows, n = logits.shape
    z = torch.full((rows + 1, int(L.rlppo_padded_out(n))), float("nan"))
    z[:rows, :n], z[rows] = torch.as_tensor(logits), 7.0
    return z.cuda()


def hip_loss(L, b, logits, t, vs, mb_ratio):
    z, td, stats, arg = padded(L, logits), dev(t), torch.zeros(8, dtype=torch.float64, device="cuda"), b.c_arg()
    vsd = None if vs is None else dev(vs)
    check(L, L.rlppo_dbg_value_bins_loss(stream(), P(z), z.shape[1], ctypes.byref(arg), P(td), len(t), mb_ratio, P(vsd), P(stats)))
    return z.cpu().double().numpy(), float(stats[2])


def hip_values(L, b, logits):
    z, out, arg = padded(L, logits), torch.full((len(logits) + 1,), 7.0, device="cuda"), b.c_arg()
    check(L, L.rlppo_value_bins_readout(stream(), P(z), z.shape[1], ctypes.byref(arg), P(out), len(logits)))
    assert out[-1] == 7.0
    return out[:-1].cpu().double().numpy()


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind", KINDS)
def test_loss_kernel_against_float64(L, kind, n, rows):
    b, logits, t, vs = case(kind, n, rows)
    scale = 0.5 * float(np.float32(1.0) / np.float32(rows))   # mb_ratio * inv_mb, as the pass applies it
    ce64, g64, _ = restate(logits, t, b, scale, vs, torch.float64)
    ce32, g32, _ = restate(logits, t, b, scale, vs, torch.float32)
    g, vloss = hip_loss(L, b, logits, t, vs, 0.5)
    again = hip_loss(L, b, logits, t, vs, 0.5)
    assert np.array_equal(g, again[0]) and vloss == again[1], "two launches differ"
    assert (g[:rows, n:] == 0).all() and (g[rows] == 7.0).all(), "padded columns are not exact zeros, or the row behind the last was touched"
    e_hip, e_32 = np.abs(g[:rows, :n] - g64).max(1), np.abs(g32 - g64).max()
    l_hip, l_32 = abs(vloss - ce64.mean()), np.abs(ce32 - ce64).max()
    print(f"[vbins loss] {kind} n={n} rows={rows}: g {e_hip.max():.2e} vs float32 {e_32:.2e}; loss {l_hip:.2e} vs {l_32:.2e}")
    assert (e_hip <= K * e_32 + np.spacing(np.abs(g64).max(1).astype(np.float32))).all(), (e_hip.max(), e_32)
    assert l_hip <= K * l_32 + ulp(ce64), (l_hip, l_32)


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("n", NS)
def test_readout_against_float64(L, n, rows):
    b, logits, t, _ = case(KINDS[n % 2], n, rows)
    v64, v32 = (restate(logits, t, b, 1.0, None, d)[2] for d in (torch.float64, torch.float32))
    e_hip, e_32 = np.abs(hip_values(L, b, logits) - v64).max(), np.abs(v32 - v64).max()
    print(f"[vbins readout] n={n} rows={rows}: {e_hip:.2e} vs float32 {e_32:.2e}")
    assert e_hip <= K * e_32 + ulp(b.value_range), (e_hip, e_32)
    flat = hip_values(L, b, np.zeros_like(logits))   # uniform softmax: the midpoint of the range
    assert np.abs(flat - sum(b.value_range) / 2).max() <= ulp(b.value_range)


@pytest.mark.parametrize("n", NS)
def test_two_hot_histogram_has_the_targets_expectation(L, n):
    """At uniform q and a row scale of exactly 1 (256 rows, mb_ratio 256) the stored gradient is 1 / n - p: the kernel's own histogram."""
    from rlgym_ppo_amd.ppo import ValueBins
    b, w = ValueBins(n, (-10.0, 10.0), "two_hot"), 20.0 / n
    t = np.random.RandomState(n).uniform(-10 + 0.51 * w, 10 - 0.51 * w, 256).astype(np.float32)
    g, _ = hip_loss(L, b, np.zeros((256, n), np.float32), t, None, 256.0)
    p = 1.0 / n - g[:256, :n]
    assert np.abs(p @ (-10 + w * (np.arange(n) + 0.5)) - t).max() <= 2 * ulp(10.0) and (np.count_nonzero(np.abs(p) > 1e-6, axis=1) <= 2).all()


# ------------------------------------------------------------------------------------------------ one whole pass
OBS, MB, ACTIONS, SEED = 20, 259, 6, 16   # (SEED: no ReLU pre-activation of the critic within 1e-4 of zero, asserted below)


def learn_once(act, norm, bins, scaled, switches=(), setup=None):
    """A PPOLearner (discrete policy 20 -> 32 -> 6, critic 20 -> 32 -> n or 1) and one learn() on 259 made-up rows under rlppo_dbg_set
    `switches`, after setup(learner) -> (the batch gradient [policy | critic] its probe shows, the learner, the critic's torch module
    before the step, the observations, the targets, the value scale or None)."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.ppo import ExperienceBuffer, LayerSizes, PPOLearner
    torch.manual_seed(SEED)
    with quiet():
        learner = PPOLearner(OBS, ACTIONS, 0, (32,), LayerSizes((32,), act, "layer" if norm else None, bins), (0.1, 1.0), MB, 1, 3e-4, 3e-4, 0.2,
                             0.005, MB, "cuda:0")
    vs = None
    if scaled:
        learner.set_value_normalization(True)
        learner.load_value_norm_state({"count": 1000.0, "mean": 0.7, "var": 4.0})
        vs = learner.value_norm.scale.cpu().numpy()
    rs = np.random.RandomState(SEED)
    obs, z = np.clip(rs.randn(MB, OBS), -5, 5).astype(np.float32), np.zeros(MB, np.float32)
    tgt = (3 * rs.randn(MB)).astype(np.float32)
    buf = ExperienceBuffer(MB, SEED, "cpu")
    buf.submit_experience(obs, rs.randint(0, ACTIONS, MB).astype(np.float32), (-1.8 + 0.1 * rs.randn(MB)).astype(np.float32), z, obs, z, z, tgt,
                          rs.randn(MB).astype(np.float32))
    seen, critic = [], copy.deepcopy(learner.value_net.model).cpu()
    learner.grad_probe = lambda g: seen.append(g.detach().cpu().clone())
    if setup is not None:
        setup(learner)
    for key, value in switches:
        N.check(N.lib().rlppo_dbg_set(key, value))
    try:
        with quiet():
            learner.learn(buf)
    finally:
        for key, _ in switches:
            N.check(N.lib().rlppo_dbg_set(key, 1))
    assert len(seen) == 1
    return seen[0], learner, critic, obs, tgt, vs


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_pass_against_float64_and_the_policy_is_untouched(L, act, norm, scaled):
    from rlgym_ppo_amd.ppo import ValueBins
    bins = ValueBins(9 if act == "relu" else 101, (-4.0, 4.0), "two_hot" if scaled else "hl_gauss")
    before = int(L.rlppo_dbg_counter(17))
    got, learner, critic, obs, tgt, vs = learn_once(act, norm, bins, scaled)
    assert int(L.rlppo_dbg_counter(17)) == before + 1   # the pass with bins ran
    grads = []
    for dtype in (torch.float64, torch.float32):
        m, x = copy.deepcopy(critic).to(dtype), torch.as_tensor(obs).to(dtype)
        assert act != "relu" or float(m[0](x).detach().abs().min()) > 1e-4, "a ReLU pre-activation lies at zero: choose another SEED"
        cross_entropy(m(x), tgt, bins, vs)[0].mean().backward()
        grads.append([p.grad for p in m.parameters()])
    n_pol = off = learner.policy.arena.n_flat
    for i, (a, b32) in enumerate(zip(*grads)):
        e_hip, e_32 = A.rel(got[off:off + a.numel()].view(a.shape), a), A.rel(b32, a)
        off += a.numel()
        print(f"[vbins pass] {act} norm={norm} scaled={scaled} tensor {i}: err(HIP, fp64)={e_hip:.2e} err(float32, fp64)={e_32:.2e}")
        assert e_hip <= max(1e-5, 1.5 * e_32), (i, e_hip, e_32)
    assert off == got.numel()
    # the chains do not meet: with the weight gradients launched per chain (switch 37 off; the grouped launch splits its rows by the
    # set of all products) the policy's gradient beside this critic equals, bit for bit, the one beside a one-output critic (whose
    # ReLU pass is made plain too, switch 19 off)
    cat = learn_once(act, norm, bins, scaled, ((37, 0),))[0][:n_pol]
    one = learn_once(act, norm, None, scaled, ((37, 0), (19, 0)))[0][:n_pol]
    assert torch.equal(cat, one) and cat.abs().max() > 0


REFUSED = {"value_clip_range": lambda p: setattr(p, "value_clip_range", 0.2), "preserve_outputs": lambda p: p.set_value_normalization(True, True),
           "'bf16'": lambda p: setattr(p, "update_precision", "bf16"), "'x3'": lambda p: setattr(p, "update_precision", "x3")}


@pytest.mark.parametrize("what", list(REFUSED))
def test_ppo_learner_refusals_launch_nothing(L, what):
    from rlgym_ppo_amd.ppo import ValueBins
    before = [int(L.rlppo_dbg_counter(k)) for k in (2, 17)]
    with pytest.raises(ValueError, match="categorical critic.*" + what + "|" + what + ".*categorical critic"):
        learn_once("relu", False, ValueBins(9), False, setup=REFUSED[what])
    assert [int(L.rlppo_dbg_counter(k)) for k in (2, 17)] == before


# ------------------------------------------------------------------------------------------------ through the public interface
def run_learner(tmp_path, **kw):
    """Two iterations of a Learner on tests/synthetic_env.py (16 agents x 8 steps each) -> (reports, what every value pass and scan saw,
    the critic module + batch + scale in front of the last learn(), the learner's ppo_learner)."""
    import rlgym_ppo_amd.learner as LM
    from test_gpu_value_norm import GAMMA, LMBDA
    cfg = dict(n_proc=1, timestep_limit=256, exp_buffer_size=128, ts_per_iteration=128, ppo_epochs=1, ppo_batch_size=128, policy_layer_sizes=(32,),
               critic_layer_sizes=(32, 32), checkpoints_save_folder=str(tmp_path), add_unix_timestamp=False, checkpoint_load_folder=None,
               save_every_ts=10 ** 12, log_to_wandb=False, random_seed=5, gae_gamma=GAMMA, gae_lambda=LMBDA, min_inference_size=1)
    cfg.update(kw)
    torch.manual_seed(5)
    with quiet():
        learner = LM.Learner(synthetic_env.make_vector_env if cfg.get("vector_env") else synthetic_env.make_discrete_env, **cfg)
    ppo, scans, reports, last = learner.ppo_learner, [], [], {}
    vnet, gae, learn, printer = ppo.value_net, LM.torch_functions.gae_device_deferred, ppo.learn, LM.reporting.report_metrics

    def value_pass(rows):
        out = vnet.__class__.forward_padded(vnet, rows)
        scans.append(dict(logits=vnet.arena.forward(rows)[:, :vnet.value_bins.n].cpu().numpy(), values=out.cpu().numpy()))
        return out

    def scan(rews, dones, trunc, values, **k):
        out = gae(rews, dones, trunc, values, **k)
        scans[-1].update(args=[x.cpu().numpy() for x in (rews, dones, trunc, values)], scale=k["value_scale"].cpu().numpy() if "value_scale" in k else None,
                         std=k.get("return_std"), out=[x.cpu().numpy() for x in out[:3]])
        return out

    def spy_learn(exp):
        last.update(critic=copy.deepcopy(vnet.model).cpu().double(), states=exp.states.cpu().numpy()[:, :vnet.arena.d_in], targets=exp.values.cpu().numpy(),
                    scale=None if ppo.value_norm is None else ppo.value_norm.scale.cpu().numpy())
        return learn(exp)
    vnet.forward_padded, LM.torch_functions.gae_device_deferred, ppo.learn = value_pass, scan, spy_learn
    LM.reporting.report_metrics = lambda loggable_metrics, debug_metrics, wandb_run=None: reports.append(dict(loggable_metrics))
    try:
        with quiet():
            learner._learn()
        torch.cuda.synchronize()
    finally:
        LM.torch_functions.gae_device_deferred, LM.reporting.report_metrics = gae, printer
        learner.agent.cleanup()
    return reports, scans, last, ppo


def test_learner_scans_the_readout_reports_the_cross_entropy_and_checkpoints(L, tmp_path):
    import value_norm_yardstick as VY
    from rlgym_ppo_amd.ppo import LayerSizes, PPOLearner, ValueBins
    from test_gpu_value_norm import GAMMA, LMBDA, assert_close_norm
    reports, scans, last, ppo = run_learner(tmp_path, vector_env=True, ppo_value_head="hl_gauss", ppo_value_bins=51, ppo_normalize_value=True)
    bins = ppo.value_net.value_bins
    assert len(reports) == 2 and bins == ValueBins(51) and ppo.value_net.arena.dims[-1] == 51
    for s in scans:   # the scan read the readout of the critic's logits, taken to real units as fmaf(v^, sigma, mu)
        v64, v32 = (restate(s["logits"], np.zeros(len(s["logits"])), bins, 1.0, None, d)[2] for d in (torch.float64, torch.float32))
        assert np.abs(s["values"] - v64).max() <= K * np.abs(v32 - v64).max() + ulp(10.0)
        if "args" in s:
            rews, dones, trunc, vhat = s["args"]
            mu, sigma = float(s["scale"][0]), float(s["scale"][2])
            want = VY.gae(rews, dones, trunc, vhat, None, mu, sigma, GAMMA, LMBDA, s["std"])
            assert_close_norm(s["out"], want, np.abs(vhat.astype(np.float64) * sigma + mu).max(), "categorical critic")
    ce = [cross_entropy(last["critic"].to(d)(torch.as_tensor(last["states"]).to(d)), last["targets"], bins, last["scale"])[0].detach().double().numpy()
          for d in (torch.float64, torch.float32)]
    vloss = reports[-1]["Value Function Loss"]
    assert np.isfinite(vloss) and abs(vloss - ce[0].mean()) <= K * np.abs(ce[1] - ce[0]).max() + ulp(ce[0]), (vloss, ce[0].mean())
    ppo.save_to(str(tmp_path))
    torch.manual_seed(0)
    with quiet():
        fresh = PPOLearner(107, 90, 0, (32,), LayerSizes((32, 32), value_head=bins), (0.1, 1.0), 128, 1, 3e-4, 3e-4, 0.2, 0.005, 128, "cuda:0")
    fresh.load_from(str(tmp_path))
    assert fresh.value_net.model[-1].weight.shape == (51, 32) and torch.equal(fresh.value_net.arena.flat, ppo.value_net.arena.flat)


@pytest.mark.parametrize("kw", [dict(vector_env=True, ppo_value_head="two_hot"), dict(ppo_value_head="hl_gauss", ppo_value_range=(-5.0, 5.0))],
                         ids=["two_hot", "process_mode"])
def test_learner_other_kind_and_process_mode_are_finite_and_reproducible(L, tmp_path, kw):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # (the default range without ppo_normalize_value: warned about once)
        runs = [run_learner(tmp_path / str(i), **kw) for i in range(2)]
    for reports, scans, _, _ in runs:
        # (the first iteration reports NaN for every critic: the reference's quirk Q10, kept by Learner._learn)
        assert all(np.isfinite(s["values"]).all() for s in scans) and len(reports) == 2 and np.isfinite(reports[1]["Value Function Loss"])
    assert torch.equal(runs[0][3].value_net.arena.flat, runs[1][3].value_net.arena.flat)
    assert runs[0][0][1]["Value Function Loss"] == runs[1][0][1]["Value Function Loss"]


