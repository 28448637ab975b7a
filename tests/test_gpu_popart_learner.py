"""PopArt's weight-preserving step at the Learner level (ppo_value_norm_popart): the critic's real-unit predictions on the iteration's
own rows across the statistic step, off is off, checkpoint and continue, two virtual ranks, one process-mode iteration.  The
environment, the sizes and the runner are tests/test_gpu_value_norm_learner.py's."""
import contextlib
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import popart_yardstick as PY  # noqa: E402
import synthetic_env  # noqa: E402
from test_gpu_value_norm_learner import ITERS, NA, T, build_ppo, host, make_learner, run_learner, same_state  # noqa: E402

POPART = dict(ppo_normalize_value=True, ppo_value_norm_popart=True)


@contextlib.contextmanager
def counted_entries():
    """Counts the calls of the two update entry points through the _native table (the library object every caller shares)."""
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    names = ("rlppo_value_norm_update", "rlppo_value_norm_update_popart")
    real, calls = {k: getattr(L, k) for k in names}, {k: 0 for k in names}

    def wrap(k):
        def fn(*a):
            calls[k] += 1
            return real[k](*a)
        return fn
    for k in names:
        setattr(L, k, wrap(k))
    try:
        yield calls
    finally:
        for k in names:
            setattr(L, k, real[k])


def spy_on_the_statistic_step(learner, seen):
    """Around PPOLearner.update_value_norm, inside add_new_experience: the critic's outputs on the iteration's own rows and the scale,
    before and after, with the weights the allowance needs."""
    p = learner.ppo_learner
    plain = p.update_value_norm

    def spy(targets):
        net, vn = p.value_net, p.value_norm
        rows = learner.agent.value_input_rows
        layers = [(host(l.weight).copy(), host(l.bias).copy()) for l in net.arena.linears]
        rec = dict(layers=layers, x=host(rows)[:, :net.arena.d_in].copy(), s0=host(vn.scale).copy(), v0=host(net.forward_padded(rows)).copy(),
                   flat0=net.arena.flat.clone())
        plain(targets)
        rec.update(s1=host(vn.scale).copy(), stale=not net.arena.packed_is_current(), flat1=net.arena.flat.clone())
        rec.update(v1=host(net.forward_padded(rows)).copy(), last=(host(net.arena.linears[-1].weight).copy(), host(net.arena.linears[-1].bias).copy()))
        seen.append(rec)
    p.update_value_norm = spy


def test_predictions_are_preserved_across_the_statistic_step(tmp_path):
    learner, seen = make_learner(tmp_path / "on", **POPART), []
    assert learner.value_norm_popart and learner.ppo_learner.value_norm_preserve_outputs and learner.config["ppo_value_norm_popart"] is True
    spy_on_the_statistic_step(learner, seen)
    with counted_entries() as calls:
        run_learner(learner)
    assert calls == {"rlppo_value_norm_update": 0, "rlppo_value_norm_update_popart": ITERS} and len(seen) == ITERS
    for it, r in enumerate(seen):
        assert r["x"].shape[0] == NA * T + 1 and r["stale"]
        (w, b), (w1, b1) = r["layers"][-1], r["last"]
        w2, b2 = PY.rescale(w, b, r["s0"], r["s1"])
        assert w1.tobytes() == w2.tobytes() and abs(float(b1[0]) - float(b2)) <= float(np.spacing(np.float32(abs(b2))))
        n_last = w.size + 1
        assert torch.equal(r["flat0"][:-n_last], r["flat1"][:-n_last]) and not torch.equal(r["flat0"], r["flat1"])
        allow = PY.allowance(w, b, w1, b1, PY.hidden64(r["layers"], r["x"]), r["s0"], r["s1"])
        V0, V1 = PY.real_units32(r["v0"], r["s0"]).astype(np.float64), PY.real_units32(r["v1"], r["s1"]).astype(np.float64)
        bare = PY.real_units32(r["v0"], r["s1"]).astype(np.float64)                     # what the critic would say without the rescale
        ratio, moved = np.abs(V1 - V0) / allow, np.abs(bare - V0) / allow
        print(f"[popart learner] iteration {it}: scale {r['s0'][[0, 2]]} -> {r['s1'][[0, 2]]}; |V1 - V0| at most {ratio.max():.3g} of the allowance "
              f"(without the rescale at least {moved.min():.3g} times it)")
        assert ratio.max() <= 1.0, (it, ratio.max())
    assert abs(seen[0]["s1"][0]) > 5.0 and seen[0]["s1"][2] > 5.0                       # targets far from the unit scale: the step matters


def test_off_leaves_the_critic_alone_and_calls_the_plain_entry(tmp_path):
    learner = make_learner(tmp_path / "off", ppo_normalize_value=True, ppo_value_norm_popart=False)
    assert not learner.value_norm_popart and not learner.ppo_learner.value_norm_preserve_outputs
    plain, flats = learner.add_new_experience, []

    def spy(experience):
        before = learner.ppo_learner.value_net.arena.flat.clone()
        out = plain(experience)
        flats.append(torch.equal(before, learner.ppo_learner.value_net.arena.flat))
        return out
    learner.add_new_experience = spy
    with counted_entries() as calls:
        off, _, _ = run_learner(learner)
    assert flats == [True] * ITERS                                                       # add_new_experience never writes the critic
    assert calls == {"rlppo_value_norm_update": ITERS, "rlppo_value_norm_update_popart": 0}
    # ... and it is the run without the keyword, bit for bit; the run with the step on is another one
    bare, _, _ = run_learner(make_learner(tmp_path / "bare", ppo_normalize_value=True))
    same_state(off, bare, ("pol", "val", "m", "vm", "book", "vnorm"))
    on, _, _ = run_learner(make_learner(tmp_path / "on", **POPART))
    assert not torch.equal(on["val"], off["val"])


def test_save_load_continue_equals_the_uninterrupted_run(tmp_path):
    """Three iterations against two + a second Learner that loads "latest" and runs the third, bit for bit (the construction of the
    test of the same name in tests/test_gpu_value_norm_learner.py).  The book holds the weights and the statistic; a load rescales
    nothing."""
    kw = dict(standardize_obs=False, standardize_returns=False, exp_buffer_size=NA * T, **POPART)
    whole, _, _ = run_learner(make_learner(tmp_path / "whole", **kw))
    first = make_learner(tmp_path / "ck", iters=2, save_every_ts=NA * T, **kw)
    s1, _, _ = run_learner(first)
    rng = torch.get_rng_state(), np.random.get_state(), first.experience_buffer.rng.get_state()
    assert s1["book"] == 2 * NA * T and whole["book"] == 3 * NA * T and s1["vnorm"] != whole["vnorm"]
    second = make_learner(tmp_path / "ck", start=2 * T, checkpoint_load_folder="latest", random_seed=9, **kw)
    try:
        vn = second.ppo_learner.value_norm
        assert host(vn.state).tobytes() + host(vn.scale).tobytes() == s1["vnorm"]
        assert torch.equal(second.ppo_learner.value_net.arena.flat, s1["val"])            # loaded as written: no rescale on load
        torch.set_rng_state(rng[0])
        np.random.set_state(rng[1])
        second.experience_buffer.rng.set_state(rng[2])
    except BaseException:
        second.agent.cleanup()
        raise
    resumed, _, _ = run_learner(second)
    same_state(resumed, whole, ("pol", "val", "m", "vm", "book", "vnorm"))


def test_two_virtual_ranks_end_a_learn_with_bit_identical_critics():
    """No collective is added: replicas that feed the same targets take the same deterministic step."""
    from rlgym_ppo_amd import dp
    from rlgym_ppo_amd.ppo import ExperienceBuffer
    from test_gpu_value_norm_learner import ACTIONS, D, ROWS
    rs = np.random.RandomState(1)
    obs = np.clip(rs.randn(ROWS, D), -5, 5).astype(np.float32)
    tgt = (40.0 + 25.0 * rs.randn(ROWS)).astype(np.float32)
    adv, z = rs.randn(ROWS).astype(np.float32), np.zeros(ROWS, np.float32)
    reps, bufs = [build_ppo() for _ in range(2)], []
    start = reps[0].value_net.arena.flat.clone()
    for learner in reps:
        learner.set_value_normalization(True, preserve_outputs=True)
        act, logp = learner.policy.get_action(obs)
        act = np.asarray(torch.as_tensor(act).cpu(), np.float32).reshape(ROWS)
        logp = np.asarray(torch.as_tensor(logp).cpu(), np.float32).reshape(ROWS)
        learner.update_value_norm(torch.as_tensor(tgt).cuda())
        buf = ExperienceBuffer(ROWS, 9, "cpu")
        buf.submit_experience(obs, act, logp, z, obs, z, z, tgt, adv)
        bufs.append(buf)
    torch.cuda.synchronize()
    rescaled = reps[0].value_net.arena.flat.clone()
    assert torch.equal(rescaled, reps[1].value_net.arena.flat) and not torch.equal(rescaled, start)
    with contextlib.redirect_stdout(io.StringIO()):
        reports = dp.run_virtual_ranks(reps, bufs)
    torch.cuda.synchronize()
    assert torch.equal(reps[0].value_net.arena.flat, reps[1].value_net.arena.flat) and not torch.equal(reps[0].value_net.arena.flat, rescaled)
    assert torch.equal(reps[0].value_optimizer.exp_avg, reps[1].value_optimizer.exp_avg)
    assert host(reps[0].value_norm.state).tobytes() == host(reps[1].value_norm.state).tobytes()
    assert all(np.isfinite(r["Value Function Loss"]) for r in reports)


def test_one_process_mode_iteration_with_the_step_on():
    from rlgym_ppo_amd import Learner
    ts = 256
    torch.manual_seed(3)
    with contextlib.redirect_stdout(io.StringIO()):
        learner = Learner(synthetic_env.make_discrete_env, n_proc=2, min_inference_size=2, timestep_limit=10 ** 9, exp_buffer_size=4 * ts,
                          ts_per_iteration=ts, ppo_epochs=1, ppo_batch_size=ts, ppo_minibatch_size=ts // 2, policy_layer_sizes=(32, 32),
                          critic_layer_sizes=(32, 32), checkpoints_save_folder=None, checkpoint_load_folder=None, save_every_ts=10 ** 12,
                          log_to_wandb=False, random_seed=5, standardize_obs=False, standardize_returns=False, gae_bootstrap_truncated=True,
                          **POPART)
    try:
        learner.ppo_learner.load_value_norm_state({"count": 500.0, "mean": 3.0, "var": 4.0})
        arena = learner.ppo_learner.value_net.arena
        before, s0 = arena.flat.clone(), host(learner.ppo_learner.value_norm.scale).copy()   # (a state load rescales nothing)
        exp, _, _, _ = learner.agent.collect_timesteps(ts)
        n = np.asarray(exp[0]).shape[0]
        with contextlib.redirect_stdout(io.StringIO()):
            learner.add_new_experience(exp)
        s1 = host(learner.ppo_learner.value_norm.scale)
        st = host(learner.ppo_learner.value_norm.state)
        assert st[0] == 500.0 + n and st[3] == 0.0
        last = arena.linears[-1]
        n_last = last.weight.numel() + 1
        w2, b2 = PY.rescale(host(before[-n_last:-1]), host(before[-1:]), s0, s1)
        assert torch.equal(arena.flat[:-n_last], before[:-n_last]) and host(last.weight).tobytes() == w2.tobytes()
        assert abs(float(last.bias.item()) - float(b2)) <= float(np.spacing(np.float32(abs(b2))))
        with contextlib.redirect_stdout(io.StringIO()):
            report = learner.ppo_learner.learn(learner.experience_buffer)
        assert np.isfinite(report["Value Function Loss"])
    finally:
        learner.agent.cleanup()
