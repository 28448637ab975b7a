"""Value normalisation without a GPU: the yardstick's merge against numpy, and the three new entry points' argument errors (1001, a
message naming the argument, before any launch -- the host never dereferences the device pointers, so placeholders do)."""
import ctypes
import inspect

import numpy as np

import value_norm_yardstick as VY


def test_merge_over_batches_is_numpys_mean_and_population_variance():
    rs = np.random.RandomState(0)
    batches = [(5e3 + 30.0 * rs.randn(n)).astype(np.float32) for n in (1, 255, 4097, 3)]
    state = (0.0, 0.0, 0.0)
    for b in batches:
        state = VY.update(state, b)
    allx = np.concatenate(batches).astype(np.float64)
    assert state[0] == allx.size
    assert abs(state[1] - allx.mean()) <= 1e-12 * abs(allx.mean())
    assert abs(state[2] / state[0] - allx.var()) <= 1e-12 * allx.var()
    s = VY.scale64(state)
    assert abs(s[2] - np.sqrt(allx.var() + 1e-5)) <= 1e-12 * s[2] and abs(s[1] * s[2] - 1.0) <= 1e-15 and s[0] == state[1] and s[3] == 0.0
    # a fresh statistic publishes the identity, a batch with a NaN changes nothing, a constant batch has M2 == 0 exactly
    assert VY.scale64((0.0, 0.0, 0.0)).tolist() == [0.0, 1.0, 1.0, 0.0]
    bad = batches[1].copy()
    bad[7] = np.nan
    assert VY.update(state, bad) == state
    c = VY.update((0.0, 0.0, 0.0), np.full(300, 7.25, np.float32))
    assert c == (300.0, 7.25, 0.0) and VY.scale32(c)[2] == np.float32(np.sqrt(1e-5))


def test_value_loss_yardstick_is_the_plain_loss_on_normalised_numbers():
    rs = np.random.RandomState(1)
    n, mu, s = 200, -3.0, 0.125
    v, t, a = rs.randn(n), (5 * rs.randn(n)).astype(np.float32), rs.randn(n).astype(np.float32)
    tn = (t.astype(np.float64) - mu) * s
    loss, g = VY.value_loss64(v, t, a, mu, s)
    assert np.isclose(loss, ((v - tn) ** 2).mean(), rtol=1e-14) and np.allclose(g, 2 * (v - tn) / n, rtol=1e-14)
    loss_c, g_c = VY.value_loss64(v, t, a, mu, s, vclip=0.25, mb_ratio=0.5)
    v_old = ((t - a).astype(np.float64) - mu) * s
    inside = np.abs(v - v_old) <= 0.25
    assert 0 < inside.sum() < n and (g_c[~inside] == 0).all()
    assert np.allclose(g_c[inside], 0.5 * 2 * (v - tn)[inside] / n, rtol=1e-12)
    # finite differences of the clipped loss, on rows away from the kink
    far = np.abs(np.abs(v - v_old) - 0.25) > 1e-3
    h = 1e-6
    for i in np.flatnonzero(far)[:20]:
        vp, vm = v.copy(), v.copy()
        vp[i] += h
        vm[i] -= h
        fd = (VY.value_loss64(vp, t, a, mu, s, 0.25)[0] - VY.value_loss64(vm, t, a, mu, s, 0.25)[0]) / (2 * h)
        assert abs(0.5 * fd - g_c[i]) <= 1e-7, i


def test_python_surface():
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.ppo import PPOLearner, ValueNorm
    from rlgym_ppo_amd.util import torch_functions as TF
    p = inspect.signature(Learner.__init__).parameters["ppo_normalize_value"]
    assert p.default is False
    assert list(inspect.signature(PPOLearner.__init__).parameters)[-1] == "max_grad_norm"   # the switch is set_value_normalization
    for name in ("set_value_normalization", "value_norm_state", "load_value_norm_state"):
        assert callable(getattr(PPOLearner, name))
    for name in ("update", "denormalize", "state_dict", "load_state_dict"):
        assert callable(getattr(ValueNorm, name))
    for fn in (TF.gae_device_deferred, TF.gae_device, TF.compute_gae):
        assert inspect.signature(fn).parameters["value_scale"].default is None


def _lib():
    from rlgym_ppo_amd import _native as N
    return N, N.lib()


def test_value_norm_update_rejects_bad_arguments_before_any_launch():
    N, L = _lib()
    targets, state, scale, ws = 0x10000, 0x20000, 0x30000, 0x40000   # distinct, aligned, never dereferenced
    call = lambda *a: (L.rlppo_value_norm_update(None, *a), L.rlppo_last_error().decode())
    rc, msg = call(targets, 0, state, scale, ws)
    assert rc == 1001 and "n=0" in msg, (rc, msg)
    rc, msg = call(targets, -5, state, scale, ws)
    assert rc == 1001 and "n=-5" in msg, (rc, msg)
    rc, msg = call(targets, 100, None, scale, ws)
    assert rc == 1001 and "state" in msg and "NULL" in msg, (rc, msg)
    for args, word in (((None, 100, state, scale, ws), "targets"), ((targets, 100, state, None, ws), "scale"),
                       ((targets, 100, state, scale, None), "ws"), ((targets, 100, state + 4, scale, ws), "state"),
                       ((targets, 100, state, scale + 8, ws), "scale"), ((targets + 2, 100, state, scale, ws), "targets")):
        rc, msg = call(*args)
        assert rc == 1001 and word in msg, (args, rc, msg)
    assert N.VALUE_NORM_WS_BYTES == 4096


def test_gae_norm_rejects_a_misaligned_value_scale_before_any_launch():
    N, L = _lib()
    n = 5000
    fake = iter(range(0x10000, 0x1000000, 0x10000))
    rews, dones, trunc, values, boot, vt, adv, ret, ws = (next(fake) for _ in range(9))
    nbytes = int(L.rlppo_gae_workspace_bytes(n))
    call = lambda scale, b=boot: (L.rlppo_gae_norm(None, rews, dones, trunc, values, b, scale, n, 0.99, 0.95, float("nan"), vt, adv, ret, ws, nbytes),
                                  L.rlppo_last_error().decode())
    for scale in (0x2000004, 0x2000008):
        for b in (boot, None):
            rc, msg = call(scale, b)
            assert rc == 1001 and "value_scale" in msg and "16-byte aligned" in msg, (rc, msg)
    rc = L.rlppo_gae_norm(None, rews, dones, trunc, values, boot, 0x2000000, n, 0.99, 0.95, float("nan"), vt, adv, ret, ws, 16)
    assert rc != 0 and rc != 1001 and b"workspace" in L.rlppo_last_error()     # (the old rules stand behind the new one)


def test_ppo_minibatch_vnorm_rejects_a_bad_head_before_any_launch():
    N, L = _lib()
    pol, val = N.dims_array([21, 32, 32, 8]), N.dims_array([21, 32, 32, 1])
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim, a.slot, a.precision = 99, 3, 3, 1, 0, N.PRECISION_FP32
    a.pol_dims = ctypes.cast(pol, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(val, ctypes.POINTER(ctypes.c_int32))
    fake = iter(range(0x10000, 0x1000000, 0x1000))
    for f in ("pol_packed", "val_packed", "pol_grad", "val_grad", "states", "actions", "old_logp", "targets", "advantages", "idx", "stats", "workspace"):
        setattr(a, f, next(fake))
    a.ld_states, a.n_rows, a.mb = int(L.rlppo_padded_width(21)), 5000, 1500
    a.clip_range, a.ent_coef, a.mb_ratio, a.var_m, a.var_b = 0.2, 0.005, 1.0, 1.0, 0.0
    a.ws_bytes = L.rlppo_minibatch_workspace_bytes_for(pol, 3, val, 3, a.mb, N.PRECISION_FP32)
    vn = N.ValueNormArg()
    vn.scale = 0x2000000
    passes = L.rlppo_dbg_counter(2)
    rc = L.rlppo_ppo_minibatch_vnorm(None, ctypes.byref(a), None, None, ctypes.byref(vn))
    msg = L.rlppo_last_error().decode()
    assert rc == 1001 and "head 99" in msg, (rc, msg)
    a.head = N.HEAD_DISCRETE
    vn.scale = 0x2000004
    rc = L.rlppo_ppo_minibatch_vnorm(None, ctypes.byref(a), None, None, ctypes.byref(vn))
    msg = L.rlppo_last_error().decode()
    assert rc == 1001 and "vnorm" in msg and "16-byte aligned" in msg, (rc, msg)
    assert L.rlppo_dbg_counter(2) == passes                                   # refused before a pass was counted
