"""PopArt's weight-preserving step without a GPU: the yardstick's rescale preserves sigma v^ + mu, the Python surface and its two
refusals, the added entry point's ctypes signature against the header and its argument errors (1001, a message naming the argument,
before any launch -- the host never dereferences the device pointers, so placeholders do)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import popart_yardstick as PY
import value_norm_yardstick as VY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_float64_rescale_preserves_the_real_unit_output_over_three_updates():
    """The contract's formulas in float64 (no rounding of w', b', no float32 scale): sigma_1 v^' + mu_1 == sigma_0 v^ + mu_0 to 1e-12."""
    rs = np.random.RandomState(0)
    K, n = 257, 48
    w, b, h = rs.randn(K) / np.sqrt(K), 0.3, np.abs(rs.randn(n, K))
    state, scale = (0.0, 0.0, 0.0), VY.scale64((0.0, 0.0, 0.0))
    V_first = (h @ w + b) * scale[2] + scale[0]
    for k, (mean, dev_) in enumerate(((50.0, 7.0), (-300.0, 0.02), (4e4, 900.0))):
        state = VY.update(state, (mean + dev_ * rs.randn(1000 + k)).astype(np.float32))
        new = VY.scale64(state)
        V0 = (h @ w + b) * scale[2] + scale[0]
        r = scale[2] / new[2]
        w, b = w * r, (b * scale[2] + (scale[0] - new[0])) / new[2]
        V1 = (h @ w + b) * new[2] + new[0]
        assert np.abs(V1 - V0).max() <= 1e-12 * np.abs(V0).max(), (k, np.abs(V1 - V0).max())
        assert abs(new[2] - scale[2]) > 0.5 * abs(scale[2]) or abs(new[0] - scale[0]) > 1.0          # (the statistic did move)
        scale = new
    assert np.abs(V1 - V_first).max() <= 3e-12 * np.abs(V_first).max()


def test_float32_rescale_stays_inside_its_allowance_and_no_rescale_misses_it_a_thousandfold():
    """The yardstick on the CPU, the case the GPU test runs: targets of mean 50 and deviation 7 against a fresh statistic.  The float32
    w', b' with float64 forwards use a small part of the allowance; the SAME update without the rescale misses it by far more than 1000."""
    rs = np.random.RandomState(1)
    for K in (64, 256):
        n = 48
        w, b = (rs.randn(K) / np.sqrt(K)).astype(np.float32), np.float32(0.1)
        h = np.maximum(rs.randn(n, K), 0.0).astype(np.float32)
        s0 = VY.scale32((0.0, 0.0, 0.0))
        s1 = VY.scale32(VY.update((0.0, 0.0, 0.0), (50.0 + 7.0 * rs.randn(3000)).astype(np.float32)))
        w2, b2 = PY.rescale(w, b, s0, s1)
        assert w2.dtype == np.float32 and np.array_equal(w2, (w.astype(np.float64) * (np.float64(s0[2]) / np.float64(s1[2]))).astype(np.float32))
        allow = PY.allowance(w, b, w2, b2, h, s0, s1)
        V0 = PY.real_units(PY.head64(w, b, h)[0], s0)
        V1 = PY.real_units(PY.head64(w2, b2, h)[0], s1)
        moved = PY.real_units(PY.head64(w, b, h)[0], s1)
        kept, missed = (np.abs(V1 - V0) / allow).max(), (np.abs(moved - V0) / allow).min()
        print(f"[popart yardstick] K={K}: with the rescale {kept:.3f} of the allowance, without it {missed:.3g} times the allowance")
        assert kept <= 1.0 and missed >= 1000.0, (K, kept, missed)


def test_python_surface_and_its_refusals():
    from rlgym_ppo_amd import Learner
    from rlgym_ppo_amd.ppo import PPOLearner, ValueNorm
    p = inspect.signature(Learner.__init__).parameters["ppo_value_norm_popart"]
    assert p.default is False
    assert list(inspect.signature(PPOLearner.__init__).parameters)[-1] == "max_grad_norm"
    sig = inspect.signature(PPOLearner.set_value_normalization).parameters
    assert sig["on"].default is True and sig["preserve_outputs"].default is False
    assert inspect.signature(ValueNorm.update).parameters["preserve"].default is None
    assert callable(PPOLearner.update_value_norm)
    # ppo_value_norm_popart without ppo_normalize_value: refused before anything is built (the factory is never called)
    def factory():
        raise AssertionError("the environment was built")
    with pytest.raises(ValueError, match="ppo_normalize_value"):
        Learner(factory, ppo_value_norm_popart=True)
    with pytest.raises(ValueError, match="ppo_normalize_value"):
        Learner(factory, ppo_value_norm_popart=True, ppo_normalize_value=False)
    # preserve_outputs=True with on=False: refused before the learner's state is read
    with pytest.raises(ValueError, match="preserve_outputs"):
        PPOLearner.set_value_normalization(object.__new__(PPOLearner), on=False, preserve_outputs=True)


def test_ctypes_signature_matches_the_header():
    from rlgym_ppo_amd import _native as N
    src = open(os.path.join(ROOT, "include", "rlppo.h")).read()
    m = re.search(r"\bint\s+rlppo_value_norm_update_popart\s*\(([^)]*)\)\s*;", src)
    assert m, "include/rlppo.h does not declare rlppo_value_norm_update_popart"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["void *stream", "const float *targets", "int64_t n", "double *state", "float *scale", "void *ws", "float *w_last",
                      "int64_t n_w", "float *b_last"]
    want = [ctypes.c_void_p if "*" in p else {"int64_t": ctypes.c_int64}[p.split()[0]] for p in params]
    assert N.SIGNATURES["rlppo_value_norm_update_popart"] == (ctypes.c_int32, want)
    plain = N.SIGNATURES["rlppo_value_norm_update"]
    assert N.SIGNATURES["rlppo_value_norm_update_popart"][1][:len(plain[1])] == plain[1]
    L = N.lib()
    assert L.rlppo_value_norm_update_popart.argtypes == want and L.rlppo_abi_version() == N.ABI_VERSION == 8


def test_popart_update_rejects_bad_arguments_before_any_launch():
    from rlgym_ppo_amd import _native as N
    L = N.lib()
    targets, state, scale, ws, w, b = 0x10000, 0x20000, 0x30000, 0x40000, 0x50004, 0x5000c   # distinct, aligned, never dereferenced
    call = lambda *a: (L.rlppo_value_norm_update_popart(None, *a), L.rlppo_last_error().decode())
    # exactly one of the two layer pointers
    rc, msg = call(targets, 100, state, scale, ws, w, 64, None)
    assert rc == 1001 and "b_last" in msg and "NULL" in msg, (rc, msg)
    rc, msg = call(targets, 100, state, scale, ws, None, 64, b)
    assert rc == 1001 and "w_last" in msg and "NULL" in msg, (rc, msg)
    # n_w < 1 with weights given
    for n_w in (0, -3):
        rc, msg = call(targets, 100, state, scale, ws, w, n_w, b)
        assert rc == 1001 and f"n_w={n_w}" in msg, (rc, msg)
    # misaligned layer pointers
    rc, msg = call(targets, 100, state, scale, ws, w + 2, 64, b)
    assert rc == 1001 and "w_last" in msg and "aligned" in msg, (rc, msg)
    rc, msg = call(targets, 100, state, scale, ws, w, 64, b + 1)
    assert rc == 1001 and "b_last" in msg and "aligned" in msg, (rc, msg)
    # the plain entry's rules stand in front, with the layer given and without it (both NULL: the plain entry itself)
    for layer in ((w, 64, b), (None, 0, None)):
        rc, msg = call(targets, 0, state, scale, ws, *layer)
        assert rc == 1001 and "n=0" in msg, (layer, rc, msg)
        rc, msg = call(targets, -5, state, scale, ws, *layer)
        assert rc == 1001 and "n=-5" in msg, (layer, rc, msg)
        for args, word in (((None, 100, state, scale, ws), "targets"), ((targets, 100, None, scale, ws), "state"),
                           ((targets, 100, state, None, ws), "scale"), ((targets, 100, state, scale, None), "ws"),
                           ((targets, 100, state + 4, scale, ws), "state"), ((targets, 100, state, scale + 8, ws), "scale"),
                           ((targets + 2, 100, state, scale, ws), "targets"), ((targets, 100, state, scale, ws + 4), "ws")):
            rc, msg = call(*args, *layer)
            assert rc == 1001 and word in msg, (args, layer, rc, msg)
