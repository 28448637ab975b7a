"""rlppo_gae_boot -- the GAE scan with truncated trajectories bootstrapped from V of their own next state -- through the C ABI
and the Python surface, against the CPU oracle applied per trajectory (tests/gae_bootstrap_yardstick.py; tolerance of
test_gae_matches_oracle: rtol 2e-6, atol 2e-6 on all three outputs).  Entries of boot_values at steps that are not
truncated-and-not-done are NaN throughout: they must never be used."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gae_bootstrap_yardstick as Y  # noqa: E402
from hip_pass import L, P, check, dev, stream  # noqa: E402,F401

GAMMA, LMBDA = 0.99, 0.95
CHUNK = 2048
# single ragged chunk | exact chunk | chunk + 1 | n mod 4, 8, 512, 2048 all non-zero | three chunks and a ragged last wave
SIZES = [1, 7, 2047, 2048, 2049, 5003, 3 * 2048 + 300]


@pytest.fixture(params=[1, 0], ids=["lookback", "two_launch"])
def form(L, request):
    check(L, L.rlppo_dbg_set(1, request.param))
    try:
        yield request.param
    finally:
        check(L, L.rlppo_dbg_set(1, 1))


def run(L, rews, dones, trunc, values, boot, std, entry="boot"):
    n = len(rews)
    vt, adv, ret = (torch.full((n,), 7.0, device="cuda") for _ in range(3))
    ws = torch.empty(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    ws[:16] = 0
    r, d, t, v = dev(rews), dev(dones), dev(trunc), dev(values)
    b = None if boot is None else dev(boot)
    s = float("nan") if std is None else float(std)
    if entry == "plain":
        check(L, L.rlppo_gae(stream(), P(r), P(d), P(t), P(v), n, GAMMA, LMBDA, s, P(vt), P(adv), P(ret), P(ws), ws.numel()))
    else:
        check(L, L.rlppo_gae_boot(stream(), P(r), P(d), P(t), P(v), P(b), n, GAMMA, LMBDA, s, P(vt), P(adv), P(ret), P(ws), ws.numel()))
    assert int(ws[4:8].view(torch.int32).item()) == 0, "a look-back wait timed out in a normal run"
    return vt.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy()


@pytest.mark.parametrize("std", [None, 1.3], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("n", SIZES)
def test_gae_boot_matches_per_trajectory_oracle(L, form, n, std):
    rews, dones, trunc, values, boot = Y.make_case(n, seed=n)
    assert np.isnan(boot[n // 2]) or n <= 2                      # the step with both flags holds NaN
    got = run(L, rews, dones, trunc, values, boot, std)
    Y.assert_close(got, Y.per_segment(rews, dones, trunc, values, boot, GAMMA, LMBDA, std), f"n={n}")


@pytest.mark.parametrize("n", [7, 2049, 3 * 2048 + 300])
def test_gae_boot_is_the_plain_scan_when_it_bootstraps_from_the_next_entry(L, form, n):
    """boot_values[t] = values[t + 1] at every truncated step (NaN elsewhere), and boot_values = NULL: rlppo_gae's bits."""
    rews, dones, trunc, values, boot = Y.make_case(n, seed=100 + n)
    idx = Y.boot_steps(dones, trunc)
    boot[idx] = values[idx + 1]
    plain = run(L, rews, dones, trunc, values, None, 1.3, entry="plain")
    for b in (boot, None):
        got = run(L, rews, dones, trunc, values, b, 1.3)
        for x, y in zip(got, plain):
            assert np.array_equal(x, y), ("NULL" if b is None else "values[t+1]", n)


def test_gae_boot_on_more_chunks_than_resident_workgroups(L):
    """A grid beyond the resident workgroups takes the kernel's chunk loop.  One truncated step per 128."""
    n = 1100 * CHUNK + 300                                       # > 4 workgroups x 256 compute units
    rs = np.random.RandomState(11)
    rews, values = rs.randn(n).astype(np.float32), rs.randn(n + 1).astype(np.float32)
    dones, trunc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    trunc[127::128] = 1.0
    boot = np.full(n, np.nan, np.float32)
    boot[127::128] = rs.randn(len(boot[127::128])).astype(np.float32)
    got = run(L, rews, dones, trunc, values, boot, 1.7)
    Y.assert_close(got, Y.per_segment(rews, dones, trunc, values, boot, GAMMA, LMBDA, 1.7), "loop form")


def test_gae_boot_under_graph_capture_replays_correctly(L):
    """Under capture the stateless two-launch form runs; replays on new inputs (new bootstrap values too) give the new outputs."""
    n = 3 * CHUNK + 300
    rews, dones, trunc, values, boot = Y.make_case(n, seed=3)
    vt, adv, ret = (torch.empty(n, device="cuda") for _ in range(3))
    ws = torch.empty(int(L.rlppo_gae_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    r, d, t, v, b = dev(rews), dev(dones), dev(trunc), dev(values), dev(boot)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            check(L, L.rlppo_gae_boot(ctypes.c_void_p(side.cuda_stream), P(r), P(d), P(t), P(v), P(b), n, GAMMA, LMBDA, 1.7,
                                      P(vt), P(adv), P(ret), P(ws), ws.numel()))
    for seed in (3, 4, 5):
        rews, dones, trunc, values, boot = Y.make_case(n, seed=seed)
        r.copy_(dev(rews)); d.copy_(dev(dones)); t.copy_(dev(trunc)); v.copy_(dev(values)); b.copy_(dev(boot))
        g.replay()
        torch.cuda.synchronize()
        Y.assert_close((vt.cpu().numpy(), adv.cpu().numpy(), ret.cpu().numpy()),
                       Y.per_segment(rews, dones, trunc, values, boot, GAMMA, LMBDA, 1.7), f"replay {seed}")


def test_python_surface_and_timeout(L):
    from rlgym_ppo_amd.util import torch_functions as TF
    n = 96 * 256
    rews, dones, trunc, values, boot = Y.make_case(n, seed=9, p_done=0.0, p_trunc=0.0)
    want = Y.per_segment(rews, dones, trunc, values, boot, GAMMA, LMBDA, 1.3)
    vt, adv, ret = TF.compute_gae(rews, dones, trunc, values, GAMMA, LMBDA, 1.3, next_values=boot)
    assert not vt.is_cuda and isinstance(ret, np.ndarray)
    Y.assert_close((vt.numpy(), adv.numpy(), ret), want, "compute_gae")
    args = (dev(rews), dev(dones), dev(trunc), dev(values), GAMMA, LMBDA, 1.3)
    got = TF.gae_device(*args, boot_values=dev(boot))
    Y.assert_close([x.cpu().numpy() for x in got], want, "gae_device")
    plain = TF.gae_device(*args)
    assert not torch.equal(plain[1], got[1]) and torch.equal(plain[2], got[2])    # advantages bootstrapped, returns not
    out = TF.gae_device_deferred(*args, boot_values=dev(boot))
    assert int(out[3].item()) == 0
    Y.assert_close([x.cpu().numpy() for x in out[:3]], want, "gae_device_deferred")
    # a bounded look-back wait that gives up (spin limit 0; long stretches without a trajectory end: chunks must chain) poisons
    # outputs with NaN and counts the event: the bootstrap form reports it like the plain one
    check(L, L.rlppo_dbg_set(21, 0))
    try:
        out = TF.gae_device_deferred(*args, boot_values=dev(boot))
        with pytest.raises(TF.GAETimeout):
            TF.raise_if_timed_out(out[3].item())
        assert np.isnan(out[1].cpu().numpy()).any()
        with pytest.raises(TF.GAETimeout):
            TF.gae_device(*args, boot_values=dev(boot))
        with pytest.raises(TF.GAETimeout):
            TF.compute_gae(rews, dones, trunc, values, GAMMA, LMBDA, 1.3, next_values=boot)
    finally:
        check(L, L.rlppo_dbg_set(21, -1))
    TF.gae_device(*args, boot_values=dev(boot))                  # and the next healthy call is clean again
