"""Every hidden-layer option through the two entry points that take them all, in one place: one rlppo_mlp_forward_res call and one
rlppo_ppo_minibatch_ex pass of a policy 13 -> w -> w -> w -> 5 and a critic 13 -> w -> w -> w -> 1 on 37 rows, for {relu, tanh, elu} x
{norm off, on} x {residual off, on}.  w = 24: a padded width that is no power of two, 16 lanes per row, 37 rows leave the third workgroup
of 16 rows ragged; w = 300: a row held by a whole wave with two chunks per lane, the second partial.  Every instantiation family the
row kernels' shape dispatcher (csrc/norm_rows.hpp: with_row_shape / with_hidden_act) selects from runs here.

The truth is the torch body build_body makes, in float64; the allowance is test_gpu_layer_norm.within's: 4 x the error of the same body in
float32, with a floor of 4 ulp of the tensor's scale.  A ReLU case is made to keep every hidden pre-activation of the float64 run 1e-4 from
zero, the rule the norm and residual tests compare a ReLU gradient under (case())."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ppo_yardstick as A
from hip_pass import L, Net, P, run_pass, stream  # noqa: F401 -- L is the fixture
from test_gpu_layer_norm import ACTS, A_CODE, within

pytestmark = pytest.mark.gpu
OBS, ROWS, ACTIONS, CLIP, ENT = 13, 37, 5, 0.2, 0.005


def nearest_units(body, obs):
    """The float64 run of a body -> per hidden Linear the smallest |pre-activation| of each of its units over the rows."""
    body, seen = copy.deepcopy(body).double(), []
    hidden = [m for m in body if isinstance(m, torch.nn.Linear)][:-1]
    for lin in hidden:
        lin.register_forward_hook(lambda mod, i, o: seen.append(o.detach().abs().amin(0)))
    with torch.no_grad():
        body(torch.as_tensor(obs).double())
    return seen


def case(act, norm, res, width, seed=0):
    """The two bodies and 37 rows of made-up experience.  ReLU: no seed keeps the 66,600 hidden pre-activations of width 300 away from
    zero, so the case is MADE to have the property a ReLU gradient is compared under -- the bias of every hidden unit with a
    pre-activation within 2e-4 of zero in the float64 run moves by 1e-3, first layer first, until no pre-activation lies within 1e-4
    (asserted).  The weights stay what torch's initialisation drew; the networks are as valid as any."""
    from rlgym_ppo_amd.ppo import LayerSizes
    from rlgym_ppo_amd.ppo._mlp import build_body
    torch.manual_seed(seed)
    sizes = LayerSizes((width,) * 3, act, "layer" if norm else None, None, res)
    pol, val = build_body(OBS, sizes, ACTIONS), build_body(OBS, sizes, 1, critic=True)
    rs = np.random.RandomState(seed)
    data = dict(obs=np.clip(rs.randn(ROWS, OBS), -5, 5).astype(np.float32), acts=rs.randint(0, ACTIONS, (ROWS, 1)).astype(np.float32),
                old=(-np.log(ACTIONS) + 0.1 * rs.randn(ROWS)).astype(np.float32), tgt=1 + rs.randn(ROWS).astype(np.float32),
                adv=rs.randn(ROWS).astype(np.float32))
    if act == "relu":
        for body in (pol, val):
            hidden = [m for m in body if isinstance(m, torch.nn.Linear)][:-1]
            for _ in range(100):
                close = [near < 2e-4 for near in nearest_units(body, data["obs"])]
                first = next((l for l, c in enumerate(close) if c.any()), None)
                if first is None:
                    break
                with torch.no_grad():
                    hidden[first].bias[close[first]] += 1e-3
            nearest = min(float(near.min()) for near in nearest_units(body, data["obs"]))
            assert nearest > 1e-4, f"a ReLU pre-activation of the float64 run lies {nearest:.1e} from zero"
    return pol, val, data


def restate(pol, val, data, dtype):
    """-> (the policy's logits [37, 5], the gradients of one PPO minibatch per layer (dW, db): the policy's, the critic's)."""
    pol, val = copy.deepcopy(pol).to(dtype), copy.deepcopy(val).to(dtype)
    t = {k: torch.as_tensor(v).to(dtype) for k, v in data.items()}
    z, v = pol(t["obs"]), val(t["obs"])
    logp, entropy = A.head_terms("discrete", z, t["acts"])
    ratio = torch.exp(logp - t["old"])
    (-torch.min(ratio * t["adv"], torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * t["adv"]).mean() - entropy * ENT).backward()
    F.mse_loss(v.view(-1), t["tgt"]).backward()
    layers = lambda m: [(lin.weight.grad, lin.bias.grad) for lin in m if isinstance(lin, torch.nn.Linear)]
    return z.detach(), layers(pol), layers(val)


@pytest.mark.parametrize("res", [False, True], ids=["chain", "res"])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("width", [24, 300])
def test_forward_and_pass_against_float64(L, width, act, norm, res):
    from rlgym_ppo_amd import _native as N
    pol, val, data = case(act, norm, res, width)
    code = A_CODE[act] | (N.ACT_NORM if norm else 0) | (N.ACT_RES if res else 0)
    label = f"w={width} {act} norm={norm} res={res}"
    params = lambda m: [(lin.weight.detach().clone(), lin.bias.detach().clone()) for lin in m if isinstance(lin, torch.nn.Linear)]
    (z64, gp64, gv64), (z32, gp32, gv32) = restate(pol, val, data, torch.float64), restate(pol, val, data, torch.float32)

    # one rlppo_mlp_forward_res call: NaN in the output buffer, rows beyond the call's untouched
    net = Net(L, params(pol))
    rows = net.pad(data["obs"])
    ws = torch.empty(int(L.rlppo_forward_workspace_bytes_act(net.dims_c, net.nl, ROWS, code)), dtype=torch.uint8, device="cuda")
    out = torch.full((ROWS + 3, net.ld_out), float("nan"), device="cuda")
    out[ROWS:] = 5.0
    opts = N.ActOpts()
    opts.hidden_act = code
    assert L.rlppo_mlp_forward_res(stream(), net.dims_c, net.nl, P(net.packed), P(rows), net.ld_in, ROWS, 0, P(out), net.ld_out, P(ws), ws.numel(),
                                   ctypes.byref(opts)) == 0, L.rlppo_last_error()
    got = out.cpu()
    assert (got[ROWS:] == 5.0).all(), "rows at and beyond n were touched"
    within(got[:ROWS, :ACTIONS], z64, z32, z64.abs().max(), f"forward {label}")

    # one rlppo_ppo_minibatch_ex pass over the 37 rows, its workspace NaN-filled and guarded (run_pass)
    r = run_pass(L, params(pol), params(val), data["obs"], data["acts"], data["old"], data["tgt"], data["adv"], np.arange(ROWS), head="discrete",
                 entry="ex", clip=CLIP, ent=ENT, pol_act=code, val_act=code, precision="fp32",
                 ws_fn=lambda *a: L.rlppo_minibatch_workspace_bytes_res(*a, 0, code, code))
    for who, got_layers, l64, l32 in (("policy", r["layers"][0], gp64, gp32), ("critic", r["layers"][1], gv64, gv32)):
        for l, (g, a, b) in enumerate(zip(got_layers, l64, l32)):
            for part, gi, ai, bi in (("dW", g[0], a[0], b[0]), ("db", g[1], a[1], b[1])):
                within(gi, ai, bi, ai.abs().max(), f"{who} layer {l} {part} {label}")
