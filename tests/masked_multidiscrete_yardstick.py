"""The yardstick of invalid-action masking on the multi-discrete head (include/rlppo.h, "[nvec, masked]"): float64 restated here,
because oracle/ppo.py's analytic multi-discrete path slices by MD_BINS and cannot take a row mask.  Semantics: a mask row has one
entry per logit, [n, S = sum(bins)]; head h owns columns [s_h, s_h + b_h) and is Categorical(logits = z_h with -inf outside its
valid set V_h); a sample is the first arg-max over c in V_h of softmax_V(z_h)_c / q[(row H + h) B + c] (the noise keeps its
[n H, B] shape); log p = sum_h (z[a_h] - lse_V(z_h)); entropy = sum_h -sum_{c in V_h} p_c log p_c; dL/dz = 0 on invalid logits.
The unmasked helpers come from tests/multidiscrete_nvec_yardstick.py."""
import ctypes

import numpy as np
import torch

import fp64_gate
import multidiscrete_nvec_yardstick as Y
from oracle import nets, ppo

CLIP, ENT = 0.2, 0.005


def starts(bins):
    return [int(s) for s in np.cumsum((0,) + tuple(bins))[:-1]]


def rand_mask(rs, n, bins, p=0.6):
    """Every bin valid with probability p and one bin forced valid per head; every 5th row (from 3) all valid; every 7th row: each
    head keeps exactly one valid bin; row 0: exactly the last bin of every head (so the last bin of the last head stands alone)."""
    S = sum(bins)
    m = rs.rand(n, S) < p
    one = np.zeros((n, S), bool)
    for s, b in zip(starts(bins), bins):
        pick = s + rs.randint(0, b, n)
        m[np.arange(n), pick] = True
        one[np.arange(n), pick] = True
    m[0::7] = one[0::7]
    m[3::5] = True
    m[0] = False
    for s, b in zip(starts(bins), bins):
        m[0, s + b - 1] = True
    return m


def head_valid(mask, bins):
    """bool [n, S] -> [n, H, B], False in the padded slots."""
    n, H, B = mask.shape[0], len(bins), max(bins)
    out = np.zeros((n, H, B), bool)
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        out[:, h, :b] = mask[:, s:s + b]
    return out


def masked_sample64(z, bins, q, mask):
    """Y.sample64 with -inf scores at invalid bins: float64 logits [n, S], noise [n H, B], bool mask [n, S] (every head >= 1 valid) ->
    (actions [n, H], logp [n], score [n, H, B], near [n, H])."""
    n, H, B = z.shape[0], len(bins), max(bins)
    q = np.asarray(q, np.float64).reshape(n, H, B)
    zz = np.where(mask, np.asarray(z, np.float64), -np.inf)
    v3 = head_valid(np.asarray(mask, bool), bins)
    assert v3.any(-1).all(), "every head of every row needs a valid bin"
    act, logp, score = np.zeros((n, H), np.int64), np.zeros(n), np.full((n, H, B), -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        lss = Y.head_log_softmax64(zz, bins)
    for h, ls in enumerate(lss):
        b = bins[h]
        score[:, h, :b] = np.where(v3[:, h, :b], np.exp(ls) / q[:, h, :b], -np.inf)
        act[:, h] = score[:, h, :b].argmax(-1)
        logp += ls[np.arange(n), act[:, h]]
    if B > 1:
        top = np.sort(score, -1)
        with np.errstate(invalid="ignore"):
            near = (top[..., -1] - top[..., -2]) <= Y.NEAR_TIE * top[..., -1]   # (one valid bin: -inf second, never near)
    else:
        near = np.zeros((n, H), bool)
    return act, logp, score, near


def check_sampled(act, logp, z64, bins, q, mask, max_rows=2):
    """Y.check_sampled's rules with the mask added: at most `max_rows` near-ties in the inputs (asserted first, from the float64
    reference alone); no sampled action invalid; indices equal except at near-ties; log p of agreeing rows within 1e-5."""
    oact, ologp, score, near = masked_sample64(z64, bins, q, mask)
    assert int(near.sum()) <= max_rows, ("the inputs hold too many near-ties", int(near.sum()))
    act = np.asarray(act)
    assert act.shape == oact.shape and (act >= 0).all() and (act < np.asarray(bins)[None, :]).all()
    v3 = head_valid(np.asarray(mask, bool), bins)
    assert np.take_along_axis(v3, act[..., None], -1).all(), "an invalid action was sampled"
    for r, h in np.argwhere(act != oact).tolist():
        s = score[r, h]
        assert abs(s[act[r, h]] - s[oact[r, h]]) <= Y.NEAR_TIE * s[oact[r, h]], ("index mismatch that is not a near-tie", r, h)
    same = (act == oact).all(1)
    assert same.sum() >= len(same) - max_rows
    err = float(np.abs(np.asarray(logp, np.float64)[same] - ologp[same]).max())
    print(f"[masked nvec] bins {tuple(bins) if len(bins) <= 8 else (bins[0], '...', len(bins))}: {int((~same).sum())} rows differ, "
          f"{int(near.sum())} near-ties, max |logp - fp64| = {err:.2e}")
    assert err < 1e-5, err
    return oact, ologp


def masked_logp64(z, bins, acts, mask):
    """float64 log p [n] of stored actions [n, H] under the mask (actions valid)."""
    zz = np.where(mask, np.asarray(z, np.float64), -np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        lss = Y.head_log_softmax64(zz, bins)
    n = z.shape[0]
    return sum(ls[np.arange(n), np.asarray(acts)[:, h].astype(int)] for h, ls in enumerate(lss))


def masked_chain(pol, val, obs, acts, old, adv, tgt, mask, bins, mb_ratio, dtype, mp=None, mv=None):
    """The masked update in torch autograd, float64 (under imposed ReLU decisions mp / mv) or float32 (the CPU restatement, its own
    decisions): per head lse over the valid bins, log p = sum_h (z[a_h] - lse_V), entropy over the valid bins.  A stored action its
    mask marks invalid contributes the literal value and no gradient through its own logit (its one-hot is dropped).
    -> (grad_policy, grad_value, [entropy, kl, vloss, clipfrac, ploss], ratio)."""
    T = lambda x: torch.as_tensor(np.asarray(x), dtype=dtype)
    Pp = [(T(w).requires_grad_(), T(b).requires_grad_()) for w, b in pol]
    Vp = [(T(w).requires_grad_(), T(b).requires_grad_()) for w, b in val]

    def fwd(ps, masks):
        h = T(obs)
        for l, (w, b) in enumerate(ps[:-1]):
            pre = torch.nn.functional.linear(h, w, b)
            h = torch.relu(pre) if masks is None else pre * T(masks[l])
        return torch.nn.functional.linear(h, *ps[-1])

    m = torch.as_tensor(np.asarray(mask, bool))
    a = torch.as_tensor(np.asarray(acts)).long().view(m.shape[0], len(bins))
    z = fwd(Pp, mp)
    logp, entropy = 0.0, 0.0
    for h, (s, b) in enumerate(zip(starts(bins), bins)):
        zh, mh = z[:, s:s + b], m[:, s:s + b]
        lse = torch.logsumexp(zh.masked_fill(~mh, float("-inf")), -1, keepdim=True)
        ls = zh - lse                                                    # finite everywhere; only the valid entries are used
        p = torch.where(mh, torch.exp(ls), torch.zeros_like(ls))
        entropy = entropy - (p * torch.where(mh, ls, torch.zeros_like(ls))).sum(-1)
        ah = a[:, h:h + 1]
        za = zh.gather(1, ah)
        za = torch.where(mh.gather(1, ah), za, za.detach())
        logp = logp + (za - lse).view(-1)
    entropy = entropy.mean()
    lr = logp - T(old)
    ratio = torch.exp(lr)
    A = T(adv)
    ploss = -torch.min(ratio * A, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * A).mean()
    vloss = ((fwd(Vp, mv).view(-1) - T(tgt)) ** 2).mean()
    ((ploss - entropy * ENT) * mb_ratio).backward()
    (vloss * mb_ratio).backward()
    g = lambda ps: [(w.grad.detach().numpy().astype(np.float64), b.grad.detach().numpy().astype(np.float64)) for w, b in ps]
    stats = [float(x.detach()) for x in (entropy, ((ratio - 1) - lr).mean(), vloss, ((ratio - 1).abs() > CLIP).double().mean(), ploss)]
    return g(Pp), g(Vp), stats, ratio.detach().numpy().astype(np.float64)


def masked_gate(L, monkeypatch, bins, pol, val, pr, got, label, mb_ratio=1.0):
    """The rule of tests/test_gpu_action_mask.py::masked_gate: err(HIP, fp64 under the HIP's ReLU decisions) <= max(1e-5, 1.5 x
    err(float32 torch restatement, fp64 under its own)), for the gradients and for the five statistics; both printed.  pr: the rows
    of the pass (obs, acts [n, H], old, adv, tgt, mask [n, S]); got = (grad_policy, grad_value, stats or None)."""
    gp, gv, stats = got
    args = (pr["obs"], pr["acts"], pr["old"], pr["adv"], pr["tgt"], pr["mask"], bins, mb_ratio)
    det = {}
    Y.patch_oracle(monkeypatch, bins)   # (the hidden layers know no mask: their float64 pre-activations and rounding scales)
    ppo.minibatch_analytic("multidiscrete", pol, val, pr["obs"], pr["acts"], pr["old"], pr["adv"], pr["tgt"], CLIP, ENT, mb_ratio, (0.1, 1.0),
                           detail=det)
    cp, cv, cstats, _ = masked_chain(pol, val, *args, torch.float32)
    res = {}
    for who, g_p, g_v, st, mp, mv in (("hip", gp, gv, stats, fp64_gate.hip_masks(L, pol, pr["obs"]), fp64_gate.hip_masks(L, val, pr["obs"])),
                                      ("cpu", cp, cv, cstats, fp64_gate.cpu_masks(pol, pr["obs"]), fp64_gate.cpu_masks(val, pr["obs"]))):
        flips = fp64_gate._check_flips(pol, mp, det["pol"], who) + fp64_gate._check_flips(val, mv, det["val"], who)
        tp, tv, tstats, _ = masked_chain(pol, val, *args, torch.float64, mp, mv)
        err = fp64_gate.grads_err(list(g_p) + list(g_v), tp + tv)
        serr = None if st is None else [abs(float(st[k]) - tstats[k]) / max(abs(tstats[k]), 1e-12) for k in range(5)]
        res[who] = (err, serr, flips)
    print(f"[masked nvec fp64 gate] {label}: err(HIP, fp64)={res['hip'][0]:.2e}  err(CPU fp32, fp64)={res['cpu'][0]:.2e}  ReLU flips HIP "
          f"{res['hip'][2]} / CPU {res['cpu'][2]}  stats (entropy, kl, vloss, clipfrac, ploss) HIP {res['hip'][1]} CPU {res['cpu'][1]}")
    assert res["hip"][0] <= max(1e-5, 1.5 * res["cpu"][0]), (label, res["hip"][0], res["cpu"][0])
    if res["hip"][1] is not None:
        for k in range(5):
            assert res["hip"][1][k] <= max(1e-5, 1.5 * res["cpu"][1][k]), (label, "statistic", k, res["hip"][1][k], res["cpu"][1][k])
    return res


def away_from_clip_edges(rs, n, scale):
    """d ~ N(0, scale^2), redrawn while exp(d) lies within 1e-3 of a clip edge: no float32 rounding decides a row's surrogate branch."""
    d = scale * rs.randn(n)
    while True:
        bad = np.minimum(np.abs(np.exp(d) - (1 - CLIP)), np.abs(np.exp(d) - (1 + CLIP))) < 1e-3
        if not bad.any():
            return d
        d[bad] = scale * rs.randn(int(bad.sum()))


def make_problem(bins, seed, n, d=107, hidden=(128, 128), saturate=False, mask_fn=None):
    """Policy + critic and an n-row buffer: random per-row masks (rand_mask, or mask_fn(obs)), actions the float64 yardstick sampled
    under them, old log-probabilities = the float64 masked log p minus d with d ~ N(0, 0.2^2) kept 1e-3 away from both clip edges
    (so both edges are crossed and no row sits on one).  saturate: logits scaled to +-30; a third of the rows carry uniformly drawn
    VALID actions with old log-probabilities 0.5 off either way (tests/test_gpu_multidiscrete_nvec.py::update_case)."""
    torch.manual_seed(seed)
    rs = np.random.RandomState(seed)
    H, S = len(bins), sum(bins)
    pol, val = nets.init_mlp(d, hidden, S), nets.init_mlp(d, hidden, 1)
    obs = np.clip(rs.randn(n, d), -5, 5).astype(np.float32)
    if saturate:
        with torch.no_grad():
            s = 30.0 / nets.mlp(pol, obs).abs().max().item()
        pol = pol[:-1] + [(pol[-1][0] * s, pol[-1][1] * s)]
    mask = rand_mask(rs, n, bins) if mask_fn is None else mask_fn(obs)
    z = Y.logits64(pol, obs)
    act, logp, _, _ = masked_sample64(z, bins, nets.draw_exp_noise(n * H, max(bins)).numpy(), mask)
    off = away_from_clip_edges(rs, n, 0.2)
    if saturate:
        third = n // 3
        v3 = head_valid(mask, bins)
        for r in range(third):
            for h in range(H):
                act[r, h] = rs.choice(np.flatnonzero(v3[r, h]))
        logp = masked_logp64(z, bins, act, mask)
        off[:third] = np.where(rs.rand(third) < 0.5, -0.5, 0.5)
    old = (logp - off).astype(np.float32)
    pr = dict(obs=obs, mask=mask, acts=act.astype(np.float32), old=old, adv=rs.randn(n).astype(np.float32),
              tgt=rs.randn(n).astype(np.float32), logp=logp)
    return pol, val, pr, rs


def rows(pr, idx):
    """The rows of a pass: the problem's fields gathered by idx."""
    return {k: np.asarray(v)[idx] for k, v in pr.items()}


def act_nvec(L, net, bins, padded_rows, n, q, mask=None):
    """rlppo_multidiscrete_act_nvec (mask None) or rlppo_multidiscrete_act_nvec_masked (mask: bool [n, S]) on padded device rows ->
    (actions, logp) as numpy; counter 6 must advance by one."""
    from rlgym_ppo_amd.util import action_mask as AM
    from test_gpu_kernels import P, check, dev, stream
    act = torch.full((n, len(bins)), -7, dtype=torch.int64, device="cuda")
    logp = torch.empty(n, device="cuda")
    w = net.ws(n)
    qd = q if isinstance(q, torch.Tensor) and q.is_cuda else dev(q)
    words = None if mask is None else AM.pack(mask, sum(bins), "cuda", heads=bins)
    c6 = L.rlppo_dbg_counter(6)
    args = (stream(), net.dims_c, net.nl, P(net.packed), P(padded_rows), net.ld_in, n, P(qd), P(act), P(logp), P(w), w.numel(), None,
            Y.nvec_array(bins), len(bins))
    if words is None:
        check(L, L.rlppo_multidiscrete_act_nvec(*args))
    else:
        check(L, L.rlppo_multidiscrete_act_nvec_masked(*args, P(words), words.shape[1]))
    torch.cuda.synchronize()
    assert L.rlppo_dbg_counter(6) == c6 + 1   # the general kernel ran
    return act.cpu().numpy(), logp.cpu().numpy()


def run_minibatch(L, bins, pol, val, pr, idx, mb_ratio, mask=True, ring=None):
    """One pass of rlppo_ppo_minibatch_nvec (md_nvec given) over rows idx of the problem's buffer, the buffer's mask field given
    (mask=True: pr["mask"]; an array: that mask; None: no mask), over a workspace prefilled with NaN bit patterns.
    -> (grad_policy, grad_value, stats, dz): dz = the policy's output buffer [mb][padded S] after the pass (the loss kernel's in-place
    gradient), as Y.run_minibatch_nvec returns it."""
    from rlgym_ppo_amd import _native as N
    from rlgym_ppo_amd.util import action_mask as AM
    from test_gpu_kernels import Net, check, dev, stream
    n = pr["obs"].shape[0]
    fields = [pr["obs"], pr["acts"], pr["old"], pr["tgt"], pr["adv"]]
    m = pr["mask"] if mask is True else mask
    if ring is not None:
        fields = [np.roll(np.asarray(x), ring, axis=0) for x in fields]
        m = None if m is None else np.roll(np.asarray(m), ring, axis=0)
    obs_all, acts_all, old_all, tgt_all, adv_all = fields
    P_, V_ = Net(L, pol), Net(L, val)
    states = P_.pad(obs_all)
    acts = dev(np.asarray(acts_all, np.float32).reshape(n, -1))
    a = N.MinibatchArgs()
    a.head, a.pol_layers, a.val_layers, a.act_dim = N.HEAD_MULTIDISCRETE, P_.nl, V_.nl, acts.shape[1]
    a.pol_dims = ctypes.cast(P_.dims_c, ctypes.POINTER(ctypes.c_int32))
    a.val_dims = ctypes.cast(V_.dims_c, ctypes.POINTER(ctypes.c_int32))
    gp, gv = torch.zeros_like(P_.flat), torch.zeros_like(V_.flat)
    old, tgt, adv = dev(old_all), dev(tgt_all), dev(adv_all)
    idxd = dev(idx, torch.int64)
    stats = torch.zeros(8, dtype=torch.float64, device="cuda")
    mb = len(idx)
    ws_bytes = int(L.rlppo_minibatch_workspace_bytes(P_.dims_c, P_.nl, V_.dims_c, V_.nl, mb))
    ws = torch.full(((ws_bytes + 3) // 4,), -1, dtype=torch.int32, device="cuda")   # 0xFFFFFFFF: a NaN in every float
    a.pol_packed, a.val_packed, a.pol_grad, a.val_grad = P_.packed.data_ptr(), V_.packed.data_ptr(), gp.data_ptr(), gv.data_ptr()
    a.states, a.ld_states, a.n_rows, a.actions = states.data_ptr(), states.shape[1], states.shape[0], acts.data_ptr()
    a.old_logp, a.targets, a.advantages, a.idx, a.mb = old.data_ptr(), tgt.data_ptr(), adv.data_ptr(), idxd.data_ptr(), mb
    if ring is not None:
        a.ring_base, a.ring_cap = ring, n
    a.clip_range, a.ent_coef, a.mb_ratio = CLIP, ENT, mb_ratio
    a.stats, a.workspace, a.ws_bytes = stats.data_ptr(), ws.data_ptr(), ws_bytes
    words = None
    if m is not None:
        words = AM.pack(np.asarray(m), sum(bins), "cuda")   # (no per-head check: the caller-error cases go through here too)
        a.action_mask, a.mask_words = words.data_ptr(), words.shape[1]
    check(L, L.rlppo_ppo_minibatch_nvec(stream(), ctypes.byref(a), Y.nvec_array(bins), len(bins)))
    torch.cuda.synchronize()
    before = sum(int(L.rlppo_padded_out(d)) for d in P_.dims[1:-1])   # the hidden layers' outputs lie in front of the head's
    dz = ws.view(torch.float32)[mb * before: mb * (before + P_.ld_out)].view(mb, P_.ld_out).cpu().numpy()
    return nets.unflatten(gp.cpu(), pol), nets.unflatten(gv.cpu(), val), stats.cpu().numpy(), dz
