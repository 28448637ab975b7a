"""The yardstick of invalid-action masking on the multi-discrete head (include/rlppo.h, "[nvec, masked]"): float64 restated here,
because oracle/ppo.py's analytic multi-discrete path slices by MD_BINS and cannot take a row mask.  Semantics: a mask row has one
entry per logit, [n, S = sum(bins)]; head h owns columns [s_h, s_h + b_h) and is Categorical(logits = z_h with -inf outside its
valid set V_h); a sample is the first arg-max over c in V_h of softmax_V(z_h)_c / q[(row H + h) B + c] (the noise keeps its
[n H, B] shape); log p = sum_h (z[a_h] - lse_V(z_h)); entropy = sum_h -sum_{c in V_h} p_c log p_c; dL/dz = 0 on invalid logits.
The unmasked helpers come from tests/multidiscrete_nvec_yardstick.py."""
import numpy as np
import torch

import multidiscrete_nvec_yardstick as Y
from oracle import nets
from ppo_yardstick import CLIP, ENT, starts

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


def pass_args(pr, bins, mask=True):
    """A problem's buffer as hip_pass.run_pass takes it, for rlppo_ppo_minibatch_nvec with md_nvec given: (the five row arrays,
    keywords).  mask=True: pr["mask"]; an array: that mask; None: no mask.  (No per-head check when the mask is packed: the
    caller-error cases go through here too.)  dz: the pass returns the policy's output buffer, the loss kernel's in-place gradient."""
    kw = dict(head="nvec", entry="nvec", bins=bins, clip=CLIP, ent=ENT, mask=pr["mask"] if mask is True else mask, dz=True)
    return (pr["obs"], pr["acts"], pr["old"], pr["tgt"], pr["adv"]), kw


def act_nvec(L, net, bins, padded_rows, n, q, mask=None):
    """rlppo_multidiscrete_act_nvec (mask None) or rlppo_multidiscrete_act_nvec_masked (mask: bool [n, S]) on padded device rows ->
    (actions, logp) as numpy; counter 6 must advance by one."""
    from rlgym_ppo_amd.util import action_mask as AM
    from hip_pass import P, check, dev, stream
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
