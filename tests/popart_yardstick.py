"""The yardstick of PopArt's weight-preserving step (rlppo_value_norm_update_popart; the contract is in include/rlppo.h, "[vnorm]"):
plain numpy float64, no import of the product.  The statistic itself is tests/value_norm_yardstick.py's.

  * rescale(): the expected last layer after a move of the published scale from {mu_0, ., sigma_0, .} to {mu_1, ., sigma_1, .}, the
    four numbers taken AS FLOATS (what the scan and the loss read) and widened to double:
        r = sigma_0 / sigma_1;   w'_i = fl32(w_i r);   b' = fl32(fma(b, sigma_0, mu_0 - mu_1) / sigma_1)
    Every step is one IEEE operation in double, so w' is the kernel's bit for bit.  numpy has no fma: b' is formed exactly (rational
    arithmetic) and rounded once where the kernel rounds, which is what an fma does.
  * allowance(): how far the critic's real-unit output V = fmaf(v^, sigma, mu) may move across the step.  Derived, not tuned; per row,
    with u = 2^-24, K = n_w, h the last hidden activations, S = sum|w_i h_i| and S' = sum|w'_i h_i|:
      - in exact arithmetic sigma_1 (w r . h + b_x) + mu_1 = sigma_0 (w . h + b) + mu_0 with b_x = (sigma_0 b + mu_0 - mu_1) / sigma_1.
        The one rounding of each w'_i moves w'_i by u |w_i r|, the output by sigma_1 u sum|w_i r h_i| = u sigma_0 S; the one rounding
        of b' moves it by u |b_x|, the output by sigma_1 u |b_x| = u |sigma_0 b + mu_0 - mu_1|:
                                            u (sigma_0 S + |sigma_0 b + mu_0 - mu_1|)
        (r and the double operations round at 2^-53: nothing at this scale);
      - each of the two float32 forwards of the head is a product of K + 1 terms: the allowance tests/gemm_yardstick.py gives it,
        nt_allow = (K + 8) u (S + |b|), in normalised units, so scaled by sigma_0 before the step and by sigma_1 (with S', b') after;
      - each final fmaf rounds once: u (|V_0| + |V_1|).
    The hidden layers are the same launches on the same rows and weights before and after: h is the same bits and adds nothing."""
from fractions import Fraction

import numpy as np

import gemm_yardstick as GY
import value_norm_yardstick as VY  # noqa: F401  (the statistic: callers advance it with VY.update / VY.scale32)

U = GY.U32


def rescale(w, b, scale0, scale1):
    """(w', b') as float32 for last-layer weights w (any shape), bias b and the published float32 scales before / after."""
    s0, s1 = np.asarray(scale0, np.float32).astype(np.float64), np.asarray(scale1, np.float32).astype(np.float64)
    mu0, sd0, mu1, sd1 = s0[0], s0[2], s1[0], s1[2]
    r = sd0 / sd1
    w2 = (np.asarray(w, np.float32).astype(np.float64) * r).astype(np.float32)
    dmu = float(mu0 - mu1)                                                   # (one double subtraction)
    b64 = float(np.asarray(b, np.float32).reshape(-1)[0])
    num = float(Fraction(b64) * Fraction(float(sd0)) + Fraction(dmu))       # fma: exact, rounded once
    return w2, np.float32(np.float64(num) / sd1)


def head64(w, b, h):
    """float64 output of the one-output head on hidden activations h [n, K] -> (v^ [n], S [n] = sum|w_i h_i|)."""
    w64, h64 = np.asarray(w, np.float64).reshape(-1), np.asarray(h, np.float64)
    return h64 @ w64 + float(np.asarray(b).reshape(-1)[0]), np.abs(h64) @ np.abs(w64)


def real_units(vhat, scale):
    """V = v^ sigma + mu in float64 from values of any precision and a published float32 scale."""
    s = np.asarray(scale, np.float32).astype(np.float64)
    return np.asarray(vhat, np.float64) * s[2] + s[0]


def real_units32(vhat32, scale):
    """fmaf(v^, sigma, mu) of float32 values: the product of two float32 is exact in double, the sum rounds to double and then to
    float32 (a double rounding that can differ from the fused result only on a tie of the first: not at these sizes)."""
    return real_units(np.asarray(vhat32, np.float32), scale).astype(np.float32)


def allowance(w, b, w2, b2, h, scale0, scale1):
    """Per row of h: the derived bound on |V_1 - V_0| (module docstring), its three parts summed."""
    s0, s1 = np.asarray(scale0, np.float32).astype(np.float64), np.asarray(scale1, np.float32).astype(np.float64)
    mu0, sd0, mu1, sd1 = s0[0], s0[2], s1[0], s1[2]
    K = int(np.asarray(w).size)
    b64, b2_64 = float(np.asarray(b).reshape(-1)[0]), float(np.asarray(b2).reshape(-1)[0])
    v0, S = head64(w, b, h)
    v1, S2 = head64(w2, b2, h)
    V0, V1 = v0 * sd0 + mu0, v1 * sd1 + mu1
    rounding = U * (sd0 * S + abs(sd0 * b64 + mu0 - mu1))
    forwards = sd0 * (K + 8) * U * (S + abs(b64)) + sd1 * (K + 8) * U * (S2 + abs(b2_64))
    final = U * (np.abs(V0) + np.abs(V1))
    return rounding + forwards + final


def hidden64(layers, x, act="relu"):
    """float64 activations in front of the last layer: layers = [(W, b), ...] of the WHOLE network, x [n, d]."""
    f = {"relu": lambda z: np.maximum(z, 0.0), "tanh": np.tanh, "elu": lambda z: np.where(z > 0, z, np.expm1(np.minimum(z, 0.0)))}[act]
    h = np.asarray(x, np.float64)
    for W, b in layers[:-1]:
        h = f(h @ np.asarray(W, np.float64).T + np.asarray(b, np.float64))
    return h
