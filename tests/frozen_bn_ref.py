"""Float64 restatement of the frozen-BatchNorm parameter backward (tests of nof._autograd.FrozenPass /
FrozenPassPoints and of the kernels k_eval_gmoments / k_eval_param_grads).

The eval-mode NOF is logit_s = a(theta) . e_s + c(theta) (every LeakyReLU has slope 1, eval BatchNorm is affine), so
with g_s = dL/dlogit_s the 34 parameter gradients of a pass are those of ONE pseudo-sample whose input is
m = sum_s g_s e_s and whose every additive constant is scaled by s0 = sum_s g_s:

    X_L = m (L = 0), [m ; y_3] (L = 4), else y_{L-1};  h_L = W_L X_L + b_L s0;  alpha_L = gamma_L / sqrt(rv_L + eps)
    y_L = alpha_L (h_L - rm_L s0) + beta_L s0;  F = out_w . y_7 + out_b s0
    u_7 = out_w, d out_w = y_7, d out_b = s0;  for L = 7..0:  d beta_L = u_L s0,
    d gamma_L = u_L (h_L - rm_L s0) / sqrt(rv_L + eps), v_L = u_L alpha_L, d W_L = v_L (x) X_L, d b_L = v_L s0,
    u_{L-1} = W_L^T v_L (at L = 4 only columns 63..318 feed back).

test_frozen_bn_cpu pins this to per-sample torch float64 autograd of oracle.ref_cpu's eval network."""
import numpy as np
import torch

from nof import synthetic as syn
from oracle import ref_cpu as O

# the 34 trainable tensors in pcnerf_nof_grads / nof._ops.grad_params order
GRAD_KEYS = ([n + ".weight" for n in O.LIN] + [n + ".bias" for n in O.LIN] + [n + ".weight" for n in O.BN]
             + [n + ".bias" for n in O.BN] + ["occ_out.0.weight", "occ_out.0.bias"])


def params64(seed):
    """init_nof_params(seed) as float64 numpy arrays (the float32 values, widened)."""
    return {k: np.asarray(v, dtype=np.float64) for k, v in syn.init_nof_params(seed).items()
            if not k.endswith("num_batches_tracked")}


def moments(E, g):
    """(64,) float64: [:63] = sum_s g_s E_s, [63] = sum_s g_s for E (N, 63), g (N,)."""
    E, g = np.asarray(E, dtype=np.float64), np.asarray(g, dtype=np.float64).reshape(-1)
    return np.concatenate([g @ E.reshape(-1, 63), [g.sum()]])


def param_grads(P, mom, eps=O.EPS_BN):
    """{key: gradient} of the 34 tensors from the pass's moments ``mom`` (64,), all float64."""
    mom = np.asarray(mom, dtype=np.float64)
    m, s0 = mom[:63], mom[63]
    X, hc, alpha, y = [], [], [], m
    for L in range(8):
        x = m if L == 0 else np.concatenate([m, y]) if L == 4 else y
        X.append(x)
        h = P[O.LIN[L] + ".weight"] @ x + P[O.LIN[L] + ".bias"] * s0
        r = 1.0 / np.sqrt(P[O.BN[L] + ".running_var"] + eps)
        hc.append((h - P[O.BN[L] + ".running_mean"] * s0) * r)
        alpha.append(P[O.BN[L] + ".weight"] * r)
        y = P[O.BN[L] + ".weight"] * hc[L] + P[O.BN[L] + ".bias"] * s0
    out = {"occ_out.0.weight": y.reshape(1, 256).copy(), "occ_out.0.bias": np.array([s0])}
    u = P["occ_out.0.weight"].reshape(-1)
    for L in range(7, -1, -1):
        out[O.BN[L] + ".bias"] = u * s0
        out[O.BN[L] + ".weight"] = u * hc[L]
        v = u * alpha[L]
        out[O.LIN[L] + ".weight"] = np.outer(v, X[L])
        out[O.LIN[L] + ".bias"] = v * s0
        u = P[O.LIN[L] + ".weight"].T @ v
        if L == 4:
            u = u[63:]
    return out


def autograd_param_grads(P, E, g):
    """The same 34 gradients by per-sample torch float64 autograd of oracle.ref_cpu's eval network on the encoded
    batch E (N, 63): L = sum_s c_s p_s with c_s = g_s / (p_s (1 - p_s)), so that dL/dlogit_s = g_s."""
    Q = {k: torch.from_numpy(np.array(v, dtype=np.float64)).requires_grad_(k in GRAD_KEYS) for k, v in P.items()}
    Et, gt = torch.from_numpy(np.asarray(E, dtype=np.float64)), torch.from_numpy(np.asarray(g, dtype=np.float64))
    p = O.nof_forward(Q, Et, False).reshape(-1)
    c = (gt / (p * (1 - p))).detach()
    (c * p).sum().backward()
    return {k: Q[k].grad.numpy() for k in GRAD_KEYS}


def grads_list(d):
    return [d[k] for k in GRAD_KEYS]
