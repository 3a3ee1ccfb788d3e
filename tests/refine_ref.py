"""Pure Python / numpy restatement of the batched pose refinement's per-pose state machine (tests of
pcnerf::lm_update, pcnerf::refine_poses_fold and nof.registration.refine_poses_fold) -- test infrastructure only.

``lm_update`` is nof.registration.register_scan_fold's loop body, one evaluation at a time, with the statuses the
device kernel records where the host loop raises or breaks: 1 |xi| < xi_tol, 2 fewer than 6 valid beams, 3 a singular
damped system or a non-finite step.  ``run`` drives it with any evaluation function; driven by registration_ref's
float64 evaluations it is registration_ref.register_f64 (test_refine_cpu asserts that, bit for bit).

The scene of the refinement tests (``scene``) is localization_ref.grid_scene()'s: the analytic cavity, 256 directions
(seed 0), ranges from the float64 render at T* = se3_exp(XI_STAR)."""
import functools
import math

import numpy as np
import torch

import localization_ref as LR
import registration_ref as RR

STATE = 64
TACC, TTRIAL, N30, LAMBDA, STATUS, EVALS, NACC, XI = 0, 12, 24, 54, 55, 56, 57, 58
DEG = math.pi / 180.0
# the four starts from which the float64 loop accepts all 20 evaluations, and the rejection-path start
CONVERGING = (tuple(RR.XI_START), tuple(-v for v in RR.XI_START), tuple(0.5 * v for v in RR.XI_START),
              (0.3, -0.25, 0.2, 6 * DEG, -5 * DEG, 8 * DEG))
REJECTING = (0.6, -0.5, 0.4, 15 * DEG, -12 * DEG, 20 * DEG)


def unpack(n30):
    v = np.asarray(n30, dtype=np.float64)
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = v[:21]
    H = H + np.triu(H, 1).T
    return H, v[21:27].copy(), float(v[27]), int(round(float(v[28])))


def damped(n30, lam):
    """A = H + lam diag H of a normal30 row."""
    H = unpack(n30)[0]
    return H + lam * np.diag(np.diag(H))


def lm_init(T, damping):
    T = torch.as_tensor(T, dtype=torch.float64).clone()
    return {"T_acc": T.clone(), "T_trial": T.clone(), "n30": np.zeros(30), "lam": float(damping), "status": 0,
            "evals": 0, "nacc": 0, "xi": np.zeros(6)}


def lm_update(st, n30, xi_tol, se3_exp):
    """One evaluation's step of a running pose, in place -> (cost or NaN when the pose had stopped, accepted)."""
    if st["status"] != 0:
        return float("nan"), False
    n30 = np.asarray(n30, dtype=np.float64)
    H, b, cost, n_valid = unpack(n30)
    st["evals"] += 1
    if n_valid < 6:
        st["status"] = 2
        return cost, False
    accepted = st["nacc"] == 0 or cost <= float(st["n30"][27])
    if accepted:
        if st["nacc"] != 0:
            st["lam"] = st["lam"] / 10.0
        st["T_acc"], st["n30"] = st["T_trial"].clone(), n30.copy()
        st["nacc"] += 1
    else:
        st["lam"] = st["lam"] * 10.0
    Ha, ba = unpack(st["n30"])[:2]
    try:
        xi = np.linalg.solve(Ha + st["lam"] * np.diag(np.diag(Ha)), -ba)
    except np.linalg.LinAlgError:
        xi = np.full(6, np.nan)
    if not np.isfinite(xi).all():
        st["status"], st["T_trial"] = 3, st["T_acc"].clone()
        return cost, accepted
    st["xi"] = xi
    st["T_trial"] = se3_exp(xi) @ st["T_acc"]
    if float(np.linalg.norm(xi)) < xi_tol:
        st["status"] = 1
    return cost, accepted


def pose_out(st):
    return st["T_acc"] if st["status"] in (2, 3) else st["T_trial"]


def rows12(T):
    T = np.asarray(T, dtype=np.float64)
    return np.concatenate([T[:3, :3].reshape(9), T[:3, 3]])


def to_row(st):
    """The restatement's state as the device's 64-double row."""
    row = np.zeros(STATE)
    row[TACC:TACC + 12], row[TTRIAL:TTRIAL + 12] = rows12(st["T_acc"]), rows12(st["T_trial"])
    row[N30:N30 + 30] = st["n30"]
    row[LAMBDA], row[STATUS], row[EVALS], row[NACC] = st["lam"], st["status"], st["evals"], st["nacc"]
    row[XI:XI + 6] = st["xi"]
    return row


def from_row(row):
    """A device state row as the restatement's state."""
    row = np.asarray(row, dtype=np.float64)

    def pose(v):
        T = torch.eye(4, dtype=torch.float64)
        T[:3, :3] = torch.from_numpy(v[:9].reshape(3, 3).copy())
        T[:3, 3] = torch.from_numpy(v[9:12].copy())
        return T

    return {"T_acc": pose(row[TACC:TACC + 12]), "T_trial": pose(row[TTRIAL:TTRIAL + 12]),
            "n30": row[N30:N30 + 30].copy(), "lam": float(row[LAMBDA]), "status": int(row[STATUS]),
            "evals": int(row[EVALS]), "nacc": int(row[NACC]), "xi": row[XI:XI + 6].copy()}


def run(evaluate, T0, se3_exp, iters=20, damping=1e-6, xi_tol=0.0):
    """``iters`` x (evaluate(T_trial) -> normal30 row, lm_update) -> dict(state, pose, eval_costs, accepted, costs
    (the accepted ones), xi_norms (per evaluation made))."""
    st = lm_init(T0, damping)
    eval_costs, mask, norms = [], [], []
    for _ in range(iters):
        if st["status"] != 0:
            eval_costs.append(float("nan"))
            mask.append(False)
            continue
        cost, acc = lm_update(st, evaluate(st["T_trial"]), xi_tol, se3_exp)
        eval_costs.append(cost)
        mask.append(acc)
        norms.append(float(np.linalg.norm(st["xi"])))
    return {"state": st, "pose": pose_out(st), "eval_costs": eval_costs, "accepted": mask,
            "costs": [c for c, a in zip(eval_costs, mask) if a], "xi_norms": norms}


# ----------------------------------------------------------------------------------------------- the 256-beam scene
def evaluate_f64(fold, dirs, ranges, n_samples=64, n_importance=128, huber_delta=0.0, min_sumw=0.5):
    """T -> the normal30 row of registration_ref's float64 evaluation (register_f64's loop body)."""
    tgt = np.asarray(ranges)

    def f(T):
        rays = RR.rays_f64(dirs, T)
        depth, sumw, jac = RR.render_two_pass(fold, fold, rays, n_samples, n_importance)
        return RR.normal_eq(rays[:, :6].numpy(), jac.numpy(), depth.numpy(), sumw.numpy(), tgt, huber_delta,
                            min_sumw)[0]
    return f


def starts():
    from nof.registration import se3_exp
    T_star = LR.grid_scene()["T_star"]
    return [se3_exp(x) @ T_star for x in CONVERGING], se3_exp(REJECTING) @ T_star


@functools.lru_cache(maxsize=None)
def f64_runs():
    """registration_ref.register_f64 (20 evaluations, 64 + 128 samples) from the four converging starts and the
    rejection start on the 256-beam scene, computed once per process -> (list of four runs, the rejection run)."""
    from nof.registration import se3_exp
    s = LR.grid_scene()
    good, bad = starts()
    rng = s["ranges"].numpy()

    def go(T0):
        return RR.register_f64(s["fold"], s["fold"], s["dirs"], rng, T0, se3_exp, T_ref=s["T_star"])
    return [go(T0) for T0 in good], go(bad)
