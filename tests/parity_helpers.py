"""What the per-kernel parity tests share: the e_hip / e32 tally of the float64 comparisons and the knife-edge
exclusion of the inverse-CDF draws -- test infrastructure only, CPU only."""
import torch

from gradcheck import _report

import render_f64 as F
import render_inputs as I

FLOOR = 2.4e-7


class Tally:
    """Collects every quantity's e_hip / e32 of one test, reports them, and fails once at the end with all misses."""

    def __init__(self, test):
        self.test, self.bad, self.worst = test, [], 0.0

    def check(self, case, name, x_hip, q32, q64, cap=I.E32_CAP):
        self.check_err(case, name, F.err(x_hip, q64), F.err(q32, q64), cap)

    def check_err(self, case, name, e_hip, e32, cap=I.E32_CAP):
        """The same rule on a pair of errors measured elsewhere (the quantile identity of tests/sampling_f64.py)."""
        tol = max(4 * e32, FLOOR)
        self.worst = max(self.worst, e_hip / tol)
        _report({"test": self.test, "case": case, "quantity": name, "e_hip": e_hip, "e32": e32, "tol": tol})
        if e32 > cap:
            self.bad.append(f"{case} {name}: float32 reference off by {e32:.3g} > {cap:.3g} (inputs too hard)")
        if not e_hip <= tol:
            self.bad.append(f"{case} {name}: e_hip {e_hip:.3g} > max(4 x e32 {e32:.3g}, {FLOOR})")

    def done(self):
        _report({"test": self.test, "worst_e_hip_over_tol": self.worst, "failed": len(self.bad)})
        assert not self.bad, "\n".join(self.bad)


def knife_edge(bins, weights, u):
    """Samples whose bin has cdf_hi - cdf_lo within 4 ulp of the reference's 1e-5 threshold (render.py:408): there
    the branch depends on the last bit of the normaliser sum, whose order torch CPU fixes per ISA."""
    w = weights + 1e-5
    cdf = torch.cat([torch.zeros_like(w[:, :1]), torch.cumsum(w / w.sum(-1, keepdim=True), -1)], -1)
    inds = torch.searchsorted(cdf, u, right=True)
    lo = torch.gather(cdf, 1, torch.clamp(inds - 1, min=0))
    hi = torch.gather(cdf, 1, torch.clamp(inds, max=cdf.shape[-1] - 1))
    ulp = torch.finfo(torch.float32).eps * torch.maximum(hi.abs(), torch.tensor(1e-30))
    near = ((hi - lo) - 1e-5).abs() <= 4 * ulp
    # a neighbouring cdf entry within an ulp of u can also move the bin
    return near | ((u - lo).abs() <= 2 * ulp) | ((hi - u).abs() <= 2 * ulp)
