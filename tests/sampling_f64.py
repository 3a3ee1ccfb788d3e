"""Inputs, float64 restatements and validity checks of the per-kernel tests of the sampling chain (k_sample_coarse,
k_perturb, k_sample_pdf, k_resample), the scalar losses (k_pointwise_loss*, k_child_range_*) and the group walk
(k_walk_*) -- test infrastructure only, CPU only.  It stands to tests/test_sampling_kernels_gpu.py and
tests/test_loss_kernels_gpu.py as render_f64.py / render_inputs.py stand to test_render_kernels_gpu.py; the
conditions the inputs must meet are checked without a GPU in tests/test_sampling_f64_cpu.py.

Every check takes the result under test as an argument, so the same function judges the kernel (GPU tests) and the
float32 oracle (CPU test: the inputs are no harder than float32 can answer).  Line numbers are the reference's
nof/render.py and train_kitti.py.
"""
import collections
import math

import numpy as np
import torch

from oracle import ref_cpu as O

from parity_helpers import knife_edge

NEXT1 = float(np.nextafter(np.float32(1), np.float32(0)))   # the largest float32 below 1


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def same_bits(a, b):
    """Bit for bit, a NaN equal to any NaN (torch.equal calls NaN unequal to itself)."""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb)) and bool(torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32)))


# ----------------------------------------------------------------------------------------------- coarse sampling
COARSE_S = tuple(range(1, 131)) + (191, 192, 193, 255, 256, 257, 768, 4096)
COARSE_R = (1, 3, 4, 5, 9)
CHILD_KINDS = ("inside", "equal", "below", "above", "zero", "reversed")
STD_COLS = (6, 7, 10, 11)          # near, far, child near, child far of the standard 15-column table
PERM_COLS = (3, 0, 8, 5)           # the same four in the 9-column table of permuted_table()


def coarse_table(R, seed, first_kind=0):
    """A 15-column ray table: near in [0.5, 10], far up to 80 (row 0 spans exactly 0.5 .. 80), the child interval
    of row r of kind CHILD_KINDS[(first_kind + r) % 6] -- inside the parent interval, equal to it (every child value
    ties with a parent value in the merge), disjoint below, disjoint above, of zero width, reversed (child_near >
    child_far: a decreasing list, the all-pairs rank fallback).  Every other column holds noise, so that reading a
    wrong column shows."""
    g = _gen(seed)
    t = torch.rand(R, 15, generator=g) * 100
    near = 0.5 + 9.5 * torch.rand(R, generator=g)
    far = near + (80 - near) * (0.2 + 0.8 * torch.rand(R, generator=g))
    near[0], far[0] = 0.5, 80.0
    a, b = torch.rand(R, generator=g), torch.rand(R, generator=g)
    cn = near + (far - near) * 0.8 * a
    cf = cn + (far - cn) * (0.1 + 0.9 * b)
    for r in range(R):
        kind = CHILD_KINDS[(first_kind + r) % 6]
        if kind == "equal":
            cn[r], cf[r] = near[r], far[r]
        elif kind == "below":
            cn[r], cf[r] = 0.2 * near[r], 0.6 * near[r]
        elif kind == "above":
            cn[r], cf[r] = 1.1 * far[r], 1.5 * far[r]
        elif kind == "zero":
            cf[r] = cn[r]
        elif kind == "reversed":
            cn[r], cf[r] = cf[r].clone(), cn[r].clone()
    for c, v in zip(STD_COLS, (near, far, cn, cf)):
        t[:, c] = v
    return t


def permuted_table(t):
    """The four columns k_sample_coarse reads, moved to columns PERM_COLS of a 9-column table of noise."""
    p = torch.rand(t.shape[0], 9, generator=_gen(99)) * 100
    for src, dst in zip(STD_COLS, PERM_COLS):
        p[:, dst] = t[:, src]
    return p


def parents_of(S):
    """The n_parent values of the segmented branch that are valid at S (1 <= n_parent < S)."""
    return sorted({n for n in (1, 2, S - 1, S - 2, int(0.9 * S), S // 2) if 1 <= n < S})


def disparity_z(t, S, cols=STD_COLS):
    """render.py:565-567 in float32 on the CPU, written as the reference writes it."""
    near, far = t[:, cols[0]:cols[0] + 1], t[:, cols[1]:cols[1] + 1]
    s = torch.linspace(0, 1, S).expand(t.shape[0], S)
    return 1 / (1 / near * (1 - s) + 1 / far * s)


def segmented_z(t, S, n_parent, cols=STD_COLS):
    """render.py:433-442: the sort of the parent and the child linspace (O.coarse_z's branch with n_parent given)."""
    zp = O.lin_z(t[:, cols[0]:cols[0] + 1], t[:, cols[1]:cols[1] + 1], n_parent)
    zc = O.lin_z(t[:, cols[2]:cols[2] + 1], t[:, cols[3]:cols[3] + 1], S - n_parent)
    return torch.sort(torch.cat([zp, zc], -1), -1)[0]


# ----------------------------------------------------------------------------------------------- perturbation
PERTURB_SHAPES = ((1, 1), (5, 1), (3, 2), (7, 37), (4, 63), (4, 64), (4, 65), (2, 300))
PERTURB_AMOUNTS = (0.0, 0.5, 1.0)


def perturb_case(R, S, sorted_rows=True):
    """z (sorted rows, or unsorted ones) and draws in [0, 1) that hold 0 and the largest float32 below 1."""
    g = _gen(1000 * R + S)
    z = 2 + 30 * torch.rand(R, S, generator=g)
    if sorted_rows:
        z = torch.sort(z, -1)[0]
    rand = torch.rand(R, S, generator=g)
    flat = rand.view(-1)
    flat[0] = 0.0
    flat[-1] = NEXT1
    if flat.numel() > 2:
        flat[flat.numel() // 2] = NEXT1
        flat[1] = 0.0
    return z, rand


# ----------------------------------------------------------------------------------------------- inverse-CDF draws
PDF_BINS = (2, 3, 64, 65, 66, 67, 129, 130, 1365, 1366, 1820, 1821, 2730, 2731, 5461)
PDF_SAMPLES = (1, 63, 64, 65, 96)
PDF_KINDS = ("uniform", "zero", "onehot10", "onehot01", "zero_run", "spread")
CLEAR, TINY = 2e-5, 5e-6          # float64 bin masses: at least CLEAR interpolates, below TINY takes denom -> 1
DELTA = 2e-6                      # how far, relative to its value, a float32 cdf entry can lie from the float64 one:
                                  # the float32 normaliser scales the whole cdf, by up to 9.7e-7 over these cases
                                  # (test_sampling_f64_cpu.py); cdf[0] = 0 is exact
UNCLEAR_CAP, KNIFE_CAP = 0.02, 0.05
# the one-hot 0.1 row's weight where it is not 0.1: with 2,730 weights every empty bin holds 1e-5 / 0.1273, and 134 of
# them make 1 / 95 to 8e-6 -- each of the 96 deterministic draws before the hot bin then sits ON a cdf entry of the
# reference's own float32 evaluation, a knife edge (21 of the row's draws)
ONEHOT01 = {2730: 0.11}


def pdf_waves(n_bins):
    """k_sample_pdf's waves per workgroup: as many rays' bins | weights | cdf as fit 64 KiB, four at the most."""
    return min(4, (64 * 1024) // (12 * n_bins))


def pdf_rays(n_bins):
    return (1, 5, pdf_waves(n_bins) + 1)


def pdf_weights(kind, npdf, g, det=False):
    """One row of weights.  Scales are chosen for the branch each kind is meant to reach: with T = sum(w + 1e-5) an
    empty bin has mass 1e-5 / T, which must be below TINY (T > 2) or at least CLEAR (T < 0.5) -- one-hot rows use 10
    and 0.1, not 1: a total near 1 puts every empty bin within 1 % of the reference's 1e-5 threshold, where the
    branch is the last bit of the normaliser.  'uniform' and 'zero_run' rows total ~2.2 whatever the bin count, so the
    20 zero weights in the middle of a 'zero_run' row keep a mass (4.5e-6) that float32 still resolves at cdf 0.5.
    The one-hot 10 row of a deterministic launch has its weight in the last bin: the last draw is u = 1 exactly,
    and with an empty last bin the reference returns the last edge or a point a bin before it as its own float32
    cdf ends at or above 1 -- it ends at 1.0000004 with 63 weights, where the float64-summed normaliser ends at 1.
    First and last weights of the random kinds are the row's mean: u = 0 and u just below 1 then fall in bins that
    clearly interpolate."""
    if kind == "zero":
        return torch.zeros(npdf)
    if kind in ("onehot10", "onehot01"):
        w = torch.zeros(npdf)
        hot = int(torch.randint(0, npdf, (1,), generator=g))
        if kind == "onehot10" and det:
            hot = npdf - 1
        w[hot] = 10.0 if kind == "onehot10" else ONEHOT01.get(npdf, 0.1)
        return w
    if kind == "spread":
        w = 10 ** (-6 + 9 * torch.rand(npdf, generator=g))
        # a weight whose bin would hold between TINY and CLEAR moves up to 1.15 CLEAR: the band is a fifteenth of
        # the bins, and two draws of 64 in it (seen at 5,461 bins) are past the 2 % a case may leave out
        wd = w.double() + 1e-5
        band = (wd >= TINY * wd.sum()) & (wd < 1.15 * CLEAR * wd.sum())
        w[band] = float(1.15 * CLEAR * wd.sum())
    else:
        w = (0.1 + 0.9 * torch.rand(npdf, generator=g)) * (4.0 / npdf)   # every mass >= 0.17 / npdf > CLEAR
        if kind == "zero_run" and npdf >= 4:
            n0 = min(20, npdf - 2)
            a = (npdf - n0) // 2
            w[a:a + n0] = 0.0
    w[0] = w[-1] = w.mean()
    return w


def pdf_bins(w, g):
    """Bin edges from 1 on for one row of weights: even widths of a total 4, jittered +-30 %, plus 0.03 X mass_i
    (X the last edge).  What float32 can say about F(x) is limited by the rounding of x itself, up to 2^-24 X,
    times the density mass_i / width_i; the added width keeps that below 2e-6 in the heaviest bin of a one-hot row
    (without it an estimated 2e-4 at 5,461 bins, ten times the cap on the float32 reference)."""
    npdf = w.numel()
    wd = w.double() + 1e-5
    mass = wd / wd.sum()
    base = (4.0 / npdf) * (0.7 + 0.6 * torch.rand(npdf, generator=g).double())
    X = (1.0 + float(base.sum())) / 0.97
    width = base + 0.03 * X * mass
    return (1.0 + torch.cat([torch.zeros(1, dtype=torch.float64), torch.cumsum(width, 0)])).float()


def cdf64(weights):
    """The exact CDF at the bin edges: cumsum of (w + 1e-5) / sum(w + 1e-5) in float64, (R, npdf + 1)."""
    wd = weights.double() + 1e-5
    pdf = wd / wd.sum(-1, keepdim=True)
    c = torch.cat([torch.zeros_like(pdf[:, :1]), torch.cumsum(pdf, -1)], -1)
    c[:, -1] = 1.0
    return c


def pdf_u(weights, n, g):
    """Given draws: exactly 0 first, the largest float32 below 1 second (not in a row whose last bin is empty, the
    one-hot 10 row: the reference returns the last edge or a point a bin before it as its float32 cdf ends below or
    above that draw -- the float64-summed normaliser's ends exactly on it), then the middle of up to 8 bins of mass
    below TINY and above 3 DELTA cdf (the denom -> 1 branch, which random draws all but never reach), the rest
    uniform."""
    R = weights.shape[0]
    u = torch.rand(R, n, generator=g)
    c = cdf64(weights)
    for r in range(R):
        mass = c[r, 1:] - c[r, :-1]
        plant = [0.0] + ([NEXT1] if mass[-1] >= CLEAR else [])
        tiny = torch.nonzero((mass < TINY) & (mass >= 3 * DELTA * c[r, 1:])).flatten()   # (wide enough to aim at)
        for j in tiny[torch.linspace(0, len(tiny) - 1, min(8, len(tiny))).long()].tolist() if len(tiny) else []:
            plant.append(float(0.5 * (c[r, j] + c[r, j + 1])))
        k = min(n, len(plant))
        u[r, :k] = torch.tensor(plant[:k], dtype=torch.float32)
    return u


def pdf_kinds(n_bins, R, n, det, first_kind):
    """Row r is of kind PDF_KINDS[(first_kind + r) % 6] -- except that an all-zero row gives way to a uniform one
    where the deterministic draws k / (n - 1) would sit ON its cdf entries j / (n_bins - 1) (the two counts share a
    factor): each such draw is a knife edge of the reference's own search, and a whole row of them is past the 5 %
    cap.  All-zero rows meet the deterministic draws at the other sample counts, and the given draws at all."""
    kinds = [PDF_KINDS[(first_kind + r) % 6] for r in range(R)]
    if det and n > 1 and math.gcd(n_bins - 1, n - 1) > 1:
        kinds = ["uniform" if k == "zero" else k for k in kinds]
    return kinds


def pdf_case(n_bins, R, n, det, first_kind):
    """bins (R, n_bins), weights (R, n_bins - 1), u (R, n) (the linspace when det); rows of pdf_kinds()."""
    g = _gen(7919 * n_bins + 131 * R + 17 * n + (1 if det else 0))
    ws = [pdf_weights(k, n_bins - 1, g, det) for k in pdf_kinds(n_bins, R, n, det, first_kind)]
    bins = torch.stack([pdf_bins(w, g) for w in ws])
    weights = torch.stack(ws)
    u = torch.linspace(0., 1., steps=n).expand(R, n).contiguous() if det else pdf_u(weights, n, g)
    return bins, weights, u


def dyadic_case(long_row):
    """Draws that sit ON cdf entries, where 'cdf <= u' and 'cdf < u' part -- made so that no evaluation can disagree
    about the entries.  The weights are dyadic numbers minus float32(1e-5), so that w + 1e-5 is exactly 2, 2^-16,
    2^-16, 2 - 2^-15 (and 64 more bins of 1/16 when ``long_row``: two bins per lane): every partial sum is a
    multiple of 2^-16 below 256, exact in float32 in any order, the total is 4 (or 8), every pdf value and cdf
    entry exact.  The two middle bins hold 2^-18 (2^-19): the denom -> 1 branch.  u = the entries 1, 2, 3 and, for
    contrast, the middle of bin 0.  -> bins (R, nb), weights, u, and the edge index each of the first three draws
    of a row must return exactly (searchsorted right=True: the draw on entry j belongs to bin j and returns edge j:
    with 'cdf < u' entry 2 and 3 return edge 1 + 2^-18 (b2 - b1) and edge 2 + ... instead, a bin short)."""
    c = np.float32(1e-5)
    wp = [2.0, 2.0 ** -16, 2.0 ** -16, 2.0 - 2.0 ** -15] + ([1 / 16] * 64 if long_row else [])
    w = torch.tensor([float(np.float32(np.float32(v) - c)) for v in wp])
    R, npdf = 5, len(wp)
    g = _gen(len(wp))
    bins = torch.stack([1 + torch.cumsum(torch.cat([torch.zeros(1), 0.5 + torch.rand(npdf, generator=g)]), 0)
                        for _ in range(R)])
    total = 8.0 if long_row else 4.0
    entries = [2.0 / total, (2.0 + 2.0 ** -16) / total, (2.0 + 2.0 ** -15) / total]
    u = torch.tensor(entries + [0.25 * 2.0 / total]).expand(R, 4).contiguous()
    return bins, w.expand(R, npdf).contiguous(), u, (1, 2, 3)


def classify(c, u):
    """-> (clear, tiny, unclear) masks of the draws u (R, n) against the float64 CDF c.  A draw's candidate bins are
    all those within d = DELTA u of u: bin i with c[i] - d <= u <= c[i + 1] + d (the float32 search may pick any of
    them; u = 0 has the first bin alone).  clear: every candidate holds at least CLEAR; the draw interpolates, and
    F(x) = u whichever candidate was taken (F is continuous across the edge).  tiny: one candidate, below TINY, and
    u not within d of the top of the CDF (past it the reference returns the last edge); in that branch x jumps by a
    bin from one candidate to the next, so a draw with two of them has no defined answer.  unclear: everything else."""
    u = u.double().contiguous()
    npdf = c.shape[1] - 1
    mass = c[:, 1:] - c[:, :-1]
    d = DELTA * u
    first = torch.searchsorted(c[:, 1:].contiguous(), u - d, right=False).clamp(max=npdf - 1)
    last = (torch.searchsorted(c[:, :-1].contiguous(), u + d, right=True) - 1).clamp(min=0)
    last = torch.maximum(last, first)
    zero = torch.zeros_like(mass[:, :1])
    n_small = torch.cat([zero, torch.cumsum((mass < CLEAR).double(), -1)], -1)     # bins below CLEAR before bin i
    small_in = torch.gather(n_small, 1, last + 1) - torch.gather(n_small, 1, first)
    clear = small_in == 0
    top = u + d >= 1.0
    tiny = (first == last) & (torch.gather(mass, 1, first) < TINY) & ~top
    return clear, tiny, ~(clear | tiny)


def quantile_error(bins, c, x, u, sel):
    """max over the selected draws of |F(x) - u|, F the piecewise-linear float64 CDF through (bins, c)."""
    if not bool(sel.any()):
        return 0.0
    b, x, u = bins.double(), x.double(), u.double()
    npdf = c.shape[1] - 1
    i = (torch.searchsorted(b.contiguous(), x.contiguous(), right=True) - 1).clamp(0, npdf - 1)
    b0, b1 = torch.gather(b, 1, i), torch.gather(b, 1, i + 1)
    c0, c1 = torch.gather(c, 1, i), torch.gather(c, 1, i + 1)
    Fx = c0 + (x - b0) / (b1 - b0) * (c1 - c0)
    return float((Fx - u).abs()[sel].max())


def tiny_error(bins, c, x, u, sel):
    """max over the selected draws (classify's tiny) of |x - (b0 + (u - c0)(b1 - b0))| / max |bins| of the row."""
    if not bool(sel.any()):
        return 0.0
    b, u = bins.double(), u.double().contiguous()
    npdf = c.shape[1] - 1
    j = (torch.searchsorted(c.contiguous(), u, right=True) - 1).clamp(0, npdf - 1)
    b0, b1 = torch.gather(b, 1, j), torch.gather(b, 1, j + 1)
    want = b0 + (u - torch.gather(c, 1, j)) * (b1 - b0)
    e = (x.double() - want).abs() / b.abs().amax(-1, keepdim=True)
    return float(e[sel].max())


def pdf_errors(bins, weights, u, x):
    """-> dict(quantile, tiny, unclear_share, n_tiny) of the draws x (R, n) for (bins, weights, u)."""
    c = cdf64(weights)
    clear, tiny, unclear = classify(c, u)
    return {"quantile": quantile_error(bins, c, x, u, clear), "tiny": tiny_error(bins, c, x, u, tiny),
            "unclear_share": float(unclear.double().mean()), "n_tiny": int(tiny.sum())}


def pdf_knife(bins, weights, u):
    """The existing knife-edge exclusion, minus the draws at exactly 0: cdf[0] is 0 in every evaluation and cdf[1]
    is positive, so u = 0 lies in the first bin whatever the rounding (knife_edge flags it because u - cdf[0] = 0;
    left in, the one draw of a one-sample case would all be excluded)."""
    return knife_edge(bins, weights, u.contiguous()) & (u != 0)


# ----------------------------------------------------------------------------------------------- resampling
RESAMPLE_S = (3, 4, 5, 63, 64, 65, 129)
RESAMPLE_I = (1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
RESAMPLE_U = ("sorted", "unsorted", "det")


def resample_case(R, S, n_imp, u_mode, idx):
    """Coarse z (even steps from 2 to 30 jittered by 30 %: no narrow mid-point bin, see pdf_bins), weights in
    [0.05, 1] (every bin clearly interpolates) and draws; one row in three -- (r + idx) % 3 == 0 -- has two
    neighbouring coarse entries swapped, which sends it through the bitonic sort of the whole concatenation (its
    mid-point bins stay increasing)."""
    g = _gen(100003 * S + 101 * n_imp + 7 * R + RESAMPLE_U.index(u_mode))
    z = 2 + 28 * (torch.arange(S).float() + 0.3 * torch.rand(R, S, generator=g)) / S
    w = 0.05 + 0.95 * torch.rand(R, S, generator=g)
    for r in range(R):
        if (r + idx) % 3 == 0:
            a = S // 2
            z[r, a], z[r, a + 1] = z[r, a + 1].clone(), z[r, a].clone()
    u = None
    if u_mode != "det":
        u = torch.rand(R, n_imp, generator=g)
        if u_mode == "sorted":
            u = torch.sort(u, -1)[0]
    return z, w, u


def resample_split(out, z):
    """The row-wise multiset difference out - z: -> (ok, rest) with ok False when a coarse value is missing from the
    output bit for bit, rest (R, I) the remaining values in ascending order."""
    rest = []
    for o, c in zip(out.tolist(), z.tolist()):
        left = collections.Counter(o)
        left.subtract(collections.Counter(c))
        if any(v < 0 for v in left.values()):
            return False, None
        rest.append(sorted(left.elements()))
    return True, torch.tensor(rest, dtype=torch.float32)


def resample_errors(z, w, u, n_imp, out):
    """The three assertions on one resample output (render.py:456-467) that do not go through pcnerf_sample_pdf:
    -> dict(sorted, contains_z, quantile, unclear_share)."""
    R = z.shape[0]
    ok, rest = resample_split(out, z)
    res = {"sorted": bool((out[:, 1:] >= out[:, :-1]).all()), "contains_z": ok}
    if not ok:
        return res
    mid = 0.5 * (z[:, 1:] + z[:, :-1])
    uu = torch.linspace(0., 1., steps=n_imp).expand(R, n_imp) if u is None else u
    uu = torch.sort(uu.contiguous(), -1)[0]
    res.update(pdf_errors(mid, w[:, 1:-1], uu, rest))
    return res


# ----------------------------------------------------------------------------------------------- pointwise loss
LOSS_N = (1, 2, 1023, 1024, 1025, 4097, 100003)
LOSS_KINDS = ("mse", "l1", "smoothl1")
LOSS_MASKS = ("none", "half", "ones", "first", "last", "zeros")
# (pred, target) with d = pred - target exact: 0, +-1, and +-1 one float32 ulp inside and outside
_IN, _OUT = NEXT1, float(np.nextafter(np.float32(1.5), np.float32(2)))
PLANTED = ((37.5, 37.5), (1.5, 0.5), (0.5, 1.5), (_IN, 0.0), (_OUT, 0.5), (0.0, _IN), (0.5, _OUT))


def loss_case(n):
    """pred and target as the criteria feed them (ranges of 2 .. 12 m times 10; differences on both sides of
    SmoothL1's |d| = 1), with as many PLANTED pairs as fit from element 0 on (starting at pair n % 7).
    -> (pred, target, planted indices, their pair numbers)."""
    g = _gen(n)
    target = 10 * (2 + 10 * torch.rand(n, generator=g))
    pred = target + 1.5 * torch.randn(n, generator=g)
    k = min(n, len(PLANTED))
    which = [(n + i) % len(PLANTED) for i in range(k)]
    for i, p in enumerate(which):
        pred[i], target[i] = PLANTED[p]
    return pred, target, list(range(k)), which


def loss_mask(name, n):
    if name == "none":
        return None
    m = torch.zeros(n, dtype=torch.bool)
    if name == "half":
        m = torch.rand(n, generator=_gen(n + 1)) < 0.5
    elif name == "ones":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[n - 1] = True
    return m


def elementwise_loss(pred, target, kind):
    """The element loss in the tensors' dtype: (a - b)^2, |a - b|, or SmoothL1 with the strict |d| < 1
    (nof/criteria/loss.py:42-50, torch's beta = 1)."""
    d = pred - target
    if kind == "mse":
        return d * d
    if kind == "l1":
        return d.abs()
    return torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5)


def pointwise_ref(pred, target, kind, mask, dtype, g_out=1.0):
    """mean over the selected elements of the torch loss in ``dtype`` and autograd's d(g_out * loss)/dpred (zero
    outside the mask; all zero for an empty selection, where the loss itself is NaN)."""
    a = pred.to(dtype).clone().requires_grad_(True)
    b = target.to(dtype)
    fn = {"mse": torch.nn.functional.mse_loss, "l1": torch.nn.functional.l1_loss,
          "smoothl1": torch.nn.functional.smooth_l1_loss}[kind]
    loss = fn(a, b) if mask is None else fn(a[mask], b[mask])
    if mask is not None and not bool(mask.any()):
        return loss.detach(), torch.zeros_like(a).detach()
    (g,) = torch.autograd.grad(loss * g_out, a)
    return loss.detach(), g


def planted_exact(pair, kind):
    """float32 loss value and gradient of one PLANTED pair alone: d is exact, 0.5 d^2 and |d| - 0.5 are rounded
    once (the kernel's 0.5f * d * d: the halving is exact)."""
    d = float(np.float32(PLANTED[pair][0])) - float(np.float32(PLANTED[pair][1]))
    sg = (d > 0) - (d < 0)
    if kind == "mse":
        return np.float32(d * d), np.float32(2 * d)
    if kind == "l1":
        return np.float32(abs(d)), np.float32(sg)
    return (np.float32(0.5 * d * d), np.float32(d)) if abs(d) < 1 else (np.float32(abs(d) - 0.5), np.float32(sg))


# ----------------------------------------------------------------------------------------------- child range loss
RANGE_N = (1, 255, 256, 257, 5000)
RANGE_CHILDREN = (1, 3, 1500, 15333)
RANGE_PRE, RANGE_POSTS = 10.0, (0.1, 0.05)
RANGE_PATTERNS = ("mixed", "one_owner")


def range_case(n, N, pattern, seed=0):
    """pred, target (ranges of 2 .. 12 m in steps of 1/1024 m: pre * pred is then exact in float32, as in float64,
    and the difference of the two products carries no rounding for a small difference to magnify) and a 15-column
    ray table whose column 9 holds the child ids.  'mixed': ids among the first 7 children and child N (all others
    own no ray), then from element 0 on 0, N + 1, k + 0.4, k + 0.5, k + 0.6 with k = min(2, N);
    'one_owner': every ray belongs to child min(2, N)."""
    g = _gen(31 * n + N + seed)
    target = torch.round((2 + 10 * torch.rand(n, generator=g)) * 1024) / 1024
    pred = target + torch.round(0.15 * torch.randn(n, generator=g) * 1024) / 1024
    rays = torch.rand(n, 15, generator=g) * 100
    k = min(2, N)
    if pattern == "one_owner":
        ids = torch.full((n,), float(k))
    else:
        ids = torch.randint(1, min(N, 7) + 1, (n,), generator=g).float()
        ids[torch.rand(n, generator=g) < 0.1] = float(N)
        plant = (0.0, N + 1.0, k + 0.4, k + 0.5, k + 0.6)
        for i in range(min(n, len(plant))):
            ids[(i + n) % min(n, len(plant))] = plant[i]
    rays[:, 9] = ids
    return pred, target, rays


def child_of(ids, N):
    """The child slot 0..N-1 of each id under the reference's comparison (train_kitti.py:131: id > i + 0.5 and
    id < i + 1.5, both strict, in float32 against exactly representable bounds), -1 for none: k + 0.4 belongs to
    child k (slot k - 1), k + 0.5 to no child, k + 0.6 to child k + 1 (slot k); 0 and N + 1 to none."""
    x = ids.double()
    s = torch.floor(x - 0.5)
    ok = (s >= 0) & (s < N) & (x > s + 0.5) & (x < s + 1.5)
    return torch.where(ok, s, torch.full_like(s, -1)).long()


def child_of_literal(ids, N):
    """child_of by the reference's loop, for the CPU test to hold the vectorised form against."""
    slot = torch.full(ids.shape, -1, dtype=torch.long)
    for i in range(N):
        slot[torch.logical_and(ids > (i + 0.5), ids < (i + 1.5))] = i
    return slot


def range_ref(pred, target, ids, N, kind, pre, post, dtype, g_out=1.0):
    """train_kitti.py:125-142 in ``dtype``: sum over the children that own >= 1 ray of post * mean over the child's
    rays of loss(pre * pred, pre * target); and autograd's d(g_out * loss)/dpred.  -> (loss, grad, slot)."""
    a = pred.to(dtype).clone().requires_grad_(True)
    slot = child_of(ids, N)
    own = slot >= 0
    if not bool(own.any()):
        return torch.zeros((), dtype=dtype), torch.zeros_like(a).detach(), slot
    v = elementwise_loss(pre * a, pre * target.to(dtype), kind)[own]
    s = slot[own]
    cnt = torch.zeros(N, dtype=dtype).index_add_(0, s, torch.ones(len(s), dtype=dtype))
    tot = torch.zeros(N, dtype=dtype).index_add(0, s, v)
    has = cnt >= 1
    loss = torch.sum(post * (tot[has] / cnt[has]))
    (g,) = torch.autograd.grad(loss * g_out, a)
    return loss.detach(), g, slot


def range_ref_literal(pred, target, ids, N, kind, pre, post):
    """The same loss by the reference's own loop and torch loss modules (float32), for the CPU test."""
    fn = {"mse": torch.nn.MSELoss(), "l1": torch.nn.L1Loss(), "smoothl1": torch.nn.SmoothL1Loss()}[kind]
    loss = torch.tensor([0.0])
    for i in range(N):
        m = torch.logical_and(ids > (i + 0.5), ids < (i + 1.5))
        if m.float().sum() >= 1:
            loss = loss + post * fn(pre * pred[m], pre * target[m])
    return loss


# ----------------------------------------------------------------------------------------------- group walk
WALK_ROWS = (1, 255, 256, 257, 513, 1000)


def literal_walk(other, at_peak, child_sum):
    """render.py:317-340 as written, on Python lists; -> flags.  Reading a row past the end raises IndexError in the
    reference: the walk ends there, with the flags it had set."""
    n = len(other)
    flag = [False] * n
    i = 0
    try:
        while i < n:
            if abs(other[i] - 0) < 0.5:
                flag[i] = True
                i = i + 1
            elif other[i] > 0.5:
                if at_peak[i]:
                    pick = i
                else:
                    pick = i
                    exist_peak = 0
                    for j in range(0, int(other[i])):
                        if at_peak[i + j + 1]:
                            pick = i + j + 1
                            exist_peak = 1
                            break
                    if exist_peak == 0:
                        for j in range(0, int(other[i])):
                            if child_sum[i + j + 1] > child_sum[pick]:
                                pick = i + j + 1
                flag[pick] = True
                i = i + int(other[i]) + 1
            else:
                i = i + 1
    except IndexError:
        pass
    return flag


def walk_forced(n):
    """The groups (head row, inner rows) a list of n rows can be made to hold at the 256-row block edge: a head in a
    block's last thread and in the next block's first, a group across the edge, a group ending on the last row."""
    cand = [(255, 3), (256, 4), (250, 10), (255, n - 256), (250, n - 251), (n - 4, 3)]
    return sorted({(h, o) for h, o in cand if h >= 0 and o >= 1 and h + o <= n - 1})


def walk_list(n, forced, seed):
    """A well-formed list: groups of 1..9 rows (other = rows after the head, then zeros), single rows with other 0
    and, outside the groups, with other -1; ``forced`` = (head, inner rows) or None is placed as given, and the last
    group ends on the last row.  at_peak: per group in turn on no row, on the head, on one inner row, on several rows;
    child_sum: small integers, so most groups hold ties for the strict > to resolve towards the earliest row.
    -> (other, at_peak, child_sum) tensors."""
    g = _gen(seed)
    other = [0] * n
    at_peak = [0] * n
    heads = []
    i = 0
    while i < n:
        past = forced is None or i > forced[0]
        room = (n - i - 1) if past else (forced[0] - i - 1)
        if not past and i == forced[0]:
            o = forced[1]
        elif past and 1 <= room <= 8:
            o = room                                      # the last group ends on the last row
        else:
            o = min(int(torch.randint(0, 9, (1,), generator=g)), room)
            if float(torch.rand(1, generator=g)) < 0.15:
                o = -1
        if o < 0:
            other[i] = -1
            at_peak[i] = int(torch.randint(0, 2, (1,), generator=g))
            i += 1
            continue
        other[i] = o
        if o > 0:
            heads.append(i)
        i += o + 1
    for k, h in enumerate(heads):
        o = other[h]
        if k % 4 == 1:
            at_peak[h] = 1
        elif k % 4 == 2:
            at_peak[h + 1 + int(torch.randint(0, o, (1,), generator=g))] = 1
        elif k % 4 == 3:
            for j in range(o + 1):
                at_peak[h + j] = int(torch.randint(0, 2, (1,), generator=g))
    child_sum = torch.randint(0, 4, (n,), generator=g).float()
    return torch.tensor(other), torch.tensor(at_peak, dtype=torch.uint8), child_sum


def walk_malformed():
    """name -> (other, at_peak, child_sum): lists the parallel path must refuse, each placed across a 256-row edge."""
    out = {}
    n = 300
    g = _gen(5)
    base = torch.zeros(n, dtype=torch.long)
    csum = torch.randint(0, 4, (n,), generator=g).float()
    peak0 = torch.zeros(n, dtype=torch.uint8)
    peak0[[251, 258]] = 1

    def put(name, edits, at_peak=peak0, other=base, cs=csum):
        o = other.clone()
        for k, v in edits.items():
            o[k] = v
        out[name] = (o, at_peak, cs)

    put("overlapping groups", {10: 4, 13: 3, 250: 6, 254: 5})
    put("head inside another group", {10: 5, 12: 1, 250: 9, 255: 2, 256: 1})
    put("negative inner row", {10: 3, 12: -1, 253: 5, 256: -1})
    put("negative row outside groups stays unflagged", {0: -1, 255: -1, 256: -2, 299: -1, 20: 2})
    # the last group runs past the end
    put("past the end, no peak in reach", {100: 2, 297: 5}, torch.zeros(n, dtype=torch.uint8))
    pk = torch.zeros(n, dtype=torch.uint8)
    pk[297] = 1
    put("past the end, peak on the head", {100: 2, 297: 5}, pk)
    pk = torch.zeros(n, dtype=torch.uint8)
    pk[299] = 1
    put("past the end, peak on an inner row in reach", {100: 2, 297: 5}, pk)
    put("a single row whose group runs past the end", {}, torch.zeros(1, dtype=torch.uint8),
        torch.tensor([3]), torch.ones(1))
    return out


def walk_opacity(n, S, seed):
    """Per-row opacity sums (float64) and their mean over n S elements."""
    op = torch.rand(n, generator=_gen(seed), dtype=torch.float64) * S * 0.4
    return op, float(op.sum() / (n * S))
