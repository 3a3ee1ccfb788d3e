"""Deterministic inputs of the per-kernel compositing / two-step tests, with their float64 and float32 reference
results (tests/render_f64.py) computed once per case and shared -- CPU only, so the conditions the inputs must meet
are also checked without a GPU (tests/test_render_f64_cpu.py)."""
import functools

import numpy as np
import torch

from nof import synthetic as syn
from oracle import ref_cpu as O

import render_f64 as F

EPS = 1e-10
N_CHILD = 4                      # sub_nerf_test_num: ids are 1 + r % 3, child 4 owns no ray
FB_S = (1, 2, 3, 63, 64, 65, 128, 129, 384, 385, 511, 513, 1024, 1025, 1536, 1537, 4095, 4096)
FWD_ONLY_S = (4097, 16384)
VIEW_S = (1, 3, 20, 21, 41, 64, 65, 129, 385, 1025, 4097, 5462, 8193)
RANGE_OFF = (0.05, -0.05, 0.3, -0.3)
GAP = 4.5                        # distance of row 1's child interval from the nearest sample on either side


E32_CAP = 2e-5                   # how far the float32 restatement may be from the float64 one, every case


def e32_cap(branch, key):
    """The cap on the float32 restatement's error for quantity ``key`` of one branch of a composite case.  2e-5,
    except for what is a function of x = 10 dc - 10 range alone (sl1_ray, the depth loss, and dL/dlogit when no
    depth gradient is given, where a row inside its child interval is driven by the depth loss only): the ranges
    put |x| at 0.5 or 3 while 10 dc is up to several hundred, so the cap holds for dc and reaches these through
    the cancellation, e(x) <= e(10 dc) |10 dc / x|, and the quadratic regime doubles it."""
    if key not in ("sl1_ray", "depth_loss"):
        return E32_CAP
    dc = branch["f64"]["dc"]
    x = 10 * dc - 10 * branch["rays"][:, 14].double()
    return E32_CAP * max(1.0, 2 * float((10 * dc / x).abs().max()))


def rays_for(S):
    return 3 if S in FWD_ONLY_S else (1, 5, 7)[FB_S.index(S) % 3]


def faint_rows(R):
    """The rows whose occupancies are faint and even, p = (0.5 + rand) 1.2 / S, so that the optical depth of the
    WHOLE row is 1.2: the only row of a one-ray case, rows 2, 3 and every odd row from 5 on otherwise (row 1's child
    masks end up holding one sample, which leaves it next to no child-loss gradient: it keeps the large weights).  With
    p = rand**8 the transmittance is gone after ~100 samples, and from there to the row's end weights and gradients
    are zero to float32: whatever a kernel does in the later lanes and across its wave boundaries would go unseen.
    A faint row keeps 30 % of its transmittance to its last sample, and every sample's weight and gradient is
    within a small factor of the row's largest (checked on the CPU: render_inputs.lane_reach)."""
    return [0] if R == 1 else [r for r in range(R) if r in (2, 3) or (r >= 5 and r % 2 == 1)]


def draw_rows(R, S, seed):
    """rays, sorted uniform z in [near, far] and occupancies p for R rays of S samples."""
    gen = torch.Generator().manual_seed(seed)
    rays = torch.from_numpy(syn.make_rays(R, seed=seed)).clone()
    z = torch.sort(rays[:, 6:7] + (rays[:, 7:8] - rays[:, 6:7]) * torch.rand(R, S, generator=gen), -1)[0]
    u = torch.rand(R, S, generator=gen)
    p = u ** 8 if S >= 64 else 0.05 + 0.9 * u   # S < 64: keeps sum w away from eps
    f = faint_rows(R)
    p[f] = (0.5 + u[f]) * (1.2 / max(S, 2))
    return gen, rays, z.contiguous(), p.contiguous()


def edge_rows(rays, z, p):
    """Rows 1-4 of a case with >= 5 rays (in place):
    1  the child interval sits in a gap of z (the samples from the middle on are moved up by 2 GAP + 0.2), GAP m from
       the nearest sample on either side: the thr0 = 0 loop runs ~450 steps, the thr0 = 2 loop ~250;
    2  the interval lies beyond z[-1];  3  before z[0];
    4  child_near is exactly z[4, k] for an early k (where the transmittance is still large) and child_far is below
       z[4, k + 1]: the inclusive mask holds exactly that sample, which carries a large weight (p = 0.5)."""
    S = z.shape[1]
    k = S // 2
    z[1, k:] += 2 * GAP + 0.2
    lo = z[1, k - 1] if k >= 1 else z[1, 0] - (2 * GAP + 0.2)
    rays[1, 10], rays[1, 11] = lo + GAP, z[1, k] - GAP
    rays[2, 10], rays[2, 11] = z[2, -1] + 0.7, z[2, -1] + 1.2
    rays[3, 10], rays[3, 11] = z[3, 0] - 1.2, z[3, 0] - 0.7
    k = min(S // 3, 3)
    rays[4, 10] = z[4, k]
    rays[4, 11] = 0.5 * (z[4, k] + z[4, k + 1]) if k + 1 < S else z[4, k] + 0.01
    p[4, k] = 0.5


def fair_draw(case):
    """Whether the float32 restatement's error in what depends on x = 10 dc - 10 range alone is a usable yardstick
    -- decided from the two references, nothing else.  The ranges put |x| at 0.5 or 3 while 10 dc is up to several
    hundred, so ONE float32 ulp of 10 dc moves sl1_ray by up to 1e-4 of itself, and no float32 evaluation, however it
    orders its sums, holds 10 dc - 10 range to better than an ulp or two (dc, 10 dc and 10 range each round once).
    e32 is one draw of that error per ray; where the restatement happens to land within a fraction of an ulp, 4 e32
    is below what any float32 arithmetic can keep and says nothing about a kernel.  A case is used when, in both
    branches, e32 of sl1_ray is at least what half an ulp of 10 dc does to the worst-placed ray (so the tolerance
    is two such ulps), and e32 of the gradients without dL/ddepth at least what half an ulp does to them
    (``x_noise`` counts 1.5)."""
    for name in ("plain", "divide"):
        br = case[name]
        dc = br["f64"]["dc"]
        x = (10 * dc - 10 * br["rays"][:, 14].double()).abs()
        ulp = torch.from_numpy(np.spacing(np.float32((10 * dc).abs().numpy())).astype(np.float64))
        one_ulp = float(torch.where(x < 1, 2 * ulp / x, ulp / (x - 0.5)).max())
        if F.err(br["f32"]["sl1_ray"], br["f64"]["sl1_ray"]) < 0.5 * one_ulp:
            return False
    if case["S"] in FB_S and case["S"] > 1:
        for name, (gd, gf, gl, g64, g32) in backward_refs_of(case, ("plain-nodepth", "divide-nodepth")).items():
            if F.err(g32, g64) < x_noise(case, name.split("-")[0], g64, gl) / 3:
                return False
    return True


@functools.lru_cache(maxsize=None)
def composite_case(S, R=None, seed=None, noisy=True):
    """The compositing case of S samples: ``draw_case`` with the given seed, or (seed None) with the first of the
    seeds S, S + 1000003, S + 2000006, ... whose float32 reference is a ``fair_draw``."""
    if seed is not None:
        return draw_case(S, rays_for(S) if R is None else R, seed, noisy)
    for k in range(64):
        case = draw_case(S, rays_for(S) if R is None else R, S + 1000003 * k, noisy)
        if fair_draw(case):
            return case
    raise AssertionError(f"no fair draw for S = {S}")


def draw_case(S, R, seed, noisy=True):
    """One compositing case: inputs for the plain and the divide branch and every reference result.
    -> dict with rays/z/p/masks and, per branch name ('plain', 'divide'), rays, noise, and the float64 / float32
    forward dicts ('f64', 'f32').  The divide branch carries noise (1e-3 randn, noise_std 1) unless ``noisy`` is
    False.  Treat everything returned as read-only."""
    gen, rays, z, p = draw_rows(R, S, seed)
    if S >= 2:
        # saturation: the U recurrence must not divide by 1 - p.  Early in row 0 (nothing of the row is left behind
        # it); in a one-ray case, whose row 0 is the faint one, on the last sample: it then carries the ~1/6 of the
        # transmittance that is left, and every earlier lane's gradient needs the suffix through all later lanes
        p[0, S - 1 if R == 1 else min(S // 2, 33)] = 1.0
    if R >= 5:
        edge_rows(rays, z, p)
    rays[:, 9] = 1 + torch.arange(R) % 3
    m0, m2, _ = F.masks(z, rays[:, 10], rays[:, 11])
    noise = 1e-3 * torch.randn(R, S, generator=torch.Generator().manual_seed(50000 + seed))
    case = {"S": S, "R": R, "seed": seed, "z": z, "p": p, "masks": (m0, m2)}
    for name, nz in (("plain", None), ("divide", noise if noisy else None)):
        r = rays.clone()
        divide = name == "divide"
        if divide and R >= 5:
            r[R - 1, 9], r[R - 2, 9] = 0.0, 9.0          # out of range: owned by no child
        # ranges from the float64 child depth: 10 dc - 10 range is +-0.5 or +-3, both SmoothL1 regimes, none at 1
        dc64 = F.composite_losses(p, z, nz, EPS, (m0, m2), r[:, 14], r[:, 9], divide, N_CHILD, torch.float64)["dc"]
        r[:, 14] = (dc64 + torch.tensor(RANGE_OFF, dtype=torch.float64)[torch.arange(R) % 4]).float()
        br = {"rays": r, "noise": nz, "divide": divide}
        for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
            br[key] = F.composite_losses(p, z, nz, EPS, (m0, m2), r[:, 14], r[:, 9], divide, N_CHILD, dt)
        case[name] = br
    return case


ULP32 = 2.0 ** -23               # the tests' floor is two of them


def grad_upstream(R, seed):
    """Upstream gradients (dL/ddepth per ray, dL/dfree, dL/d(depth loss)) before ``upstream`` scales the last."""
    gen = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(R, generator=gen), torch.tensor(1.0), torch.tensor(-0.25)


def x_noise(case, branch, g, g_dl):
    """How far float32 rounding of x = 10 dc - 10 range alone can move dL/dlogit ``g`` (float64), relative to each
    ray's largest entry, worst ray: a ray in the quadratic SmoothL1 regime gets its depth-loss gradient in
    proportion to x, which float32 holds to ~1.5 ulp of 10 dc (dc, 10 dc and 10 range each round once) -- 1e-5 to
    1e-4 of |x| = 0.5.  From the float64 reference alone."""
    br = case[branch]
    g_b = F.g_logit(case["p"], case["z"], br["noise"], EPS, case["masks"], br["rays"][:, 14], br["rays"][:, 9],
                    br["divide"], N_CHILD, torch.float64, g_dl=g_dl)
    dc = br["f64"]["dc"]
    x = (10 * dc - 10 * br["rays"][:, 14].double()).abs()
    scale = g.abs().amax(1)
    share = torch.where(scale > 0, g_b.abs().amax(1) / scale.clamp_min(1e-300), torch.zeros_like(scale))
    ulp = torch.from_numpy(np.spacing(np.float32((10 * dc).abs().numpy())).astype(np.float64))
    return float((share * (1.5 * ulp / x) * (x < 1)).max())


def upstream(case, branch, has_d, has_f, has_l):
    """The upstream gradients of one backward combination (None where absent).  Where a depth gradient is given,
    dL/d(depth loss) is halved from -0.25 until ``x_noise`` is within one float32 ulp: the test's tolerance is 4 x
    ONE float32 evaluation's error (floor: 2 ulps), and next to a well-conditioned depth term a depth-loss share
    that float32 can only hold to 1e-5 would make kernel and yardstick two draws of a lottery (the divide branch
    weights it (R / count)^2 more than the plain one).  The term stays >= 6e-5 of a quadratic row's gradient, 60 x
    the tolerance (-0.25 / 2^12 at the least; the combinations without a depth gradient carry it in full).  Without a depth gradient the value is -0.25 as it stands: scaling the only terms changes
    nothing."""
    gd, gf, gl = grad_upstream(case["R"], case["S"])
    if has_d and has_l and case["S"] > 1:
        br = case[branch]
        for _ in range(16):
            g = F.g_logit(case["p"], case["z"], br["noise"], EPS, case["masks"], br["rays"][:, 14], br["rays"][:, 9],
                          br["divide"], N_CHILD, torch.float64, gd, gf if has_f else None, gl)
            if x_noise(case, branch, g, gl) <= ULP32:
                break
            gl = gl / 2
    return gd if has_d else None, gf if has_f else None, gl if has_l else None


# (name, branch, g_depth given, g_free given, g_dl given, rays given)
BWD_COMBOS = (("plain", "plain", True, True, True, True), ("plain-nodepth", "plain", False, True, True, True),
              ("plain-nofree", "plain", True, False, True, True), ("divide", "divide", True, True, True, True),
              ("divide-nodl", "divide", True, True, False, True), ("divide-nodepth", "divide", False, True, True, True),
              ("depth-only", "plain", True, False, False, False))


def backward_refs_of(case, names=None):
    """{combo name: (g_depth, g_free, g_dl, g_logit float64, g_logit float32)} for a composite case (all of
    BWD_COMBOS, or ``names``)."""
    out = {}
    for name, branch, has_d, has_f, has_l, has_r in BWD_COMBOS:
        if names is not None and name not in names:
            continue
        br = case[branch]
        gd, gf, gl = upstream(case, branch, has_d, has_f, has_l) if has_r else (grad_upstream(case["R"], case["S"])[0],
                                                                                 None, None)
        args = (case["p"], case["z"], br["noise"], EPS, case["masks"] if has_r else None, br["rays"][:, 14],
                br["rays"][:, 9], br["divide"], N_CHILD)
        out[name] = (gd, gf, gl, F.g_logit(*args, torch.float64, gd, gf, gl), F.g_logit(*args, torch.float32, gd, gf, gl))
    return out


def lane_reach(S, q64, last_is_zero=False):
    """How much of a per-sample float64 result (R, S) lies where the kernels' lanes and waves end, for the group
    sizes 64 and 256 (thread t holds samples [t B, (t + 1) B), B = ceil(S / G)): -> {(G, place): the largest
    |q| / row maximum over the rows}, place 'last' for the last non-empty thread's samples and 'w<k>-' / 'w<k>+' for
    the sample before / after the boundary between waves k - 1 and k (G = 256).  ``last_is_zero``: the last sample is
    the saturated one of a one-ray case (gradient exactly 0), and 'last' also takes the sample before it."""
    rel = q64.abs() / q64.abs().amax(1, keepdim=True).clamp_min(1e-300)
    out = {}
    for G in (64, 256):
        B = -(-S // G)
        lo = (S - 1) // B * B
        out[G, "last"] = float(rel[:, (min(lo, S - 2) if last_is_zero else lo):].max())
        for k in range(1, G // 64):
            i = 64 * B * k
            if i < S - (1 if last_is_zero else 0):
                out[G, f"w{k}-"], out[G, f"w{k}+"] = float(rel[:, i - 1].max()), float(rel[:, i].max())
    return out


@functools.lru_cache(maxsize=None)
def backward_refs(S):
    return backward_refs_of(composite_case(S))


def first_rows(case, n):
    """The case made of the first n rays of ``case`` (same p, z, masks, noise and ranges), with its own references:
    the per-ray results are those rows', the scalar losses and dL/dlogit change with the ray count."""
    m0, m2 = case["masks"]
    sub = {"S": case["S"], "R": n, "z": case["z"][:n].contiguous(), "p": case["p"][:n].contiguous(),
           "masks": (m0[:n], m2[:n])}
    for name in ("plain", "divide"):
        b = case[name]
        br = {"rays": b["rays"][:n].contiguous(), "noise": None if b["noise"] is None else b["noise"][:n].contiguous(),
              "divide": b["divide"]}
        for key, dt in (("f64", torch.float64), ("f32", torch.float32)):
            br[key] = F.composite_losses(sub["p"], sub["z"], br["noise"], EPS, sub["masks"], br["rays"][:, 14],
                                         br["rays"][:, 9], br["divide"], N_CHILD, dt)
        sub[name] = br
    return sub


@functools.lru_cache(maxsize=None)
def view_case(S):
    """Five two-step rows of S samples: z sorted uniform in [parent_near, parent_far]; p a faint background with one
    dominant sample per row (the smoothed weight row has one clear peak) and a few percent behind it.
    row 0, 2  the dominant sample is the one nearest the child interval's middle;
    row 1     a sample (the dominant one) is set to exactly fl32(child_near - fl32(0.01)), the first strict bound,
              and (S >= 2) another to the middle of the child interval: the strict mask must leave the first out;
    row 3     the child interval sits in a 1 m gap of z, 0.45 m from either neighbour: the expansion loop runs;
    row 4     the dominant sample is the first one."""
    rows = torch.from_numpy(syn.make_view_rows(8, seed=S)[0][:5]).clone()
    assert rows.shape[0] == 5
    gen = torch.Generator().manual_seed(7000 + S)
    z = torch.sort(rows[:, 9:10] + (rows[:, 10:11] - rows[:, 9:10]) * torch.rand(5, S, generator=gen), -1)[0]
    # background of optical depth ~1 over the whole row, every p different (with p so small that fl32(0.1 + p) is
    # 0.1 the opacity terms would all round the same way and float32 would drift from float64 in proportion to S)
    p = (0.5 + torch.rand(5, S, generator=gen)) / max(S, 2)
    k = S // 2
    z[3, k:] += 1.0
    lo = z[3, k - 1] if k >= 1 else z[3, 0] - 1.0
    rows[3, 6], rows[3, 7] = lo + 0.45, z[3, k] - 0.45
    lo1 = rows[1, 6] - torch.tensor(0.01, dtype=torch.float32)      # float32: the kernel's first strict bound
    k1 = min(int((z[1] < lo1).sum()), S - 1)
    z[1, k1] = lo1
    if S >= 2:   # and a sample in the middle of the child interval: the loop stops at its first bound, at every S
        z[1, k1 + 1 if k1 + 1 < S else k1 - 1] = 0.5 * (rows[1, 6] + rows[1, 7])
    z = torch.sort(z, -1)[0].contiguous()
    k1 = int((z[1] == lo1).nonzero()[0])
    peak = [int(torch.argmin((z[r] - 0.5 * (rows[r, 6] + rows[r, 7])).abs())) for r in range(5)]
    peak[1], peak[3], peak[4] = k1, min(S - 1, k + 3), 0
    after = 0.02 + 0.05 * torch.rand(5, S, generator=gen)
    for r in range(5):
        # for 64 samples behind the dominant one p is a few percent: weights 100x below the peak's, and opacity terms of order
        # 1 (for p -> 0 the reference's log(0.1 + p) + log(1.1 - p) + 2.20727 cancels to ~2e-6, which float32
        # cannot hold to 2e-5 of the row sum)
        p[r, peak[r] + 1:peak[r] + 65] = after[r, peak[r] + 1:peak[r] + 65]
        p[r, peak[r]] = 0.8
    mv = F.masks(z, rows[:, 6], rows[:, 7])[2]
    case = {"S": S, "rows": rows, "z": z, "p": p.contiguous(), "mv": mv, "k1": k1}
    for method in (0, 2):
        case[method] = {key: F.view_rows(p, z, mv, method, EPS, dt)
                        for key, dt in (("f64", torch.float64), ("f32", torch.float32))}
    return case


def peak_reference(w32, mv):
    """-> (at_peak (R,) bool, unclear (R,) bool): the strict mask at argmax(gaussian_filter1d(w, 5, 'reflect'))
    (render.py:306-311) on float32 weights; a row is unclear when its two largest distinct smoothed values differ by
    less than one float32 ulp."""
    sm = O.gaussian_smooth(torch.as_tensor(w32).float().cpu())
    peak = torch.argmax(sm, dim=1)
    at = mv[torch.arange(sm.shape[0]), peak]
    unclear = []
    for row in sm.numpy():
        v = np.unique(row)[::-1]
        unclear.append(len(v) > 1 and float(v[0] - v[1]) < float(np.spacing(np.float32(v[0]))))
    return at, torch.tensor(unclear)


def child_reduce_case(R, N, seed):
    """Per-ray terms and child ids for the reduce kernels alone: ids drawn from 0..N+1 (0 and N+1 belong to no
    child; with N > R most children own no ray)."""
    gen = torch.Generator().manual_seed(seed)
    fr = torch.rand(R, generator=gen) ** 2
    sl = 3.0 * torch.rand(R, generator=gen)
    rays = torch.zeros(R, 15)
    rays[:, 9] = torch.randint(0, N + 2, (R,), generator=gen).float()
    return fr, sl, rays
