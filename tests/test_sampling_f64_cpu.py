"""The inputs and restatements of tests/sampling_f64.py, held against the float32 oracle without a GPU: every check
the GPU tests make of a kernel is made here of the oracle's own float32 result, so an input that float32 cannot
answer (too many unclear or knife-edge draws, a float32 error past render_inputs.E32_CAP) fails here first."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O

import render_inputs as I
import sampling_f64 as F


def test_coarse_inputs_cover_every_branch():
    """Every S of the sweep has a plain, a disparity and (from S = 2) a segmented case; the tables hold every child
    interval kind; the segmented reference is O.coarse_z's where that can be asked (n_parent = int(S (1 - ratio)));
    the permuted table gives the same z as the standard one."""
    assert F.parents_of(1) == [] and F.parents_of(2) == [1] and F.parents_of(130) == [1, 2, 65, 117, 128, 129]
    t = F.coarse_table(9, 3)
    near, far, cn, cf = (t[:, c] for c in F.STD_COLS)
    assert float(near.min()) == 0.5 and float(far.max()) == 80.0 and bool((far > near).all())
    assert bool((cn[0] >= near[0]) & (cf[0] <= far[0]) & (cn[0] < cf[0]))                 # inside
    assert cn[1] == near[1] and cf[1] == far[1] and cf[2] < near[2] and cn[3] > far[3]     # equal, below, above
    assert cn[4] == cf[4] and cn[5] > cf[5]                                                # zero width, reversed
    for S, ratio in ((64, 0.5), (130, 0.1), (7, 0.5)):
        sp = int(S * (1 - ratio))
        assert torch.equal(F.segmented_z(t, S, sp), O.coarse_z(t, S, True, ratio))
    p = F.permuted_table(t)
    assert p.shape[1] == 9 and torch.equal(F.segmented_z(p, 65, 32, F.PERM_COLS), F.segmented_z(t, 65, 32))
    assert F.same_bits(F.disparity_z(p, 65, F.PERM_COLS), F.disparity_z(t, 65))
    # near = 0: inf in the reciprocal, NaN where it meets 1 - s = 0, and same_bits still compares
    t0 = t.clone()
    t0[0, 6] = 0.0
    z = F.disparity_z(t0, 5)
    assert bool(torch.isnan(z[0, -1])) and float(z[0, 0]) == 0.0 and F.same_bits(z, z.clone())
    assert not F.same_bits(z, F.disparity_z(t, 5))


def test_coarse_checks_bite():
    """S for S - 1 in a linspace moves the values: the bit-for-bit comparisons see it at every S >= 3."""
    t = F.coarse_table(5, 1)
    for S in (3, 64, 130):
        s_bad = (torch.arange(S) / S).expand(5, S)
        near, far = t[:, 6:7], t[:, 7:8]
        assert not torch.equal(near * (1 - s_bad) + far * s_bad, O.coarse_z(t, S, False, 0))
        assert not F.same_bits(1 / (1 / near * (1 - s_bad) + 1 / far * s_bad), F.disparity_z(t, S))


def test_perturb_inputs():
    for R, S in F.PERTURB_SHAPES:
        z, rand = F.perturb_case(R, S)
        assert bool((z[:, 1:] >= z[:, :-1]).all()) and float(rand.max()) == F.NEXT1 < 1
        assert R * S == 1 or float(rand.min()) == 0.0
        out = O.perturb_z(z, 1.0, rand)
        assert out.shape == (R, S)
        if S == 1:
            assert torch.equal(out, z)                  # lower and upper are both the sample
    z, _ = F.perturb_case(7, 37, sorted_rows=False)
    assert not bool((z[:, 1:] >= z[:, :-1]).all())


@pytest.mark.parametrize("n_bins", F.PDF_BINS)
def test_pdf_inputs_within_the_caps(n_bins):
    """For every launch of the GPU test: the float32 oracle satisfies the quantile identity and the denom -> 1 value
    to E32_CAP, at most 2 % of the draws are unclear and at most 5 % knife-edged; over one bin count's launches
    every weight kind, the denom -> 1 branch and (from 64 bins) u = 0 and u just below 1 are reached."""
    kind0, n_tiny, worst, cdf_off, seen, top = 0, 0, 0.0, 0.0, set(), 0
    for R in F.pdf_rays(n_bins):
        for n in F.PDF_SAMPLES:
            for det in (True, False):
                bins, w, u = F.pdf_case(n_bins, R, n, det, kind0)
                seen |= {(k, det) for k in F.pdf_kinds(n_bins, R, n, det, kind0)}
                kind0 += R
                assert bool((bins[:, 1:] > bins[:, :-1]).all())
                if not det and n >= 2:
                    last_clear = F.cdf64(w)[:, -2] <= 1 - F.CLEAR
                    assert bool((u[:, 0] == 0).all()) and bool((u[last_clear, 1] == F.NEXT1).all())
                    top += int(last_clear.sum())
                x = O.sample_pdf(bins, w, n, det, None if det else u)
                e = F.pdf_errors(bins, w, u, x)
                tag = (n_bins, R, n, det)
                assert e["unclear_share"] <= F.UNCLEAR_CAP, (tag, e)
                assert float(F.pdf_knife(bins, w, u).float().mean()) <= F.KNIFE_CAP, tag
                assert e["quantile"] <= I.E32_CAP and e["tiny"] <= I.E32_CAP, (tag, e)
                n_tiny += e["n_tiny"]
                worst = max(worst, e["quantile"], e["tiny"])
                wf = w + 1e-5
                c32 = torch.cumsum(wf / wf.sum(-1, keepdim=True), -1)
                c64 = F.cdf64(w)[:, 1:]
                cdf_off = max(cdf_off, float(((c32.double() - c64).abs() / c64).max()))
    assert seen == {(k, det) for k in F.PDF_KINDS for det in (True, False)}
    assert cdf_off <= 0.6 * F.DELTA, cdf_off          # the float32 cdf stays inside classify's DELTA
    assert top >= 20                                  # rows with a draw just below 1
    if n_bins >= 64:
        assert n_tiny > 0


def _sample_pdf_lt(bins, weights, u):
    """O.sample_pdf with '<' for '<=' in the bin search (searchsorted right=False)."""
    wt = weights + 1e-5
    cdf = torch.cumsum(wt / wt.sum(-1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[..., :1]), cdf], -1)
    inds = torch.searchsorted(cdf, u.contiguous(), right=False)
    below, above = torch.clamp(inds - 1, min=0), torch.clamp(inds, max=cdf.shape[-1] - 1)
    lo, hi = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b0, b1 = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    den = hi - lo
    den = torch.where(den < 1e-5, torch.ones_like(den), den)
    return b0 + (u - lo) / den * (b1 - b0)


@pytest.mark.parametrize("long_row", [False, True])
def test_pdf_draws_on_cdf_entries(long_row):
    """dyadic_case is what it says: the oracle's float32 cdf holds the planted entries exactly, the draws on them
    return their edge exactly, and '<' for '<=' in the search returns a bin less for the entries of the empty bins --
    the one perturbation of the search that the quantile identity and the knife-edge-free comparison cannot see
    (neither fails on any of the 450 launches of test_pdf_inputs_within_the_caps with it: a draw differs only ON an
    entry, which is a knife edge unless the entry is exact)."""
    bins, w, u, edges = F.dyadic_case(long_row)
    wt = w + 1e-5
    total = 8.0 if long_row else 4.0
    assert float(wt[0].double().sum()) == total and float(wt[0].sum()) == total
    cdf = torch.cumsum(wt / wt.sum(-1, keepdim=True), -1)
    assert cdf[0, :3].tolist() == u[0, :3].tolist() and float(cdf[0, -1]) == 1.0
    x = O.sample_pdf(bins, w, 4, False, u)
    for k, j in enumerate(edges):
        assert torch.equal(x[:, k], bins[:, j])
    assert bool(((x[:, 3] > bins[:, 0]) & (x[:, 3] < bins[:, 1])).all())
    x_lt = _sample_pdf_lt(bins, w, u)
    assert bool((x_lt[:, 1] < bins[:, 2] - 0.4).all()) and bool((x_lt[:, 2] < bins[:, 3] - 0.4).all())


def test_pdf_quantile_check_bites():
    """A draw moved by a bin and a half is seen by the quantile identity."""
    bins, w, u = F.pdf_case(65, 5, 64, False, 0)
    x = O.sample_pdf(bins, w, 64, False, u)
    shifted = x.clone()
    shifted[:, 5] = x[:, 5] + 1.5 * (bins[:, 2] - bins[:, 1])
    assert F.pdf_errors(bins, w, u, x)["quantile"] <= I.E32_CAP
    assert F.pdf_errors(bins, w, u, shifted)["quantile"] > 1e-3


@pytest.mark.parametrize("S,n_imp", [(S, 37) for S in F.RESAMPLE_S] + [(S, n) for n in F.RESAMPLE_I for S in (8, 65)])
def test_resample_inputs_within_the_caps(S, n_imp):
    """The oracle's own sort(cat(z, sample_pdf)) passes the three assertions the GPU test makes, to E32_CAP and
    with no unclear draw to speak of; a row with a swapped pair is present among the cases of each size."""
    idx, swapped = 0, 0
    for R in (1, 3):
        for mode in F.RESAMPLE_U:
            z, w, u = F.resample_case(R, S, n_imp, mode, idx)
            swapped += int((z[:, 1:] < z[:, :-1]).any())
            idx += 1
            mid = 0.5 * (z[:, 1:] + z[:, :-1])
            assert bool((mid[:, 1:] > mid[:, :-1]).all())
            xs = O.sample_pdf(mid, w[:, 1:-1], n_imp, u is None, u)
            out = torch.sort(torch.cat([z, xs], -1), -1)[0]
            e = F.resample_errors(z, w, u, n_imp, out)
            assert e["sorted"] and e["contains_z"], (R, mode)
            assert e["unclear_share"] <= F.UNCLEAR_CAP and e["quantile"] <= I.E32_CAP, (R, mode, e)
            # and the checks bite: a coarse value nudged by an ulp, a fine value moved by a bin
            bad = out.clone()
            k = int((bad[0] == z[0, 0]).nonzero()[0])
            bad[0, k] = float(np.nextafter(np.float32(bad[0, k]), np.float32(100)))
            assert not F.resample_errors(z, w, u, n_imp, bad)["contains_z"]
    assert swapped >= 2


@pytest.mark.parametrize("n", F.LOSS_N)
def test_loss_inputs(n):
    """The planted pairs are exact in float32 and sit where planted_exact says; the float32 torch losses stay
    within E32_CAP of float64 for every mask and kind; elementwise_loss is torch's loss."""
    pred, target, where, which = F.loss_case(n)
    for i, p in zip(where, which):
        assert (float(pred[i]), float(target[i])) == tuple(float(np.float32(v)) for v in F.PLANTED[p])
    d = [float(np.float32(a)) - float(np.float32(b)) for a, b in F.PLANTED]
    assert d[0] == 0 and d[1] == 1 and d[2] == -1 and d[3] == 1 - 2.0 ** -24 and d[4] == 1 + 2.0 ** -23
    assert d[5] == -d[3] and d[6] == -d[4]
    assert F.planted_exact(3, "smoothl1")[1] == np.float32(d[3]) and F.planted_exact(1, "smoothl1") == (0.5, 1.0)
    assert F.planted_exact(4, "smoothl1") == (np.float32(d[4] - 0.5), 1.0) and F.planted_exact(0, "l1") == (0.0, 0.0)
    for kind in F.LOSS_KINDS:
        for name in F.LOSS_MASKS:
            m = F.loss_mask(name, n)
            l64, g64 = F.pointwise_ref(pred, target, kind, m, torch.float64)
            l32, g32 = F.pointwise_ref(pred, target, kind, m, torch.float32)
            if m is not None and not bool(m.any()):
                assert bool(torch.isnan(l64)) and bool(torch.isnan(l32)) and not bool(g64.any())
                continue
            sel = slice(None) if m is None else m
            mine = F.elementwise_loss(pred.double()[sel], target.double()[sel], kind).mean()
            assert abs(float(mine) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64)))
            from render_f64 import err
            assert err(l32, l64) <= I.E32_CAP and err(g32, g64) <= I.E32_CAP, (kind, name)


@pytest.mark.parametrize("N", F.RANGE_CHILDREN)
@pytest.mark.parametrize("n", F.RANGE_N)
def test_range_loss_restatement(n, N):
    """child_of against the reference's loop, range_ref (float32) against the reference's loop with torch's loss
    modules, and float32 within E32_CAP of float64; the planted ids land where child_of's docstring says."""
    from render_f64 import err
    k = min(2, N)
    ids = torch.tensor([0.0, N + 1.0, k + 0.4, k + 0.5, k + 0.6, 1.0, float(N)])
    want = [-1, -1, k - 1, -1, k if k < N else -1, 0, N - 1]
    assert F.child_of(ids, N).tolist() == want
    for pattern in F.RANGE_PATTERNS:
        pred, target, rays = F.range_case(n, N, pattern)
        ids = rays[:, 9]
        slot = F.child_of(ids, N)
        if N <= 1500:
            assert torch.equal(slot, F.child_of_literal(ids, N))
        if pattern == "one_owner":
            assert bool((slot == k - 1).all())
        elif n >= 255:
            assert bool((slot < 0).any()) and (N < 1500 or len(torch.unique(slot[slot >= 0])) < N)
        for kind in F.LOSS_KINDS:
            l64, g64, _ = F.range_ref(pred, target, ids, N, kind, F.RANGE_PRE, 0.1, torch.float64, 0.7)
            l32, g32, _ = F.range_ref(pred, target, ids, N, kind, F.RANGE_PRE, 0.1, torch.float32, 0.7)
            assert bool((g64[slot < 0] == 0).all())
            if not bool((slot >= 0).any()):
                assert float(l64) == 0
                continue
            assert err(l32, l64) <= I.E32_CAP and err(g32[None], g64[None]) <= I.E32_CAP, (pattern, kind)
            if N <= 1500:
                lit = F.range_ref_literal(pred, target, ids, N, kind, F.RANGE_PRE, 0.1)
                np.testing.assert_allclose(float(lit), float(l32), rtol=1e-5)


def _walk_cases():
    for n in F.WALK_ROWS:
        for k, forced in enumerate([None] + F.walk_forced(n)):
            yield n, forced, 17 * n + k


def test_walk_lists_are_what_they_claim():
    """The generated lists are well formed (every group's inner rows are 0, groups disjoint and inside the list, the
    last one ending on the last row), place heads on rows 255 and 256 and a group across 250..260, hold every
    at_peak pattern, ties in child_sum and negative rows; the malformed lists are malformed."""
    seen_heads, patterns, ties, negatives = set(), set(), 0, 0
    for n, forced, seed in _walk_cases():
        other, at_peak, csum = F.walk_list(n, forced, seed)
        o = other.tolist()
        i = 0
        while i < n:
            if o[i] > 0:
                assert i + o[i] <= n - 1 and all(v == 0 for v in o[i + 1:i + o[i] + 1]), (n, forced, i)
                seen_heads.add((i, o[i]))
                grp = at_peak[i:i + o[i] + 1].tolist()
                patterns.add("none" if not any(grp) else "head" if grp[0] and sum(grp) == 1 else
                             "inner" if sum(grp) == 1 else "several")
                ties += len(set(csum[i:i + o[i] + 1].tolist())) < o[i] + 1
                i += o[i] + 1
            else:
                negatives += o[i] < 0
                i += 1
        if n > 1:
            assert any(h + k == n - 1 for h, k in seen_heads), (n, forced)
        if forced is not None:
            assert o[forced[0]] == forced[1]
        flags = F.literal_walk(o, at_peak.tolist(), csum.tolist())
        assert sum(flags) == sum(1 for v in o if v == 0) - sum(v for v in o if v > 0) + sum(1 for v in o if v > 0)
    assert {(255, 3), (256, 4), (250, 10)} <= seen_heads
    assert patterns == {"none", "head", "inner", "several"} and ties > 20 and negatives > 20
    # the hand-written case of test_view_walk_fallback_matches_parallel
    at = [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0]
    cs = list(range(11, -1, -1))
    nz = lambda f: [i for i, v in enumerate(f) if v]
    assert nz(F.literal_walk([2, 0, 0, 0, 3, 0, 0, 0, 1, 0, 0, 0], at, cs)) == [2, 3, 6, 8, 10, 11]
    assert nz(F.literal_walk([2, 1, 0, 0, 3, 0, -1, 0, 0, 0, 0, 0], at, cs)) == [2, 3, 6, 8, 9, 10, 11]
    bad = F.walk_malformed()
    assert len(bad) == 8
    o, p, c = bad["past the end, no peak in reach"]
    f = F.literal_walk(o.tolist(), p.tolist(), c.tolist())
    assert not any(f[297:]) and all(f[103:297]) and sum(f[100:103]) == 1
    for name, first in (("past the end, peak on the head", 297), ("past the end, peak on an inner row in reach", 299)):
        o, p, c = bad[name]
        f = F.literal_walk(o.tolist(), p.tolist(), c.tolist())
        assert nz(f[297:]) == [first - 297], name     # the reference never reads past the end there
    o, p, c = bad["a single row whose group runs past the end"]
    assert F.literal_walk(o.tolist(), p.tolist(), c.tolist()) == [False]


def test_walk_check_bites():
    """'>=' for '>' in the group pick moves the flag to the last of tied rows: the flags differ on the first list."""
    def walk_ge(other, at_peak, child_sum):
        class GE(float):
            def __gt__(self, o):
                return float(self) >= float(o)
        return F.literal_walk(other, at_peak, [GE(v) for v in child_sum])
    other, at_peak, csum = F.walk_list(257, None, 1)
    args = other.tolist(), at_peak.tolist(), csum.tolist()
    assert walk_ge(*args) != F.literal_walk(*args)
