"""k_sample_coarse, k_perturb, k_sample_pdf, k_resample and the group walk (k_walk_cover / k_walk_pick /
k_walk_finish), each alone against the oracle (bit for bit where the reference's float32 arithmetic defines the
answer) or a float64 restatement (tests/sampling_f64.py: inputs, restatements and the conditions the inputs meet,
checked without a GPU in tests/test_sampling_f64_cpu.py), at the sizes where their lane blocks, waves per workgroup,
workgroup sizes and index arithmetic change.

The float64 comparisons follow parity_helpers.Tally: e_hip <= max(4 e32, 2.4e-7), e32 the same measure of the
float32 oracle on the CPU.  For the inverse-CDF draws the measure is the quantile identity |F(x_k) - u_k| with F the
exact float64 CDF -- continuous in u, so it has no bin-selection knife edge -- and, in the bins the reference
treats as empty (denom -> 1), the distance from b0 + (u - c0)(b1 - b0).
"""
import numpy as np
import pytest
import torch

from nof import _ops
from oracle import ref_cpu as O

import sampling_f64 as F
from parity_helpers import Tally

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ----------------------------------------------------------------------------------------------- k_sample_coarse
def test_coarse_plain_bitexact():
    """n_parent == S: z = near (1 - s) + far s, torch.equal with O.coarse_z, for every S of the sweep (1..130 and
    the lane-loop multiples around 192, 256, 768, 4096) and 1 / 3 / 4 / 5 / 9 rays (the last workgroup holds 1, 3,
    4, 1 and 1 of its 4 rays)."""
    for S in F.COARSE_S:
        for R in F.COARSE_R:
            t = F.coarse_table(R, S + R)
            got = _ops.sample_coarse(t.to(DEV), S, S, 6, 7, 10, 11).cpu()
            assert torch.equal(got, O.coarse_z(t, S, False, 0.0)), (S, R)


def test_coarse_disparity_bitexact():
    """use_disp: z = 1 / (1 / near (1 - s) + 1 / far s), bit for bit the float32 torch-CPU evaluation of
    render.py:565-567 (three correctly rounded divisions, one rounding per op), bounds from 0.5 to 80 m, the same
    sweep; and one table whose first row has near = 0 (inf in the reciprocal, NaN where it meets 1 - s = 0)."""
    for S in F.COARSE_S:
        for R in F.COARSE_R:
            t = F.coarse_table(R, 3 * S + R)
            got = _ops.sample_coarse(t.to(DEV), S, S, 6, 7, disparity=True).cpu()
            assert torch.equal(got, F.disparity_z(t, S)), (S, R)
    t = F.coarse_table(5, 7)
    t[0, 6] = 0.0
    for S in (1, 2, 5, 64, 65):
        got = _ops.sample_coarse(t.to(DEV), S, S, 6, 7, disparity=True).cpu()
        want = F.disparity_z(t, S)
        assert F.same_bits(got, want), S
        assert S == 1 or bool(torch.isnan(want[0, -1]))


def test_coarse_segmented_bitexact():
    """The merge of the parent and the child linspace, torch.equal with the sort of the two (O.coarse_z's branch):
    every S of the sweep from 2 on, n_parent in {1, 2, S - 1, S - 2, int(0.9 S), S // 2}, nine rays holding every
    child interval kind (inside the parent's, equal to it -- ties across the two lists in both binary searches --,
    disjoint below and above, zero width, reversed: the all-pairs rank fallback) and a second table of 1 / 3 / 4 / 5
    rays starting at another kind."""
    for i, S in enumerate(F.COARSE_S):
        for n_parent in F.parents_of(S):
            for R, first in ((9, 0), (F.COARSE_R[i % 4], i)):
                t = F.coarse_table(R, 5 * S + n_parent + R, first)
                got = _ops.sample_coarse(t.to(DEV), S, n_parent, 6, 7, 10, 11).cpu()
                assert torch.equal(got, F.segmented_z(t, S, n_parent)), (S, n_parent, R, first)


def test_coarse_permuted_columns():
    """A 9-column table with near / far / child near / child far in columns 3, 0, 8, 5: nothing depends on stride
    15 or columns 6, 7, 10, 11 (every other column of either table is noise)."""
    t = F.coarse_table(9, 11)
    p = F.permuted_table(t)
    near, far, cn, cf = F.PERM_COLS
    for S, n_parent in ((65, 32), (130, 117), (7, 1)):
        got = _ops.sample_coarse(p.to(DEV), S, n_parent, near, far, cn, cf).cpu()
        assert torch.equal(got, F.segmented_z(t, S, n_parent)), (S, n_parent)
        got = _ops.sample_coarse(p.to(DEV), S, S, near, far, cn, cf).cpu()
        assert torch.equal(got, O.coarse_z(t, S, False, 0.0)), S
        got = _ops.sample_coarse(p.to(DEV), S, S, near, far, cn, cf, disparity=True).cpu()
        assert torch.equal(got, F.disparity_z(t, S)), S


# ----------------------------------------------------------------------------------------------- k_perturb
@pytest.mark.parametrize("R,S", F.PERTURB_SHAPES)
def test_perturb_bitexact(R, S):
    """z' = lower + (upper - lower) (perturb rand) against O.perturb_z, bit for bit: one sample per row (lower and
    upper are both the sample), two, rows whose ends fall inside a 256-thread block ((7, 37): 259 elements, the
    g % S addressing with z[g +- 1] across the block edge), perturb 0 / 0.5 / 1, draws holding 0 and the largest
    float32 below 1, sorted rows and unsorted ones."""
    for sorted_rows in (True, False):
        z, rand = F.perturb_case(R, S, sorted_rows)
        for amount in F.PERTURB_AMOUNTS:
            got = _ops.perturb(z.to(DEV), amount, rand.to(DEV)).cpu()
            assert torch.equal(got, O.perturb_z(z, amount, rand)), (sorted_rows, amount)


# ----------------------------------------------------------------------------------------------- k_sample_pdf
@pytest.mark.parametrize("n_bins", F.PDF_BINS)
def test_sample_pdf_vs_f64(n_bins):
    """pcnerf_sample_pdf at one bin count -- 2 and 3 bins, the lane block B = ceil(npdf / 64) going 1 -> 2 -> 3 (64 ..
    67, 129, 130 bins: lanes with empty blocks), 4 -> 3 -> 2 -> 1 waves per workgroup (1365 / 1366, 1820 / 1821,
    2730 / 2731, 5461) -- with 1, 5 and waves + 1 rays (inactive waves in the last workgroup), 1 / 63 / 64 / 65 / 96
    draws, deterministic and given (u = 0, the largest float32 below 1, the middle of empty bins), rows of uniform,
    all-zero, one-hot 10, one-hot 0.1, zero-run and 1e-6 .. 1e3 weights.  Per launch:
    (a) the quantile identity |F(x) - u| over the draws whose candidate bins all hold >= 2e-5, and the distance from
        b0 + (u - c0)(b1 - b0) over the draws of a bin below 5e-6, both by Tally's rule against the float32 oracle;
        at most 2 % of the draws are neither;
    (b) element by element against O.sample_pdf outside the knife edges (at most 5 %), as test_sample_pdf does.
    Measured on the MI355X: over the 450 launches worst e_hip / max(4 e32, 2.4e-7) 0.33 (67 bins,
    one ray, 65 given draws: quantile e_hip 9.8e-8, e32 7.4e-8), worst e_hip / e32 above the floor 1.14; largest
    quantile error 1.65e-6 where the float32 oracle's is 2.07e-6 (both the float32 rounding of x in a heavy bin);
    denom -> 1 values off by at most 2.6e-8 of the row's largest edge, as the oracle's."""
    t = Tally("sample_pdf")
    kind0 = 0
    for R in F.pdf_rays(n_bins):
        for n in F.PDF_SAMPLES:
            for det in (True, False):
                bins, w, u = F.pdf_case(n_bins, R, n, det, kind0)
                kind0 += R
                got = _ops.sample_pdf_standalone(bins.to(DEV), w.to(DEV), n, det, None if det else u.to(DEV)).cpu()
                want = O.sample_pdf(bins, w, n, det, None if det else u)
                tag = f"b{n_bins}R{R}n{n}{'det' if det else 'u'}"
                e_hip, e32 = F.pdf_errors(bins, w, u, got), F.pdf_errors(bins, w, u, want)
                assert e_hip["unclear_share"] <= F.UNCLEAR_CAP, tag
                t.check_err(tag, "quantile", e_hip["quantile"], e32["quantile"])
                t.check_err(tag, "denom->1", e_hip["tiny"], e32["tiny"])
                edge = F.pdf_knife(bins, w, u)
                assert float(edge.float().mean()) <= F.KNIFE_CAP, tag
                ok = ~edge
                np.testing.assert_allclose(got[ok].numpy(), want[ok].numpy(), rtol=1e-4, atol=1e-5, err_msg=tag)
    t.done()


@pytest.mark.parametrize("long_row", [False, True])
def test_sample_pdf_draws_on_cdf_entries(long_row):
    """Draws exactly ON cdf entries whose value no evaluation can disagree about (sampling_f64.dyadic_case: dyadic
    weights, exact sums): searchsorted right=True puts the draw on entry j into bin j, and in the empty bins (denom
    -> 1) that returns edge j exactly -- 'cdf < u' for 'cdf <= u' in the kernel's search returns a point a bin
    before it.  Five rays (a second workgroup with three inactive waves), 5 and 69 bins (one and two per lane)."""
    bins, w, u, edges = F.dyadic_case(long_row)
    got = _ops.sample_pdf_standalone(bins.to(DEV), w.to(DEV), 4, False, u.to(DEV)).cpu()
    for k, j in enumerate(edges):
        assert torch.equal(got[:, k], bins[:, j]), (k, j)
    assert torch.equal(got, O.sample_pdf(bins, w, 4, False, u))


def test_sample_pdf_too_many_bins_refused():
    """5,462 bins: one ray's bins | weights | cdf no longer fit 64 KiB -- an error naming it, no launch."""
    bins = torch.sort(torch.rand(2, 5462, device=DEV), -1)[0]
    w = torch.rand(2, 5461, device=DEV)
    with pytest.raises(RuntimeError, match="too many bins"):
        _ops.sample_pdf_standalone(bins, w, 8, True)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- k_resample
def _resample_checks(t, S, n_imp):
    idx = 0
    for R in (1, 3):
        for mode in F.RESAMPLE_U:
            z, w, u = F.resample_case(R, S, n_imp, mode, idx)
            idx += 1
            zd, wd, ud = z.to(DEV), w.to(DEV), None if u is None else u.to(DEV)
            out = _ops.resample(zd, wd, n_imp, ud).cpu()
            tag = f"S{S}I{n_imp}R{R}{mode}"
            assert out.shape == (R, S + n_imp), tag
            e_hip = F.resample_errors(z, w, u, n_imp, out)
            assert e_hip["sorted"], tag + ": output row not non-decreasing"
            assert e_hip["contains_z"], tag + ": a coarse z is missing from the output"
            assert e_hip["unclear_share"] <= F.UNCLEAR_CAP, tag
            mid = 0.5 * (z[:, 1:] + z[:, :-1])
            fine32 = O.sample_pdf(mid, w[:, 1:-1], n_imp, u is None, u)
            e32 = F.resample_errors(z, w, u, n_imp, torch.sort(torch.cat([z, fine32], -1), -1)[0])
            t.check_err(tag, "quantile", e_hip["quantile"], e32["quantile"])
            # the fourth line: the sort of the coarse z and the draws of the stand-alone kernel, bit for bit
            fine = _ops.sample_pdf_standalone(mid.to(DEV), wd[:, 1:-1], n_imp, u is None, ud).cpu()
            assert torch.equal(out, torch.sort(torch.cat([z, fine], -1), -1)[0]), tag


@pytest.mark.parametrize("S", F.RESAMPLE_S)
def test_resample_coarse_counts(S):
    """pcnerf_resample with 37 draws at S = 3 (two mid-point bins, one weight), 4, 5, 63, 64, 65 (the lane block of
    the scan 1 -> 2 in a 64-thread workgroup) and 129; 1 and 3 rays; u sorted, unsorted and None (the deterministic
    draws); one row in three with two coarse entries swapped (the bitonic sort of the whole concatenation).  Three
    assertions that do not go through pcnerf_sample_pdf -- the output row is non-decreasing, holds the coarse z as a
    sub-multiset bit for bit, and the remaining values satisfy the quantile identity against the CDF built from
    mid(z) and w[1:-1] with the sorted u -- then the equality with sort(cat(z, sample_pdf_standalone)).
    Measured on the MI355X: worst e_hip / max(4 e32, 2.4e-7) 0.25 (S 64, unsorted u: e_hip 6.3e-8, e32 6.2e-8),
    e_hip / e32 above the floor 1.0 (the same float32 draws)."""
    t = Tally("resample_coarse_counts")
    _resample_checks(t, S, 37)
    t.done()


@pytest.mark.parametrize("n_imp", F.RESAMPLE_I)
def test_resample_fine_counts(n_imp):
    """The same assertions with I draws at S = 8 and S = 65: I = 1 (a one-slot bitonic sort), 2, 3, both sides of
    the fine list's power-of-two padding (63 .. 65, 255 .. 257) and of every workgroup-size step (511 / 512 / 513:
    64 -> 128 threads, 1023 .. 1025: 256, 2047 .. 2049: 512, where the float64 scan crosses waves through LDS).
    Measured on the MI355X: worst e_hip / max(4 e32, 2.4e-7) 0.35 (S 8, 511 deterministic draws: e_hip 1.4e-7,
    e32 1.0e-7), e_hip / e32 above the floor 1.0."""
    t = Tally("resample_fine_counts")
    for S in (8, 65):
        _resample_checks(t, S, n_imp)
    t.done()


def test_resample_lds_refused():
    """8,192 coarse and 16,384 fine samples need 224 KiB of LDS: an error naming it, no launch."""
    z = torch.sort(torch.rand(1, 8192, device=DEV), -1)[0]
    w = torch.rand(1, 8192, device=DEV)
    with pytest.raises(RuntimeError, match="LDS"):
        _ops.resample(z, w, 16384)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------- group walk
def _walk(other, at_peak, csum, n_samples=16, seed=1):
    n = other.numel()
    op, mean = F.walk_opacity(n, n_samples, seed)
    flags, opac = _ops.view_walk(other.to(DEV), at_peak.to(DEV), csum.to(DEV), op.to(DEV), n_samples)
    assert flags.shape == (n, 1) and flags.dtype == torch.bool
    # the opacity mean: within one float32 rounding of the float64 mean
    assert abs(float(opac) - mean) <= 2.0 ** -24 * abs(mean) * (1 + 1e-6), (float(opac), mean)
    return flags[:, 0].cpu().tolist()


@pytest.mark.parametrize("n", F.WALK_ROWS)
def test_view_walk_generated_lists(n):
    """Well-formed lists (the parallel path) of 1 .. 1000 rows against the literal walk of render.py:317-340, flag
    for flag: groups of 1 .. 9 rows, a head on row 255 (a block's last thread) and on row 256, a group over rows
    250 .. 260, the last group ending on the last row, at_peak on no row / the head / an inner row / several rows
    of a group, ties in child_sum (the strict > keeps the earliest row), negative rows outside the groups."""
    for k, forced in enumerate([None] + F.walk_forced(n)):
        other, at_peak, csum = F.walk_list(n, forced, 17 * n + k)
        want = F.literal_walk(other.tolist(), at_peak.tolist(), csum.tolist())
        assert _walk(other, at_peak, csum, seed=n + k) == want, (n, forced)


def test_view_walk_malformed_lists():
    """Lists the parallel path refuses -- overlapping groups, a head inside another group, a negative inner row,
    a last group running past the end -- give the sequential walk's flags.  Past the end the reference raises
    IndexError only when it READS a row that is not there: with the peak on the head, or on an inner row it reaches
    first, it flags that row and ends normally; otherwise the flags set before are kept and nothing is flagged
    after.  Before k_walk_finish looked for the peak among the rows that
    exist, it ended the walk as soon as a group reached past the end: 'peak on the head' left row 297 unflagged and
    'peak on an inner row in reach' row 299 (2 of the 8 lists failed; all 8 pass since)."""
    bad = []
    for name, (other, at_peak, csum) in F.walk_malformed().items():
        want = F.literal_walk(other.tolist(), at_peak.tolist(), csum.tolist())
        got = _walk(other, at_peak, csum)
        if got != want:
            bad.append(f"{name}: flags differ at rows {[i for i, (a, b) in enumerate(zip(got, want)) if a != b]}")
    assert not bad, "\n".join(bad)
