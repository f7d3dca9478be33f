"""CPU: the restatement of the normal estimation (tests/normals_reference.py) against independent facts, and mutants of it
against the criteria tests/test_gpu_normals.py applies to the kernels: each criterion fails on the input named for it, so the
GPU tests' bounds are not vacuous."""
import numpy as np
import pytest

import normals_reference as R


@pytest.fixture(scope="module")
def room2048():
    xyz = R.room(2048)
    return xyz, R.knn(xyz, 16)


def test_fma32_rounds_once():
    """the emulated f32 fma equals the exactly rounded a * b + c (python's integers), also where the f64 sum is a tie"""
    from fractions import Fraction
    rng = np.random.RandomState(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.randint(-12, 3, 4000)).astype(np.float32)
    a[:3], b[:3] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12)     # 1 + 2^-11 + 2^-24: an f32 tie once c is added
    c[:3] = (2.0 ** -30, -2.0 ** -30, 0.0)
    got = R.fma32(a, b, c)
    for i in range(4000):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                  # float(Fraction) rounds once to f64; settle the f32 neighbours exactly
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        errs = [abs(Fraction(float(v)) - exact) for v in cands]
        best = min(errs)
        winners = [v for v, e in zip(cands, errs) if e == best]
        if len(winners) == 2:                          # a true tie: to even
            winners = [v for v in winners if (v.view(np.uint32) & 1) == 0]
        assert got[i] == winners[0], (i, a[i], b[i], c[i])


def test_neighbour_sets_equal_ckdtree_where_the_kth_place_has_no_tie():
    from scipy.spatial import cKDTree
    rng = np.random.RandomState(1)
    xyz = (rng.rand(1500, 3) * [4.0, 4.0, 2.5]).astype(np.float32)
    k = 16
    idx, d2 = R.knn(xyz, k + 1)
    clear = d2[:, k] > d2[:, k - 1] * (1 + 1e-5)                               # the (k+1)-th is clearly farther
    assert clear.mean() > 0.95
    _, tree = cKDTree(xyz.astype(np.float64)).query(xyz.astype(np.float64), k)
    assert (np.sort(idx[clear, :k], 1) == np.sort(tree[clear], 1)).all()
    assert (idx[:, 0] == np.arange(1500)).all() and (d2[:, 0] == 0).all()     # the point itself leads its row
    assert (np.diff(d2.astype(np.float64), axis=1) >= 0).all()


def test_rows_are_ordered_by_distance_then_index_and_short_clouds_pad():
    import synth
    xyz = synth.adversarial_cloud(1, 1, 1024)[0].numpy()
    idx, d2 = R.knn(xyz, 100)
    same = d2[:, 1:] == d2[:, :-1]
    assert same.any() and (idx[:, 1:][same] > idx[:, :-1][same]).all()
    full, d2f = R.knn(xyz, 101)
    ties = (d2f[:, 100] == d2f[:, 99]).mean()
    assert 0.01 < ties < 0.2, ties                                            # the k-th-place tie rule is exercised
    idx5, d5 = R.knn(xyz[:5], 8)
    assert (idx5[:, 5:] == -1).all() and np.isinf(d5[:, 5:]).all() and (np.sort(idx5[:, :5], 1) == np.arange(5)).all()
    idx0, d0 = R.knn(xyz[:0], 4, queries=xyz[:3])
    assert (idx0 == -1).all() and np.isinf(d0).all()


def test_noiseless_tilted_plane_gives_its_normal():
    """z = x / 2 + y / 4 on a dyadic lattice: every coordinate is exact in f32"""
    g = np.arange(-8, 9) / 64.0
    x, y = np.meshgrid(g, g, indexing="ij")
    xyz = np.stack([x.ravel() + 1.0, y.ravel() - 2.0, 0.5 * x.ravel() + 0.25 * y.ravel() + 0.75], 1).astype(np.float32)
    idx, _ = R.knn(xyz, 24)
    nrm, vec, eig = R.plane_fit(xyz, idx)
    want = np.array([-0.5, -0.25, 1.0]) / np.linalg.norm([-0.5, -0.25, 1.0])
    assert R.angle(vec, want).max() < 1e-12
    assert np.abs(eig[:, 0]).max() < 1e-18 and R.canonical(nrm).all() and (nrm[:, 2] > 0).all()
    assert np.abs(np.linalg.norm(vec, axis=1) - 1).max() < 1e-14


def test_plane_fit_degenerate_rows_give_finite_unit_vectors():
    xyz = np.zeros((40, 3), np.float32) + np.float32(0.3)
    xyz[30:] = np.arange(10, dtype=np.float32)[:, None] * np.float32(0.125)    # collinear
    nrm, _, _ = R.plane_fit(xyz, R.knn(xyz, 8)[0])
    assert np.isfinite(nrm).all() and np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_orientation_rule(room2048):
    xyz, (idx, _) = room2048
    nrm = R.plane_fit(xyz, idx)[0]
    c = R.view_centre(xyz)
    xyz, nrm = xyz.copy(), nrm.copy()
    xyz[:4] = c.astype(np.float32)                                             # dot == 0 up to the centre's f32 rounding ...
    c32 = c.astype(np.float32).astype(np.float64)
    out = R.orient(xyz, nrm, c32)                                              # ... and exactly with the rounded centre
    flips, dot = R.orient_flips(xyz, nrm, c32)
    assert (dot[:4] == 0).all() and not flips[:4].any() and 0.2 < flips.mean() < 0.8
    assert (out[flips] == -nrm[flips]).all() and (out[~flips] == nrm[~flips]).all()
    assert (R.orient_flips(xyz, out, c32)[1] >= 0).all()
    assert np.allclose(c, [xyz[4:, 0].mean(), xyz[4:, 1].mean(), (xyz[:, 2].max() + xyz[4:, 2].mean()) / 2], atol=0.05)


def test_smoothing_aligns_and_keeps_unit_length(room2048):
    xyz, (idx, _) = room2048
    nrm = R.plane_fit(xyz, idx)[0]
    out, votes = R.smooth_step(nrm, idx)
    assert (votes[:, 0] == 1).all() and np.abs(np.linalg.norm(out.astype(np.float64), axis=1) - 1).max() < 1e-6
    flipped = np.where(np.arange(2048)[:, None] % 2 == 0, nrm, -nrm)           # the sign of the inputs does not matter ...
    out2, _ = R.smooth_step(flipped, idx)
    assert (R.angle(out, out2) < 1e-6).all()                                   # ... to the line of the result


# ---- mutants: each criterion of tests/test_gpu_normals.py fails on the input named for it ----------------------------------
def test_mutant_vote_ge_fails_the_smoothing_criterion(room2048):
    _, (idx, _) = room2048
    nrm, rows = R.smooth_inputs(idx)
    want, votes = R.smooth_step(nrm, rows)
    got, mvotes = R.smooth_step(nrm, rows, vote_ge=True)
    assert votes[3, 1] == -1 and mvotes[3, 1] == 1 and (want[0] == nrm[0]).all()
    assert R.ulp_distance(got, want).max() > 1                                  # the criterion: <= 1 ulp per component


def test_mutant_unaligned_averaging_fails_the_smoothing_criterion(room2048):
    _, (idx, _) = room2048
    nrm, rows = R.smooth_inputs(idx)
    want, _ = R.smooth_step(nrm, rows)
    got, _ = R.smooth_step(nrm, rows, unaligned=True)
    assert (R.ulp_distance(got, want).max(1) > 1).mean() > 0.9


def test_mutant_without_self_fails_the_exact_neighbour_criterion(room2048):
    xyz, (idx, d2) = room2048
    midx, md2 = R.knn(xyz, 16, skip_self=True)
    assert not np.array_equal(midx, idx) and not np.array_equal(md2, d2)        # the criterion: bit-equal idx and dist2
    assert (midx != np.arange(2048)[:, None]).all()


def test_mutant_f32_mean_fails_the_eigenvalue_bound(room2048):
    """An f32 mean moves C by its error SQUARED (the covariance is taken about that mean, the first-order term sums to zero):
    ~1e-12 relative, which the f32 store of the normal (6e-8 rad) hides -- measured here: the mutant's normals stay within the
    angle bound -- but not the f64 eigenvalues the kernel also returns."""
    xyz, (idx, _) = room2048
    honest, vec, eig = R.plane_fit(xyz, idx)
    keep = ~R.plane_fit_excluded(eig)
    assert keep.mean() >= 0.995
    assert (R.angle(honest, vec)[keep] <= R.plane_fit_bound(eig, 16)[keep]).all()   # the restatement's own f32 output passes
    _, _, meig = R.plane_fit(xyz, idx, mean_f32=True)
    assert (np.abs(meig - eig).max(1) > R.eig_bound(eig, 16)).mean() > 0.2      # the criterion: every point within it
