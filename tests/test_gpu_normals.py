"""GPU: csrc/point_normals.hip through the C ABI (include/omnipq_normals.h) against the float64 / numpy-f32 restatement
tests/normals_reference.py, stage by stage and composed, and the route through pointnet2_utils, point_normals and SceneBank.

Criteria (tests/test_normals_reference.py shows on the CPU that each one can fail):
  knn        idx and dist2 bit-equal to the brute-force restatement (f32 d2 with the contract's contraction, ties by index).
  plane_fit  angle(gpu f32, restatement's unrounded f64 eigenvector) <= theta_f32-store + c 2^-53 trace(C) / (lambda_1 - lambda_0)
             and |eigenvalue - restatement's| <= c 2^-53 trace(C), c = normals_reference.plane_fit_ops(k): counted there from the
             kernel's operations (k + 4 roundings per entry of C, 8 per entry and Jacobi rotation, Davis-Kahan's 2, the
             restatement's own share 2).  Angles are atan2(|a x b|, |a . b|), never arccos.  Points with
             (lambda_1 - lambda_0) < 1e-6 lambda_2 in the restatement are left out (at most 0.5 %).
  smooth     every component within 1 f32 ulp of the restatement, which takes every vote s_ij exactly as stated (one wrong
             vote moves the sum by 2 n_j: thousands of ulps); bit-equality is printed, not required.
  orient     bit-equal (a sign decision in f64 without contraction and a negation).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import capi
import normals_reference as R
import synth

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda")


def t(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).to(dev()).contiguous()


def bytes_of(name, *sizes):
    fn = getattr(capi.lib(), name)
    fn.restype = ctypes.c_longlong
    return int(fn(*sizes))


def knn_gpu(xyz, k, cell, queries=None, want_dist=True):
    """xyz (b, n, 3), queries (b, m, 3) or None -> numpy idx, dist2; outputs pre-filled with garbage"""
    x = t(xyz, torch.float32)
    q = x if queries is None else t(queries, torch.float32)
    b, n, m = x.shape[0], x.shape[1], q.shape[1]
    idx = torch.full((b, m, k), -7, dtype=torch.int32, device=dev())
    d2 = torch.full((b, m, k), -7.0, dtype=torch.float32, device=dev())
    ws = torch.empty(max(bytes_of("omnipq_knn_workspace_bytes", b, n, m), 16), dtype=torch.uint8, device=dev())
    capi.ok("omnipq_knn", b, n, m, k, ctypes.c_float(cell), capi.P(q), capi.P(x), capi.P(idx), capi.P(d2) if want_dist else None,
            capi.P(ws))
    return idx.cpu().numpy(), d2.cpu().numpy()


def plane_fit_gpu(xyz, idx, eig=True):
    x, i = t(xyz[None], torch.float32), t(idx[None], torch.int32)
    n, k = idx.shape
    out = torch.full((1, n, 3), 7.0, dtype=torch.float32, device=dev())
    ev = torch.full((1, n, 3), 7.0, dtype=torch.float64, device=dev())
    capi.ok("omnipq_normals_plane_fit", 1, n, k, capi.P(x), capi.P(i), capi.P(out), capi.P(ev) if eig else None)
    return out[0].cpu().numpy(), ev[0].cpu().numpy()


def smooth_gpu(nrm, idx, iters):
    i = t(idx[None], torch.int32)
    n, k = idx.shape
    cur, nxt = t(nrm[None], torch.float32), torch.full((1, n, 3), 7.0, dtype=torch.float32, device=dev())
    for _ in range(iters):
        capi.ok("omnipq_normals_smooth", 1, n, k, capi.P(i), capi.P(cur), capi.P(nxt))
        cur, nxt = nxt, cur
    return cur[0].cpu().numpy()


def orient_gpu(xyz, nrm, centre):
    x, v, c = t(xyz[None], torch.float32), t(nrm[None], torch.float32), t(np.asarray(centre, np.float64)[None], torch.float64)
    capi.ok("omnipq_normals_orient", 1, xyz.shape[0], capi.P(x), capi.P(c), capi.P(v))
    return v[0].cpu().numpy()


def estimate_gpu(xyz, k, iters, cell, centre):
    x, c = t(xyz, torch.float32), t(centre, torch.float64)
    b, n = x.shape[0], x.shape[1]
    out = torch.full((b, n, 3), 7.0, dtype=torch.float32, device=dev())
    ws = torch.empty(max(bytes_of("omnipq_estimate_normals_workspace_bytes", b, n, k), 16), dtype=torch.uint8, device=dev())
    capi.ok("omnipq_estimate_normals", b, n, k, iters, ctypes.c_float(cell), capi.P(x), capi.P(c), capi.P(out), capi.P(ws))
    return out.cpu().numpy()


# ---- references, computed once ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adversarial():
    """synth.adversarial_cloud(1, 2, 1024): duplicates, a lattice of equal distances, a dense cluster, an outlier at 50 --
    and the restatement's rows for k = 128 (the rows for a smaller k are their first k entries)"""
    xyz = synth.adversarial_cloud(1, 2, 1024).numpy()
    ref = [R.knn(xyz[s], 128) for s in range(2)]
    return xyz, np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref])


@functools.lru_cache(maxsize=None)
def room_rows(n, k):
    xyz = R.room(n)
    idx, d2 = R.knn(xyz, k)
    for a in (xyz, idx, d2):
        a.setflags(write=False)
    return xyz, idx, d2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- knn ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [0.01, 0.2, 100.0])      # shell growth then the walk | the normal path | all in one cell
@pytest.mark.parametrize("k", [1, 8, 64, 100, 128])
def test_knn_is_exact_on_the_adversarial_cloud(k, cell):
    xyz, want_idx, want_d2 = adversarial()
    idx, d2 = knn_gpu(xyz, k, cell)
    assert np.array_equal(idx, want_idx[:, :, :k])
    assert np.array_equal(bits(d2), bits(want_d2[:, :, :k]))


@pytest.mark.parametrize("k", [1, 100, 128])
def test_knn_more_candidates_than_the_list_holds(k):
    """2048 points in one cell (and 4096 room points in a few): past the 1024 candidates a wave keeps in LDS the selection
    reads the grid again on every pass"""
    xyz = synth.adversarial_cloud(2, 1, 2048).numpy()
    want_idx, want_d2 = R.knn(xyz[0], k)
    idx, d2 = knn_gpu(xyz, k, 100.0)
    assert np.array_equal(idx[0], want_idx) and np.array_equal(bits(d2[0]), bits(want_d2))
    xyz, want_idx, want_d2 = room_rows(4096, 100)
    kr = min(k, 100)                                                           # the shared room rows hold 100 neighbours
    idx, d2 = knn_gpu(xyz[None], kr, 2.5)
    assert np.array_equal(idx[0], want_idx[:, :kr]) and np.array_equal(bits(d2[0]), bits(want_d2[:, :kr]))


def test_knn_tie_rule_is_exercised():
    _, _, want_d2 = adversarial()
    ties = (want_d2[:, :, 100] == want_d2[:, :, 99]).mean()
    assert 0.01 < ties < 0.2


@pytest.mark.parametrize("cell", [0.05, 0.3])
def test_knn_separate_query_set(cell):
    xyz, _, _ = adversarial()
    rng = np.random.RandomState(5)
    q = np.concatenate([xyz[:, 500:520] + np.float32(1e-3), rng.uniform(-1.2, 1.2, (2, 17, 3)).astype(np.float32)], 1)   # m = 37
    idx, d2 = knn_gpu(xyz, 16, cell, queries=q)
    for s in range(2):
        want_idx, want_d2 = R.knn(xyz[s], 16, queries=q[s])
        assert np.array_equal(idx[s], want_idx) and np.array_equal(bits(d2[s]), bits(want_d2))


def test_knn_short_and_empty_clouds_pad_with_minus_one_and_inf():
    xyz, _, _ = adversarial()
    for cell in (0.2, 100.0):
        idx, d2 = knn_gpu(xyz[:, 100:105], 8, cell)                            # n = 5, k = 8
        for s in range(2):
            want_idx, want_d2 = R.knn(xyz[s, 100:105], 8)
            assert np.array_equal(idx[s], want_idx) and np.array_equal(bits(d2[s]), bits(want_d2))
        assert (idx[:, :, 5:] == -1).all() and np.isinf(d2[:, :, 5:]).all()
    idx, d2 = knn_gpu(xyz[:, :0], 4, 0.2, queries=xyz[:, :3])                  # n = 0
    assert (idx == -1).all() and np.isinf(d2).all() and (d2 > 0).all()
    idx, _ = knn_gpu(xyz[:, :0], 4, 0.2, queries=xyz[:, :3], want_dist=False)  # dist2 = NULL
    assert (idx == -1).all()


def test_knn_far_query_takes_the_walk():
    xyz, _, _ = adversarial()
    q = np.array([[[1e6, 1e6, 1e6], [0.1, 0.2, 0.3]]] * 2, np.float32)
    idx, d2 = knn_gpu(xyz, 8, 0.2, queries=q)
    for s in range(2):
        want_idx, want_d2 = R.knn(xyz[s], 8, queries=q[s])
        assert np.array_equal(idx[s], want_idx) and np.array_equal(bits(d2[s]), bits(want_d2))
    assert idx[0, 0, 0] == 1023                                                # the outlier at (50, 50, 50) is the nearest


def test_knn_room_scene_4096_k100_and_the_wrapper():
    xyz, want_idx, want_d2 = room_rows(4096, 100)
    idx, d2 = knn_gpu(xyz[None], 100, 0.25, want_dist=False)
    assert np.array_equal(idx[0], want_idx)
    import pointnet2_utils
    widx, wd2 = pointnet2_utils.knn_query(100, t(xyz[None]))                   # the default cell
    assert widx.dtype == torch.int32 and tuple(widx.shape) == (1, 4096, 100)
    assert np.array_equal(widx[0].cpu().numpy(), want_idx) and np.array_equal(bits(wd2[0].cpu().numpy()), bits(want_d2))
    widx, _ = pointnet2_utils.knn_query(8, t(xyz[None]), t(xyz[None, :37]), cell=0.1)
    assert np.array_equal(widx[0].cpu().numpy(), want_idx[:37, :8])


# ---- plane fit -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(2048, 16), (4096, 32), (4096, 100)])
def test_plane_fit_within_the_counted_bound(n, k):
    xyz, idx, _ = room_rows(n, k)
    want, vec, eig = R.plane_fit(xyz, idx)
    got, got_eig = plane_fit_gpu(xyz, idx)
    out = R.plane_fit_excluded(eig)
    assert out.mean() <= 0.005
    theta, bound = R.angle(got, vec), R.plane_fit_bound(eig, k)
    eig_err, eig_bound = np.abs(got_eig - eig).max(1), R.eig_bound(eig, k)
    print(f"plane_fit n={n} k={k}: excluded {out.sum()}, max angle {theta[~out].max():.3e} rad (bound >= {bound[~out].min():.3e}), "
          f"max angle / bound {(theta / bound)[~out].max():.3f}, max eig err / bound {(eig_err / eig_bound).max():.3f}, "
          f"bit-equal normals {np.array_equal(bits(got), bits(want))}")
    assert (theta[~out] <= bound[~out]).all()
    assert (eig_err <= eig_bound).all() and (np.diff(got_eig, axis=1) >= 0).all()
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert R.canonical(got).all()                                              # the largest component is positive ...
    clear = np.sort(np.abs(want), 1)[:, 2] - np.sort(np.abs(want), 1)[:, 1] > 1e-5
    assert ((got * want).sum(1)[clear & ~out] > 0).all()                       # ... and it is the restatement's sign
    other, _ = plane_fit_gpu(xyz, idx, eig=False)                              # eig_out = NULL
    assert np.array_equal(bits(other), bits(got))


def test_plane_fit_degenerate_neighbourhoods_give_finite_unit_vectors():
    xyz = R.room(512).copy()
    xyz[:200] = xyz[0]                                                         # more than k identical points
    xyz[200:240] = xyz[200] + np.arange(40, dtype=np.float32)[:, None] * np.float32(1e-4)     # collinear
    idx, _ = R.knn(xyz, 32)
    idx[300:310, 2:] = -1                                                      # two points
    idx[310, :] = -1                                                           # none
    got, eig = plane_fit_gpu(xyz, idx)
    assert np.isfinite(got).all() and np.isfinite(eig).all()
    assert np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert (eig[:200] == 0).all() and R.canonical(got).all()


# ---- smoothing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 5])
def test_smoothing_votes_exact_values_within_one_ulp(iters):
    _, idx, _ = room_rows(4096, 32)
    nrm, rows = R.smooth_inputs(idx)
    want = nrm
    for _ in range(iters):
        want, votes = R.smooth_step(want, rows)
    got = smooth_gpu(nrm, rows, iters)
    ulps = R.ulp_distance(got, want)
    print(f"smooth iters={iters}: max {ulps.max():.2f} ulp, bit-equal {np.array_equal(bits(got), bits(want))}")
    assert ulps.max() <= 1.0
    if iters == 1:
        assert (got[0] == nrm[0]).all()                                        # the zero-sum row keeps its normal
        assert votes[3, 1] == -1 and np.array_equal(bits(got[3]), bits(want[3]))          # the vote at dot == 0 is -1


# ---- orientation ---------------------------------------------------------------------------------------------------------
def test_orientation_signs_are_exact():
    xyz, idx, _ = room_rows(2048, 16)
    nrm = R.plane_fit(xyz, idx)[0]
    centre = R.view_centre(xyz).astype(np.float32).astype(np.float64)
    xyz = xyz.copy()
    xyz[:4] = centre.astype(np.float32)                                        # dot == 0: not flipped
    for row, towards in ((4, 1.0), (5, -1.0)):                                 # dot > 0 / dot < 0 by one ulp of one coordinate
        j = int(np.argmax(np.abs(nrm[row])))
        xyz[row] = centre.astype(np.float32)
        xyz[row, j] = np.nextafter(xyz[row, j], np.float32(towards * np.sign(nrm[row, j]) * np.inf))
    flips, dot = R.orient_flips(xyz, nrm, centre)
    assert (dot[:4] == 0).all() and dot[4] > 0 and dot[5] < 0 and flips[5] and not flips[:5].any()
    got = orient_gpu(xyz, nrm, centre)
    assert np.array_equal(bits(got), bits(R.orient(xyz, nrm, centre)))
    assert (R.orient_flips(xyz, got, centre)[1] >= 0).all()


# ---- composition ---------------------------------------------------------------------------------------------------------
def test_estimate_normals_is_the_four_stage_calls_chained():
    clouds = np.stack([R.room(1024, seed=s) for s in (1, 2)])
    centre = np.stack([R.view_centre(c) for c in clouds])
    for k, iters, cell in ((16, 2, 0.3), (24, 5, 0.2), (8, 0, 0.5)):
        got = estimate_gpu(clouds, k, iters, cell, centre)
        idx, _ = knn_gpu(clouds, k, cell * 1.7)                                # the cell does not matter
        for s in range(2):
            nrm, _ = plane_fit_gpu(clouds[s], idx[s])
            nrm = smooth_gpu(nrm, idx[s], iters)
            assert np.array_equal(bits(got[s]), bits(orient_gpu(clouds[s], nrm, centre[s]))), (k, iters, s)


def test_estimate_normals_end_to_end_against_the_restatement():
    import point_normals
    xyz, idx, _ = room_rows(4096, 32)
    x = t(xyz[None])
    centre = point_normals.recipe_view_centre(x)
    c = centre[0].cpu().numpy()
    assert np.abs(c - R.view_centre(xyz)).max() < 1e-12 and centre.dtype == torch.float64
    want = R.estimate(xyz, 32, 5, c, idx=idx)
    got = point_normals.estimate_normals(x, k=32, smooth_iters=5)[0].cpu().numpy()
    raw = want
    dot = R.orient_flips(xyz, raw, c)[1]
    keep = np.abs(dot) >= 1e-9
    theta = R.angle(got, want)
    signed = (got.astype(np.float64) * want.astype(np.float64)).sum(1)
    print(f"end to end: max angle {theta.max():.3e} rad, beyond 1e-6: {(theta > 1e-6).sum()}, min |orientation dot| "
          f"{np.abs(dot).min():.3e}, bit-equal {np.array_equal(bits(got), bits(want))}")
    bad = (theta > 1e-6) | (signed < 0)
    assert keep.mean() >= 0.995 and bad[keep].mean() <= 0.005
    assert (R.orient_flips(xyz, got, c)[1] >= 0).all()


# ---- SceneBank -----------------------------------------------------------------------------------------------------------
def test_scene_bank_estimates_missing_normals_at_upload():
    import device_data as D
    import point_normals
    import assemble_inputs
    cfg = assemble_inputs.Config
    pts = [R.room(2048, seed=s) for s in (3, 4)]
    rng = np.random.RandomState(0)
    inst, sem = rng.randint(0, 5, 2048), rng.randint(0, 18, 2048)
    boxes = np.array([[0.0, 0.0, 1.0, 1.0, 1.0, 1.0, float(cfg.nyu40ids[2])]])
    rect, hq = np.zeros((0, 8)), np.zeros((0, 4, 3))
    ubox = np.array([[0.0, 0.0, 1.0, 1.0, 1.5, 1.0, 0.3]])
    given = [point_normals.estimate_normals(t(p[None]))[0].cpu().numpy() for p in pts]

    def banks(normals):
        lab = D.SceneBank(dev(), cfg)
        unl = D.SceneBank(dev())
        for i, p in enumerate(pts):
            lab.add_scene(f"s{i}", p, None if normals is None else normals[i], inst, sem, boxes, rect, 0, hq)
            unl.add_unlabelled_scene(f"u{i}", p, None if normals is None else normals[i], ubox)
        return lab, unl

    for missing, brought in zip(banks(None), banks(given)):
        a = missing.assemble([0, 1], num_points=1024, augment=False)
        b = brought.assemble([0, 1], num_points=1024, augment=False)
        assert sorted(a) == sorted(b)
        assert torch.equal(missing.upload()["normals"], brought.upload()["normals"])
        for key in a:
            if torch.is_tensor(a[key]):
                assert torch.equal(a[key], b[key]), key
            else:
                assert a[key] == b[key], key
        assert float(a["vertex_normals"].norm(dim=-1).sub(1).abs().max()) < 1e-5
