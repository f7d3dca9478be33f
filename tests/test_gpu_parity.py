"""GPU: the HIP path against the CPU oracle and the committed reference fixtures.

Index outputs (FPS, ball query, 3-NN) must be bit-exact; float outputs within 1e-4 of max-abs
(BASELINE.json north_star).  Kernel-level tests call the C ABI directly with raw device pointers
(tests/capi.py); layer/model tests go through `pointnet2._ext` as a user of the drop-in would.
"""
import ctypes

import pytest
import torch

import capi
import synth
from conftest import load_golden
from oracle import oracle_ext

pytestmark = pytest.mark.gpu
TOL = 1e-4
# End-to-end tensors (6 decoder layers deep) are compared against the FLOAT64 evaluation of the
# reference stored in the fixtures, with 1e-4 or 6x the reference's own f32-vs-f64 distance on
# that tensor, whichever is larger (tests/test_oracle_golden.py:run_model_case): in train mode the
# reference's f32 arithmetic is itself up to 2.9e-4 away from f64 (fixture key f32_vs_f64.*).
MODEL_TOL = 1e-4


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel_err(a, b):
    return float((a.cpu().float() - b.float()).abs().max()) / (float(b.abs().max()) + 1e-30)


# --------------------------------------------------------------------------- FPS
FPS_CASES = [
    # (kind, B, N, M)   -- covers every launch shape of csrc/fps.hip
    ("uniform", 2, 1, 1), ("uniform", 2, 7, 7), ("uniform", 3, 64, 16), ("uniform", 2, 100, 37),
    ("adv", 2, 256, 64), ("adv", 2, 300, 300), ("room", 2, 512, 128), ("adv", 2, 777, 200),
    ("room", 2, 1024, 256), ("room", 2, 2048, 1024), ("adv", 2, 2049, 300), ("room", 2, 4096, 512),
    ("room", 1, 8192, 512), ("adv", 2, 8193, 400),        # first multi-workgroup size
    ("room", 2, 20000, 600), ("room", 2, 40000, 2048),    # sa1 of BASELINE configs 2/3
    ("room", 1, 50000, 700), ("uniform", 2, 80000, 300),  # configs 4 and 5
    ("adv", 1, 140000, 64),                               # 8 points per thread, many workgroups
]


def cloud(kind, seed, b, n):
    if kind == "adv":
        return synth.adversarial_cloud(seed, b, max(n, 32))[:, :n].contiguous()
    return synth.make_clouds(seed, b, n, kind=kind) if n >= 64 else \
        torch.rand((b, n, 3), generator=torch.Generator().manual_seed(seed)) * 2 + 0.1


@pytest.mark.parametrize("kind,b,n,m", FPS_CASES)
def test_fps_index_exact(kind, b, n, m):
    xyz = cloud(kind, 5, b, n)
    want = oracle_ext.furthest_point_sampling(xyz, m)
    got, tmp = capi.fps(xyz.to(dev()), m)
    assert torch.equal(got.cpu(), want), f"first mismatch at {(got.cpu() != want).nonzero()[:3].tolist()}"
    # the scratch buffer holds the final running min-distances, as the reference leaves it
    want_tmp = torch.full((b, n), 1e10)
    scratch_idx = torch.zeros((b, m), dtype=torch.int32)        # must outlive the call
    oracle_ext.lib().oracle_furthest_point_sampling(b, n, m, ctypes.c_void_p(xyz.data_ptr()),
                                                    ctypes.c_void_p(want_tmp.data_ptr()),
                                                    ctypes.c_void_p(scratch_idx.data_ptr()))
    assert torch.equal(scratch_idx, want)
    assert torch.equal(tmp.cpu(), want_tmp)


@pytest.mark.parametrize("kind,b,n,m", [c for c in FPS_CASES if c[2] > 8192])
def test_fps_small_footprint_variant_gives_the_same_indices(kind, b, n, m):
    """omnipq_furthest_point_sampling_ex(flags = OMNIPQ_FPS_SMALL_FOOTPRINT): 16 points per thread, fewer workgroups per scene
    (what the prefetched sampling chain of a training step runs on) -- indices and running distances equal the oracle's and
    the default launch's; the choice is an ARGUMENT of the call, nothing lingers for the next one."""
    xyz = cloud(kind, 5, b, n)
    want = oracle_ext.furthest_point_sampling(xyz, m)
    got, tmp = capi.fps(xyz.to(dev()), m, flags=1)
    fast, tmp_fast = capi.fps(xyz.to(dev()), m)
    again, tmp_again = capi.fps(xyz.to(dev()), m, flags=0)
    assert torch.equal(got.cpu(), want), f"first mismatch at {(got.cpu() != want).nonzero()[:3].tolist()}"
    assert torch.equal(fast, got) and torch.equal(tmp, tmp_fast)
    assert torch.equal(again, got) and torch.equal(tmp, tmp_again)


def test_fps_all_points_inside_skip_ball_yields_zeros():
    xyz = torch.rand(2, 500, 3) * 0.01            # |p|^2 <= 1e-3 everywhere
    got, _ = capi.fps(xyz.to(dev()), 40)
    assert torch.equal(got.cpu(), oracle_ext.furthest_point_sampling(xyz, 40))
    assert int(got.abs().sum()) == 0


def test_fps_all_duplicates_tie_rule():
    xyz = torch.ones(2, 1500, 3)
    got, _ = capi.fps(xyz.to(dev()), 20)
    assert torch.equal(got.cpu(), oracle_ext.furthest_point_sampling(xyz, 20))


def test_fps_lattice_ties_follow_launch_geometry():
    """Many exactly equal distances: the winner is decided by (k mod opt_n_threads(n), k)."""
    g = torch.arange(12, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3) + 1.0
    for n in (1728, 1000, 600):
        xyz = lat[:, :n].contiguous()
        got, _ = capi.fps(xyz.to(dev()), 200)
        assert torch.equal(got.cpu(), oracle_ext.furthest_point_sampling(xyz, 200)), n


def test_fps_empty_and_degenerate_arguments():
    d = dev()
    xyz = torch.rand(2, 10, 3, device=d)
    out = torch.full((2, 0), -7, device=d, dtype=torch.int32)
    tmp = torch.full((2, 10), 1e10, device=d)
    assert capi.call("omnipq_furthest_point_sampling", 2, 10, 0, capi.P(xyz), capi.P(tmp), capi.P(out)) == 0
    assert capi.call("omnipq_furthest_point_sampling", 0, 10, 4, capi.P(xyz), capi.P(tmp), capi.P(out)) == 0
    assert capi.call("omnipq_furthest_point_sampling", 2, 10, 4, capi.P(None), capi.P(tmp), capi.P(out)) == 10001
    out4 = torch.zeros((2, 4), device=d, dtype=torch.int32)
    assert capi.call("omnipq_furthest_point_sampling", 1, (1 << 20) + 1, 4, capi.P(xyz), capi.P(tmp),
                     capi.P(out4)) == 10002


# --------------------------------------------------------------------------- ball query
BQ_CASES = [
    ("room", 2, 512, 128, 0.4, 16), ("room", 2, 4096, 1024, 0.2, 32), ("adv", 2, 600, 150, 0.3, 8),
    ("adv", 2, 2048, 512, 0.25, 64), ("uniform", 1, 100, 3, 0.5, 5), ("uniform", 2, 65, 17, 5.0, 100),
    ("room", 2, 40000, 2048, 0.2, 64), ("room", 1, 2048, 1024, 0.4, 32), ("room", 1, 1024, 512, 0.8, 16),
    ("room", 1, 512, 256, 1.2, 16), ("uniform", 1, 300, 300, 1e-4, 8),
]


@pytest.mark.parametrize("kind,b,n,m,radius,nsample", BQ_CASES)
def test_ball_query_index_exact(kind, b, n, m, radius, nsample):
    xyz = cloud(kind, 9, b, n)
    centres = xyz[:, torch.randperm(n, generator=torch.Generator().manual_seed(1))[:m]].contiguous()
    if kind == "adv":
        centres[:, 0] = 50.0          # the outlier's own ball
        centres[:, 1] = -40.0         # an empty ball
    want = oracle_ext.ball_query(centres, xyz, radius, nsample)
    got = capi.ball_query(centres.to(dev()), xyz.to(dev()), radius, nsample)
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("kind,b,n,m,radius,nsample", BQ_CASES + [("room", 8, 40000, 2048, 0.2, 64),
                                                                  ("uniform", 2, 5000, 500, 3.0, 16),
                                                                  ("room", 2, 20000, 256, 2.5, 2000)])
def test_ball_query_through_the_hash_grid_gives_the_same_indices(kind, b, n, m, radius, nsample):
    """omnipq_ball_query_grid == omnipq_ball_query (== the oracle where the oracle is quick): same strict radius,
    the nsample smallest indices in order, first hit repeated in the tail, zeros for empty balls -- including balls
    with more hits than the kernel's hit list holds (radius 2.5 / 3.0: the per-centre fallback), duplicate points
    and centres far outside the cloud."""
    xyz = cloud(kind, 9, b, n)
    centres = xyz[:, torch.randperm(n, generator=torch.Generator().manual_seed(1))[:m]].contiguous()
    if kind == "adv":
        centres[:, 0] = 50.0
        centres[:, 1] = -40.0
    brute = capi.ball_query(centres.to(dev()), xyz.to(dev()), radius, nsample)
    grid = capi.ball_query_grid(centres.to(dev()), xyz.to(dev()), radius, nsample)
    assert torch.equal(grid, brute)
    if b * n * m <= 2 * 4096 * 1024:
        assert torch.equal(grid.cpu(), oracle_ext.ball_query(centres, xyz, radius, nsample))


def test_ball_query_grid_boundary_and_cell_edges():
    """Points exactly at the radius stay out (strict <), points a hair inside stay in even when they sit across a
    cell edge from the centre; negative coordinates; a centre whose 27 cells are all empty."""
    r = 0.5
    xyz = torch.zeros(1, 12, 3)
    xyz[0, :, 0] = torch.tensor([0.0, 0.5, 0.25, 0.5, 1.0, 0.499999, 0.5, 0.125, -0.499999, -0.5, 0.50005, -0.50005])
    centres = torch.tensor([[[0.0, 0.0, 0.0], [0.50004, 0.0, 0.0], [-0.25, 0.0, 0.0], [100.0, 100.0, 100.0]]])
    want = oracle_ext.ball_query(centres, xyz, r, 8)
    got = capi.ball_query_grid(centres.to(dev()), xyz.to(dev()), r, 8)
    assert torch.equal(got.cpu(), want)
    assert want[0, 3].tolist() == [0] * 8


def test_ball_query_grid_far_from_the_origin_and_non_finite_coordinates():
    """A scene in un-centred world coordinates (|x| / r ~ 5000: beyond the range in which a point's cell is exact) and a
    cloud with NaN / inf rows: centres outside the exact range take the reference walk inside the grid kernel, so the
    indices still equal the brute-force kernel's (and the oracle's)."""
    gen = torch.Generator().manual_seed(4)
    xyz = torch.rand(2, 9000, 3, generator=gen) * 3.0
    xyz[0] += torch.tensor([1000.0, -1000.0, 999.5])            # r = 0.2: |x| / h = 5000
    xyz[1, 17] = float("nan")
    xyz[1, 18, 1] = float("inf")
    centres = xyz[:, torch.randperm(9000, generator=gen)[:300]].contiguous()
    centres[1, 0] = float("nan")
    centres[1, 1] = xyz[1, 19]
    brute = capi.ball_query(centres.to(dev()), xyz.to(dev()), 0.2, 32)
    grid = capi.ball_query_grid(centres.to(dev()), xyz.to(dev()), 0.2, 32)
    assert torch.equal(grid, brute)
    assert torch.equal(grid.cpu(), oracle_ext.ball_query(centres, xyz, 0.2, 32))
    assert int((grid[0] != grid[0, :, :1]).sum()) > 0             # the far scene does have multi-point balls


def test_ball_query_radius_boundary_is_strict():
    """d2 == radius^2 exactly must be OUT (ball_query_gpu.cu:35 `d2 < radius2`)."""
    xyz = torch.zeros(1, 8, 3)
    xyz[0, :, 0] = torch.tensor([0.0, 0.5, 0.25, 0.5, 1.0, 0.499999, 0.5, 0.125])
    centres = torch.zeros(1, 1, 3)
    want = oracle_ext.ball_query(centres, xyz, 0.5, 8)
    got = capi.ball_query(centres.to(dev()), xyz.to(dev()), 0.5, 8)
    assert torch.equal(got.cpu(), want)
    assert want[0, 0].tolist() == [0, 2, 5, 7, 0, 0, 0, 0]


# --------------------------------------------------------------------------- gather / group / 3-NN
@pytest.mark.parametrize("b,c,n,m,s", [(2, 5, 512, 128, 16), (2, 259, 2048, 1024, 32), (1, 1, 64, 1, 1),
                                       (3, 13, 1000, 77, 9), (8, 3, 40000, 2048, 64)])
def test_group_and_gather_exact_and_grads(b, c, n, m, s):
    gen = torch.Generator().manual_seed(3)
    pts = torch.randn((b, c, n), generator=gen)
    idx = torch.randint(0, n, (b, m, s), generator=gen, dtype=torch.int32)
    idx[:, :, 0] = idx[:, :, -1]                      # repeated targets in the scatter
    d = dev()
    got = capi.group_points(pts.to(d), idx.to(d))
    assert torch.equal(got.cpu(), oracle_ext.group_points(pts, idx))
    go = torch.randn((b, c, m, s), generator=gen)
    gg = capi.group_points_grad(go.to(d), idx.to(d), n)
    assert rel_err(gg, oracle_ext.group_points_grad(go, idx, n)) <= TOL
    idx1 = idx[:, :, 0].contiguous()
    got1 = capi.gather_points(pts.to(d), idx1.to(d))
    assert torch.equal(got1.cpu(), oracle_ext.gather_points(pts, idx1))
    go1 = torch.randn((b, c, m), generator=gen)
    gg1 = capi.gather_points_grad(go1.to(d), idx1.to(d), n)
    assert rel_err(gg1, oracle_ext.gather_points_grad(go1, idx1, n)) <= TOL


@pytest.mark.parametrize("b,c,n,m,s,empty_balls", [(2, 5, 512, 128, 16, 0), (8, 3, 40000, 2048, 64, 0), (2, 19, 2048, 1024, 32, 300),
                                                   (1, 8, 4096, 1024, 64, 1024)])
def test_group_and_gather_gradients_are_bit_reproducible(b, c, n, m, s, empty_balls):
    """the scatter-add gradients of gather / group are sums in a FIXED order (positions sorted by source
    point with a stable sort, one owner per source point) instead of f32 atomics: two runs are bit-equal, and runs of up to
    128 positions -- the owner thread adds them in ascending position order, as the oracle's loop does -- are bit-equal to the
    oracle.  `empty_balls` balls name source point 0 in every slot (what ball_query returns for a ball without neighbours):
    that run is longer than 128 and goes to the workgroup-per-run kernel (a fixed tree: reproducible, equal to the oracle to
    rounding)."""
    gen = torch.Generator().manual_seed(11)
    idx = torch.randint(0, n, (b, m, s), generator=gen, dtype=torch.int32)
    idx[:, :, 1:4] = idx[:, :, :1]                    # repeated targets inside a ball, as ball_query's padding makes them
    idx[:, :empty_balls] = 0
    go = torch.randn((b, c, m, s), generator=gen)
    d = dev()
    runs = [capi.group_points_grad(go.to(d), idx.to(d), n) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    want = oracle_ext.group_points_grad(go, idx, n)
    counts = torch.zeros(b, n, dtype=torch.long).scatter_add_(1, idx.reshape(b, -1).long(), torch.ones(b, m * s, dtype=torch.long))
    short = (counts <= 128)[:, None, :].expand(b, c, n)
    assert torch.equal(runs[0].cpu()[short], want[short])
    assert rel_err(runs[0], want) <= TOL
    if empty_balls:
        assert int(counts.max()) > 128
    idx1 = idx[:, :, 0].contiguous()
    go1 = torch.randn((b, c, m), generator=gen)
    runs1 = [capi.gather_points_grad(go1.to(d), idx1.to(d), n) for _ in range(2)]
    assert torch.equal(runs1[0], runs1[1])
    assert rel_err(runs1[0], oracle_ext.gather_points_grad(go1, idx1, n)) <= TOL


@pytest.mark.parametrize("kind,b,n,m", [("room", 2, 512, 256), ("room", 8, 1024, 512), ("adv", 2, 600, 150),
                                        ("uniform", 1, 70, 2), ("uniform", 1, 5, 1), ("room", 1, 3000, 2500)])
def test_three_nn_exact_and_interpolate(kind, b, n, m):
    xyz = cloud(kind, 13, b, max(n, m))
    unknown = xyz[:, :n].contiguous()
    known = xyz[:, torch.randperm(xyz.shape[1], generator=torch.Generator().manual_seed(2))[:m]].contiguous()
    d = dev()
    d2, idx = capi.three_nn(unknown.to(d), known.to(d))
    w_d2, w_idx = oracle_ext.three_nn(unknown, known)
    assert torch.equal(idx.cpu(), w_idx)
    assert torch.equal(d2.cpu(), w_d2)                 # same fma form -> bit-equal squared distances
    if m < 3:
        return
    gen = torch.Generator().manual_seed(4)
    c = 11
    feats = torch.randn((b, c, m), generator=gen)
    dist = torch.sqrt(w_d2)
    recip = 1.0 / (dist + 1e-8)
    weight = (recip / recip.sum(2, keepdim=True)).contiguous()
    # omnipq_three_nn_weights: the same indices / squared distances and the reference's weight formula
    # (pointnet2_modules.py:395-397, evaluated above by torch on the CPU) out of one launch -- f32, within 1e-6 relative
    import ctypes
    d2w = torch.empty((b, n, 3), device=d)
    idxw = torch.empty((b, n, 3), device=d, dtype=torch.int32)
    ww = torch.empty((b, n, 3), device=d)
    capi.ok("omnipq_three_nn_weights", b, n, m, capi.P(unknown.to(d)), capi.P(known.to(d)), capi.P(d2w), capi.P(idxw),
            capi.P(ww))
    assert torch.equal(idxw.cpu(), w_idx) and torch.equal(d2w.cpu(), w_d2)
    assert float(((ww.cpu() - weight).abs() / weight.abs().clamp_min(1e-30)).max()) < 1e-6
    assert float((ww.sum(2) - 1).abs().max()) < 1e-6
    got = capi.three_interpolate(feats.to(d), w_idx.to(d), weight.to(d))
    assert torch.equal(got.cpu(), oracle_ext.three_interpolate(feats, w_idx, weight))
    go = torch.randn((b, c, n), generator=gen)
    gg = capi.three_interpolate_grad(go.to(d), w_idx.to(d), weight.to(d), m)
    assert rel_err(gg, oracle_ext.three_interpolate_grad(go, w_idx, weight, m)) <= TOL


# --------------------------------------------------------------------------- full-size properties
def test_full_size_properties_config2():
    """BASELINE config 2 sizes (B=8, N=40000): properties that need no oracle run."""
    xyz = synth.make_clouds(2, 8, 40000, kind="room").to(dev())
    inds, tmp = capi.fps(xyz, 2048)
    assert int(inds[:, 0].abs().sum()) == 0 and int(inds.min()) >= 0 and int(inds.max()) < 40000
    centres = torch.gather(xyz, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    # FPS never re-picks a point while un-picked points remain at positive distance
    assert all(len(set(row.tolist())) == 2048 for row in inds.cpu())
    # the scratch buffer is the coverage distance: temp[k] == min_j |p_k - c_j|^2 over the picks
    # (the last pick is never folded into temp: the loop ends before using it, sampling_gpu.cu:94-178)
    d = ((xyz[0, :4000, None, :] - centres[0, None, :-1, :]) ** 2).sum(-1)
    seen = (xyz[0, :4000] ** 2).sum(-1) > 1.1e-3          # points inside the 1e-3 ball keep 1e10
    assert torch.allclose(d.min(-1).values[seen], tmp[0, :4000][seen], rtol=1e-5, atol=1e-7)
    assert bool((tmp[0, :4000][(xyz[0, :4000] ** 2).sum(-1) < 0.9e-3] == 1e10).all())
    idx = capi.ball_query(centres, xyz, 0.2, 64)
    assert int(idx.min()) >= 0 and int(idx.max()) < 40000
    # first slot of every ball is the smallest member index and members are inside the ball
    members = torch.gather(xyz, 1, idx.long().reshape(8, -1, 1).expand(-1, -1, 3)).reshape(8, 2048, 64, 3)
    d2 = ((members - centres.unsqueeze(2)) ** 2).sum(-1)
    assert float(d2.max()) < 0.2 * 0.2 * (1 + 1e-5)
    assert bool((idx[:, :, :1] <= idx).all())           # padding repeats the first (smallest) hit
    # a ball that is not full (its tail repeats the first hit) lists every member, so it must
    # contain its own centre (distance 0 < r^2)
    not_full = idx[:, :, -1] == idx[:, :, 0]
    has_self = (idx == inds.unsqueeze(-1)).any(-1)
    assert bool(has_self[not_full].all()) and int(not_full.sum()) > 1000


def test_config4_ball_query_50k_points_matches_oracle():
    """BASELINE configs[3] (50 000-point clouds): brute force and hash grid against the oracle, index-exact."""
    pc = synth.make_clouds(1004, 2, 50000, extra_channels=6, kind="room")
    xyz_cpu = pc[..., :3].contiguous()
    xyz = xyz_cpu.to(dev())
    inds, _ = capi.fps(xyz, 2048)
    assert torch.equal(inds.cpu(), oracle_ext.furthest_point_sampling(xyz_cpu, 2048))
    centres = torch.gather(xyz, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3)).contiguous()
    want = oracle_ext.ball_query(centres.cpu(), xyz_cpu, 0.2, 64)
    assert torch.equal(capi.ball_query(centres, xyz, 0.2, 64).cpu(), want)
    assert torch.equal(capi.ball_query_grid(centres, xyz, 0.2, 64).cpu(), want)


# --------------------------------------------------------------------------- layers and model vs fixtures
@pytest.mark.parametrize("name", ["ops_room512", "ops_room4096", "ops_adv600", "ops_adv2048"])
def test_ops_through_python_layers_match_reference_fixture(name):
    import pointnet2_utils
    from test_oracle_golden import run_op_case
    assert pointnet2_utils._ext.__name__ == "pointnet2._ext"
    run_op_case(name, load_golden(name), pointnet2_utils, device="cuda", tol=1e-5)


@pytest.mark.parametrize("name", ["sa1_uniform4096", "sa_feat_room2048", "sa1_room40000_b2", "sa2_room2048_b8"])
def test_sa_module_on_gpu_matches_reference_fixture(name):
    import pointnet2_modules
    from test_oracle_golden import run_sa_case
    run_sa_case(name, load_golden(name), pointnet2_modules, device="cuda", tol=TOL, grad_tol=1e-2,
                grad_metric="l2")


def test_fp_module_on_gpu_matches_reference_fixture():
    import pointnet2_modules
    from test_oracle_golden import run_fp_case
    run_fp_case("fp2_like", load_golden("fp2_like"), pointnet2_modules, device="cuda", tol=TOL, grad_tol=1e-2,
                grad_metric="l2")


def test_model_eval_on_gpu_matches_reference_fixture():
    from test_oracle_golden import run_model_case
    ep = run_model_case(load_golden("model_eval_8192"), device="cuda", tol=MODEL_TOL, forced=True)
    assert ep["sa1_inds"].dtype == torch.int32 and ep["sa1_inds"].is_cuda


def test_model_train_on_gpu_matches_reference_fixture():
    from test_oracle_golden import run_model_case
    run_model_case(load_golden("model_train_8192"), device="cuda", tol=MODEL_TOL, grad_tol=2e-2, forced=True)


def test_in_model_sampling_on_learned_votes_is_index_exact():
    """FPS / ball query on the model's OWN vote coordinates (learned, so not covered by fixtures)
    agree with the oracle run on exactly those coordinates."""
    from test_oracle_golden import build_model
    from procedural import load_procedural
    fx = load_golden("model_eval_8192")
    net = load_procedural(build_model(0)).to(dev()).eval()
    with torch.no_grad():
        ep = net({"point_clouds": fx["inputs"]["point_clouds"].to(dev())})
    votes = ep["vote_xyz"].cpu().contiguous()
    inds = oracle_ext.furthest_point_sampling(votes, 256)
    want = torch.gather(votes, 1, inds.long().unsqueeze(-1).expand(-1, -1, 3))
    assert torch.equal(ep["aggregated_vote_xyz"].cpu(), want)
    seeds = ep["seed_xyz"].cpu().contiguous()
    inds_q = oracle_ext.furthest_point_sampling(seeds, 256)
    want_q = torch.gather(seeds, 1, inds_q.long().unsqueeze(-1).expand(-1, -1, 3))
    assert torch.equal(ep["aggregated_sample_xyz"].cpu(), want_q)


def test_sampling_plan_and_prefetch_do_not_change_results(monkeypatch):
    """The side-stream FPS chain (models/backbone_module.py) and its one-batch-ahead prefetch return
    exactly what the in-layer sampling returns."""
    from test_oracle_golden import build_model
    from procedural import load_procedural
    net = load_procedural(build_model(0)).to(dev()).eval()
    pcs = [synth.make_clouds(60 + i, 2, 8192, kind="room").to(dev()) for i in range(2)]
    keys = ("sa1_inds", "sa2_inds", "sa1_xyz", "sa4_xyz", "seed_features", "last_center", "last_quad_center")
    with torch.no_grad():
        monkeypatch.setenv("OMNIPQ_SAMPLING_PLAN", "0")
        want = [net({"point_clouds": pc}) for pc in pcs]
        monkeypatch.setenv("OMNIPQ_SAMPLING_PLAN", "1")
        got0 = net({"point_clouds": pcs[0]})
        net.prefetch({"point_clouds": pcs[1]})
        assert net.backbone._plan is not None
        got1 = net({"point_clouds": pcs[1]})           # consumes the prefetched plan
        assert net.backbone._plan is None
        net.prefetch({"point_clouds": pcs[0]})
        got1b = net({"point_clouds": pcs[1]})          # stale plan (other tensor): recomputed
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(got0[k], want[0][k]), k
        assert torch.equal(got1[k], want[1][k]), k
        assert torch.equal(got1b[k], want[1][k]), k


def test_fps_on_two_streams_at_once():
    """Two multi-workgroup FPS launches in flight on different streams (a model and its EMA teacher prefetching
    their sampling plans) must not share exchange slots: both equal their sequential results."""
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    dev = torch.device("cuda", 0)
    a = synth.make_clouds(31, 4, 40000, kind="room").to(dev)[..., :3].contiguous()
    b = synth.make_clouds(32, 4, 40000, kind="room").to(dev)[..., :3].contiguous()
    want_a = ext.furthest_point_sampling(a, 1024).clone()
    want_b = ext.furthest_point_sampling(b, 1024).clone()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(s1):
            got_a = ext.furthest_point_sampling(a, 1024)
        with torch.cuda.stream(s2):
            got_b = ext.furthest_point_sampling(b, 1024)
        torch.cuda.synchronize()
        assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    ext.fps_check()


def test_gather_xyz_equals_transpose_gather_transpose():
    """omnipq_gather_xyz == the reference's sequence (pointnet2_modules.py:137-141) bit for bit, incl. repeated indices."""
    import pointnet2_utils
    gen = torch.Generator().manual_seed(9)
    xyz = torch.randn(3, 5000, 3, generator=gen).cuda()
    idx = torch.randint(0, 5000, (3, 777), generator=gen, dtype=torch.int32).cuda()
    idx[:, :5] = idx[:, 5:10]
    got = pointnet2_utils._ext.gather_xyz(xyz, idx)
    want = pointnet2_utils.gather_operation(xyz.transpose(1, 2).contiguous(), idx).transpose(1, 2).contiguous()
    assert torch.equal(got, want)
    assert pointnet2_utils._ext.gather_xyz(xyz[:, :0], idx[:, :0]).shape == (3, 0, 3)


def test_fps_one_wave_per_scene_sizes_and_ties():
    """256 < n <= 1024 run one wave per scene (csrc/fps.hip: fps_wave_kernel) with the register slots loaded in the
    reference's tie order: every residue-class count r = bs / 64 in {4, 8, 16}, ragged last slots, lattice ties, duplicates."""
    g = torch.arange(11, dtype=torch.float32)
    lat = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(1, -1, 3) + 1.0
    for n, m in ((257, 257), (300, 64), (511, 200), (512, 512), (513, 100), (777, 300), (1023, 256), (1024, 1024)):
        for xyz in (lat[:, :n].contiguous().repeat(2, 1, 1), cloud("adv", 11 + n, 2, n)):
            want = oracle_ext.furthest_point_sampling(xyz, m)
            got, tmp = capi.fps(xyz.to(dev()), m)
            assert torch.equal(got.cpu(), want), (n, m, (got.cpu() != want).nonzero()[:3].tolist())
    dup = torch.ones(2, 900, 3)
    dup[:, 450:] += 1.0
    got, _ = capi.fps(dup.to(dev()), 30)
    assert torch.equal(got.cpu(), oracle_ext.furthest_point_sampling(dup, 30))


def test_gather_rows_e16_and_its_adjoint():
    """omnipq_gather_rows_e16 == rows[b, idx[b, p]] bit for bit; the adjoint writes EVERY row: zeros where nothing was selected,
    the f32 sum (rounded once) where an index repeats -- against index_add on a zero tensor."""
    gen = torch.Generator().manual_seed(3)
    d = dev()
    for dt in (torch.bfloat16,):
        for (b, n, p, c) in ((2, 1024, 256, 288), (3, 700, 700, 64), (1, 16384, 5, 8)):
            rows = torch.randn(b, n, c, generator=gen).to(dt).to(d)
            idx = torch.stack([torch.randperm(n, generator=gen)[:p] for _ in range(b)]).int().to(d)
            out = torch.full((b, p, c), 7.0, device=d, dtype=dt)
            capi.ok("omnipq_gather_rows_e16", b, n, p, c, capi.P(rows), capi.P(idx), capi.P(out))
            want = torch.gather(rows, 1, idx.long().unsqueeze(-1).expand(b, p, c))
            assert torch.equal(out, want)
            for dups in (False, True):
                if dups:
                    idx[:, : p // 2] = idx[:, p - p // 2:][:, : p // 2] if p > 1 else idx[:, : p // 2]
                    idx[0, :3] = idx[0, 3]
                g = torch.randn(b, p, c, generator=gen).to(dt).to(d)
                grad = torch.full((b, n, c), 5.0, device=d, dtype=dt)          # NOT zero-filled: every row must be written
                capi.ok("omnipq_gather_rows_e16_grad", b, n, p, c, capi.P(g), capi.P(idx), capi.P(grad))
                ref = torch.zeros(b, n, c, device=d, dtype=torch.float32)
                for bi in range(b):
                    ref[bi].index_add_(0, idx[bi].long(), g[bi].float())
                assert torch.equal(grad, ref.to(dt)), (b, n, p, c, dups)
    null = capi.P(None)
    assert capi.call("omnipq_gather_rows_e16", 1, 8, 4, 12, null, null, null) == 10001          # C % 8
    assert capi.call("omnipq_gather_rows_e16_grad", 1, 20000, 4, 8, null, null, null) != 0       # n too large / null


def test_grouping_ahead_of_the_stages_is_taken_and_changes_nothing(monkeypatch):
    """A prefetched sampling chain also makes the stages' centres, ball queries, row plans, backward CSRs and the FP modules'
    3-NN (backbone_module.GROUP_AHEAD): training mode under bf16 autocast at the benchmark's shape (row plans engage), the
    stages take what the chain made -- no ball query / plan / CSR launch of sa1..sa4 on the forward/backward path -- and every
    backbone output and parameter gradient equals the run without it, bit for bit."""
    import bench
    import backbone_module
    import pointnet2_utils
    import sa_fused
    torch.manual_seed(2)
    net = bench.build_model(0).to(dev()).train()
    pc = synth.make_clouds(77, 8, 40000, kind="room").to(dev())
    keys = ("sa1_inds", "sa2_inds", "sa1_xyz", "sa2_xyz", "sa3_xyz", "sa4_xyz", "sa1_features", "sa2_features", "sa3_features",
            "sa4_features", "fp2_features")
    calls = {"bq": 0, "plan": 0, "csr": 0}
    real_bq, real_plan, real_call = pointnet2_utils._ext.ball_query, sa_fused.make_row_plan, sa_fused._call

    def spy_call(fn, *a):
        if fn.__name__ == "omnipq_sa_build_csr":
            calls["csr"] += 1
        return real_call(fn, *a)

    def run(group):
        monkeypatch.setattr(backbone_module, "GROUP_AHEAD", group)
        for p in net.parameters():
            p.grad = None
        net.prefetch({"point_clouds": pc})
        torch.cuda.synchronize()
        for k in calls:
            calls[k] = 0
        monkeypatch.setattr(pointnet2_utils._ext, "ball_query", lambda *a, **kw: (calls.__setitem__("bq", calls["bq"] + 1), real_bq(*a, **kw))[1])
        monkeypatch.setattr(sa_fused, "make_row_plan", lambda *a, **kw: (calls.__setitem__("plan", calls["plan"] + 1), real_plan(*a, **kw))[1])
        monkeypatch.setattr(sa_fused, "_call", spy_call)
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ep = net.backbone(pc, {})
            loss = sum(ep[k].float().sum() for k in ("fp2_features", "sa4_features"))
            loss.backward()
        finally:
            monkeypatch.setattr(pointnet2_utils._ext, "ball_query", real_bq)
            monkeypatch.setattr(sa_fused, "make_row_plan", real_plan)
            monkeypatch.setattr(sa_fused, "_call", real_call)
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in net.backbone.named_parameters() if p.grad is not None}
        return {k: ep[k].detach().clone() for k in keys}, grads, dict(calls)

    want, gwant, c0 = run(False)
    got, ggot, c1 = run(True)
    assert c0["bq"] == 4 and c0["plan"] >= 2 and c0["csr"] >= 5          # in line: every stage makes its own
    assert c1 == {"bq": 0, "plan": 0, "csr": 0}, c1                        # ahead: nothing left on the path
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    assert sorted(ggot) == sorted(gwant) and len(ggot) >= 30
    for n in gwant:
        assert torch.equal(ggot[n], gwant[n]), n


@pytest.mark.gpu
def test_grouping_ahead_at_a_small_batch_where_only_sa1_is_planned(monkeypatch):
    """Companion of the test above at 2 x 8192 points (sa1 is planned, sa2..sa4 are not: their CSRs are made in the full row
    space): the same launch counts and bit equality, and what the chain made reaches the stages in typed records -- none of
    the tuple attributes the hand-off once used hangs on a tensor reachable from end_points, and no record keeps the tensor
    it rides on alive."""
    import gc
    import weakref
    import bench
    import backbone_module
    import pointnet2_utils
    import sa_fused
    torch.manual_seed(2)
    net = bench.build_model(0).to(dev()).train()
    pc = synth.make_clouds(79, 2, 8192, kind="room").to(dev())
    keys = ("sa1_inds", "sa2_inds", "sa1_xyz", "sa2_xyz", "sa3_xyz", "sa4_xyz", "sa1_features", "sa2_features", "sa3_features",
            "sa4_features", "fp2_features")
    removed = ("omnipq_group", "omnipq_plan", "omnipq_csr", "omnipq_nn", "omnipq_csr3")
    real = {"bq": pointnet2_utils._ext.ball_query, "plan": sa_fused.make_row_plan, "csr": sa_fused._call}
    calls = dict.fromkeys(real, 0)

    def counted(what):
        def spy(*a, **kw):
            if what != "csr" or a[0].__name__ == "omnipq_sa_build_csr":
                calls[what] += 1
            return real[what](*a, **kw)
        return spy

    def carried(obj, seen):
        """names of the attributes on every tensor reachable from obj through containers, records and tensor attributes"""
        if id(obj) in seen:
            return set()
        seen.add(id(obj))
        if isinstance(obj, torch.Tensor):
            names = set(vars(obj))
            return names.union(*(carried(v, seen) for v in list(vars(obj).values()) + [obj._base]))
        if isinstance(obj, dict):
            obj = list(obj.values())
        if isinstance(obj, (list, tuple)):
            return set().union(*(carried(v, seen) for v in obj))
        return set()

    def run(group):
        monkeypatch.setattr(backbone_module, "GROUP_AHEAD", group)
        for p in net.parameters():
            p.grad = None
        net.prefetch({"point_clouds": pc})
        torch.cuda.synchronize()
        calls.update(dict.fromkeys(calls, 0))
        monkeypatch.setattr(pointnet2_utils._ext, "ball_query", counted("bq"))
        monkeypatch.setattr(sa_fused, "make_row_plan", counted("plan"))
        monkeypatch.setattr(sa_fused, "_call", counted("csr"))
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                ep = net.backbone(pc, {})
            (ep["fp2_features"].float().sum() + ep["sa4_features"].float().sum()).backward()
        finally:
            monkeypatch.setattr(pointnet2_utils._ext, "ball_query", real["bq"])
            monkeypatch.setattr(sa_fused, "make_row_plan", real["plan"])
            monkeypatch.setattr(sa_fused, "_call", real["csr"])
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in net.backbone.named_parameters() if p.grad is not None}
        alive = [weakref.ref(ep[k]) for k in ("sa1_inds", "sa2_xyz", "sa3_xyz", "sa4_xyz")]
        return {k: ep[k].detach().clone() for k in keys}, grads, dict(calls), carried(ep, set()), alive

    gc.collect()
    gc.disable()
    try:
        want, gwant, c0, names0, _ = run(False)
        got, ggot, c1, names1, alive = run(True)
        # a record rides on a tensor it describes: it must not hold that tensor, or the step's copy of the chain's buffer
        # (10 MB at the benchmark's shape) lives until a garbage collection instead of until its last user
        assert [r() is None for r in alive] == [True] * 4
    finally:
        gc.enable()
    assert c0["bq"] == 4 and c0["plan"] >= 1 and c0["csr"] >= 5          # in line: every stage makes its own
    assert c1 == {"bq": 0, "plan": 0, "csr": 0}, c1                        # ahead: nothing left on the path
    for k in keys:
        assert torch.equal(got[k], want[k]), k
    assert sorted(ggot) == sorted(gwant) and len(ggot) >= 30
    for n in gwant:
        assert torch.equal(ggot[n], gwant[n]), n
    assert "omnipq_stage_ahead" in names1 and "omnipq_stage_ahead" not in names0      # the walk does reach the hand-off
    assert not (names0 | names1) & set(removed), (names0 | names1) & set(removed)


@pytest.mark.gpu
def test_a_csr_made_ahead_in_another_row_space_is_not_reused(monkeypatch):
    """the backward CSR of a stage is made ahead of it in the row space of the plan the chain built.  If what
    decides the row space changes between prefetch and forward (here: ROW_PLAN switched off after the chain ran), the stage
    runs unplanned and must NOT take that CSR: outputs and gradients equal the run that never prefetched."""
    import bench
    import sa_fused
    torch.manual_seed(2)
    net = bench.build_model(0).to(dev()).train()
    pc = synth.make_clouds(78, 8, 40000, kind="room").to(dev())

    def run(prefetch_with_plan):
        for p in net.parameters():
            p.grad = None
        net.backbone.forget_plan()
        if prefetch_with_plan:
            monkeypatch.setattr(sa_fused, "ROW_PLAN", True)
            net.prefetch({"point_clouds": pc})            # the chain builds plans and CSRs in their compact row space
            torch.cuda.synchronize()
        monkeypatch.setattr(sa_fused, "ROW_PLAN", False)   # ... and the stages run without one
        uses = sa_fused.row_plan_uses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            ep = net.backbone(pc, {})
        (ep["fp2_features"].float().sum() + ep["sa4_features"].float().sum()).backward()
        torch.cuda.synchronize()
        assert sa_fused.row_plan_uses == uses
        return ep["fp2_features"].detach().clone(), {n: p.grad.clone() for n, p in net.backbone.named_parameters()
                                                     if p.grad is not None}

    want, gwant = run(False)
    got, ggot = run(True)
    assert torch.equal(got, want)
    assert sorted(ggot) == sorted(gwant) and len(ggot) >= 30
    for n in gwant:
        assert torch.equal(ggot[n], gwant[n]), n
