"""The gamma-mixture guide criterion on the HIP kernels (omni-pq_amd/models/utils/gamma_mixture_loss_util.py ->
csrc/gamma_guide.hip, include/omnipq_semi.h) against (1) the outputs of the REFERENCE with its own draws
(tests/golden/gamma_mixture.npz) and (2) the float64 restatement (tests/gm_restatement.py) on those cases and on the edge
cases; the draws of its own; forward + backward inside a hipGraph.  Tolerance: see tests/test_gamma_mixture_golden.py."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import gm_inputs
import gm_restatement as R
from test_gamma_mixture_golden import (CASES, LEAVES, NOISE_MAX, WEIGHTS, check_against_fixture, check_grad_rows, check_terms,
                                       gold, inputs, restated)

pytestmark = pytest.mark.gpu


def hip():
    from models.utils import gamma_mixture_loss_util
    return gamma_mixture_loss_util


def to_device(ep_np):
    """numpy batch -> (end_points on the GPU with the three differentiable inputs as leaves, leaves)"""
    ep = {k: torch.from_numpy(v.copy()).cuda() for k, v in ep_np.items()}
    leaves = {k: ep[k].requires_grad_(True) for k in LEAVES}
    return ep, leaves


def run_device(ep_np, pick, inds):
    """-> (terms as floats, {leaf: gradient array}, n_k per scene, branch per scene); the inputs must come back bit-unchanged"""
    ep, leaves = to_device(ep_np)
    before = {k: v.detach().clone() for k, v in ep.items()}
    pick_t, inds_t = torch.from_numpy(np.asarray(pick)).cuda(), torch.from_numpy(np.asarray(inds)).cuda()
    terms = hip().gamma_mixture_guide_criterion(ep, None, None, pick=pick_t, sample_inds=inds_t)
    assert len(terms) == 4 and all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in terms)
    sum(w * t for w, t in zip(WEIGHTS, terms)).backward()
    rec = hip().scene_records(ep, pick_t, inds_t).cpu().numpy()
    for k, v in ep.items():
        assert torch.equal(v.detach(), before[k]), f"{k} was modified"
    grads = {k: leaf.grad.cpu().numpy() for k, leaf in leaves.items()}
    for g in grads.values():
        assert np.isfinite(g).all()
    return [float(t.detach()) for t in terms], grads, rec[:, 5].astype(np.int64), rec[:, 11].astype(np.int64)


@pytest.mark.parametrize("name", CASES + ["batch"])
def test_criterion_reproduces_the_reference_fixture_and_the_restatement(name):
    ep_np, pick, inds = inputs(name)
    terms, grads, n_k, branch = run_device(ep_np, pick, inds)
    check_against_fixture(name, terms, grads, n_k, branch)
    want, scenes, want_grads = restated(name)
    check_terms(terms, want, gold(name, "noise"), (name, "restatement"))
    B = len(pick)
    for k in LEAVES:
        check_grad_rows(grads[k], want_grads[k][np.arange(B), pick], pick, (name, k, "restatement"))


# ------------------------------------------------------------------------------------------------------------ edge cases
def wall_scene(rng, on_quad, away, nv=(-1.0, 0.02, 0.3), size=(3.9, 2.0)):
    """`on_quad` points within a quad on the plane x = 2 (normals along -x, a few millimetres off the plane) and `away` points
    1 m in front of it (0.5 * 1 > T_STAR: dropped); every point is sampled exactly once, so n_k = on_quad."""
    n = on_quad + away
    pts = np.stack([np.full(n, 2.0), rng.uniform(-1.2, 1.2, n), rng.uniform(0.3, 2.1, n)], axis=1)
    pts[:on_quad, 0] += rng.uniform(-0.02, 0.02, on_quad)
    pts[on_quad:, 0] -= 1.0
    nrm = np.array([-1.0, 0.0, 0.0])[None] + 0.02 * rng.standard_normal((n, 3))
    order = rng.permutation(n)
    sc = np.array([[3.0, -3.0]] * 4, dtype=np.float64)
    sc[2] = (-0.4, 0.7)
    qc = rng.uniform(-1, 1, (4, 3))
    qc[2] = (2.01, 0.03, 1.22)
    nvs = rng.standard_normal((4, 3))
    nvs[2] = nv
    qs = rng.uniform(0.5, 3, (4, 2))
    qs[2] = size
    f = np.float32
    ep = {"point_clouds": pts[order].astype(f)[None], "vertex_normals": nrm[order].astype(f)[None],
          "last_quad_scores": sc.astype(f)[None], "last_quad_center": qc.astype(f)[None],
          "last_normal_vector": nvs.astype(f)[None], "last_quad_size": qs.astype(f)[None]}
    return ep, np.array([2]), np.arange(n)[None]


def against_restatement(ep_np, pick, inds, what, n_k=None):
    terms, grads, got_n_k, branch = run_device(ep_np, pick, inds)
    ep, leaves = R.leaves(ep_np)
    want, scenes = R.criterion(ep, pick, inds)
    loss = sum(w * t for w, t in zip(WEIGHTS, want))
    if loss.requires_grad:
        loss.backward()
    check_terms(terms, [float(t.detach()) for t in want], NOISE_MAX, what)
    B = len(pick)
    assert list(got_n_k) == [s["n_k"] for s in scenes] and list(branch) == [s["branch"] for s in scenes], what
    if n_k is not None:
        assert list(got_n_k) == list(n_k), what
    for k in LEAVES:
        g = leaves[k].grad.numpy() if leaves[k].grad is not None else np.zeros(leaves[k].shape)
        check_grad_rows(grads[k], g[np.arange(B), pick], pick, (what, k))
    return terms, grads


def test_the_300_kept_points_threshold():
    """n_k == 300 is computed, n_k == 299 gives nothing (gamma_mixture_loss_util.py:78)"""
    ep, pick, inds = wall_scene(np.random.default_rng(1), 300, 700)
    terms, _ = against_restatement(ep, pick, inds, "n_k=300", n_k=[300])
    assert terms[1] > 0 and terms[2] > 0
    ep, pick, inds = wall_scene(np.random.default_rng(2), 299, 701)
    terms, grads = against_restatement(ep, pick, inds, "n_k=299", n_k=[299])
    assert terms == [0.0] * 4 and not any(g.any() for g in grads.values())


def test_smallest_sample_counts_and_point_counts():
    ep, pick, inds = wall_scene(np.random.default_rng(3), 1, 0)                       # K = 1, N = 1
    assert against_restatement(ep, pick, inds, "K=1", n_k=[1])[0] == [0.0] * 4
    ep, pick, inds = wall_scene(np.random.default_rng(4), 300, 0)                     # K = 300, all kept
    assert against_restatement(ep, pick, inds, "K=300", n_k=[300])[0][2] > 0
    ep, pick, _ = wall_scene(np.random.default_rng(5), 1, 0)                          # N = 1 sampled 400 times
    terms, _ = against_restatement(ep, pick, np.zeros((1, 400), dtype=np.int64), "N=1", n_k=[400])
    assert terms[1] == 0.0 and terms[2] > 0            # every order statistic ties: nothing is below q85, pseudo_x = 0


def test_every_sampled_index_equal():
    ep, pick, _ = wall_scene(np.random.default_rng(6), 500, 500)
    kept = int(np.flatnonzero(ep["point_clouds"][0, :, 0] > 1.5)[0])
    terms, _ = against_restatement(ep, pick, np.full((1, 777), kept, dtype=np.int64), "all equal", n_k=[777])
    assert terms[1] == 0.0
    away = int(np.flatnonzero(ep["point_clouds"][0, :, 0] < 1.5)[0])
    assert against_restatement(ep, pick, np.full((1, 777), away, dtype=np.int64), "all equal, away", n_k=[0])[0] == [0.0] * 4


def test_a_quad_normal_along_z_drops_everything_and_stays_finite():
    """nv.x = nv.y = 0: n = 0 / 0, every distance is NaN, nothing is kept -- zero terms, zero (finite) gradients"""
    ep, pick, inds = wall_scene(np.random.default_rng(7), 600, 100, nv=(0.0, 0.0, 1.0))
    terms, grads, n_k, branch = run_device(ep, pick, inds)
    assert terms == [0.0] * 4 and list(n_k) == [0] and list(branch) == [0]
    assert not any(g.any() for g in grads.values())


def test_point_clouds_with_more_than_three_columns():
    """only the first three columns are read (the row pitch is passed on)"""
    ep, pick, inds = wall_scene(np.random.default_rng(8), 400, 100)
    want = run_device(ep, pick, inds)[0]
    wide = dict(ep)
    wide["point_clouds"] = np.concatenate([ep["point_clouds"], np.full((1, 500, 3), 7.0, dtype=np.float32)], axis=2)
    assert run_device(wide, pick, inds)[0] == want


# ----------------------------------------------------------------------------------------------------------- own draws
def draw_inputs(B=6, Q=37, N=1000, seed=11):
    rng = np.random.default_rng(seed)
    scenes = [gm_inputs.make(seed + b, "a", n=N) for b in range(B)]
    ep = gm_inputs.batch(scenes)
    sc = np.stack([rng.uniform(0.5, 3.0, (B, Q)), rng.uniform(-3.0, 0.5, (B, Q))], axis=2)
    sc[1] = (3.0, -3.0)                                     # scenes 1 and 4: no candidate
    if B > 4:
        sc[4] = (3.0, -3.0)
    sc[2, :, :] = (3.0, -3.0)
    sc[2, Q - 1] = (0.0, 1.0)                               # scene 2: exactly one, the last quad
    ep["last_quad_scores"] = sc.astype(np.float32)
    for k, c in (("last_quad_center", 3), ("last_normal_vector", 3), ("last_quad_size", 2)):
        ep[k] = np.concatenate([ep[k]] * 3, axis=1)[:, :Q].copy()
    return ep


def set_counter(value):
    import dropout_state
    with dropout_state.STATE.use(hip().SEED_SLOT):
        dropout_state.STATE.set_state("cuda:%d" % torch.cuda.current_device(), value)


def test_draws_pick_candidates_and_points_in_range_and_repeat_with_the_counter():
    ep_np = draw_inputs()
    scores = torch.from_numpy(ep_np["last_quad_scores"]).cuda()
    B, Q, N, K = scores.shape[0], scores.shape[1], 1000, 513
    cand = torch.stack([R.candidates(s) for s in scores.cpu()])
    set_counter(1234)
    pick, skip, inds = (t.cpu() for t in hip().draw(scores, N, K))
    assert skip.tolist() == [int(not c.any()) for c in cand] == [0, 1, 0, 0, 1, 0]
    for b in range(B):
        assert skip[b] or bool(cand[b, pick[b]]), b
    assert int(pick[2]) == Q - 1
    assert int(inds.min()) >= 0 and int(inds.max()) < N and inds.dtype == torch.int32 and tuple(inds.shape) == (B, K)
    assert len(torch.unique(inds[0])) > K // 2 and not torch.equal(inds[0], inds[1])
    set_counter(1234)
    again = [t.cpu() for t in hip().draw(scores, N, K)]
    assert torch.equal(again[0], pick) and torch.equal(again[1], skip) and torch.equal(again[2], inds)
    other = hip().draw(scores, N, K)[2].cpu()                 # the counter has moved on
    assert not torch.equal(other, inds)


def test_draws_are_uniform():
    """uniform with replacement over the points, uniform over the candidates: counts within 5 sigma of their expectation"""
    B, Q = 512, 16
    sc = np.tile(np.array([3.0, -3.0], dtype=np.float32), (B, Q, 1))
    cands = (1, 6, 7, 15)
    sc[:, cands] = (0.0, 1.0)
    set_counter(99)
    pick, skip, inds = (t.cpu().numpy() for t in hip().draw(torch.from_numpy(sc).cuda(), 10, 2000))
    assert not skip.any() and set(pick.tolist()) == set(cands)
    counts = np.array([(pick == c).sum() for c in cands])
    assert np.abs(counts - B / 4).max() < 5 * np.sqrt(B * 0.25 * 0.75), counts
    hist = np.bincount(inds.reshape(-1), minlength=10)
    total = inds.size
    assert np.abs(hist - total / 10).max() < 5 * np.sqrt(total * 0.1 * 0.9), hist


def test_result_with_own_draws_equals_a_call_fed_those_draws():
    ep_np = draw_inputs(B=4, Q=16, N=20000, seed=21)
    ep_np["last_quad_scores"][0] = (3.0, -3.0)
    ep_np["last_quad_scores"][0, 3] = (-0.5, 1.0)            # scene 0: the wall quad of case "a" is the only candidate
    ep, _ = to_device(ep_np)
    set_counter(7)
    *terms, draws = hip().gamma_mixture_guide_criterion(ep, None, None, K=4099, return_draws=True)
    assert tuple(draws["sample_inds"].shape) == (4, 4099) and draws["skip"].tolist() == [0, 1, 0, 0]
    fed = hip().gamma_mixture_guide_criterion(ep, None, None, pick=draws["pick"], sample_inds=draws["sample_inds"])
    assert all(torch.equal(a, b) for a, b in zip(terms, fed))
    want, _ = R.criterion(R.leaves(ep_np)[0], draws["pick"].cpu().numpy(), draws["sample_inds"].cpu().numpy())
    assert any(float(t) > 0 for t in want)
    set_counter(7)
    same = hip().gamma_mixture_guide_criterion(ep, None, None, K=4099)
    assert all(torch.equal(a, b) for a, b in zip(terms, same))


# -------------------------------------------------------------------------------------------------------------- capture
def test_forward_and_backward_replay_from_a_hip_graph(monkeypatch):
    """No host read anywhere: draw, forward and backward are captured once on ONE stream (a graph without side branches)
    and replayed on new inputs; each replay is bit-equal to an eager call at the same counter value and draws afresh."""
    from pointnet2 import _ext
    seed = int(gold("batch", "seed")[0])
    make = lambda s: gm_inputs.batch([gm_inputs.make(s + i, c) for i, c in enumerate(("a", "c", "e", "a"))])  # noqa: E731
    ep, leaves = to_device(make(seed))
    streams = []
    real_stream = _ext._stream
    monkeypatch.setattr(_ext, "_stream", lambda *a: streams.append(real_stream(*a)) or streams[-1])

    def run():
        *terms, draws = hip().gamma_mixture_guide_criterion(ep, None, None, K=4099, return_draws=True)
        loss = sum(w * t for w, t in zip(WEIGHTS, terms))
        grads = torch.autograd.grad(loss, list(leaves.values()))
        return torch.stack(terms), grads, draws["pick"], draws["sample_inds"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del streams[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = run()
    assert len(streams) == 3 and len({s.value for s in streams}) == 1, streams      # draw, guide, guide_grad: one stream
    replays = []
    for counter, s in ((1000, seed + 50), (2000, seed + 60)):
        fresh = make(s)
        with torch.no_grad():
            for k, v in ep.items():
                v.copy_(torch.from_numpy(fresh[k]))
        set_counter(counter)
        graph.replay()
        torch.cuda.synchronize()
        got = [out_g[0].clone(), [g.clone() for g in out_g[1]], out_g[2].clone(), out_g[3].clone()]
        set_counter(counter)
        want = run()
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        assert float(got[0][1]) > 0 and any(bool(g.any()) for g in got[1])
        replays.append(got)
    assert not torch.equal(replays[0][3], replays[1][3])
