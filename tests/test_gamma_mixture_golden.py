"""The gamma-mixture guide criterion without a GPU: the float64 restatement (tests/gm_restatement.py) against the outputs of
the REFERENCE (tests/golden/gamma_mixture.npz, written by tests/golden/make_golden_gamma_mixture.py with the real
`fit_gamma`), the finding that `fit_gamma`'s labels are `|t| <= T_STAR`, and the argument validation of the three C-ABI
entry points (include/omnipq_semi.h).

Tolerance, shared with tests/test_gpu_gamma_mixture.py: the project's bound for a loss (tests/test_gpu_get_loss.py: 2e-5
relative on a scalar term, 1e-4 of the largest entry on a gradient) plus, per term, an absolute floor of 4 x the `noise` the
fixture records for it -- |reference in f32 - restatement in f64|, i.e. the reference's own rounding (metric_normal is
1 - |cos| near 5e-4, where one f32 rounding of the cosine is a relative 1e-4).  Two independent roundings cover the sum
with 2 x, the other 2 x is slack.  The floor comes from the fixture, never from the code under test.
"""
import ctypes
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN
import capi
import gm_inputs
import gm_restatement as R

GOLD = np.load(os.path.join(GOLDEN, "gamma_mixture.npz"))
CASES = list(gm_inputs.ORDER)
TERM_RTOL = 2e-5
GRAD_RTOL = 1e-4
LEAVES = ("last_quad_scores", "last_quad_center", "last_quad_size")
WEIGHTS = tuple(float(w) for w in GOLD["weights"])
# floor for inputs the fixture has no record of (the GPU edge cases): the largest noise any fixture case shows per term
NOISE_MAX = np.max([GOLD[f"{c}.noise"] for c in CASES + ["batch"]], axis=0)


def gold(name, key):
    return GOLD[f"{name}.{key}"]


def inputs(name):
    """-> (batched numpy end_points, pick (B,), sample_inds (B, K)) of a fixture case, or of the B = 5 call ("batch")"""
    seed = int(gold(name, "seed")[0])
    if name == "batch":
        scenes = [gm_inputs.make(seed + i, c) for i, c in enumerate(gm_inputs.ORDER)]
        return gm_inputs.batch(scenes), gold(name, "pick").astype(np.int64), gold(name, "sample_inds").astype(np.int64)
    return (gm_inputs.batch([gm_inputs.make(seed, name)]), gold(name, "pick").astype(np.int64),
            gold(name, "sample_inds").astype(np.int64)[None])


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement on a fixture case, computed once: (terms as floats, per-scene dicts, gradient rows at the picks)"""
    ep_np, pick, inds = inputs(name)
    ep, leaves = R.leaves(ep_np)
    terms, scenes = R.criterion(ep, pick, inds)
    loss = sum(w * t for w, t in zip(WEIGHTS, terms))
    if loss.requires_grad:
        loss.backward()
    grads = {}
    for k, leaf in leaves.items():
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        grads[k] = g.numpy()
    return [float(t.detach()) for t in terms], scenes, grads


def check_terms(got, want, noise, what):
    for t in range(4):
        bound = TERM_RTOL * abs(want[t]) + 4.0 * noise[t]
        assert abs(got[t] - want[t]) <= bound, (what, t, got[t], want[t], bound)


def check_grad_rows(got_full, want_rows, pick, what):
    """got_full (B, Q, c): the picked rows against want_rows (B, c), everything else exactly zero"""
    got_full = np.asarray(got_full, dtype=np.float64)
    B = got_full.shape[0]
    rows = got_full[np.arange(B), pick]
    scale = max(np.abs(want_rows).max(), 1e-6)
    assert np.abs(rows - want_rows).max() <= GRAD_RTOL * scale, (what, rows, want_rows)
    rest = got_full.copy()
    rest[np.arange(B), pick] = 0
    assert not rest.any(), what


def check_against_fixture(name, terms, grads, n_k, branch):
    """terms: four floats; grads: {leaf: (B, Q, c) array}; n_k, branch: per scene"""
    ep_np, pick, _ = inputs(name)
    B = len(pick)
    check_terms(terms, gold(name, "terms"), gold(name, "noise"), name)
    assert list(n_k) == list(gold(name, "n_k")), (name, n_k)
    assert list(branch) == list(gold(name, "branch")), (name, branch)
    for k in LEAVES:
        check_grad_rows(grads[k], gold(name, f"grad.{k}").reshape(B, -1), pick, (name, k))


def test_fixture_holds_the_cases_it_was_built_for():
    assert int(gold("a", "branch")[0]) == 1 and int(gold("a", "K")[0]) == 10000
    assert int(gold("b", "branch")[0]) == 0 and int(gold("b", "K")[0]) == 4099 and int(gold("b", "n_k")[0]) >= 300
    assert int(gold("c", "branch")[0]) == 2 and int(gold("c", "n_k")[0]) >= 300
    assert 0 < int(gold("d", "n_k")[0]) < 300 and not gold("d", "terms").any()
    assert not gold("e", "terms").any()
    assert list(gold("batch", "skipped")) == [False, False, False, False, True]
    # the divergence the implementation documents: the reference divided the caller's last_quad_size in place
    assert bool(gold("a", "mutated")[0]) and bool(gold("batch", "mutated")[0])


def test_restatement_reproduces_the_reference():
    for name in CASES + ["batch"]:
        terms, scenes, grads = restated(name)
        check_against_fixture(name, terms, grads, [s["n_k"] for s in scenes], [s["branch"] for s in scenes])


def test_fit_gamma_labels_are_a_threshold_at_t_star():
    """fit.py:168-173 labels with the densities built from fit_gamma's ARGUMENTS: keep <=> |t| <= T_STAR, on every distance
    the fixture's cases produce and on a grid that straddles the root; 0 is kept, NaN is not."""
    for name in CASES[:4]:
        _, (s,), _ = restated(name)
        assert torch.equal(s["keep"], s["total"].abs() <= R.T_STAR), name
        assert int(s["keep"].sum()) == int(gold(name, "n_k")[0])          # what the real fit_gamma kept
    grid = torch.cat([torch.linspace(0.0, 3.0, 30001, dtype=torch.float64),
                      R.T_STAR + torch.linspace(-1e-9, 1e-9, 2001, dtype=torch.float64)])
    grid = grid[(grid - R.T_STAR).abs() > 1e-13]
    assert torch.equal(R.keep_mask(grid), grid <= R.T_STAR)
    assert torch.equal(R.keep_mask(-grid), grid <= R.T_STAR)
    edge = R.keep_mask(torch.tensor([0.0, float("nan"), float("inf")], dtype=torch.float64))
    assert edge.tolist() == [True, False, False]
    f = lambda t: 40.0 * np.exp(-19.0 * t) - 0.45 * t                      # noqa: E731  (the inequality divided by e^(-t) t)
    assert f(R.T_STAR - 1e-12) > 0 > f(R.T_STAR + 1e-12)


def test_module_constants_are_the_ones_the_restatement_uses():
    src = open(os.path.join(capi.REPO, "omni-pq_amd", "models", "utils", "gamma_mixture_loss_util.py")).read()
    assert f"T_STAR = {R.T_STAR!r}" in src and f"MIN_KEPT = {R.MIN_KEPT}" in src and "GM_CLIP = 0.85" in src


def test_entry_points_validate_before_they_touch_the_device(built_lib):
    """omnipq_gm_draw / omnipq_gm_guide / omnipq_gm_guide_grad: OMNIPQ_EINVAL for k < 1, n < 1, q < 1, a pitch < 3, a negative
    scene count or a null required pointer, OMNIPQ_ETOOLARGE for a k whose distances do not fit in LDS, success for zero
    scenes.  The pointers are never dereferenced: validation comes first (no GPU here)."""
    EINVAL, ETOOLARGE = 10001, 10002
    p, null = ctypes.c_void_p(0x1000), None
    declared = capi.declared_signatures()
    assert declared["omnipq_gm_draw"] == ("i", "iiiippuppp" + "p")
    assert declared["omnipq_gm_guide"] == ("i", "iiiii" + "p" * 11 + "p")
    assert declared["omnipq_gm_guide_grad"] == ("i", "iiiii" + "p" * 13 + "p")
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        assert lib.omnipq_abi_version() == 5                          # additions only
        reported = capi.reported_signatures(lib)
        for name in ("omnipq_gm_draw", "omnipq_gm_guide", "omnipq_gm_guide_grad"):
            fn = getattr(lib, name)
            assert reported[name] == declared[name]
            fn.argtypes = [{"i": ctypes.c_int, "u": ctypes.c_uint, "p": ctypes.c_void_p}[c] for c in declared[name][1]]
            fn.restype = ctypes.c_int

        def draw(b=2, n=100, q=16, k=64, ptrs=None):
            a = ptrs or [p] * 5                                          # quad_scores, seed, pick, skip, sample_inds
            return lib.omnipq_gm_draw(b, n, q, k, a[0], a[1], 0, a[2], a[3], a[4], null)

        def guide(b=2, n=100, q=16, k=64, pitch=3, ptrs=None):
            return lib.omnipq_gm_guide(b, n, q, k, pitch, *(ptrs or [p] * 11), null)

        def grad(b=2, n=100, q=16, k=64, pitch=3, ptrs=None):
            return lib.omnipq_gm_guide_grad(b, n, q, k, pitch, *(ptrs or [p] * 13), null)

        for fn in (draw, guide, grad):
            assert fn(k=0) == EINVAL and fn(n=0) == EINVAL and fn(q=0) == EINVAL and fn(b=-1) == EINVAL
            assert fn(k=15361) == ETOOLARGE and fn(k=1 << 20) == ETOOLARGE
            assert fn(b=0) == 0                                          # zero scenes: nothing to do
        assert guide(pitch=2) == EINVAL and grad(pitch=2) == EINVAL
        for i in range(5):
            assert draw(ptrs=[null if j == i else p for j in range(5)]) == EINVAL, i
        for i in range(11):
            if i != 7:                                                   # skip (index 7) may be NULL: that call would launch
                assert guide(ptrs=[null if j == i else p for j in range(11)]) == EINVAL, i
        for i in range(13):
            assert grad(ptrs=[null if j == i else p for j in range(13)]) == EINVAL, i
