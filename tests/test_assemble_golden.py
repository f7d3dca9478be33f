"""CPU: the restatement of the dataset item (tests/assemble_restatement.py, the arithmetic of include/omnipq_data.h) against
the outputs of the REFERENCE's own `__getitem__` (tests/golden/assemble.npz, made by tests/golden/make_golden_assemble.py)
on the scenes of tests/assemble_inputs.py, with the reference's choices and augmentation parameters passed in.

Rules (shared with tests/test_gpu_assemble.py):
  integer keys                                         exact
  points, normals, votes, ema_point_clouds, colours    bit-equal
  box and quad floats                                  within 1 float32 ulp: both sides round a float64 value once, and the
                                                       reference's float64 value comes from a BLAS product whose last bits
                                                       may differ from a multiply-add chain
Discrete decisions (vote mask, instance -> box label) are compared exactly; what makes that meaningful is asserted first: the
smallest non-tie argmin margin of every case exceeds MARGIN, on the reference's outputs and in the restatement's float64.
`thin` has no box: all 64 label centres are exactly 1000, every distance ties and the label must be 0.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
import assemble_inputs as A
import assemble_restatement as R

MARGIN = 1e-6
CASES = list(A.CASES)
BIT_EQUAL = ("point_clouds", "vertex_normals", "ema_point_clouds", "vote_label", "pcl_color", "semantic_labels", "rot_mat",
             "scale", "heading_residual_label", "box_label_mask")
ONE_ULP = ("center_label", "size_residual_label", "size_gts", "size_label", "gt_quad_centers", "gt_normal_vectors",
           "gt_quad_sizes", "horizontal_quads")
_gold = None


def gold(name, key):
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(GOLDEN, "assemble.npz")))
    return _gold[f"{name}.{key}"]


def gold_item(name):
    prefix = f"{name}.out."
    gold(name, "seed")
    return {k[len(prefix):]: v for k, v in _gold.items() if k.startswith(prefix)}


def params(name):
    fx, fy = (bool(v) for v in gold(name, "flips"))
    return fx, fy, gold(name, "param_rot_mat"), float(gold(name, "param_scale")[0])


_restated = {}


def restated(name):
    """the restatement's item for the case, from the fixture's choices and parameters; computed once"""
    if name not in _restated:
        sc = A.scene(name)
        if name == "arkit":
            _restated[name] = R.arkit_item(sc, gold(name, "choices"), gold(name, "ema_choices"), params(name))
        else:
            _restated[name] = R.scannet_item(sc, A.Config, gold(name, "choices"), gold(name, "ema_choices"), params(name))
    return _restated[name]


def ulps(a, b):
    """distance in float32 steps, +0 and -0 zero apart"""
    def line(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(line(a) - line(b))


def compare(got, want, what, skip=()):
    """every key of `want` (the reference's, or the restatement's) under the rules above; -> the keys compared"""
    seen = []
    for key, w in want.items():
        if key in skip or key == "argmin_margins":
            continue
        assert key in got, (what, key, "missing")
        g = np.asarray(got[key])
        w = np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, key, g.dtype, w.dtype, g.shape, w.shape)
        if key in ONE_ULP:
            worst = int(ulps(g, w).max()) if g.size else 0
            assert worst <= 1, (what, key, worst)
        elif key in BIT_EQUAL:
            assert g.tobytes() == w.tobytes(), (what, key, int((g != w).sum()))
        else:
            assert not np.issubdtype(g.dtype, np.floating), (what, key, "a float key without a rule")
            assert np.array_equal(g, w), (what, key, int((g != w).sum()))
        seen.append(key)
    return seen


@pytest.mark.parametrize("name", CASES)
def test_margins_make_the_exact_comparisons_meaningful(name):
    if name == "arkit":
        return
    for marg in (gold(name, "margins"), restated(name)["argmin_margins"]):
        if name == "thin":
            assert marg.size > 0 and not marg.any()                  # the intended tie
        else:
            assert marg.size > 3 and marg.min() > MARGIN, marg.min()


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_item(name):
    want = gold_item(name)
    seen = compare(restated(name), want, name, skip=("use_gt",))
    assert len(seen) == len(want) - ("use_gt" in want) and len(seen) >= 12


def test_cases_cover_what_they_are_for():
    room = gold_item("room")
    assert room["vote_label_mask"].min() == 0 and room["vote_label_mask"].max() == 1
    sc = A.scene("room")
    counts = np.bincount(np.unique(sc["instance_labels"], return_inverse=True)[1][gold("room", "choices")], minlength=40)
    assert (counts == 0).any() and (counts == 1).any()              # instances that draw no point, and a single one
    # an instance with two semantic labels point by point: its points all vote or all abstain
    for ins in np.unique(sc["instance_labels"]):
        rows = sc["instance_labels"][gold("room", "choices")] == ins
        assert len(set(room["vote_label_mask"][rows])) <= 1
    mixed = [i for i in np.unique(sc["instance_labels"]) if len(set(sc["semantic_labels"][sc["instance_labels"] == i])) > 1]
    assert len(mixed) == 2
    thin = gold_item("thin")
    assert (thin["center_label"] == 1000).all() and thin["vote_label_mask"].any()
    assert (thin["point_instance_label"][thin["vote_label_mask"] == 1] == 0).all()
    assert len(set(gold("thin", "choices"))) < 1024                  # drawn with replacement
    assert gold_item("full")["box_label_mask"].all()
    arkit = gold_item("arkit")
    assert "vote_label" not in arkit and gold("arkit", "flips").tolist() == [1, 1]
    assert int(arkit["flip_x_axis"]) == 0 and int(arkit["flip_y_axis"]) == 0          # the line that clears flag 0
    assert gold("plain", "param_scale")[0] == 1.0 and np.array_equal(gold("plain", "param_rot_mat"), np.identity(3))


def test_draw_is_a_permutation_and_passes_the_inclusion_bound():
    """n >= k: distinct rows in range (n = k: a full permutation); n < k: in range.  Inclusion: n = 1000, k = 400, 256 seed
    values -- every row's count is Binomial(256, 0.4): within 6 sigma of 102.4 (sigma = 7.84)."""
    for n, k in ((1000, 1000), (3000, 1024), (5, 5), (1, 1), (4097, 300), (150000, 40000)):
        d = R.draw(77, 0, 3, n, k)
        assert d.dtype == np.int32 and d.min() >= 0 and d.max() < n and len(set(d.tolist())) == k, (n, k)
    d = R.draw(77, 0, 0, 700, 1024)
    assert d.min() >= 0 and d.max() < 700 and len(set(d.tolist())) > 400
    assert not np.array_equal(R.draw(77, 0, 3, 3000, 1024), R.draw(77, 1, 3, 3000, 1024))       # student / teacher
    assert not np.array_equal(R.draw(77, 0, 3, 3000, 1024), R.draw(77, 0, 2, 3000, 1024))       # slot
    assert not np.array_equal(R.draw(77, 0, 3, 3000, 1024), R.draw(78, 0, 3, 3000, 1024))       # seed
    counts = np.zeros(1000, np.int64)
    for seed in range(256):
        counts[R.draw(seed, 0, 0, 1000, 400)] += 1
    sigma = (256 * 0.4 * 0.6) ** 0.5
    assert abs(sigma - 7.84) < 0.01
    assert np.abs(counts - 102.4).max() <= 6 * sigma, (counts.min(), counts.max())
