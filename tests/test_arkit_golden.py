"""The ARKit physical-constraint loss without a GPU: the float64 restatement (tests/arkit_restatement.py) against the outputs
of the REFERENCE (tests/golden/arkit_pc.npz, written by tests/golden/make_golden_arkit.py), the margins of every discrete
decision in every input the GPU tests compare decisions on, the branches those inputs exercise, the module's constants
against the header, and the argument validation of the two C-ABI entry points (include/omnipq_semi.h).

Tolerance, shared with tests/test_gpu_arkit.py and the same as tests/test_consistency_golden.py: 2e-5 relative on the loss
plus an absolute floor of 4 x the `noise` the fixture records for the case -- |reference in f32 - restatement in f64| -- and
1e-4 of the largest entry on a gradient.  The floor comes from the fixture, never from the code under test.

Decisions (gate, reversal, inside, behind the quad, collision) are compared EXACTLY, so the inputs must keep them away from
the knife's edge: coordinates of magnitude <= 6 carry about 2e-6 of f32 rounding through these expressions; every margin is
asserted to exceed 1e-4, fifty times that."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import arkit_inputs
import arkit_restatement as R
import capi

GOLD = np.load(os.path.join(GOLDEN, "arkit_pc.npz"))
CASES = list(arkit_inputs.CASES)
TERM_RTOL = 2e-5
GRAD_RTOL = 1e-4
MARGIN = 1e-4


def gold(name, key):
    return GOLD[f"{name}.{key}"]


@functools.lru_cache(maxsize=None)
def inputs(name):
    return arkit_inputs.make(name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement on a case, computed once: (loss, collisions, record, margins, {leaf: gradient of the loss})"""
    pred, unl = inputs(name)
    leaves = R.leaves(pred)
    loss, collisions, record, margins, _ = R.arkit_pc(leaves, unl)
    loss.backward()
    grads = {k: leaves[k].grad.numpy() for k in R.GRAD_KEYS}
    assert all(leaves[k].grad is None for k in R.PREDICTION_KEYS if k not in R.GRAD_KEYS)
    return float(loss.detach()), collisions, record, margins, grads


def check_loss(got, want, noise, what):
    bound = TERM_RTOL * abs(want) + 4.0 * noise
    print(what, "loss", got, "want", want, "error / bound", abs(got - want) / bound if bound else 0.0)
    assert abs(got - want) <= bound, (what, got, want, bound)


def check_grads(got, want, what):
    """{leaf: array}: every leaf within GRAD_RTOL of its largest wanted entry"""
    for k in R.GRAD_KEYS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), (what, k)
        scale = max(np.abs(w).max(), 1e-12)
        print(what, k, "error / bound", np.abs(g - w).max() / (GRAD_RTOL * scale))
        assert np.abs(g - w).max() <= GRAD_RTOL * scale, (what, k, np.abs(g - w).max(), scale)


def test_inputs_are_the_cases_of_the_issue():
    assert {k: v[:4] for k, v in arkit_inputs.CASES.items()} == {
        "s": (2, 37, 7, (5, 7)), "m": (3, 64, 64, (1, 30, 64)), "q300": (2, 300, 64, (64, 17))}
    for name in CASES:
        pred, unl = inputs(name)
        Bu, Q, K2, counts = arkit_inputs.CASES[name][:4]
        assert pred["last_quad_center"].shape == (2 * Bu, Q, 3) and pred["last_quad_scores"].shape == (2 * Bu, Q, 2)
        assert unl["center_label"].shape == (Bu, K2, 3) and tuple(unl["num_gt_boxes"][:, 0]) == counts
        assert all(v.dtype == np.float32 for v in pred.values())
        for s, n in enumerate(counts):                               # padding is NaN, the real rows are not
            assert np.isnan(unl["center_label"][s, n:]).all() and np.isnan(unl["size_label"][s, n:]).all()
            assert np.isfinite(unl["center_label"][s, :n]).all() and np.isfinite(unl["size_label"][s, :n]).all()
        # the labelled half differs from the unlabelled one: reading the wrong half cannot go unnoticed
        assert not np.array_equal(pred["last_quad_center"][:Bu], pred["last_quad_center"][Bu:])
        again = arkit_inputs.make(name)
        assert all(np.array_equal(pred[k], again[0][k]) for k in pred)


def test_no_decision_of_a_case_is_on_the_knifes_edge():
    for name in CASES:
        margins = restated(name)[3]
        assert set(margins) == {"gate", "rev", "inside", "live"}
        assert min(margins.values()) > MARGIN, (name, margins)


def test_every_case_exercises_every_branch():
    for name in CASES:
        pred, unl = inputs(name)
        record = restated(name)[2]
        Bu, Q, K2, counts = arkit_inputs.CASES[name][:4]
        gate, rev, inside, live, hits = (record[..., i] for i in range(5))
        corners = 4 * np.array(counts)[:, None]
        assert (gate == 0).any() and (gate == 1).any(), name
        assert (rev[gate == 1] == 1).any() and (rev[gate == 1] == 0).any(), name
        assert (inside > live).any(), (name, "an inside pair with delta >= 0")
        assert (hits > 0).any() and (live >= hits).all() and (inside <= corners).all(), name
        assert not record[gate == 0].any(), name
        # an outside pair with delta < 0: counted from the restatement's own quantities
        behind = 0
        for s in range(Bu):
            c = pred["last_quad_center"][Bu + s, :, :2].astype(np.float64)
            n = pred["last_normal_vector"][Bu + s, :, :2].astype(np.float64)
            ab = np.where((rev[s] == 1)[:, None], -n, n)
            P = R.corners(unl["center_label"][s], unl["size_label"][s], counts[s]).numpy()
            delta = ab @ P.T - (ab * c).sum(-1, keepdims=True)
            behind += int(((delta < 0).sum(1) - live[s])[gate[s] == 1].sum())
        assert behind > 0, (name, "an outside pair with delta < 0")


def test_restatement_reproduces_the_reference():
    for name in CASES:
        loss, collisions, _, _, _ = restated(name)
        check_loss(loss, float(gold(name, "loss")[0]), float(gold(name, "noise")[0]), name)
        assert collisions == int(gold(name, "collisions")[0]) and collisions > 0, name
    check_grads(restated("s")[4], {k: gold("s", f"grad.{k}") for k in R.GRAD_KEYS}, "s")
    for k in R.GRAD_KEYS:                                            # nothing in z, nothing in the labelled half
        g = restated("s")[4][k]
        assert not g[..., 2].any() and not g[:2].any() and g[2:, :, :2].any(), k


def test_module_constants_are_the_headers(built_lib):
    from models.utils import arkit_loss_util as ak
    defines = {name: v for name, v in capi.declared_records()[0].items() if name.startswith("OMNIPQ_ARKIT_")}
    assert defines == {"OMNIPQ_ARKIT_MAX_BOXES": ak.MAX_BOXES, "OMNIPQ_ARKIT_RECORD_INTS": ak.RECORD_INTS}
    assert ak.MAX_BOXES == 256 and ak.RECORD_KEYS == R.RECORD_KEYS and len(ak.RECORD_KEYS) == ak.RECORD_INTS == 5
    assert ak.GATE == R.GATE == 0.1 and ak.COLLISION == R.COLLISION == 1e-4
    assert tuple(ak.PREFIX + k for k in ak.PREDICTION_KEYS) == R.PREDICTION_KEYS
    pred, unl = arkit_inputs.make((1, 2, 2, (1,)), repair=False)
    with pytest.raises(RuntimeError, match="CUDA"):
        ak.get_arkit_pc_loss({k: torch.from_numpy(v) for k, v in pred.items()}, {k: torch.from_numpy(v) for k, v in unl.items()},
                             None)


def test_entry_points_are_declared_and_reported_by_both_libraries(built_lib):
    # four sizes, seven inputs, the count stride, the outputs (3 forward, 4 backward), the stream
    want = {"omnipq_arkit_pc": ("i", "iiii" + "ppppppp" + "l" + "ppp" + "p"),
            "omnipq_arkit_pc_grad": ("i", "iiii" + "ppppppp" + "l" + "pppp" + "p")}
    declared = capi.declared_signatures()
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        reported = capi.reported_signatures(lib)
        for name, sig in want.items():
            assert declared[name] == sig and reported[name] == sig and hasattr(lib, name), (path, name)
        assert lib.omnipq_abi_version() == 5


def test_argument_validation_needs_no_gpu(built_lib):
    lib = capi.lib()
    EINVAL, ETOOLARGE = 10001, 10002
    p = ctypes.c_void_p(0x1000)                       # never dereferenced: validation comes first
    null = ctypes.c_void_p(0)
    ll = ctypes.c_longlong

    def fwd(first=2, b=2, q=256, k2=64, stride=1, hole=None):
        ptrs = [null if i == hole else p for i in range(10)]
        return lib.omnipq_arkit_pc(first, b, q, k2, *ptrs[:7], ll(stride), *ptrs[7:], null)

    def bwd(first=2, b=2, q=256, k2=64, stride=1, hole=None):
        ptrs = [null if i == hole else p for i in range(11)]
        return lib.omnipq_arkit_pc_grad(first, b, q, k2, *ptrs[:7], ll(stride), *ptrs[7:], null)

    for bad in (dict(b=-1), dict(first=-1), dict(q=0), dict(k2=0), dict(stride=0), dict(stride=-3)):
        assert fwd(**bad) == EINVAL and bwd(**bad) == EINVAL, bad
    for hole in range(10):
        assert fwd(hole=hole) == EINVAL, hole
    for hole in range(11):
        assert bwd(hole=hole) == EINVAL, hole
    assert fwd(k2=257) == ETOOLARGE and bwd(k2=257) == ETOOLARGE
    assert fwd(first=1 << 20, b=1 << 20, q=1 << 10) == ETOOLARGE and bwd(first=1 << 20, b=1 << 20, q=1 << 10) == ETOOLARGE
    # the sizes are judged before the pointers, and a zero-sized batch succeeds without a device, whatever the pointers
    assert fwd(k2=257, hole=0) == ETOOLARGE and fwd(b=-1, hole=0) == EINVAL
    assert fwd(b=0, hole=0) == 0 and bwd(b=0, hole=9) == 0 and fwd(first=0, b=0) == 0
