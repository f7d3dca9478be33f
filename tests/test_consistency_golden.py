"""The mean-teacher consistency loss without a GPU: the float64 restatement (tests/mt_restatement.py) against the outputs of
the REFERENCE (tests/golden/consistency.npz, written by tests/golden/make_golden_consistency.py), the margins of every
discrete decision in every input the GPU tests compare decisions on, the module's constants against the header, and the
argument validation of the C-ABI entry points (include/omnipq_semi.h).

Tolerance, shared with tests/test_gpu_consistency.py: the project's bound for a loss (tests/test_gamma_mixture_golden.py:
2e-5 relative on a scalar term, 1e-4 of the largest entry on a gradient) plus, per term, an absolute floor of 4 x the `noise`
the fixture records for it -- |reference in f32 - restatement in f64|.  The floor comes from the fixture, never from the
code under test.

Decisions (nearest neighbours, arg-max classes, quantile masks) are compared EXACTLY, so the inputs must keep them away from
the knife's edge: an f32 squared distance between rotated and scaled points of magnitude <= 8 carries about 2e-6 of absolute
rounding; every margin is asserted to exceed 1e-4, fifty times that."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import capi
import mt_inputs
import mt_restatement as R

GOLD = np.load(os.path.join(GOLDEN, "consistency.npz"))
CASES = list(mt_inputs.CASES)
TERM_RTOL = 2e-5
GRAD_RTOL = 1e-4
MARGIN = 1e-4
WEIGHTS = tuple(float(w) for w in GOLD["weights"])
GRAD_NAMES = [p + k for p in mt_inputs.PREFIXES for k in mt_inputs.GRAD_KEYS]
# floor for inputs the fixture has no record of (the edge cases): the largest noise any fixture case shows per term
NOISE_MAX = np.max([GOLD[f"{c}.noise"] for c in CASES], axis=0)
# every input on which the GPU tests compare decisions: name -> arguments of mt_inputs.make
INPUTS = {"s": ("s",), "m": ("m",), "k256": ("k256",), "flips_on": ("s", 0, True), "flips_off": ("s", 5, False)}


def gold(name, key):
    return GOLD[f"{name}.{key}"]


def inputs(name):
    return mt_inputs.make(*INPUTS[name])


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement on a named input, computed once: (terms as floats, decisions, margins, outputs, {leaf: gradient of
    sum_t WEIGHTS[t] terms[t]})"""
    S_np, T_np, mean_size = inputs(name)
    S, T, ms = R.leaves(S_np, T_np, mean_size, set(GRAD_NAMES))
    terms, decisions, margins, outputs = R.consistency(S, T, ms, mt_inputs.PREFIXES)
    sum(w * t for w, t in zip(WEIGHTS, terms)).backward()
    grads = {k: S[k].grad.numpy() for k in GRAD_NAMES}
    assert all(S[p + k].grad is None for p in mt_inputs.PREFIXES for k in mt_inputs.NO_GRAD_KEYS)
    outputs = {k: v.detach().numpy() for k, v in outputs.items()}
    return [float(t.detach()) for t in terms], decisions, margins, outputs, grads


def check_terms(got, want, noise, what):
    for t in range(10):
        bound = TERM_RTOL * abs(want[t]) + 4.0 * noise[t]
        assert abs(got[t] - want[t]) <= bound, (what, t, got[t], want[t], bound)


def check_grads(got, want, what):
    """{leaf: array}: every leaf within GRAD_RTOL of its largest wanted entry"""
    for k in GRAD_NAMES:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), (what, k)
        scale = max(np.abs(w).max(), 1e-12)
        assert np.abs(g - w).max() <= GRAD_RTOL * scale, (what, k, np.abs(g - w).max(), scale)


def assignments(decisions):
    return np.stack([np.stack([decisions[(p, 0)]["ind2"].numpy(), decisions[(p, 1)]["ind2"].numpy()])
                     for p in mt_inputs.PREFIXES])


def quantile_fraction(B, K):
    rank = 0.85 * (B * K - 1)
    return rank - np.floor(rank)


@pytest.mark.filterwarnings("ignore:reduction")
def test_restatement_reproduces_the_reference():
    for name in CASES:
        terms, decisions, _, _, grads = restated(name)
        check_terms(terms, gold(name, "terms"), gold(name, "noise"), name)
        assert np.array_equal(assignments(decisions), gold(name, "assignment")), name
        # the divergence the implementation documents: the reference flipped the teacher's centres in place
        assert bool(gold(name, "mutated")[0]), name
    check_grads(restated("s")[4], {k: gold("s", f"grad.{k}") for k in GRAD_NAMES}, "s")
    t = gold("s", "terms")
    assert abs(t[3] - (0.5 * t[0] + t[1] + 0.05 * t[2])) < 1e-6 and abs(t[8] - (0.5 * t[4] + t[6] + 0.05 * t[7])) < 1e-6
    assert abs(t[9] - (t[3] + t[8])) < 1e-6


@pytest.mark.filterwarnings("ignore:reduction")
def test_no_decision_of_a_compared_input_is_on_the_knifes_edge():
    assert [round(quantile_fraction(*mt_inputs.CASES[c][:2]), 2) for c in CASES] == [0.5, 0.75, 0.35]
    for name in INPUTS:
        B, K = mt_inputs.CASES[INPUTS[name][0]][:2]
        assert 0.1 <= quantile_fraction(B, K) <= 0.9, name
        margins = restated(name)[2]
        assert set(margins) == {"nn", "argmax", "eps"}
        assert min(margins.values()) > MARGIN, (name, margins)


def test_k256_assigns_some_student_rows_several_times_and_some_never():
    a = gold("k256", "assignment")
    for p in range(a.shape[0]):
        for kind in range(2):
            for b in range(a.shape[2]):
                counts = np.bincount(a[p, kind, b], minlength=256)
                assert (counts == 0).sum() == 64 and counts.max() == 4 and (counts == 2).sum() > 0
                assert not np.array_equal(a[p, kind, b], np.arange(256))


def test_module_constants_are_the_headers(built_lib):
    from models.utils import mean_teacher_consistency_util as mt
    defines = {name: v for name, v in capi.declared_records()[0].items() if name.startswith("OMNIPQ_MT_")}
    assert defines == {"OMNIPQ_MT_MAX_PREFIXES": mt.MAX_PREFIXES, "OMNIPQ_MT_MAX_CLASSES": mt.MAX_CLASSES,
                       "OMNIPQ_MT_MAX_K": mt.MAX_K, "OMNIPQ_MT_MAX_ROWS": mt.MAX_ROWS, "OMNIPQ_MT_TERMS": mt.TERMS}
    assert mt.MAX_PREFIXES == 8 and mt.EMA_CLIP == 0.85 and mt.PREFIXES == mt_inputs.PREFIXES and len(mt.PREFIXES) == 7
    assert mt.TERM_KEYS == R.TERMS and mt.GRAD_KEYS == mt_inputs.GRAD_KEYS
    assert (mt.MAX_PREFIXES, mt.MAX_CLASSES, mt.MAX_K, mt.MAX_ROWS, mt.TERMS) == (8, 64, 512, 15360, 10)
    # the two structs: five ints, 17 + 8 pointer arrays, five pointers
    assert ctypes.sizeof(mt._Desc) == 24 + 17 * 8 * 8 + 5 * 8 and ctypes.sizeof(mt._Grads) == 8 * 8 * 8
    with pytest.raises(RuntimeError, match="CUDA"):
        S, T, _ = mt_inputs.make((1, 2, 2, 2))
        mt.get_consistency_loss({k: torch.from_numpy(v) for k, v in S.items()}, {k: torch.from_numpy(v) for k, v in T.items()},
                                mt_inputs.Config(2))


def test_entry_points_are_declared_and_reported_by_both_libraries(built_lib):
    want = {"omnipq_mt_consistency_workspace_bytes": ("l", "iii"), "omnipq_mt_consistency": ("i", "ppppppp"),
            "omnipq_mt_consistency_grad": ("i", "ppppp")}
    declared = capi.declared_signatures()
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        reported = capi.reported_signatures(lib)
        for name, sig in want.items():
            assert declared[name] == sig and reported[name] == sig and hasattr(lib, name), (path, name)
        assert lib.omnipq_abi_version() == 5


def test_argument_validation_needs_no_gpu(built_lib):
    from models.utils import mean_teacher_consistency_util as mt
    lib = capi.lib()
    EINVAL, ETOOLARGE = 10001, 10002
    p = ctypes.c_void_p(0x1000)                       # never dereferenced: validation comes first
    null = ctypes.c_void_p(0)
    lib.omnipq_mt_consistency_workspace_bytes.restype = ctypes.c_longlong

    def desc(prefixes=7, b=2, k=256, nc=18, ns=18, hole=None):
        d = mt._Desc(prefixes, b, k, nc, ns)
        for name, _ in mt._Desc._fields_[5:]:
            if name in ("flip_x", "flip_y", "rot_mat", "scale", "mean_size"):
                setattr(d, name, 0 if name == hole else 0x1000)
            else:
                for i in range(max(0, min(prefixes, 8))):
                    getattr(d, name)[i] = 0 if name == hole and i == prefixes - 1 else 0x1000
        return d

    def fwd(d, out=p, ws=p):
        return lib.omnipq_mt_consistency(ctypes.byref(d), out, p, p, ws, p, null)

    def bwd(d, g=None, ws=p, g_terms=p):
        grads = mt._Grads()
        for name, _ in mt._Grads._fields_:
            for i in range(8):
                getattr(grads, name)[i] = 0x1000
        if g is not None:
            getattr(grads, g)[0] = 0
        return lib.omnipq_mt_consistency_grad(ctypes.byref(d), ws, g_terms, ctypes.byref(grads), null)

    for bad in (dict(b=-1), dict(k=0), dict(prefixes=0), dict(prefixes=9), dict(nc=0), dict(nc=65), dict(ns=0), dict(ns=65)):
        assert fwd(desc(**bad)) == EINVAL and bwd(desc(**bad)) == EINVAL, bad
    for hole in ("center", "objectness_scores", "size_residuals", "quad_size", "t_center", "t_quad_scores", "flip_x", "scale",
                 "mean_size"):
        assert fwd(desc(hole=hole)) == EINVAL and bwd(desc(hole=hole)) == EINVAL, hole
    assert fwd(desc(), out=null) == EINVAL and fwd(desc(), ws=null) == EINVAL
    assert bwd(desc(), g="normal_vector") == EINVAL and bwd(desc(), ws=null) == EINVAL and bwd(desc(), g_terms=null) == EINVAL
    assert lib.omnipq_mt_consistency(null, p, p, p, p, p, null) == EINVAL
    # b * k beyond the clip kernel's LDS, k beyond the rows kernel's
    assert fwd(desc(b=61, k=256)) == ETOOLARGE and bwd(desc(b=61, k=256)) == ETOOLARGE
    assert fwd(desc(b=1, k=513)) == ETOOLARGE
    assert lib.omnipq_mt_consistency_workspace_bytes(7, 61, 256) == 0 and lib.omnipq_mt_consistency_workspace_bytes(9, 2, 256) == 0
    # a zero-sized batch succeeds without a device, whatever the pointers
    assert fwd(desc(b=0, hole="center"), out=null, ws=null) == 0 and bwd(desc(b=0), ws=null) == 0
    # the workspace: 16 f64 + 4 f32 per (prefix, kind), 8 f64 per scene of it, 27 bytes per row of it; a multiple of 256
    n, pk = 60 * 256, 14
    want = pk * (60 * 8 + 32 + 16 + n * 27)
    assert lib.omnipq_mt_consistency_workspace_bytes(7, 60, 256) == (want + 255) // 256 * 256
