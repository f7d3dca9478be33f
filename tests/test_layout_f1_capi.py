"""CPU: omnipq_layout_f1 and omnipq_layout_f1_max_gt (include/omnipq_eval.h, csrc/layout_f1.hip) are exported by both libraries
with the signature the header declares, every refusal the header lists comes back as OMNIPQ_EINVAL before the device is touched
(the pointers below are never dereferenced, and this machine has no GPU to launch on), an empty batch launches nothing, and
the limit the library exports is the one the Python wrapper enforces."""
import ctypes

import numpy as np
import pytest

import capi
from test_capi_symbols import both

EINVAL = 10001
p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
POINTERS = ("count_f1", "verts4", "gt_verts4", "num_total", "horizontal", "per_scene", "acc")


def typed(path):
    lib = ctypes.CDLL(path)
    ctype = {"i": ctypes.c_int, "d": ctypes.c_double, "p": ctypes.c_void_p}
    for name, (ret, params) in capi.reported_signatures(lib).items():
        if name.startswith("omnipq_layout_f1"):
            getattr(lib, name).restype = ctype[ret]
            getattr(lib, name).argtypes = [ctype[c] for c in params]
    return lib


def args(b=2, k=256, g=32, cols=256, h=4, thr=0.40, **ptrs):
    q = {name: ptrs.get(name, p) for name in POINTERS}
    return [b, k, q["count_f1"], q["verts4"], g, q["gt_verts4"], q["num_total"], cols, h, q["horizontal"], thr,
            q["per_scene"], q["acc"], null]


def test_symbols_are_exported_and_typed(built_lib):
    want = capi.declared_signatures()
    assert want["omnipq_layout_f1"] == ("i", "iippippiipdppp")
    assert want["omnipq_layout_f1_max_gt"] == ("i", "")
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name in ("omnipq_layout_f1", "omnipq_layout_f1_max_gt"):
            assert hasattr(lib, name) and got[name] == want[name], (path, name)
        assert lib.omnipq_abi_version() == 5                 # additive: the version stays


def test_refusals_need_no_gpu(built_lib):
    for path in both(built_lib):
        lib = typed(path)
        limit = lib.omnipq_layout_f1_max_gt()
        assert limit >= 32
        for bad in (dict(b=-1), dict(k=-1), dict(g=-1), dict(h=-1), dict(k=4097), dict(g=limit + 1), dict(h=9), dict(cols=0),
                    dict(thr=float("nan")), dict(thr=-0.25), dict(thr=float("inf")), dict(thr=-float("inf"))):
            assert lib.omnipq_layout_f1(*args(**bad)) == EINVAL, bad
        for name in POINTERS[:5]:                             # every required pointer in turn
            assert lib.omnipq_layout_f1(*args(**{name: null})) == EINVAL, name
        assert lib.omnipq_layout_f1(*args(per_scene=null, acc=null)) == EINVAL              # either output, not neither
        # nothing to do: returns before looking at a pointer, launches nothing
        assert lib.omnipq_layout_f1(*args(b=0, **{name: null for name in POINTERS})) == 0
        assert lib.omnipq_layout_f1(*args(b=0)) == 0
        assert lib.omnipq_layout_f1(*args(b=0, k=4097)) == EINVAL                           # the limits come first


def test_exported_limit_is_what_the_wrapper_enforces(built_lib):
    import ap_helper_pq
    for path in both(built_lib):
        assert typed(path).omnipq_layout_f1_max_gt() == ap_helper_pq.MAX_F1_GT
    assert ap_helper_pq.MAX_F1_GT >= ap_helper_pq.MAX_NUM_QUAD == 32 and ap_helper_pq.MAX_F1_HORIZONTAL == 8
    quad = np.zeros((4, 3), np.float32)

    def calc(pred=1, gt=1, corner=quad, hz=np.zeros((4, 4, 3), np.float32)):
        c = ap_helper_pq.QUADAPCalculator(f1="device")
        c.step([[]], [[]], [[corner] * pred], [[quad] * gt], [hz])
        return c

    # the wrapper's own refusals come before anything is sent to a device
    with pytest.raises(ValueError, match="at most 4096 predicted"):
        calc(pred=4097).compute_F1()
    with pytest.raises(ValueError, match=f"at most {ap_helper_pq.MAX_F1_GT} ground-truth"):
        calc(gt=ap_helper_pq.MAX_F1_GT + 1).compute_F1()
    with pytest.raises(ValueError, match="not exactly representable in float32"):
        calc(corner=quad.astype(np.float64) + 0.1).compute_F1()
    with pytest.raises(ValueError, match="horizontal quads"):
        calc(hz=np.zeros((9, 4, 3), np.float32)).compute_F1()
    with pytest.raises(ValueError, match="'host' or 'device'"):
        ap_helper_pq.QUADAPCalculator(f1="gpu")
    assert ap_helper_pq.QUADAPCalculator().f1 == "host"
    with pytest.raises(ZeroDivisionError):                   # no ground truth at all: as the host route
        ap_helper_pq.QUADAPCalculator(f1="device").compute_F1()
    with pytest.raises(ZeroDivisionError):
        ap_helper_pq.QUADAPCalculator().compute_F1()
    # f64 corners that ARE float32 values pass the check (exercised up to the refusals only: no GPU here)
    assert ap_helper_pq._exact_f32(quad.astype(np.float64) + 0.5, "corners").dtype == np.float32
    assert ap_helper_pq.f1_from_counts({"tp_wall": 3, "fp": 1, "npos": 4, "tp_horizontal": 2}, True) == \
        2.0 * (5 / 6) * (5 / 4) / (5 / 6 + 5 / 4)
