"""CPU: the packed-detection entry points of include/omnipq_eval.h (csrc/detect.hip) are exported by both libraries with typed
signatures, every refusal the header lists comes back as OMNIPQ_EINVAL before the device is touched (the pointers below are
never dereferenced, and this machine has no GPU to launch on), and the limit the library exports is the one the Python
wrapper enforces."""
import ctypes

import pytest
import torch

import capi
from test_capi_symbols import both

EINVAL = 10001
p, null = ctypes.c_void_p(0x1000), ctypes.c_void_p(0)
f = ctypes.c_float


def typed(path):
    lib = ctypes.CDLL(path)
    ctype = {"i": ctypes.c_int, "f": ctypes.c_float, "d": ctypes.c_double, "p": ctypes.c_void_p, "l": ctypes.c_longlong}
    for name, (ret, params) in capi.reported_signatures(lib).items():
        if name.startswith(("omnipq_decode_boxes", "omnipq_pack_")):
            getattr(lib, name).restype = ctype[ret]
            getattr(lib, name).argtypes = [ctype[c] for c in params]
    return lib


def decode_args(b=2, k=256, nh=1, ns=18, ncls=18, rule=0, bev=0, ptrs=None):
    ptrs = list(ptrs) if ptrs is not None else [p] * 17
    return [b, k, nh, ns, ncls] + ptrs[:8] + [rule, bev] + ptrs[8:] + [null]


def pack_boxes_args(b=2, k=256, ncls=18, ptrs=None):
    ptrs = list(ptrs) if ptrs is not None else [p] * 11
    return [b, k, ncls, ptrs[0], ptrs[1], 0.3] + ptrs[2:] + [null]


def pack_quads_args(b=2, k=256, ptrs=None):
    ptrs = list(ptrs) if ptrs is not None else [p] * 11
    return [b, k, ptrs[0], ptrs[1], 0.3, 0.5] + ptrs[2:] + [null]


def test_symbols_are_exported_and_typed(built_lib):
    want = capi.declared_signatures()
    assert want["omnipq_decode_boxes"] == ("i", "iiiii" + "p" * 8 + "ii" + "p" * 9 + "p")
    assert want["omnipq_decode_boxes_max_classes"] == ("i", "")
    assert want["omnipq_pack_boxes"] == ("i", "iiippfpppppppppp")
    assert want["omnipq_pack_quads"] == ("i", "iippffpppppppppp")
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name in ("omnipq_decode_boxes", "omnipq_decode_boxes_max_classes", "omnipq_pack_boxes", "omnipq_pack_quads"):
            assert hasattr(lib, name) and got[name] == want[name], (path, name)
        assert lib.omnipq_abi_version() == 5                 # additive: the version stays


def test_decode_refusals_need_no_gpu(built_lib):
    for path in both(built_lib):
        lib = typed(path)
        limit = lib.omnipq_decode_boxes_max_classes()
        assert lib.omnipq_decode_boxes(*decode_args(k=4097)) == EINVAL
        assert lib.omnipq_decode_boxes(*decode_args(b=-1)) == EINVAL
        assert lib.omnipq_decode_boxes(*decode_args(k=-1)) == EINVAL
        for which in ("nh", "ns", "ncls"):
            assert lib.omnipq_decode_boxes(*decode_args(**{which: limit + 1})) == EINVAL, which
            assert lib.omnipq_decode_boxes(*decode_args(**{which: 0})) == EINVAL, which
            assert lib.omnipq_decode_boxes(*decode_args(**{which: -3})) == EINVAL, which
        assert lib.omnipq_decode_boxes(*decode_args(rule=2)) == EINVAL
        for i in range(17):
            if i == 14:                                       # sem_prob, the one optional output: that call would launch
                continue
            ptrs = [p] * 17
            ptrs[i] = null
            assert lib.omnipq_decode_boxes(*decode_args(ptrs=ptrs)) == EINVAL, i
        # nothing to do: returns before looking at a pointer, launches nothing
        assert lib.omnipq_decode_boxes(*decode_args(b=0, ptrs=[null] * 17)) == 0
        assert lib.omnipq_decode_boxes(*decode_args(k=0, ptrs=[null] * 17)) == 0


def test_pack_refusals_need_no_gpu(built_lib):
    for path in both(built_lib):
        lib = typed(path)
        limit = lib.omnipq_decode_boxes_max_classes()
        assert lib.omnipq_pack_boxes(*pack_boxes_args(k=4097)) == EINVAL
        assert lib.omnipq_pack_boxes(*pack_boxes_args(b=-1)) == EINVAL
        assert lib.omnipq_pack_boxes(*pack_boxes_args(k=-2)) == EINVAL
        assert lib.omnipq_pack_boxes(*pack_boxes_args(ncls=limit + 1)) == EINVAL
        assert lib.omnipq_pack_boxes(*pack_boxes_args(ncls=0)) == EINVAL
        for i in range(11):
            ptrs = [p] * 11
            ptrs[i] = null                                    # sem_prob (4) without out_sem_prob (10) or the reverse: refused too
            assert lib.omnipq_pack_boxes(*pack_boxes_args(ptrs=ptrs)) == EINVAL, i
        assert lib.omnipq_pack_boxes(*pack_boxes_args(b=0, ptrs=[null] * 11)) == 0
        assert lib.omnipq_pack_boxes(*pack_boxes_args(k=0, ptrs=[null] * 11)) == 0

        assert lib.omnipq_pack_quads(*pack_quads_args(k=4097)) == EINVAL
        assert lib.omnipq_pack_quads(*pack_quads_args(b=-1)) == EINVAL
        assert lib.omnipq_pack_quads(*pack_quads_args(k=-1)) == EINVAL
        for i in range(11):
            ptrs = [p] * 11
            ptrs[i] = null
            assert lib.omnipq_pack_quads(*pack_quads_args(ptrs=ptrs)) == EINVAL, i
        assert lib.omnipq_pack_quads(*pack_quads_args(b=0, ptrs=[null] * 11)) == 0
        assert lib.omnipq_pack_quads(*pack_quads_args(k=0, ptrs=[null] * 11)) == 0


def test_exported_limit_is_what_the_wrapper_enforces(built_lib):
    import ap_helper_pq
    import loss_inputs
    for path in both(built_lib):
        assert typed(path).omnipq_decode_boxes_max_classes() == ap_helper_pq.MAX_DECODE_CLASSES == 64
    assert ap_helper_pq.MAX_PROPOSALS == 4096

    class Fake(torch.Tensor):
        """a CPU tensor that says it is on the GPU: the wrapper's checks run in front of every launch"""
        is_cuda = True

    def ep(K=8, ncls=18):
        shapes = {"center": (1, K, 3), "heading_scores": (1, K, 1), "heading_residuals": (1, K, 1), "size_scores": (1, K, 18),
                  "size_residuals": (1, K, 18, 3), "sem_cls_scores": (1, K, ncls), "objectness_scores": (1, K, 2)}
        return {k: torch.zeros(s).as_subclass(Fake) for k, s in shapes.items()}

    cfg = loss_inputs.eval_config()
    with pytest.raises(ValueError, match=r"\[1, 64\]"):
        ap_helper_pq.detect_predictions(ep(ncls=ap_helper_pq.MAX_DECODE_CLASSES + 1), cfg)
    with pytest.raises(ValueError, match="at most 4096"):
        ap_helper_pq.detect_predictions(ep(K=4097), cfg)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ap_helper_pq.detect_predictions({k: torch.zeros(v.shape) for k, v in ep().items()}, cfg)


def test_record_layout_is_aligned_and_results_come_first():
    import ap_helper_pq
    for kind, kw in (("boxes", dict(ncls=18, ns=18, per_class=True)), ("boxes", dict(ncls=5, ns=3)), ("quads", {})):
        fields, result_bytes, total = ap_helper_pq.detections_layout(kind, 3, 37, **kw)
        names = [f[0] for f in fields]
        assert len(set(names)) == len(names) and names[0] == "count"
        ends = []
        for name, dtype, shape, off in fields:
            assert off % 16 == 0 and (not ends or off >= ends[-1]), name
            n = 1
            for s in shape:
                n *= s
            ends.append(off + n * torch.empty((), dtype=dtype).element_size())
        assert ends[-1] <= total and 0 < result_bytes < total
        results = [f[0] for f in fields if f[3] < result_bytes]
        assert {"count", "index", "score", "corners8", "keep"} <= set(results) and "aabb" not in results
        assert ("sem_prob" in results) == bool(kw.get("per_class"))
