"""CPU: the entry points of include/omnipq_normals.h are exported by both libraries with typed signatures, and every refusal
the header lists comes back before the device is touched: the pointers below are never dereferenced, and nothing is launched."""
import ctypes

import capi
from test_capi_symbols import both

EINVAL = 10001
P = ctypes.c_void_p(0x1000)                               # "some non-null pointer"
NULL = ctypes.c_void_p(0)
f = ctypes.c_float

SIGNATURES = {"omnipq_knn_workspace_bytes": ("l", "iii"), "omnipq_knn": ("i", "iiiifpppppp"),
              "omnipq_normals_plane_fit": ("i", "iiippppp"), "omnipq_normals_smooth": ("i", "iiipppp"),
              "omnipq_normals_orient": ("i", "iipppp"), "omnipq_estimate_normals_workspace_bytes": ("l", "iii"),
              "omnipq_estimate_normals": ("i", "iiiifppppp")}


def libs(built_lib):
    out = []
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        for name in ("omnipq_knn_workspace_bytes", "omnipq_estimate_normals_workspace_bytes"):
            getattr(lib, name).restype = ctypes.c_longlong
        out.append(lib)
    return out


def test_symbols_are_exported_and_typed(built_lib):
    want = capi.declared_signatures()
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name, sig in SIGNATURES.items():
            assert hasattr(lib, name) and got[name] == want[name] == sig, (path, name)
        assert lib.omnipq_abi_version() == 5                 # additive: the version stays
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    assert ext._lib0.omnipq_knn.argtypes[4] is ctypes.c_float and ext._lib0.omnipq_knn_workspace_bytes.restype is ctypes.c_longlong
    assert callable(pointnet2_utils.knn_query) and ext.KNN_MAX_K == 128


def test_workspace_bytes(built_lib):
    H = 8192
    for lib in libs(built_lib):
        knn = lib.omnipq_knn_workspace_bytes
        assert knn(2, 1000, 37) == 2 * (1000 * 4 + (H + 1) * 4 + 1000 * 4 + 1000 * 12 + H * 4)
        assert knn(0, 1000, 5) == 0 and knn(3, 0, 0) == 3 * ((H + 1) * 4 + H * 4)
        assert knn(-1, 10, 10) < 0 and knn(1, -10, 10) < 0 and knn(1, 10, -1) < 0
        est = lib.omnipq_estimate_normals_workspace_bytes
        assert est(2, 1000, 100) == knn(2, 1000, 1000) + 2 * 1000 * 100 * 4 + 2 * 1000 * 12
        assert est(-1, 10, 8) < 0 and est(1, -1, 8) < 0 and est(1, 10, 0) < 0 and est(1, 10, 129) < 0 and est(65536, 10, 8) < 0
        assert est(65535, 50000, 128) > 2 ** 40              # no 32-bit overflow


def test_every_refusal_comes_before_the_device(built_lib):
    for lib in libs(built_lib):
        def knn(b=2, n=100, m=50, k=8, cell=0.2, q=P, xyz=P, idx=P, d2=P, ws=P):
            return lib.omnipq_knn(b, n, m, k, f(cell), q, xyz, idx, d2, ws, NULL)

        for kw in ({"k": 0}, {"k": -3}, {"k": 129}, {"cell": 0.0}, {"cell": -0.2}, {"cell": float("nan")}, {"cell": float("inf")},
                   {"b": -1}, {"n": -1}, {"m": -1}, {"b": 65536}, {"q": NULL}, {"xyz": NULL}, {"idx": NULL}, {"ws": NULL}):
            assert knn(**kw) == EINVAL, kw
        assert knn(b=0, q=NULL, xyz=NULL, idx=NULL, ws=NULL) == 0 and knn(m=0, q=NULL, idx=NULL, ws=NULL) == 0
        assert knn(b=0, k=0) == EINVAL                       # a bad k is refused whatever the sizes

        def fit(b=2, n=100, k=8, xyz=P, idx=P, out=P, eig=NULL):
            return lib.omnipq_normals_plane_fit(b, n, k, xyz, idx, out, eig, NULL)

        for kw in ({"k": 0}, {"k": 129}, {"b": -1}, {"n": -1}, {"b": 65536}, {"xyz": NULL}, {"idx": NULL}, {"out": NULL}):
            assert fit(**kw) == EINVAL, kw
        assert fit(b=0, xyz=NULL) == 0 and fit(n=0, xyz=NULL, idx=NULL, out=NULL) == 0

        def smooth(b=2, n=100, k=8, idx=P, src=P, dst=ctypes.c_void_p(0x2000)):
            return lib.omnipq_normals_smooth(b, n, k, idx, src, dst, NULL)

        for kw in ({"k": 0}, {"k": 129}, {"b": -1}, {"n": -1}, {"b": 65536}, {"idx": NULL}, {"src": NULL}, {"dst": NULL},
                   {"dst": P}):                              # in place: the step reads its neighbours' previous values
            assert smooth(**kw) == EINVAL, kw
        assert smooth(b=0, idx=NULL) == 0 and smooth(n=0, idx=NULL, src=NULL, dst=NULL) == 0

        def orient(b=2, n=100, xyz=P, centre=P, nrm=P):
            return lib.omnipq_normals_orient(b, n, xyz, centre, nrm, NULL)

        for kw in ({"b": -1}, {"n": -1}, {"b": 65536}, {"xyz": NULL}, {"centre": NULL}, {"nrm": NULL}):
            assert orient(**kw) == EINVAL, kw
        assert orient(b=0, xyz=NULL) == 0 and orient(n=0, xyz=NULL, centre=NULL, nrm=NULL) == 0

        def est(b=2, n=100, k=8, iters=5, cell=0.2, xyz=P, centre=P, out=P, ws=P):
            return lib.omnipq_estimate_normals(b, n, k, iters, f(cell), xyz, centre, out, ws, NULL)

        for kw in ({"k": 0}, {"k": 129}, {"iters": -1}, {"cell": 0.0}, {"cell": float("nan")}, {"b": -1}, {"n": -1}, {"b": 65536},
                   {"xyz": NULL}, {"centre": NULL}, {"out": NULL}, {"ws": NULL}):
            assert est(**kw) == EINVAL, kw
        assert est(b=0, xyz=NULL, ws=NULL) == 0 and est(n=0, xyz=NULL, centre=NULL, out=NULL, ws=NULL) == 0


def test_scene_bank_takes_scenes_without_normals_on_the_host(built_lib):
    """registration is host work: the old positional order still binds, `normals` may be left out, nothing else may"""
    import numpy as np
    import pytest
    import device_data as D
    rng = np.random.RandomState(0)
    pts = rng.rand(64, 3).astype(np.float32)
    boxes = np.array([[0.5, 0.5, 0.5, 0.2, 0.2, 0.2, 0.1]])
    bank = D.SceneBank("cpu")
    assert bank.add_unlabelled_scene("a", pts, np.ones((64, 3), np.float32), boxes) == 0      # positional, as before
    assert bank.add_unlabelled_scene("b", pts, boxes=boxes) == 1 and bank.add_unlabelled_scene("c", pts, None, boxes) == 2
    assert [r["estimate_normals"] for r in bank._rows] == [False, True, True]
    assert bank._rows[1]["normals"].shape == (64, 3) and bank._rows[1]["normals"].dtype == np.float32
    with pytest.raises(TypeError, match="only `normals`"):
        bank.add_unlabelled_scene("d", pts)
    with pytest.raises(ValueError, match="differ in length"):
        bank.add_unlabelled_scene("e", pts, np.ones((63, 3), np.float32), boxes)
    cell = D._ext.default_knn_cell(pts.min(0), pts.max(0), 64, 100)
    assert 0 < cell < 10 and D._ext.default_knn_cell([0, 0, 0], [0, 0, 0], 1, 100) == 1.0
