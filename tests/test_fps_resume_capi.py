"""CPU: omnipq_furthest_point_sampling_resume is exported by both element-type libraries, at the ABI version the binding asks for, and
validates its arguments before it touches the device.  No kernel is launched here; pointers are never dereferenced."""
import ctypes

import capi

EINVAL = 10001
NAME = "omnipq_furthest_point_sampling_resume"


def test_resume_is_declared_and_exported_by_both_libraries(built_lib):
    assert NAME in capi.declared_symbols()
    for path in (built_lib, built_lib[:-3] + "_f16.so"):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, NAME), path
        assert lib.omnipq_abi_version() == 5
    import pointnet2_utils
    assert pointnet2_utils._ext.ABI_VERSION == 5
    assert callable(pointnet2_utils._ext.furthest_point_sampling_resume)


def test_resume_validates_before_it_touches_the_device(built_lib):
    lib = capi.lib()
    fn = getattr(lib, NAME)
    p = ctypes.c_void_p(0x1000)                       # "some non-null pointer"
    null = ctypes.c_void_p(0)
    flags = ctypes.c_uint(0)

    def call(b, n, m, first, count, dataset=p, temp=p, idxs=p, fl=flags):
        return fn(b, n, m, first, count, dataset, temp, idxs, fl, null)

    assert call(2, 100, 16, -1, 4) == EINVAL                      # first < 0
    assert call(2, 100, 16, 4, -1) == EINVAL                      # count < 0
    assert call(2, 100, 16, 8, 9) == EINVAL                       # first + count > m
    assert call(2, 100, 16, 17, 0) == EINVAL                      # ... also for an empty piece
    assert call(2, 100, 16, 0, 17) == EINVAL
    assert call(2, 100, 16, 2 ** 31 - 1, 2 ** 31 - 1) == EINVAL   # the sum does not wrap
    assert call(-1, 100, 16, 0, 16) == EINVAL and call(2, -1, 16, 0, 16) == EINVAL and call(2, 100, -1, 0, 0) == EINVAL
    assert call(2, 0, 16, 0, 16) == EINVAL                        # no points to sample from
    for fl in (ctypes.c_uint(0), ctypes.c_uint(1)):
        assert call(2, 100, 16, 4, 4, dataset=null, fl=fl) == EINVAL
        assert call(2, 100, 16, 4, 4, temp=null, fl=fl) == EINVAL
        assert call(2, 100, 16, 4, 4, idxs=null, fl=fl) == EINVAL
    # empty pieces and empty batches succeed and write nothing
    assert call(2, 100, 16, 0, 0) == 0
    assert call(2, 100, 16, 16, 0) == 0
    assert call(2, 100, 16, 7, 0, dataset=null, temp=null, idxs=null) == 0
    assert call(0, 100, 16, 3, 5) == 0
    assert call(2, 100, 0, 0, 0) == 0
    # the entry points it now serves keep their own checks
    assert lib.omnipq_furthest_point_sampling_ex(2, 100, 16, null, p, p, flags, null) == EINVAL
    assert lib.omnipq_furthest_point_sampling_ex(2, 100, 0, p, p, p, flags, null) == 0
    assert lib.omnipq_furthest_point_sampling(0, 100, 16, p, p, p, null) == 0
    assert lib.omnipq_furthest_point_sampling(2, 100, -1, p, p, p, null) == EINVAL


def test_sampler_rejects_bad_arguments_without_a_gpu(built_lib):
    import pytest
    import torch
    import pointnet2_utils
    with pytest.raises(ValueError):
        pointnet2_utils.FurthestPointSampler((2, 100, 4), 16, "cuda")
    with pytest.raises(ValueError):
        pointnet2_utils.FurthestPointSampler((2, 100), -1, "cuda")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils.FurthestPointSampler((2, 100), 16, "cpu")
    with pytest.raises(RuntimeError, match="CPU not supported"):
        pointnet2_utils._ext.furthest_point_sampling_resume(torch.rand(2, 100, 3), torch.zeros(2, 16, dtype=torch.int32),
                                                            torch.full((2, 100), 1e10), 0, 16)
