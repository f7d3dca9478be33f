"""The arithmetic of the IoU kernels without a GPU: omni-pq_amd/csrc/obb_iou.h -- what one thread of
csrc/eval_iou.hip computes -- compiled as host C++ with the build's -ffp-contract=off into a small stand-alone program
(tests/obb_iou_host_twin.cpp), under AddressSanitizer and UBSan, against eval_det.box3d_iou.

The program gives every pair a heap block of exactly the kernels' LDS array and the slice of its last thread, so a clip that
produced more vertices than the two buffers hold would write outside the block and stop the run.  The bound on the vertex
count (obb_iou.h) counts outcomes of the `inside` test only; the hostile inputs below are there to make those outcomes
arbitrary: zero-sized, denormal-sized, infinite and NaN boxes, and pairs equal up to a few units of 2^-53."""
import os
import subprocess
import warnings

import numpy as np
import pytest

from conftest import PKG
import test_parse_quads
from test_eval_det_device_host import box, degenerate_pairs, host_pairs

TOL = 1e-12               # as tests/test_gpu_eval_det_device.py: only the order of the shoelace sums differs from the host's


def compiler():
    import build as omnipq_build
    clang = os.path.join(os.path.dirname(os.path.realpath(omnipq_build.hipcc())), "..", "lib", "llvm", "bin", "clang++")
    for cand in (clang, "/opt/rocm/lib/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    return "g++"


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("obb_iou") / "obb_iou_host_twin")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "obb_iou_host_twin.cpp")
    cmd = [compiler(), "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(PKG, "csrc"), "-o", exe, src]
    done = subprocess.run(cmd, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr

    def run(a, b):
        work = os.path.dirname(exe)
        with open(os.path.join(work, "in.bin"), "wb") as fh:
            fh.write(np.int64(len(a)).tobytes() + np.ascontiguousarray(a, np.float64).tobytes()
                     + np.ascontiguousarray(b, np.float64).tobytes())
        # no leak check at exit: it needs ptrace, which a container may deny, and is not what this run is for
        done = subprocess.run([exe, os.path.join(work, "in.bin"), os.path.join(work, "out.bin")], capture_output=True, text=True,
                              env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert done.returncode == 0, done.stderr[-2000:]
        out = np.fromfile(os.path.join(work, "out.bin"), dtype=np.float64).reshape(len(a), 2)
        return out[:, 0], out[:, 1]

    return run


def test_twin_equals_the_host_on_the_reference_samples_and_the_degenerate_pairs(twin):
    boxes = test_parse_quads.GOLD["iou.boxes"]
    ia = [i for i in range(0, 40, 2) for j in range(1, 40, 2)]
    ib = [j for i in range(0, 40, 2) for j in range(1, 40, 2)]
    da, db, _ = degenerate_pairs()
    rs = np.random.RandomState(0)
    ra = np.stack([box(*(rs.rand(2) * 2), 0.3 + rs.rand(), 0.3 + rs.rand(), rs.rand() * 0.3, 0.5 + rs.rand(), rs.rand() * 7)
                   for _ in range(600)])
    rb = np.stack([box(*(rs.rand(2) * 2), 0.3 + rs.rand(), 0.3 + rs.rand(), rs.rand() * 0.3, 0.5 + rs.rand(), rs.rand() * 7)
                   for _ in range(600)])
    a, b = np.concatenate([boxes[ia], da, ra]), np.concatenate([boxes[ib], db, rb])
    got3, got2 = twin(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # the identical rotated pair divides by zero, here as there
        want3, want2 = host_pairs(a, b)
    assert np.abs(got3[:400] - test_parse_quads.GOLD["iou.values"]).max() <= TOL
    nan = np.isnan(want3)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got3), nan) and np.array_equal(np.isnan(got2), np.isnan(want2))
    assert np.abs(got3 - want3)[~nan].max() <= TOL and np.abs(got2 - want2)[~nan].max() <= TOL
    assert np.array_equal(got3 == 0, want3 == 0) and np.array_equal(got2 == 0, want2 == 0)
    assert (want3[400 + len(da):] > 0).sum() > 150                                  # the random pairs do overlap


def test_twin_stays_inside_its_buffers_on_hostile_boxes(twin):
    """No value is compared where the problem is ill-conditioned (for a box of 1e-300 m, or two boxes 1e-16 apart, the order
    of a sum decides every digit of the result): the run must end clean under the sanitizers, and the result must be NaN
    exactly where the host's is, since NaN comes from the clip's decisions and divisions, which are the host's."""
    rs = np.random.RandomState(1)
    unit = box(0, 0)
    with np.errstate(invalid="ignore"):
        a = [box(0, 0, 0, 0), box(0, 0, 1e-300, 1e-300), unit * np.inf, unit * np.nan, unit, box(0, 0, 1e-9, 1e-9, ang=0.3),
             np.where(np.arange(24).reshape(8, 3) % 5 == 0, np.nan, unit), box(1e150, -1e150, 1e140, 1e160)]
        b = [box(0, 0, 0, 0), box(0, 0, 1e-300, 1e-300), unit, unit, unit * -np.inf, box(0, 0, 1e-9, 1e-9, ang=0.3),
             unit, box(1e150, -1e150, 1e160, 1e140, ang=1.0)]
    for _ in range(1500):                                             # tiny boxes: products underflow towards denormals
        a.append(box(*(rs.rand(2) * 1e-160), 1e-160 * rs.rand(), 1e-160 * rs.rand(), ang=rs.rand()))
        b.append(box(*(rs.rand(2) * 1e-160), 1e-160 * rs.rand(), 1e-160 * rs.rand(), ang=rs.rand()))
    for _ in range(3000):                                             # the same box up to rounding noise, and exactly
        one = box(*rs.rand(2), 0.2 + rs.rand(), 0.2 + rs.rand(), ang=rs.rand() * 7)
        a.append(one)
        b.append(one + (rs.rand() < 0.7) * rs.randn(8, 3) * 1e-16)
    a, b = np.stack(a), np.stack(b)
    got3, got2 = twin(a, b)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        want3, want2 = host_pairs(a, b)
    assert np.array_equal(np.isnan(got3), np.isnan(want3)) and np.array_equal(np.isnan(got2), np.isnan(want2))
    assert 100 < np.isnan(want3).sum() < len(a) - 100                  # both outcomes occur
    assert np.array_equal(np.isinf(got3), np.isinf(want3)) and np.array_equal(np.isinf(got2), np.isinf(want2))
