"""CPU: the entry points of the split attention backward (include/omnipq_attn.h: omnipq_attn_bwd_dq, omnipq_attn_bwd_dkdv,
omnipq_attn_bwd_mode) are exported and reported by both libraries, and the two launching ones validate their arguments as
omnipq_attn_bwd does -- OMNIPQ_EINVAL / OMNIPQ_ETOOLARGE before anything touches a device.  No kernel is launched here:
the pointers below are never dereferenced."""
import ctypes

import capi

EINVAL, ETOOLARGE = 10001, 10002
NEW = {"omnipq_attn_bwd_dq": ("i", "iiiiippppppppppfpup"), "omnipq_attn_bwd_dkdv": ("i", "iiiiippppppppppfpup"),
       "omnipq_attn_bwd_mode": ("v", "i")}
p = ctypes.c_void_p(0x1000)                           # "some non-null pointer"
null = ctypes.c_void_p(0)
f, ll = ctypes.c_float, ctypes.c_longlong
GOOD = [288, 2304, 288, 2304, 288, 2304, 288, 2304]
DIMS = (8, 8, 256, 256, 36)


def both(built_lib):
    return [built_lib, built_lib[:-3] + "_f16.so"]


def dq(lib, dims=DIMS, st=GOOD, gst=(288, 2304), q=p, o=p, d_o=p, delta=p, out=p, drop=0.0, seed=null):
    return lib.omnipq_attn_bwd_dq(*dims, q, p, p, o, d_o, (ll * 8)(*st), p, delta, out, (ll * 2)(*gst), f(drop), seed, 0, null)


def dkdv(lib, dims=DIMS, st=GOOD, gst=(288, 2304, 288, 2304), q=p, o=p, d_o=p, dk=p, dv=p, drop=0.0, seed=null):
    return lib.omnipq_attn_bwd_dkdv(*dims, q, p, p, o, d_o, (ll * 8)(*st), p, dk, dv, (ll * 4)(*gst), f(drop), seed, 0, null)


def test_both_libraries_export_and_report_the_new_entry_points(built_lib):
    declared = capi.declared_signatures()
    for name, sig in NEW.items():
        assert declared[name] == sig, name
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        got = capi.reported_signatures(lib)
        for name, sig in NEW.items():
            assert hasattr(lib, name) and got[name] == sig, (path, name)
    import pointnet2_utils
    ext = pointnet2_utils._load_ext()
    for lib in ext._LIBS.values():
        assert len(lib.omnipq_attn_bwd_dkdv.argtypes) == 19 and lib.omnipq_attn_bwd_mode.restype is None


def test_null_pointers_are_refused(built_lib):
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        for arg in ("o", "dk", "dv", "q", "d_o"):
            assert dkdv(lib, **{arg: null}) == EINVAL, arg
        for arg in ("o", "delta", "out", "q", "d_o"):
            assert dq(lib, **{arg: null}) == EINVAL, arg
        assert lib.omnipq_attn_bwd_dkdv(*DIMS, p, p, p, p, p, null, p, p, p, (ll * 4)(288, 2304, 288, 2304), f(0.0), null, 0,
                                        null) == EINVAL                                 # no strides
        assert lib.omnipq_attn_bwd_dkdv(*DIMS, p, p, p, p, p, (ll * 8)(*GOOD), p, p, p, null, f(0.0), null, 0, null) == EINVAL
        assert lib.omnipq_attn_bwd_dq(*DIMS, p, p, p, p, p, (ll * 8)(*GOOD), p, p, p, null, f(0.0), null, 0, null) == EINVAL
        assert dkdv(lib, drop=0.1) == EINVAL and dq(lib, drop=0.1) == EINVAL            # dropout without a seed
        assert dkdv(lib, drop=1.0, seed=p) == EINVAL and dq(lib, drop=1.0, seed=p) == EINVAL


def test_strides_are_validated_like_the_whole_backward(built_lib):
    lib = capi.lib()
    for i in range(8):                                 # a stride that is no multiple of 4
        st = list(GOOD)
        st[i] += 2
        assert dq(lib, st=st) == EINVAL and dkdv(lib, st=st) == EINVAL, i
    for i in range(2):
        gst = [288, 2304]
        gst[i] += 2
        assert dq(lib, gst=gst) == EINVAL, i
    for i in range(4):
        gst = [288, 2304, 288, 2304]
        gst[i] += 2
        assert dkdv(lib, gst=gst) == EINVAL, i
    for bad in (-288, -4):                             # a negative token stride has no extent to bound the reads by
        for i in (0, 2, 4, 6):
            st = list(GOOD)
            st[i] = bad
            assert dq(lib, st=st) == EINVAL and dkdv(lib, st=st) == EINVAL, i
        assert dq(lib, gst=[bad, 2304]) == EINVAL
        assert dkdv(lib, gst=[bad, 2304, 288, 2304]) == EINVAL and dkdv(lib, gst=[288, 2304, bad, 2304]) == EINVAL
    for dims in ((8, 8, 256, 256, 37), (8, 8, 256, 256, 52), (0, 8, 256, 256, 36)):
        assert dq(lib, dims=dims) == EINVAL and dkdv(lib, dims=dims) == EINVAL, dims


def test_oversize_problems_are_refused(built_lib):
    lib = capi.lib()
    big = (64, 16, 4096, 4096, 36)                     # N * H * L * S beyond 32-bit indexing
    assert dq(lib, dims=big) == ETOOLARGE and dkdv(lib, dims=big) == ETOOLARGE
    st = list(GOOD)
    st[2] = 1 << 30                                    # a token stride beyond 32-bit byte offsets
    assert dq(lib, st=st) == ETOOLARGE and dkdv(lib, st=st) == ETOOLARGE
    assert dq(lib, gst=[1 << 30, 2304]) == ETOOLARGE
    assert dkdv(lib, gst=[288, 2304, 1 << 30, 2304]) == ETOOLARGE and dkdv(lib, gst=[1 << 30, 2304, 288, 2304]) == ETOOLARGE


def test_mode_switch_needs_no_device(built_lib):
    for path in both(built_lib):
        lib = ctypes.CDLL(path)
        lib.omnipq_attn_bwd_mode.restype = None
        lib.omnipq_attn_bwd_mode(0)
        lib.omnipq_attn_bwd_mode(1)
    # the whole backward still validates first in either mode
    lib = capi.lib()
    for mode in (0, 1):
        lib.omnipq_attn_bwd_mode(mode)
        assert lib.omnipq_attn_bwd(*DIMS, p, p, p, p, p, (ll * 8)(*GOOD), p, p, p, p, null, (ll * 6)(*GOOD[:6]), f(0.0), null, 0,
                                   null) == EINVAL
    lib.omnipq_attn_bwd_mode(1)
