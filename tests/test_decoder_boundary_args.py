"""CPU: the stage-boundary entry points (include/omnipq_decoder.h: the LayerNorm split variants, omnipq_decode_pair_pos16,
omnipq_merge_rows_f32 / omnipq_split_rows_sum) refuse malformed arguments with OMNIPQ_EINVAL before they touch a device.
Pointers below are never dereferenced: validation comes first."""
import ctypes

import capi

EINVAL = 10001


def test_boundary_entry_points_validate_without_a_gpu(built_lib):
    lib = capi.lib()
    p = ctypes.c_void_p(0x1000)                        # "some non-null pointer"
    null = ctypes.c_void_p(0)
    f, ll = ctypes.c_float, ctypes.c_longlong

    def fwd(R=12, C=40, x=p, gamma=p, beta=p, mean=p, rstd=p, tokens=6, n_obj=2, obj=p, quad=p):
        return lib.omnipq_add_dropout_layernorm_split(ll(R), C, x, p, gamma, beta, f(1e-5), f(0.0), null, 0, p, p, null, null,
                                                      mean, rstd, tokens, n_obj, obj, quad, null)

    for bad in (dict(x=null), dict(gamma=null), dict(beta=null), dict(mean=null), dict(rstd=null), dict(obj=null),
                dict(quad=null), dict(tokens=0), dict(tokens=-6), dict(tokens=5), dict(n_obj=-1), dict(n_obj=7), dict(C=36),
                dict(C=42), dict(R=13)):
        assert fwd(**bad) == EINVAL, bad
    assert fwd(n_obj=0, quad=null) == EINVAL and fwd(n_obj=6, obj=null) == EINVAL
    assert fwd(R=0) == 0                               # nothing to do: succeeds without a device

    def bwd(fn, R=12, C=40, x=p, gamma=p, mean=p, rstd=p, dx=p, y=p, dy=p, tokens=6, n_obj=2, out=p):
        return fn(ll(R), C, x, y, gamma, f(0.0), null, 0, mean, rstd, p, p, null, dx, dy, out, tokens, n_obj, p, null, null)

    for fn in (lib.omnipq_add_dropout_layernorm_bwd_split, lib.omnipq_add_dropout_layernorm_bwd_partials_split):
        for bad in (dict(x=null), dict(gamma=null), dict(mean=null), dict(rstd=null), dict(dx=null), dict(out=null),
                    dict(dy=null), dict(y=null), dict(tokens=0), dict(tokens=5), dict(n_obj=-1), dict(n_obj=7), dict(C=36),
                    dict(R=13)):
            assert bwd(fn, **bad) == EINVAL, (fn.__name__, bad)
        assert bwd(fn, R=0) == 0

    ptrs10 = (ctypes.c_void_p * 10)(*([0x1000] * 10))
    ptrs4 = (ctypes.c_void_p * 4)(*([0x1000] * 4))

    def decode(pos=p, pos16=p, kpad=32, yh=p, norm=p, Kq=2, ldyh=32):
        return lib.omnipq_decode_pair_pos16(6, 3, 1, 2, 3, yh, ldyh, p, p, f(3.14), ptrs10, 4, Kq, p, 16, p, ptrs4, norm, pos,
                                            pos16, kpad, null)

    for bad in (dict(pos=null), dict(pos16=null), dict(kpad=2), dict(kpad=0), dict(kpad=-32), dict(yh=null), dict(norm=null),
                dict(Kq=4), dict(Kq=3), dict(ldyh=8)):                       # Kq = 4: one scene of quads against two of objects
        assert decode(**bad) == EINVAL, bad

    def join(b=2, tokens=6, n_obj=2, c=40, obj=p, quad=p, out32=p, out16=p):
        return lib.omnipq_merge_rows_f32(b, tokens, n_obj, c, obj, quad, out32, out16, null)

    def unjoin(b=2, tokens=6, n_obj=2, c=40, d_obj=p, d_quad=p):
        return lib.omnipq_split_rows_sum(b, tokens, n_obj, c, p, p, d_obj, d_quad, null)

    for bad in (dict(obj=null), dict(quad=null), dict(out32=null), dict(out16=null), dict(tokens=0), dict(n_obj=-1),
                dict(n_obj=7), dict(c=36), dict(c=0), dict(b=-1)):
        assert join(**bad) == EINVAL, bad
    for bad in (dict(d_obj=null), dict(d_quad=null), dict(tokens=0), dict(n_obj=-1), dict(n_obj=7), dict(c=36), dict(b=-1)):
        assert unjoin(**bad) == EINVAL, bad
    assert join(b=0) == 0 and unjoin(b=0) == 0
