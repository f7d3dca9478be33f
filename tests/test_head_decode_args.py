"""CPU: the decode entry points of the prediction heads (include/omnipq_decoder.h: omnipq_head_decode, omnipq_quad_decode,
their _bwd twins, omnipq_decode_pair, omnipq_decode_pair_pos16, omnipq_decode_pair_bwd, omnipq_decode_pair_group_bwd) refuse
malformed arguments with OMNIPQ_EINVAL before they touch a device: every required pointer null in turn, every lower bound one
below in turn, rows that are no multiple of the proposals per scene, too many quad rows, a gradient's n2 below one, positions
with unequal scene counts, a sink next to a stage's own base gradient.  Device pointers below are never dereferenced:
validation comes first; the HOST arrays (output pointers, gradient descriptors, per-stage pointers) are real."""
import ctypes

import capi

EINVAL = 10001
NH, NS, NCLS = 1, 2, 3
WIDTH = 5 + 2 * NH + 4 * NS + NCLS                     # 18
P = 0x1000                                             # "some non-null device pointer"


def _ptrs(n, hole=None):
    return (ctypes.c_void_p * n)(*[None if i == hole else P for i in range(n)])


def _ints(n, value=1, hole=None, low=0):
    return (ctypes.c_int * n)(*[low if i == hole else value for i in range(n)])


def _check(call, good, bad_cases):
    """every case of bad_cases, one changed argument each, is refused; nothing else about `good` is"""
    for bad in bad_cases:
        assert call(**dict(good, **bad)) == EINVAL, (call.__name__, sorted(bad))


def _nulls(*names):
    return [{n: None} for n in names]


def test_single_decodes_validate_without_a_gpu(built_lib):
    lib = capi.lib()
    f = ctypes.c_float

    def head_decode(R, nh, ns, ncls, y, ldy, base, means, outs):
        return lib.omnipq_head_decode(R, nh, ns, ncls, y, ldy, base, means, f(3.14), outs, None)

    good = dict(R=6, nh=NH, ns=NS, ncls=NCLS, y=P, ldy=WIDTH, base=P, means=P, outs=_ptrs(10))
    _check(head_decode, good, _nulls("y", "base", "means", "outs") + [dict(outs=_ptrs(10, hole=i)) for i in range(10)] +
           [dict(ldy=WIDTH - 1), dict(nh=0), dict(ns=0), dict(ncls=0), dict(R=-1)])
    assert head_decode(**dict(good, R=0)) == 0          # nothing to do: succeeds without a device
    assert head_decode(**dict(good, R=0, nh=0)) == EINVAL

    def head_decode_bwd(R, K, nh, ns, ncls, y, ldy, means, gptr, gstrides, gn2, gbf, dy, lddy, dbase=None):
        return lib.omnipq_head_decode_bwd(R, K, nh, ns, ncls, y, ldy, means, f(3.14), gptr, gstrides, gn2, gbf, dy, lddy,
                                          dbase, None)

    good = dict(R=6, K=3, nh=NH, ns=NS, ncls=NCLS, y=P, ldy=WIDTH, means=P, gptr=_ptrs(10), gstrides=_ints(40),
                gn2=_ints(10), gbf=_ints(10), dy=P, lddy=WIDTH)
    _check(head_decode_bwd, good, _nulls("y", "means", "gptr", "gstrides", "gn2", "gbf", "dy") +
           [dict(gn2=_ints(10, hole=i)) for i in range(10)] +
           [dict(ldy=WIDTH - 1), dict(lddy=WIDTH - 1), dict(nh=0), dict(ns=0), dict(ncls=0), dict(K=0), dict(R=-1), dict(R=7)])
    assert head_decode_bwd(**dict(good, R=0)) == 0
    assert head_decode_bwd(**dict(good, R=0, K=0)) == EINVAL

    def quad_decode(R, y, ldy, base, outs, norm):
        return lib.omnipq_quad_decode(R, y, ldy, base, outs, norm, None)

    good = dict(R=4, y=P, ldy=10, base=P, outs=_ptrs(4), norm=P)
    _check(quad_decode, good, _nulls("y", "base", "outs", "norm") + [dict(outs=_ptrs(4, hole=i)) for i in range(4)] +
           [dict(ldy=9), dict(R=-1), dict(R=(1 << 24) + 1)])
    assert quad_decode(**dict(good, R=0)) == 0

    def quad_decode_bwd(R, K, y, ldy, norm, gptr, gstrides, gbf, dy, lddy, dbase=None):
        return lib.omnipq_quad_decode_bwd(R, K, y, ldy, norm, gptr, gstrides, gbf, dy, lddy, dbase, None)

    good = dict(R=4, K=2, y=P, ldy=10, norm=P, gptr=_ptrs(4), gstrides=_ints(16), gbf=_ints(4), dy=P, lddy=10)
    _check(quad_decode_bwd, good, _nulls("y", "norm", "gptr", "gstrides", "gbf", "dy") +
           [dict(ldy=9), dict(lddy=9), dict(K=0), dict(R=-1), dict(R=5), dict(R=(1 << 24) + 2)])
    assert quad_decode_bwd(**dict(good, R=0)) == 0
    assert quad_decode_bwd(**dict(good, R=0, K=0)) == EINVAL


def test_pair_decodes_validate_without_a_gpu(built_lib):
    lib = capi.lib()
    f = ctypes.c_float

    def pair(fn, Rh, Kh, nh, ns, ncls, yh, ldyh, baseh, means, outs_h, Rq, Kq, yq, ldyq, baseq, outs_q, norm, pos, *tail):
        return fn(Rh, Kh, nh, ns, ncls, yh, ldyh, baseh, means, f(3.14), outs_h, Rq, Kq, yq, ldyq, baseq, outs_q, norm, pos,
                  *tail, None)

    def decode_pair(**kw):
        return pair(lib.omnipq_decode_pair, **kw)

    def decode_pair_pos16(pos16, kpad, **kw):
        order = ("Rh", "Kh", "nh", "ns", "ncls", "yh", "ldyh", "baseh", "means", "outs_h", "Rq", "Kq", "yq", "ldyq", "baseq",
                 "outs_q", "norm", "pos")
        return pair(lib.omnipq_decode_pair_pos16, *[kw[n] for n in order], pos16, kpad)

    good = dict(Rh=6, Kh=3, nh=NH, ns=NS, ncls=NCLS, yh=P, ldyh=WIDTH, baseh=P, means=P, outs_h=_ptrs(10), Rq=4, Kq=2, yq=P,
                ldyq=10, baseq=P, outs_q=_ptrs(4), norm=P, pos=P)
    common = _nulls("yh", "baseh", "means", "outs_h", "yq", "baseq", "outs_q", "norm") + \
        [dict(outs_h=_ptrs(10, hole=i)) for i in range(10)] + [dict(outs_q=_ptrs(4, hole=i)) for i in range(4)] + \
        [dict(ldyh=WIDTH - 1), dict(ldyq=9), dict(nh=0), dict(ns=0), dict(ncls=0), dict(Kh=0), dict(Kq=0), dict(Rh=0),
         dict(Rh=-6), dict(Rq=0), dict(Rq=-4), dict(Rh=7), dict(Rq=5), dict(Rq=(1 << 24) + 2),
         dict(Kq=4), dict(Kq=1)]                       # Kq = 4 / 1: one / four scenes of quads against two of objects, with pos
    _check(decode_pair, good, common)
    _check(decode_pair_pos16, dict(good, pos16=P, kpad=32),
           common + _nulls("pos", "pos16") + [dict(kpad=2), dict(kpad=0), dict(kpad=-32)])

    def decode_pair_bwd(Rh, Kh, nh, ns, ncls, yh, ldyh, means, gptr_h, gstrides_h, gn2_h, gbf_h, dyh, lddyh, Rq, Kq, yq, ldyq,
                        norm, gptr_q, gstrides_q, gbf_q, dyq, lddyq, dbaseh=None, dbaseq=None, accumulate=0):
        return lib.omnipq_decode_pair_bwd(Rh, Kh, nh, ns, ncls, yh, ldyh, means, f(3.14), gptr_h, gstrides_h, gn2_h, gbf_h, dyh,
                                          lddyh, dbaseh, Rq, Kq, yq, ldyq, norm, gptr_q, gstrides_q, gbf_q, dyq, lddyq, dbaseq,
                                          accumulate, None)

    good = dict(Rh=6, Kh=3, nh=NH, ns=NS, ncls=NCLS, yh=P, ldyh=WIDTH, means=P, gptr_h=_ptrs(10), gstrides_h=_ints(40),
                gn2_h=_ints(10), gbf_h=_ints(10), dyh=P, lddyh=WIDTH, Rq=4, Kq=2, yq=P, ldyq=10, norm=P, gptr_q=_ptrs(4),
                gstrides_q=_ints(16), gbf_q=_ints(4), dyq=P, lddyq=10)
    bwd_common = _nulls("yh", "means", "gptr_h", "gstrides_h", "gn2_h", "gbf_h", "dyh", "yq", "norm", "gptr_q", "gstrides_q",
                        "gbf_q", "dyq") + [dict(gn2_h=_ints(10, hole=i)) for i in range(10)] + \
        [dict(ldyh=WIDTH - 1), dict(lddyh=WIDTH - 1), dict(ldyq=9), dict(lddyq=9), dict(nh=0), dict(ns=0), dict(ncls=0),
         dict(Kh=0), dict(Kq=0), dict(Rh=0), dict(Rh=-6), dict(Rq=0), dict(Rq=-4), dict(Rh=7), dict(Rq=5),
         dict(Rq=(1 << 24) + 2)]
    _check(decode_pair_bwd, good, bwd_common)

    def group_bwd(nstage, Rh, Kh, nh, ns, ncls, yh, ldyh, means, gptr_h, gstrides_h, gn2_h, gbf_h, dyh, lddyh, Rq, Kq, yq,
                  ldyq, norm, gptr_q, gstrides_q, gbf_q, dyq, lddyq, dbaseh=None, dbaseq=None, sink=None, accumulate=0):
        return lib.omnipq_decode_pair_group_bwd(nstage, Rh, Kh, nh, ns, ncls, yh, ldyh, means, f(3.14), gptr_h, gstrides_h,
                                                gn2_h, gbf_h, dyh, lddyh, dbaseh, Rq, Kq, yq, ldyq, norm, gptr_q, gstrides_q,
                                                gbf_q, dyq, lddyq, dbaseq, sink, accumulate, None)

    n = 3
    good = dict(nstage=n, Rh=6, Kh=3, nh=NH, ns=NS, ncls=NCLS, yh=_ptrs(n), ldyh=WIDTH, means=_ptrs(n), gptr_h=_ptrs(10 * n),
                gstrides_h=_ints(40 * n), gn2_h=_ints(10), gbf_h=_ints(10 * n), dyh=_ptrs(n), lddyh=WIDTH, Rq=4, Kq=2,
                yq=_ptrs(n), ldyq=10, norm=_ptrs(n), gptr_q=_ptrs(4 * n), gstrides_q=_ints(16 * n), gbf_q=_ints(4 * n),
                dyq=_ptrs(n), lddyq=10)
    per_stage = [{name: _ptrs(n, hole=s)} for name in ("yh", "means", "dyh", "yq", "norm", "dyq") for s in range(n)]
    _check(group_bwd, good, bwd_common + per_stage + [dict(nstage=0), dict(nstage=65), dict(nstage=-1)] +
           [dict(sink=P, dbaseh=(ctypes.c_void_p * n)(*[P if s == t else None for s in range(n)])) for t in range(n)])
