"""GPU: the supervised-loss row kernels (csrc/loss_rows.hip) through the C ABI of include/omnipq_loss.h against the float64
reference, ELEMENT BY ELEMENT.

Every entry point but the two nn_distance ones (tests/test_nn_distance.py) is called directly, in both libraries, with
descriptors built from pointnet2._ext.struct(...) as models/loss_helper_pq.py builds them, on the case tables of
tests/loss_rows_reference.py.  Every buffer, input or output, sits between two guard bands and is filled with a NaN pattern
beforehand (float32 and float64 NaNs, int64 / int32 garbage: test_gpu_decoder_f64.Buf knows the 16-bit types and f32 only, the
other patterns live here); every output has one spare row that must keep the pattern.  After every call: the guards hold the
pattern, the inputs are bit-identical, every owned element is written and finite, structural zeros are the bits of +0.0,
discrete outputs (label, mask, assignment, counts, the collision count; the winning vote and every gate through the zeros they
imply) equal the numpy-float32 emulation exactly, and every continuous element lies within error / bound <= 1 / MARGIN of the
float64 reference.  Every forward runs twice into fresh scratch and both results must pass: the f64 atomics make the sums
order-dependent in their last bits, which the bounds cover.  tests/test_loss_rows_reference.py holds the emulation, and
sixteen mutants of it, against the same bounds on the same cases.

Each test prints the largest error / bound ratio per output (`RATIO <library> <case>: terms=... center=...`, pytest -s).
Largest ratios per output over all cases, measured on an MI355X (the case that set it; the kernels are f32 in both libraries
and the bfloat16 and the half library gave the same figures to three digits):
    assign      label, mask, assignment, counts: equal to the emulation bit for bit on all seven cases
    box rows    terms 0.165  box-R1-h1-w1            objectness_scores 0.393  box-R513-h3-kink     center 0.378  box-R257-h1-equal
                heading_scores 0.363  box-R513-h3-kink     heading_residuals_normalized 0.243  box-R256-h8-pm60
                size_scores 0.322  box-R513-h3-kink  size_residuals_normalized 0.498  box-R256-h8-pm60
                sem_cls_scores 0.318  box-R513-h3-kink
    quad rows   terms 0.165  quad-R257-h8-kink       quad_scores 0.432  quad-R513-h1-mixed         quad_center 0.292  quad-R513-h1-mixed
                normal_vector 0.159  quad-R256-h7    quad_size 0.157  quad-R257-h8-kink
    votes       loss 0.137, grad 0.415  votes-1x33x40-f1-g1
    physical    out 0.039  pc-outside                g_center 0.109  pc-2x513-q7                   g_size_residuals 0.090  pc-2x65-q5
                g_quad_center 0.512, g_normal 0.372  pc-1x20-q600          collisions: equal to the emulation on all thirteen cases
Nothing is above 1 / MARGIN, no guard was touched, every decision is the emulation's.  The figures are the emulation's own
(tests/test_loss_rows_reference.py) except on the cross-entropy outputs, where the device's expf / logf differ from the
correctly rounded ones of the emulation by a few hundredths of the bound.  One deviation from the +0.0 rule was found while
the suite was written, by reading the kernel against that rule, and fixed before the device run: omnipq_loss_votes_grad wrote
g_loss * 0 * sign(...) into the winning vote of a seed WITHOUT a vote label, which is -0.0 when g_loss and the sign differ
(votes-mask0 and votes-2x100x150-f3-g3 have a negative g_loss); such a vote now receives +0.0 like every other structural zero.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import loss_rows_reference as lr
from test_gpu_decoder_f64 import DEV, GUARD, LIBS, LIB_IDS, lib_of

pytestmark = pytest.mark.gpu
F32, F64, I64, I32 = torch.float32, torch.float64, torch.int64, torch.int32
PATTERN = {F32: (torch.int32, 0x7FC00001), F64: (torch.int64, 0x7FF8000000000001), I64: (torch.int64, 0x7FC000017FC00001),
           I32: (torch.int32, 0x7FC00001)}
NP = {np.dtype(np.float32): F32, np.dtype(np.float64): F64, np.dtype(np.int64): I64, np.dtype(np.int32): I32}


class Buf:
    """`numel` elements of f32 / f64 / int64 / int32 between two guard bands, all of it the pattern of the type; `data` (a
    numpy array of that type) is copied to the front of the owned part and kept for the bit comparison afterwards"""

    def __init__(self, numel, dtype, data=None):
        self.n, self.dtype = numel, dtype
        self.it, self.pat = PATTERN[dtype]
        self.t = torch.empty(numel + 2 * GUARD, dtype=dtype, device=DEV)
        self.t.view(self.it).fill_(self.pat)
        self.src = None
        if data is not None:
            self.src = torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).clone()
            assert self.src.dtype is dtype and self.src.numel() <= numel
            self.t[GUARD:GUARD + self.src.numel()].copy_(self.src)

    def ptr(self):
        return self.t.data_ptr() + GUARD * self.t.element_size()

    def guards_intact(self):
        b = self.t.view(self.it)
        return bool((b[:GUARD] == self.pat).all()) and bool((b[GUARD + self.n:] == self.pat).all())

    def unchanged(self):
        """an input: the guards hold and the owned part is what was copied in, bit for bit"""
        own = self.t[GUARD:GUARD + self.src.numel()].cpu()
        return self.guards_intact() and torch.equal(own.view(self.it), self.src.view(self.it))

    def read(self, rows, width):
        """an output of `rows` rows and one spare row -> numpy (rows, width); every owned element written"""
        assert self.guards_intact(), "wrote outside the buffer"
        b = self.t.view(self.it)[GUARD:GUARD + self.n].cpu()
        assert bool((b[rows * width:] == self.pat).all()), "wrote behind the last row"
        assert not bool((b[:rows * width] == self.pat).any()), "an owned element was not written"
        out = self.t[GUARD:GUARD + rows * width].cpu().numpy().reshape(rows, width)
        assert np.isfinite(out).all()
        return out


def IN(a):
    a = np.asarray(a)
    return Buf(a.size, NP[a.dtype], a)


def OUT(rows, width, dtype=F32):
    return Buf((rows + 1) * width, dtype)


def P(buf):
    return ctypes.c_void_p(0 if buf is None else buf.ptr())


def libname(dtype):
    return LIB_IDS[LIBS.index(dtype)]


def merge(total, new):
    for n, r in new.items():
        total[n] = (max(total[n][0], r[0]), total[n][1] + r[1]) if n in total else r


def report(dtype, id, rat):
    print(f"\n  RATIO {libname(dtype)} {id}: {lr.fmt(rat)}")
    assert not lr.outside(rat), (libname(dtype), id, lr.outside(rat))
    assert all(r[0] <= 1.0 / lr.MARGIN for r in rat.values()), (libname(dtype), id, lr.fmt(rat))


def inputs_unchanged(bufs):
    return all(b.unchanged() for b in bufs)


# ---- assignment -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", lr.ids(lr.ASSIGN_CASES))
def test_assign_equals_the_emulation_exactly(id, dtype):
    lib, stream = lib_of(dtype)
    inp = lr.assign_inputs(lr.case_of(id))
    b, k, k2 = inp["b"], inp["k"], inp["k2"]
    want = lr.assign_emulate(inp)
    ins = [IN(inp["query"]), IN(inp["gt"]), IN(inp["num_gt"])]
    for _ in range(2):
        label, mask, assignment, counts = OUT(b * k, 1, I64), OUT(b * k, 1, F32), OUT(b * k, 1, I64), OUT(1, 2, F32)
        rc = lib.omnipq_loss_assign(b, k, k2, *[P(x) for x in ins], inp["near"], inp["far"], P(label), P(mask), P(assignment),
                                    P(counts), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert inputs_unchanged(ins)
        assert np.array_equal(label.read(b * k, 1).reshape(b, k), want["label"])
        assert np.array_equal(mask.read(b * k, 1).reshape(b, k).view(np.int32), want["mask"].view(np.int32))
        assert np.array_equal(assignment.read(b * k, 1).reshape(b, k), want["assignment"])
        assert np.array_equal(counts.read(1, 2)[0].view(np.int32), want["counts"].view(np.int32))     # garbage before: overwritten
    print(f"\n  EXACT {libname(dtype)} {id}: counts={want['counts'].tolist()}")


# ---- box and quad rows ----------------------------------------------------------------------------------------------------

def rows_call(lib, ext, stream, kind, inp, dtype):
    """forward twice, backward once -> ratios; every check of the module docstring on the way"""
    keys = (lr.BOX_KEYS[:1] if inp["only_objectness"] else lr.BOX_KEYS) if kind == "box" else lr.QUAD_KEYS
    H, R = inp["heads"], inp["b"] * inp["k"]
    desc = ext.struct(f"omnipq_{kind}_rows_desc")()
    for name in ("heads", "b", "k", "k2") + (("nh", "ns", "nc", "only_objectness") if kind == "box" else ()):
        setattr(desc, name, inp[name])
    desc.w_background = float(inp["w"][0])
    setattr(desc, "w_object" if kind == "box" else "w_quad", float(inp["w"][1]))
    ins, heads = {}, {}
    if kind == "box" and inp["only_objectness"]:
        aux = ("label", "mask", "counts")                                          # every optional pointer stays NULL
    else:
        aux = ("label", "mask", "assignment", "counts", "gt_center") + \
            (("gt_heading_class", "gt_heading_residual", "gt_size_class", "gt_size_residual", "gt_sem_cls", "mean_size")
             if kind == "box" else ("gt_normal", "gt_size"))
    for name in aux:
        ins[name] = IN(inp[name])
        setattr(desc, name, ins[name].ptr())
    for key in keys:
        arr = getattr(desc, key)
        for h in range(H):
            heads[key, h] = IN(inp[key][h])
            arr[h] = heads[key, h].ptr()
    every = list(ins.values()) + list(heads.values())
    if kind == "box":
        ref, bnd, zeros = lr.box_reference(inp)
    else:
        ref, bnd, zeros, _ = lr.quad_reference(inp, lr.quad_emulate(inp)["branch"])
    fwd = lib.omnipq_loss_box_rows if kind == "box" else lib.omnipq_loss_quad_rows
    bwd = lib.omnipq_loss_box_rows_grad if kind == "box" else lib.omnipq_loss_quad_rows_grad
    rat = {}
    for _ in range(2):
        sums, terms = OUT(H, 8, F64), OUT(H, 8, F32)
        rc = fwd(ctypes.byref(desc), P(sums), P(terms), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert inputs_unchanged(every)
        sums.read(H, 8)
        got = terms.read(H, 8)
        first_zero = 7 if kind == "box" and not inp["only_objectness"] else (1 if kind == "box" else 4)
        assert lr.plus_zero(got[:, first_zero:]), "terms the contract makes zero are not +0.0"
        if inp["counts"][0] == 0:
            assert lr.plus_zero(got[:, 1:]), "no positive proposal: the positive terms are not +0.0"
        merge(rat, lr.rat(dict(terms=got), ref, bnd))
    grads = ext.struct(f"omnipq_{kind}_rows_grads")()
    g_terms = IN(inp["g_terms"])
    outs = {}
    widths = dict(zip(lr.BOX_KEYS, lr.box_widths(inp["nh"], inp["ns"], inp["nc"]))) if kind == "box" else dict(zip(lr.QUAD_KEYS, lr.QUAD_WIDTHS))
    for key in keys:
        arr = getattr(grads, key)
        for h in range(H):
            if (key, h) not in inp["nulls"]:
                outs[key, h] = OUT(R, widths[key], F32)
                arr[h] = outs[key, h].ptr()
    rc = bwd(ctypes.byref(desc), P(g_terms), ctypes.byref(grads), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert inputs_unchanged(every + [g_terms])
    for (key, h), buf in outs.items():
        got = buf.read(R, widths[key])
        assert lr.plus_zero(got, zeros[key]), (key, h, "a structural zero is not +0.0")
        merge(rat, lr.rat({key: got}, {key: ref["grads"][key][h]}, {key: bnd["grads"][key][h]}))
    assert set(rat) == {"terms"} | {key for key, _ in outs}
    return rat


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", lr.ids(lr.BOX_CASES))
def test_box_rows_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    inp = lr.box_inputs(lr.case_of(id))
    report(dtype, id, rows_call(lib, ext_of(dtype), stream, "box", inp, dtype))


@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", lr.ids(lr.QUAD_CASES))
def test_quad_rows_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    inp = dict(lr.quad_inputs(lr.case_of(id)), only_objectness=0, nh=1, ns=1, nc=1)
    report(dtype, id, rows_call(lib, ext_of(dtype), stream, "quad", inp, dtype))


def ext_of(dtype):
    import capi
    return capi.lib_of(dtype)[1]


# ---- votes ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", lr.ids(lr.VOTE_CASES))
def test_votes_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    inp = lr.votes_inputs(lr.case_of(id))
    b, s, n, vf, gv = inp["dims"]
    emu = lr.votes_emulate(inp)
    ref, bnd, zeros, _ = lr.votes_reference(inp, emu)
    ins = [IN(inp[key]) for key in ("seed_xyz", "vote_xyz", "seed_inds", "vote_label", "vote_label_mask")]
    rat = {}
    for _ in range(2):
        sums, loss = OUT(1, 2, F64), OUT(1, 1, F32)
        rc = lib.omnipq_loss_votes(b, s, n, vf, gv, *[P(x) for x in ins], P(sums), P(loss), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert inputs_unchanged(ins)
        assert sums.read(1, 2)[0, 1] == float(emu["m"].sum())                      # the number of seeds with a vote label
        got = loss.read(1, 1)[0]
        if not emu["m"].any():
            assert lr.plus_zero(got), "no seed has a vote label: the loss is not +0.0"
        merge(rat, lr.rat(dict(loss=got), ref, bnd))
    g_loss, grad = IN(np.array([inp["g_loss"]], dtype=np.float32)), OUT(b * s * vf, 3, F32)
    sums.src = sums.t[GUARD:GUARD + 2].cpu().clone()                                # the backward reads the forward's buffer
    rc = lib.omnipq_loss_votes_grad(b, s, n, vf, gv, *[P(x) for x in ins], P(sums), P(g_loss), P(grad), stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert inputs_unchanged(ins + [g_loss, sums])
    got = grad.read(b * s * vf, 3)
    assert lr.plus_zero(got, zeros), "a vote that does not win, or the vote of a seed without a label, is not +0.0"
    merge(rat, lr.rat(dict(grad=got), ref, bnd))
    report(dtype, id, rat)


# ---- physical constraints -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", LIBS, ids=LIB_IDS)
@pytest.mark.parametrize("id", lr.ids(lr.PC_CASES))
def test_physical_every_element_is_inside_its_bound(id, dtype):
    lib, stream = lib_of(dtype)
    inp = lr.pc_inputs(lr.case_of(id))
    b, k, k2, ns, q = inp["dims"]
    emu = lr.pc_emulate(inp)
    ref, bnd, zeros, _ = lr.pc_reference(inp, emu)
    desc = ext_of(dtype).struct("omnipq_pc_desc")()
    for name, v in zip(("b", "k", "k2", "ns", "q"), inp["dims"]):
        setattr(desc, name, v)
    desc.not_solid = inp["not_solid"]
    ins = {}
    for name in ("center", "size_scores", "size_residuals", "object_label", "object_assignment", "sem_cls_label", "mean_size64",
                 "quad_center", "normal_vector", "quad_size", "quad_label"):
        ins[name] = IN(inp[name])
        setattr(desc, name, ins[name].ptr())
    every = list(ins.values())
    nws = int(lib.omnipq_loss_physical_workspace_floats(b, k))
    assert nws == b * k * 5 + b
    rat = {}
    for _ in range(2):
        ws, sums, out = Buf(nws, F32), OUT(1, 2, F64), OUT(1, 2, F32)
        rc = lib.omnipq_loss_physical(ctypes.byref(desc), P(ws), P(sums), P(out), stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert inputs_unchanged(every) and ws.guards_intact()
        sums.read(1, 2)
        got = out.read(1, 2)[0]
        assert got[1] == emu["out"][1], ("collisions", got[1], emu["out"][1])
        if emu["out"][0] == 0:
            assert lr.plus_zero(got[:1])
        merge(rat, lr.rat(dict(out=got), ref, bnd))
    ws, g_out = Buf(nws, F32), IN(np.array([inp["g_out"]], dtype=np.float32))
    outs = dict(g_center=OUT(b * k, 3), g_size_residuals=OUT(b * k, ns * 3), g_quad_center=OUT(b * q, 3), g_normal=OUT(b * q, 3))
    rc = lib.omnipq_loss_physical_grad(ctypes.byref(desc), P(ws), P(g_out), *[P(outs[n]) for n in lr.PC_GRADS], stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert inputs_unchanged(every + [g_out]) and ws.guards_intact()
    for name in lr.PC_GRADS:
        got = outs[name].read(*((b * k, ns * 3) if name == "g_size_residuals" else (ref[name].shape[0] * ref[name].shape[1], 3)))
        got = got.reshape(ref[name].shape)
        assert lr.plus_zero(got, zeros[name]), (name, "a structural zero is not +0.0")
        merge(rat, lr.rat({name: got}, ref, bnd))
    assert set(rat) == {"out"} | set(lr.PC_GRADS)
    report(dtype, id, rat)
