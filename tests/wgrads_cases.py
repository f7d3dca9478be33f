"""Deferred weight gradients on the CPU: the cases of pointnet2/wgrads.py's placement rules (one per rule), what each
case's gradients are (restated from the operands, independently of the placement), and a stand-in for the grouped launch.
Shared by tests/test_host_logic.py (place() alone) and tests/test_wgrads_host.py (the same cases through deferred_wgrads)."""
import ctypes

import torch

P = 37                      # rows of every operand
NAMES = ("a_whole", "b_ranges_cover", "c_one_range", "d_range_twice", "e_joint", "e2_joint_part_seen", "f_columns", "g_rot",
         "h1_bias_whole", "h1_bias_whole_padded", "h2_bias_ranges", "h3_bias_joint_padded")         # of cases()


def _param(*shape):
    return torch.nn.Parameter(torch.zeros(*shape))


def _operands(M, N, gen):
    """positive values: no sum cancels, so a relative bound holds element by element"""
    return [(torch.rand(P, n, generator=gen) + 0.5).to(torch.bfloat16) for n in (M, N)]


class Case:
    """items: [wgrads.Item] of ONE grouped launch; sa: collected by add_sa (else add); params: every parameter involved"""

    def __init__(self, sa=False):
        self.items, self.params, self.sa = [], [], sa
        self.gen = torch.Generator().manual_seed(11)

    def own(self, *params):
        self.params.extend(params)
        return params if len(params) > 1 else params[0]

    def add(self, M, N, w, crop, b=None):
        """w, b: the tensors a layer would hold (a Parameter, a row range of one, a cat_params), or a Target"""
        import wgrads
        wt, bt = [t if (t is None or isinstance(t, wgrads.Target)) else wgrads.grad_target(t) for t in (w, b)]
        assert wt is not None and (b is None or bt is not None)
        dY, X = _operands(M, N, self.gen)
        self.items.append(wgrads.Item(dY, X, M, N, P, wt, crop, bt))
        return self


def cases():
    """{name: Case}; the names follow the list of rules (a .. h) in the docstring of test_place_rules"""
    import wgrads
    from wgrads import Crop, cat_params
    out = {}
    c = out["a_whole"] = Case()
    c.add(16, 8, c.own(_param(16, 8)), Crop(16, 8))
    c = out["b_ranges_cover"] = Case()
    w = c.own(_param(24, 8))
    c.add(8, 8, w[0:8], Crop(8, 8)).add(16, 8, w[8:24], Crop(16, 8))
    c = out["c_one_range"] = Case()
    c.add(8, 8, c.own(_param(24, 8))[0:8], Crop(8, 8))
    c = out["d_range_twice"] = Case()
    w = c.own(_param(24, 8))
    c.add(16, 8, w[8:24], Crop(16, 8)).add(16, 8, w[8:24], Crop(16, 8))
    # a joint weight of 4 + 8 + 5 rows under a GEMM padded to 32: a whole unseen parameter, rows 8:16 of a packed one, and (e2)
    # a whole parameter that the same launch has also met on its own
    for name in ("e_joint", "e2_joint_part_seen"):
        c = out[name] = Case()
        a, packed, b = c.own(_param(4, 8), _param(24, 8), _param(5, 8))
        if name == "e2_joint_part_seen":
            c.add(5, 8, b, Crop(5, 8))
        c.add(32, 8, cat_params([a, packed[8:16], b]), Crop(17, 8))
    c = out["f_columns"] = Case(sa=True)
    w = c.own(_param(16, 7))
    c.add(16, 8, w, Crop(16, 4, col0=3, ld=7)).add(16, 8, w, Crop(16, 3, col0=0, ld=7))
    c = out["g_rot"] = Case(sa=True)
    c.add(16, 16, c.own(_param(16, 11)), Crop(16, 11, rot=3 | 8 << 8))
    c = out["h1_bias_whole"] = Case()
    c.add(16, 8, c.own(_param(16, 8)), Crop(16, 8), c.own(_param(16)))
    c = out["h1_bias_whole_padded"] = Case()
    c.add(32, 8, c.own(_param(20, 8)), Crop(20, 8), c.own(_param(20)))
    c = out["h2_bias_ranges"] = Case()
    w, b = c.own(_param(24, 8), _param(24))
    c.add(8, 8, w[0:8], Crop(8, 8), b[0:8]).add(16, 8, w[8:24], Crop(16, 8), b[8:24])
    c = out["h3_bias_joint_padded"] = Case()
    ws, bs = c.own(_param(4, 8), _param(8, 8), _param(5, 8)), c.own(_param(4), _param(8), _param(5))
    c.add(32, 8, cat_params(ws), Crop(17, 8), cat_params(bs, pad_to=32))
    assert tuple(out) == NAMES and all(isinstance(it.wt, wgrads.Target) for c in out.values() for it in c.items)
    return out


def collected(items, ones=False):
    """{id(param): (param, f64 flat gradient)}: what the items' gradients are and which elements of which parameter they belong
    to, from the operands and the records alone -- out = crop(dY^T X) with the `rot` column map of include/omnipq_sa.h, bias =
    column sums of dY.  ones: every collected value is 1 (how often each element was collected)."""
    got = {}

    def into(param, idx, values):
        flat = got.setdefault(id(param), (param, torch.zeros(param.numel(), dtype=torch.float64)))[1]
        flat.index_add_(0, idx.reshape(-1), values.reshape(-1))

    for it in items:
        rows, cols, rot, col0, ld = it.crop
        full = torch.ones(it.M, it.N, dtype=torch.float64) if ones else it.dY.double().T @ it.X.double()
        src = [(rot >> 8) + c if c < (rot & 255) else c - (rot & 255) for c in range(cols)]
        G = full[:rows, src]
        sums = torch.ones(it.M, dtype=torch.float64) if ones else it.dY.double().sum(0)
        r, c = torch.meshgrid(torch.arange(rows), torch.arange(cols), indexing="ij")
        if it.wt.single:
            into(it.wt.param, it.wt.off + r * (cols if ld is None else ld) + col0 + c, G)
        else:
            for param, off, r0, r1 in it.wt.parts:
                into(param, off + torch.arange((r1 - r0) * cols), G[r0:r1])
        if it.bt is not None and it.bt.single:
            into(it.bt.param, it.bt.off + torch.arange(rows), sums[:rows])
        elif it.bt is not None:
            for param, off, r0, r1 in it.bt.parts:
                into(param, off + torch.arange(r1 - r0), sums[r0:r1])
    return got


def _host(addr, n, dtype):
    """n elements of host memory at `addr`, as a tensor that shares it"""
    size = torch.empty((), dtype=dtype).element_size()
    return torch.frombuffer((ctypes.c_char * (n * size)).from_address(addr), dtype=dtype)


def grouped_tn_on_host(fn, anchor, *args):
    """In place of sa_fused._call: omnipq_gemm_tn_grouped as include/omnipq_sa.h states it, on host memory, read through the
    problems' pointers; float64 arithmetic, float32 stores.  Any other entry point is an error."""
    assert fn.__name__ == "omnipq_gemm_tn_grouped", fn.__name__
    n, probs, _ = args
    for q in probs._obj[:n]:
        assert not q.ba and not q.bb and not q.rows_dev, "no affine operand, no row plan on the CPU"
        A = _host(q.A, q.P * q.lda, torch.bfloat16).view(q.P, q.lda)[:, :q.M].double()
        B = _host(q.B, q.P * q.ldb, torch.bfloat16).view(q.P, q.ldb)[:, :q.N].double()
        C = A.T @ B
        rot, split = q.rot & 255, q.rot >> 8
        src = [split + c if c < rot else c - rot for c in range(q.out_cols)]
        out = _host(q.out, (q.out_rows - 1) * q.out_ld + q.out_cols, torch.float32)
        for r in range(q.out_rows):
            row = out[r * q.out_ld:r * q.out_ld + q.out_cols]
            row.copy_(((row.double() if q.flags & 1 else 0) + C[r, src]).float())
        if q.colsum:
            sums = _host(q.colsum, q.M, torch.float32)
            sums.copy_((sums.double() + A.sum(0)).float())
