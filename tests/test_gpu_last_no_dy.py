"""GPU: the backward of a planned SA stage's LAST layer without its output gradient (sa_fused.LAST_NO_DY; csrc/sa_last_bwd.hip,
gemm_bf16.hip: DzGen, gemm_tn_bf16.hip: gemm_tn_dz_kernel), entry point by entry point, against a float64
reference of one synthetic last layer -- conv C2 -> C3 on the layer below's X2 = relu(a2 Y2 + b2), BatchNorm over all P
positions of the FULL layout, ReLU, max-pool over each ball -- differentiated by autograd and folded back onto the compact rows
of the stage's row plan.  The stored-dY3 route (omnipq_sa_pool_bwd_apply_gb, omnipq_gemm_nt_e16_bnbwd, omnipq_gemm_tn_e16_affine)
runs on the same inputs as the yardstick: the route without dY3 must be as close to float64 as the stored one, up to a factor
of two and a floor of one e16 rounding (2^-9 bf16, 2^-12 f16), and under an absolute ceiling per gradient.

The reference takes two DECISIONS from the kernels -- the pooled row of every (ball, column) (`arg`) and the pooled ReLU's mask
(`out_pm > 0`) -- and checks each against float64 within a stated tolerance, so that near-ties cannot make the comparison flaky.
Every index a kernel reads comes from omnipq_sa_ball_plan_src over in-range ball indices."""
import ctypes

import pytest
import torch

import capi
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS, MOMENTUM = 1e-5, 0.1
FLOOR = {torch.bfloat16: 2.0 ** -9, torch.float16: 2.0 ** -12}
G_SCALE = {torch.bfloat16: 1.0, torch.float16: 1024.0}      # f16: upstream gradients scaled as torch.amp.GradScaler would
P_ = capi.P
LL, DBL, FLT = ctypes.c_longlong, ctypes.c_double, ctypes.c_float
NULL = ctypes.c_void_p(0)


def _sa():
    import sa_fused
    return sa_fused


def rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm()) / (float(b.norm()) + 1e-30)


def ok(dt, name, *args, plan=None):
    """the entry point `name` of the library of element type dt (sa_fused._ext: E16.select) on the current stream"""
    sa = _sa()
    sa.E16.select(dt)
    if name in sa.PLAN_AWARE:
        args = args + (plan,)
    rc = getattr(sa._lib, name)(*args, sa._ext._stream())
    assert rc == 0, f"{name} -> {rc}"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.uint8)


def _ball_idx(fill, B, M, S, seed):
    """(B, M, S) int32 ball indices as omnipq_ball_query leaves them: a ball's real neighbours first, the rest copies of its
    first one.  fill: 'room' (ball query around furthest-point centres of a synthetic room scene), 'full' (every ball full),
    'single' (one neighbour per ball), 'edges' (counts cycling over the group boundaries 1, 8, 9, 16, 17, S - 1, S)."""
    if fill == "room":
        xyz = synth.make_clouds(seed, B, 40000, kind="room")[..., :3].contiguous().to(DEV)
        cen, _ = capi.fps(xyz, M)
        new_xyz = torch.gather(xyz, 1, cen.long().unsqueeze(-1).expand(B, M, 3)).contiguous()
        idx = capi.ball_query(new_xyz, xyz, 0.2 if S >= 64 else 0.4, S)
        assert int(idx.min()) >= 0 and int(idx.max()) < 40000
        return idx
    if fill == "full":
        cnt = torch.full((B, M), S, dtype=torch.long)
    elif fill == "single":
        cnt = torch.ones((B, M), dtype=torch.long)
    else:
        cycle = torch.tensor([1, 8, 9, 16, 17, S - 1, S])
        cnt = cycle[torch.arange(B * M) % len(cycle)].view(B, M)
    real = (torch.arange(B * M * S) % 60000).view(B, M, S).to(torch.int32)     # distinct within a ball
    idx = torch.where(torch.arange(S).view(1, 1, S) < cnt.unsqueeze(-1), real, real[..., :1])
    return idx.to(torch.int32).contiguous().to(DEV)


def _plan_maps(plan, idx, B, M, S, P):
    """-> (rows in use, comp: full position -> compact row (a dropped position maps to its ball's first row), row weights)"""
    BM = B * M
    rows = int(plan.rows_dev.item())
    assert 0 < rows <= P and rows % plan.gs == 0
    r = torch.arange(rows, device=DEV)
    pos = plan.unit_src[: rows // 8].long()[r // 8] * 8 + r % 8        # full-layout position of every compact row
    assert int(pos.min()) >= 0 and int(pos.max()) < P and torch.unique(pos).numel() == rows
    comp = torch.full((P,), -1, dtype=torch.long, device=DEV)
    comp[pos] = r
    comp = comp.view(BM, S)
    assert bool((comp[:, 0] >= 0).all())                             # every ball keeps its first row
    dropped = comp < 0
    flat = idx.view(BM, S)
    assert torch.equal(flat[dropped], flat[:, :1].expand(BM, S)[dropped])   # what the plan drops are copies of row 0
    comp = torch.where(dropped, comp[:, :1].expand(BM, S), comp).reshape(P)
    w = plan.row_w[:rows].long()
    assert torch.equal(torch.bincount(comp, minlength=rows), w)        # a row stands for exactly row_w positions ...
    per_ball = torch.zeros(BM, dtype=torch.long, device=DEV).index_add_(0, pos // S, w)
    assert torch.equal(per_ball, torch.full((BM,), S, dtype=torch.long, device=DEV))   # ... and row_w sums to S per ball
    return rows, comp, w


def _plan_arg(plan, rows, pool_gamma=None):
    st = _sa().RowPlanArg(P_(plan.rows_dev).value, P_(plan.row_w).value, P_(plan.goff).value, rows, plan.gs,
                          P_(pool_gamma).value if pool_gamma is not None else None)
    return st, ctypes.pointer(st)


class Layer:
    """Inputs of one synthetic last layer."""


def _inputs(dt, C2, C3, B, M, S, gs, fill, seed, monkeypatch):
    sa = _sa()
    monkeypatch.setattr(sa, "PLAN_GROUP", gs)
    L = Layer()
    L.dt, L.C2, L.C3, L.B, L.M, L.S, L.BM, L.P = dt, C2, C3, B, M, S, B * M, B * M * S
    P = L.P
    gen = torch.Generator().manual_seed(seed)
    L.idx = _ball_idx(fill, B, M, S, seed)
    sa.E16.select(dt)
    L.plan = sa.make_row_plan(L.idx, P)
    L.rows, L.comp, L.w = _plan_maps(L.plan, L.idx, B, M, S, P)
    # the layer below: pre-BN output Y2 on the compact rows (rows past the ones in use: filler the kernels never read), its
    # BatchNorm totals over the FULL layout (row weights); gamma2 negative on a third of the columns, zero on two
    L.Y2 = (torch.randn((P, C2), generator=gen) * 1.5 + 0.3).to(dt).to(DEV)
    y2 = L.Y2[: L.rows].double()
    wd = L.w.double().unsqueeze(1)
    L.fin2 = torch.stack([(wd * y2).sum(0), (wd * y2 * y2).sum(0)]).contiguous()
    gamma2 = (0.5 + torch.rand(C2, generator=gen)) * torch.where(torch.arange(C2) % 3 == 1, -1.0, 1.0)
    gamma2[[5, 77]] = 0.0
    L.gamma2, L.beta2 = gamma2.to(DEV), (0.4 * torch.randn(C2, generator=gen)).to(DEV)
    # the last layer: its weight prepared as the stage prepares it; gamma3 negative on every third column (the pool selects
    # the ball's MINIMUM there), zero on two, and three columns whose pooled output is clamped to 0 in every ball
    W3 = torch.randn((C3, C2), generator=gen) / C2 ** 0.5
    L.Wp, L.Wt = sa.prep_weight(W3.to(DEV), C3, C2, transpose=True)
    gamma3 = (0.5 + torch.rand(C3, generator=gen)) * torch.where(torch.arange(C3) % 3 == 2, -1.0, 1.0)
    beta3 = 0.3 * torch.randn(C3, generator=gen)
    gamma3[[3, 40]] = 0.0
    gamma3[[7, 50, 101]], beta3[[7, 50, 101]] = 0.25, -30.0
    L.gamma3, L.beta3 = gamma3.to(DEV), beta3.to(DEV)
    g = torch.randn((L.BM, C3), generator=gen)
    g[torch.rand((L.BM, C3), generator=gen) < 0.1] = 0.0               # exact zeros in the upstream gradient
    L.g = (g * G_SCALE[dt]).to(DEV).contiguous()
    return L


def _forward(L, store):
    """omnipq_gemm_nt_e16_bnaffine_pool (C = NULL, or the stored Y3) + omnipq_sa_pool_select_finalize -> what they wrote"""
    dt, P, BM, C2, C3 = L.dt, L.P, L.BM, L.C2, L.C3
    sa = _sa()
    one_sided = L.plan.gs == 8 and sa.ONE_SIDED_EXTREMA
    st, pa = _plan_arg(L.plan, P, L.gamma3 if one_sided else None)
    o = {"abmi2": torch.full((4, C2), float("nan"), device=DEV), "sums3": torch.zeros((2, C3), device=DEV, dtype=torch.float64)}
    ws = torch.empty((int(sa._lib.omnipq_gemm_nt_stats_workspace_floats(P, C3)),), device=DEV)
    slots = P // L.plan.gs
    o["ext16"] = torch.zeros((2, slots, C3), device=DEV, dtype=dt)
    o["ext8"] = torch.zeros((2, slots, C3), device=DEV, dtype=torch.uint8)
    o["Y3"] = torch.empty((P, C3), device=DEV, dtype=dt) if store else None
    a2 = o["abmi2"]
    ok(dt, "omnipq_gemm_nt_e16_bnaffine_pool", P, C3, C2, P_(L.Y2), C2, P_(L.fin2), DBL(float(P)), P_(L.gamma2), P_(L.beta2),
       FLT(EPS), FLT(MOMENTUM), NULL, NULL, NULL, P_(a2[0]), P_(a2[1]), P_(a2[2]), P_(a2[3]), P_(L.Wp), C2, P_(o["Y3"]), C3,
       NULL, P_(o["sums3"]), P_(ws), L.plan.gs, P_(o["ext16"][0]), P_(o["ext16"][1]), P_(o["ext8"][0]), P_(o["ext8"][1]),
       plan=pa)
    o["abmi3"] = torch.full((4, C3), float("nan"), device=DEV)
    o["out"] = torch.empty((BM, C3), device=DEV)
    o["out_pm"] = torch.empty((BM, C3), device=DEV, dtype=dt)
    o["arg"] = torch.empty((BM, C3), device=DEV, dtype=torch.uint8)
    o["ysel"] = torch.empty((BM, C3), device=DEV, dtype=dt)
    a3 = o["abmi3"]
    ok(dt, "omnipq_sa_pool_select_finalize", LL(BM), C3, P_(o["ext16"][0]), P_(o["ext16"][1]), P_(o["ext8"][0]),
       P_(o["ext8"][1]), P_(o["sums3"]), DBL(float(P)), P_(L.gamma3), P_(L.beta3), FLT(EPS), FLT(MOMENTUM), NULL, NULL,
       P_(a3[0]), P_(a3[1]), P_(a3[2]), P_(a3[3]), P_(o["out"]), P_(o["out_pm"]), P_(o["arg"]), P_(o["ysel"]), plan=pa)
    return o


def _reference(L, fw):
    """float64 over the full layout, with the kernels' layer-below constants and their pooling decisions -> dict"""
    BM, S, C3 = L.BM, L.S, L.C3
    ref = {}
    a2, b2, mean2, invstd2 = (v.double() for v in fw["abmi2"])
    y2 = L.Y2[: L.rows].double()
    X2c = torch.relu(a2 * y2 + b2).requires_grad_(True)
    W3 = L.Wp.double().requires_grad_(True)                     # the e16 weight the kernels were given
    gamma3 = L.gamma3.double().requires_grad_(True)
    beta3 = L.beta3.double().requires_grad_(True)
    Y3 = X2c[L.comp] @ W3.t()                                   # the full layout: a dropped position repeats its ball's row 0
    mean3 = Y3.mean(0)
    invstd3 = torch.rsqrt(Y3.var(0, unbiased=False) + EPS)
    pre = gamma3 * (Y3 - mean3) * invstd3 + beta3
    ref["sums3"] = torch.stack([Y3.sum(0), (Y3 * Y3).sum(0)]).detach()
    ref["abmi3"] = torch.stack([gamma3 * invstd3, beta3 - mean3 * gamma3 * invstd3, mean3, invstd3]).detach()
    pre_b = pre.view(BM, S, C3)
    picked = torch.gather(pre_b, 1, fw["arg"].long().unsqueeze(1)).squeeze(1)
    # the decisions taken from the kernels, each checked against float64: arg selects the ball's maximum of a3 y3 + b3 (the
    # maximum of y3 where a3 >= 0, its minimum where a3 < 0), the mask is the sign of the pooled value, both up to the e16
    # rounding of Y3 the kernels decided on (tol: 2^-6 of |a3| (|y3| + |mean3|))
    with torch.no_grad():
        tol = 2.0 ** -6 * (gamma3.abs() * invstd3 * (Y3.abs().view(BM, S, C3).max(1).values + mean3.abs())) + 1e-9
        gap = pre_b.max(1).values - picked
        live = fw["out"] > 0                                    # a clamped result (pooled 0) routes nothing: arg is 0 there
        ref["arg_gap"] = float((gap / tol)[live].max())
        ref["arg_zero"] = bool((fw["arg"][~live] == 0).all())
        mask = fw["out_pm"].double() > 0
        ref["mask_bad"] = int(((mask != (picked > 0)) & (picked.abs() > tol)).sum())
        ref["pooled"] = torch.relu(picked)
    (picked * mask * L.g.double()).sum().backward()
    ref["dX2"] = X2c.grad                                       # folded onto the compact rows by the index's backward
    ref["dW3"], ref["dgamma3"], ref["dbeta3"] = W3.grad, gamma3.grad, beta3.grad
    dz2 = ref["dX2"] * (a2 * y2 + b2 > 0)
    ref["sums2"] = torch.stack([dz2.sum(0), (dz2 * (y2 - mean2) * invstd2).sum(0)])
    mu2 = L.fin2[0] / L.P
    is2 = torch.rsqrt((L.fin2[1] / L.P - mu2 * mu2).clamp_min(0) + EPS)
    g2 = L.gamma2.double()
    ref["abmi2"] = torch.stack([g2 * is2, L.beta2.double() - mu2 * g2 * is2, mu2, is2])
    return ref


def _no_dy_route(L, fw):
    dt, P, BM, S, C2, C3 = L.dt, L.P, L.BM, L.S, L.C2, L.C3
    sa = _sa()
    st, pa = _plan_arg(L.plan, P)
    a3, mean3, invstd3 = fw["abmi3"][0], fw["abmi3"][2], fw["abmi3"][3]
    a2, b2, mean2, invstd2 = fw["abmi2"]
    r = {"sums": torch.zeros((3, C3), device=DEV, dtype=torch.float64), "hot": torch.zeros((BM, C3), device=DEV, dtype=torch.int32)}
    ok(dt, "omnipq_sa_pool_bwd_stats_sel_hot", LL(BM), C3, P_(fw["ysel"]), P_(mean3), P_(invstd3), P_(L.g), P_(fw["out_pm"]),
       P_(r["sums"]), 1, P_(a3), P_(fw["arg"]), P_(r["hot"]))
    outs = {}
    for form in ("hot", "nohot"):
        hot2 = torch.zeros((BM, C3), device=DEV, dtype=torch.int32) if form == "hot" else None
        B1 = torch.full((C2, C2 + 32), float("nan"), device=DEV, dtype=dt)
        ab = torch.full((2, C3), float("nan"), device=DEV)
        gb = torch.full((2, C3), float("nan"), device=DEV)
        on = hot2 is not None
        ok(dt, "omnipq_sa_last_bwd_prep", LL(BM), C3, C2, P_(r["sums"]), DBL(float(P)), P_(a3), P_(mean3), P_(invstd3),
           P_(L.g if on else None), P_(fw["out_pm"] if on else None), P_(fw["arg"] if on else None), P_(L.Wt),
           L.Wt.stride(0), P_(hot2), P_(B1), C2 + 32, P_(ab[0]), P_(ab[1]), P_(gb))
        outs[form] = (hot2, B1, ab, gb)
    r["hot_prep"] = outs["hot"][0]
    r["B1"], r["ab"], r["gb"] = outs["nohot"][1:]
    r["prep_forms_equal"] = all(torch.equal(_bits(x), _bits(y)) for x, y in zip(outs["hot"][1:], outs["nohot"][1:]))
    r["dX2"] = torch.empty((P, C2), device=DEV, dtype=dt)
    r["X2"] = torch.empty((P, C2), device=DEV, dtype=dt)
    r["sums2"] = torch.zeros((3, C2), device=DEV, dtype=torch.float64)
    ws = torch.empty((int(sa._lib.omnipq_gemm_nt_stats_workspace_floats(P, C2)),), device=DEV)
    ok(dt, "omnipq_gemm_nt_e16_dz_bnbwd", P, C2, C3, P_(L.Y2), C2, P_(r["B1"]), C2 + 32, P_(L.Wt), L.Wt.stride(0), P_(r["hot"]),
       P_(L.plan.unit_src), S, P_(r["dX2"]), C2, P_(a2), P_(b2), P_(mean2), P_(invstd2), P_(r["sums2"]), P_(ws), P_(r["X2"]),
       plan=pa)
    for form, src, ba, bb in (("x2", r["X2"], None, None), ("y2", L.Y2, a2, b2)):
        wsz = torch.empty((int(sa._lib.omnipq_gemm_tn_dz_workspace_floats(C3, C2, P)),), device=DEV)
        slabs, cs_off = ctypes.c_int(0), ctypes.c_longlong(0)
        ok(dt, "omnipq_gemm_tn_dz", C3, C2, P, P_(src), C2, P_(ba), P_(bb), P_(r["hot"]), P_(L.plan.unit_src), S, P_(wsz),
           ctypes.byref(slabs), ctypes.byref(cs_off), plan=pa)
        assert slabs.value >= 1
        out = torch.full((C3, C2), float("nan"), device=DEV)
        cs = ctypes.c_void_p(wsz.data_ptr() + 4 * cs_off.value)
        for acc in (0, 1):
            ok(dt, "omnipq_sa_last_wgrad_combine", C3, C2, P_(wsz), cs, slabs.value, C3 + C2, P_(r["ab"][0]), P_(r["ab"][1]),
               P_(L.Wp), L.Wp.stride(0), P_(out), C2, acc)
            if acc == 0:
                r["dW3_" + form] = out.clone()
        r["dW3_acc_" + form] = out
    return r


def _stored_route(L, fw):
    dt, P, BM, S, C2, C3 = L.dt, L.P, L.BM, L.S, L.C2, L.C3
    sa = _sa()
    st, pa = _plan_arg(L.plan, P)
    a3, mean3, invstd3 = fw["abmi3"][0], fw["abmi3"][2], fw["abmi3"][3]
    a2, b2, mean2, invstd2 = fw["abmi2"]
    r = {}
    sums = torch.zeros((3, C3), device=DEV, dtype=torch.float64)
    ok(dt, "omnipq_sa_pool_bwd_stats_sel", LL(BM), C3, P_(fw["ysel"]), P_(mean3), P_(invstd3), P_(L.g), P_(fw["out_pm"]),
       P_(sums), 1)
    dY = torch.empty((P, C3), device=DEV, dtype=dt)
    r["gb"] = torch.empty((2, C3), device=DEV)
    ok(dt, "omnipq_sa_pool_bwd_apply_gb", L.B, L.M, S, C3, DBL(float(P)), P_(fw["Y3"]), P_(a3), P_(mean3), P_(invstd3), P_(sums),
       P_(L.g), P_(fw["out_pm"]), P_(fw["arg"]), P_(dY), P_(r["gb"]), plan=pa)
    r["dX2"] = torch.empty((P, C2), device=DEV, dtype=dt)
    r["sums2"] = torch.zeros((3, C2), device=DEV, dtype=torch.float64)
    ws = torch.empty((int(sa._lib.omnipq_gemm_nt_stats_workspace_floats(P, C2)),), device=DEV)
    ok(dt, "omnipq_gemm_nt_e16_bnbwd", P, C2, C3, P_(dY), C3, P_(L.Wt), C3, P_(r["dX2"]), C2, P_(L.Y2), P_(a2), P_(b2),
       P_(mean2), P_(invstd2), P_(r["sums2"]), P_(ws), plan=pa)
    r["dW3"] = torch.empty((C3, C2), device=DEV)
    wst = torch.empty((int(sa._lib.omnipq_gemm_tn_workspace_floats(C3, C2, P)),), device=DEV)
    ok(dt, "omnipq_gemm_tn_e16_affine", C3, C2, P, P_(dY), C3, P_(L.Y2), C2, P_(a2), P_(b2), P_(r["dW3"]), P_(wst), NULL,
       plan=pa)
    return r


BF, HF = torch.bfloat16, torch.float16
# (name, element type, C2, C3, B, M, S, plan group, ball fill); every P = B M S a multiple of 128 with more than 64 row tiles
CASES = [
    ("sa1_room_g8", BF, 128, 256, 2, 2048, 64, 8, "room"),              # the benchmark's sa1 per 2 scenes
    ("sa1_room_g16", BF, 128, 256, 2, 2048, 64, 16, "room"),
    ("min_tiles_full_c128", BF, 128, 128, 2, 65, 64, 8, "full"),        # ceil(P / 128) = 65, every ball full: rows == P
    ("single_g8", BF, 128, 256, 2, 256, 64, 8, "single"),               # row_w up to S - 7, most TN slabs empty
    ("single_g16_s128", BF, 128, 128, 1, 128, 128, 16, "single"),       # row_w up to S - 15
    ("edges_s32_g8", BF, 128, 128, 2, 160, 32, 8, "edges"),             # rows in use not a multiple of 128
    ("edges_s128_g16", BF, 128, 256, 1, 131, 128, 16, "edges"),
    ("sa2_widths_edges", BF, 256, 512, 2, 512, 32, 8, "edges"),         # sa2 under LAST_NO_DY_MAX_C3 = 1 << 30
    ("f16_sa1_room_g8", HF, 128, 256, 2, 2048, 64, 8, "room"),
    ("f16_edges_s64_g16", HF, 128, 128, 2, 160, 64, 16, "edges"),
]

# ceilings on the rel-L2 against float64 of the route without dY3: about twice the worst measured over CASES
# (bf16: dX2 2.4e-3, sums2 4.4e-3, dW3 3.3e-3, dgamma3 2.3e-3, dbeta3 8.4e-8; f16: 3.0e-4, 5.4e-4, 3.8e-4, 3.2e-4, 7.5e-8)
CEIL = {BF: dict(dX2=5e-3, sums2=9e-3, dW3=6.5e-3, dgamma3=4.5e-3, dbeta3=2e-7),
        HF: dict(dX2=6e-4, sums2=1.1e-3, dW3=8e-4, dgamma3=6.5e-4, dbeta3=2e-7)}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_last_layer_without_dy_matches_float64_entry_point_by_entry_point(case, monkeypatch):
    name, dt, C2, C3, B, M, S, gs, fill = case
    L = _inputs(dt, C2, C3, B, M, S, gs, fill, 11 + len(name), monkeypatch)
    P = L.P
    assert (P + 127) // 128 > 64 and P % 128 == 0
    if fill == "full":
        assert L.rows == P and bool((L.w == 1).all())
    if fill == "single":
        assert int(L.w.max()) == S - gs + 1
    if fill == "edges":
        assert L.rows % 128 != 0
    # ---- forward: the no-store GEMM is the storing GEMM without the store
    fw, fs = _forward(L, store=False), _forward(L, store=True)
    for k in ("abmi2", "sums3", "ext16", "ext8", "abmi3", "out", "out_pm", "arg", "ysel"):
        assert torch.equal(_bits(fw[k]), _bits(fs[k])), k
    ref = _reference(L, fw)
    assert rel_l2(fw["abmi2"], ref["abmi2"]) < 1e-5
    assert rel_l2(fw["sums3"][0], ref["sums3"][0]) < 1e-3 and rel_l2(fw["sums3"][1], ref["sums3"][1]) < 1e-3
    for i, k in enumerate(("a3", "b3", "mean3", "invstd3")):
        assert rel_l2(fw["abmi3"][i], ref["abmi3"][i]) < 5e-3, k
    assert ref["arg_gap"] <= 1.0 and ref["arg_zero"], ref["arg_gap"]  # arg: an extremum of its ball
    assert ref["mask_bad"] == 0
    assert rel_l2(fw["out"], ref["pooled"]) < 8 * FLOOR[dt]
    # ---- the route without dY3
    nd = _no_dy_route(L, fw)
    hot = nd["hot"]
    assert torch.equal(hot, nd["hot_prep"]), "omnipq_sa_pool_bwd_stats_sel_hot and omnipq_sa_last_bwd_prep wrote different words"
    assert torch.equal(hot & 0xFF, fw["arg"].int())
    a3 = fw["abmi3"][0]
    want_val = (a3.unsqueeze(0) * torch.where(fw["out_pm"].float() > 0, L.g, torch.zeros_like(L.g))).to(dt)
    assert torch.equal((hot >> 16) & 0xFFFF, _bits(want_val).int() & 0xFFFF), "hot values: e16(a3 g [pooled > 0])"
    assert nd["prep_forms_equal"], "prep with and without hot: B1 / alpha / beta / gb differ"
    assert rel_l2(nd["sums"][0], ref["dbeta3"]) < 1e-6
    m1, m2 = nd["sums"][0] / P, nd["sums"][1] / P
    a3d, mean3d, invstd3d = (fw["abmi3"][i].double() for i in (0, 2, 3))
    alpha, beta = a3d * (m1 - mean3d * invstd3d * m2), a3d * invstd3d * m2
    assert rel_l2(nd["ab"][0], alpha) < 1e-5 and rel_l2(nd["ab"][1], beta) < 1e-5
    W3 = L.Wp.double()
    G, v = W3.t() @ (beta.unsqueeze(1) * W3), W3.t() @ alpha
    B1 = nd["B1"].double()
    e_G = rel_l2(-B1[:, :C2], G)
    assert e_G < 2 * FLOOR[dt], e_G                                  # one e16 rounding per element
    v_got = -(B1[:, C2] + B1[:, C2 + 1])
    scale = alpha.abs() @ W3.abs()
    e_v = float(((v_got - v).abs() / (2.0 ** -14 * v.abs() + 2.0 ** -16 * scale + 1e-30)).max())
    assert e_v <= 1.0, e_v                                            # v_hi + v_lo: about 16 bits
    assert bool((B1[:, C2 + 2:] == 0).all())
    # dz_bnbwd: X2 exactly the forward's operand; the data gradient and the layer below's BatchNorm-backward sums
    rows = L.rows
    y2 = L.Y2[:rows].double()
    a2d, b2d, mean2d, invstd2d = (fw["abmi2"][i].double() for i in range(4))
    x2_want = torch.relu(a2d * y2 + b2d).float().to(dt)
    assert torch.equal(nd["X2"][:rows].float(), x2_want.float()), "X2out"
    # the epilogue sums the ROUNDED dX2 (its C tile is staged in e16): equal to the sums of the stored dX2 up to f32 order
    dz_k = nd["dX2"][:rows].double() * (a2d * y2 + b2d > 0)
    own = torch.stack([dz_k.sum(0), (dz_k * (y2 - mean2d) * invstd2d).sum(0)])
    assert rel_l2(nd["sums2"][:2], own) < 1e-5, rel_l2(nd["sums2"][:2], own)
    assert torch.equal(nd["dW3_acc_x2"], 2 * nd["dW3_x2"]) and torch.equal(nd["dW3_acc_y2"], 2 * nd["dW3_y2"])
    st = _stored_route(L, fs)                                         # (the storing forward: Y3)
    assert rel_l2(st["gb"], nd["gb"]) < 1e-6
    errs = {
        "dX2": (rel_l2(nd["dX2"][:rows], ref["dX2"]), rel_l2(st["dX2"][:rows], ref["dX2"])),
        "sums2": (rel_l2(nd["sums2"][:2], ref["sums2"]), rel_l2(st["sums2"][:2], ref["sums2"])),
        "dW3": (rel_l2(nd["dW3_x2"], ref["dW3"]), rel_l2(st["dW3"], ref["dW3"])),
        "dW3_y2": (rel_l2(nd["dW3_y2"], ref["dW3"]), rel_l2(st["dW3"], ref["dW3"])),
        "dgamma3": (rel_l2(nd["gb"][1], ref["dgamma3"]), rel_l2(st["gb"][1], ref["dgamma3"])),
        "dbeta3": (rel_l2(nd["gb"][0], ref["dbeta3"]), rel_l2(st["gb"][0], ref["dbeta3"])),
    }
    print(f"\n{name}: rows {rows} of {P} ({rows / P:.3f}), max row_w {int(L.w.max())}; B1 vs -G {e_G:.2e}, v {e_v:.2f}")
    for k, (e_new, e_old) in errs.items():
        print(f"  {k:8s} rel-L2 vs f64: without dY3 {e_new:.2e}   stored dY3 {e_old:.2e}")
    assert rel_l2(nd["dW3_y2"], nd["dW3_x2"]) < 8 * FLOOR[dt]
    for k, (e_new, e_old) in errs.items():
        assert e_new <= 2.0 * e_old + FLOOR[dt], (k, e_new, e_old)
        assert e_new <= CEIL[dt][k.replace("_y2", "")], (k, e_new)


def test_the_benchmarked_step_takes_the_route_on_sa1_and_not_on_sa2(monkeypatch):
    """bench.build_model(0), training mode, bf16 autocast, the benchmark's shapes (8 scenes x 40 000 points), backward inside
    deferred_wgrads as the benchmarked step runs it: the last layer of sa1 (128 -> 256) takes the route without dY3 exactly once
    per step, sa2 (256 -> 512, above LAST_NO_DY_MAX_C3) keeps the stored dY3 -- a silent fallback fails here."""
    import bench
    sa = _sa()
    seen = []
    real = sa.last_no_dy_ok

    def spy(plan, L, P, c2, c3, S, below):
        r = real(plan, L, P, c2, c3, S, below)
        seen.append((c3, P, r))
        return r

    monkeypatch.setattr(sa, "last_no_dy_ok", spy)
    torch.manual_seed(1)
    net = bench.build_model(0).to(DEV).train()
    pc = synth.make_clouds(2, 8, 40000, kind="room").to(DEV)
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        seen.clear()
        uses = sa.last_no_dy_uses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = bench.loss_of(net({"point_clouds": pc}))
        assert sa.last_no_dy_uses == uses + 1
        assert [(c3, P) for c3, P, r in seen if r] == [(256, 8 * 2048 * 64)]          # sa1
        assert not any(r for c3, P, r in seen if c3 > 256)                             # sa2 (and nothing wider) stays off
        with sa.deferred_wgrads() as dfr:
            loss.backward()
            assert len(dfr.dz_items) == 1
        torch.cuda.synchronize()
        w = net.backbone.sa1.mlp_module.layer2.conv.weight.grad
        assert w is not None and bool(torch.isfinite(w).all()) and float(w.abs().max()) > 0
