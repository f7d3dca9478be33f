"""GPU: the fused bf16 set-abstraction stage (sa_fused.py + csrc/sa_stage.hip, gemm_*.hip) against
f32 PyTorch references of the same operators.

Tolerances here are bf16 tolerances and say so: operands and stored activations have an 8-bit
mantissa (relative step 2^-8 = 3.9e-3), accumulation is f32.  The 1e-4 parity bar of the
north star applies to the f32 mode (test_gpu_parity.py); this file checks that the bf16 stage computes
the same function -- forward, every gradient, BatchNorm running statistics.
"""
import ctypes
import os

import pytest
import torch

import capi
import synth
from procedural import load_procedural, procedural_tensor

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm()) / (float(b.norm()) + 1e-30)


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (300, 136, 96), (4096, 256, 128), (1000, 288, 320),
                                   (77, 16, 544), (2048, 512, 256)])
def test_gemm_nt_matches_torch(M, N, K):
    gen = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    B = torch.randn((N, K), generator=gen).to(torch.bfloat16).to(dev())     # asymmetric, random
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    capi.ok("omnipq_gemm_nt_e16", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C), N)
    want = A.float() @ B.float().t()
    assert torch.isfinite(C.float()).all()
    # bf16 output rounding: half a step of 2^-8 relative to each element, plus f32 accumulation noise
    assert float((C.float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    assert rel_l2(C.float(), want) < 3e-3


@pytest.mark.parametrize("M,N,K,bias", [(4096, 288, 2048, True), (2048, 288, 1024, False), (300, 96, 4096, True),
                                        (4096, 2048, 288, True)])
def test_gemm_nt_split_k_matches_single_pass(M, N, K, bias):
    """Long contractions over few tiles are split over K; the result equals the single-pass kernel up to the bf16
    rounding of sums taken in a different f32 order."""
    gen = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    B = (torch.randn((N, K), generator=gen) / K ** 0.5).to(torch.bfloat16).to(dev())
    bvec = torch.randn(N, generator=gen).to(dev()) if bias else None
    capi.lib().omnipq_gemm_nt_workspace_floats.restype = ctypes.c_longlong
    n_ws = int(capi.lib().omnipq_gemm_nt_workspace_floats(M, N, K))
    assert (n_ws > 0) == (K >= 1024)
    ws = torch.empty(max(n_ws, 1), device=dev())
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    capi.ok("omnipq_gemm_nt_e16_ws", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C), N,
            capi.P(bvec) if bias else ctypes.c_void_p(0), capi.P(ws))
    want = A.float() @ B.float().t() + (bvec if bias else 0.0)
    assert torch.isfinite(C.float()).all()
    assert float((C.float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    assert rel_l2(C.float(), want) < 3e-3


@pytest.mark.parametrize("M,N,K,bias", [(100, 128, 32, False), (2048, 288, 288, False), (8192, 64, 64, True),
                                        (8193, 128, 128, False), (40000, 256, 32, False), (300, 544, 96, True)])
def test_gemm_nt_stats_epilogue(M, N, K, bias):
    """GEMM + BatchNorm statistics in one pass == the plain GEMM and the column sums of what it stored
    (both the direct-atomics and the per-tile-partials variants; sums are ADDED to the buffer)."""
    gen = torch.Generator().manual_seed(M + N + K)
    A = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    B = torch.randn((N, K), generator=gen).to(torch.bfloat16).to(dev())
    bvec = torch.randn(N, generator=gen).to(dev()) if bias else None
    C0 = torch.empty((M, N), device=dev(), dtype=torch.bfloat16)
    if bias:
        capi.ok("omnipq_gemm_nt_e16_bias", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C0), N, capi.P(bvec))
    else:
        capi.ok("omnipq_gemm_nt_e16", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C0), N)
    C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    sums = torch.ones((2, N), device=dev(), dtype=torch.float64)
    capi.lib().omnipq_gemm_nt_stats_workspace_floats.restype = ctypes.c_longlong
    n_ws = int(capi.lib().omnipq_gemm_nt_stats_workspace_floats(M, N))
    assert (n_ws == 0) == (M <= 64 * 128)
    ws = torch.empty(max(n_ws, 1), device=dev())
    capi.ok("omnipq_gemm_nt_e16_stats", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C), N,
            capi.P(bvec) if bias else ctypes.c_void_p(0), capi.P(sums), capi.P(ws))
    assert torch.equal(C, C0)
    y = C.double()
    want = torch.stack([y.sum(0), (y * y).sum(0)]) + 1.0
    # f32 partial sums over 128-row tiles, f64 across tiles
    assert float(((sums - want).abs() / (want.abs() + 1.0)).max()) < 1e-5


@pytest.mark.parametrize("M0,M1,N0,N1,K", [(2048, 2048, 288, 288, 288), (2048, 2048, 128, 32, 288), (300, 77, 96, 96, 64)])
def test_pair_launch_equals_two_launches(M0, M1, N0, N1, K):
    """omnipq_pair_hold / omnipq_pair_flush: two independent small GEMMs (plain, and with the statistics epilogue) go out
    as one grid and give the same bits as one after the other; a held GEMM without a partner goes out on flush, and a
    partner of another variant does not pair."""
    lib = capi.lib()
    lib.omnipq_pair_flush.restype = ctypes.c_longlong
    lib.omnipq_pair_hold.restype = None
    gen = torch.Generator().manual_seed(M0 + N1 + K)

    def problem(M, N):
        A = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
        B = torch.randn((N, K), generator=gen).to(torch.bfloat16).to(dev())
        bias = torch.randn(N, generator=gen).to(dev())
        return A, B, bias, M, N

    def run(pr, stats):
        A, B, bias, M, N = pr
        C = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
        sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
        if stats:
            capi.ok("omnipq_gemm_nt_e16_stats", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C), N, capi.P(bias),
                    capi.P(sums), ctypes.c_void_p(0))
        else:
            capi.ok("omnipq_gemm_nt_e16_bias", M, N, K, capi.P(A), K, capi.P(B), K, capi.P(C), N, capi.P(bias))
        return C, sums

    p0, p1 = problem(M0, N0), problem(M1, N1)
    for stats in (False, True):
        want0, want1 = run(p0, stats), run(p1, stats)
        before = int(lib.omnipq_pair_flush())
        lib.omnipq_pair_hold()
        got0 = run(p0, stats)
        got1 = run(p1, stats)
        after = int(lib.omnipq_pair_flush())
        assert after == before + 1                           # they did go out together
        for (c, s_), (c_want, s_want) in ((got0, want0), (got1, want1)):
            assert torch.equal(c, c_want)
            assert float(((s_ - s_want).abs() / (s_want.abs() + 1.0)).max()) < 1e-12 if stats else True
    # no partner: flush launches it alone
    lib.omnipq_pair_hold()
    alone = run(p0, False)
    n = int(lib.omnipq_pair_flush())
    assert torch.equal(alone[0], run(p0, False)[0])
    # different variants do not pair, both still run
    lib.omnipq_pair_hold()
    a = run(p0, False)
    b = run(p1, True)
    assert int(lib.omnipq_pair_flush()) == n
    assert torch.equal(a[0], run(p0, False)[0]) and torch.equal(b[0], run(p1, True)[0])


@pytest.mark.parametrize("M,N,K", [(100, 128, 32), (2048, 288, 288), (8320, 128, 256), (40000, 64, 128)])
def test_gemm_nt_bn_backward_epilogue(M, N, K):
    """Data-gradient GEMM with the BatchNorm-backward sums folded in == GEMM followed by omnipq_bn_bwd_stats."""
    gen = torch.Generator().manual_seed(M + N + K + 1)
    dY = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    Wt = (torch.randn((N, K), generator=gen) / K ** 0.5).to(torch.bfloat16).to(dev())
    Y = torch.randn((M, N), generator=gen).to(torch.bfloat16).to(dev())
    a = (torch.randn(N, generator=gen)).to(dev())
    b = (0.3 * torch.randn(N, generator=gen)).to(dev())
    mean = (0.1 * torch.randn(N, generator=gen)).to(dev())
    invstd = (0.5 + torch.rand(N, generator=gen)).to(dev())
    dX0 = torch.empty((M, N), device=dev(), dtype=torch.bfloat16)
    capi.ok("omnipq_gemm_nt_e16", M, N, K, capi.P(dY), K, capi.P(Wt), K, capi.P(dX0), N)
    want = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    capi.ok("omnipq_bn_bwd_stats", ctypes.c_longlong(M), N, capi.P(dX0), capi.P(Y), capi.P(a), capi.P(b),
            capi.P(mean), capi.P(invstd), capi.P(want))
    dX = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    capi.lib().omnipq_gemm_nt_stats_workspace_floats.restype = ctypes.c_longlong
    ws = torch.empty(max(int(capi.lib().omnipq_gemm_nt_stats_workspace_floats(M, N)), 1), device=dev())
    capi.ok("omnipq_gemm_nt_e16_bnbwd", M, N, K, capi.P(dY), K, capi.P(Wt), K, capi.P(dX), N, capi.P(Y), capi.P(a),
            capi.P(b), capi.P(mean), capi.P(invstd), capi.P(sums), capi.P(ws))
    assert torch.equal(dX, dX0)
    scale = want.abs().max(dim=1, keepdim=True).values + 1e-3          # f32 partial sums, different order
    assert float(((sums - want).abs() / scale).max()) < 1e-5


@pytest.mark.parametrize("P,M,N", [(32, 128, 128), (1000, 72, 40), (8192, 256, 128), (5000, 288, 320),
                                   (333, 16, 544)])
def test_gemm_tn_matches_torch(P, M, N):
    gen = torch.Generator().manual_seed(P + M + N)
    A = torch.randn((P, M), generator=gen).to(torch.bfloat16).to(dev())
    B = torch.randn((P, N), generator=gen).to(torch.bfloat16).to(dev())
    C = torch.full((M, N), float("nan"), device=dev())
    capi.lib().omnipq_gemm_tn_workspace_floats.restype = ctypes.c_longlong
    ws = torch.empty(int(capi.lib().omnipq_gemm_tn_workspace_floats(M, N, P)), device=dev())
    capi.ok("omnipq_gemm_tn_e16", M, N, P, capi.P(A), M, capi.P(B), N, capi.P(C), capi.P(ws))
    want = A.float().t() @ B.float()
    assert rel_l2(C, want) < 1e-5          # exact bf16 products, f32 accumulation: only summation order differs
    # the variant that also returns the column sums of A (bias gradient), added to what is there
    C2 = torch.full((M, N), float("nan"), device=dev())
    cs = torch.ones(M, device=dev())
    capi.ok("omnipq_gemm_tn_e16_colsum", M, N, P, capi.P(A), M, capi.P(B), N, capi.P(C2), capi.P(ws), capi.P(cs))
    assert rel_l2(C2, want) < 1e-5
    tot = A.double().sum(0) + 1.0
    assert float((cs.double() - tot).abs().max()) < 1e-4 * (1 + float(tot.abs().max()))


def _sa_pair(spec, seed):
    import pointnet2_modules
    mods = []
    for _ in range(2):
        m = pointnet2_modules.PointnetSAModuleVotes(mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"})
        load_procedural(m, seed)
        mods.append(m.to(dev()).train())
    return mods


SA_SPECS = [
    # sa1-like: no input features
    (dict(npoint=512, radius=0.3, nsample=64, mlp=[0, 64, 64, 128], use_xyz=True, normalize_xyz=True), 4096, 0),
    # sa2-like: 32 nsample, wide
    (dict(npoint=256, radius=0.4, nsample=32, mlp=[128, 128, 128, 256], use_xyz=True, normalize_xyz=True), 2048, 128),
    # vote-aggregation-like: 288 channels (not a multiple of the 128-wide tile), 16 nsample
    (dict(npoint=128, radius=0.5, nsample=16, mlp=[288, 288, 288, 288], use_xyz=True, normalize_xyz=True), 1024, 288),
    # two-layer MLP, un-normalised xyz
    (dict(npoint=64, radius=0.6, nsample=16, mlp=[16, 32, 64], use_xyz=True, normalize_xyz=False), 512, 16),
]


@pytest.mark.parametrize("spec,n,cin", SA_SPECS)
def test_fused_sa_stage_matches_f32_composition(spec, n, cin, monkeypatch):
    _fused_vs_f32(spec, n, cin, 2, monkeypatch)


def test_fused_sa_stage_config4_50k_points_six_extra_channels(monkeypatch):
    """BASELINE configs[3]: ARKitScenes-like clouds of 50 000 points with 6 extra input channels (rgb + normals), batch 4
    per GPU -- sa1 with a 9-channel first layer (the 6 feature channels travel padded to 8) and the hash-grid ball
    query at 50 000 points, against the f32 op-by-op composition."""
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[6, 64, 64, 128], use_xyz=True, normalize_xyz=True)
    _fused_vs_f32(spec, 50000, 6, 4, monkeypatch)


def test_fused_sa_stage_config5_80k_points(monkeypatch):
    """BASELINE configs[4]: dense clouds of 80 000 points (batch 16 per GPU in the benchmark; 2 scenes here so that the f32
    op-by-op yardstick fits the test's time): sa1 of the backbone with the hash-grid ball query at 80 000 points and the
    multi-workgroup furthest-point sampling, in bf16 (the type this configuration is measured in: DESIGN.md §6), against
    the f32 composition."""
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[0, 64, 64, 128], use_xyz=True, normalize_xyz=True)
    _fused_vs_f32(spec, 80000, 0, 2, monkeypatch)


def test_fused_sa_stage_config4_at_the_backbones_real_widths(monkeypatch):
    """BASELINE configs[3] as the backbone runs it (reference models/backbone_module.py:38-46 with input_feature_dim=6):
    sa1 = 2048 centres, r 0.2, 64 samples, mlp [6, 128, 128, 256] on 4 scenes x 50 000 points."""
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[6, 128, 128, 256], use_xyz=True, normalize_xyz=True)
    _fused_vs_f32(spec, 50000, 6, 4, monkeypatch)


def test_fused_sa_stage_config5_at_the_backbones_real_widths(monkeypatch):
    """BASELINE configs[4] at sa1's real widths [0, 128, 128, 256] on 80 000-point clouds (4 scenes: the f32 op-by-op
    yardstick materialises (B, 256, 2048, 64) tensors); no gradient into the coordinates, as in the backbone, so the
    coordinate-generated first layer is the path that runs."""
    import sa_fused
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[0, 128, 128, 256], use_xyz=True, normalize_xyz=True)
    before = sa_fused.xyzgen_uses
    _fused_vs_f32(spec, 80000, 0, 4, monkeypatch, xyz_grad=False)
    assert sa_fused.xyzgen_uses == before + 1


def test_first_layer_generated_from_coordinates_matches_f32_composition(monkeypatch):
    """sa1 as the backbone runs it: no input features and no gradient into the coordinates, so the first layer (conv 3 -> C)
    is never materialised (sa_fused.XYZGEN: activations rebuilt from the grouped coordinates inside the consumer GEMMs,
    BatchNorm statistics and the weight gradient from the coordinate moments).  Same yardstick as the stored dataflow:
    the f32 op-by-op composition, with PyTorch's bf16 autocast path as the noise floor -- and the stored dataflow beside it."""
    import sa_fused
    spec, n, cin = SA_SPECS[0]
    before = sa_fused.xyzgen_uses
    gen = _fused_vs_f32(spec, n, cin, 2, monkeypatch, xyz_grad=False)
    assert sa_fused.xyzgen_uses == before + 1                       # the path under test is the one that ran
    monkeypatch.setattr(sa_fused, "XYZGEN", False)
    stored = _fused_vs_f32(spec, n, cin, 2, monkeypatch, xyz_grad=False)
    assert sa_fused.xyzgen_uses == before + 1
    for k in gen:                                                   # not worse than the stored dataflow by more than noise
        assert gen[k] < max(1.5 * stored[k], 2e-2), (k, gen[k], stored[k])


def _fused_vs_f32(spec, n, cin, B, monkeypatch, xyz_grad=True, dtype=torch.bfloat16, g_scale=1.0):
    xyz = synth.make_clouds(41, B, n, kind="room").to(dev())
    feats = None
    if cin:
        feats = procedural_tensor("fused.feats", (B, cin, n), torch.float32).to(dev())
    import pointnet2_modules
    ref_mod, fus_mod = _sa_pair(spec, seed=3)
    amp_mod = load_procedural(pointnet2_modules.PointnetSAModuleVotes(
        mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"}), 3).to(dev()).train()
    want_xyz = xyz.clone().requires_grad_(xyz_grad)    # gradients w.r.t. coordinates (vote aggregation)
    got_xyz = xyz.clone().requires_grad_(xyz_grad)
    amp_xyz = xyz.clone().requires_grad_(xyz_grad)
    want_f = None if feats is None else feats.clone().requires_grad_(True)
    got_f = None if feats is None else feats.clone().requires_grad_(True)
    amp_f = None if feats is None else feats.clone().requires_grad_(True)

    monkeypatch.setenv("OMNIPQ_SA", "composed")
    w_new_xyz, w_out, w_inds = ref_mod(want_xyz, want_f)               # f32 op-by-op: the yardstick
    with torch.autocast("cuda", dtype=dtype):                           # PyTorch's own 16-bit autocast path
        _, a_out, _ = amp_mod(amp_xyz, amp_f)
    monkeypatch.setenv("OMNIPQ_SA", "fused")
    with torch.autocast("cuda", dtype=dtype):
        g_new_xyz, g_out, g_inds = fus_mod(got_xyz, got_f)
    import sa_fused
    assert sa_fused.E16.dtype == dtype and g_out.omnipq_rows16.dtype == dtype
    assert torch.equal(w_inds, g_inds) and torch.equal(w_new_xyz, g_new_xyz)
    assert g_out.dtype == torch.float32 and g_out.shape == w_out.shape
    assert rel_l2(g_out, w_out) < 2e-2, rel_l2(g_out, w_out)

    g_up = procedural_tensor("fused.g_up", tuple(w_out.shape), torch.float32).to(dev()) * g_scale
    w_out.backward(g_up)
    g_out.backward(g_up)
    a_out.float().backward(g_up)

    errors = {"out": rel_l2(g_out, w_out)}

    def ok(name, got, amp, want, floor):
        """bf16 gradients are sums of ~1e5 quantised signed terms: demand the fused stage be no further
        from the f32 result than `floor`, or than twice what PyTorch's bf16 autocast path manages."""
        e_got, e_amp = rel_l2(got, want), rel_l2(amp, want)
        errors[name] = e_got
        assert e_got < max(floor, 2.0 * e_amp), (name, e_got, e_amp)

    for (k, pw), (_, pg), (_, pa) in zip(ref_mod.named_parameters(), fus_mod.named_parameters(),
                                         amp_mod.named_parameters()):
        assert pg.grad is not None and pg.grad.shape == pw.grad.shape, k
        ok(k, pg.grad, pa.grad, pw.grad, 6e-2)
    if feats is not None:
        ok("features", got_f.grad, amp_f.grad, want_f.grad, 6e-2)
    if xyz_grad:
        ok("xyz", got_xyz.grad, amp_xyz.grad, want_xyz.grad, 8e-2)
    for (k, bw), (_, bg) in zip(ref_mod.named_buffers(), fus_mod.named_buffers()):
        if bw.is_floating_point():
            assert rel_l2(bg, bw) < 1e-2, k
        else:
            assert torch.equal(bg, bw), k       # num_batches_tracked
    return errors


@pytest.mark.parametrize("case", ["sa1_like", "sa2_like", "vote_like", "six_padded_features"])
def test_sa_weight_gradients_deferred_into_one_grouped_launch_equal_the_immediate_ones(case, monkeypatch):
    """Inside `sa_fused.deferred_wgrads()` the layers of a fused SA stage hand their weight gradients to the block
    (`add_sa`): one grouped launch for all stages at its end, the first layer's columns rotated back from the kernels'
    [features | xyz] order to the parameter's [xyz | features] (and the zero-padded feature columns dropped) by the
    launch's reduction.  Same operands, another partition of the position axis: equal to the immediate GEMMs up to f32
    summation order."""
    import pointnet2_modules
    import sa_fused
    spec, n, cin = {"sa1_like": SA_SPECS[0], "sa2_like": SA_SPECS[1], "vote_like": SA_SPECS[2],
                    "six_padded_features": (dict(npoint=256, radius=0.4, nsample=32, mlp=[6, 64, 64, 128], use_xyz=True,
                                                 normalize_xyz=True), 4096, 6)}[case]
    xyz = synth.make_clouds(47, 2, n, kind="room").to(dev())
    feats = procedural_tensor("defer.feats", (2, cin, n), torch.float32).to(dev()) if cin else None
    monkeypatch.setenv("OMNIPQ_SA", "fused")
    grads = {}
    for mode in ("immediate", "deferred"):
        mod = load_procedural(pointnet2_modules.PointnetSAModuleVotes(
            mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"}), 9).to(dev()).train()
        f = None if feats is None else feats.clone().requires_grad_(True)
        h0 = sa_fused.hoist_uses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, out, _ = mod(xyz, f)
        hoisted = sa_fused.hoist_uses > h0
        g_up = procedural_tensor("defer.g_up", tuple(out.shape), torch.float32).to(dev())
        if mode == "deferred":
            with sa_fused.deferred_wgrads() as dfr:
                out.backward(g_up)
                # sa1-like stages generate their first layer from coordinates: its gradient comes from moments, the second
                # layer's from the coordinate-generating GEMM -- only the third is an ordinary weight-gradient problem
                expect = 1 if case == "sa1_like" else len(spec["mlp"]) - 1
                if hoisted:
                    expect += 1        # the first layer on the source points hands over two problems (features | coordinates)
                assert len(dfr.sa_items) == expect, "the stage did not hand its weight gradients over"
                assert all(p.grad is None for k, p in mod.named_parameters() if k.endswith("conv.weight")
                           and not (case == "sa1_like" and ("layer0" in k or "layer1" in k)))
        else:
            out.backward(g_up)
        grads[mode] = {k: p.grad.clone() for k, p in mod.named_parameters()}
    for k, g in grads["immediate"].items():
        assert grads["deferred"][k].shape == g.shape, k
        assert rel_l2(grads["deferred"][k], g) < 2e-5, (k, rel_l2(grads["deferred"][k], g))


def test_fused_sa_eval_mode_uses_running_statistics(monkeypatch):
    spec, n, cin = SA_SPECS[1]
    xyz = synth.make_clouds(43, 2, n, kind="room").to(dev())
    feats = procedural_tensor("fused.feats", (2, cin, n), torch.float32).to(dev())
    ref_mod, fus_mod = _sa_pair(spec, seed=5)
    ref_mod.eval()
    fus_mod.eval()
    with torch.no_grad():
        monkeypatch.setenv("OMNIPQ_SA", "composed")
        _, w_out, _ = ref_mod(xyz, feats)
        monkeypatch.setenv("OMNIPQ_SA", "fused")
        _, g_out, _ = fus_mod(xyz, feats)
    assert rel_l2(g_out, w_out) < 2e-2


def test_fused_stage_is_selected_under_16_bit_autocast_only(monkeypatch):
    import pointnet2_modules
    monkeypatch.delenv("OMNIPQ_SA", raising=False)
    spec, n, cin = SA_SPECS[0]
    mod = pointnet2_modules.PointnetSAModuleVotes(mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"}).to(dev())
    xyz = synth.make_clouds(44, 1, n, kind="room").to(dev())
    assert not mod._fused(xyz, None)
    import sa_fused
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert mod._fused(xyz, None) and sa_fused.E16.dtype == torch.bfloat16
    with torch.autocast("cuda", dtype=torch.float16):                     # the IEEE-half library (BASELINE configs[4])
        assert mod._fused(xyz, None) and sa_fused.E16.dtype == torch.float16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert mod._fused(xyz, None) and sa_fused.E16.dtype == torch.bfloat16


def test_graph_replay_reproduces_the_eager_step():
    """bench.py's hipGraph mode (whole step captured once, next batch's sampling pipelined on the side
    stream through the backbone's persistent plan buffers) must compute what the eager step computes:
    same loss per batch, same gradients."""
    import argparse
    import bench
    from test_oracle_golden import zero_dropout

    def run(graph):
        torch.manual_seed(7)
        net = bench.build_model(0).to(dev()).train()
        zero_dropout(net)                                       # dropout would draw different masks
        pool = [synth.make_clouds(70 + i, 2, 8192, kind="room").to(dev()) for i in range(3)]
        args = argparse.Namespace(graph="on" if graph else "off", no_prefetch=False, warmup=3)
        step, mode = bench.make_step(net, net, pool, args, torch.bfloat16, 1)
        losses = []
        for i in range(5):
            losses.append(float(step(i).detach()))
        torch.cuda.synchronize()
        gnorm = torch.stack([p.grad.float().norm() for p in net.parameters() if p.grad is not None])
        return mode, losses, gnorm.cpu()

    m0, l0, g0 = run(False)
    m1, l1, g1 = run(True)
    assert m0 == "eager" and m1 == "hipGraph replay"
    # BN running statistics evolve with every step (warm-up included), so compare batch-for-batch
    # losses loosely and the periodicity exactly: batches repeat with period 3
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 2e-2 * abs(a), (l0, l1)
    assert rel_l2(g1, g0) < 5e-2


@pytest.mark.parametrize("na,nb,wa,wb", [(2048, 2048, (288, 288, 128), (288, 288, 32)), (2048, 1000, (288, 288, 128), (288, 32)),
                                         (300, 300, (96, 64), (96, 64))])
def test_rows_mlp_pair_equals_the_two_stacks(na, nb, wa, wb):
    """rows_mlp.run_pair (two independent stacks in lockstep, their GEMMs launched pairwise) against rows_mlp.run on
    each: same outputs, input gradients, parameter gradients and running statistics; the GEMMs did pair (launch counter);
    stacks of different depth still work (the longer one's tail goes out alone); one output unused downstream."""
    import rows_mlp
    import capi
    d = dev()
    cin = 288 if wa[0] == 288 else 96
    lib = capi.lib()
    lib.omnipq_pair_flush.restype = ctypes.c_longlong

    def build(seed, widths):
        torch.manual_seed(seed)
        lins, bns = [], []
        c = cin
        for i, w in enumerate(widths):
            lins.append(torch.nn.Conv1d(c, w, 1).to(d))
            bns.append(torch.nn.BatchNorm1d(w).to(d) if i < len(widths) - 1 else None)
            if bns[-1] is not None:
                with torch.no_grad():
                    bns[-1].weight.uniform_(0.5, 1.5)
                    bns[-1].bias.uniform_(-0.3, 0.3)
            c = w
        return lins, bns

    xa0, xb0 = torch.randn(na, cin, device=d), torch.randn(nb, cin, device=d)
    ga, gb = torch.randn(na, wa[-1], device=d), torch.randn(nb, wb[-1], device=d)

    def run(pair, use_b=True):
        (la, ba), (lb, bb) = build(21, wa), build(22, wb)
        xa, xb = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
        sa = [rows_mlp.Layer(l.weight, l.bias, b) for l, b in zip(la, ba)]
        sb = [rows_mlp.Layer(l.weight, l.bias, b) for l, b in zip(lb, bb)]
        before = int(lib.omnipq_pair_flush())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            if pair:
                ya, yb = rows_mlp.run_pair(xa, sa, xb, sb, True)
            else:
                ya, yb = rows_mlp.run(xa, sa, True), rows_mlp.run(xb, sb, True)
        loss = (ya.float() * ga).sum()
        if use_b:
            loss = loss + (yb.float() * gb).sum()
        loss.backward()
        pairs = int(lib.omnipq_pair_flush()) - before
        mods = [m for m in la + ba + lb + bb if m is not None]
        grads = [xa.grad] + ([xb.grad] if use_b else []) + \
            [p.grad for m in mods for p in m.parameters() if p.grad is not None]
        stats = [t.clone() for m in ba + bb if m is not None for t in (m.running_mean, m.running_var)]
        return ya.detach(), yb.detach(), grads, stats, pairs

    for use_b in (True, False):
        y1a, y1b, g1, s1, pairs = run(True, use_b)
        y0a, y0b, g0, s0, none = run(False, use_b)
        assert none == 0
        if len(wa) == len(wb):          # same structure: every forward GEMM paired, and every backward one if both are used
            # (backward: the data-gradient GEMM of every layer and the BatchNorm-backward apply of every BN layer)
            assert pairs == len(wa) + ((2 * len(wa) - 1) if use_b else 0), pairs
        else:                           # otherwise the first layers at least (same kind of GEMM)
            assert pairs >= 1
        assert torch.equal(y1a, y0a) and torch.equal(y1b, y0b)
        assert len(g1) == len(g0)
        for u, v in zip(g1, g0):
            assert rel_l2(u, v) < 1e-5, rel_l2(u, v)
        for u, v in zip(s1, s0):
            assert torch.equal(u, v)


@pytest.mark.parametrize("cin,widths,n", [(288, (288, 288, 97), 2048), (3, (288, 288), 8192), (288, (288, 288, 291), 8192),
                                          (1024, (512, 288), 4096)])
def test_rows_mlp_matches_f32_layers(cin, widths, n):
    """rows_mlp.RowsMLP (linear [+BN+ReLU] stacks on the hand-written kernels) against the same stack in f32
    PyTorch: outputs, every parameter gradient, the input gradient, BatchNorm running statistics.
    Layer layout as in the reference's heads: all but the last layer are Linear(bias)+BN+ReLU."""
    import rows_mlp
    torch.manual_seed(cin + n)
    d = dev()

    def build():
        torch.manual_seed(11)
        lins, bns = [], []
        c = cin
        for i, w in enumerate(widths):
            lins.append(torch.nn.Conv1d(c, w, 1).to(d))
            bns.append(torch.nn.BatchNorm1d(w).to(d) if i < len(widths) - 1 else None)
            if bns[-1] is not None:
                with torch.no_grad():
                    bns[-1].weight.uniform_(0.5, 1.5)
                    bns[-1].bias.uniform_(-0.3, 0.3)
            c = w
        return lins, bns

    x0 = torch.randn(n, cin, device=d)
    g_up = torch.randn(n, widths[-1], device=d)

    lins, bns = build()
    x_ref = x0.clone().requires_grad_(True)
    h = x_ref
    for lin_, bn in zip(lins, bns):
        h = torch.nn.functional.linear(h, lin_.weight.squeeze(-1), lin_.bias)
        if bn is not None:
            h = torch.relu(bn(h))
    h.backward(g_up)
    ref_out = h.detach()

    lins2, bns2 = build()
    x_got = x0.clone().requires_grad_(True)
    stack = [rows_mlp.Layer(l.weight, l.bias, b) for l, b in zip(lins2, bns2)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert rows_mlp.usable(x_got, stack, True)
        y = rows_mlp.run(x_got, stack, True)
    assert y.shape == ref_out.shape
    y.float().backward(g_up)
    assert rel_l2(y, ref_out) < 2e-2
    assert rel_l2(x_got.grad, x_ref.grad) < 1e-1          # three bf16 layers deep
    for a, b in zip(lins2, lins):
        assert rel_l2(a.weight.grad, b.weight.grad) < 1e-1
    # bias of the last (plain) layer has a real gradient; biases feeding a BatchNorm have exactly zero
    assert rel_l2(lins2[-1].bias.grad, lins[-1].bias.grad) < 3e-2
    for a, bn in zip(lins2[:-1], bns2[:-1]):
        assert float(a.bias.grad.abs().max()) == 0.0
    for a, b in zip(bns2[:-1], bns[:-1]):
        assert rel_l2(a.weight.grad, b.weight.grad) < 1e-1 and rel_l2(a.bias.grad, b.bias.grad) < 1e-1
        assert rel_l2(a.running_mean, b.running_mean) < 1e-2 and rel_l2(a.running_var, b.running_var) < 1e-2
        assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1


def test_feature_propagation_on_rows_matches_f32_composition(monkeypatch):
    """SA -> SA -> FP chain: under bf16 autocast the FP module takes the position-major twins of the fused SA
    outputs (interpolation + concatenation + MLP on rows, no (B, C, n) round trip) and must agree with the f32
    composition of the reference ops, outputs and gradients, within the bf16 tolerances of the fused SA tests."""
    import pointnet2_modules
    import sa_fused

    class Chain(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.sa1 = pointnet2_modules.PointnetSAModuleVotes(npoint=256, radius=0.5, nsample=32, mlp=[0, 64, 64, 128],
                                                               use_xyz=True, normalize_xyz=True)
            self.sa2 = pointnet2_modules.PointnetSAModuleVotes(npoint=64, radius=1.0, nsample=16, mlp=[128, 128, 128, 256],
                                                               use_xyz=True, normalize_xyz=True)
            self.fp = pointnet2_modules.PointnetFPModule(mlp=[256 + 128, 256, 96])

        def forward(self, xyz):
            x1, f1, _ = self.sa1(xyz, None)
            x2, f2, _ = self.sa2(x1, f1)
            return self.fp(x1, x2, f1, f2)

    nets = [load_procedural(Chain(), 3).to(dev()).train() for _ in range(3)]
    xyz = (torch.rand(4, 2048, 3, generator=torch.Generator().manual_seed(5)) * 3).to(dev())
    monkeypatch.setenv("OMNIPQ_SA", "composed")
    want = nets[0](xyz)                                                  # f32 op-by-op: the yardstick
    with torch.autocast("cuda", dtype=torch.bfloat16):                   # PyTorch's own bf16 path
        amp = nets[2](xyz)
    monkeypatch.delenv("OMNIPQ_SA")
    calls = []
    orig = sa_fused.FPGatherRows.apply
    monkeypatch.setattr(sa_fused.FPGatherRows, "apply", staticmethod(lambda *a: (calls.append(1), orig(*a))[1]))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        got = nets[1](xyz)
    assert calls, "the rows path of the FP module did not run"
    assert got.shape == want.shape

    def ok(name, g_, a_, w_, floor):
        e_got, e_amp = rel_l2(g_.float(), w_), rel_l2(a_.float(), w_)
        assert e_got < max(floor, 2.0 * e_amp), (name, e_got, e_amp)

    ok("output", got, amp, want, 3e-2)
    g = torch.randn(want.shape, generator=torch.Generator().manual_seed(6)).to(dev())
    a = torch.autograd.grad(got, list(nets[1].parameters()), g.to(got.dtype))
    b = torch.autograd.grad(want, list(nets[0].parameters()), g)
    c = torch.autograd.grad(amp, list(nets[2].parameters()), g.to(amp.dtype))
    for (name, _), u, v, w in zip(nets[0].named_parameters(), a, b, c):
        ok(name, u, w, v, 8e-2)


@pytest.mark.parametrize("B,n,m,C,extra", [(2, 300, 70, 64, 0), (3, 1024, 512, 512, 256), (1, 5, 3, 8, 8)])
def test_interp_rows_kernels_match_torch(B, n, m, C, extra):
    """Feature propagation on rows: interpolation into a column range, both gradient kernels (atomics / CSR of
    readers), the column placement and the column sums, against plain PyTorch on the same bf16 operands."""
    gen = torch.Generator().manual_seed(B + n + m + C)
    feat = torch.randn(B, m, C, generator=gen).to(torch.bfloat16).to(dev())
    idx = torch.randint(0, m, (B, n, 3), generator=gen).to(torch.int32).to(dev())
    w = torch.rand(B, n, 3, generator=gen)
    w = (w / w.sum(-1, keepdim=True)).to(dev())
    ld = C + extra
    rows = torch.zeros(B * n, ld, device=dev(), dtype=torch.bfloat16)
    capi.ok("omnipq_interp_rows", B, n, m, C, capi.P(feat), capi.P(idx), capi.P(w), capi.P(rows), ld, 0)
    gathered = torch.stack([feat[b][idx[b].long()] for b in range(B)]).float()          # (B, n, 3, C)
    want = (gathered * w.unsqueeze(-1)).sum(2).reshape(B * n, C)
    assert float((rows[:, :C].float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()) + 1e-6
    if extra:
        skip = torch.randn(B * n, extra, generator=gen).to(torch.bfloat16).to(dev())
        capi.ok("omnipq_place_rows", ctypes.c_longlong(B * n), extra, capi.P(skip), capi.P(rows), ld, C)
        assert torch.equal(rows[:, C:], skip)
        assert float((rows[:, :C].float() - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max()) + 1e-6
    # gradient: dfeat[b][j] = sum over (i, k) with idx[b,i,k] == j of w[b,i,k] * g[(b,i)]
    g = torch.randn(B * n, ld, generator=gen).to(torch.bfloat16).to(dev())
    ref = torch.zeros(B, m, C, device=dev())
    for b in range(B):
        contrib = (g[b * n:(b + 1) * n, :C].float().unsqueeze(1) * w[b].unsqueeze(-1)).reshape(n * 3, C)
        ref[b].index_add_(0, idx[b].reshape(-1).long(), contrib)
    d1 = torch.zeros(B, m, C, device=dev())
    capi.ok("omnipq_interp_rows_grad", B, n, m, C, capi.P(g), ld, 0, capi.P(idx), capi.P(w), capi.P(d1))
    offsets = torch.empty(B, m + 1, device=dev(), dtype=torch.int32)
    order = torch.empty(B, 3 * n, device=dev(), dtype=torch.int32)
    scratch = torch.empty(B, m, device=dev(), dtype=torch.int32)
    capi.ok("omnipq_sa_build_csr", B, m, n, 3, capi.P(idx), capi.P(offsets), capi.P(order), capi.P(scratch))
    d2 = torch.full((B, m, C), float("nan"), device=dev())
    capi.ok("omnipq_interp_rows_grad_csr", B, n, m, C, capi.P(g), ld, 0, capi.P(offsets), capi.P(order), capi.P(w),
            capi.P(d2))
    for d in (d1, d2):
        assert torch.isfinite(d).all()
        assert rel_l2(d, ref) < 1e-5
    # column sums (bias gradients), both accumulator types; they ADD to what is there
    s64 = torch.ones(ld, device=dev(), dtype=torch.float64)
    s32 = torch.ones(ld, device=dev())
    capi.ok("omnipq_colsum", ctypes.c_longlong(B * n), ld, capi.P(g), capi.P(s64))
    capi.ok("omnipq_colsum_f32", ctypes.c_longlong(B * n), ld, capi.P(g), capi.P(s32))
    tot = g.double().sum(0) + 1.0
    assert float((s64 - tot).abs().max()) < 1e-4 * (1 + float(tot.abs().max()))
    assert float((s32.double() - tot).abs().max()) < 1e-3 * (1 + float(tot.abs().max()))


@pytest.mark.parametrize("M,N,K,stats,bias", [(100, 128, 32, True, False), (2048, 288, 288, True, True),
                                             (8320, 128, 256, True, False), (4096, 96, 288, False, True),
                                             (333, 544, 64, False, False)])
def test_gemm_nt_affine_operand_equals_the_materialised_activations(M, N, K, stats, bias):
    """relu(a * Y + b) built inside the GEMM's operand staging == omnipq_bnrelu followed by the plain GEMM: the same
    bf16 activations enter the MFMAs, so outputs (and the statistics epilogue) are the same bits."""
    gen = torch.Generator().manual_seed(M + N + K + 7)
    Y = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    W = (torch.randn((N, K), generator=gen) / K ** 0.5).to(torch.bfloat16).to(dev())
    a = (0.5 + torch.rand(K, generator=gen)).to(dev()) * torch.where(torch.rand(K, generator=gen) < 0.2, -1.0, 1.0).to(dev())
    b = (0.3 * torch.randn(K, generator=gen)).to(dev())
    bvec = torch.randn(N, generator=gen).to(dev()) if bias else None
    X = torch.empty_like(Y)
    capi.ok("omnipq_bnrelu", ctypes.c_longlong(M), K, capi.P(Y), capi.P(a), capi.P(b), capi.P(X))
    want = torch.empty((M, N), device=dev(), dtype=torch.bfloat16)
    null = ctypes.c_void_p(0)
    capi.lib().omnipq_gemm_nt_stats_workspace_floats.restype = ctypes.c_longlong
    ws = torch.empty(max(int(capi.lib().omnipq_gemm_nt_stats_workspace_floats(M, N)), 1), device=dev())
    want_sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    if stats:
        capi.ok("omnipq_gemm_nt_e16_stats", M, N, K, capi.P(X), K, capi.P(W), K, capi.P(want), N,
                capi.P(bvec) if bias else null, capi.P(want_sums), capi.P(ws))
    else:
        capi.ok("omnipq_gemm_nt_e16_bias", M, N, K, capi.P(X), K, capi.P(W), K, capi.P(want), N,
                capi.P(bvec) if bias else null)
    got = torch.full((M, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    capi.ok("omnipq_gemm_nt_e16_affine", M, N, K, capi.P(Y), K, capi.P(a), capi.P(b), capi.P(W), K, capi.P(got), N,
            capi.P(bvec) if bias else null, capi.P(sums) if stats else null, capi.P(ws))
    assert torch.equal(got, want)
    if stats:
        scale = want_sums.abs().max(dim=1, keepdim=True).values + 1e-3
        assert float(((sums - want_sums).abs() / scale).max()) < 1e-6
    # and against f64 torch on the rounded activations
    ref = X.double() @ W.double().t() + (bvec.double() if bias else 0.0)
    assert float((got.double() - ref).abs().max()) <= 2.0 ** -8 * float(ref.abs().max())


@pytest.mark.parametrize("P,M,N,colsum", [(1000, 72, 40, False), (8192, 256, 128, True), (5000, 288, 320, True),
                                          (33, 128, 32, False)])
def test_gemm_tn_affine_operand_equals_the_materialised_activations(P, M, N, colsum):
    gen = torch.Generator().manual_seed(P + M + N + 3)
    dY = torch.randn((P, M), generator=gen).to(torch.bfloat16).to(dev())
    Y = torch.randn((P, N), generator=gen).to(torch.bfloat16).to(dev())
    a = (0.5 + torch.rand(N, generator=gen)).to(dev()) * torch.where(torch.rand(N, generator=gen) < 0.2, -1.0, 1.0).to(dev())
    b = (0.3 * torch.randn(N, generator=gen)).to(dev())
    X = torch.empty_like(Y)
    capi.ok("omnipq_bnrelu", ctypes.c_longlong(P), N, capi.P(Y), capi.P(a), capi.P(b), capi.P(X))
    capi.lib().omnipq_gemm_tn_workspace_floats.restype = ctypes.c_longlong
    ws = torch.empty(int(capi.lib().omnipq_gemm_tn_workspace_floats(M, N, P)), device=dev())
    want = torch.empty((M, N), device=dev())
    capi.ok("omnipq_gemm_tn_e16", M, N, P, capi.P(dY), M, capi.P(X), N, capi.P(want), capi.P(ws))
    got = torch.full((M, N), float("nan"), device=dev())
    cs = torch.zeros(M, device=dev()) if colsum else None
    capi.ok("omnipq_gemm_tn_e16_affine", M, N, P, capi.P(dY), M, capi.P(Y), N, capi.P(a), capi.P(b), capi.P(got),
            capi.P(ws), capi.P(cs) if colsum else ctypes.c_void_p(0))
    assert torch.equal(got, want)
    ref = dY.double().t() @ X.double()
    assert float((got.double() - ref).abs().max()) < 1e-5 * (float(ref.abs().max()) + 1.0) * P ** 0.5
    if colsum:
        assert float((cs.double() - dY.double().sum(0)).abs().max()) < 1e-4 * (float(dY.double().sum(0).abs().max()) + 1.0)


def test_stacks_without_stored_activations_equal_the_materialised_dataflow(monkeypatch):
    """sa_fused.AFFINE_OPERANDS: rows_mlp stacks and the fused SA stage with relu(bn(Y)) rebuilt inside the consumer
    GEMMs give the outputs, input gradients and parameter gradients of the dataflow that stores the activations
    (the same bf16 values enter every MFMA; only f32 summation orders of the deferred paths may differ)."""
    import rows_mlp
    import sa_fused
    torch.manual_seed(5)
    d = dev()
    lins = [torch.nn.Conv1d(288, 288, 1).to(d), torch.nn.Conv1d(288, 288, 1).to(d), torch.nn.Conv1d(288, 97, 1).to(d)]
    bns = [torch.nn.BatchNorm1d(288).to(d), torch.nn.BatchNorm1d(288).to(d), None]
    for bn in bns[:2]:
        with torch.no_grad():
            bn.weight.uniform_(-1.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    x = torch.randn(4096, 288, device=d).requires_grad_(True)
    g = torch.randn(4096, 97, device=d).to(torch.bfloat16)
    params = [t for l_ in lins for t in (l_.weight, l_.bias)] + [t for bn in bns[:2] for t in (bn.weight, bn.bias)]
    state = [{k: v.clone() for k, v in bn.state_dict().items()} for bn in bns[:2]]

    def run(flag):
        monkeypatch.setattr(sa_fused, "AFFINE_OPERANDS", flag)
        for bn, st in zip(bns[:2], state):
            bn.load_state_dict(st)
        for t in [x] + params:
            t.grad = None
        stack = [rows_mlp.Layer(l_.weight, l_.bias, bn) for l_, bn in zip(lins, bns)]
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = rows_mlp.run(x, stack, True)
        y.backward(g)
        return y.detach().clone(), [t.grad.clone() for t in [x] + params], [bn.running_var.clone() for bn in bns[:2]]

    y1, g1, rv1 = run(True)
    y0, g0, rv0 = run(False)
    assert torch.equal(y1, y0)
    assert torch.equal(g1[0], g0[0])                 # input gradient: same bits
    for u, v in zip(g1[1:], g0[1:]):                 # f32 atomics (bias column sums) and f64 atomics (BN sums) may
        assert rel_l2(u, v) < 1e-6                   # land in a different order from run to run
    for u, v in zip(rv1, rv0):
        assert rel_l2(u, v) < 1e-6


def test_weight_gradients_flushed_on_the_side_stream_are_the_same(monkeypatch):
    """pq_transformer._WGRAD_SIDE: the decoder's / heads' collected weight gradients start on the sampling stream
    when the gradient reaches the backbone (sa_fused.WgradFlushPoint) instead of at the end of backward.  Every
    problem is computed by the same kernel with the same partition either way: against the same graph with the
    early flush switched off, all parameter gradients agree to the run-to-run noise of the step (f64 / f32 atomics
    in the statistics; the flush point itself re-associates the bf16 sum of the seed features' gradients, which
    moves the ill-conditioned BatchNorm shifts of the backbone by a few percent -- hence not compared across
    graphs), and the early flush really happens."""
    import bench
    import pq_transformer as pq
    import sa_fused
    from test_oracle_golden import zero_dropout
    flushed = []
    orig = sa_fused.deferred_wgrads.flush_on

    def spy(self, stream):
        flushed.append(len(self.items))
        return orig(self, stream)

    monkeypatch.setattr(pq, "_WGRAD_SIDE", True)

    def run():
        torch.manual_seed(7)
        net = bench.build_model(0).to(dev()).train()
        zero_dropout(net)
        pc = synth.make_clouds(70, 2, 8192, kind="room").to(dev())
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = bench.loss_of(net({"point_clouds": pc}))
        with sa_fused.deferred_wgrads():
            loss.backward()
        torch.cuda.synchronize()
        return {n: p.grad.float().clone() for n, p in net.named_parameters() if p.grad is not None}

    monkeypatch.setattr(sa_fused.deferred_wgrads, "flush_on", lambda self, stream: None)      # all at the end
    base = run()
    again = run()
    monkeypatch.setattr(sa_fused.deferred_wgrads, "flush_on", spy)
    side = run()
    assert flushed and flushed[0] >= 80                       # the decoder and head stacks were launched early
    assert side.keys() == base.keys()
    noise = max(rel_l2(again[n], base[n]) for n in base)
    worst = max(rel_l2(side[n], base[n]) for n in base)
    assert worst <= max(3.0 * noise, 1e-5), (worst, noise)


@pytest.mark.parametrize("M,N,K,S", [(2048, 256, 128, 64), (8192 + 256, 128, 64, 16), (4096, 288, 96, 32)])
def test_ball_extrema_epilogue_and_pool_select_equal_the_pooling_pass(M, N, K, S):
    """The statistics GEMM's ball extrema + omnipq_sa_pool_select == omnipq_sa_pool on the stored outputs (values,
    bf16 twin, arg-max rows where the result is positive), for positive, negative and zero BatchNorm scales; and
    omnipq_sa_pool_bwd_stats_sel == omnipq_sa_pool_bwd_stats."""
    gen = torch.Generator().manual_seed(M + N + S)
    A = torch.randn((M, K), generator=gen).to(torch.bfloat16).to(dev())
    W = (torch.randn((N, K), generator=gen) / K ** 0.5).to(torch.bfloat16).to(dev())
    a = (0.5 + torch.rand(N, generator=gen)) * torch.where(torch.rand(N, generator=gen) < 0.3, -1.0, 1.0)
    a[:3] = torch.tensor([0.0, 1.0, -1.0])
    a = a.to(dev())
    b = (0.4 * torch.randn(N, generator=gen)).to(dev())
    BM = M // S
    null = ctypes.c_void_p(0)
    capi.lib().omnipq_gemm_nt_stats_workspace_floats.restype = ctypes.c_longlong
    ws = torch.empty(max(int(capi.lib().omnipq_gemm_nt_stats_workspace_floats(M, N)), 1), device=dev())
    Y = torch.empty((M, N), device=dev(), dtype=torch.bfloat16)
    sums = torch.zeros((2, N), device=dev(), dtype=torch.float64)
    ext16 = torch.full((2, BM, N), float("nan"), device=dev(), dtype=torch.bfloat16)
    ext8 = torch.full((2, BM, N), 255, device=dev(), dtype=torch.uint8)
    capi.ok("omnipq_gemm_nt_e16_stats_pool", M, N, K, capi.P(A), K, capi.P(W), K, capi.P(Y), N, null, capi.P(sums),
            capi.P(ws), S, capi.P(ext16[0]), capi.P(ext16[1]), capi.P(ext8[0]), capi.P(ext8[1]))
    Yb = Y.float().view(BM, S, N)
    assert torch.equal(ext16[0].float(), Yb.max(1).values) and torch.equal(ext16[1].float(), Yb.min(1).values)
    first_max = (Yb == Yb.max(1, keepdim=True).values).float().argmax(1)
    assert torch.equal(ext8[0].long(), first_max)
    want32 = torch.empty((BM, N), device=dev())
    want16 = torch.empty((BM, N), device=dev(), dtype=torch.bfloat16)
    want_arg = torch.empty((BM, N), device=dev(), dtype=torch.uint8)
    capi.ok("omnipq_sa_pool", 1, BM, S, N, capi.P(Y), capi.P(a), capi.P(b), capi.P(want32), capi.P(want16), capi.P(want_arg))
    got32, got16 = torch.empty_like(want32), torch.empty_like(want16)
    got_arg, ysel = torch.empty_like(want_arg), torch.empty_like(want16)
    capi.ok("omnipq_sa_pool_select", ctypes.c_longlong(BM), N, capi.P(ext16[0]), capi.P(ext16[1]), capi.P(ext8[0]),
            capi.P(ext8[1]), capi.P(a), capi.P(b), capi.P(got32), capi.P(got16), capi.P(got_arg), capi.P(ysel))
    assert torch.equal(got32, want32) and torch.equal(got16, want16)
    live = (want32 > 0) & (a != 0)[None, :]          # clamped results route no gradient; a == 0 ties every row
    assert torch.equal(got_arg[live], want_arg[live])
    assert bool((got_arg[want32 == 0] == 0).all())
    picked = torch.gather(Yb, 1, got_arg.long().unsqueeze(1)).squeeze(1)
    assert torch.equal(ysel.float()[live], picked[live])
    # backward statistics from the selection
    mean = (0.1 * torch.randn(N, generator=gen)).to(dev())
    invstd = (0.5 + torch.rand(N, generator=gen)).to(dev())
    g = torch.randn((BM, N), generator=gen).to(dev())
    s0 = torch.empty((3, N), device=dev(), dtype=torch.float64)
    s1 = torch.empty((3, N), device=dev(), dtype=torch.float64)
    capi.ok("omnipq_sa_pool_bwd_stats", 1, BM, S, N, capi.P(Y), capi.P(mean), capi.P(invstd), capi.P(g), capi.P(want16),
            capi.P(got_arg), capi.P(s0))
    capi.ok("omnipq_sa_pool_bwd_stats_sel", ctypes.c_longlong(BM), N, capi.P(ysel), capi.P(mean), capi.P(invstd), capi.P(g),
            capi.P(got16), capi.P(s1), 0)
    scale = s0[:2].abs().max(dim=1, keepdim=True).values + 1e-3
    assert float(((s1[:2] - s0[:2]).abs() / scale).max()) < 1e-6


@pytest.mark.parametrize("B,n,m,s", [(8, 2048, 1024, 32), (3, 1024, 2750, 3), (2, 8192, 40000, 1), (2, 1000, 9000, 1),
                                     (2, 5000, 100, 16), (1, 40000, 2048, 64)])
def test_build_csr_groups_every_position_under_its_source_point(B, n, m, s):
    """omnipq_sa_build_csr on all three of its paths (one workgroup per scene with LDS counters; eight workgroups per scene,
    each owning a key range and counting what lies below it; global counters for more than 8192 source points): offsets =
    exclusive prefix of the per-key counts, and `order` lists exactly the positions of every key inside its range (in any
    order), incl. keys nobody references and a key everybody references."""
    gen = torch.Generator().manual_seed(n + m)
    idx = torch.randint(0, n, (B, m, s), generator=gen, dtype=torch.int32)
    idx[0, : m // 2] = 7                                           # a hot key
    idx[-1][idx[-1] == 11] = 12                                    # an unused key
    idx = idx.to(dev())
    offsets = torch.full((B, n + 1), -1, device=dev(), dtype=torch.int32)
    order = torch.full((B, m * s), -1, device=dev(), dtype=torch.int32)
    scratch = torch.empty(B, n, device=dev(), dtype=torch.int32)
    capi.ok("omnipq_sa_build_csr", B, n, m, s, capi.P(idx), capi.P(offsets), capi.P(order), capi.P(scratch))
    flat = idx.view(B, -1).long()
    counts = torch.zeros(B, n, device=dev(), dtype=torch.long).scatter_add_(1, flat, torch.ones_like(flat))
    want = torch.cat([torch.zeros(B, 1, device=dev(), dtype=torch.long), counts.cumsum(1)], 1)
    assert torch.equal(offsets.long(), want)
    # every slot of `order` holds a position whose key owns that slot's range, and every position appears once
    for b in range(B):
        o = order[b].long()
        assert torch.equal(torch.sort(o).values, torch.arange(m * s, device=dev()))
        key_of_slot = torch.searchsorted(want[b, 1:].contiguous(), torch.arange(m * s, device=dev()), right=True)
        assert torch.equal(flat[b][o], key_of_slot)


@pytest.mark.parametrize("group", [8, 16])
@pytest.mark.parametrize("case", ["coordinates_only", "six_extra_channels", "deferred_grouped", "sa2_feature_gradient",
                                  "sa2_batch_4"])
def test_row_plan_equals_the_full_stage(case, group, monkeypatch):
    """sa_fused.ROW_PLAN: the rows of a ball behind its real neighbours hold copies of the ball's first row (ball_query pads with
    the first neighbour); a planned stage keeps whole groups of `group` rows (sa_fused.PLAN_GROUP) up to the last real
    neighbour, packs them into a compact row space every kernel of the stage works on, and accounts for the dropped copies by
    row weights.  The stage must give what the full computation gives -- same pooled arg-max rows, outputs and
    gradients equal up to the order of the f32 sums (statistics: weighted instead of repeated rows) and the bf16 roundings
    that order can flip -- on the backbone's sa1 at the benchmark's per-scene size, with the coordinate-generated first layer,
    with extra input channels (BASELINE configs[3]: no gradient into the raw features), and through the deferred grouped
    weight-gradient launch."""
    import pointnet2_modules
    import sa_fused
    cin = 6 if case == "six_extra_channels" else 0
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[cin, 128, 128, 256], use_xyz=True, normalize_xyz=True)
    B, n = 2, 40000
    if case in ("sa2_feature_gradient", "sa2_batch_4"):
        # the backbone's sa2 (nsample 32: two 16-row groups per ball at most) with a gradient into its input features: the
        # data-gradient GEMM of the first layer and the CSR scatter run on the compact rows too
        cin, B, n = 256, (4 if case == "sa2_batch_4" else 8), 2048         # batch 4: 2^17 grouped rows, the smallest planned stage
        spec = dict(npoint=1024, radius=0.4, nsample=32, mlp=[cin, 256, 256, 512], use_xyz=True, normalize_xyz=True)
    xyz = synth.make_clouds(77, B, n, kind="room").to(dev())
    feats = procedural_tensor("plan.feats", (B, cin, n), torch.float32).to(dev()) if cin else None
    if case in ("sa2_feature_gradient", "sa2_batch_4"):
        feats = (feats * 0.5).requires_grad_(True)
    monkeypatch.setenv("OMNIPQ_SA", "fused")
    monkeypatch.setattr(sa_fused, "KEEP_LAST_PLANS", True)
    monkeypatch.setattr(sa_fused, "PLAN_GROUP", group)
    if case == "sa2_batch_4":
        monkeypatch.setattr(sa_fused, "ONE_SIDED_EXTREMA", False)      # (every other case runs the one-sided extrema)
    res = {}
    for on in (False, True):
        monkeypatch.setattr(sa_fused, "ROW_PLAN", on)
        mod = load_procedural(pointnet2_modules.PointnetSAModuleVotes(
            mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"}), 3).to(dev()).train()
        with torch.no_grad():
            # every third BatchNorm weight negative: the max-pool of those columns selects the ball's MINIMUM
            # (the one-sided extrema of a planned stage must pick that side)
            for name, prm in mod.named_parameters():
                if name.endswith("bn.bn.weight"):
                    prm[::3] *= -1.0
        uses = sa_fused.row_plan_uses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            _, out, inds = mod(xyz, feats)
        assert (sa_fused.row_plan_uses > uses) == on
        g_up = procedural_tensor("plan.g_up", tuple(out.shape), torch.float32).to(dev())
        if feats is not None and feats.requires_grad:
            feats.grad = None
        if case == "deferred_grouped":
            with sa_fused.deferred_wgrads():
                out.backward(g_up)
        else:
            out.backward(g_up)
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
        if feats is not None and feats.requires_grad:
            grads["features"] = feats.grad.detach().clone()
        res[on] = (out.detach().clone(), inds.clone(), grads,
                   {k: b.detach().clone() for k, b in mod.named_buffers() if b.is_floating_point()})
    full, plan = res[False], res[True]
    assert torch.equal(full[1], plan[1])
    e_out = rel_l2(plan[0], full[0])
    print(f"\n{case}: output rel-L2 plan vs full {e_out:.2e}")
    assert e_out < 3e-3, e_out
    for k in full[2]:
        e = rel_l2(plan[2][k], full[2][k])
        print(f"  grad {k:40s} rel-L2 {e:.2e}")
        # two runs of the FULL stage differ by up to ~5e-3 on a weight gradient (order of the f32 sums, flipped bf16 roundings)
        assert e < 2e-2, (k, e)
    for k in full[3]:
        assert rel_l2(plan[3][k], full[3][k]) < 1e-4, k       # running statistics: weighted sums == repeated rows
    # the plan did drop something on this cloud: most balls are far from full
    idx = pointnet2_modules.pointnet2_utils.ball_query(spec["radius"], spec["nsample"], xyz,
                                                       pointnet2_modules.pointnet2_utils.gather_operation(
        xyz.transpose(1, 2).contiguous(), full[1]).transpose(1, 2).contiguous())
    cnt = 1 + (idx[..., 1:] != idx[..., :1]).sum(-1)
    kept = ((cnt + group - 1) // group * group).float().mean() / spec["nsample"]
    print(f"  rows kept: {float(kept):.3f} of the full layout")
    P = cnt.numel() * spec["nsample"]
    assert int(sa_fused.row_plan_last[P].rows_dev.item()) == int(((cnt + group - 1) // group * group).sum())
    assert 0.2 < float(kept) < 0.9


@pytest.mark.parametrize("case", ["sa2_planned", "sa4", "vote_with_coordinate_gradient", "sa3_deferred_grouped"])
def test_first_layer_on_the_source_points_equals_the_grouped_first_layer(case, monkeypatch):
    """sa_fused.HOIST_L1 (round 5): the first conv of a stage with features is linear in the grouped row, so it is computed once
    per SOURCE point and gathered (omnipq_sa_l1_rows), and in backward the rows' gradients are summed per point before the
    weight-gradient / data-gradient contractions.  Must equal the grouped first layer (reference pointnet2_modules.py:243-257
    groups first) up to the order of the f32 sums: same pooled rows' outputs, every parameter gradient, the feature gradient and
    -- for the vote aggregation, whose coordinates are learned -- the coordinate gradients; with a row plan (sa2), without one,
    and through the deferred grouped weight-gradient launch."""
    import pointnet2_modules
    import sa_fused
    spec, B, n, cin = {
        "sa2_planned": (dict(npoint=1024, radius=0.4, nsample=32, mlp=[256, 256, 256, 512]), 8, 2048, 256),
        "sa4": (dict(npoint=256, radius=1.2, nsample=16, mlp=[512, 256, 256, 512]), 8, 512, 512),
        "sa3_deferred_grouped": (dict(npoint=512, radius=0.8, nsample=16, mlp=[512, 256, 256, 512]), 4, 1024, 512),
        "vote_with_coordinate_gradient": (dict(npoint=256, radius=0.3, nsample=16, mlp=[288, 288, 288, 288]), 8, 1024, 288),
    }[case]
    xyz = synth.make_clouds(91, B, n, kind="room").to(dev())
    want_xyz = case == "vote_with_coordinate_gradient"
    feats = (procedural_tensor("hoist.feats", (B, cin, n), torch.float32).to(dev()) * 0.5).requires_grad_(True)
    monkeypatch.setenv("OMNIPQ_SA", "fused")
    res = {}
    for on in (False, True):
        monkeypatch.setattr(sa_fused, "HOIST_L1", on)
        mod = load_procedural(pointnet2_modules.PointnetSAModuleVotes(
            mlp=list(spec["mlp"]), use_xyz=True, normalize_xyz=True, **{k: v for k, v in spec.items() if k != "mlp"}), 3)
        mod = mod.to(dev()).train()
        with torch.no_grad():
            for name, prm in mod.named_parameters():
                if name.endswith("bn.bn.weight"):
                    prm[::3] *= -1.0
        pts = xyz.clone().requires_grad_(want_xyz)
        uses, plans = sa_fused.hoist_uses, sa_fused.row_plan_uses
        with torch.autocast("cuda", dtype=torch.bfloat16):
            new_xyz, out, inds = mod(pts, feats)
        assert (sa_fused.hoist_uses > uses) == on
        assert (sa_fused.row_plan_uses > plans) == (case == "sa2_planned")
        g_up = procedural_tensor("hoist.g_up", tuple(out.shape), torch.float32).to(dev())
        feats.grad = None
        loss_terms = (out.float() * g_up).sum()
        if want_xyz:
            loss_terms = loss_terms + (new_xyz * procedural_tensor("hoist.g_xyz", tuple(new_xyz.shape), torch.float32).to(dev())).sum()
        if case == "sa3_deferred_grouped":
            with sa_fused.deferred_wgrads():
                loss_terms.backward()
        else:
            loss_terms.backward()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
        grads["features"] = feats.grad.detach().clone()
        if want_xyz:
            grads["xyz"] = pts.grad.detach().clone()
        res[on] = (out.detach().clone(), inds.clone(), grads,
                   {k: b.detach().clone() for k, b in mod.named_buffers() if b.is_floating_point()})
    grouped, hoisted = res[False], res[True]
    assert torch.equal(grouped[1], hoisted[1])
    e_out = rel_l2(hoisted[0], grouped[0])
    print(f"\n{case}: output rel-L2 hoisted vs grouped {e_out:.2e}")
    assert e_out < 3e-3, e_out
    assert set(grouped[2]) == set(hoisted[2])
    for k in grouped[2]:
        e = rel_l2(hoisted[2][k], grouped[2][k])
        print(f"  grad {k:40s} rel-L2 {e:.2e}  |g| {float(grouped[2][k].norm()):.3e}")
        assert torch.isfinite(hoisted[2][k]).all(), k
        assert e < 2e-2, (k, e)
    for k in grouped[3]:
        assert rel_l2(hoisted[3][k], grouped[3][k]) < 1e-4, k


@pytest.mark.parametrize("case", ["sa1_coordinates_only", "six_extra_channels", "plan_group_16", "deferred_grouped",
                                  "last_x2_off", "force_collectives", "sa2_feature_gradient", "fp16"])
def test_last_layer_without_dy_equals_the_stored_route(case, monkeypatch):
    """sa_fused.LAST_NO_DY on one stage, on and off from the same state: the route engages exactly when on, the
    forward is the same bits (it only stores less: outputs, pooled indices, running statistics), and every gradient is as close
    to the f32 op-by-op composition (OMNIPQ_SA=composed) as the stored-dY3 route's -- at most 1.25 times its rel-L2 plus one
    e16 rounding.  Cases: sa1 at 2 x 40 000 points, six extra input channels, 16-row plan groups, inside deferred_wgrads, the
    weight gradient on Y2 with the affine (LAST_X2 = False), the SyncBatchNorm branch without a process group
    (_FORCE_COLLECTIVES: gb = NULL, statistics "all-reduced"), sa2 on the route (LAST_NO_DY_MAX_C3 = 1 << 30) with a feature
    gradient, fp16."""
    import pointnet2_modules
    import sa_fused
    dtype = torch.float16 if case == "fp16" else torch.bfloat16
    g_scale = 1024.0 if dtype == torch.float16 else 1.0
    cin = 6 if case == "six_extra_channels" else 0
    spec = dict(npoint=2048, radius=0.2, nsample=64, mlp=[cin, 128, 128, 256], use_xyz=True, normalize_xyz=True)
    B, n, feat_grad = 2, 40000, False
    if case == "sa2_feature_gradient":
        cin, B, n, feat_grad = 256, 8, 2048, True
        spec = dict(npoint=1024, radius=0.4, nsample=32, mlp=[cin, 256, 256, 512], use_xyz=True, normalize_xyz=True)
        monkeypatch.setattr(sa_fused, "LAST_NO_DY_MAX_C3", 1 << 30)
    if case == "plan_group_16":
        monkeypatch.setattr(sa_fused, "PLAN_GROUP", 16)
    if case == "last_x2_off":
        monkeypatch.setattr(sa_fused, "LAST_X2", False)
    if case == "force_collectives":
        monkeypatch.setattr(sa_fused, "_FORCE_COLLECTIVES", True)
    xyz = synth.make_clouds(83, B, n, kind="room").to(dev())
    feats = procedural_tensor("nody.feats", (B, cin, n), torch.float32).to(dev()) * 0.5 if cin else None

    def run(mode):
        mod = load_procedural(pointnet2_modules.PointnetSAModuleVotes(
            mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"}), 3).to(dev()).train()
        with torch.no_grad():
            for name, prm in mod.named_parameters():
                if name.endswith("bn.bn.weight"):
                    prm[::3] *= -1.0
        f = None if feats is None else feats.clone().requires_grad_(feat_grad)
        uses = sa_fused.last_no_dy_uses
        monkeypatch.setenv("OMNIPQ_SA", "composed" if mode == "f32" else "fused")
        monkeypatch.setattr(sa_fused, "LAST_NO_DY", mode == "on")
        with torch.autocast("cuda", dtype=dtype, enabled=mode != "f32"):
            _, out, inds = mod(xyz, f)
        used = sa_fused.last_no_dy_uses - uses
        g_up = procedural_tensor("nody.g_up", tuple(out.shape), torch.float32).to(dev()) * g_scale
        if case == "deferred_grouped" and mode != "f32":
            with sa_fused.deferred_wgrads() as dfr:
                out.backward(g_up)
                assert len(dfr.dz_items) == (1 if mode == "on" else 0)
        else:
            out.backward(g_up)
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in mod.named_parameters()}
        if feat_grad:
            grads["features"] = f.grad.detach().clone()
        return out.detach().clone(), inds.clone(), grads, {k: b.detach().clone() for k, b in mod.named_buffers()}, used

    try:
        want, on, off = run("f32"), run("on"), run("off")
    finally:
        sa_fused.E16.select(torch.bfloat16)
    assert on[4] == 1 and off[4] == 0 and want[4] == 0
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and torch.equal(on[1], want[1])
    for k in off[3]:
        assert torch.equal(on[3][k], off[3][k]), k
    floor = 2.0 ** -9 if dtype == torch.bfloat16 else 2.0 ** -12
    apart_max = 1.2e-2 if dtype == torch.bfloat16 else 1.5e-3     # ~2x the largest measured (5.2e-3 bf16, 7.1e-4 fp16)
    print(f"\n{case}: rel-L2 vs the f32 composition, without dY3 | stored dY3")
    for k in want[2]:
        e_on, e_off, apart = rel_l2(on[2][k], want[2][k]), rel_l2(off[2][k], want[2][k]), rel_l2(on[2][k], off[2][k])
        print(f"  {k:40s} {e_on:.2e} | {e_off:.2e}   (routes apart {apart:.2e})")
        assert e_on <= 1.25 * e_off + floor, (k, e_on, e_off)
        assert apart <= apart_max, (k, apart)
