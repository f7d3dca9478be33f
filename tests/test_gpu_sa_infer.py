"""GPU: the inference set-abstraction stage in one launch (csrc/sa_infer.hip, omnipq_sa_infer) against its float64 reference,
elementwise, inside the bound its arithmetic allows (tests/sa_infer_reference.py: reference, bound, cases; the CPU suite holds
the bound against an emulation and eight mutants) -- through the C ABI on the case table, and through
PointnetSAModuleVotes.forward in eval mode under no_grad and 16-bit autocast, eager and replayed from a captured graph."""
import ctypes
import functools

import pytest
import torch

import capi
import sa_infer_reference as R

pytestmark = pytest.mark.gpu
CANARY = 256                                             # elements behind each output buffer that must stay untouched


def dev():
    return torch.device("cuda:0")


def _lib(dtype):
    lib, ext = capi.lib_of(dtype)
    if lib is None:
        pytest.skip("the IEEE-half library is not built")
    return lib, ext


def _launch(id):
    """the case through omnipq_sa_infer -> (out_f32 [B M][C], out_pm, the two canary tails), on the CPU.  The outputs are
    pre-filled with NaN, the tails behind them with a pattern."""
    case = R.case_of(id)
    lib, ext = _lib(case["dtype"])
    inp, _ = R.case_data(id)
    B, N, M, S = case["shape"]
    cin, dt, L = case["cin"], case["dtype"], len(case["widths"])
    C, kpad = case["widths"][-1], R.kpad_of(case["cin"])
    d = dev()
    xyz, new_xyz, idx = inp["xyz"].to(d), inp["new_xyz"].to(d), inp["idx"].to(d)
    feat = inp["feat"].to(d).contiguous() if cin else None
    keep = []
    recs = (ext.sa_infer_layer_struct() * L)()
    for rec, lay in zip(recs, inp["layers"]):
        t = [lay["W"].to(d).contiguous()] + [lay[k].to(d).contiguous() for k in ("gamma", "beta", "mean", "var")]
        keep.append(t)
        rec.W, rec.ldw, rec.C = t[0].data_ptr(), t[0].shape[1], t[0].shape[0]
        rec.gamma, rec.beta, rec.running_mean, rec.running_var = (v.data_ptr() for v in t[1:])
        rec.eps = lay["eps"]
    n = B * M * C
    buf32 = torch.full((n + CANARY,), float("nan"), device=d, dtype=torch.float32)
    buf16 = torch.full((n + CANARY,), float("nan"), device=d, dtype=dt)
    buf32[n:] = 12345.0
    buf16[n:] = 77.0
    rc = lib.omnipq_sa_infer(B, N, M, S, cin, kpad, inp["inv_radius"], capi.P(xyz), capi.P(new_xyz), capi.P(idx), capi.P(feat),
                             L, ctypes.byref(recs), capi.P(buf32), capi.P(buf16), capi.stream())
    assert rc == 0, (id, rc)
    torch.cuda.synchronize()
    return buf32[:n].view(B * M, C).cpu(), buf16[:n].view(B * M, C).cpu(), buf32[n:].cpu(), buf16[n:].cpu()


@functools.lru_cache(maxsize=None)
def _first_run(id):
    return _launch(id)


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_outputs_are_within_the_elementwise_bounds_of_the_float64_reference(id):
    _, ref = R.case_data(id)
    out_f32, out_pm, _, _ = _first_run(id)
    rat = R.ratios(out_f32, out_pm, ref)
    print(id, R.fmt(rat))
    assert not R.outside(rat), rat


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_sixteen_bit_twin_is_the_rounded_f32_output(id):
    out_f32, out_pm, _, _ = _first_run(id)
    dt = R.case_of(id)["dtype"]
    assert out_pm.dtype == dt and torch.equal(out_pm.view(torch.int16), out_f32.to(dt).view(torch.int16))


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_every_output_element_is_written_and_nothing_behind_them(id):
    out_f32, out_pm, tail32, tail16 = _first_run(id)
    assert bool(torch.isfinite(out_f32).all()) and bool(torch.isfinite(out_pm.float()).all())
    assert bool((tail32 == 12345.0).all()) and bool((tail16.float() == 77.0).all())


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_two_runs_are_bit_equal(id):
    a32, a16, _, _ = _first_run(id)
    b32, b16, _, _ = _launch(id)
    assert torch.equal(a32.view(torch.int32), b32.view(torch.int32)) and torch.equal(a16.view(torch.int16), b16.view(torch.int16))


# ---- through the module -----------------------------------------------------------------------------------------------------

MODULE_SPECS = {
    # sa1-like: no input features
    "sa1_like": (dict(npoint=64, radius=0.3, nsample=64, mlp=[0, 64, 64, 128], use_xyz=True, normalize_xyz=True), 2048, 0),
    # sa2-like: features, 32 neighbours
    "sa2_like": (dict(npoint=48, radius=0.4, nsample=32, mlp=[128, 128, 128, 256], use_xyz=True, normalize_xyz=True), 1024, 128),
    # vote-aggregation-like: 288 channels, 16 neighbours, a partial last tile (82 balls of 16 rows)
    "vote_like": (dict(npoint=41, radius=0.5, nsample=16, mlp=[288, 288, 288, 288], use_xyz=True, normalize_xyz=True), 512, 288),
    # two layers, coordinates not normalised
    "two_layers": (dict(npoint=32, radius=0.6, nsample=16, mlp=[16, 32, 64], use_xyz=True, normalize_xyz=False), 512, 16),
}


def _module(spec, seed=3):
    import pointnet2_modules
    from procedural import load_procedural
    mod = pointnet2_modules.PointnetSAModuleVotes(mlp=list(spec["mlp"]), **{k: v for k, v in spec.items() if k != "mlp"})
    return load_procedural(mod, seed).to(dev())


def _cloud(seed, n, cin, B=2):
    import synth
    from procedural import procedural_tensor
    xyz = synth.make_clouds(seed, B, n, kind="room").to(dev())
    feats = procedural_tensor(f"sa_infer.feats.{seed}", (B, cin, n), torch.float32).to(dev()) if cin else None
    return xyz, feats


def _module_reference(mod, spec, xyz, feats, new_xyz, dtype):
    """the float64 reference and bounds from the module's own parameters and the operands its forward reads: the ball query's
    indices, the features as position-major e16, the weights as omnipq_prep_weight leaves them (columns [features | xyz | 0])"""
    import pointnet2_utils
    B, N, _ = xyz.shape
    cin = 0 if feats is None else feats.shape[1]
    assert cin % 8 == 0
    kpad = R.kpad_of(cin)
    idx = pointnet2_utils.ball_query(spec["radius"], spec["nsample"], xyz, new_xyz.contiguous())
    layers = []
    for l, layer in enumerate(mod.mlp_module):
        conv, bn = layer.conv, layer.bn.bn
        W = conv.weight.detach().reshape(conv.out_channels, -1).float().cpu()
        if l == 0:
            Wp = torch.zeros((W.shape[0], kpad))
            Wp[:, :cin], Wp[:, cin:cin + 3] = W[:, 3:], W[:, :3]
            W = Wp
        layers.append(dict(W=W.to(dtype), gamma=bn.weight.detach().float().cpu(), beta=bn.bias.detach().float().cpu(),
                           mean=bn.running_mean.float().cpu(), var=bn.running_var.float().cpu(), eps=float(bn.eps)))
    inp = dict(xyz=xyz.cpu(), new_xyz=new_xyz.cpu(), idx=idx.cpu(), inv_radius=(1.0 / spec["radius"]) if spec["normalize_xyz"] else 1.0,
               feat=None if feats is None else feats.transpose(1, 2).to(dtype).cpu().contiguous(), layers=layers)
    return R.reference(inp, (B, N, spec["npoint"], spec["nsample"]), cin, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.lib_name)
@pytest.mark.parametrize("name", sorted(MODULE_SPECS))
def test_module_in_eval_under_no_grad_runs_the_chain_within_the_bound(name, dtype, monkeypatch):
    import sa_fused
    _lib(dtype)
    monkeypatch.delenv("OMNIPQ_SA", raising=False)
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", True)
    spec, n, cin = MODULE_SPECS[name]
    mod = _module(spec).eval()
    xyz, feats = _cloud(71, n, cin)
    before = sa_fused.eval_chain_uses
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        new_xyz, out, _ = mod(xyz, feats)
    assert sa_fused.eval_chain_uses == before + 1                   # the path under test is the one that ran
    B, C, M = out.shape
    assert out.dtype == torch.float32 and (B, M) == (2, spec["npoint"]) and C == spec["mlp"][-1]
    twin = out.omnipq_rows16
    assert twin.dtype == dtype and tuple(twin.shape) == (B, M, C)
    ref = _module_reference(mod, spec, xyz, feats, new_xyz, dtype)
    rat = R.ratios(out.transpose(1, 2).reshape(B * M, C).cpu(), twin.reshape(B * M, C).cpu(), ref)
    print(name, R.lib_name(dtype), R.fmt(rat))
    assert not R.outside(rat), rat
    # the stored route computes the same function (two roundings per hidden activation: compared in norm, not by the bound)
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", False)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        _, stored, _ = mod(xyz, feats)
    assert sa_fused.eval_chain_uses == before + 1
    err = float((stored.double() - out.double()).norm()) / float(out.double().norm())
    assert err < 2e-2, err


def test_training_and_grad_enabled_forwards_do_not_take_the_chain(monkeypatch):
    import sa_fused
    monkeypatch.delenv("OMNIPQ_SA", raising=False)
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", True)
    spec, n, cin = MODULE_SPECS["sa2_like"]
    mod = _module(spec)
    xyz, feats = _cloud(72, n, cin)
    before = sa_fused.eval_chain_uses
    with torch.autocast("cuda", dtype=torch.bfloat16):
        mod.train()
        mod(xyz, feats)                                  # training
        with torch.no_grad():
            mod(xyz, feats)                              # training-mode BatchNorm under no_grad: batch statistics
        mod.eval()
        _, out, _ = mod(xyz, feats)                      # eval with grad enabled: the composed path
    assert out.requires_grad and sa_fused.eval_chain_uses == before


def test_captured_eval_forward_replays_bit_equal_on_a_second_cloud(monkeypatch):
    """torch.cuda.graph capture of the module's eval forward (one stream, no parallel branch); after the input buffers are
    refilled with a second cloud the replay equals the eager forward on that cloud, bit for bit"""
    import sa_fused
    monkeypatch.delenv("OMNIPQ_SA", raising=False)
    monkeypatch.setattr(sa_fused, "EVAL_CHAIN", True)
    spec, n, cin = MODULE_SPECS["sa2_like"]
    mod = _module(spec).eval()
    xyz1, feats1 = _cloud(73, n, cin)
    xyz2, feats2 = _cloud(74, n, cin)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        _, want, _ = mod(xyz2, feats2)
        want, want16 = want.clone(), want.omnipq_rows16.clone()
        sx, sf = xyz1.clone(), feats1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod(sx, sf)                                  # warm-up: every allocation the forward makes outside a capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        sa_fused.reset_pools()
        before = sa_fused.eval_chain_uses
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, got, _ = mod(sx, sf)
            got16 = got.omnipq_rows16
        assert sa_fused.eval_chain_uses == before + 1
    sx.copy_(xyz2)
    sf.copy_(feats2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(got16.view(torch.int16), want16.view(torch.int16))
