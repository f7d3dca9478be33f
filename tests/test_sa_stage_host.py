"""CPU only: the explicit arguments of the fused SA stage (pointnet2/sa_fused.py) -- `stage_call()`, the record run() hands to
FusedSAStage.apply, and `Finalize.tail()`, the argument run the finalising entry points share."""
import ctypes

import torch

import capi


def _module(**kw):
    import pointnet2_modules
    return pointnet2_modules.PointnetSAModuleVotes(mlp=[0, 32, 64], npoint=128, radius=0.4, nsample=16, **kw)


def test_stage_call_label_is_the_modules_name_or_its_geometry(built_lib):
    import sa_fused
    mod = _module()
    assert sa_fused.stage_call(mod, True).label == "m128s16"
    mod.omnipq_stage = "sa3"
    assert sa_fused.stage_call(mod, True).label == "sa3"


def test_stage_call_syncs_only_when_every_layer_is_a_syncbatchnorm_on_the_default_group(built_lib):
    import sa_fused
    assert sa_fused.stage_call(_module(), True).sync is False
    mod = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_module())
    assert sa_fused.stage_call(mod, True).sync is True
    mod.mlp_module[1].bn.bn = torch.nn.BatchNorm2d(64)                 # one plain layer: per-rank statistics for the stage
    assert sa_fused.stage_call(mod, True).sync is False
    mod = torch.nn.SyncBatchNorm.convert_sync_batchnorm(_module())
    mod.mlp_module[0].bn.bn.process_group = object()                    # a group of its own: not the kernels' collective
    assert sa_fused.stage_call(mod, True).sync is False


def test_stage_call_carries_the_arguments_and_the_modules_own_buffers(built_lib):
    import sa_fused
    mod = _module(normalize_xyz=True).eval()
    plan, csr = object(), object()
    call = sa_fused.stage_call(mod, False, plan, csr)
    assert (call.no_grad, call.training, call.radius, call.normalize_xyz) == (True, False, 0.4, True)
    assert call.plan is plan and call.csr is csr and sa_fused.stage_call(mod, True).no_grad is False
    assert sa_fused.stage_call(mod, True)[-2:] == (None, None)
    assert len(call.bn) == 2
    for rec, layer in zip(call.bn, mod.mlp_module):
        bn = layer.bn.bn
        assert rec.running_mean is bn.running_mean and rec.running_var is bn.running_var
        assert rec.num_batches_tracked is bn.num_batches_tracked
        assert (rec.momentum, rec.eps) == (bn.momentum, bn.eps)


class _Calls:
    def __init__(self):
        self.seen = []

    def __call__(self, fn, anchor, *args):
        self.seen.append((fn.__name__, args))


EPS, MOMENTUM = 0.125, 0.375           # numbers no other argument of the calls below has


def _finalising_calls(sa_fused, monkeypatch):
    """every call site that spends a Finalize, once, on CPU tensors -> [(entry point, its arguments)]"""
    rec = _Calls()
    monkeypatch.setattr(sa_fused, "_call", rec)
    C, P = 32, 64
    vec = lambda: torch.zeros(C)

    def layer():
        lay = sa_fused._Layer()
        lay.C, lay.K, lay.X, lay.fin = C, C, None, None
        lay.Y = torch.zeros(P, C, dtype=torch.bfloat16)
        lay.Wp = torch.zeros(C, 32, dtype=torch.bfloat16)
        sums = torch.zeros(2, C, dtype=torch.float64)
        bn = sa_fused.StageBN(vec(), vec(), None, MOMENTUM, EPS)
        lay.fin = sa_fused.batch_constants(lay, sums, float(P), vec(), vec(), bn)
        return lay

    W = torch.zeros(C, C, dtype=torch.bfloat16)
    ext = sa_fused.BallExtrema(8, *(torch.zeros(P // 8, C) for _ in range(4)))
    sa_fused.gemm_nt_affine(layer().Y, layer(), W, P, C, C, sums=torch.zeros(2, C, dtype=torch.float64))
    sa_fused.gemm_nt_affine(layer().Y, layer(), W, P, C, C, sums=torch.zeros(2, C, dtype=torch.float64), pool=ext)
    sa_fused.gemm_nt_xyz(torch.zeros(P, 8, dtype=torch.bfloat16), layer(), W, P, C, C, torch.zeros(2, C, dtype=torch.float64))
    route = sa_fused.StageRoute(True, "grouped", 0, False, (), ("pool",), "both", "ysel", False)
    sa_fused._pool_forward(route, sa_fused._Geom(1, 8, P // 8, 8, P, 0, 0, 32, 1.0, 1), layer(), ext, torch.device("cpu"))
    for relu in (False, True):
        lay = layer()
        sa_fused.finalize_launch(lay, P, lay.fin, relu)
    return rec.seen


def test_finalize_tail_lands_on_pointer_pointer_float_float_pointer_pointer_at_every_call_site(built_lib, monkeypatch):
    import sa_fused
    reported = capi.reported_signatures(ctypes.CDLL(built_lib))
    seen = _finalising_calls(sa_fused, monkeypatch)
    assert [name for name, _ in seen] == [
        "omnipq_gemm_nt_e16_bnaffine", "omnipq_gemm_nt_e16_bnaffine_pool", "omnipq_gemm_nt_e16_xyz_bnaffine",
        "omnipq_sa_pool_select_finalize", "omnipq_bn_finalize", "omnipq_bn_finalize_relu"]
    for name, args in seen:
        letters = reported[name][1]
        at = [i for i, a in enumerate(args) if isinstance(a, float) and a == EPS]
        assert len(at) == 1 and args[at[0] + 1] == MOMENTUM, name
        first = at[0] - 2                                                   # gamma, beta, eps, momentum, running mean, running var
        assert letters[first:first + 6] == "ppffpp", (name, letters)
        assert all(isinstance(args[first + k], ctypes.c_void_p) and args[first + k].value for k in (0, 1, 4, 5)), name
        # the head is the call site's: totals then count in front of the GEMM prologues and the pool, count then totals else
        head = letters[first - 2:first]
        assert head == ("dp" if name.startswith("omnipq_bn_finalize") else "pd"), (name, head)
        assert isinstance(args[first - 2 if head == "dp" else first - 1], float)

