"""GPU: an inference per-point stack in one launch (csrc/rows_infer.hip, omnipq_rows_infer) against its float64 reference,
elementwise, inside the bound its arithmetic allows (tests/rows_infer_reference.py: reference, bound, cases; the CPU suite
holds the bound against an emulation and its mutants) -- through the C ABI on the case table, and through the model's modules
in eval mode under no_grad and 16-bit autocast, eager and replayed from a captured graph."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import capi
import rows_infer_reference as R

pytestmark = pytest.mark.gpu
CANARY = 256                                             # elements behind the output buffer that must stay untouched


def dev():
    return torch.device("cuda:0")


def _lib(dtype):
    lib, ext = capi.lib_of(dtype)
    if lib is None:
        pytest.skip("the IEEE-half library is not built")
    return lib, ext


@functools.lru_cache(maxsize=None)
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _data(id):
    return R.case_data(id, _cus())


def _records(ext, layers, d):
    """-> (the host records of `layers` (rows_infer_reference's dicts), the device tensors they point to)"""
    recs = (ext.rows_infer_layer_struct() * len(layers))()
    keep = []
    for rec, lay in zip(recs, layers):
        t = {k: lay[k].to(d).contiguous() for k in ("W", "bias", "gamma", "beta", "mean", "var") if lay[k] is not None}
        keep.append(t)
        rec.W, rec.ldw, rec.C = t["W"].data_ptr(), t["W"].shape[1], t["W"].shape[0]
        rec.bias = t["bias"].data_ptr() if "bias" in t else 0
        if "gamma" in t:
            rec.gamma, rec.beta, rec.running_mean, rec.running_var = (t[k].data_ptr() for k in ("gamma", "beta", "mean", "var"))
        rec.eps, rec.relu = lay["eps"], int(lay["relu"] and "gamma" not in t)
    return recs, keep


def _launch(id):
    """the case through omnipq_rows_infer -> (out [n][C_last padded], the canary tail), on the CPU.  The output is pre-filled
    with NaN, the tail behind it with a pattern."""
    case = R.case_of(id)
    lib, ext = _lib(case["dtype"])
    inp, ref = _data(id)
    n, Cp = ref["out"].shape
    d = dev()
    x = inp["x"].to(d).contiguous()
    recs, keep = _records(ext, inp["layers"], d)
    buf = torch.full((n * Cp + CANARY,), float("nan"), device=d, dtype=case["dtype"])
    buf[n * Cp:] = 77.0
    rc = lib.omnipq_rows_infer(n, case["cin"], case["ldx"], capi.P(x), int(x.dtype == torch.float32), len(recs),
                               ctypes.byref(recs), capi.P(buf), capi.stream())
    assert rc == 0, (id, rc)
    torch.cuda.synchronize()
    return buf[:n * Cp].view(n, Cp).cpu(), buf[n * Cp:].cpu()


@functools.lru_cache(maxsize=None)
def _first_run(id):
    return _launch(id)


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_output_is_within_the_elementwise_bound_of_the_float64_reference(id):
    _, ref = _data(id)
    out, _ = _first_run(id)
    rat = R.ratios(out, ref)
    print(id, R.fmt(rat))
    assert not R.outside(rat), rat


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_padded_columns_are_exact_zeros(id):
    out, _ = _first_run(id)
    C = R.case_of(id)["layers"][-1][0]
    assert bool((out[:, C:].view(torch.int16) == 0).all())


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_every_output_element_is_written_and_nothing_behind_them(id):
    out, tail = _first_run(id)
    assert bool(torch.isfinite(out.float()).all())
    assert bool((tail.float() == 77.0).all())


@pytest.mark.parametrize("id", R.CASE_IDS)
def test_two_runs_are_bit_equal(id):
    a, _ = _first_run(id)
    b, _ = _launch(id)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.lib_name)
def test_lds_bytes_and_the_call_agree_on_every_case(dtype):
    """what omnipq_rows_infer_lds_bytes says of a shape is what the call does with it (1024 -> 512 -> 512 included: taken,
    on the 32-row tile), and it is the header's sum"""
    lib, _ = _lib(dtype)
    for case in R.CASES:
        if case["dtype"] is not dtype:
            continue
        widths = R.widths_of(case)
        got = int(lib.omnipq_rows_infer_lds_bytes(R.kpad_of(case), len(widths), (ctypes.c_int * len(widths))(*widths)))
        assert got == R.lds_bytes(R.kpad_of(case), widths)[0] and got > 0, case["id"]
        _first_run(case["id"])                            # asserts rc == 0


# ---- through the modules ----------------------------------------------------------------------------------------------------

class _Spy:
    """records what rows_mlp._infer was given and what it returned (calls), and what every rows_mlp.run returned (ran)"""

    def __init__(self, rows_mlp, monkeypatch):
        self.calls, self.ran, real, real_run = [], [], rows_mlp._infer, rows_mlp.run

        def infer(x, layers, route, padded):
            y = real(x, layers, route, padded)
            self.calls.append((x, layers, y))
            return y

        def run(*args, **kw):
            y = real_run(*args, **kw)
            self.ran.append(y)
            return y

        monkeypatch.setattr(rows_mlp, "_infer", infer)
        monkeypatch.setattr(rows_mlp, "run", run)


def _stack_reference(x, layers, dtype):
    """the float64 reference and bound of a rows_mlp stack from the module's own parameters and the rows its forward reads; the
    weights as omnipq_prep_weight leaves them (e16, zero rows up to the padded width, zero columns behind the contraction)"""
    cin = x.shape[1]
    K, recs = R.round_up(cin, 32), []
    for lay in layers:
        W2 = lay.weight.detach().reshape(lay.weight.shape[0], -1).float().cpu()
        C, Cp = W2.shape[0], R.round_up(W2.shape[0], 32)
        W = torch.zeros((Cp, K))
        W[:C, :W2.shape[1]] = W2
        bias = None
        if lay.bias is not None:
            bias = torch.zeros(Cp)
            bias[:C] = lay.bias.detach().float().cpu()[:C]
        rec = dict(W=W.to(dtype), bias=bias, gamma=None, beta=None, mean=None, var=None, eps=0.0,
                   relu=lay.bn is not None or lay.relu_dropout is not None)
        if lay.bn is not None:
            bn = lay.bn
            rec.update(gamma=bn.weight.detach().float().cpu(), beta=bn.bias.detach().float().cpu(),
                       mean=bn.running_mean.float().cpu(), var=bn.running_var.float().cpu(), eps=float(bn.eps))
        recs.append(rec)
        K = Cp
    return R.reference(dict(x=x.detach().cpu(), layers=recs), cin, dtype)


def _loaded(mod, seed=5):
    from procedural import load_procedural
    return load_procedural(mod, seed).to(dev())


def _tensor(name, shape):
    from procedural import procedural_tensor
    return procedural_tensor(f"rows_infer.{name}", shape, torch.float32).to(dev())


def _voting():
    import voting_module
    mod = _loaded(voting_module.VotingModule(1, 288))
    return mod, lambda s: mod(_tensor(f"vote.xyz{s}", (2, 75, 3)), _tensor(f"vote.feat{s}", (2, 288, 75)))


def _head():
    import pq_transformer as pq
    mod = _loaded(pq.PredictHead(288, 1, 18, 18, (np.arange(54, dtype=np.float32).reshape(18, 3) % 5 + 0.5)))
    return mod, lambda s: mod(_tensor(f"head.net{s}", (2, 288, 65)), _tensor(f"head.base{s}", (2, 65, 3)), {}, "x_")[2]


def _posembed():
    import pq_transformer as pq
    mod = _loaded(pq.PositionEmbeddingLearned(3, 288))
    return mod, lambda s: mod(_tensor(f"pos.xyz{s}", (2, 77, 3)))


def _fp():
    import pointnet2_modules
    mod = _loaded(pointnet2_modules.PointnetFPModule(mlp=[256 + 128, 256, 96 + 32]))
    return mod, lambda s: mod(_tensor(f"fp.unknown{s}", (2, 100, 3)), _tensor(f"fp.known{s}", (2, 40, 3)),
                              _tensor(f"fp.uf{s}", (2, 128, 100)), _tensor(f"fp.kf{s}", (2, 256, 40)))


MODULES = {"voting": _voting, "head": _head, "posembed": _posembed, "fp": _fp}


def _heads_opt_in(monkeypatch, on=True):
    """the prediction heads' stacks opt into the chain through pred_heads._HEAD_EVAL_CHAIN (shipped off: an existing test
    pins the eval forward's head stacks as pair launches)"""
    import pred_heads
    monkeypatch.setattr(pred_heads, "_HEAD_EVAL_CHAIN", on)


def _flat(out):
    """every tensor of a module's output, in a fixed order"""
    if torch.is_tensor(out):
        return [out]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    return [t for o in out for t in _flat(o)]


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.lib_name)
@pytest.mark.parametrize("name", sorted(MODULES))
def test_module_in_eval_under_no_grad_runs_the_chain_within_the_bound(name, dtype, monkeypatch):
    import rows_mlp
    _lib(dtype)
    monkeypatch.delenv("OMNIPQ_ROWS", raising=False)
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", True)
    _heads_opt_in(monkeypatch)
    spy = _Spy(rows_mlp, monkeypatch)
    mod, forward = MODULES[name]()
    mod.eval()
    before = rows_mlp.eval_chain_uses
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        out = _flat(forward(1))
    assert rows_mlp.eval_chain_uses == before + 1 and len(spy.calls) == 1          # the path under test is the one that ran
    x, layers, y = spy.calls[0]
    assert y.dtype == dtype
    ref = _stack_reference(x, layers, dtype)
    C = y.shape[1]
    rat = R.ratios(y.cpu(), dict(out=ref["out"][:, :C], bound=ref["bound"][:, :C]))
    print(name, R.lib_name(dtype), R.fmt(rat))
    assert not R.outside(rat), rat
    # The stored route computes the same function with one more rounding per hidden layer: z goes through e16 before the
    # affine, where the cancellation in a z + b (|a z| / |y|, of order ten for a BatchNorm that normalises) amplifies its u.
    # The stacks' own outputs are compared in norm against 32 u -- two such roundings with that amplification; a wrong slice,
    # layer order or bias is of order one.  Not the bound: that is held above.  What the module makes of the rows (an argmax
    # among them may fall the other way) is compared in shape and type.
    tol = 32 * R.unit_roundoff(dtype)
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", False)
    with torch.no_grad(), torch.autocast("cuda", dtype=dtype):
        stored = _flat(forward(1))
    assert rows_mlp.eval_chain_uses == before + 1 and len(out) == len(stored) and len(spy.ran) == 2
    assert all(a.shape == b.shape and a.dtype == b.dtype for a, b in zip(out, stored))
    ya, yb = spy.ran
    assert ya.shape == yb.shape and ya.dtype == yb.dtype and ya.data_ptr() == y.data_ptr()
    err = float((ya.double() - yb.double()).norm()) / float(yb.double().norm())
    print(name, R.lib_name(dtype), "chain against stored, in norm:", err)
    assert err < tol, (err, tol)


@pytest.mark.parametrize("name", sorted(MODULES))
def test_training_and_grad_enabled_forwards_do_not_take_the_chain_and_keep_their_bits(name, monkeypatch):
    import rows_mlp
    monkeypatch.delenv("OMNIPQ_ROWS", raising=False)
    _heads_opt_in(monkeypatch)
    mod, forward = MODULES[name]()
    state = {k: v.clone() for k, v in mod.state_dict().items()}
    before = rows_mlp.eval_chain_uses
    outs = {}
    for flag in (True, False):
        monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", flag)
        mod.load_state_dict(state)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            mod.train()
            a = _flat(forward(1))                        # training
            with torch.no_grad():
                b = _flat(forward(1))                    # training-mode BatchNorm under no_grad: batch statistics
            mod.eval()
            c = _flat(forward(1))                        # eval with grad enabled: the composed path
        outs[flag] = [t.detach().clone() for t in a + b + c]
    assert rows_mlp.eval_chain_uses == before
    assert len(outs[True]) == len(outs[False])
    for a, b in zip(outs[True], outs[False]):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_captured_eval_stack_replays_bit_equal_on_a_second_input(monkeypatch):
    """torch.cuda.graph capture of a position embedding's eval forward (one stream, no parallel branch); after the input
    buffer is refilled the replay equals the eager forward on that input, bit for bit"""
    import rows_mlp
    import sa_fused
    monkeypatch.delenv("OMNIPQ_ROWS", raising=False)
    monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", True)
    mod, _ = _posembed()
    mod.eval()
    x1, x2 = _tensor("graph.xyz1", (2, 77, 3)), _tensor("graph.xyz2", (2, 77, 3))
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        want = mod(x2).clone()
        sx = x1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            mod(sx)                                      # warm-up: every allocation the forward makes outside a capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        sa_fused.reset_pools()
        before = rows_mlp.eval_chain_uses
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = mod(sx)
        assert rows_mlp.eval_chain_uses == before + 1
    sx.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("heads", [False, True], ids=["heads-stored", "heads-on-the-chain"])
def test_model_eval_forward_takes_the_chain_for_every_stack_the_route_sends_there(heads, monkeypatch):
    """PQ_Transformer at its smallest configuration, eval / no_grad / bf16: every end_points entry of the stored forward is
    there, finite where that one is, and eval_chain_uses moved by the number of stacks stack_route sent to the chain -- 15
    as shipped (twelve position embeddings, the voting module, two FP modules), 14 more with the heads opted in"""
    import rows_mlp
    from pq_transformer import PQ_Transformer
    monkeypatch.delenv("OMNIPQ_ROWS", raising=False)
    _heads_opt_in(monkeypatch, heads)
    torch.manual_seed(0)
    means = (np.arange(54, dtype=np.float32).reshape(18, 3) % 5 + 0.5)
    net = PQ_Transformer(input_feature_dim=1, num_class=18, num_proposal=256, num_quad_proposal=256, num_heading_bin=1,
                         num_size_cluster=18, mean_size_arr=means).to(dev()).eval()
    import synth
    cloud = synth.make_clouds(81, 1, 4096, kind="room").to(dev())
    cloud = torch.cat([cloud[..., :3], cloud[..., 2:3]], dim=2).contiguous()
    sent, real = [], rows_mlp._chain_route

    def counting(x, layers, training):
        route = real(x, layers, training)
        sent.append(route is not None)
        return route

    monkeypatch.setattr(rows_mlp, "_chain_route", counting)
    eps, counts = {}, {}
    for flag in (False, True):
        monkeypatch.setattr(rows_mlp, "EVAL_CHAIN", flag)
        before, n0 = rows_mlp.eval_chain_uses, len(sent)
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            eps[flag] = net({"point_clouds": cloud})
        torch.cuda.synchronize()
        uses = rows_mlp.eval_chain_uses - before
        assert uses == sum(sent[n0:])
        assert (uses > 0) == flag
        counts[flag] = uses
    print("stacks on the chain:", counts[True])
    assert counts[True] == (29 if heads else 15)
    assert sorted(eps[True]) == sorted(eps[False])
    for k, v in eps[False].items():
        if torch.is_tensor(v):
            w = eps[True][k]
            assert w.shape == v.shape and w.dtype == v.dtype, k
            if v.is_floating_point() and bool(torch.isfinite(v.float()).all()):
                assert bool(torch.isfinite(w.float()).all()), k
