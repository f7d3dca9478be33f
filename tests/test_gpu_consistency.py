"""The mean-teacher consistency loss on the HIP kernels (omni-pq_amd/models/utils/mean_teacher_consistency_util.py ->
csrc/consistency.hip, include/omnipq_semi.h) against (1) the outputs of the REFERENCE (tests/golden/consistency.npz) and (2)
the float64 restatement (tests/mt_restatement.py): terms, gradients, and every discrete decision exactly; the edge cases;
forward + backward inside a hipGraph; the criterion of a CapturedStep with a teacher.  Tolerances and the margins that make
the exact comparisons meaningful: tests/test_consistency_golden.py."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (sys.path set-up)
import mt_inputs
import mt_restatement as R
from test_consistency_golden import (CASES, GRAD_NAMES, INPUTS, NOISE_MAX, WEIGHTS, assignments, check_grads, check_terms, gold,
                                     inputs, restated)

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:reduction")]
P = len(mt_inputs.PREFIXES)


def hip():
    from models.utils import mean_teacher_consistency_util
    return mean_teacher_consistency_util


def to_device(S_np, T_np, dtype=None):
    """-> (student end_points on the GPU, its differentiable tensors as leaves; teacher end_points)"""
    def put(v):
        t = torch.from_numpy(v.copy()).cuda()
        return t.to(dtype) if dtype is not None and t.is_floating_point() else t

    S = {k: put(v) for k, v in S_np.items()}
    for k in GRAD_NAMES:
        S[k].requires_grad_(True)
    return S, {k: put(v) for k, v in T_np.items()}


def run_device(S_np, T_np, mean_size, dtype=None):
    """-> (terms as floats, {leaf: gradient array}, the end_points after the call); the inputs must come back bit-unchanged"""
    S, T = to_device(S_np, T_np, dtype)
    before = {("S", k): v.detach().clone() for k, v in S.items()}
    before.update({("T", k): v.detach().clone() for k, v in T.items()})
    total, ep = hip().get_consistency_loss(S, T, mt_inputs.Config(mean_size.shape[0]))
    assert ep is S
    terms = [ep[k] for k in hip().TERM_KEYS] + [total]
    assert all(t.dim() == 0 and t.dtype == torch.float32 and t.is_cuda for t in terms)
    sum(w * t for w, t in zip(WEIGHTS, terms)).backward()
    for (side, k), v in before.items():
        assert torch.equal((S if side == "S" else T)[k].detach(), v), f"{side} {k} was modified"
    assert all(S[p + k].grad is None for p in mt_inputs.PREFIXES for k in mt_inputs.NO_GRAD_KEYS)
    grads = {k: S[k].grad.float().cpu().numpy() for k in GRAD_NAMES}
    assert all(S[k].grad.dtype == S[k].dtype for k in GRAD_NAMES)
    return [float(t.detach()) for t in terms], grads, ep


def device_decisions(S_np, T_np, mean_size):
    S, T = to_device(S_np, T_np)
    return {k: v.cpu().numpy() for k, v in hip().decisions(S, T, mt_inputs.Config(mean_size.shape[0])).items()}


def check_decisions(got, want, n, what):
    """every nearest neighbour, arg-max class and mask bit equal to the restatement's; each mask keeps floor(0.85 (n - 1)) + 1"""
    kept = int(np.floor(0.85 * (n - 1))) + 1
    for i, p in enumerate(mt_inputs.PREFIXES):
        for kind in (0, 1):
            w = want[(p, kind)]
            assert np.array_equal(got["ind1"][i, kind], w["ind1"].numpy()), (what, p, kind, "ind1")
            assert np.array_equal(got["ind2"][i, kind], w["ind2"].numpy()), (what, p, kind, "ind2")
            for j, mask in enumerate(w["masks"]):
                assert np.array_equal(got["masks"][i, kind, j].astype(bool), mask.numpy()), (what, p, kind, "mask", j)
                assert int(got["masks"][i, kind, j].sum()) == kept, (what, p, kind, j)
        assert np.array_equal(got["cls"][i, 0], want[(p, 0)]["cls_s"].numpy()), (what, p, "student's size class")
        assert np.array_equal(got["cls"][i, 1], want[(p, 0)]["cls_t"].numpy()), (what, p, "teacher's size class")
        assert not got["masks"][i, 0, 2].any()


def check_outputs(ep, outputs, what):
    for k, want in outputs.items():
        got = ep[k].detach().cpu().numpy()
        assert got.shape == want.shape, (what, k)
        if k.endswith("ema_assignment") or k.endswith("ema_assignment_quad"):
            assert ep[k].dtype == torch.int64 and np.array_equal(got, want), (what, k)
        else:
            assert ep[k].dtype == torch.float32 and not ep[k].requires_grad
            assert np.abs(got - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0), (what, k)


@pytest.mark.parametrize("name", list(INPUTS))
def test_loss_reproduces_the_restatement_and_the_reference_fixture(name):
    S_np, T_np, mean_size = inputs(name)
    terms, grads, ep = run_device(S_np, T_np, mean_size)
    want, decisions, _, outputs, want_grads = restated(name)
    print(name, "terms", terms, "want", want)
    noise = gold(name, "noise") if name in CASES else NOISE_MAX
    check_terms(terms, want, noise, (name, "restatement"))
    check_grads(grads, want_grads, (name, "restatement"))
    check_outputs(ep, outputs, name)
    B, K = S_np["last_center"].shape[:2]
    check_decisions(device_decisions(S_np, T_np, mean_size), decisions, B * K, name)
    if name in CASES:
        check_terms(terms, gold(name, "terms"), gold(name, "noise"), (name, "fixture"))
        got = np.stack([np.stack([ep[p + "ema_assignment"].cpu().numpy(), ep[p + "ema_assignment_quad"].cpu().numpy()])
                        for p in mt_inputs.PREFIXES])
        assert np.array_equal(got, gold(name, "assignment")) and np.array_equal(got, assignments(decisions)), name
    if name == "s":
        check_grads(grads, {k: gold("s", f"grad.{k}") for k in GRAD_NAMES}, ("s", "fixture"))


def test_two_calls_give_the_same_bits():
    S_np, T_np, mean_size = inputs("m")
    a, b = run_device(S_np, T_np, mean_size), run_device(S_np, T_np, mean_size)
    assert a[0] == b[0]
    assert all(np.array_equal(a[1][k], b[1][k]) for k in GRAD_NAMES)
    assert all(torch.equal(a[2][p + "ema_center"], b[2][p + "ema_center"]) for p in mt_inputs.PREFIXES)


def test_teacher_equal_to_student_under_the_identity_augmentation():
    """every centre distance is exactly 0, so are both centre terms; all gradients finite"""
    S_np, T_np, mean_size = mt_inputs.make("s", 9, identity=True)
    terms, grads, ep = run_device(S_np, T_np, mean_size)
    assert terms[0] == 0.0 and terms[4] == 0.0
    assert all(np.isfinite(t) for t in terms) and all(np.isfinite(g).all() for g in grads.values())
    assert abs(terms[1]) < 1e-6 and abs(terms[2]) < 1e-12 and abs(terms[7]) < 1e-12      # KL(p, p), |size - size|^2
    K = S_np["last_center"].shape[1]
    for p in mt_inputs.PREFIXES:
        assert torch.equal(ep[p + "ema_assignment"].cpu(), torch.arange(K).expand(3, K))
        assert torch.equal(ep[p + "ema_center"].cpu(), torch.from_numpy(T_np[p + "center"]))
        assert not grads[p + "center"].any() and not grads[p + "quad_center"].any()


def test_one_scene_of_one_proposal():
    S_np, T_np, mean_size = mt_inputs.make((1, 1, 3, 2), 4)
    terms, grads, ep = run_device(S_np, T_np, mean_size)
    S, T, ms = R.leaves(S_np, T_np, mean_size, set(GRAD_NAMES))
    want = R.consistency(S, T, ms, mt_inputs.PREFIXES)[0]
    sum(w * t for w, t in zip(WEIGHTS, want)).backward()
    # n = 1: eps is the value itself, nothing is below it -- every clipped term is 0 and only the KL terms remain
    assert [terms[t] for t in (0, 2, 4, 6, 7)] == [0.0] * 5 and terms[1] > 0 and terms[5] > 0
    check_terms(terms, [float(t.detach()) for t in want], NOISE_MAX, "B=K=1")
    check_grads(grads, {k: S[k].grad.numpy() for k in GRAD_NAMES}, "B=K=1")
    assert all(int(ep[p + "ema_assignment"]) == 0 for p in mt_inputs.PREFIXES)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_inputs_are_computed_in_float32_and_get_gradients_in_their_dtype(dtype):
    S_np, T_np, mean_size = inputs("s")
    terms16, grads16, _ = run_device(S_np, T_np, mean_size, dtype)          # run_device checks the gradients' dtype
    rounded = lambda d: {k: (torch.from_numpy(v).to(dtype).float().numpy() if v.dtype == np.float32 else v)  # noqa: E731
                         for k, v in d.items()}
    terms32, grads32, _ = run_device(rounded(S_np), rounded(T_np), mean_size)
    assert terms16 == terms32
    for k in GRAD_NAMES:
        assert np.array_equal(grads16[k], torch.from_numpy(grads32[k]).to(dtype).float().numpy()), k


def test_cpu_tensors_and_oversized_calls_are_refused():
    S_np, T_np, mean_size = mt_inputs.make((1, 2, 2, 2))
    cfg = mt_inputs.Config(2)
    S, T = to_device(S_np, T_np)
    with pytest.raises(RuntimeError, match="CUDA"):
        hip().get_consistency_loss(S, {k: v.cpu() for k, v in T.items()}, cfg)
    with pytest.raises(ValueError, match="shape"):
        hip().get_consistency_loss(S, dict(T, last_quad_size=T["last_quad_size"][:, :1]), cfg)
    big = {k: (v.expand(61 * 128, *v.shape[1:]) if k not in ("rot_mat",) else v.expand(61 * 128, 3, 3)) for k, v in S.items()}
    with pytest.raises(ValueError, match="LDS"):
        hip().get_consistency_loss(big, T, cfg)


# -------------------------------------------------------------------------------------------------------------- capture
def test_forward_and_backward_replay_from_a_hip_graph(monkeypatch):
    """No host read anywhere: forward and backward are captured once on ONE stream -- two C-ABI calls, four launches -- and
    replayed on fresh inputs; each replay is bit-equal to an eager call on the same inputs."""
    from pointnet2 import _ext
    S_np, T_np, mean_size = inputs("s")
    cfg = mt_inputs.Config(mean_size.shape[0])
    S, T = to_device(S_np, T_np)
    weights = torch.tensor(WEIGHTS, device="cuda")               # an upload inside the capture would be refused
    calls = []
    real_run = _ext._run
    real_stream = _ext._stream
    streams = []
    monkeypatch.setattr(_ext, "_stream", lambda *a: streams.append(real_stream(*a)) or streams[-1])
    monkeypatch.setattr(_ext, "_run", lambda fn, *a: calls.append(fn.__name__) or real_run(fn, *a))

    def run():
        ep = dict(S)
        total, ep = hip().get_consistency_loss(ep, T, cfg)
        terms = torch.stack([ep[k] for k in hip().TERM_KEYS] + [total])
        grads = torch.autograd.grad((terms * weights).sum(), [S[k] for k in GRAD_NAMES])
        return terms, grads, ep["last_ema_assignment"], ep["2head_ema_center_quad"]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    del streams[:], calls[:]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g = run()
    assert calls == ["omnipq_mt_consistency", "omnipq_mt_consistency_grad"], calls
    assert len(streams) == 2 and len({s.value for s in streams}) == 1, streams
    for seed in (31, 32):
        fresh_S, fresh_T, _ = mt_inputs.make("s", seed)
        with torch.no_grad():
            for k, v in S.items():
                v.copy_(torch.from_numpy(fresh_S[k]))
            for k, v in T.items():
                v.copy_(torch.from_numpy(fresh_T[k]))
        graph.replay()
        torch.cuda.synchronize()
        got = [out_g[0].clone(), [g.clone() for g in out_g[1]], out_g[2].clone(), out_g[3].clone()]
        want = run()
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and torch.equal(got[3], want[3])
        assert all(torch.equal(a, b) for a, b in zip(got[1], want[1]))
        assert float(got[0][9]) > 0 and all(bool(g.any()) for g in got[1])


def test_criterion_of_a_captured_step_with_a_teacher():
    """CapturedStep(teacher=..., teacher_to_criterion=True) with the consistency loss in its criterion: the replay equals the
    eager stepper to the noise tests/test_train_step.py allows between the two, and the student's gradients are not those of
    the criterion without the term."""
    import copy
    import bench
    import synth
    import train_step
    from procedural import load_procedural
    from test_oracle_golden import zero_dropout
    dev = torch.device("cuda", 0)
    pc = synth.make_clouds(80, 2, 8192, kind="room").to(dev)
    aug = {k: torch.from_numpy(v).to(dev) for k, v in mt_inputs.augmentation(np.random.default_rng(5), 2).items()}
    cfg = mt_inputs.Config(18)
    cfg.mean_size_arr = bench.mean_size_arr()
    watch = "decoder.0.linear1.weight"

    def run(graph, with_term):
        net = load_procedural(bench.build_model(0)).to(dev).train()
        zero_dropout(net)
        teacher = copy.deepcopy(net)
        for p in teacher.parameters():
            p.requires_grad_(False)
        seen = {}

        def criterion(ep, labels, teacher_ep):
            loss = bench.loss_of(ep)
            if with_term:
                ep.update(aug)
                term, ep = hip().get_consistency_loss(ep, teacher_ep, cfg)
                seen["term"] = term.detach()           # attached, it would keep the autograd graph alive past the capture
                loss = loss + term
            return loss

        st = train_step.CapturedStep(net, criterion, {"point_clouds": pc}, graph=graph, teacher=teacher,
                                     teacher_to_criterion=True)
        assert st.launch == ("hipGraph replay" if graph else "eager")
        loss = st.step({"point_clouds": pc}, None)
        torch.cuda.synchronize()
        grad = dict(net.named_parameters())[watch].grad.detach().float().clone()
        return float(loss), grad, float(seen["term"]) if with_term else 0.0

    def rel(x, y):
        return float((x.double() - y.double()).norm() / (y.double().norm() + 1e-30))

    replay, eager, plain = run(True, True), run(False, True), run(False, False)
    assert replay[2] > 0 and np.isfinite(replay[0])
    assert abs(replay[0] - eager[0]) <= 1e-5 * abs(eager[0]), (replay[0], eager[0])
    assert abs(replay[2] - eager[2]) <= 1e-4 * abs(eager[2]), (replay[2], eager[2])
    assert rel(replay[1], eager[1]) <= 3e-2 + 1e-4, rel(replay[1], eager[1])
    assert abs(eager[0] - plain[0] - eager[2]) <= 1e-5 * abs(eager[0])
    # two eager steps are bit-reproducible (tests/test_train_step.py): what differs here is the term's gradient
    assert rel(eager[1], plain[1]) > 1e-3, rel(eager[1], plain[1])
