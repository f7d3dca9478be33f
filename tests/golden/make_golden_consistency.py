"""Generate tests/golden/consistency.npz: outputs of the REFERENCE's own mean-teacher consistency loss

    get_consistency_loss(end_points, ema_end_points, DATASET_CONFIG)     models/utils/mean_teacher_consistency_util.py:201-270

imported in place (no bytecode written, nothing copied) and run on the CPU in float32 on the seeded inputs of
tests/mt_inputs.py.  The fixture holds DATA only, per case: the ten terms, the assignments (`*ema_assignment*`), per term
`noise` = |reference (f32) - tests/mt_restatement.py (f64)|, which the tests use as the floor of their tolerance, and whether
the reference changed the teacher's centres in place; for the smallest case also the gradients of sum_t WEIGHTS[t] * term[t]
with respect to every differentiable input of the student.  The inputs are regenerated from the seeds by the tests.

What has to be neutralised to run the module without a GPU: `Tensor.cuda` returns the tensor itself.

    python tests/golden/make_golden_consistency.py            write the fixture
    python tests/golden/make_golden_consistency.py --scan     print, per case, the first seeds whose decisions have margins
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OMNIPQ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mt_inputs  # noqa: E402
import mt_restatement as R  # noqa: E402

torch.set_num_threads(8)
WEIGHTS = (1.0, 2.0, 3.0, 0.5, 1.5, 2.5, 3.5, 4.5, 0.25, 0.75)   # every gradient path with a factor of its own
MARGIN = 1e-4
GRAD_CASE = "s"


def load_reference():
    sys.path.insert(0, os.path.join(REF, "utils"))
    sys.path.insert(0, REF)
    from models.utils import mean_teacher_consistency_util as mt
    assert mt.__file__.startswith(REF), mt.__file__
    return mt


class cpu_as_cuda:
    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved


def grad_names():
    return [p + k for p in mt_inputs.PREFIXES for k in mt_inputs.GRAD_KEYS]


def restate(case, seed=None):
    S_np, T_np, mean_size = mt_inputs.make(case, seed)
    S, T, ms = R.leaves(S_np, T_np, mean_size, set(grad_names()))
    terms, decisions, margins, outputs = R.consistency(S, T, ms, mt_inputs.PREFIXES)
    return terms, decisions, margins, outputs, S


def frac(case):
    B, K = mt_inputs.CASES[case][:2]
    rank = 0.85 * (B * K - 1)
    return rank - np.floor(rank)


def quick_nn_margin(S, T):
    """the nearest-neighbour margin alone, in numpy: a cheap filter in front of the restatement"""
    B = S["scale"].shape[0]
    sign = np.ones((B, 1, 3))
    sign[:, 0, 0] = np.where(S["flip_x_axis"] != 0, -1.0, 1.0)
    sign[:, 0, 1] = np.where(S["flip_y_axis"] != 0, -1.0, 1.0)
    worst = np.inf
    for p in mt_inputs.PREFIXES:
        for kind in ("center", "quad_center"):
            e = np.einsum("bkj,bij->bki", T[p + kind].astype(np.float64) * sign, S["rot_mat"].astype(np.float64))
            e = e * S["scale"].astype(np.float64).reshape(B, 1, 1)
            dist = ((S[p + kind].astype(np.float64)[:, :, None] - e[:, None]) ** 2).sum(-1)
            for axis in (1, 2):
                two = np.sort(dist, axis=axis).take([0, 1], axis=axis)
                lo, hi = two.take(0, axis=axis), two.take(1, axis=axis)
                worst = min(worst, float(((hi - lo) / (1.0 + lo)).min()))
    return worst


def scan(count=2, limit=3000, headroom=1.2):
    for case in mt_inputs.CASES:
        found = []
        for seed in range(limit):
            S, T, _ = mt_inputs.make(case, seed)
            if quick_nn_margin(S, T) <= headroom * MARGIN:
                continue
            margins = restate(case, seed)[2]
            if min(margins.values()) > headroom * MARGIN:
                found.append((seed, {k: f"{v:.2e}" for k, v in margins.items()}))
                if len(found) == count:
                    break
        print(case, f"frac {frac(case):.2f}", found, flush=True)


def run_case(mt, case):
    S_np, T_np, mean_size = mt_inputs.make(case)
    terms_r, decisions, margins, _, _ = restate(case)
    assert min(margins.values()) > MARGIN and 0.1 <= frac(case) <= 0.9, (case, margins, frac(case))
    names = grad_names()
    leaves = {k: torch.from_numpy(S_np[k].copy()).requires_grad_(True) for k in names}
    ep = {k: torch.from_numpy(v.copy()) for k, v in S_np.items()}
    ep.update({k: v * 1.0 for k, v in leaves.items()})               # non-leaf, as a network's outputs are
    ema = {k: torch.from_numpy(v.copy()) for k, v in T_np.items()}
    with cpu_as_cuda():
        total, ep = mt.get_consistency_loss(ep, ema, mt_inputs.Config(mean_size.shape[0]))
    terms = [ep[k] for k in R.TERMS] + [total]
    mutated = any(not np.array_equal(ema[p + k].numpy(), T_np[p + k]) for p in mt_inputs.PREFIXES
                  for k in ("center", "quad_center"))
    out = {"terms": np.array([float(t) for t in terms], dtype=np.float64), "mutated": np.array([mutated])}
    out["noise"] = np.abs(out["terms"] - np.array([float(t) for t in terms_r]))
    assign = np.stack([np.stack([ep[p + "ema_assignment"].numpy(), ep[p + "ema_assignment_quad"].numpy()])
                       for p in mt_inputs.PREFIXES])
    want = np.stack([np.stack([decisions[(p, 0)]["ind2"].numpy(), decisions[(p, 1)]["ind2"].numpy()])
                     for p in mt_inputs.PREFIXES])
    assert np.array_equal(assign, want), case                        # f32 and f64 take the same decisions
    out["assignment"] = assign.astype(np.int16)
    if case == GRAD_CASE:
        sum(w * t for w, t in zip(WEIGHTS, terms)).backward()
        for k in names:
            out[f"grad.{k}"] = leaves[k].grad.numpy().astype(np.float32)
    print(f"{case}: terms {out['terms']}\n   noise {out['noise']} margins {margins} mutated {mutated}")
    return out


def main():
    if "--scan" in sys.argv:
        return scan()
    mt = load_reference()
    out = {"weights": np.array(WEIGHTS)}
    for case in mt_inputs.CASES:
        out.update({f"{case}.{k}": v for k, v in run_case(mt, case).items()})
    path = os.path.join(HERE, "consistency.npz")
    np.savez_compressed(path, **out)
    print(f"consistency.npz: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
