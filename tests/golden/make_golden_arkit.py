"""Generate tests/golden/arkit_pc.npz: outputs of the REFERENCE's own ARKit physical-constraint loss

    get_arkit_pc_loss(end_points, batch_data_unlabeled, DATASET_CONFIG)            models/utils/arkit_loss_util.py:5-52

imported in place (no bytecode written, nothing copied) and run on the CPU in float32 on the seeded inputs of
tests/arkit_inputs.py.  The fixture holds DATA only, per case: the loss, the collision count and `noise` = |reference (f32) -
tests/arkit_restatement.py (f64)|, which the tests use as the floor of their tolerance; for the smallest case also the
gradients of the loss with respect to `last_quad_center` and `last_normal_vector`.  The inputs are regenerated from the seeds
by the tests.

The reference slices the labels with `[:n]`, so the NaN rows the inputs carry beyond a scene's count never reach it.
What has to be neutralised to import and run the module without a GPU or a display: `Tensor.cuda` returns the tensor itself,
and an empty module named `turtle` stands in for the unused tkinter import of models/loss_helper_pq.py:1.

    python tests/golden/make_golden_arkit.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OMNIPQ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import arkit_inputs  # noqa: E402
import arkit_restatement as R  # noqa: E402

torch.set_num_threads(8)
MARGIN = 1e-4
GRAD_CASE = "s"


def load_reference():
    sys.path.insert(0, os.path.join(REF, "utils"))
    sys.path.insert(0, os.path.join(REF, "models"))
    sys.path.insert(0, REF)
    sys.modules.setdefault("turtle", types.ModuleType("turtle"))
    sys.modules["turtle"].distance = None
    from models.utils import arkit_loss_util
    assert arkit_loss_util.__file__.startswith(REF), arkit_loss_util.__file__
    return arkit_loss_util


class cpu_as_cuda:
    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved


def run_case(ref, case):
    pred, unl = arkit_inputs.make(case)
    want, collisions, record, margins, _ = R.arkit_pc(R.leaves(pred), unl)
    assert min(margins.values()) > MARGIN, (case, margins)
    leaves = {k: torch.from_numpy(pred[k].copy()).requires_grad_(True) for k in R.GRAD_KEYS}
    ep = {k: torch.from_numpy(v.copy()) for k, v in pred.items()}
    ep.update({k: v * 1.0 for k, v in leaves.items()})               # non-leaf, as a network's outputs are
    batch = {k: torch.from_numpy(v.copy()) for k, v in unl.items()}
    with cpu_as_cuda():
        loss, hits = ref.get_arkit_pc_loss(ep, batch, None)
    assert int(hits) == collisions, (case, int(hits), collisions)    # f32 and f64 take the same decisions
    got = float(loss.detach())
    out = {"loss": np.array([got]), "collisions": np.array([int(hits)], dtype=np.int64),
           "noise": np.array([abs(got - float(want.detach()))])}
    if case == GRAD_CASE:
        loss.backward()
        for k in R.GRAD_KEYS:
            out[f"grad.{k}"] = leaves[k].grad.numpy().astype(np.float32)
    print(f"{case}: loss {out['loss'][0]:.9g} collisions {int(hits)} noise {out['noise'][0]:.3g} margins {margins} "
          f"gated {int(record[..., 0].sum())} of {record[..., 0].size}")
    return out


def main():
    ref = load_reference()
    out = {}
    for case in arkit_inputs.CASES:
        out.update({f"{case}.{k}": v for k, v in run_case(ref, case).items()})
    path = os.path.join(HERE, "arkit_pc.npz")
    np.savez_compressed(path, **out)
    print(f"arkit_pc.npz: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
