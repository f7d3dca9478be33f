"""Generate tests/golden/lr_schedule.npz: what the REFERENCE's own schedulers do

    get_scheduler(optimizer, n_iter_per_epoch, args)          utils/lr_scheduler.py:65-87

imported in place (no bytecode written, nothing copied), on a torch.optim.AdamW over two parameter groups.  The fixture holds
DATA only, per case of tests/lr_schedule_restatement.py: CASES ({cosine, step} x {warm-up 2, none}):

    <case>/lrs        (STEPS + 1, 2) f64: param_groups' learning rates at construction and after every scheduler.step()
    <case>/maxrel     max over steps and groups of |reference - restatement| / reference
    <case>/dict<e>    the scheduler's state_dict() after e steps, e in DICT_STEPS, as JSON text

    python tests/golden/make_golden_lr_schedule.py
"""
import json
import os
import sys
import types
import warnings

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OMNIPQ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import lr_schedule_restatement as R  # noqa: E402


def load_reference():
    sys.path.insert(0, os.path.join(REF, "utils"))
    import lr_scheduler
    assert lr_scheduler.__file__.startswith(REF), lr_scheduler.__file__
    return lr_scheduler


def plain(x):
    """a state_dict as JSON-able data: Counter -> {str: int} under its own marker, tuples -> lists"""
    from collections import Counter
    if isinstance(x, Counter):
        return {"__counter__": {str(k): int(v) for k, v in x.items()}}
    if isinstance(x, dict):
        return {str(k): plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if isinstance(x, (bool, int, float, str)) or x is None:
        return x
    raise TypeError(f"state_dict holds a {type(x).__name__}")


def main():
    ref = load_reference()
    out = {}
    for name, (kind, warm) in R.CASES.items():
        params = [torch.nn.Parameter(torch.zeros(1)) for _ in R.BASE_LRS]
        opt = torch.optim.AdamW([{"params": [p], "lr": lr} for p, lr in zip(params, R.BASE_LRS)])
        args = types.SimpleNamespace(lr_scheduler=kind, max_epoch=R.MAX_EPOCH, warmup_epoch=warm, warmup_multiplier=R.MULTIPLIER,
                                     lr_decay_epochs=list(R.DECAY_EPOCHS), lr_decay_rate=R.DECAY_RATE)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sched = ref.get_scheduler(opt, R.N_ITER, args)
            restated = R.case(name)
            rows, worst = [], 0.0
            for e in range(R.STEPS + 1):
                if e:
                    opt.step()
                    sched.step()
                lrs = [float(g["lr"]) for g in opt.param_groups]
                rows.append(lrs)
                worst = max(worst, max(abs(a - b) / a for a, b in zip(lrs, restated.lrs(e))))
                if e in R.DICT_STEPS:
                    out[f"{name}/dict{e}"] = np.array(json.dumps(plain(sched.state_dict()), sort_keys=True))
        out[f"{name}/lrs"] = np.asarray(rows, dtype=np.float64)
        out[f"{name}/maxrel"] = np.float64(worst)
        print(f"{name}: max relative difference to the restatement {worst:.3e}")
    path = os.path.join(HERE, "lr_schedule.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
