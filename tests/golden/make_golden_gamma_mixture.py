"""Generate tests/golden/gamma_mixture.npz: outputs of the REFERENCE's own gamma-mixture guide

    quad_point_mixture_metric(...)                          /root/reference/models/utils/gamma_mixture_loss_util.py:27-127
    gamma_mixture_guide_criterion(end_points, None, None)   :130-192

imported in place (no bytecode written, nothing copied) and run on the CPU with the real fit.py `fit_gamma` (scipy), on the
seeded inputs of tests/gm_inputs.py.  The fixture holds DATA only: the draws, the four terms, the gradients of sum_t weights[t] * term[t] at the
picked rows, n_k, the score branch, whether the caller's `last_quad_size` was changed, and per term `noise` = |reference (f32) -
tests/gm_restatement.py (f64)|, which the tests use as the floor of their tolerance.  Point clouds are regenerated from
the seed by the tests.

What has to be neutralised to import and run those modules on a machine without a GPU or IPython (none of it changes the
arithmetic): `Tensor.cuda` returns the tensor itself; `IPython`, `models.dump_helper`, `models.dump_helper_quad` and
`models.utils.distance_util` (dumping and plotting only) are empty stand-ins that carry the imported names.
`torch.randint` and `random.choice` are wrapped while the criterion runs, to RECORD what it drew.

Decisions that a last-bit difference could flip are checked to have a margin (asserted below; a failing seed is replaced
by the next): no sampled distance within 1e-4 of t*, every score-branch threshold missed by more than 1e-3, no kept
vertical distance other than the bracketing order statistics within 4 f32 ulp of its 0.85 quantile.

    python tests/golden/make_golden_gamma_mixture.py
"""
import os
import random
import sys
import types

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("OMNIPQ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import gm_inputs  # noqa: E402
import gm_restatement as R  # noqa: E402

torch.set_num_threads(8)
WEIGHTS = (1.0, 2.0, 3.0, 4.0)        # loss = sum_t WEIGHTS[t] * term[t]: every gradient path with a factor of its own
BATCH_K = 10000                       # gamma_mixture_loss_util.py:176
SEEDS = {"a": 101, "b": 102, "c": 103, "d": 104, "e": 105, "batch": 200}


def load_reference():
    sys.path.insert(0, REF)
    for name, attrs in (("IPython", ("embed",)), ("models.dump_helper", ("dump_results", "dump_pc", "dump_pc_colored")),
                        ("models.dump_helper_quad", ("dump_results_quad", "dump_single_quad")),
                        ("models.utils.distance_util", ("Palette",))):
        mod = types.ModuleType(name)
        for a in attrs:
            setattr(mod, a, None)
        sys.modules[name] = mod
    import fit
    from models.utils import gamma_mixture_loss_util as gm
    assert gm.__file__.startswith(REF) and fit.__file__.startswith(REF), (gm.__file__, fit.__file__)
    return gm, fit


class cpu_as_cuda:
    def __enter__(self):
        self.saved = torch.Tensor.cuda
        torch.Tensor.cuda = lambda self, *a, **k: self

    def __exit__(self, *exc):
        torch.Tensor.cuda = self.saved


class recording:
    """While active: fit.fit_gamma reports how many samples it kept; torch.randint and random.choice report their results."""

    def __init__(self, fit):
        self.fit, self.kept, self.randint, self.choice = fit, [], [], []

    def __enter__(self):
        self.saved = (self.fit.fit_gamma, torch.randint, random.choice)
        fit_gamma, randint, choice = self.saved

        def fit_gamma_(arr, *a, **k):
            mask = fit_gamma(arr, *a, **k)
            self.kept.append(len(mask) - int(np.sum(mask)))
            return mask

        def randint_(*a, **k):
            out = randint(*a, **k)
            self.randint.append(out.clone())
            return out

        def choice_(seq):
            out = choice(seq)
            self.choice.append(int(out))
            return out

        self.fit.fit_gamma, torch.randint, random.choice = fit_gamma_, randint_, choice_
        return self

    def __exit__(self, *exc):
        self.fit.fit_gamma, torch.randint, random.choice = self.saved


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def margins(s):
    """Smallest distance of the decisions of one restated scene to their thresholds."""
    out = {"t_star": float((s["total"].abs() - R.T_STAR).abs().min())}
    if s["n_k"] >= R.MIN_KEPT:
        mn, mv, ms, _ = (float(t.detach()) for t in s["terms"])
        out["branch"] = min(abs(mv - 0.05), abs(mv - 0.3), abs(mn - 0.02), abs(mn - 0.05), abs(ms - 0.10), abs(ms - 0.35))
        vk = np.sort(s["v_keep"].numpy())
        rank = 0.85 * (len(vk) - 1)
        lo, hi = vk[int(np.floor(rank))], vk[int(np.ceil(rank))]
        others = vk[(vk != lo) & (vk != hi)]
        q85 = float(s["q85"])
        out["q85"] = float(np.abs(others - q85).min()) / ulp32(q85)
    return out


def margins_ok(m):
    return m["t_star"] > 1e-4 and m.get("branch", 1.0) > 1e-3 and m.get("q85", 100.0) > 4.0


def run_case(gm, fit, case, seed):
    """The reference's quad_point_mixture_metric on one scene with draws of our own -> the case's arrays, or None when a
    decision has no margin."""
    K = gm_inputs.CASES[case][0]
    sc_np = gm_inputs.make(seed, case)
    rng = np.random.default_rng(seed + 1)
    pick = gm_inputs.SLOTS[int(rng.integers(0, 2))]
    inds = rng.integers(0, gm_inputs.N, K)
    ep_r, lv_r = R.leaves(gm_inputs.batch([sc_np]))
    terms_r, (s,) = R.criterion(ep_r, [pick], [inds])
    m = margins(s) if not s["skipped"] else {"t_star": 1.0}
    if not margins_ok(m):
        print(f"{case}: seed {seed} has a rounding-sensitive decision {m}, trying the next")
        return None
    leaves = {k: torch.from_numpy(sc_np[k].copy()).requires_grad_(True)
              for k in ("last_quad_scores", "last_quad_center", "last_quad_size")}
    ep = {k: torch.from_numpy(v.copy()) for k, v in sc_np.items()}
    ep.update({k: v * 1.0 for k, v in leaves.items()})          # non-leaf, as a network's outputs are
    size_before = ep["last_quad_size"].detach().clone()
    out = {}
    if s["skipped"]:
        terms, n_k, mutated = [0.0] * 4, 0, False                 # the criterion never reaches the metric (:168)
    else:
        t = torch.from_numpy(inds)
        with cpu_as_cuda(), recording(fit) as rec:
            terms = gm.quad_point_mixture_metric(ep["last_quad_center"][pick], ep["last_normal_vector"][pick],
                                                 ep["last_quad_size"][pick], ep["last_quad_scores"][pick],
                                                 ep["point_clouds"][t], ep["vertex_normals"][t], save_name=None)
        n_k = rec.kept[0]
        loss = sum(w * x for w, x in zip(WEIGHTS, terms) if torch.is_tensor(x) and x.requires_grad)
        if torch.is_tensor(loss):
            loss.backward()
        changed = (ep["last_quad_size"].detach() != size_before).nonzero().tolist()
        assert changed == [[pick, 0]], changed
        mutated = True
    assert n_k == s["n_k"] or s["skipped"], (n_k, s["n_k"])
    terms = np.array([float(x) for x in terms], dtype=np.float64)
    branch = 0 if terms[3] == 0 else (1 if terms[1] < 0.05 and terms[0] < 0.02 and terms[2] < 0.10 else 2)
    assert branch == s["branch"], (branch, s["branch"])
    out["seed"] = np.array([seed], dtype=np.int64)
    out["K"] = np.array([K], dtype=np.int64)
    out["pick"] = np.array([pick], dtype=np.int32)
    out["sample_inds"] = inds.astype(np.uint16)
    out["terms"] = terms
    out["n_k"] = np.array([n_k], dtype=np.int64)
    out["branch"] = np.array([branch], dtype=np.int64)
    out["mutated"] = np.array([mutated])
    out["noise"] = np.abs(terms - np.array([float(x) for x in terms_r]))
    for k, leaf in leaves.items():
        g = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        rest = g.clone()
        rest[pick] = 0
        assert not rest.any(), k                                 # zero outside the picked row
        out[f"grad.{k}"] = g[pick].numpy().astype(np.float64)
    print(f"{case}: seed {seed} K {K} n_k {n_k} branch {branch} terms {terms} noise {out['noise']} margins {m}")
    return out


def run_batch(gm, fit, seed):
    """The reference's whole criterion on the five cases stacked, with ITS draws recorded."""
    scenes = [gm_inputs.make(seed + i, c) for i, c in enumerate(gm_inputs.ORDER)]
    ep_np = gm_inputs.batch(scenes)
    B = len(scenes)
    leaves = {k: torch.from_numpy(ep_np[k].copy()).requires_grad_(True)
              for k in ("last_quad_scores", "last_quad_center", "last_quad_size")}
    ep = {k: torch.from_numpy(v.copy()) for k, v in ep_np.items()}
    ep.update({k: v * 1.0 for k, v in leaves.items()})
    size_before = ep["last_quad_size"].detach().clone()
    random.seed(seed)
    torch.manual_seed(seed)
    with cpu_as_cuda(), recording(fit) as rec:
        terms = gm.gamma_mixture_guide_criterion(ep, None, None)
    # what was drawn, scene by scene: a skipped scene draws its quad with torch.randint (:157), the others with
    # random.choice (:163, two candidates per scene here) and then their K samples (:177)
    cand = [R.candidates(torch.from_numpy(s["last_quad_scores"])) for s in scenes]
    draws, choices, kept = list(rec.randint), list(rec.choice), list(rec.kept)
    pick = np.zeros(B, dtype=np.int32)
    inds = np.zeros((B, BATCH_K), dtype=np.int64)
    skipped = np.zeros(B, dtype=bool)
    n_k = np.zeros(B, dtype=np.int64)
    for b in range(B):
        if not cand[b].any():
            pick[b] = int(draws.pop(0)[0])
            skipped[b] = True
            continue
        assert int(cand[b].sum()) == 2
        pick[b] = choices.pop(0)
        inds[b] = draws.pop(0).numpy()
        n_k[b] = kept.pop(0)
    assert not draws and not choices and not kept
    loss = sum(w * x for w, x in zip(WEIGHTS, terms))
    loss.backward()
    changed = (ep["last_quad_size"].detach() != size_before).nonzero().tolist()
    assert changed == [[b, int(pick[b]), 0] for b in range(B) if not skipped[b]], changed
    # the restatement on the same draws: margins, n_k, noise
    ep_r, _ = R.leaves(ep_np)
    terms_r, restated = R.criterion(ep_r, pick, inds)
    branch = np.zeros(B, dtype=np.int64)
    for b, s in enumerate(restated):
        if s["skipped"]:
            assert skipped[b]
            continue
        m = margins(s)
        if not margins_ok(m):
            print(f"batch: seed {seed}, scene {b} has a rounding-sensitive decision {m}, trying the next")
            return None
        assert s["n_k"] == n_k[b], (b, s["n_k"], n_k[b])
        branch[b] = s["branch"]
    terms = np.array([float(x) for x in terms], dtype=np.float64)
    out = {"seed": np.array([seed], dtype=np.int64), "K": np.array([BATCH_K], dtype=np.int64), "pick": pick,
           "sample_inds": inds.astype(np.uint16), "skipped": skipped, "n_k": n_k, "branch": branch, "terms": terms,
           "mutated": np.array([bool(changed)]), "noise": np.abs(terms - np.array([float(x) for x in terms_r]))}
    for k, leaf in leaves.items():
        g = leaf.grad
        rows = g[torch.arange(B), torch.from_numpy(pick).long()]
        rest = g.clone()
        rest[torch.arange(B), torch.from_numpy(pick).long()] = 0
        assert not rest.any(), k
        out[f"grad.{k}"] = rows.numpy().astype(np.float64)
    print(f"batch: seed {seed} pick {pick} n_k {n_k} branch {branch} terms {terms} noise {out['noise']}")
    return out


def main():
    gm, fit = load_reference()
    out = {"weights": np.array(WEIGHTS)}
    for name in list(gm_inputs.ORDER) + ["batch"]:
        seed = SEEDS[name]
        while True:
            got = run_batch(gm, fit, seed) if name == "batch" else run_case(gm, fit, name, seed)
            if got is not None:
                break
            seed += 100
        out.update({f"{name}.{k}": v for k, v in got.items()})
    # what the cases are there for
    assert out["a.branch"][0] == 1 and out["b.branch"][0] == 0 and out["c.branch"][0] == 2 and out["c.n_k"][0] >= 300
    assert out["b.n_k"][0] >= 300 and 0 < out["d.n_k"][0] < 300 and not out["e.terms"].any()
    assert list(out["batch.branch"]) == [1, 0, 2, 0, 0] and list(out["batch.skipped"]) == [False] * 4 + [True]
    path = os.path.join(HERE, "gamma_mixture.npz")
    np.savez_compressed(path, **out)
    print(f"gamma_mixture.npz: {len(out)} arrays, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
