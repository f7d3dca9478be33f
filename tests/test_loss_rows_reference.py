"""CPU: the float64 reference of the supervised-loss row kernels and its elementwise bounds (tests/loss_rows_reference.py) have
teeth.

On every case the GPU suite runs (tests/test_gpu_loss_rows_f64.py walks the same tables) the numpy-float32 emulation of the
kernels' arithmetic stays inside every bound, at or below 1 / MARGIN of it; its structural zeros are the bits of +0.0; the
decisions it takes (nearest ground truth, NEAR / FAR, winning votes, signs, the cosine branch, every corner x quad gate) agree
with the same decisions taken in float64 wherever those are not undecided, at most 0.5 % of a random case's decisions are
undecided and none of a lattice case's; assembled the way get_loss weighs them, the reference functions reproduce the existing
oracle (oracle/get_loss_oracle.py, itself pinned by tests/golden/get_loss.npz) at the tolerances of test_get_loss_oracle.py;
and each of sixteen plausible kernel defects put into the emulation leaves a bound or flips an exact output on the case named
for it.

Largest error / bound ratio of the emulation per output over all cases (expf / logf emulated as correctly rounded), measured:
    box rows    terms 0.171   objectness 0.409   center 0.378   heading_scores 0.344   heading_residuals 0.243
                size_scores 0.313   size_residuals 0.502   sem_cls_scores 0.321
    quad rows   terms 0.165   quad_scores 0.432   quad_center 0.380   normal_vector 0.184   quad_size 0.230
    votes       loss 0.137   grad 0.415
    physical    out 0.039   g_center 0.109   g_size_residuals 0.090   g_quad_center 0.512   g_normal 0.372
"""
import os
import re

import numpy as np
import pytest

import loss_inputs
import loss_rows_reference as lr
from test_get_loss_oracle import GRAD_RTOL, TERM_RTOL, build

F, D = np.float32, np.float64


def flat(x):
    out = {"terms": x["terms"]}
    out.update(x["grads"])
    return out


def zeros_ok(got, zeros):
    """names of the gradients whose structural zeros are not all +0.0"""
    return {n for n, z in zeros.items() if not lr.plus_zero(got[n], np.broadcast_to(z, got[n].shape))}


def run(case, mutant=None):
    """-> (ratios, names of exact outputs that differ, Tally): the emulation (with a defect put in) against the reference"""
    id = case["id"]
    if id.startswith("assign"):
        inp = lr.assign_inputs(case)
        good, got = lr.assign_emulate(inp), lr.assign_emulate(inp, mutant)
        flips = {n for n in ("label", "mask", "assignment", "counts") if not np.array_equal(good[n], got[n])}
        return {}, flips, lr.assign_decisions(inp, good)
    if id.startswith("box"):
        inp = lr.box_inputs(case)
        got = flat(lr.box_emulate(inp, mutant))
        ref, bnd, zeros = lr.box_reference(inp)
        flips = zeros_ok(got, zeros) | ({"terms7"} if not lr.plus_zero(got["terms"][:, 7]) else set())
        return lr.rat(got, flat(ref), flat(bnd)), flips, lr.Tally()
    if id.startswith("quad"):
        inp = lr.quad_inputs(case)
        good, got = lr.quad_emulate(inp), lr.quad_emulate(inp, mutant)
        ref, bnd, zeros, tally = lr.quad_reference(inp, good["branch"])
        flips = zeros_ok(got["grads"], zeros) | ({"terms4to7"} if not lr.plus_zero(got["terms"][:, 4:]) else set())
        return lr.rat(flat(got), flat(ref), flat(bnd)), flips, tally
    if id.startswith("votes"):
        inp = lr.votes_inputs(case)
        good, got = lr.votes_emulate(inp), lr.votes_emulate(inp, mutant)
        ref, bnd, zeros, tally = lr.votes_reference(inp, good)
        return lr.rat({n: got[n] for n in ("loss", "grad")}, ref, bnd), zeros_ok(got, dict(grad=zeros)), tally
    assert id.startswith("pc"), id
    inp = lr.pc_inputs(case)
    good, got = lr.pc_emulate(inp), lr.pc_emulate(inp, mutant)
    ref, bnd, zeros, tally = lr.pc_reference(inp, good)
    return lr.rat({n: got[n] for n in ("out",) + lr.PC_GRADS}, ref, bnd), zeros_ok(got, zeros), tally


def test_case_tables_cover_what_they_say():
    ids = lr.ids(lr.ALL_CASES)
    assert len(set(ids)) == len(ids)
    assert {(c["b"], c["k"], c["k2"]) for c in lr.ASSIGN_CASES} >= {(1, 1, 1), (2, 257, 64), (3, 300, 513), (1, 64, 1100)}
    full = [c for c in lr.BOX_CASES if not c.get("only_objectness")]
    assert {c["b"] * c["k"] for c in full} >= {1, 255, 256, 257, 513} and {c["heads"] for c in full} >= {1, 3, 8}
    assert all(c["b"] > 1 for c in full if c["b"] * c["k"] > 1)
    assert {c["dims"] for c in full} == {(1, 1, 1), (12, 18, 18), (64, 64, 64), (5, 64, 2)}
    assert {c["k2"] for c in full if c["dims"] == (1, 1, 1)} == {1, 64}
    assert {c.get("scores", "randn") for c in lr.BOX_CASES} == {"randn", "pm60", "equal", "onelow"}
    assert {c.get("ptrs", "all") for c in lr.BOX_CASES} == {"all", "none", "rot"} == {c.get("ptrs", "all") for c in lr.QUAD_CASES}
    assert {c["b"] * c["k"] for c in lr.QUAD_CASES} >= {1, 256, 257, 513} and {c["heads"] for c in lr.QUAD_CASES} == {1, 7, 8}
    assert {c["dims"] for c in lr.VOTE_CASES} >= {(1, 1, 1, 1, 1), (2, 257, 300, 1, 3), (2, 100, 150, 3, 3), (1, 65, 70, 2, 8),
                                                 (1, 33, 40, 1, 1)}
    assert {c["dims"] for c in lr.PC_CASES} >= {(1, 1, 1, 1, 1), (2, 63, 8, 3, 5), (2, 64, 8, 3, 5), (2, 65, 8, 3, 5),
                                               (2, 513, 64, 18, 7), (2, 40, 64, 18, 257), (1, 20, 8, 3, 600)}
    assert len(lr.KINKS) == 9 and float(lr.LO) < 1.0 < float(lr.HI) and lr.LIBM_ULP == 2.0 and len(lr.MUTANTS) == 16


def test_inputs_are_what_their_kind_promises():
    inp = lr.assign_inputs(lr.case_of("assign-3x300x513"))
    emu = lr.assign_emulate(inp)
    assert (emu["bi"] == 512).any() and (emu["bi"][emu["label"] == 1] == 512).any()              # behind the first tile, labelled
    big = lr.assign_emulate(lr.assign_inputs(lr.case_of("assign-1x64x1100")))["bi"]
    assert (big >= 1024).any() and (big < 512).any() and ((big >= 512) & (big < 1024)).any()
    for id in ("assign-2x257x64", "assign-3x300x513"):
        inp = lr.assign_inputs(lr.case_of(id))
        emu = lr.assign_emulate(inp)
        isnear = emu["e"] < F(inp["near"])
        assert {0, 1} <= set(emu["label"][isnear & (inp["num_gt"] == emu["bi"] + 1)]) | set(emu["label"][isnear & (inp["num_gt"] == emu["bi"])])
        assert (emu["label"][isnear & (inp["num_gt"] == emu["bi"])] == 0).all() and (emu["label"][isnear & (inp["num_gt"] == emu["bi"] + 1)] == 1).all()
        padded = ~inp["gt"].any(-1)
        assert np.take_along_axis(padded, emu["bi"], 1).any()                                   # nearest to a padded all-zero slot
    inp = lr.assign_inputs(lr.case_of("assign-lattice"))
    d = lr.assign_emulate(inp)["d"].astype(D)
    assert ((d == d.min(-1, keepdims=True)).sum(-1) > 1).mean() > 0.3                           # exact ties in a third of the rows
    inp = lr.assign_inputs(lr.case_of("assign-atnear"))
    emu = lr.assign_emulate(inp)
    at = emu["e"] == F(inp["near"])
    assert at.sum() >= 5 and not emu["label"][at].any() and not emu["mask"][at].any() and emu["label"].any()
    inp = lr.box_inputs(lr.case_of("box-R513-h3-kink"))
    lab = inp["label"] != 0
    assert set(np.unique(inp["center"][0][lab])) == set(lr.KINKS) and not inp["gt_center"].any()
    assert len(np.unique(inp["gt_heading_class"])) == 12 and len(np.unique(inp["gt_size_class"])) == 18
    inp = lr.box_inputs(lr.case_of("box-R256-h8-pm60"))
    assert set(np.unique(inp["sem_cls_scores"])) == {-60.0, 60.0}
    inp = lr.quad_inputs(lr.case_of("quad-R256-h7"))
    nx = np.linalg.norm(inp["normal_vector"][0].astype(D), axis=1)
    assert (nx == 0).any() and ((nx > 0) & (nx < 1e-8)).any() and (inp["label"] != 0).all()
    y = inp["gt_normal"][lr._gi(inp)].astype(D)
    cs = (inp["normal_vector"][0].astype(D) * y).sum(1) / np.maximum(nx, 1e-8) / np.maximum(np.linalg.norm(y, axis=1), 1e-8)
    assert (cs > 1 - 1e-6).any() and (cs < -1 + 1e-6).any() and (np.linalg.norm(y, axis=1) == 0).any()
    inp = lr.pc_inputs(lr.case_of("pc-lattice"))
    emu = lr.pc_emulate(inp)
    g, live = emu["geo"], np.broadcast_to(emu["live"], emu["gate"].shape)
    assert ((g["delta"] == 0) & live).any()                                                        # a corner on the wall: no hit
    behind = live & emu["neg"]
    assert (behind & (g["w"] == g["half"])).any() and (behind & (g["w"] == F(2.0)) & emu["inside"]).any()
    pens = g["kk"][emu["gate"]]
    assert (pens == F(1677 * 2.0 ** -24)).any() and (pens == F(1678 * 2.0 ** -24)).any()
    assert F(1677 * 2.0 ** -24) < lr.PEN_THR < F(1678 * 2.0 ** -24)
    inp = lr.pc_inputs(lr.case_of("pc-nosolid"))
    use = lr.pc_emulate(inp)["use"]
    assert not use[0].any() and use[1].any()
    inp = lr.pc_inputs(lr.case_of("pc-outside"))                          # every bit of not_solid set: only ids outside 0..63 are solid
    emu = lr.pc_emulate(inp)
    sem = np.take_along_axis(inp["sem_cls_label"], np.clip(inp["object_assignment"], 0, 63), 1)
    assert set(np.unique(sem[emu["use"]])) == {-1, 64} and (sem == 7).any() and emu["out"][1] > 0
    assert (inp["object_assignment"] < 0).any() and (inp["object_assignment"] >= 64).any()
    inp = lr.pc_inputs(lr.case_of("pc-bit63"))
    emu = lr.pc_emulate(inp)
    sem = np.take_along_axis(inp["sem_cls_label"], inp["object_assignment"], 1)
    assert ((sem == 63) & (inp["object_label"] != 0)).any() and not (sem[emu["use"]] == 63).any()
    inp = lr.pc_inputs(lr.case_of("pc-ties"))
    s = inp["size_scores"]
    assert ((s == s.max(-1, keepdims=True)).sum(-1) > 1).all()


@pytest.mark.parametrize("id", lr.ids(lr.ALL_CASES))
def test_emulated_kernel_arithmetic_is_inside_every_bound(id):
    rat, flips, tally = run(lr.case_of(id))
    print(f"\n  RATIO emulation {id}: {lr.fmt(rat)}  decisions {tally.n} undecided {tally.undecided}")
    assert not flips, (id, flips)
    assert not lr.outside(rat), (id, lr.outside(rat))
    assert all(r[0] <= 1.0 / lr.MARGIN for r in rat.values()), (id, lr.fmt(rat))
    assert tally.disagree == 0, (id, tally.disagree)
    assert tally.share() <= (0.0 if id in lr.LATTICE_CASES else lr.UNDECIDED_CAP), (id, tally.undecided, tally.n)


def test_assignment_inputs_of_the_model_are_far_inside_the_cap():
    for seed in range(3):
        lab, _ = loss_inputs.make(seed, K=257, KQ=257, num_seed=8, N=16)
        for q, g in (("aggregated_vote_xyz", "center_label"), ("aggregated_sample_xyz", "gt_quad_centers")):
            inp = dict(query=lab[q], gt=np.ascontiguousarray(lab[g][:, :, :3]), num_gt=np.zeros((2, 257), np.int64), near=0.3, far=0.6)
            t = lr.assign_decisions(inp, lr.assign_emulate(inp))
            assert t.undecided == 0 and t.disagree == 0


def test_out_of_range_labels_give_what_the_clamped_labels_give():
    inp = lr.box_inputs(lr.case_of("box-clamp"))
    assert (inp["assignment"] < 0).any() and (inp["assignment"] >= inp["k2"]).any() and (inp["gt_size_class"] >= inp["ns"]).any()
    a, b = flat(lr.box_emulate(inp)), flat(lr.box_emulate(lr.box_clamped_twin(inp)))
    assert all(np.array_equal(a[n].view(np.int32), b[n].view(np.int32)) for n in a)
    ra, rb = flat(lr.box_reference(inp)[0]), flat(lr.box_reference(lr.box_clamped_twin(inp))[0])
    assert all(np.array_equal(ra[n], rb[n]) for n in ra)


# ---- the reference against the existing oracle, at the model's configuration ---------------------------------------------

def reference_get_loss(lab, pred):
    """the total loss and every gradient from the reference functions, weighed the way get_loss weighs them"""
    pfx = loss_inputs.prefixes()
    H = len(pfx)
    B, K = lab["aggregated_vote_xyz"].shape[:2]
    KQ = lab["aggregated_sample_xyz"].shape[1]
    ns, nc, nh = loss_inputs.NUM_SIZE_CLUSTER, loss_inputs.NUM_CLASS, loss_inputs.NUM_HEADING_BIN
    means = loss_inputs.MEAN_SIZE_ARR
    grads = {}

    def assign(q, g, num, k):
        inp = dict(query=lab[q], gt=np.ascontiguousarray(lab[g][:, :, :3]), near=0.3, far=0.6,
                   num_gt=np.broadcast_to(lab[num].reshape(B, -1), (B, k)))
        return lr.assign_emulate(inp)

    def stack(key, w):
        return np.stack([pred[p + key].reshape(-1, w) for p in pfx])

    scale = 10.0 / H
    oa = assign("aggregated_vote_xyz", "center_label", "num_gt_boxes", K)
    box = dict(b=B, k=K, k2=lab["center_label"].shape[1], heads=H, nh=nh, ns=ns, nc=nc, only_objectness=0,
               label=oa["label"].reshape(-1), mask=oa["mask"].reshape(-1), assignment=oa["assignment"].reshape(-1),
               counts=oa["counts"], w=np.array([0.2, 0.8], dtype=F),
               g_terms=np.tile(np.array([0.5, 1.0, 0.1, 1.0, 0.1, 1.0, 0.1, 0.0]) * 0.9 * scale, (H, 1)).astype(F),
               gt_center=lab["center_label"][:, :, :3].reshape(-1, 3), gt_heading_class=lab["heading_class_label"].reshape(-1),
               gt_heading_residual=lab["heading_residual_label"].reshape(-1), gt_size_class=lab["size_class_label"].reshape(-1),
               gt_size_residual=lab["size_residual_label"].reshape(-1, 3), gt_sem_cls=lab["sem_cls_label"].reshape(-1),
               mean_size=means.astype(F))
    for key, w in zip(lr.BOX_KEYS, lr.box_widths(nh, ns, nc)):
        box[key] = stack(key, w)
    bref = lr.box_reference(box)[0]
    qa = assign("aggregated_sample_xyz", "gt_quad_centers", "num_gt_quads", KQ)
    quad = dict(b=B, k=KQ, k2=lab["gt_quad_centers"].shape[1], heads=H, label=qa["label"].reshape(-1), mask=qa["mask"].reshape(-1),
                assignment=qa["assignment"].reshape(-1), counts=qa["counts"], w=np.array([0.4, 0.6], dtype=F),
                g_terms=np.tile(np.array([0.5, 1.0, 1.0, 1.0, 0, 0, 0, 0]) * 0.1 * scale, (H, 1)).astype(F),
                gt_center=lab["gt_quad_centers"][:, :, :3].reshape(-1, 3), gt_normal=lab["gt_normal_vectors"].reshape(-1, 3),
                gt_size=lab["gt_quad_sizes"].reshape(-1, 2))
    for key, w in zip(lr.QUAD_KEYS, lr.QUAD_WIDTHS):
        quad[key] = stack(key, w)
    qref = lr.quad_reference(quad, lr.quad_emulate(quad)["branch"])[0]
    S, N = lab["seed_xyz"].shape[1], lab["vote_label"].shape[1]
    votes = dict(dims=(B, S, N, 1, 3), seed_xyz=lab["seed_xyz"].reshape(-1, 3), vote_xyz=pred["vote_xyz"].reshape(-1, 3),
                 seed_inds=lab["seed_inds"].reshape(-1), vote_label=lab["vote_label"].reshape(-1, 9),
                 vote_label_mask=lab["vote_label_mask"].reshape(-1), g_loss=F(10.0))
    vref = lr.votes_reference(votes, lr.votes_emulate(votes))[0]
    srn = pred["last_size_residuals_normalized"].reshape(B, K, ns, 3)
    pc = dict(dims=(B, K, lab["sem_cls_label"].shape[1], ns, KQ), center=pred["last_center"], size_scores=pred["last_size_scores"],
              size_residuals=srn * means.astype(F)[None, None], object_label=oa["label"], object_assignment=oa["assignment"],
              sem_cls_label=lab["sem_cls_label"], mean_size64=means, quad_center=pred["last_quad_center"],
              normal_vector=pred["last_normal_vector"], quad_size=pred["last_quad_size"], quad_label=qa["label"],
              not_solid=lr.NOT_SOLID, g_out=F(10.0))
    pref = lr.pc_reference(pc, lr.pc_emulate(pc))[0]
    loss = pref["out"][0] * 10.0 + vref["loss"][0] * 10.0 + float((bref["terms"] * box["g_terms"].astype(D)).sum()) \
        + float((qref["terms"] * quad["g_terms"].astype(D)).sum())
    for i, p in enumerate(pfx):
        for key in lr.BOX_KEYS:
            grads[p + key] = bref["grads"][key][i].reshape(pred[p + key].shape).copy()
        for key in lr.QUAD_KEYS:
            grads[p + key] = qref["grads"][key][i].reshape(pred[p + key].shape).copy()
    grads["vote_xyz"] = vref["grad"].reshape(pred["vote_xyz"].shape)
    grads["last_center"] += pref["g_center"]
    grads["last_size_residuals_normalized"] += (pref["g_size_residuals"] * means[None, None]).reshape(grads["last_size_residuals_normalized"].shape)
    grads["last_quad_center"] += pref["g_quad_center"]
    grads["last_normal_vector"] += pref["g_normal"]
    return loss, dict(box=bref["terms"], quad=qref["terms"], vote=vref["loss"][0], pc=pref["out"]), grads, (oa, qa)


def test_reference_reproduces_the_oracle_at_the_model_configuration():
    from oracle import get_loss_oracle
    lab, pred = loss_inputs.make(5)
    ep, leaves = build(lab, pred)
    want, ep = get_loss_oracle.get_loss(ep, loss_inputs.Config, pc_loss=True)
    want.backward()
    loss, terms, grads, (oa, qa) = reference_get_loss(lab, pred)
    close = lambda g, w: abs(g - float(w.detach())) <= TERM_RTOL * max(1.0, abs(float(w.detach())))              # noqa: E731
    assert close(loss, want), (loss, float(want))
    assert close(terms["vote"], ep["vote_loss"]) and close(terms["pc"][0], ep["physical_constraints_loss"])
    assert float(terms["pc"][1]) == float(ep["collisions"]) > 0
    for i, p in enumerate(loss_inputs.prefixes()):
        for col, key in ((0, "objectness_loss"), (1, "center_loss"), (2, "heading_cls_loss"), (3, "heading_reg_loss"),
                         (4, "size_cls_loss"), (5, "size_reg_loss"), (6, "sem_cls_loss")):
            assert close(terms["box"][i, col], ep[p + key]), (p, key)
        for col, key in ((0, "quad_scores_loss"), (1, "quad_center_loss"), (2, "normal_vector_loss"), (3, "quad_size_loss")):
            assert close(terms["quad"][i, col], ep[p + key]), (p, key)
    for key, a in (("objectness_label", oa["label"]), ("objectness_mask", oa["mask"]), ("object_assignment", oa["assignment"]),
                   ("quad_label", qa["label"]), ("quad_mask", qa["mask"]), ("quad_assignment", qa["assignment"])):
        assert np.array_equal(ep["last_" + key].numpy().astype(D), a.astype(D)), key
    for k, leaf in leaves.items():
        w = np.zeros(leaf.shape) if leaf.grad is None else leaf.grad.numpy().astype(D)
        scale = max(np.abs(w).max(), 1e-6)
        assert np.abs(grads[k] - w).max() <= GRAD_RTOL * scale, (k, np.abs(grads[k] - w).max(), scale)


# ---- mutants ----------------------------------------------------------------------------------------------------------------

MUTANT_CASES = [
    ("near_le", "assign-atnear", "label"),                               # rows with e == near, bit for bit
    ("tie_last", "assign-lattice", "assignment"),
    ("numgt_le", "assign-2x257x64", "label"),
    ("pos_over_mask_count", "box-R255-h3-randn", "terms"),
    ("pos_over_mask_count", "quad-R513-h1-mixed", "terms"),
    ("obj_grad_no_weight", "box-R255-h3-randn", "objectness_scores"),
    ("obj_grad_no_weight", "quad-R256-h7", "quad_scores"),
    ("hres_grad_col0", "box-R255-h3-randn", "heading_residuals_normalized"),
    ("heading_wrong_nh", "box-R255-h3-randn", "terms"),
    ("mean_of_predicted", "box-R255-h3-randn", "size_residuals_normalized"),
    ("slope_linear", "box-R513-h3-kink", "center"),
    ("slope_linear", "quad-R257-h8-kink", "quad_size"),
    ("g_terms_head0", "box-R256-h8-pm60", "center"),
    ("g_terms_head0", "quad-R256-h7", "normal_vector"),
    ("no_scene_offset", "box-R255-h3-randn", "center"),
    ("no_scene_offset", "quad-R256-h7", "terms"),
    ("cos_grad_no_norm", "quad-R256-h7", "normal_vector"),
    ("vote_grad_last", "votes-dupvotes", "grad"),
    ("corner_signs_swapped", "pc-2x65-q5", "g_size_residuals"),
    ("not_solid_shifted", "pc-bit63", "out"),
    ("not_solid_shifted", "pc-2x65-q5", "g_center"),
    ("quad_tile_drop_partial", "pc-2x40-q257", "g_center"),
    ("quad_tile_drop_partial", "pc-1x20-q600", "g_size_residuals"),
]


@pytest.mark.parametrize("mutant,id,where", MUTANT_CASES)
def test_mutant_leaves_a_bound_or_flips_an_exact_output(mutant, id, where):
    assert {m for m, _, _ in MUTANT_CASES} == set(lr.MUTANTS)
    rat, flips, _ = run(lr.case_of(id))
    assert not lr.outside(rat) and not flips
    rat, flips, _ = run(lr.case_of(id), mutant)
    assert where in set(lr.outside(rat)) | flips, (mutant, id, lr.outside(rat), flips)


def test_one_wrong_small_entry_is_seen():
    """what a max-norm over the tensor hides: one row of 255 with its residual gradient in the wrong column"""
    inp = lr.box_inputs(lr.case_of("box-R255-h3-randn"))
    ref, bnd, _ = lr.box_reference(inp)
    good, bad = lr.box_emulate(inp), lr.box_emulate(inp, "hres_grad_col0")
    key = "heading_residuals_normalized"
    got = good["grads"][key].copy()
    row = int(np.flatnonzero((inp["label"] != 0) & (np.abs(ref["grads"][key][1]).max(1) > 0))[-1])
    got[1, row] = bad["grads"][key][1, row]
    err = np.abs(got - ref["grads"][key]).max()
    assert 0 < err <= 1.001 * np.abs(ref["grads"][key]).max()
    out = lr.outside(lr.rat({key: got}, ref["grads"], bnd["grads"]))
    assert set(out) == {key} and 1 <= out[key][1] <= 2


def test_gpu_suite_calls_every_entry_point_of_the_loss_rows():
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, "..", "omni-pq_amd", "csrc", "loss_rows.hip")).read()
    names = set(re.findall(r'extern "C" (?:int|long long) (omnipq_\w+)\(', src))
    gpu = open(os.path.join(here, "test_gpu_loss_rows_f64.py")).read()
    names -= {"omnipq_nn_distance", "omnipq_nn_distance_grad"}                   # tests/test_nn_distance.py
    assert len(names) == 10 and not {n for n in names if not re.search(rf"lib\.{n}\b", gpu)}
