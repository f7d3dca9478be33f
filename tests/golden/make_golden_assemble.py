"""Generate tests/golden/assemble.npz: outputs of the REFERENCE's own dataset items

    ScannetDetectionDataset.__getitem__     scannet/scannet_detection_dataset.py:86-312
    ARKitSceneDataset.__getitem__           ARKitScenes/arkitscenes_dataset.py:83-233

on the seeded scenes of tests/assemble_inputs.py.  DATA only.  Neither module can be imported here (their import blocks pull
in torch datasets, trimesh, IPython and files of the real datasets); no stand-in of the code under test is made: the two
methods and the helpers they call (`random_sampling`, `rotz`, `rotate_aligned_boxes`, `rotate_quad`) are taken out of the
reference files IN PLACE with `ast` and executed against the real numpy.  The scene arrives through a patched `np.load` and a
stand-in `get_quads_fn`; `DC` is tests/assemble_inputs.py:Config (the dataset's class list, a synthetic mean-size table).

`np.random` and `random` are seeded before the call and the same seed is replayed afterwards, in the order the method draws,
to recover the two choice arrays, the flips, the angle and the scale.  The seed of a case is the first one from its start value
whose flips are the ones tests/assemble_inputs.py:CASES asks for and whose smallest instance -> box argmin margin exceeds
MARGIN (the bound is never widened: the generator is reseeded).

    python tests/golden/make_golden_assemble.py
"""
import ast
import copy
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.environ.get("OMNIPQ_REFERENCE", "/root/reference")

import numpy as np  # noqa: E402

import assemble_inputs as A  # noqa: E402

MARGIN = 1e-6


def take(path, names, ns, method_of=None):
    """function definitions `names` of the file (methods of class `method_of` when given) and the module's constant
    assignments, executed in `ns`"""
    tree = ast.parse(open(path).read(), filename=path)
    scope = tree.body
    consts = [n for n in tree.body if isinstance(n, ast.Assign) and isinstance(n.value, (ast.Constant, ast.Dict))]
    if method_of:
        scope = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == method_of][0].body
    body = [n for n in scope if isinstance(n, ast.FunctionDef) and n.name in names]
    assert {n.name for n in body} == set(names)
    exec(compile(ast.Module(body=consts + body, type_ignores=[]), path, "exec"), ns)


def helpers():
    pc_util, model_util = {"np": np}, {"np": np}
    take(os.path.join(REF, "utils", "pc_util.py"), ["random_sampling", "rotz"], pc_util)
    take(os.path.join(REF, "scannet", "model_util_scannet.py"), ["rotate_aligned_boxes", "rotate_quad"], model_util)
    return {"np": np, "os": os, "random": random, "pc_util": types.SimpleNamespace(**pc_util), "DC": A.Config,
            "rotate_aligned_boxes": model_util["rotate_aligned_boxes"], "rotate_quad": model_util["rotate_quad"]}


def serve(files):
    """np.load that answers from `files` by the end of the path (a fresh copy each time: the methods write into what they load)"""
    def load(path, **kw):
        for tail, value in files.items():
            if str(path).endswith(tail):
                return copy.deepcopy(value)
        raise FileNotFoundError(path)
    return load


def run_scannet(ns, sc, k, augment, seed):
    me = types.SimpleNamespace(scan_names=["scene"], data_path="/data", num_points=k, use_color=False, use_height=True,
                               augment=augment, start_idx=0,
                               get_quads_fn=lambda name: (np.array(sc["rectangles"], np.float64), sc["total_quad_num"],
                                                          np.array(sc["horizontal_quads"], np.float64)))
    files = {"_vert.npy": sc["vertices"], "_ins_label.npy": sc["instance_labels"], "_sem_label.npy": sc["semantic_labels"],
             "_bbox.npy": sc["boxes"], ".normal.npy": sc["normals"]}
    real = np.load
    np.load = serve(files)
    try:
        np.random.seed(seed)
        random.seed(seed)
        return ns["__getitem__"](me, 0)
    finally:
        np.load = real


def run_arkit(ns, sc, k, augment, seed):
    me = types.SimpleNamespace(scan_names=["scene"], data_path="/data", num_points=k, augment=augment, split_set="train")
    files = {"_pc.npy": sc["vertices"], "_normal.npy": sc["normals"],
             "_bbox.npy": np.array({"bboxes": np.array(sc["boxes"]), "types": list(sc["types"])}, dtype=object)}
    real = np.load
    np.load = serve(files)
    try:
        np.random.seed(seed)
        random.seed(seed)
        return ns["__getitem__"](me, 0)
    finally:
        np.load = real


def replay(ns, n, k, augment, seed, arkit):
    """the draws of the method, in its order -> (choices, ema_choices, flip_x, flip_y, rot_mat, scale)"""
    np.random.seed(seed)
    random.seed(seed)
    first = np.random.choice(n, k, replace=n < k)
    second = np.random.choice(n, k, replace=n < k)
    choices, ema = (first, second) if arkit else (second, first)
    if not augment:
        return choices, ema, False, False, np.identity(3), 1.0
    flip_x = np.random.random() > 0.5
    flip_y = np.random.random() > 0.5
    angle = (np.random.random() * np.pi / 18) - np.pi / 36
    angle += random.choice([0, 1, 2, 3]) * np.pi / 2
    rot = ns["pc_util"].rotz(angle)
    scale = np.random.random() * 0.3 + 0.85
    return choices, ema, bool(flip_x), bool(flip_y), rot, scale


def margins(sc, item, choices):
    """per voting instance: second smallest minus smallest squared distance of its centre to the 64 label centres, from the
    reference's outputs alone"""
    ins = sc["instance_labels"][choices]
    x = item["point_clouds"][:, :3]
    gt = item["center_label"].astype(np.float64)
    out = []
    for g in np.unique(ins):
        ind = np.where(ins == g)[0]
        if item["vote_label_mask"][ind[0]] == 0:
            continue
        centre = 0.5 * (x[ind].min(0) + x[ind].max(0))
        two = np.sort(((centre - gt) ** 2).sum(-1))[:2]
        out.append(two[1] - two[0])
    return np.array(out, np.float64)


def main():
    out = {}
    scannet, arkit = helpers(), helpers()
    take(os.path.join(REF, "scannet", "scannet_detection_dataset.py"), ["__getitem__"], scannet, "ScannetDetectionDataset")
    take(os.path.join(REF, "ARKitScenes", "arkitscenes_dataset.py"), ["__getitem__"], arkit, "ARKitSceneDataset")
    for name, (gseed, n, k, _, _, _, _, augment, want) in A.CASES.items():
        sc = A.scene(name)
        is_arkit = name == "arkit"
        ns = arkit if is_arkit else scannet
        for seed in range(100 * gseed, 100 * gseed + 100):
            choices, ema, fx, fy, rot, scale = replay(ns, n, k, augment, seed, is_arkit)
            if (fx, fy) != want:
                continue
            item = (run_arkit if is_arkit else run_scannet)(ns, sc, k, augment, seed)
            marg = np.zeros(0) if is_arkit else margins(sc, item, choices)
            tie_free = marg[marg > 0] if name == "thin" else marg          # `thin` has no box: every distance ties
            if tie_free.size == 0 or tie_free.min() > MARGIN:
                break
        else:
            raise SystemExit(f"{name}: no seed gives flips {want} and margins above {MARGIN}")
        out[f"{name}.seed"] = np.array([seed], np.int64)
        out[f"{name}.choices"], out[f"{name}.ema_choices"] = choices.astype(np.int32), ema.astype(np.int32)
        out[f"{name}.flips"] = np.array([fx, fy], np.int64)
        out[f"{name}.param_rot_mat"], out[f"{name}.param_scale"] = np.asarray(rot, np.float64), np.array([scale], np.float64)
        out[f"{name}.margins"] = marg
        for key, val in item.items():
            if key != "scan_name":
                out[f"{name}.out.{key}"] = np.asarray(val)
        print(name, "seed", seed, "flips", fx, fy, "scale", scale, "min margin", marg.min() if marg.size else None)
    path = os.path.join(HERE, "assemble.npz")
    np.savez_compressed(path, **out)
    print("wrote assemble.npz:", os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
