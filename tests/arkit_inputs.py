"""Seeded inputs of the ARKit physical-constraint tests: the four `last_` quad predictions of a full batch of 2 Bu scenes and
the labels of its unlabelled half, as float32 numpy arrays (every value f32-representable, so the float64 restatement and the
device read the same numbers).  The labelled half of the predictions is filled with different random values, so a wrong
scene offset shows; label rows at and beyond a scene's count are NaN; `num_gt_boxes` has the count in column 0 and rubbish
in the others, so a wrong stride shows.

No decision may sit on the knife's edge: after the draw, every quad of the unlabelled half that has a margin below
REPAIR (tests/arkit_restatement.py: quad_margin) gets a new centre and new scores, until the case is clean.  With 300 quads
against 256 corners hardly any seed is clean as drawn.  tests/test_arkit_golden.py asserts the margins."""
import numpy as np

F = np.float32
# name: (Bu, Q, K2, counts, seed)
CASES = {"s": (2, 37, 7, (5, 7), 0), "m": (3, 64, 64, (1, 30, 64), 1), "q300": (2, 300, 64, (64, 17), 2)}
REPAIR = 2e-4                          # twice the margin the tests assert
COUNT_COLUMNS = 3


def quads(rng, B, Q):
    angle, length = rng.uniform(0, 2 * np.pi, (B, Q)), rng.uniform(0.5, 1.5, (B, Q))
    normal = np.stack([length * np.cos(angle), length * np.sin(angle), rng.standard_normal((B, Q))], -1)
    return {"last_quad_center": rng.uniform((-3, -3, 0), (3, 3, 2.5), (B, Q, 3)), "last_normal_vector": normal,
            "last_quad_size": rng.uniform(0.5, 3.0, (B, Q, 2)), "last_quad_scores": scores(rng, (B, Q))}


def scores(rng, shape):
    """two logits whose softmax[1] lies between 0.012 and 0.62: about half of them pass 0.1"""
    out = rng.standard_normal(shape + (2,))
    out[..., 1] = out[..., 0] + rng.uniform(-4.4, 0.5, shape)
    return out


def labels(rng, Bu, K2, counts):
    center = rng.uniform((-2.5, -2.5, 0), (2.5, 2.5, 2), (Bu, K2, 3))
    size = rng.uniform(0.3, 2.0, (Bu, K2, 3))
    nums = np.full((Bu, COUNT_COLUMNS), -7, dtype=np.int64)
    for s, n in enumerate(counts):
        center[s, n:] = np.nan
        size[s, n:] = np.nan
        nums[s, 0] = n
    return {"center_label": center.astype(F), "size_label": size.astype(F), "num_gt_boxes": nums}


def make(case, seed=None, repair=True):
    """case: a name of CASES or (Bu, Q, K2, counts); -> (predictions {last_*: (2 Bu, Q, .) float32}, unlabelled labels)"""
    Bu, Q, K2, counts = (CASES[case] if isinstance(case, str) else tuple(case))[:4]
    if seed is None:
        seed = CASES[case][4] if isinstance(case, str) else 0
    rng = np.random.default_rng([seed, Bu, Q, K2])
    pred = {k: v.astype(F) for k, v in quads(rng, 2 * Bu, Q).items()}
    unl = labels(rng, Bu, K2, counts)
    if repair:
        import arkit_restatement as R
        for _ in range(200):
            bad = R.arkit_pc(R.leaves(pred, ()), unl)[4] < REPAIR
            if not bad.any():
                break
            for s, j in zip(*np.nonzero(bad)):
                pred["last_quad_center"][Bu + s, j] = rng.uniform((-3, -3, 0), (3, 3, 2.5)).astype(F)
                pred["last_quad_scores"][Bu + s, j] = scores(rng, ())[...].astype(F)
        else:
            raise RuntimeError(f"arkit_inputs: case {case!r} seed {seed} is not clean after 200 rounds")
    return pred, unl
