"""Seeded inputs of the mean-teacher consistency tests: a student's and a teacher's end_points, the augmentation that relates
them and the size templates, as float32 numpy arrays (every value f32-representable, so the float64 restatement and the
device read the same numbers).  The seeds were chosen by scanning (tests/golden/make_golden_consistency.py --scan): at these
seeds no discrete decision of the loss is within 1e-4 of flipping (tests/test_consistency_golden.py asserts it)."""
import numpy as np

PREFIXES = ("last_", "proposal_") + tuple(f"{i}head_" for i in range(5))
GRAD_KEYS = ("center", "objectness_scores", "sem_cls_scores", "size_residuals", "quad_center", "quad_scores", "normal_vector",
             "quad_size")
NO_GRAD_KEYS = ("size_scores",)
# name: (B, K, nc, ns, seed)
CASES = {"s": (3, 37, 4, 5, 0), "m": (4, 64, 18, 18, 186), "k256": (2, 256, 18, 18, 178)}
F = np.float32


def mean_sizes(ns):
    return (0.3 + 0.05 * np.arange(ns * 3).reshape(ns, 3)).astype(F)


class Config:
    """what the loss reads of the reference's DATASET_CONFIG"""

    def __init__(self, ns):
        self.mean_size_arr = mean_sizes(ns).astype(np.float64)


def augmentation(rng, B, flips=None, identity=False):
    """flips: None random, True every flip on, False every flip off"""
    if identity:
        angle, scale = np.zeros(B), np.ones(B)
        flips = False
    else:
        angle, scale = rng.uniform(-0.5, 0.5, B), rng.uniform(0.85, 1.15, B)
    rot = np.zeros((B, 3, 3))
    rot[:, 0, 0] = rot[:, 1, 1] = np.cos(angle)
    rot[:, 0, 1] = -np.sin(angle)
    rot[:, 1, 0] = np.sin(angle)
    rot[:, 2, 2] = 1.0
    fx, fy = rng.integers(0, 2, B), rng.integers(0, 2, B)
    if flips is not None:
        fx = fy = np.full(B, int(flips))
    return {"flip_x_axis": fx.astype(np.int64), "flip_y_axis": fy.astype(np.int64), "rot_mat": rot.astype(F),
            "scale": scale.astype(F).reshape(B, 1, 1)}


def scores(rng, shape):
    """two logits whose softmax[1] lies in (0.2, 0.9)"""
    out = rng.standard_normal(shape + (2,))
    out[..., 1] = out[..., 0] + rng.uniform(-1.4, 2.2, shape)
    return out


def size_scores(rng, B, K, ns):
    """a clear winner per row: the arg-max is not a matter of the last bits"""
    out = rng.standard_normal((B, K, ns))
    np.put_along_axis(out, rng.integers(0, ns, (B, K, 1)), 4.0, 2)
    return out


def head(rng, B, K, nc, ns):
    return {"center": rng.uniform((-3, -3, 0), (3, 3, 2.5), (B, K, 3)), "objectness_scores": scores(rng, (B, K)),
            "sem_cls_scores": 2.0 * rng.standard_normal((B, K, nc)), "size_scores": size_scores(rng, B, K, ns),
            "size_residuals": 0.2 * rng.standard_normal((B, K, ns, 3)),
            "quad_center": rng.uniform((-3, -3, 0), (3, 3, 2.5), (B, K, 3)), "quad_scores": scores(rng, (B, K)),
            "normal_vector": rng.standard_normal((B, K, 3)), "quad_size": rng.uniform(0.5, 3.0, (B, K, 2))}


def unalign(e, aug):
    """the teacher's raw centres whose alignment is e (up to f32 rounding)"""
    B = e.shape[0]
    raw = np.einsum("bkj,bji->bki", e / aug["scale"].astype(np.float64).reshape(B, 1, 1), aug["rot_mat"].astype(np.float64))
    raw[..., 0] *= np.where(aug["flip_x_axis"] != 0, -1.0, 1.0)[:, None]
    raw[..., 1] *= np.where(aug["flip_y_axis"] != 0, -1.0, 1.0)[:, None]
    return raw


def lattice(rng, B, K):
    """K jittered lattice points per scene, in a random order: neighbours at least 0.5 apart"""
    side = int(np.ceil(K ** (1.0 / 3.0)))
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:K] * 0.7
    pts = np.stack([grid[rng.permutation(K)] for _ in range(B)]) + rng.uniform(-0.1, 0.1, (B, K, 3))
    return pts - np.array([0.7 * side / 2, 0.7 * side / 2, 0.0])


def rotate2(v, angle):
    out = v.copy()
    out[..., 0] = np.cos(angle) * v[..., 0] - np.sin(angle) * v[..., 1]
    out[..., 1] = np.sin(angle) * v[..., 0] + np.cos(angle) * v[..., 1]
    return out


def structured_head(rng, B, K, nc, ns, aug, mean_size):
    """The teacher is a per-scene permutation of the student plus small noise; the last quarter of the teacher's rows map
    many-to-one (some student rows are assigned two or four times, a quarter never).  About one row in seven (never the same number
    as 0.85 of the rows) deviates strongly in size, normal and quad size, so that every 0.85 quantile falls into a gap."""
    S = head(rng, B, K, nc, ns)
    T = head(rng, B, K, nc, ns)
    n_wild = B * K - (int(np.floor(0.85 * (B * K - 1))) + 1)
    scale = aug["scale"].astype(np.float64).reshape(B, 1, 1)
    for kind in ("center", "quad_center"):
        S[kind] = lattice(rng, B, K)
        perm = np.stack([rng.permutation(K) for _ in range(B)])
        q = K - K // 4
        # the last quarter: three more teacher rows for each of the first targets, then one more for each of the next ones
        extra = ([t for t in range(K // 16) for _ in range(3)] + list(range(K // 16, q)))[:K - q]
        rank = np.zeros(K, dtype=np.int64)
        for j, t in enumerate(extra):
            rank[q + j] = 1 + extra[:j].count(t)
        perm[:, q:] = perm[:, extra]
        target = np.stack([S[kind][b, perm[b]] for b in range(B)])
        S[kind] = S[kind].astype(F).astype(np.float64)
        # teacher rows that share a target lie at clearly different distances from it (squared radii at least 4e-4 apart)
        radius = rng.uniform(np.array([0.0, 0.025, 0.036, 0.045])[rank], np.array([0.015, 0.03, 0.04, 0.05])[rank], (B, K))
        direction = rng.standard_normal((B, K, 3))
        direction /= np.linalg.norm(direction, axis=-1, keepdims=True)
        T[kind] = unalign(target + radius[..., None] * direction, aug)
        wild = np.zeros(B * K, dtype=bool)
        wild[rng.permutation(B * K)[:n_wild]] = True
        wild = wild.reshape(B, K)
        take = lambda x: np.stack([x[b, perm[b]] for b in range(B)])  # noqa: E731
        if kind == "center":
            T["size_scores"] = take(S["size_scores"])
            cls = T["size_scores"].argmax(-1)
            size = mean_size.astype(np.float64)[cls] + np.take_along_axis(take(S["size_residuals"]), cls[..., None, None].repeat(3, -1),
                                                                          2)[:, :, 0]
            noise = np.where(wild[..., None], rng.choice([-1.0, 1.0], (B, K, 3)) * rng.uniform(0.5, 0.8, (B, K, 3)),
                             rng.uniform(-0.03, 0.03, (B, K, 3)))
            res = (size + noise) / scale - mean_size.astype(np.float64)[cls]
            np.put_along_axis(T["size_residuals"], cls[..., None, None].repeat(3, -1), res[:, :, None, :], 2)
            T["sem_cls_scores"] = take(S["sem_cls_scores"]) + 0.3 * rng.standard_normal((B, K, nc))
        else:
            angle = np.where(wild, rng.choice([-1.0, 1.0], (B, K)) * rng.uniform(0.6, 0.9, (B, K)), rng.uniform(-0.05, 0.05, (B, K)))
            T["normal_vector"] = rotate2(take(S["normal_vector"]), angle)
            noise = np.where(wild[..., None], rng.choice([-1.0, 1.0], (B, K, 2)) * rng.uniform(0.5, 0.8, (B, K, 2)),
                             rng.uniform(-0.03, 0.03, (B, K, 2)))
            T["quad_size"] = take(S["quad_size"]) + noise
    return S, T


def make(case, seed=None, flips=None, identity=False, structured=None):
    """-> (student end_points with the augmentation, teacher end_points, mean_size (ns, 3)): float32 / int64 numpy arrays"""
    B, K, nc, ns, case_seed = CASES[case] if isinstance(case, str) else tuple(case) + (0,)
    rng = np.random.default_rng(case_seed if seed is None else seed)
    structured = (case == "k256") if structured is None else structured
    aug = augmentation(rng, B, flips, identity)
    mean_size = mean_sizes(ns)
    S, T = dict(aug), {}
    for p in PREFIXES:
        hs, ht = structured_head(rng, B, K, nc, ns, aug, mean_size) if structured else (head(rng, B, K, nc, ns),
                                                                                      head(rng, B, K, nc, ns))
        if identity:
            ht = hs
        S.update({p + k: v.astype(F) for k, v in hs.items()})
        T.update({p + k: v.astype(F) for k, v in ht.items()})
    return S, T, mean_size
