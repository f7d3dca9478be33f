"""numpy / float64 restatement of omnipq_layout_f1 (include/omnipq_eval.h): the counts of the reference's
QUADAPCalculator.compute_F1 (models/ap_helper_pq.py:647-736) per scene, as rows [tp_wall, fp, npos, tp_horizontal].

    layout_f1(count_f1, verts4, gt_verts4, num_total, horizontal, same_thres=0.40, mutant=None, num_gt=None, seen=None)

mutant: one deliberate misreading of the rule (MUTANTS); tests/test_layout_f1_restatement.py shows that each one changes the
counts of an input built for it (mutant_input), so the inputs the kernel is checked on can tell the rule from its neighbours.
seen: a list that receives every distance that was compared with the threshold -- all of them, not only those in front of an
early exit -- for the tests' guard that none lies at the threshold.
Below the restatement: the inputs the CPU and GPU tests share (random_scenes, MERGE_CASES, boundary_scene, mutant_input) and the
list form the host calculator takes (to_lists)."""
import numpy as np

SAME_THRES = 0.40
MUTANTS = ("swap_3210",          # the swapped order taken as [3, 2, 1, 0]
           "strict",             # `<` at the threshold
           "any_corner",         # any corner within reach instead of all four
           "num_gt",             # the list cut at num_gt_quads instead of num_total_quads
           "every_count",        # ceiling and floor scored for every quad count (the first four entries)
           "skip_padding",       # the all-zero rows of `horizontal` skipped
           "replace_merged",     # a merged corner replaces the entry it merged with instead of being appended
           "last_match")         # the midpoint is taken with the LAST entry within reach instead of the first
f32 = np.float32


def dist(a, b, seen=None):
    """sqrt((dx dx + dy dy) + dz dz) of f32 corners widened to f64, over the leading axes"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32
    with np.errstate(over="ignore", invalid="ignore"):
        d = a.astype(np.float64) - b.astype(np.float64)
        out = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    if seen is not None:
        seen.extend(np.ravel(out).tolist())
    return out


def near(d, thr, mutant=None):
    with np.errstate(invalid="ignore"):
        return d < thr if mutant == "strict" else d <= thr          # a NaN never passes


def match_orders(p, quads, thr=SAME_THRES, mutant=None, seen=None):
    """p (..., 4, 3) against quads (n, 4, 3) -> (does some quad match in the same order, does some quad match in the swapped
    order), each of p's leading shape"""
    p = np.asarray(p, f32)
    quads = np.asarray(quads, f32).reshape(-1, 4, 3)
    if len(quads) == 0:
        none = np.zeros(p.shape[:-2], bool)
        return none, none
    order = [3, 2, 1, 0] if mutant == "swap_3210" else [1, 0, 3, 2]
    reduce = np.any if mutant == "any_corner" else np.all
    same = reduce(near(dist(p[..., None, :, :], quads, seen), thr, mutant), axis=-1)
    swapped = reduce(near(dist(p[..., None, :, :], quads[:, order], seen), thr, mutant), axis=-1)
    return same.any(-1), swapped.any(-1)


def correct(p, quads, thr=SAME_THRES, mutant=None, seen=None):
    same, swapped = match_orders(p, quads, thr, mutant, seen)
    return same | swapped


def ceiling_and_floor(quads, thr=SAME_THRES, mutant=None, seen=None):
    """-> (ceiling entries, floor entries) of get_ceiling_and_floor on quads (n, 4, 3) f32: lists of (3,) f32 corners"""
    out = []
    for side in (0, 2):
        entries = []
        for quad in np.asarray(quads, f32).reshape(-1, 4, 3):
            for i in (side, side + 1):
                c = quad[i]
                hits = [e for e in range(len(entries)) if near(dist(entries[e], c, seen), thr, mutant)]
                if not hits:
                    entries.append(c)
                    continue
                e = hits[-1] if mutant == "last_match" else hits[0]
                with np.errstate(over="ignore", invalid="ignore"):
                    mid = ((entries[e] + c) / f32(2)).astype(f32)            # the sum is rounded to f32, the halving is exact
                if mutant == "replace_merged":
                    entries[e] = mid
                else:
                    entries.append(mid)
        out.append(entries)
    return out


def layout_f1(count_f1, verts4, gt_verts4, num_total, horizontal, same_thres=SAME_THRES, mutant=None, num_gt=None, seen=None):
    """-> (b, 4) int32 rows [tp_wall, fp, npos, tp_horizontal].  count_f1 (b), verts4 (b, k, 4, 3) f32, gt_verts4 (b, g, 4, 3)
    f32, num_total (b, cols) integers, horizontal (b, h, 4, 3) f32; num_gt (b, cols) only for the mutant that reads it."""
    assert mutant is None or mutant in MUTANTS
    verts4, gt_verts4, horizontal = (np.asarray(a) for a in (verts4, gt_verts4, horizontal))
    assert verts4.dtype == gt_verts4.dtype == horizontal.dtype == np.float32
    b, k = verts4.shape[:2]
    g, h = gt_verts4.shape[1], horizontal.shape[1]
    limit = np.asarray(num_gt if mutant == "num_gt" else num_total).reshape(b, -1)
    rows = np.zeros((b, 4), np.int32)
    for s in range(b):
        gt = [gt_verts4[s, j] for j in range(g) if j < limit[s, min(j, limit.shape[1] - 1)]]
        gt = np.asarray(gt, f32).reshape(-1, 4, 3)
        n = min(max(int(count_f1[s]), 0), k)
        tp = int(correct(verts4[s, :n], gt, same_thres, mutant, seen).sum())
        tp_h = 0
        if n == 2 or (mutant == "every_count" and n >= 2):
            hz = horizontal[s]
            if mutant == "skip_padding":
                hz = hz[np.any(hz.reshape(h, -1) != 0, axis=1)]
            for entries in ceiling_and_floor(verts4[s, :n], same_thres, mutant, seen):
                if len(entries) == 4 or (mutant == "every_count" and len(entries) >= 4):
                    tp_h += bool(correct(np.stack(entries[:4]), hz, same_thres, mutant, seen))
        rows[s] = (tp, n - tp, len(gt), tp_h)
    return rows


def layout_f1_scene(sc, mutant=None, seen=None):
    """layout_f1 on a dict of the generators below (its optional "same_thres" included)"""
    return layout_f1(sc["count_f1"], sc["verts4"], sc["gt_verts4"], sc["num_total"], sc["horizontal"],
                     sc.get("same_thres", SAME_THRES), mutant=mutant, num_gt=sc["num_gt"], seen=seen)


def f1_of(counts, calculated):
    """compute_F1's closing expression in Python floats; counts = (tp_wall, fp, npos, tp_horizontal, ...)"""
    tp_wall, fp, npos, tp_h = (int(v) for v in counts[:4])
    tp = tp_wall + (tp_h if calculated else 0)
    p = tp / max((tp + fp), 1e-6)
    r = tp / npos
    return 2.0 * p * r / max((p + r), 1e-6)


# -------------------------------------------------------------------------------------------------------------- inputs
def to_lists(count_f1, verts4, gt_verts4, num_total, horizontal):
    """the three lists QUADAPCalculator.step takes for the F1: predicted corners, ground-truth corners, horizontal quads"""
    b, k = verts4.shape[:2]
    nt = np.asarray(num_total).reshape(b, -1)
    pred = [[verts4[s, j] for j in range(min(max(int(count_f1[s]), 0), k))] for s in range(b)]
    gt = [[gt_verts4[s, j] for j in range(gt_verts4.shape[1]) if j < nt[s, min(j, nt.shape[1] - 1)]] for s in range(b)]
    return pred, gt, [horizontal[s] for s in range(b)]


def wall(rs, width=None):
    """a vertical rectangle in get_verts' corner order: 0, 1 the upper edge, 2, 3 the lower edge"""
    a = rs.rand(2) * 6.0
    t = rs.rand() * 2 * np.pi
    w = 0.9 + 2.0 * rs.rand() if width is None else width
    c = a + w * np.array([np.cos(t), np.sin(t)])
    lo, hi = 0.1 * rs.rand(), 2.2 + 0.5 * rs.rand()
    return np.array([[a[0], a[1], hi], [c[0], c[1], hi], [a[0], a[1], lo], [c[0], c[1], lo]], f32)


def random_scenes(seed, b, k, g, cols=1, h=4, family="walls", counts=None):
    """Seeded scenes whose predicted corners are ground-truth corners plus noise on the scale of the threshold, so that correct
    and incorrect quads both occur, some of them in the swapped corner order.  family "walls": any number of quads per scene;
    "two_quads": two quads per scene and, in `horizontal`, the ceiling and floor they span, displaced by noise of the same
    scale.  -> dict of arrays (count_f1, verts4, gt_verts4, num_total, num_gt, horizontal)."""
    rs = np.random.RandomState(seed)
    gt = np.stack([np.stack([wall(rs) for _ in range(g)]) for _ in range(b)]) if g else np.zeros((b, 0, 4, 3), f32)
    n_total = rs.randint(0, g + 1, size=b) if g else np.zeros(b, np.int64)
    if g and b:
        n_total[0] = g
    verts = (rs.rand(b, k, 4, 3) * 6).astype(f32)
    for s in range(b):
        for j in range(k):
            if g == 0 or rs.rand() < 0.15:
                continue                                                  # a quad that resembles nothing
            q = gt[s, rs.randint(0, g)].copy()
            if rs.rand() < 0.4:
                q = q[[1, 0, 3, 2]]
            scale = (0.02, 0.15, 0.25)[rs.randint(0, 3)]
            verts[s, j] = q + (scale * rs.randn(4, 3)).astype(f32)
    if counts is None:
        counts = 2 * np.ones(b, np.int64) if family == "two_quads" else rs.randint(0, k + 1, size=b)
    counts = np.asarray(counts, np.int32)
    horizontal = np.zeros((b, h, 4, 3), f32)
    for s in range(b):
        if h >= 2 and k >= 2:
            a, c = verts[s, 0], verts[s, 1]
            noise = (0.15 * rs.randn(2, 4, 3)).astype(f32)
            horizontal[s, 0] = np.stack([a[0], a[1], c[0], c[1]]) + noise[0]
            horizontal[s, 1] = np.stack([a[3], a[2], c[3], c[2]]) + noise[1]          # the floor in the swapped order
    num_total = np.repeat(n_total[:, None], cols, axis=1).astype(np.int64)
    num_gt = np.maximum(num_total - 2, 0)
    return dict(count_f1=counts, verts4=verts, gt_verts4=gt.astype(f32), num_total=num_total, num_gt=num_gt,
                horizontal=horizontal)


def scene(quads, gt=(), horizontal=(), num_total=None, num_gt=None, h=None):
    """one scene from explicit corner lists"""
    quads = np.asarray(quads, f32).reshape(-1, 4, 3)
    gt = np.asarray(gt, f32).reshape(-1, 4, 3)
    hz = np.asarray(horizontal, f32).reshape(-1, 4, 3)
    if h is not None:
        hz = np.concatenate([hz, np.zeros((h - len(hz), 4, 3), f32)])
    nt = len(gt) if num_total is None else num_total
    return dict(count_f1=np.array([len(quads)], np.int32), verts4=quads[None], gt_verts4=gt[None],
                num_total=np.array([[nt]], np.int64), num_gt=np.array([[nt if num_gt is None else num_gt]], np.int64),
                horizontal=hz[None])


def quad_at(c0, c1, lo=0.0, hi=2.5):
    """the wall over the segment c0 -> c1 (x, y): corners 0, 1 at height hi, 2, 3 at height lo"""
    return np.array([[c0[0], c0[1], hi], [c1[0], c1[1], hi], [c0[0], c0[1], lo], [c1[0], c1[1], lo]], f32)


def boundary_scene(passes):
    """Exactly representable distances at the threshold: the ground-truth corners at the origin, every predicted corner offset
    along one axis by the largest f32 not above 0.4 (passes: sqrt(x x) == x exactly in f64) or by f32(0.4) > 0.4 (fails)."""
    x = np.nextafter(f32(0.4), f32(0)) if passes else f32(0.4)
    assert (float(x) <= 0.4) == passes and float(np.nextafter(x, f32(1))) > 0.4
    quad = np.zeros((4, 3), f32)
    for i in range(4):
        quad[i, i % 3] = x if i % 2 == 0 else -x
    return scene([quad], gt=[np.zeros((4, 3), f32)])


def _merge_cases():
    far = quad_at((5.0, 5.0), (8.0, 5.0))
    cases = {
        # name: (quad 0, quad 1, the ceiling entries expected, as x, y of the four entries)
        "no_merge": (quad_at((0, 0), (3, 0)), far, [(0, 0), (3, 0), (5, 5), (8, 5)]),
        "shared_corner": (quad_at((0, 0), (3, 0)), quad_at((3.25, 0), (3.25, 4)), [(0, 0), (3, 0), (3.125, 0), (3.25, 4)]),
        "narrow_quad": (quad_at((0, 0), (0.25, 0)), far, [(0, 0), (0.125, 0), (5, 5), (8, 5)]),
        "two_in_reach": (quad_at((0, 0), (0.5, 0)), quad_at((0.25, 0), (8, 5)), [(0, 0), (0.5, 0), (0.125, 0), (8, 5)]),
        # 0.5 is out of reach of the corner at 0 and within reach of the midpoint 0.125 listed behind it
        "midpoint_only": (quad_at((0, 0), (0.25, 0)), quad_at((0.5, 0), (8, 5)),
                          [(0, 0), (0.125, 0), (0.3125, 0), (8, 5)]),
    }
    return cases


MERGE_CASES = _merge_cases()


def merge_scene(name, shift=0.125):
    """The two quads of MERGE_CASES[name] with `horizontal` holding the expected ceiling (row 0) and floor (row 2, swapped
    order), each displaced by `shift` along x: within reach of the expected entries up to 0.4, out of reach beyond."""
    q0, q1, want = MERGE_CASES[name]
    shift = np.array([shift, 0, 0], f32)
    ceiling = np.array([(x, y, 2.5) for x, y in want], f32) + shift
    floor = np.array([(x, y, 0.0) for x, y in want], f32)[[1, 0, 3, 2]] + shift
    hz = np.zeros((4, 4, 3), f32)
    hz[0], hz[2] = ceiling, floor
    return scene([q0, q1], gt=[q0], horizontal=hz)


def mutant_input(mutant):
    """a scene on which the rule and `mutant` give different rows"""
    w = quad_at((0, 0), (3, 0))
    if mutant == "swap_3210":                       # a quad in the order [1, 0, 3, 2]: correct; [3, 2, 1, 0] is another quad
        return scene([w[[1, 0, 3, 2]]], gt=[w])
    if mutant == "strict":                          # every distance is exactly the threshold, here 0.5 (0.40 is no f32)
        q = w.copy()
        q[:, 0] += f32(0.5)
        return dict(scene([q], gt=[w]), same_thres=0.5)
    if mutant == "any_corner":                      # one corner right, three far off
        q = w.copy()
        q[1:] += f32(1.0)
        return scene([q], gt=[w])
    if mutant == "num_gt":                          # the quad matches the row between num_gt and num_total
        other = quad_at((5, 5), (5, 9))
        return scene([w], gt=[other, w], num_total=2, num_gt=1)
    if mutant == "every_count":                     # three quads whose first two span the ceiling in `horizontal`
        s = merge_scene("no_merge")
        q = np.concatenate([s["verts4"][0], quad_at((20, 20), (24, 20))[None]])
        return dict(s, count_f1=np.array([3], np.int32), verts4=q[None])
    if mutant == "skip_padding":                    # ceiling corners all within reach of the origin: a zero row matches
        a = quad_at((0.125, 0), (0, 0.125), lo=-0.125, hi=0.125)
        c = quad_at((-0.125, 0), (0, -0.125), lo=-0.125, hi=0.125)
        return scene([a, c], gt=[w], horizontal=[], h=4)
    if mutant == "replace_merged":
        return merge_scene("shared_corner")
    if mutant == "last_match":                      # the first midpoint is 0.125, the last 0.375: only the first reaches -0.1875
        return merge_scene("two_in_reach", shift=-0.3125)
    raise KeyError(mutant)
