"""float64 / numpy-f32 restatement of the four stages of include/omnipq_normals.h, operation by operation, and the criteria
the GPU tests hold csrc/point_normals.hip to (tests/test_gpu_normals.py) -- shared with tests/test_normals_reference.py, which
shows on the CPU that each criterion can fail (mutants of this restatement).

Neighbours are found by brute force: every f32 d2 with the contraction pattern of csrc/common.h: sumsq3, a stable sort per
query (ties: the lower index first).
"""
import numpy as np

F32, F64 = np.float32, np.float64


def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, for float32 arrays: the product is exact in f64, the f64 sum is made round-to-odd
    with the error term of TwoSum, so the final rounding to f32 sees the exact sum's sticky bit (no double rounding)."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    nudge = (e != 0) & even & np.isfinite(s)
    s = np.where(nudge, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def sumsq3(a, b, c):
    """fma(c, c, fma(a, a, fl(b * b))) in f32 (csrc/common.h)"""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    return fma32(c, c, fma32(a, a, b * b))


def dist2(queries, xyz):
    """(m, 3), (n, 3) f32 -> (m, n) f32 on d = query - point"""
    q, p = np.asarray(queries, F32), np.asarray(xyz, F32)
    d = q[:, None, :] - p[None, :, :]
    return sumsq3(d[..., 0], d[..., 1], d[..., 2])


def knn(xyz, k, queries=None, skip_self=False, chunk=256):
    """-> idx (m, k) int32, dist2 (m, k) f32: the k smallest (d2, index) per query, ascending; -1 / +inf behind the n-th.
    skip_self (a MUTANT): the query's own index is left out (queries=None only)."""
    xyz = np.ascontiguousarray(xyz, F32)
    q = xyz if queries is None else np.ascontiguousarray(queries, F32)
    m, n = q.shape[0], xyz.shape[0]
    idx = np.full((m, k), -1, np.int32)
    d2o = np.full((m, k), np.inf, F32)
    kk = min(k, n - (1 if skip_self else 0))
    for c0 in range(0, m, chunk):
        d2 = dist2(q[c0:c0 + chunk], xyz) if n else np.zeros((min(chunk, m - c0), 0), F32)
        if skip_self:
            d2[np.arange(d2.shape[0]), np.arange(c0, c0 + d2.shape[0])] = np.inf
        order = np.argsort(d2, axis=1, kind="stable")[:, :max(kk, 0)]
        idx[c0:c0 + chunk, :kk] = order
        d2o[c0:c0 + chunk, :kk] = np.take_along_axis(d2, order, 1)
    return idx, d2o


JACOBI_SWEEPS = 10


def _rotate(a, v, p, q, r):
    """one Jacobi rotation in the plane (p, q) on dicts of arrays a[(i, j)], i <= j, and v[(i, j)]"""
    key = lambda i, j: (min(i, j), max(i, j))
    apq, app, aqq = a[key(p, q)], a[(p, p)], a[(q, q)]
    on = apq != 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        t = np.where(theta >= 0.0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        new = {(p, p): app - t * apq, (q, q): aqq + t * apq, key(p, q): np.zeros_like(apq)}
        arp, arq = a[key(r, p)], a[key(r, q)]
        new[key(r, p)] = c * arp - s * arq
        new[key(r, q)] = s * arp + c * arq
        for kk, val in new.items():
            a[kk] = np.where(on, val, a[kk])
        for i in range(3):
            vp, vq = v[(i, p)], v[(i, q)]
            v[(i, p)] = np.where(on, c * vp - s * vq, vp)
            v[(i, q)] = np.where(on, s * vp + c * vq, vq)


def plane_fit(xyz, idx, mean_f32=False):
    """-> (normals (n, 3) f32 with the canonical sign, the unrounded f64 eigenvector (n, 3), eigenvalues (n, 3) ascending).
    mean_f32 (a MUTANT): the mean is accumulated in float32."""
    xyz = np.asarray(xyz, F32)
    n_rows, k = idx.shape
    ok = (idx >= 0) & (idx < xyz.shape[0])
    safe = np.where(ok, idx, 0)
    acc = F32 if mean_f32 else F64
    s = np.zeros((n_rows, 3), acc)
    for j in range(k):                                        # row order
        s = s + np.where(ok[:, j:j + 1], xyz[safe[:, j]].astype(acc), acc(0))
    cnt = ok.sum(1).astype(F64)
    with np.errstate(all="ignore"):
        mean = np.where(cnt[:, None] > 0, s.astype(F64) / cnt[:, None], 0.0) if not mean_f32 else \
            np.where(cnt[:, None] > 0, (s / cnt[:, None].astype(F32)).astype(F64), 0.0)
    a = {kk: np.zeros(n_rows, F64) for kk in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))}
    for j in range(k):
        d = np.where(ok[:, j:j + 1], xyz[safe[:, j]].astype(F64) - mean, 0.0)
        for (i0, i1) in a:
            a[(i0, i1)] = a[(i0, i1)] + d[:, i0] * d[:, i1]
    with np.errstate(all="ignore"):
        for kk in a:
            a[kk] = np.where(cnt > 0, a[kk] / cnt, 0.0)
    v = {(i, j): np.full(n_rows, 1.0 if i == j else 0.0) for i in range(3) for j in range(3)}
    for _ in range(JACOBI_SWEEPS):
        _rotate(a, v, 0, 1, 2)
        _rotate(a, v, 0, 2, 1)
        _rotate(a, v, 1, 2, 0)
    lam = np.stack([a[(0, 0)], a[(1, 1)], a[(2, 2)]], 1)
    col = np.argmin(lam, 1)                                   # the first among equal ones
    rows = np.arange(n_rows)
    vec = np.stack([np.stack([v[(i, j)] for j in range(3)], 1)[rows, col] for i in range(3)], 1)
    out = vec.astype(F32)
    big = out[rows, np.argmax(np.abs(out), 1)]                # the first among equal magnitudes
    out = np.where(big[:, None] < 0, -out, out)
    vec = np.where(big[:, None] < 0, -vec, vec)
    return out, vec, np.sort(lam, 1)


def smooth_step(normals, idx, vote_ge=False, unaligned=False):
    """one step of stage 3 -> (f32 output, the votes s_ij (n, k) int8 with 0 for skipped entries).
    vote_ge / unaligned (MUTANTS): `>=` for `>`; every s_ij = +1."""
    nrm = np.asarray(normals, F32)
    ok = (idx >= 0) & (idx < nrm.shape[0])
    safe = np.where(ok, idx, 0)
    me = nrm.astype(F64)
    t = np.zeros_like(me)
    votes = np.zeros(idx.shape, np.int8)
    for j in range(idx.shape[1]):
        o = nrm[safe[:, j]].astype(F64)
        dot = (me[:, 0] * o[:, 0] + me[:, 1] * o[:, 1]) + me[:, 2] * o[:, 2]
        pos = (dot >= 0) if vote_ge else (dot > 0)
        if unaligned:
            pos = np.ones_like(pos)
        sgn = np.where(ok[:, j], np.where(pos, 1.0, -1.0), 0.0)
        votes[:, j] = sgn.astype(np.int8)
        t = t + sgn[:, None] * o
    zero = (t == 0).all(1)
    with np.errstate(all="ignore"):
        length = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
        out = (t / length[:, None]).astype(F32)
    return np.where(zero[:, None], nrm, out), votes


def orient_flips(xyz, normals, centre):
    """stage 4 -> (flip mask, the f64 dot)"""
    p, nrm, c = np.asarray(xyz, F32).astype(F64), np.asarray(normals, F32).astype(F64), np.asarray(centre, F64)
    dot = ((p[:, 0] - c[0]) * nrm[:, 0] + (p[:, 1] - c[1]) * nrm[:, 1]) + (p[:, 2] - c[2]) * nrm[:, 2]
    return dot < 0, dot


def orient(xyz, normals, centre):
    flip, _ = orient_flips(xyz, normals, centre)
    return np.where(flip[:, None], -np.asarray(normals, F32), np.asarray(normals, F32))


def view_centre(xyz):
    """(mean x, mean y, (max z + mean z) / 2) in f64 (scannet/compute_normal_for_pc.py:34-35)"""
    p = np.asarray(xyz, F32).astype(F64)
    c = p.mean(0)
    c[2] = (p[:, 2].max() + c[2]) / 2
    return c


def estimate(xyz, k, iters, centre, idx=None):
    idx = knn(xyz, k)[0] if idx is None else idx
    nrm = plane_fit(xyz, idx)[0]
    for _ in range(iters):
        nrm = smooth_step(nrm, idx)[0]
    return orient(xyz, nrm, centre)


# ---- the criteria -------------------------------------------------------------------------------------------------------
def angle(a, b):
    """unsigned angle between the lines of a and b, atan2(|a x b|, |a . b|) in f64: exact where arccos of a dot of f32 unit
    vectors reads 2e-2 degrees for vectors that agree to 1e-7 rad"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), np.abs((a * b).sum(-1)))


U64 = 2.0 ** -53
THETA_STORE = 2.0 ** -24 * (1 + 2.0 ** -20)      # rounding a unit vector to f32 moves each component by <= 2^-24 |component|


def plane_fit_ops(k):
    """c of the plane-fit bound, counted from plane_fit_kernel: an entry of C carries, per unit roundoff u and relative to
    sum |d_a d_b| / cnt <= trace(C) / 2 ... trace(C): 2 (the subtraction of the mean in each factor) + 1 (the product) +
    (k - 1) (the sum) + 1 (the division) = k + 3; nine entries bound the 2-norm of the perturbation by 3 (k + 3) u trace(C).
    The mean's own error enters squared (the first-order term sums to zero) and is below one more unit.  Each of the
    3 * JACOBI_SWEEPS rotations is an orthogonal similarity applied with <= 8 roundings per touched entry: 8 u |A| each.  An
    eigenvector of a simple eigenvalue turns by <= 2 |dC| / gap (Davis-Kahan, sin 2 theta form).  The restatement carries the
    same bound, hence the last factor 2."""
    return 2 * 2 * (3 * (k + 4) + 8 * 3 * JACOBI_SWEEPS)


def plane_fit_bound(eig, k):
    """theta <= theta_f32-store + c 2^-53 trace(C) / (lambda_1 - lambda_0), per point (inf where the gap is zero)"""
    with np.errstate(all="ignore"):
        return THETA_STORE + plane_fit_ops(k) * U64 * eig.sum(1) / (eig[:, 1] - eig[:, 0])


def eig_bound(eig, k):
    """|lambda - lambda_ref| <= c 2^-53 trace(C), per point (Weyl: an eigenvalue moves by at most |dC|; the c above).  This is
    the criterion that sees a mean of lower precision: its error enters C squared, far below the f32 store of the normal but
    orders of magnitude above this."""
    return plane_fit_ops(k) * U64 * eig.sum(1)


def plane_fit_excluded(eig):
    """points whose smallest two eigenvalues are not separated: (lambda_1 - lambda_0) < 1e-6 lambda_2"""
    return (eig[:, 1] - eig[:, 0]) < 1e-6 * eig[:, 2]


def canonical(normals):
    """the component of largest magnitude (the first among equal ones) is positive"""
    nrm = np.asarray(normals)
    big = nrm[np.arange(nrm.shape[0]), np.argmax(np.abs(nrm), 1)]
    return big > 0


def ulp_distance(a, b):
    """per element, in units of the f32 spacing at the reference value b"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(b), np.finfo(F32).tiny)).astype(F64)


# ---- the named inputs ---------------------------------------------------------------------------------------------------
def room(n, seed=0):
    """one synth.room_scene cloud (n, 3) f32"""
    import synth
    return synth.make_clouds(seed, 1, n)[0].numpy()


def smooth_inputs(idx, seed=0):
    """random unit f32 normals on the rows `idx` (n, k >= 2) plus what the rows of a k-NN never show: rows with -1 entries
    (the first ten lose their last three), a zero-sum row (row 0: two opposite normals, both at dot == 0, so t = 0 and the
    normal is kept) and a vote at dot == 0 next to the point's own (row 3: `>` sends it to -1)."""
    rng = np.random.RandomState(seed)
    n, _ = idx.shape
    nrm = rng.standard_normal((n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
    idx = idx.copy()
    idx[:10, -3:] = -1
    nrm[0], nrm[1], nrm[2] = (0, 0, 1), (1, 0, 0), (-1, 0, 0)
    idx[0, :] = -1
    idx[0, :2] = (1, 2)
    nrm[3], nrm[4] = (0, 1, 0), (1, 0, 0)
    idx[3, :] = -1
    idx[3, :2] = (3, 4)
    return nrm, idx
