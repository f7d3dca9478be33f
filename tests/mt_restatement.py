"""The mean-teacher consistency loss restated in float64 torch on the CPU, from its mathematics (include/omnipq_semi.h):
align, assign, clip, the object and quad terms, the weighted sums per prefix, the means over the prefixes.  It uses
F.cosine_similarity, F.kl_div and torch.quantile themselves, reads no file of the reference, and returns next to the ten
terms every discrete decision it took (ind1, ind2, the arg-max classes, the masks) and how far each was from flipping."""
import torch
import torch.nn.functional as F

CLIP = 0.85
TERMS = ("center_consistency_loss", "class_consistency_loss", "size_consistency_loss", "consistency_loss",
         "quad_center_consistency_loss_sum", "quad_class_consistency_loss_sum", "quad_normal_consistency_loss_sum",
         "quad_size_consistency_loss_sum", "quad_consistency_loss_sum")
INF = float("inf")


def _gap_of_smallest(dist, dim):
    """(second smallest - smallest) / (1 + smallest) along dim, minimum over the rest"""
    if dist.shape[dim] < 2:
        return INF
    two = torch.topk(dist, 2, dim=dim, largest=False).values
    lo, hi = two.select(dim, 0), two.select(dim, 1)
    return float(((hi - lo) / (1.0 + lo)).min())


def _gap_of_largest(scores):
    if scores.shape[-1] < 2:
        return INF
    two = torch.topk(scores, 2, dim=-1).values
    return float((two[..., 0] - two[..., 1]).min())


def clip(v):
    """-> (mean((v < eps) v), mask, min |v - eps| / eps)"""
    eps = torch.quantile(v.detach().flatten(), CLIP)
    mask = v.detach() < eps
    margin = float(((v.detach() - eps).abs().min() / eps)) if float(eps) > 0 else INF
    return (mask * v).mean(), mask, margin


def align(e, S):
    B = e.shape[0]
    sign = torch.ones(B, 1, 3, dtype=e.dtype)
    sign[:, 0, 0] = torch.where(S["flip_x_axis"].reshape(B) != 0, -1.0, 1.0).to(e.dtype)
    sign[:, 0, 1] = torch.where(S["flip_y_axis"].reshape(B) != 0, -1.0, 1.0).to(e.dtype)
    e = e * sign
    e = torch.bmm(e, S["rot_mat"].to(e.dtype).transpose(1, 2))
    return e * S["scale"].to(e.dtype).reshape(B, 1, 1)


def take(x, a):
    """x[b, a[b, r]] for x of shape (B, K, ...)"""
    return torch.stack([xb[ab] for xb, ab in zip(x, a)])


def assign(c, e, scores):
    """-> (d (B, K), ind1, ind2, s, nearest-neighbour margin)"""
    dist = ((c.unsqueeze(2) - e.unsqueeze(1)) ** 2).sum(-1)              # [b, i, j] = |c_i - e_j|^2
    dist1, ind1 = dist.min(dim=2)
    dist2, ind2 = dist.min(dim=1)
    s = F.softmax(scores, dim=2)[..., 1]
    d = dist1 * take(s, ind1) + dist2 * s
    margin = min(_gap_of_smallest(dist.detach(), 2), _gap_of_smallest(dist.detach(), 1))
    return d, ind1, ind2, s, margin


def sizes(ep, p, mean_size):
    cls = ep[p + "size_scores"].argmax(-1)
    res = torch.gather(ep[p + "size_residuals"], 2, cls[..., None, None].expand(-1, -1, 1, 3)).squeeze(2)
    return mean_size[cls] + res, cls


def consistency(S, T, mean_size, prefixes):
    """S, T: float64 end_points (S also holds flip_x_axis, flip_y_axis, rot_mat, scale); mean_size (ns, 3) float64.
    -> (ten terms, {(prefix, kind): decisions}, margins {nn, argmax, eps}, outputs {key: tensor} as the reference stores them)"""
    B = S[prefixes[0] + "center"].shape[0]
    scale = S["scale"].to(torch.float64).reshape(B, 1, 1)
    sums = [0.0] * 9
    decisions, outputs = {}, {}
    margins = {"nn": INF, "argmax": INF, "eps": INF}

    def note(name, value):
        margins[name] = min(margins[name], value)

    for p in prefixes:
        # objects
        e = align(T[p + "center"], S)
        d, ind1, a, s, m = assign(S[p + "center"], e, S[p + "objectness_scores"])
        note("nn", m)
        centre, mask_c, m = clip(d)
        note("eps", m)
        log_p = take(F.log_softmax(S[p + "sem_cls_scores"], dim=2), a)
        cls = 2.0 * F.kl_div(log_p, F.softmax(T[p + "sem_cls_scores"], dim=2), reduction="mean")
        size_s, cls_s = sizes(S, p, mean_size)
        size_t, cls_t = sizes(T, p, mean_size)
        note("argmax", min(_gap_of_largest(S[p + "size_scores"].detach()), _gap_of_largest(T[p + "size_scores"])))
        dsz = ((take(size_s, a) - size_t * scale) ** 2).sum(-1) * s
        size, mask_s, m = clip(dsz)
        note("eps", m)
        obj = 0.5 * centre + 1.0 * cls + 0.05 * size
        decisions[(p, 0)] = {"ind1": ind1, "ind2": a, "cls_s": cls_s, "cls_t": cls_t, "masks": [mask_c, mask_s]}
        outputs[p + "ema_center"], outputs[p + "ema_assignment"] = e, a
        outputs[p + "ema_assignment_confidence"] = s.detach()
        # quads
        e = align(T[p + "quad_center"], S)
        d, ind1, a, s, m = assign(S[p + "quad_center"], e, S[p + "quad_scores"])
        note("nn", m)
        q_centre, mask_c, m = clip(d)
        note("eps", m)
        cos = F.cosine_similarity(take(S[p + "normal_vector"], a)[..., :2], T[p + "normal_vector"][..., :2], dim=2)
        q_normal, mask_n, m = clip((1.0 - cos.abs()) * s)
        note("eps", m)
        q_size, mask_q, m = clip(((take(S[p + "quad_size"], a) - T[p + "quad_size"]) ** 2).sum(-1) * s)
        note("eps", m)
        log_p = take(F.log_softmax(S[p + "quad_scores"], dim=2), a)
        q_cls = 2.0 * F.kl_div(log_p, F.softmax(T[p + "quad_scores"], dim=2), reduction="batchmean")
        quad = 0.5 * q_centre + 0.0 * q_cls + 1.0 * q_normal + 0.05 * q_size
        decisions[(p, 1)] = {"ind1": ind1, "ind2": a, "masks": [mask_c, mask_n, mask_q]}
        outputs[p + "ema_center_quad"], outputs[p + "ema_assignment_quad"] = e, a
        outputs[p + "ema_assignment_quad_confidence"] = s.detach()
        for t, v in enumerate((centre, cls, size, obj, q_centre, q_cls, q_normal, q_size, quad)):
            sums[t] = sums[t] + v
    terms = [v / len(prefixes) for v in sums]
    terms.append(terms[3] + terms[8])
    return terms, decisions, margins, outputs


def leaves(S_np, T_np, mean_size_np, grad_keys):
    """numpy inputs -> (S, T, mean_size) in float64, the student's `grad_keys` as leaves"""
    S = {}
    for k, v in S_np.items():
        t = torch.from_numpy(v.copy())
        S[k] = t.double().requires_grad_(True) if k in grad_keys else (t.double() if t.is_floating_point() else t)
    T = {k: torch.from_numpy(v.copy()).double() for k, v in T_np.items()}
    return S, T, torch.from_numpy(mean_size_np.copy()).double()
