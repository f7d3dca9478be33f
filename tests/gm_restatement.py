"""The gamma-mixture guide criterion in float64 torch on the CPU: the math of include/omnipq_semi.h written out with
tensor ops, for the tests to hold the HIP path against.  It takes the two draws as arguments, reads no reference code and
needs no GPU.  Gradients come from autograd; what the reference detaches (`.detach()`, `.item()`, `torch.tensor([...])`,
the numpy round trip into fit_gamma) is detached here.
"""
import math

import torch

T_STAR = 0.29961316955346434
MIN_KEPT = 300
F64 = torch.float64


def keep_mask(total):
    """fit.py:168-173 with the arguments of gamma_mixture_loss_util.py:65 -- NOT `|t| <= T_STAR`: the golden test shows
    that the two agree."""
    t = total.abs()
    lhs = 0.1 * (20.0 ** 2 / math.gamma(2)) * torch.exp(-20.0 * t) * t
    rhs = 0.9 * (1.0 ** 3 / math.gamma(3)) * torch.exp(-1.0 * t) * t ** 2
    return lhs >= rhs


def sl1(e):
    d = e.abs()
    return torch.where(d < 1.0, 0.5 * d * d, d - 0.5)


def distances(xyz, normals, center, nv, size, inds):
    """Per-sample quantities of one scene (all float64)."""
    x, m = xyz[inds, :3], normals[inds]
    s0, s1 = size[0] / 1.5, size[1]
    nxy = nv[:2].detach()
    n = torch.cat([nxy / nxy.norm(), torch.zeros(1, dtype=F64)])
    xdir = torch.stack([-n[1], n[0], torch.zeros((), dtype=F64)])
    mh = m / m.norm(dim=1, keepdim=True).clamp(min=1e-5)
    dc = 1.0 - (mh @ n).abs()
    o = x - center
    v = (o @ n).abs()
    xd, zd = (o @ xdir).abs(), o[:, 2].abs()
    a = torch.stack([2 * xd - s0, 2 * zd - s1], dim=1).clamp(min=0.0).norm(dim=1)
    total = (2.5 * dc + 0.2 * a ** 2 + 0.5 * v).detach()
    return dict(x=x, m=m, n=n, xdir=xdir, v=v, total=total, s0=s0)


def scene(xyz, normals, score, center, nv, size, inds):
    """-> dict: terms (four 0-dim float64 tensors), n_k, branch (0 none, 1 CE(score, 1), 2 CE(score, 0)), total, keep and,
    for a scene that counts, q85, pseudo_x, mu, v_keep"""
    xyz, normals, nv = xyz.to(F64), normals.to(F64), nv.to(F64)
    inds = torch.as_tensor(inds).long()
    d = distances(xyz, normals, center, nv, size, inds)
    keep = keep_mask(d["total"])
    n_k = int(keep.sum())
    zero = torch.zeros((), dtype=F64)
    out = dict(n_k=n_k, branch=0, total=d["total"], keep=keep, q85=None, terms=(zero, zero, zero, zero))
    if n_k < MIN_KEPT:
        return out
    x, m, n, xdir = d["x"][keep], d["m"][keep], d["n"], d["xdir"]
    est = m.mean(0)[:2]
    est = torch.cat([est, torch.zeros(1, dtype=F64)])
    est = est / est.norm()
    mn = (1.0 - torch.nn.functional.cosine_similarity(est[None], n[None]).abs()).detach()[0]
    vk = d["v"][keep]
    q85 = torch.quantile(vk.detach(), 0.85)
    mv = (vk * (vk < q85)).sum() / n_k
    mu = x.mean(0)
    xdp = ((x - mu) @ xdir).abs()
    pseudo = torch.stack([torch.quantile(xdp, t) / t for t in (0.85, 0.925, 1.0)]).mean().detach()
    ms = sl1(d["s0"] - 2.0 * pseudo) + sl1(mu - center).sum()
    branch = 0
    if mv < 0.05 and mn < 0.02 and ms < 0.10:
        branch = 1
    elif mv > 0.3 or mn > 0.05 or ms > 0.35:
        branch = 2
    msc = zero
    if branch:
        msc = torch.logsumexp(score, 0) - score[1 if branch == 1 else 0]
    out.update(branch=branch, q85=q85, terms=(mn, mv, ms, msc), pseudo_x=pseudo, mu=mu.detach(), v_keep=vk.detach())
    return out


def candidates(scores):
    """(Q, 2) -> bool (Q,): softmax(scores)[:, 1] > 0.1"""
    return torch.softmax(scores.to(F64), dim=-1)[:, 1] > 0.1


def criterion(ep, pick, sample_inds):
    """ep: dict of tensors with a batch dimension (any float dtype; `last_quad_scores`, `last_quad_center`,
    `last_quad_size` may be float64 leaves).  -> (four 0-dim float64 tensors summed over the scenes / B, per-scene dicts)"""
    B = ep["point_clouds"].shape[0]
    sums = [torch.zeros((), dtype=F64) for _ in range(4)]
    scenes = []
    for b in range(B):
        p = int(pick[b])
        if not bool(candidates(ep["last_quad_scores"][b].detach()).any()) or not 0 <= p < ep["last_quad_scores"].shape[1]:
            scenes.append(dict(n_k=0, branch=0, skipped=True))
            continue
        s = scene(ep["point_clouds"][b], ep["vertex_normals"][b], ep["last_quad_scores"][b, p].to(F64),
                  ep["last_quad_center"][b, p].to(F64), ep["last_normal_vector"][b, p], ep["last_quad_size"][b, p].to(F64),
                  sample_inds[b])
        s["skipped"] = False
        scenes.append(s)
        for t in range(4):
            sums[t] = sums[t] + s["terms"][t]
    return tuple(t / B for t in sums), scenes


def leaves(ep_np):
    """numpy batch -> (ep of float64/float32 CPU tensors with the three differentiable inputs as float64 leaves, leaves)"""
    ep = {k: torch.from_numpy(v.copy()) for k, v in ep_np.items()}
    lv = {k: ep[k].to(F64).requires_grad_(True) for k in ("last_quad_scores", "last_quad_center", "last_quad_size")}
    ep.update(lv)
    return ep, lv
