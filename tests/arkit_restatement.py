"""The ARKit physical-constraint loss restated in float64 torch, written from the mathematics of include/omnipq_semi.h (not
from the reference's code and not from the kernels): the terms, the record of every discrete decision and the margins by
which each decision was taken.  Differentiable with respect to the predictions."""
import numpy as np
import torch

PREDICTION_KEYS = ("last_quad_center", "last_normal_vector", "last_quad_size", "last_quad_scores")
GRAD_KEYS = ("last_quad_center", "last_normal_vector")
RECORD_KEYS = ("gate", "rev", "inside", "live", "collisions")
GATE = 0.1
COLLISION = 1e-4
SIGNS = ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0))       # the corner order of get_2d_box


def leaves(pred_np, grad_keys=PREDICTION_KEYS):
    """float64 leaves of the predictions; those in grad_keys require a gradient"""
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64).copy()).requires_grad_(k in grad_keys)
            for k, v in pred_np.items()}


def corners(center_label, size_label, n):
    """(4 n, 2): the footprint corners of the first n boxes, box by box"""
    g = torch.from_numpy(np.asarray(center_label[:n, :2], dtype=np.float64))
    half = torch.from_numpy(np.asarray(size_label[:n, :2], dtype=np.float64)) / 2
    sign = torch.tensor(SIGNS, dtype=torch.float64)
    return (g[:, None, :] + sign[None] * half[:, None, :]).reshape(-1, 2)


def arkit_pc(pred, unlabeled):
    """pred: float64 tensors under PREDICTION_KEYS, (Bt, Q, .); unlabeled: numpy `center_label`, `size_label` (Bu, K2, 3) and
    `num_gt_boxes` (Bu, >= 1).  -> (loss: 0-dim float64 tensor, collisions: int, record (Bu, Q, 5) int32 array in the order of
    RECORD_KEYS, margins {name: the smallest distance of any decision of that kind from flipping}, quad_margin (Bu, Q): the
    smallest margin of any kind per quad)."""
    cl, sl = unlabeled["center_label"], unlabeled["size_label"]
    counts = np.asarray(unlabeled["num_gt_boxes"])[..., 0]
    Bu, K2 = cl.shape[:2]
    qc, nv, qs, sc = (pred[k] for k in PREDICTION_KEYS)
    Bt, Q = qc.shape[:2]
    if Bt != 2 * Bu:
        raise ValueError("the predictions must hold twice the unlabelled batch")
    loss = torch.zeros((), dtype=torch.float64)
    collisions = 0
    record = np.zeros((Bu, Q, len(RECORD_KEYS)), dtype=np.int32)
    margins = {"gate": np.inf, "rev": np.inf, "inside": np.inf, "live": np.inf}
    quad_margin = np.full((Bu, Q), np.inf)
    for s in range(Bu):
        n_s = int(counts[s])
        c, n = qc[Bu + s, :, :2], nv[Bu + s, :, :2]
        p1 = torch.softmax(sc[Bu + s].detach(), dim=-1)[:, 1]
        gate = p1 > GATE
        away = -(c.detach() * n.detach()).sum(-1)
        rev = away < 0
        ab = torch.where(rev[:, None], -n, n)
        P = corners(cl[s], sl[s], min(max(n_s, 0), K2))
        delta = ab @ P.T - (ab * c).sum(-1, keepdim=True)                        # (Q, corners)
        t = P[None] - ab[:, None, :] * delta[:, :, None]
        w = (t - c[:, None, :]).detach().norm(dim=-1)
        inside = w < qs[Bu + s, :, 0].detach()[:, None]
        pair = torch.relu(-delta) * inside
        live = inside & (delta.detach() < 0)
        hit = pair.detach() > COLLISION
        if n_s > 0:
            loss = loss + (pair.sum(1) / n_s)[gate].sum()
            collisions += int(hit[gate].sum())
        g = gate.numpy().astype(np.int32)
        record[s] = np.stack([g, g * rev.numpy(), g * inside.sum(1).numpy(), g * live.sum(1).numpy(), g * hit.sum(1).numpy()], 1)
        # margins: the gate of every quad; of the gated quads the reversal, every pair's inside test and, of the inside pairs,
        # the distance of -delta from 0 and from the collision threshold
        m_gate = (p1 - GATE).abs().numpy()
        m_quad = m_gate.copy()
        margins["gate"] = min(margins["gate"], float(m_gate.min()))
        if bool(gate.any()):
            big = torch.full((Q,), np.inf, dtype=torch.float64)
            m_rev = torch.where(gate, away.abs(), big)
            margins["rev"] = min(margins["rev"], float(m_rev.min()))
            m_quad = np.minimum(m_quad, m_rev.numpy())
            if P.shape[0]:
                m_in = torch.where(gate[:, None], (w - qs[Bu + s, :, 0].detach()[:, None]).abs(), big[:, None]).min(1).values
                depth = -delta.detach()
                edge = torch.minimum(depth.abs(), (depth - COLLISION).abs())
                m_live = torch.where(gate[:, None] & inside, edge, big[:, None]).min(1).values
                margins["inside"] = min(margins["inside"], float(m_in.min()))
                margins["live"] = min(margins["live"], float(m_live.min()))
                m_quad = np.minimum(m_quad, np.minimum(m_in.numpy(), m_live.numpy()))
        quad_margin[s] = m_quad
    return loss, collisions, record, margins, quad_margin
