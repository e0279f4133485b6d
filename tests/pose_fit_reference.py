"""The yardstick of the pose-fit tests: the alignment scripts' RANSAC over matched 3-D point pairs (pc_align_ransac,
utils/solution.py:476-557) and their 9-DoF Adam fit (adam_algorithm_3d3d_9dof, :363-446), restated from their formulas
in float64 numpy (LAPACK's SVD) and torch (autograd, torch.optim.Adam).  No GPU needed; `device=` and `dtype=` let the
timing script run the Adam loop the way the reference runs it."""
import numpy as np
import torch


def similarity_fit(p, q, method="umeyama"):
    """(R, t, s) of q ~ s R p + t: cov = sum (p - pm)(q - qm)^T = U S V^T, D = diag(1, 1, det(U V^T) < 0 ? -1 : 1),
    R = V D U^T, s = sum(S diag D) / sum |p - pm|^2 (umeyama) or 1 (kabsch), t = qm - s R pm."""
    p = np.asarray(p, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    pm, qm = p.mean(axis=0), q.mean(axis=0)
    pc, qc = p - pm, q - qm
    U, S, Vt = np.linalg.svd(pc.T @ qc)
    d = np.ones(3)
    if np.linalg.det(U @ Vt) < 0:
        d[2] = -1.0
    R = Vt.T @ np.diag(d) @ U.T
    if method == "umeyama":
        s = float((S * d).sum() / (pc ** 2).sum())
    elif method == "kabsch":
        s = 1.0
    else:
        raise NotImplementedError(method)
    return R, qm - s * (R @ pm), s


def residuals(p, q, R, t, s):
    """| R (s p) + t - q | per pair."""
    return np.linalg.norm((R @ (s * p).T).T + t - q, axis=1)


def ransac_fit(source, target, samples, threshold, min_inlier_ratio=-1.0, method="umeyama"):
    """dict(R, t, s, winner, count, counts[n_hyp], mask[n], iterations): every hypothesis's inlier count, the winner by the
    reference's rule (the first hypothesis with the highest count; with min_inlier_ratio > 0 the first whose count exceeds
    min_inlier_ratio * n, where the reference's loop ends after `iterations` draws), the fit over its inliers."""
    p = np.asarray(source, dtype=np.float64)
    q = np.asarray(target, dtype=np.float64)
    samples = np.asarray(samples)
    n = len(p)
    counts = np.zeros(len(samples), dtype=np.int32)
    masks = []
    with np.errstate(all="ignore"):
        for h, idx in enumerate(samples):
            R, t, s = similarity_fit(p[idx], q[idx], method)
            m = residuals(p, q, R, t, s) < threshold
            masks.append(m)
            counts[h] = m.sum()
    winner, iterations = int(np.argmax(counts)), len(samples)
    if min_inlier_ratio > 0:
        over = np.nonzero((counts > min_inlier_ratio * n) & (counts > 0))[0]
        if len(over):
            winner, iterations = int(over[0]), int(over[0]) + 1
    count = int(counts[winner])
    if count < 3:
        raise ValueError("No inliers found in RANSAC.")
    mask = masks[winner]
    R, t, s = similarity_fit(p[mask], q[mask], method)
    return {"R": R, "t": t, "s": s, "winner": winner, "count": count, "counts": counts, "mask": mask, "iterations": iterations}


def draw_triples(n, count):
    """`count` triples as the reference draws them: one np.random.choice(n, 3, replace=False) per iteration on numpy's
    global generator."""
    return np.stack([np.random.choice(n, 3, replace=False) for _ in range(count)]).astype(np.int32)


def pc_align_ransac(source_points, target_points, threshold=0.5, max_iterations=2000, min_inlier_ratio=-1.0, method="umeyama"):
    """(R, t, s) as the reference's loop gives them, leaving numpy's global generator where that loop leaves it."""
    if len(source_points) != len(target_points):
        raise ValueError("Source and target points must have the same length")
    if len(source_points) < 3:
        raise ValueError("At least 3 points are required to solve Umeyama.")
    n = len(source_points)
    state = np.random.get_state()
    res = ransac_fit(source_points, target_points, draw_triples(n, max_iterations), threshold, min_inlier_ratio, method)
    if res["iterations"] < max_iterations:
        np.random.set_state(state)
        draw_triples(n, res["iterations"])
    return res["R"], res["t"], res["s"]


def quaternion_to_matrix(q):
    """R = I + 2 B(q) / (q.q), q = (r, i, j, k) (utils/geometry.py:43-72)."""
    r, i, j, k = q[0], q[1], q[2], q[3]
    ts = 2.0 / (q * q).sum()
    return torch.stack([1 - ts * (j * j + k * k), ts * (i * j - k * r), ts * (i * k + j * r),
                        ts * (i * j + k * r), 1 - ts * (i * i + k * k), ts * (j * k - i * r),
                        ts * (i * k - j * r), ts * (j * k + i * r), 1 - ts * (i * i + j * j)]).reshape(3, 3)


def start_scale(init_scale, scale_min, scale_max):
    """The reference's rule for init_scale (:379-388): a float becomes three, a list or tuple an array, anything else or
    another shape raises; one component outside [scale_min, scale_max] turns all three into the mid-point."""
    if isinstance(init_scale, float):
        init_scale = np.array(3 * [init_scale])
    elif isinstance(init_scale, (list, tuple)):
        init_scale = np.array(init_scale)
    if not isinstance(init_scale, np.ndarray) or init_scale.shape != (3,):
        raise ValueError("`init_scale` must be a float, list, or tuple of length 3.")
    if init_scale.min() < scale_min or init_scale.max() > scale_max:
        init_scale = np.array(3 * [scale_min + (scale_max - scale_min) / 2])
    return init_scale.astype(np.float64)


def adam_9dof(source_points, target_points, iterations=1000, lr=1e-3, lambda_reg_scale=2e-5, lambda_reg_rot=1e-4, scale_max=1.5,
              scale_min=0.75, init_scale=1.0, device="cpu", dtype=torch.float64, loss_every=0):
    """dict(rotation, translation, scale, rotation_orthogonal, M, losses) in float64 numpy: `iterations` steps of
    torch.optim.Adam on t, q, qo and the scale logits l with M = R(q) Ro(qo)^T diag(s) Ro(qo), s = scale_min + (scale_max -
    scale_min) sigmoid(l) and the loss  mean |M p + t - q|^2 + lambda_reg_scale (mean (l - 1)^2 + mean (s - mean s)^2) +
    lambda_reg_rot arccos(clamp((tr R - 1) / 2, -1, 1))^2.  One small torch kernel per operation: the reference's pattern."""
    P = torch.tensor(np.asarray(source_points), dtype=dtype, device=device)
    Q = torch.tensor(np.asarray(target_points), dtype=dtype, device=device)
    s0 = start_scale(init_scale, scale_min, scale_max)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=device).to(dtype)   # the start values are fp32 constants there
    t = torch.nn.Parameter(f32([0.01, 0.01, 0.01]))
    q = torch.nn.Parameter(f32([0.9, 0.01, 0.01, 0.01]))
    qo = torch.nn.Parameter(f32([1.0, 0.0, 0.0, 0.0]))
    with torch.no_grad():
        logit = torch.nn.Parameter(torch.logit((torch.tensor(s0, dtype=dtype, device=device) - scale_min) / (scale_max - scale_min)))
    opt = torch.optim.Adam([{"params": x, "lr": lr} for x in (t, q, qo, logit)])
    span = scale_max - scale_min
    losses = []
    for it in range(iterations):
        s = scale_min + span * torch.sigmoid(logit)
        R, Ro = quaternion_to_matrix(q), quaternion_to_matrix(qo)
        pred = (R @ Ro.T @ (s[:, None] * (Ro @ P.T))).T + t
        data = torch.mean((pred - Q) ** 2)
        reg = torch.mean((logit - 1) ** 2) + torch.mean((s - torch.mean(s)) ** 2)
        rot = torch.arccos(torch.clamp((torch.trace(R) - 1) / 2, -1, 1)) ** 2
        loss = data + lambda_reg_scale * reg + lambda_reg_rot * rot
        opt.zero_grad()
        loss.backward()
        opt.step()
        if loss_every > 0 and (it + 1) % loss_every == 0:
            losses.append(float(loss.detach()))
    with torch.no_grad():
        R, Ro = quaternion_to_matrix(q), quaternion_to_matrix(qo)
        s = scale_min + span * torch.sigmoid(logit)
        out = {"rotation": R, "translation": t, "scale": s, "rotation_orthogonal": Ro}
        out = {k: v.detach().cpu().double().numpy() for k, v in out.items()}
    out["M"] = compose(out["rotation"], out["scale"], out["rotation_orthogonal"])
    out["losses"] = np.array(losses)
    return out


def compose(rotation, scale, rotation_orthogonal):
    """M = R Ro^T diag(s) Ro in float64."""
    R, s, Ro = (np.asarray(a, dtype=np.float64) for a in (rotation, scale, rotation_orthogonal))
    return R @ Ro.T @ np.diag(s) @ Ro


def rotation_about(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)
