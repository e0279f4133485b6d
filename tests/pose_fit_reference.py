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
    winner, iterations = select_winner(counts, n, min_inlier_ratio)
    count = int(counts[winner])
    if count < 3:
        raise ValueError("No inliers found in RANSAC.")
    mask = masks[winner]
    R, t, s = similarity_fit(p[mask], q[mask], method)
    return {"R": R, "t": t, "s": s, "winner": winner, "count": count, "counts": counts, "mask": mask, "iterations": iterations}


def select_winner(counts, n, min_inlier_ratio=-1.0):
    """(winner, iterations) by the reference's rule: the first hypothesis with the highest count; with min_inlier_ratio > 0
    the first whose count exceeds (strictly) min_inlier_ratio * n, where the reference's loop ends."""
    winner, iterations = int(np.argmax(counts)), len(counts)
    if min_inlier_ratio > 0:
        over = np.nonzero((counts > min_inlier_ratio * n) & (counts > 0))[0]
        if len(over):
            winner, iterations = int(over[0]), int(over[0]) + 1
    return winner, iterations


def similarity_fits(p3, q3, method="umeyama"):
    """similarity_fit over a batch of samples p3, q3 [n_hyp, k, 3] with one stacked np.linalg.svd: (R [n_hyp, 3, 3],
    t [n_hyp, 3], s [n_hyp], sv [n_hyp, 3]).  A sample with a non-finite covariance (LAPACK refuses it) gets a NaN model,
    which counts nothing."""
    if method not in ("umeyama", "kabsch"):
        raise NotImplementedError(method)
    p3 = np.asarray(p3, dtype=np.float64)
    q3 = np.asarray(q3, dtype=np.float64)
    with np.errstate(all="ignore"):
        pm, qm = p3.mean(axis=1), q3.mean(axis=1)
        pc, qc = p3 - pm[:, None], q3 - qm[:, None]
        cov = np.matmul(pc.transpose(0, 2, 1), qc)
        finite = np.isfinite(cov).all(axis=(1, 2))
        U, S, Vt = np.linalg.svd(np.where(finite[:, None, None], cov, 0.0))
        d = np.ones((len(cov), 3))
        d[:, 2] = np.where(np.linalg.det(np.matmul(U, Vt)) < 0, -1.0, 1.0)
        R = np.matmul(Vt.transpose(0, 2, 1) * d[:, None, :], U.transpose(0, 2, 1))
        s = (S * d).sum(axis=1) / (pc ** 2).sum(axis=(1, 2)) if method == "umeyama" else np.ones(len(cov))
        t = qm - s[:, None] * np.einsum("hab,hb->ha", R, pm)
    bad = ~finite
    R[bad], t[bad], s[bad], S[bad] = np.nan, np.nan, np.nan, np.nan
    return R, t, s, S


def ransac_table(source, target, samples, threshold, method="umeyama", chunk=4096):
    """Every hypothesis against every pair, batched: dict(counts [n_hyp] int32, margin: the smallest |residual - threshold|
    / threshold over all finite (hypothesis, pair), cond: the smallest second-over-first singular value of the hypotheses
    whose three indices differ, R, t, s: the models)."""
    p = np.asarray(source, dtype=np.float64)
    q = np.asarray(target, dtype=np.float64)
    samples = np.asarray(samples)
    R, t, s, S = similarity_fits(p[samples], q[samples], method)
    counts = np.zeros(len(samples), dtype=np.int32)
    margin = np.inf
    with np.errstate(all="ignore"):
        for b in range(0, len(samples), chunk):
            e = slice(b, b + chunk)
            pred = np.einsum("hab,nb->hna", R[e], p) * s[e, None, None] + t[e, None, :]
            res = np.linalg.norm(pred - q[None], axis=2)
            counts[e] = (res < threshold).sum(axis=1)
            gap = np.abs(res - threshold)[np.isfinite(res)]
            if gap.size:
                margin = min(margin, float(gap.min()) / threshold)
        distinct = (samples[:, 0] != samples[:, 1]) & (samples[:, 0] != samples[:, 2]) & (samples[:, 1] != samples[:, 2])
        distinct &= np.isfinite(S).all(axis=1)
        cond = float((S[distinct, 1] / S[distinct, 0]).min()) if distinct.any() else np.inf
    return {"counts": counts, "margin": margin, "cond": cond, "R": R, "t": t, "s": s}


def ransac_counts(source, target, samples, threshold, method="umeyama"):
    """ransac_fit's counts with one stacked SVD over all hypotheses (65 535 of them take seconds)."""
    return ransac_table(source, target, samples, threshold, method)["counts"]


def ransac_fit_batched(source, target, samples, threshold, min_inlier_ratio=-1.0, method="umeyama"):
    """ransac_fit on the batched counts, and without its error: dict(counts, margin, cond, winner, count, mask, iterations)
    always, and R, t, s (the fit over the winner's inliers) when the winner has at least 3."""
    p = np.asarray(source, dtype=np.float64)
    q = np.asarray(target, dtype=np.float64)
    out = ransac_table(p, q, samples, threshold, method)
    w, out["iterations"] = select_winner(out["counts"], len(p), min_inlier_ratio)
    with np.errstate(all="ignore"):
        mask = residuals(p, q, out["R"][w], out["t"][w], out["s"][w]) < threshold
    out.update(winner=w, count=int(out["counts"][w]), mask=mask, R=None, t=None, s=None)
    if out["count"] >= 3:
        out["R"], out["t"], out["s"] = similarity_fit(p[mask], q[mask], method)
    return out


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
              scale_min=0.75, init_scale=1.0, device="cpu", dtype=torch.float64, loss_every=0, centred=False,
              reg_factors=(1.0, 1.0, 1.0)):
    """dict(rotation, translation, scale, rotation_orthogonal, M, losses) in float64 numpy: `iterations` steps of
    torch.optim.Adam on t, q, qo and the scale logits l with M = R(q) Ro(qo)^T diag(s) Ro(qo), s = scale_min + (scale_max -
    scale_min) sigmoid(l) and the loss  mean |M p + t - q|^2 + lambda_reg_scale (mean (l - 1)^2 + mean (s - mean s)^2) +
    lambda_reg_rot arccos(clamp((tr R - 1) / 2, -1, 1))^2.  One small torch kernel per operation: the reference's pattern.
    centred=True states the data term a second way, mean |M pc + (M pm + t - qm) - qc|^2 about the two centroids: the same
    function of the parameters, so the distance between the two runs is the yardstick's own formulation error.
    reg_factors scales the three regulariser contributions (logit term, scale-spread term, rotation term) so that a test
    can show that a case would see one of them wrong.  Also returned: grad0 [14], the gradient at the start (t, q, qo,
    logits), and loss, the last step's loss."""
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
    f_logit, f_spread, f_rot = reg_factors
    pm, qm = P.mean(dim=0), Q.mean(dim=0)
    Pc, Qc = P - pm, Q - qm
    losses, grad0, last = [], None, 0.0
    for it in range(iterations):
        s = scale_min + span * torch.sigmoid(logit)
        R, Ro = quaternion_to_matrix(q), quaternion_to_matrix(qo)
        if centred:
            M = R @ Ro.T @ (s[:, None] * Ro)
            data = torch.mean(((M @ Pc.T).T + (M @ pm + t - qm) - Qc) ** 2)
        else:
            pred = (R @ Ro.T @ (s[:, None] * (Ro @ P.T))).T + t
            data = torch.mean((pred - Q) ** 2)
        reg = f_logit * torch.mean((logit - 1) ** 2) + f_spread * torch.mean((s - torch.mean(s)) ** 2)
        rot = f_rot * torch.arccos(torch.clamp((torch.trace(R) - 1) / 2, -1, 1)) ** 2
        loss = data + lambda_reg_scale * reg + lambda_reg_rot * rot
        opt.zero_grad()
        loss.backward()
        if it == 0:
            grad0 = torch.cat([x.grad.detach().reshape(-1) for x in (t, q, qo, logit)]).cpu().double().numpy()
        last = float(loss.detach())
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
    out["grad0"] = grad0
    out["loss"] = last
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
