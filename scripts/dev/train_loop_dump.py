"""What the optimisation loops of scorp_amd/train.py leave behind - per-iteration losses, the six leaves, Adam's step / exp_avg /
exp_avg_sq - dumped by one checkout and compared with another's in dtype, shape and bytes (profiles/train_loop_bitequal.json).

    python scripts/dev/train_loop_dump.py dump cpu a_cpu.npz [TREE]      (a fresh process per dump; TREE: the checkout whose
    python scripts/dev/train_loop_dump.py dump gpu a_gpu.npz [TREE]       scorp_amd and tests are loaded, default this one)
    python scripts/dev/train_loop_dump.py compare out.json a_cpu.npz b_cpu.npz a_gpu.npz b_gpu.npz [a2_gpu.npz]

cpu (no GPU; the stand-ins of tests/test_parallel_cpu.py for the rasterizer, the one-call view and the guarded optimizer), each
in one process and on two gloo ranks:
    autograd      train(data_parallel=True), 14 iterations with a caller's render / loss, densifying at 4, 8, 12
    overflow      train(fused_view=True, data_parallel=True), 5 iterations, rank 0's first view overflows and is run again
                  (two ranks only)
    path_change   training_iteration: 1-4 through the fused branch (4 densifies), 5-6 through the autograd branch; the state
                  after 4 and after 6.  On two ranks "after6" is where the parent averaged the arena of the leaves that 4
                  replaced: it is EXPECTED to differ there and is reported, not judged.
gpu (SCORP_BACKWARD_DETERMINISTIC=1): 2000 Gaussians, 4 cameras at 96x64, 24 iterations of train() with densify_from_iter 2,
densification_interval 8, opacity_reset_interval 12, depth_from_iter 10, the isotropic term and seeded depth maps, for
{3DGS, 2DGS} x {fused view with the step inside, fused view with a separate step, autograd loop}; 8 surfel iterations from 8001
(regulariser and depth-normal weights on); post_refine, 16 iterations on an SH-0 object, one-call and autograd.

compare: a = the parent, b = this tree, a2 = the parent once more.  A tensor the parent's two dumps agree on in bytes must
be equal in bytes in b; one they do not is named and b is held inside their spread (worst |b - a| <= worst |a - a2|)."""
import json
import os
import sys

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
EXPECTED_DIFFERENT = "cpu/ranks2/path_change/after6/"


def _state(out, case, m, losses=None):
    """the leaves and the optimizer's state of model `m` (and the losses) under `case`"""
    if losses is not None:
        out[f"{case}/losses"] = np.array([float(l) for l in losses], np.float64)
    for name in LEAVES:
        out[f"{case}/{name}"] = getattr(m, name).detach().cpu().numpy().copy()     # (a copy: on the CPU numpy() shares the leaf)
    for g in m.optimizer.param_groups:
        st = m.optimizer.state.get(g["params"][0], {})
        for k in ("step", "exp_avg", "exp_avg_sq"):
            if k in st:
                out[f"{case}/adam/{g.get('name', '?')}/{k}"] = np.array(st[k].detach().cpu().numpy())


# ---- cpu ----
def _cpu_cases(out, prefix, rank, ranks):
    import warnings
    import torch
    import scorp_amd.train as T
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from tests import test_parallel_cpu as P
    data_parallel = True

    m, opt, cams, gts = P._dp_setup()
    losses = T.train(m, cams, gts, opt, iterations=14, data_parallel=data_parallel, render_fn=P._fake_render, loss_fn=P._plain_loss,
                     scene_extent=4.0)
    _state(out, f"{prefix}/autograd", m, losses)

    if ranks:    # (in one process train() is not data-parallel, and the stand-in view is only that of the data-parallel loop)
        m, opt, cams, gts = P._dp_setup()
        opt.densify_from_iter = 1 << 30
        m.training_setup(opt)
        m.optimizer = P._GuardedAdamStandin(m.optimizer.param_groups, lr=0.0, eps=1e-15)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            losses = T.train(m, cams, gts, opt, T.PipelineParams(), iterations=5, data_parallel=data_parallel, fused_view=True,
                             loss_fn=fused_l1_ssim_loss, view_fn=P._overflowing_view(rank, []), scene_extent=4.0)
        _state(out, f"{prefix}/overflow", m, losses)

    drain, T._drain_reservation = T._drain_reservation, lambda **kw: True     # (no real view: nothing is pending)
    try:
        m, opt, cams, gts = P._dp_setup()
        m.training_setup(opt)
        view, losses = P._overflowing_view(-1, []), []
        for it in range(1, 7):
            k = (2 * it + rank) % len(cams)
            path = dict(loss_fn=fused_l1_ssim_loss, view_fn=view) if it <= 4 else dict(render_fn=P._fake_render, loss_fn=P._plain_loss)
            losses.append(T.training_iteration(m, cams[k], gts[k], opt, T.PipelineParams(), torch.zeros(3), it, data_parallel=True,
                                               fused_view=True, **path)[0].detach())
            if it in (4, 6):
                _state(out, f"{prefix}/path_change/after{it}", m, losses)
    finally:
        T._drain_reservation = drain


def _cpu_rank(rank, port, tree, q):
    sys.path.insert(0, tree)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        out = {}
        _cpu_cases(out, f"cpu/ranks2/rank{rank}" if rank else "cpu/ranks2", rank, True)
        q.put(out)
    finally:
        dist.destroy_process_group()


def dump_cpu(path, tree):
    import torch.multiprocessing as mp
    from tests.test_parallel_cpu import _free_port
    out = {}
    _cpu_cases(out, "cpu/single", 0, False)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_cpu_rank, args=(r, port, tree, q)) for r in range(2)]
    for p in procs:
        p.start()
    for _ in procs:
        out.update(q.get(timeout=600))
    for p in procs:
        p.join(timeout=60)
    np.savez(path, **out)
    print(f"{len(out)} tensors -> {path}")


# ---- gpu ----
def dump_gpu(path):
    os.environ["SCORP_BACKWARD_DETERMINISTIC"] = "1"
    import math
    import torch
    from scorp_amd import _C
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams, OptimizationParams2D
    from scorp_amd.renderer import render as render3d
    from scorp_amd.renderer2d import GaussianModel2D, render as render2d
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams, post_refine, train, training_iteration
    dev = torch.device("cuda:0")
    out = {"library_source_sha": np.array(_C.lib().scorp_source_sha().decode())}
    W, H = 96, 64
    cams = ring_cameras(4, W, H, 4, radius=3.0, device=dev)
    g = torch.Generator(device=dev).manual_seed(1)
    sensors = [2.0 + 2.0 * torch.rand(1, H, W, device=dev, generator=g) for _ in cams]
    monos = [torch.rand(1, H, W, device=dev, generator=g) for _ in cams]
    bg = torch.zeros(3, device=dev)
    pipe = PipelineParams()
    pipe.depth_ratio = 1.0

    def setup(surfels, deg=1):
        raw = make_gaussians(2000, deg, 21, extent=1.0, log_scale_mean=math.log(0.05), scale_dims=2 if surfels else 3)
        raw["opacity"] += 1.5
        Model, rfn = (GaussianModel2D, render2d) if surfels else (GaussianModel, render3d)
        teacher = Model.from_raw(raw, deg, device=dev)
        teacher.active_sh_degree = deg
        with torch.no_grad():
            gts = [rfn(c, teacher, pipe, bg)["render"].clamp(0, 1).clone() for c in cams]
        raw2 = {k: v.copy() for k, v in raw.items()}
        raw2["features_dc"] += np.random.default_rng(22).normal(0, 0.6, raw2["features_dc"].shape).astype(np.float32)
        m = Model.from_raw(raw2, deg, device=dev)
        m.active_sh_degree = deg
        opt = OptimizationParams2D() if surfels else OptimizationParams()
        opt.random_background, opt.opacity_cull = False, 0.005
        opt.densify_from_iter, opt.densification_interval, opt.opacity_reset_interval, opt.depth_from_iter = 2, 8, 12, 10
        assert opt.lambda_isotropic > 0
        return m, opt, gts, rfn

    paths = {"fused_step": dict(fused_view=True), "fused_nostep": dict(fused_view=True, fused_step=False), "autograd": {}}
    for surfels in (False, True):
        kind = "2dgs" if surfels else "3dgs"
        for name, kw in paths.items():
            m, opt, gts, rfn = setup(surfels)
            if surfels:
                kw = dict(kw, surfels=True, **({} if kw else {"render_fn": rfn}))
            torch.manual_seed(7)
            losses = train(m, cams, gts, opt, pipe, iterations=24, scene_extent=3.0, background=bg, gt_depths=sensors,
                           gt_depth_ests=monos, **kw)
            out[f"gpu/{kind}/{name}/n"] = np.array(m.get_xyz.shape[0])
            _state(out, f"gpu/{kind}/{name}", m, losses)
    # the surfel schedules that 24 iterations from 1 never reach: regulariser weights (> 7000 / 3000), depth-normal (> 1010)
    for name, kw in (("fused_step", dict(fused_view=True)), ("autograd", dict(render_fn=render2d))):
        m, opt, gts, _ = setup(True)
        opt.lambda_dist = 100.0
        m.training_setup(opt)
        torch.manual_seed(7)
        losses = [training_iteration(m, cams[i % 4], gts[i % 4], opt, pipe, bg, 8001 + i, scene_extent=3.0, surfels=True,
                                     gt_depth=sensors[i % 4], gt_depth_est=monos[i % 4], **kw)[0].detach() for i in range(8)]
        out[f"gpu/2dgs_late/{name}/n"] = np.array(m.get_xyz.shape[0])
        _state(out, f"gpu/2dgs_late/{name}", m, losses)
    for name, fused in (("fused", None), ("autograd", False)):
        m, opt, gts, _ = setup(False, deg=0)
        with torch.no_grad():
            masks = [(render3d(c, m, pipe, bg)["render_alpha"] > 0.5).float() for c in cams]
        losses = post_refine(m, cams, gts, masks, OptimizationParams(), iterations=16, background=bg, fused_view=fused)
        _state(out, f"gpu/post_refine/{name}", m, losses)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} tensors, {sum(a.nbytes for a in out.values())} bytes -> {path}")


# ---- compare ----
def _compare(a, b, a2=None):
    keys = sorted((set(a) | set(b)) - {"library_source_sha"})
    res = {"tensors": len(keys), "bytes": int(sum(a[k].nbytes for k in keys if k in a)), "equal_in_bytes": 0,
           "parent_runs_differ": [], "expected_different": [], "different": []}
    for k in keys:
        if k not in a or k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape:
            res["different"].append(f"{k}: missing, or another dtype or shape")
        elif a[k].tobytes() == b[k].tobytes() and (a2 is None or k not in a2 or a2[k].tobytes() == a[k].tobytes()):
            res["equal_in_bytes"] += 1
        elif k.startswith(EXPECTED_DIFFERENT) or k.startswith(EXPECTED_DIFFERENT.replace("ranks2/", "ranks2/rank1/")):
            res["expected_different"].append(f"{k}: worst difference {float(np.abs(a[k].astype(np.float64) - b[k]).max()):.3e}")
        elif a2 is not None and k in a2 and a2[k].shape == a[k].shape and a2[k].tobytes() != a[k].tobytes():
            spread = float(np.abs(a[k].astype(np.float64) - a2[k]).max())
            worst = float(np.abs(a[k].astype(np.float64) - b[k]).max())
            note = f"{k}: the parent's two runs differ by {spread:.3e}, this tree from the parent by {worst:.3e}"
            res["parent_runs_differ" if worst <= spread else "different"].append(note)
        else:
            res["different"].append(f"{k}: worst difference {float(np.abs(a[k].astype(np.float64) - b[k]).max()):.3e}")
    return res


def compare(out_path, a_cpu, b_cpu, a_gpu, b_gpu, a2_gpu=None):
    load = lambda p: dict(np.load(p))
    ag, bg = load(a_gpu), load(b_gpu)
    res = {"what": "losses, leaves and Adam state after the loops of scorp_amd/train.py (scripts/dev/train_loop_dump.py), the parent "
                   "commit's checkout against this tree's, a fresh process each; dtype, shape and bytes",
           "library_source_sha": [str(ag["library_source_sha"]), str(bg["library_source_sha"])],
           "cpu": _compare(load(a_cpu), load(b_cpu)), "gpu": _compare(ag, bg, load(a2_gpu) if a2_gpu else None)}
    with open(out_path, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    for half in ("cpu", "gpu"):
        r = res[half]
        print(f"{half}: {r['tensors']} tensors, {r['equal_in_bytes']} equal in bytes, {len(r['parent_runs_differ'])} where the parent's runs differ, "
              f"{len(r['expected_different'])} expected to differ, {len(r['different'])} different")
    return 1 if res["cpu"]["different"] or res["gpu"]["different"] or res["library_source_sha"][0] != res["library_source_sha"][1] else 0


if __name__ == "__main__":
    if len(sys.argv) in (4, 5) and sys.argv[1] == "dump" and sys.argv[2] in ("cpu", "gpu"):
        tree = os.path.abspath(sys.argv[4] if len(sys.argv) == 5 else HERE)
        sys.path.insert(0, tree)
        dump_cpu(sys.argv[3], tree) if sys.argv[2] == "cpu" else dump_gpu(sys.argv[3])
    elif len(sys.argv) in (7, 8) and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
