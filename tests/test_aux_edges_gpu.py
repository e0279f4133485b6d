"""The kernels of scorp_amd/csrc/aux_kernels.hip at their block, tile, tail and alignment edges, through the C ABI, against
the float64 yardsticks of tests/aux_reference.py (which tests/test_aux_reference_cpu.py holds to torch and to the golden
tables).  Every buffer a kernel writes is carved out of a larger allocation filled with 0xFF bytes, at least 256 of them
before and behind every region; after the calls every byte outside the regions must still be 0xFF.

Bars and what was measured (MI355X, on the tree of the commit that adds this file, parent 1500973; the module prints the
numbers again at its end, run with -s):

* Adam: truth `adam_step64`; the bar was, per element of p, m, v, |kernel - ref64| <= |adam_step32 - ref64| + 1 ulp.
  Measured: 0 of 2 218 404 elements not bit-equal to `adam_step32` (worst distance 0 ulp) over every case below, the
  scalar form, the late steps and the subnormal squares included, and 0 subnormal exp_avg_sq flushed to zero.  The count
  being zero in every case, the bar IS NOW BIT-EQUALITY to `adam_step32` (adam_one has fp contract(off), no fast-math
  flag in the build); the distance to `adam_step64` is still computed and held to the old bar, which bit-equality
  implies.  Only exp_avg_sq of the subnormal block keeps the old bar plus an absolute 1.2e-38: a flush to zero there
  would be tolerated, counted and printed.
* Transform: worst absolute error against `transform64` per tensor <= 4 x that of the numpy float32 restatement on the
  same 1001-Gaussian cloud (4: the order of a 7-term dot product is free).
  Measured worst errors, kernel / float32 restatement: xyz 7.33e-06 / 7.91e-06, rotation 1.59e-07 / 1.78e-07,
  scaling 2.22e-07 / 2.22e-07, rest 2.29e-07 / 2.43e-07.
* 3-NN: relative error against `knn_mean_dist2_64` <= 4 x the worst relative error of the numpy float32 restatement
  over the same clouds (4: the order of the three-term sums is free); exact zeros exact.
  Measured worst relative errors, kernel / float32 restatement: 1.853e-07 / 1.853e-07.
* Row gather, render tail forward, visibility, max_radii2D and denom: the reference's bits.  Accumulated gradient norm:
  1 ulp.  Render tail backward: 2 ulp, plain zeros where the quotient is not finite.
* Pose score, random maps: |got - (0.25 + scale * sum64)| <= gamma * scale * sum |term| with the derived
  gamma = (k + 6 + 3 + B + 2) * 2^-24 (aux_reference.pose_gamma).  Planted maps: every term exactly zero except at probe
  pixels whose terms are distinct powers of two, and a power-of-two scale (the one at or below 1 / HW: with any other
  scale the rounding of each workgroup's `scale * partial sum` would depend on which probes share a workgroup); the result
  must then EQUAL 0.25 + scale * their sum.

One-line mutations of aux_kernels.hip tried against this module on a scratch copy (never committed):
  guard returning only for blockIdx.x == 0      -> test_adam_guard_skips_every_block_and_counts_once and the FusedAdam test
  `k_rest >= 8` weakened to `k_rest >= 5`       -> test_transform_at_every_band_count_and_block_edge[5-2], [5-3]
  pose tail starting at 4 * Q + threadIdx.x     -> the pose score test at HW 1025, 2097157, 4194311 (aligned)
  `cnt = kKnnTile` in the 3-NN                  -> the 3-NN test at every N but 1023 and 1024 (tests/test_aux_gpu.py sees it too)
  `quad[r] = vec && e[r] + 4 < T.numel`         -> nothing can: the last quad then takes the scalar form, which computes and
                                                   stores the same bits (adam_one is contract(off) in both forms)
  dropping `k < pk.n &&`, removing `s & 0x7FFFFFFFu`: not run, both read or write outside their buffers (an uninitialised
  host table entry as a tensor; a source row 2^31 rows away).  The second cannot pass the gather tests, whose fresh rows of
  the zero_if_fresh == 0 tensors must be copies of row `index & 0x7fffffff`; the first shows only through what the
  host's stack happens to hold behind the live tensors, the launches with 6 and 8 live tensors pin the table itself.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import aux_reference as ref

pytestmark = pytest.mark.gpu

ADAM_BIT_EXACT = True       # the measured count of elements not bit-equal to adam_step32 was zero in every case (docstring)
B1, B2 = 0.9, 0.999


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def L():
    from scorp_amd import _C
    return _C.lib()


@pytest.fixture(scope="module", autouse=True)
def measured():
    """Numbers the docstring quotes, collected over the module and printed at its end."""
    m = {"adam_unequal": 0, "adam_elements": 0, "adam_worst_ulp": 0.0, "adam_flushed_v": 0,
         "transform_kernel": {}, "transform_f32": {}, "knn_kernel": 0.0, "knn_f32": 0.0}
    yield m
    print("\nMEASURED " + repr(m))


def _check(rc, what):
    from scorp_amd import _C
    _C.check(rc, what)


def _stream():
    from scorp_amd import _C
    return ctypes.c_void_p(_C.current_stream_ptr())


class Arena:
    """One allocation of 0xFF bytes; regions are taken from it 256-byte aligned (plus `off` bytes), with at least 256
    untouched bytes before and behind each."""

    def __init__(self, dev, sizes):
        total = 512 + sum(int(s) + 768 for s in sizes)
        self.whole = torch.full((total,), 0xFF, dtype=torch.uint8, device=dev)
        assert self.whole.data_ptr() % 256 == 0 or not self.whole.is_cuda
        self.used = np.zeros(total, dtype=bool)
        self.top = 256

    def take(self, nbytes, off=0, fill=None, dtype=torch.float32):
        start = self.top + off
        assert off % 4 == 0 and start + nbytes + 256 <= self.whole.numel()
        self.used[start:start + nbytes] = True
        self.top = (start + nbytes + 255) // 256 * 256 + 256
        t = self.whole[start:start + nbytes].view(dtype)
        if fill is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(fill)).view(dtype) if isinstance(fill, np.ndarray) else fill)
        return t

    def floats(self, values, off=0):
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        return self.take(4 * values.size, off, values)

    def intact(self):
        free = torch.from_numpy(~self.used).to(self.whole.device)
        return bool((self.whole[free] == 0xFF).all())


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _np(t):
    return t.cpu().numpy().copy()


# ---- Adam -------------------------------------------------------------------------------------------------------------
def _adam_pack(tensors):
    """tensors: (p, g, m, v, lr) device tensors, or (None, None, None, None, lr) for an empty one."""
    from scorp_amd import _C
    arr = (_C.ScorpAdamTensor * len(tensors))()
    for k, (p, g, m, v, lr) in enumerate(tensors):
        if p is not None:
            arr[k].param, arr[k].grad, arr[k].exp_avg, arr[k].exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
            arr[k].numel = p.numel()
        arr[k].lr = lr
    return arr


def _adam_check(measured, got, before, lr, beta1, beta2, eps, step, tag, tiny=False):
    """got (p, m, v) from the kernel, before (p, g, m, v): the bars of the module docstring, element by element."""
    p0, g0, m0, v0 = before
    r64 = ref.adam_step64(p0, g0, m0, v0, float(np.float32(lr)), beta1, beta2, eps, step)
    r32 = ref.adam_step32(p0, g0, m0, v0, np.float32(lr), beta1, beta2, eps, step)
    for name, k, k64, k32 in zip(("param", "exp_avg", "exp_avg_sq"), got, (r64[0], r64[1], r64[2]), (r32[0], r32[1], r32[2])):
        err = np.abs(k.astype(np.float64) - k64)
        bar = np.abs(k32.astype(np.float64) - k64) + ref.ulp32(k32)
        if tiny and name == "exp_avg_sq":
            bar = bar + 1.2e-38                  # a subnormal square flushed to zero is tolerated - and counted
            measured["adam_flushed_v"] += int(((k == 0) & (k32 != 0)).sum())
        unequal = _bits(k) != _bits(k32)
        dist = float((np.abs(k.astype(np.float64) - k32) / ref.ulp32(k32)).max()) if k.size else 0.0
        measured["adam_unequal"] += int(unequal.sum())
        measured["adam_elements"] += k.size
        measured["adam_worst_ulp"] = max(measured["adam_worst_ulp"], dist)
        bad = np.flatnonzero(err > bar)
        assert bad.size == 0, f"{tag} {name}: {bad.size} elements beyond the bar, first {bad[:4]}, got {k[bad[:4]]}, float64 {k64[bad[:4]]}"
        if ADAM_BIT_EXACT and not (tiny and name == "exp_avg_sq"):
            assert not unequal.any(), f"{tag} {name}: {int(unequal.sum())} elements not bit-equal to adam_step32 (worst {dist} ulp)"


@pytest.mark.parametrize("offset", ref.ADAM_OFFSET, ids=lambda o: o or "aligned")
@pytest.mark.parametrize("numel", ref.ADAM_SIZES)
def test_adam_one_tensor_at_the_block_edges_and_off_the_16_byte_grid(numel, offset, dev, L, measured):
    """Steps 1, 2, 3 from zero moments; each step is held against the yardsticks started from the kernel's own state
    before it.  One pointer 4 bytes off a 16-byte boundary sends every element through the scalar form."""
    lr, eps = 2.5e-3, 1e-15
    p0, g0 = ref.adam_inputs(numel, numel)
    arena = Arena(dev, [4 * numel] * 4)
    off = {n: (4 if offset == n else 0) for n in ref.ADAM_OFFSET[1:]}
    p, g = arena.floats(p0, off["param"]), arena.floats(g0, off["grad"])
    m, v = arena.floats(np.zeros(numel), off["exp_avg"]), arena.floats(np.zeros(numel), off["exp_avg_sq"])
    assert all((t.data_ptr() % 16 == 4) == (offset == n) for t, n in zip((p, g, m, v), ref.ADAM_OFFSET[1:]))
    for step in (1, 2, 3):
        before = (_np(p), g0, _np(m), _np(v))
        _check(L.scorp_adam_step(_adam_pack([(p, g, m, v, lr)]), 1, B1, B2, eps, step, _stream()), "adam")
        _adam_check(measured, (_np(p), _np(m), _np(v)), before, lr, B1, B2, eps, step, f"numel {numel} {offset} step {step}")
        assert np.array_equal(_bits(_np(g)), _bits(g0))
    assert arena.intact()


def test_adam_block_of_gradients_whose_squares_are_subnormal(dev, L, measured):
    numel, lr, eps = 4096, 2.5e-3, 1e-15
    p0, g0 = ref.adam_inputs(numel, 77, tiny=True)
    assert 0 < float((g0.astype(np.float32) ** 2).max()) < 1.1754944e-38
    arena = Arena(dev, [4 * numel] * 4)
    p, g, m, v = arena.floats(p0), arena.floats(g0), arena.floats(np.zeros(numel)), arena.floats(np.zeros(numel))
    for step in (1, 2, 3):
        before = (_np(p), g0, _np(m), _np(v))
        _check(L.scorp_adam_step(_adam_pack([(p, g, m, v, lr)]), 1, B1, B2, eps, step, _stream()), "adam")
        _adam_check(measured, (_np(p), _np(m), _np(v)), before, lr, B1, B2, eps, step, f"subnormal squares, step {step}", tiny=True)
    assert arena.intact()
    print(f"subnormal exp_avg_sq flushed to zero by the kernel: {measured['adam_flushed_v']} elements")


@pytest.mark.parametrize("beta1, beta2, eps", ref.ADAM_LATE_CONFIGS, ids=("eps1e-15", "eps1e-8"))
@pytest.mark.parametrize("step", ref.ADAM_LATE_STEPS)
def test_adam_bias_correction_at_a_late_step(step, beta1, beta2, eps, dev, L, measured):
    numel, lr = 4097, 1.6e-4
    p0, g0 = ref.adam_inputs(numel, step)
    m0, v0 = ref.adam_moments(numel, step)
    arena = Arena(dev, [4 * numel] * 4)
    p, g, m, v = arena.floats(p0), arena.floats(g0), arena.floats(m0), arena.floats(v0)
    _check(L.scorp_adam_step(_adam_pack([(p, g, m, v, lr)]), 1, beta1, beta2, eps, step, _stream()), "adam")
    _adam_check(measured, (_np(p), _np(m), _np(v)), (p0, g0, m0, v0), lr, beta1, beta2, eps, step, f"step {step} eps {eps}")
    assert arena.intact()


def test_adam_eight_tensors_in_one_launch_each_with_its_own_lr_and_extent(dev, L, measured):
    """4097, 0, 1, 4096, 0, 8193, 3, 12289 elements back to back in one arena: the two empty ones are passed as NULL and
    skipped (six tensors reach the kernel), every other one must get its own lr over its own extent."""
    sizes, lrs, eps, step = ref.ADAM_PACK_SIZES, ref.ADAM_PACK_LR, 1e-15, 2
    arena = Arena(dev, [4 * n for n in sizes for _ in range(4)])
    host, tensors = [], []
    for k, (n, lr) in enumerate(zip(sizes, lrs)):
        if n == 0:
            host.append(None)
            tensors.append((None, None, None, None, lr))
            continue
        p0, g0 = ref.adam_inputs(n, 50 + k)
        m0, v0 = ref.adam_moments(n, 50 + k)
        host.append((p0, g0, m0, v0))
        tensors.append((arena.floats(p0), arena.floats(g0), arena.floats(m0), arena.floats(v0), lr))
    _check(L.scorp_adam_step(_adam_pack(tensors), 8, B1, B2, eps, step, _stream()), "adam")
    for k, (h, t) in enumerate(zip(host, tensors)):
        if h is not None:
            _adam_check(measured, (_np(t[0]), _np(t[2]), _np(t[3])), h, t[4], B1, B2, eps, step, f"tensor {k} of 8")
            assert np.array_equal(_bits(_np(t[1])), _bits(h[1]))
    assert arena.intact()
    # eight live tensors: the last slot of the block -> tensor table is used too
    sizes8 = (1, 4097, 2, 4096, 8193, 3, 5, 4095)
    arena = Arena(dev, [4 * n for n in sizes8 for _ in range(4)])
    host, tensors = [], []
    for k, n in enumerate(sizes8):
        p0, g0 = ref.adam_inputs(n, 80 + k)
        m0, v0 = ref.adam_moments(n, 80 + k)
        host.append((p0, g0, m0, v0))
        tensors.append((arena.floats(p0), arena.floats(g0), arena.floats(m0), arena.floats(v0), lrs[7 - k]))
    _check(L.scorp_adam_step(_adam_pack(tensors), 8, B1, B2, eps, step, _stream()), "adam")
    for k, (h, t) in enumerate(zip(host, tensors)):
        _adam_check(measured, (_np(t[0]), _np(t[2]), _np(t[3])), h, t[4], B1, B2, eps, step, f"tensor {k} of 8 live")
    assert arena.intact()


def test_fused_adam_steps_seventeen_parameters_in_three_launches_and_counts_a_skipped_step_once(dev, L, measured, monkeypatch):
    """17 parameters, each its own group and lr, two (betas, eps) configurations interleaved: FusedAdam.step sorts them into
    9 + 8, i.e. launches of 8, 1 and 8 tensors; the skip counter goes to the first launch only."""
    from scorp_amd.fused_adam import FusedAdam
    sizes = (5, 4097, 1, 300, 7, 4096, 33, 2, 1000, 8193, 3, 64, 129, 4095, 17, 256, 12289)
    cfgs = (((0.9, 0.999), 1e-15), ((0.8, 0.99), 1e-8))
    arena = Arena(dev, [4 * n for n in sizes for _ in range(3)] + [4])
    params, host, groups = [], [], []
    for k, n in enumerate(sizes):
        p0, g0 = ref.adam_inputs(n, 200 + k)
        p = torch.nn.Parameter(arena.floats(p0))
        p.grad = torch.from_numpy(g0).to(dev)
        betas, eps = cfgs[k % 2]
        lr = 1e-4 * (k + 1)
        groups.append({"params": [p], "lr": lr, "betas": betas, "eps": eps})
        params.append(p)
        host.append((p0, g0, betas, eps, lr))
    opt = FusedAdam(groups, lr=0.0)
    for p in params:
        opt.state[p] = {"step": torch.tensor(0.0), "exp_avg": arena.floats(np.zeros(p.numel())),
                        "exp_avg_sq": arena.floats(np.zeros(p.numel()))}
    calls = []
    real = L.scorp_adam_step_guarded_ex

    def counting(arr, n, b1, b2, eps, step, skip, count, stream):
        calls.append((n, b1, eps, step, skip is not None, count is not None))
        return real(arr, n, b1, b2, eps, step, skip, count, stream)
    monkeypatch.setattr(L, "scorp_adam_step_guarded_ex", counting)
    opt.step()
    assert [(c[0], c[2]) for c in calls] == [(8, 1e-15), (1, 1e-15), (8, 1e-8)] and not any(c[4] or c[5] for c in calls)
    for k, (p, (p0, g0, betas, eps, lr)) in enumerate(zip(params, host)):
        st = opt.state[p]
        zero = np.zeros_like(p0)
        _adam_check(measured, (_np(p.data), _np(st["exp_avg"]), _np(st["exp_avg_sq"])), (p0, g0, zero, zero), lr, betas[0], betas[1],
                    eps, 1, f"FusedAdam parameter {k}")
    assert arena.intact() and opt.take_skipped() == 0
    # a skipped step: nothing moves, and the three launches count it once
    skip = arena.take(4, dtype=torch.int32)
    skip.fill_(1)
    snapshot = arena.whole.clone()
    del calls[:]
    opt.skip_flag = skip
    opt.step()
    assert [c[4:] for c in calls] == [(True, True), (True, False), (True, False)]
    assert torch.equal(arena.whole, snapshot)
    assert opt.take_skipped() == 1 and opt.take_skipped() == 0
    assert all(int(opt.state[p]["step"]) == 2 for p in params)
    opt.rollback_steps(1)
    assert all(int(opt.state[p]["step"]) == 1 for p in params)


def test_adam_guard_skips_every_block_and_counts_once(dev, L, measured):
    numel, lr, eps, step = 3 * 4096 + 1, 2.5e-3, 1e-15, 4
    p0, g0 = ref.adam_inputs(numel, 9)
    m0, v0 = ref.adam_moments(numel, 9)
    arena = Arena(dev, [4 * numel] * 4 + [4, 4])
    p, g, m, v = arena.floats(p0), arena.floats(g0), arena.floats(m0), arena.floats(v0)
    word, counter = arena.take(4, dtype=torch.int32), arena.take(4, dtype=torch.int32)
    word.fill_(1)
    counter.fill_(5)
    pack = _adam_pack([(p, g, m, v, lr)])
    before = arena.whole.clone()
    _check(L.scorp_adam_step_guarded_ex(pack, 1, B1, B2, eps, step, _ptr(word), _ptr(counter), _stream()), "adam")
    assert int(counter.item()) == 6 and int(word.item()) == 1
    counter.fill_(5)
    assert torch.equal(arena.whole, before)                       # every block of p, m, v, bit for bit
    _check(L.scorp_adam_step_guarded_ex(pack, 1, B1, B2, eps, step, _ptr(word), None, _stream()), "adam")
    _check(L.scorp_adam_step_guarded(pack, 1, B1, B2, eps, step, _ptr(word), _stream()), "adam")
    assert torch.equal(arena.whole, before)
    # the word 0: the unguarded call's bits, and nothing counted
    word.fill_(0)
    _check(L.scorp_adam_step_guarded_ex(pack, 1, B1, B2, eps, step, _ptr(word), _ptr(counter), _stream()), "adam")
    guarded = arena.whole.clone()
    assert int(counter.item()) == 5
    for t, h in ((p, p0), (m, m0), (v, v0)):
        t.copy_(torch.from_numpy(h))
    _check(L.scorp_adam_step(pack, 1, B1, B2, eps, step, _stream()), "adam")
    assert torch.equal(arena.whole, guarded) and not torch.equal(arena.whole, before)
    _adam_check(measured, (_np(p), _np(m), _np(v)), (p0, g0, m0, v0), lr, B1, B2, eps, step, "guard word 0")
    assert arena.intact()


# ---- row gather -------------------------------------------------------------------------------------------------------
def _gather(L, dev, row_floats, zero_if_fresh, n_out, seed, n_tensors=None):
    from scorp_amd import _C
    n = len(row_floats) if n_tensors is None else n_tensors
    rng = np.random.default_rng(seed)
    idx = ref.gather_index(n_out, ref.GATHER_SRC_ROWS, seed)
    srcs = [rng.normal(0.0, 1.0, (ref.GATHER_SRC_ROWS, w)).astype(np.float32) for w in row_floats]
    arena = Arena(dev, [4 * max(n_out, 1) * w for w in row_floats])
    nan = np.float32(np.nan)
    dsts = [arena.floats(np.full(max(n_out, 1) * w, nan)) for w in row_floats]
    dev_src = [torch.from_numpy(s).to(dev) for s in srcs]
    dev_idx = torch.from_numpy(idx if n_out else np.zeros(1, np.int32)).to(dev)
    arr = (_C.ScorpRowTensor * max(n, 1))()
    for k in range(n):
        arr[k].src, arr[k].dst = dev_src[k].data_ptr(), dsts[k].data_ptr()
        arr[k].row_floats, arr[k].zero_if_fresh = row_floats[k], zero_if_fresh[k]
    _check(L.scorp_gather_rows(arr, n, _ptr(dev_idx), n_out, _stream()), "gather_rows")
    got = [_np(d) for d in dsts]
    for s, d in zip(srcs, dev_src):
        assert np.array_equal(_bits(_np(d)), _bits(s))
    assert arena.intact()
    return got, ref.gather_rows(srcs, row_floats, zero_if_fresh, idx), idx


@pytest.mark.parametrize("n_out", ref.GATHER_N_OUT)
def test_gather_rows_of_different_widths_in_one_launch(n_out, dev, L):
    """Row widths 1, 3, 4, 45, 48, 3, 1, 4 (the grid is sized by the widest), zero_if_fresh alternating: a fresh row is a
    copy of row `index & 0x7fffffff` for the tensors that do not ask for zeros and +0.0 for those that do."""
    widths = ref.GATHER_ROW_FLOATS
    zero = tuple(k % 2 for k in range(len(widths)))
    got, want, idx = _gather(L, dev, widths, zero, n_out, n_out)
    fresh = (idx.view(np.uint32) >> 31).astype(bool)
    assert n_out < 255 or fresh.sum() > 20
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1)), f"tensor {k} (row_floats {widths[k]}, zero_if_fresh {zero[k]})"
        rows = _bits(a).reshape(n_out, widths[k])[fresh]
        assert bool((rows == 0).all()) == bool(zero[k]) or not fresh.any()          # +0.0, not -0.0, not the NaN fill


def test_gather_rows_with_the_most_tensors_a_launch_takes(dev, L):
    widths = tuple(1 + (k % 5) for k in range(24))
    got, want, _ = _gather(L, dev, widths, tuple((k // 3) % 2 for k in range(24)), 257, 24)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(_bits(a).reshape(-1), _bits(b).reshape(-1)), f"tensor {k}"


def test_gather_rows_with_nothing_to_do_launches_nothing(dev, L):
    got, _, _ = _gather(L, dev, (3, 4), (0, 1), 0, 5)                  # no output rows
    assert all(np.isnan(g).all() for g in got)
    got, _, _ = _gather(L, dev, (3, 4), (0, 1), 7, 5, n_tensors=0)     # no tensors
    assert all(np.isnan(g).all() for g in got)


# ---- transform --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _golden():
    import os
    return dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "wigner_d.npz")))


def _transform_call(L, dev, parts, n, k_rest, dims, P, null=None):
    """-> (xyz, rot, scaling, rest) after the call (numpy), parts = the float32 inputs; `null`: the one passed as NULL."""
    arena = Arena(dev, [a.nbytes for a in parts] + [420])
    t = [arena.floats(a) for a in parts]
    block = arena.floats(ref.transform_block(P))
    args = [None if null == name else _ptr(x) for name, x in zip(("xyz", "rot", "scaling", "rest"), t)]
    _check(L.scorp_gaussians_transform(args[0], args[1], args[2], args[3], n, k_rest, dims, _ptr(block), _stream()), "transform")
    out = [_np(x).reshape(a.shape) for x, a in zip(t, parts)]
    assert np.array_equal(_bits(_np(block)), _bits(ref.transform_block(P))) and arena.intact()
    return out


@pytest.mark.parametrize("dims", ref.TRANSFORM_DIMS)
@pytest.mark.parametrize("k_rest", ref.TRANSFORM_K_REST)
def test_transform_at_every_band_count_and_block_edge(k_rest, dims, dev, L, measured):
    """N = 1, 255, 256, 257, 1001 are the leading rows of one cloud around (100, -50, 30) with quaternion norms 0.1 .. 10,
    anisotropic scale, rotation and blocks from the golden table; the float32 restatement's error is taken once, on the
    whole cloud.  The coefficients of an incomplete band, and a tensor passed as NULL, keep their bits."""
    P = ref.transform_params(_golden(), (k_rest + dims) % 8)
    full = ref.transform_inputs(1001, k_rest, dims, 10 * k_rest + dims)
    want = ref.transform64(*full, dims=dims, **P)
    f32 = ref.transform32(*full, dims=dims, **P)
    names = ("xyz", "rotation", "scaling", "rest")
    err32 = {nm: float(np.abs(a.astype(np.float64) - w).max()) if w.size else 0.0 for nm, a, w in zip(names, f32, want)}
    done = max([first + width for first, width in ref._bands(k_rest)] + [0])
    assert done == {0: 0, 1: 0, 3: 3, 5: 3, 8: 8, 12: 8, 15: 15}[k_rest]
    for n in ref.TRANSFORM_N:
        parts = [a[:n] for a in full]
        got = _transform_call(L, dev, parts, n, k_rest, dims, P)
        for nm, a, w in zip(names, got, want):
            err = float(np.abs(a.astype(np.float64) - w[:n]).max()) if a.size else 0.0
            key = f"{nm}"
            measured["transform_kernel"][key] = max(measured["transform_kernel"].get(key, 0.0), err)
            measured["transform_f32"][key] = max(measured["transform_f32"].get(key, 0.0), err32[nm])
            assert err <= 4 * err32[nm], f"{nm} at N={n}: kernel {err:.3g}, float32 restatement {err32[nm]:.3g}"
        assert np.array_equal(_bits(got[3][:, done:]), _bits(parts[3][:, done:]))
    n = 257
    parts = [a[:n] for a in full]
    for null, slot in (("rot", 1), ("scaling", 2), ("rest", 3)):
        got = _transform_call(L, dev, parts, n, k_rest, dims, P, null=null)
        assert np.array_equal(_bits(got[slot]), _bits(parts[slot])), f"{null} passed as NULL was written"
        for j, (nm, a, w) in enumerate(zip(names, got, want)):
            if j != slot and a.size:
                assert float(np.abs(a.astype(np.float64) - w[:n]).max()) <= 4 * err32[nm], f"{nm} with {null} = NULL"


# ---- view statistics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride, comps", ref.STATS_FORMS)
@pytest.mark.parametrize("n", ref.STATS_N)
def test_view_statistics_two_views_and_a_skipped_one(n, stride, comps, dev, L):
    state, views = ref.stats_inputs(n, stride, 100 * n + 10 * stride + comps)
    arena = Arena(dev, [4 * n] * 3 + [4])
    mx, ac, de = (arena.floats(s) for s in state)
    word = arena.take(4, dtype=torch.int32)
    word.fill_(0)
    for k, (radii, vis, grad) in enumerate(views):
        d_r, d_v, d_g = torch.from_numpy(radii).to(dev), torch.from_numpy(vis).to(dev), torch.from_numpy(grad).to(dev)
        before = (_np(mx), _np(ac), _np(de))
        if comps == 2 and k == 1:
            rc = L.scorp_densification_stats(n, _ptr(d_r), _ptr(d_v), _ptr(d_g), stride, _ptr(word), _ptr(mx), _ptr(ac), _ptr(de), _stream())
        else:
            rc = L.scorp_densification_stats_ex(n, _ptr(d_r), _ptr(d_v), _ptr(d_g), stride, comps, None if k == 0 else _ptr(word),
                                                _ptr(mx), _ptr(ac), _ptr(de), _stream())
        _check(rc, "stats")
        w_mx, w_ac, w_de = ref.densification_stats64(radii, vis, grad, comps, *before)
        g_mx, g_ac, g_de = _np(mx), _np(ac), _np(de)
        assert np.array_equal(_bits(g_mx), _bits(w_mx)) and np.array_equal(_bits(g_de), _bits(w_de))
        w32 = w_ac.astype(np.float32)
        assert np.all(np.abs(g_ac.astype(np.float64) - w32) <= ref.ulp32(w32)), f"view {k}"
        off = vis == 0
        for got, was in zip((g_mx, g_ac, g_de), before):
            assert np.array_equal(_bits(got)[off], _bits(was)[off])
        assert n < 3 or not np.array_equal(_bits(g_ac), _bits(before[1]))
    word.fill_(1)
    before = arena.whole.clone()
    _check(L.scorp_densification_stats_ex(n, _ptr(d_r), _ptr(d_v), _ptr(d_g), stride, comps, _ptr(word), _ptr(mx), _ptr(ac), _ptr(de),
                                          _stream()), "stats")
    assert torch.equal(arena.whole, before) and arena.intact()


# ---- pose score -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _pose_case(hw):
    rnd = ref.pose_maps(hw, hw)
    terms = ref.pose_score_terms64(*rnd)
    planted = ref.pose_planted(hw, hw)
    return rnd, float(terms.sum()), float(np.abs(terms).sum()), planted[:4], planted[4]


def _pose_call(L, dev, maps, offset, scale, acc):
    bufs = []
    for name, x in zip(ref.POSE_OFFSET[1:], maps):
        off = 1 if offset == name else 0
        buf = torch.empty(x.size + 4, dtype=torch.float32, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = buf[off:off + x.size]
        view.copy_(torch.from_numpy(x))
        bufs.append(view)
    _check(L.scorp_gs3d_pose_score_accumulate(_ptr(bufs[0]), _ptr(bufs[1]), _ptr(bufs[2]), _ptr(bufs[3]), maps[0].size,
                                              ctypes.c_float(scale), _ptr(acc), _stream()), "pose_score")
    return float(acc.item())


@pytest.mark.parametrize("offset", ref.POSE_OFFSET, ids=lambda o: o or "aligned")
@pytest.mark.parametrize("hw", ref.POSE_HW)
def test_pose_score_random_maps_inside_the_derived_bound_and_planted_probes_exactly(hw, offset, dev, L):
    rnd, total, total_abs, planted, probes = _pose_case(hw)
    arena = Arena(dev, [4, 4])
    acc = arena.floats(np.array([0.25]))
    scale = float(np.float32(1.0 / hw))
    got = _pose_call(L, dev, rnd, offset, scale, acc)
    want = 0.25 + scale * total
    bound = ref.pose_gamma(hw) * scale * total_abs
    print(f"pose score HW={hw} {offset}: |got - want| = {abs(got - want):.3g}, bound {bound:.3g}")
    assert abs(got - want) <= bound, (got, want, bound)
    acc2 = arena.floats(np.array([0.25]))
    pscale = ref.pose_planted_scale(hw)
    got = _pose_call(L, dev, planted, offset, pscale, acc2)
    want = 0.25 + pscale * sum(probes.values())
    missing = (want - got) / pscale
    assert got == want, f"planted probes {probes}: result off by {missing} (in units of one probe term 2^0)"
    assert arena.intact()


# ---- render tail ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw, n", ref.TAIL_SHAPES)
def test_render_tail_with_more_gaussians_than_pixels_and_none_of_either(hw, n, dev, L):
    depth, alpha, g, radii = ref.tail_inputs(hw, n, hw + n)
    assert ref.double_rounding_cases(depth, alpha) == 0
    want, want_vis = ref.render_tail64(depth, alpha, radii)
    arena = Arena(dev, [4 * hw, n, 4 * hw, 4 * hw])
    out, vis = arena.take(4 * hw), arena.take(n, dtype=torch.uint8)
    d_d, d_a, d_g, d_r = (torch.from_numpy(x).to(dev) if x.size else None for x in (depth, alpha, g, radii))
    _check(L.scorp_gs3d_render_tail(_ptr(d_d), _ptr(d_a), hw, _ptr(d_r), n, _ptr(out) if hw else None, _ptr(vis) if n else None,
                                    _stream()), "render_tail")
    with np.errstate(over="ignore"):
        assert np.array_equal(_bits(_np(out)), _bits(want.astype(np.float32)))
    assert np.array_equal(_np(vis), want_vis.astype(np.uint8))
    if hw:
        assert want[1] == 0 and want[3] == 0 and want[2] > 9e29
    if n:
        assert (radii < 0).any() and not want_vis[radii < 0].any()
    # backward
    g_d, g_a = arena.take(4 * hw), arena.take(4 * hw)
    _check(L.scorp_gs3d_render_tail_backward(_ptr(d_g), _ptr(d_d), _ptr(d_a), hw, _ptr(g_d) if hw else None, _ptr(g_a) if hw else None,
                                             _stream()), "render_tail_backward")
    w_d, w_a = ref.render_tail_backward64(g, depth, alpha)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dead = ~((alpha != 0) & np.isfinite((depth.astype(np.float64) / alpha.astype(np.float64)).astype(np.float32)))
        for got, w64, name in ((_np(g_d), w_d, "g_depth"), (_np(g_a), w_a, "g_alpha")):
            assert np.array_equal(_bits(got)[dead], np.zeros(int(dead.sum()), np.int32)), name       # plain +0.0
            w32 = w64.astype(np.float32)
            same_inf = np.isinf(w32) & (got == w32)
            finite = ~dead & ~same_inf
            assert not np.isinf(w32[finite]).any() and np.isfinite(got[finite]).all(), name
            assert np.all(np.abs(got[finite].astype(np.float64) - w64[finite]) <= 2 * ref.ulp32(w32[finite])), name
    assert hw == 0 or dead.sum() > hw // 8
    assert arena.intact()


# ---- 3-NN -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _knn_cases():
    cases, worst32 = {}, 0.0
    for n in ref.KNN_N:
        pts = ref.knn_points(n)
        want, f32 = ref.knn_mean_dist2_64(pts), ref.knn_mean_dist2_32(pts)
        ok = want > 0
        assert np.all(f32[~ok] == 0)
        if ok.any():
            worst32 = max(worst32, float((np.abs(f32[ok] - want[ok]) / want[ok]).max()))
        cases[n] = (pts, want)
    return cases, worst32


@pytest.mark.parametrize("n", ref.KNN_N)
def test_knn_at_the_tile_and_block_edges_with_duplicates_and_far_copies(n, dev, L, measured):
    cases, worst32 = _knn_cases()
    pts, want = cases[n]
    arena = Arena(dev, [4 * n])
    out = arena.take(4 * n)
    d_pts = torch.from_numpy(pts).to(dev)
    _check(L.scorp_knn_dist2(_ptr(d_pts), n, _ptr(out), _stream()), "knn")
    got = _np(out)
    assert arena.intact() and np.array_equal(_bits(_np(d_pts)), _bits(pts))
    ok = want > 0
    assert np.array_equal(_bits(got)[~ok], np.zeros(int((~ok).sum()), np.int32))          # exact zeros are exact
    if n >= 255:
        half = (n + 1) // 2
        assert not ok[3:8].any() and not ok[half + 3:half + 8].any() and ok[20] and ok[21]
    rel = float((np.abs(got[ok] - want[ok]) / want[ok]).max()) if ok.any() else 0.0
    measured["knn_kernel"], measured["knn_f32"] = max(measured["knn_kernel"], rel), worst32
    assert rel <= 4 * worst32, f"N={n}: kernel {rel:.3g}, float32 restatement {worst32:.3g}"
