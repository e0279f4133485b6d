"""The argument checks the point-cloud drivers share (icp, cloud, global_registration, pose_fit): what a cloud argument
must look like, which device a call runs on, and the scalar checks of the cleaning and registration parameters."""
import numpy as np
import torch


def _check_finite(name, a):
    if isinstance(a, torch.Tensor):
        bad_nan, bad_inf = bool(torch.isnan(a).any()), bool(torch.isinf(a).any())
    else:
        a = np.asarray(a)
        bad_nan, bad_inf = bool(np.isnan(a).any()), bool(np.isinf(a).any())
    if bad_nan:
        raise ValueError(f"{name} contains NaN values")
    if bad_inf:
        raise ValueError(f"{name} contains Inf values")


def _check_shape(name, a):
    shape = tuple(np.shape(a))
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError(f"{name} must be [n, 3]; got {shape}")
    if shape[0] == 0:
        raise ValueError(f"{name} is empty")
    if shape[0] >= 2 ** 31:
        raise ValueError(f"{name} has more than 2^31 - 1 points")


def _points(name, a, device):
    _check_shape(name, a)
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(device=device, dtype=torch.float32).contiguous()


def _device(*arrays):
    for a in arrays:
        if isinstance(a, torch.Tensor) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _positive(name, v):
    v = float(v)
    if not (v > 0.0 and np.isfinite(v)):
        raise ValueError(f"{name} must be positive and finite; got {v}")
    return v


def _at_least(name, v, least):
    if int(v) != v or int(v) < least:
        raise ValueError(f"{name} must be an integer >= {least}; got {v}")
    return int(v)


def _cloud(points):
    """The checked cloud as a contiguous fp32 device tensor."""
    _check_shape("points", points)
    if np.shape(points)[0] > 2 ** 30:
        raise ValueError("points has more than 2^30 points")
    _check_finite("points", points)
    return _points("points", points, _device(points))
