"""Import-path shim: ``from pre_set_prop import set_PRE`` (Inverse_residuals/Python/pre_set_prop.py:29)."""
import numpy as np

from cp_pre_amd.set_prop import Interval, _intervals, set_pre_bounds  # noqa: F401


def compute_inverse(kernel_fft, eps=1e-16):
    """``pre_set_prop.py:16``: the regularised inverse of a kernel spectrum."""
    return 1.0 / (kernel_fft + eps)


def set_PRE(neural_test):
    """``pre_set_prop.py:29-91``: bounds on ``neural_test[:, 0]`` for the fixed SHO operator m = k = 1, dt = 0.1010101
    (kernel ``[1, -2, 1] + dt^2 [0, 1, 0]``, eps = 1e-16), as a list of Nt + 1 ``Interval``."""
    m, k, dt = 1, 1, 0.1010101
    kernel = m * np.array([1, -2, 1]) + dt ** 2 * k * np.array([0, 1, 0])
    return _intervals(*set_pre_bounds(neural_test[:, 0], kernel, eps=1e-16))
