"""NumPy restatement of the parameter draw of ilqr_set_param_spread (include/ilqr_hip.h) on top of the generator of
policy_noise_ref (test helper, not a test module): parameter j of sample s of trajectory b takes component j mod 4 of the
Philox call at counter (s, first_trajectory + b, 1 + j // 4, 1), clamped to [-c, c] with c = float32(clip), and
    p = base + sd * float64(clamp(z))
with the product and the add rounded separately, as NumPy does.  UNIFORM is exact; GAUSSIAN is evaluated in float64 and the
device's variate is held to GAUSSIAN_BOUND of it.
"""
import numpy as np

from policy_noise_ref import GAUSSIAN_BOUND, MASK, STREAM_X0, gaussian_z, philox4x32_10, uniform_z  # noqa: F401


def counters(B, S, n_sys, first_trajectory=0):
    """(B, S, G, 4) uint64: the counter of every generator call, G = ceil(n_sys / 4) groups per sample"""
    G = (n_sys + 3) // 4
    b, s, g = np.meshgrid(np.arange(B, dtype=np.uint64) + np.uint64(first_trajectory), np.arange(S, dtype=np.uint64),
                          np.arange(G, dtype=np.uint64), indexing="ij")
    return np.stack([s, b, g + np.uint64(1), np.full_like(s, STREAM_X0)], axis=-1)


def x0_counters(B, S, first_trajectory=0):
    """(B, S, 2, 4) uint64: the counters of the x_0 draw on the same stream, groups 0 and 1 (third word 0 and 2^31)"""
    b, s, g = np.meshgrid(np.arange(B, dtype=np.uint64) + np.uint64(first_trajectory), np.arange(S, dtype=np.uint64),
                          np.arange(2, dtype=np.uint64), indexing="ij")
    return np.stack([s, b, g << np.uint64(31), np.full_like(s, STREAM_X0)], axis=-1)


def variates(seed, distribution, B, S, n_sys, first_trajectory=0):
    """z (B, S, n_sys) before the clamp: float32 for "uniform" (exact), float64 for "gaussian".  The transform is applied to
    whole four-word calls and the components are sliced afterwards (the Gaussian transform pairs the words)."""
    key = np.array([seed & MASK, (seed >> 32) & MASK], dtype=np.uint64)
    r = philox4x32_10(counters(B, S, n_sys, first_trajectory), key)               # (B, S, G, 4)
    z = {"uniform": uniform_z, "gaussian": gaussian_z}[distribution](r)
    return z.reshape(B, S, -1)[:, :, :n_sys]


def spread_sd(base, std, relative):
    """sd (B, n_sys): |base| * std, one rounded double product, or std"""
    base, std = np.asarray(base, dtype=np.float64), np.asarray(std, dtype=np.float64)
    return np.abs(base) * std if relative else std.copy()


def draw(seed, distribution, base, std, relative, clip, S, first_trajectory=0):
    """(p (B, S, n_sys) float64, clamped (B, S, n_sys) bool): the drawn parameters and which variates the clamp moved.
    base, std (B, n_sys).  Bit for bit the device's for "uniform"."""
    base = np.asarray(base, dtype=np.float64)
    B, n_sys = base.shape
    sd = spread_sd(base, std, relative)
    c = np.float32(clip)
    z = variates(seed, distribution, B, S, n_sys, first_trajectory)
    zc = np.clip(z, -c, c) if z.dtype == np.float32 else np.clip(z, -float(c), float(c))
    e = sd[:, None, :] * zc.astype(np.float64)        # rounded on its own
    return base[:, None, :] + e, np.abs(z) > c
