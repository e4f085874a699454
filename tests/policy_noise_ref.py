"""NumPy restatement of the noise generator of ilqr_policy_monte_carlo (include/ilqr_hip.h): Philox4x32-10 at counter
(s, first_trajectory + b, t, stream), key (seed & 0xffffffff, seed >> 32), and the two transforms of its four words to
unit-variance variates (test helper, not a test module).

UNIFORM is bit-reproducible in float32: every step before its one multiply is exact.  GAUSSIAN is evaluated here in
float64 from u1 and u2, which are exact float32 values; the device's hardware logarithm, root, sine and cosine are held to
GAUSSIAN_BOUND of it.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
SQRT3_F32 = np.float32(float.fromhex("0x1.bb67aep+0"))
STREAM_W, STREAM_X0 = 0, 1
# |z_device - z_float64| for GAUSSIAN: hardware sin / cos err by at most 8e-7 absolute (hw_sincos), the
# radius is at most sqrt(-2 ln 2^-24) = 5.77, plus a few ulp of the radius (log, root, the product), times a margin of 4
GAUSSIAN_BOUND = 2e-5


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) -> (..., 4) uint32; ten rounds, the key bumped between rounds."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                     # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return np.stack(c, axis=-1).astype(np.uint32)


def words(seed, B, S, T, stream, first_trajectory=0):
    """(B, S, T, 4) uint32: the generator's output at every (b, s, t) of one stream"""
    b, s, t = np.meshgrid(np.arange(B, dtype=np.uint64) + first_trajectory, np.arange(S, dtype=np.uint64),
                          np.arange(T, dtype=np.uint64), indexing="ij")
    counter = np.stack([s, b, t, np.full_like(s, stream)], axis=-1)
    return philox4x32_10(counter, np.array([seed & MASK, (seed >> 32) & MASK], dtype=np.uint64))


def uniform_z(r):
    """float32, bit for bit what the device computes"""
    k = (np.asarray(r, dtype=np.uint32) >> np.uint32(9)).astype(np.int64)
    v = (2 * k + 1 - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23)       # exact
    return SQRT3_F32 * v


def gaussian_u(r):
    """(u1, u2) of the pairs (r0, r1), (r2, r3) as float32, both exact; shapes (..., 2)"""
    r = np.asarray(r, dtype=np.uint32)
    ra, rb = r[..., 0::2], r[..., 1::2]
    u1 = (2 * (ra >> np.uint32(9)).astype(np.int64) + 1).astype(np.float32) * np.float32(2.0 ** -24)
    u2 = (rb >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u1, u2


def gaussian_z(r):
    """float64 Box-Muller: z_a = rad cos(2 pi u2), z_b = rad sin(2 pi u2) interleaved as components (0, 1), (2, 3)"""
    u1, u2 = (a.astype(np.float64) for a in gaussian_u(r))
    rad = np.sqrt(-2.0 * np.log(u1))
    z = np.empty(np.shape(r), dtype=np.float64)
    z[..., 0::2] = rad * np.cos(2.0 * np.pi * u2)
    z[..., 1::2] = rad * np.sin(2.0 * np.pi * u2)
    return z


def variates(seed, distribution, B, S, N, n, first_trajectory=0):
    """(z_x0 (B, S, n), z_w (B, S, N, n)): stream 1 at t = 0 and stream 0 at t = 0..N-1, components 0..n-1; float32 for
    "uniform" (exact), float64 for "gaussian" """
    tr = {"uniform": uniform_z, "gaussian": gaussian_z}[distribution]
    zx = tr(words(seed, B, S, 1, STREAM_X0, first_trajectory))[:, :, 0, :n]
    zw = tr(words(seed, B, S, N, STREAM_W, first_trajectory))[..., :n]
    return zx, zw


def uniform_noise(seed, dtype, B, S, N, x0, x0_std, w_std, first_trajectory=0):
    """(x_0 (B, S, n), w (B, S, N, n)) in `dtype`, bit for bit what the device returns for UNIFORM: each product rounded to
    dtype, then added.  x0, x0_std, w_std (B, n)."""
    dt = np.dtype(dtype).type
    n = x0.shape[1]
    zx, zw = variates(seed, "uniform", B, S, N, n, first_trajectory)
    c = lambda a: np.asarray(a).astype(dt)
    x = c(x0)[:, None, :] + c(x0_std)[:, None, :] * c(zx)
    w = c(w_std)[:, None, None, :] * c(zw)
    return x, w
