"""numpy restatement of the sampler's counter-based generator (DDK_RNG_LAYOUT 1 of include/ddk.h; csrc/k_philox.h, csrc/k_rng.hip).
Words are held as uint64 and masked to 32 bits.  The uniform and torsion conversions use np.float32 operations and are bit-exact; the normals, rotations
and translations are computed in fp64 from the same words (cos / sin of pi x after an exact fold of x onto [-1/4, 1/4]), the yardstick the device's fp32
library functions are measured against."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
PURPOSE = dict(noise=0, initial_torsion=1, initial_rotation=2, initial_translation=3, ar_pick=4, ar_rotation=5)
Z_MAX = float(np.sqrt(48 * np.log(2.0)))      # 5.768: the largest |normal| the conversion can give


def _u64(a):
    return np.asarray(a, dtype=np.uint64)


def philox4x32_10(ctr, key):
    """ctr: four broadcastable arrays of 32-bit words, key: two -> the four output words (uint64 arrays holding 32-bit values)"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[_u64(c) & MASK for c in ctr])
    k0, k1 = _u64(key[0]) & MASK, _u64(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def fnv1a64(name):
    h = 0xcbf29ce484222325
    for byte in str(name).encode('utf-8'):
        h = ((h ^ byte) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def block(seed, stream, sample, purpose, step, blk):
    """the four words [..., 4] of Philox block `blk` of (purpose, step) for the global sample index `sample` (arrays broadcast)"""
    seed, stream = int(seed), int(stream)
    sample, step, blk = _u64(sample), _u64(step), _u64(blk)
    assert (step < 1 << 20).all() and (blk < 256).all() and (sample < 1 << 32).all() and 0 <= purpose < 16
    c3 = (np.uint64(purpose) << np.uint64(28)) | (step << np.uint64(8)) | blk
    return philox4x32_10((stream & 0xFFFFFFFF, stream >> 32, sample, c3), (seed & 0xFFFFFFFF, seed >> 32))


def uniform32(x):
    """fp32, bit-exact: (x >> 8) * 2^-24"""
    return (_u64(x) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def torsion32(x):
    """fp32, bit-exact: (float)pi * (2u - 1)"""
    return np.float32(np.pi) * (np.float32(2) * uniform32(x) - np.float32(1))


def _cossinpi(a):
    """cos(pi a), sin(pi a) in fp64 for a in [0, 2): a is folded onto [-1/4, 1/4] exactly first, so the zeros and the small values keep their relative accuracy"""
    a = np.asarray(a, np.float64)
    k = np.floor(2 * a + 0.5)
    f = np.pi * (a - 0.5 * k)
    cf, sf = np.cos(f), np.sin(f)
    q = k.astype(np.int64) & 3
    c = np.choose(q, [cf, -sf, -cf, sf])
    s = np.choose(q, [sf, cf, -sf, -cf])
    return c, s


def normals64(words):
    """words [..., 4] -> the four normals [..., 4] of the block in fp64 (two Box-Muller pairs, words (0, 1) and (2, 3))"""
    w = _u64(words)
    out = np.empty(w.shape, np.float64)
    for p in (0, 2):
        u1 = ((w[..., p] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24      # (0, 1]
        u2 = (w[..., p + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        c, s = _cossinpi(2 * u2)
        out[..., p], out[..., p + 1] = r * c, r * s
    return out


def rotation64(q):
    """quaternions (x, y, z, w) [..., 4] -> row-major rotation matrices [..., 3, 3], scipy's Rotation.from_quat expressions; |q|^2 < 2^-60: identity"""
    q = np.asarray(q, np.float64)
    n2 = (q * q).sum(-1)
    small = n2 < 2.0 ** -60
    qn = q / np.sqrt(np.where(small, 1.0, n2))[..., None]
    x, y, z, w = (qn[..., i] for i in range(4))
    x2, y2, z2, w2, xy, zw, xz, yw, yz, xw = x * x, y * y, z * z, w * w, x * y, z * w, x * z, y * w, y * z, x * w
    R = np.stack([x2 - y2 - z2 + w2, 2 * (xy - zw), 2 * (xz + yw),
                  2 * (xy + zw), -x2 + y2 - z2 + w2, 2 * (yz - xw),
                  2 * (xz - yw), 2 * (yz + xw), -x2 - y2 + z2 + w2], -1).reshape(q.shape[:-1] + (3, 3))
    R[small] = np.eye(3)
    return R


# ---- the three calls of the C ABI ------------------------------------------------------------------------------------------------------------------------
def noise(seed, stream, sample0, B, step0, steps, n_cols, n_active_cols=None, noise_coeff=None):
    """ddk_rng_noise: [steps, B, n_cols] fp64"""
    n_active_cols = n_cols if n_active_cols is None else n_active_cols
    n_blk = (n_cols + 3) // 4
    k = np.arange(steps)[:, None, None] + step0
    b = np.arange(B)[None, :, None] + sample0
    z = normals64(block(seed, stream, b, PURPOSE['noise'], k, np.arange(n_blk)[None, None, :])).reshape(steps, B, 4 * n_blk)[:, :, :n_cols].copy()
    z[:, :, n_active_cols:] = 0
    if noise_coeff is not None:
        z[~np.asarray(noise_coeff).reshape(steps, 3).any(axis=1)] = 0
    return z


def initial(seed, stream, sample0, B, n_rot, tr_sigma=1.0, purpose_rot=2):
    """ddk_rng_initial: (tor [B, n_rot] fp32 bit-exact, rot [B, 3, 3] fp64, tr [B, 3] fp64)"""
    b = np.arange(B) + sample0
    n_blk = (n_rot + 3) // 4
    tor = torsion32(block(seed, stream, b[:, None], PURPOSE['initial_torsion'], 0, np.arange(n_blk)[None, :])).reshape(B, 4 * n_blk)[:, :n_rot]
    rot = rotation64(normals64(block(seed, stream, b, purpose_rot, 0, 0)))
    tr = np.float64(np.float32(tr_sigma)) * normals64(block(seed, stream, b, PURPOSE['initial_translation'], 0, 0))[:, :3]
    return tor, rot, tr


def uniform(seed, stream, sample0, B, decoding_idx):
    """ddk_rng_uniform: [B] fp32 bit-exact"""
    return uniform32(block(seed, stream, np.arange(B) + sample0, PURPOSE['ar_pick'], decoding_idx, 0)[:, 0])


# ---- the statistical checks both test files run, on the same seeds and counts ----------------------------------------------------------------------------
STAT_SEED, STAT_STREAM = 20240607, fnv1a64('statistics')
STAT_NORMALS = dict(B=1024, steps=1, n_cols=1024)      # N = 2^20 normals through ddk_rng_noise
STAT_ROTATIONS = 1 << 16


def normal_statistics(z):
    """(|mean|, |var - 1|, Kolmogorov-Smirnov distance to the normal CDF) of the flat sample z, in fp64"""
    from scipy.special import ndtr
    z = np.sort(np.asarray(z, np.float64).reshape(-1))
    n = z.size
    cdf = ndtr(z)
    i = np.arange(1, n + 1, dtype=np.float64)
    ks = max(float((i / n - cdf).max()), float((cdf - (i - 1) / n).max()))
    return abs(float(z.mean())), abs(float(z.var()) - 1.0), ks


def normal_statistics_bounds(n):
    """5-sigma widths of the mean and the variance of n N(0,1) draws and the 0.1 % critical value of the Kolmogorov-Smirnov distance"""
    return 5 / np.sqrt(n), 5 * np.sqrt(2 / n), 1.95 / np.sqrt(n)


def rotation_mean_bound(n):
    """every entry of a uniformly random rotation matrix has mean 0 and variance 1/3: 5 sigma of the mean of n"""
    return 5 * np.sqrt(1 / 3) / np.sqrt(n)
