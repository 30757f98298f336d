"""Independent CPU reference for the hit-and-run kernel (k_hit_and_run, mpc_hit_and_run): numpy and scipy only, no code of
ppopt_amd.  A plain helper module (not a conftest), imported by tests/test_hit_and_run_cpu.py and tests/test_gpu_hit_and_run.py.

* ``philox4x32_10``: the counter-based generator of Salmon et al. (SC'11) with the Random123 constants, vectorised over counters.
* ``chains``: the chain of DESIGN §3.11 replayed for all chains of one polytope at once.
* ``ks_uniform`` / ``ks_cdf`` / ``chi2_cells``: the statistics of the distribution tests, with the thresholds they use.
"""
import numpy
import scipy.stats

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = numpy.uint64(0xffffffff)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counter words (arrays or scalars, broadcast) under the key (k0, k1) -> four uint64 arrays of 32-bit words."""
    c = [numpy.asarray(v, dtype=numpy.uint64) & _MASK for v in numpy.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = numpy.uint64(k0), numpy.uint64(k1)
    for r in range(10):
        if r:
            k0 = (k0 + numpy.uint64(W0)) & _MASK
            k1 = (k1 + numpy.uint64(W1)) & _MASK
        p0 = numpy.uint64(M0) * c[0]
        p1 = numpy.uint64(M1) * c[2]
        c = [((p1 >> numpy.uint64(32)) ^ c[1] ^ k0) & _MASK, p1 & _MASK, ((p0 >> numpy.uint64(32)) ^ c[3] ^ k1) & _MASK, p0 & _MASK]
    return c


def u53(a, b):
    """((a >> 5) 2^26 + (b >> 6)) 2^-53, in [0, 1)."""
    a = numpy.asarray(a, dtype=numpy.uint64)
    b = numpy.asarray(b, dtype=numpy.uint64)
    return ((a >> numpy.uint64(5)).astype(numpy.float64) * 67108864.0 + (b >> numpy.uint64(6)).astype(numpy.float64)) * 2.0 ** -53


def chains(A, b, start, n_chains, samples, n_steps, seed, p=0, chain_ids=None):
    """The chains k of polytope p (global ids g = p * n_chains + k) in {x : A x <= b} from ``start``.  Returns
    (samples [len(chain_ids), samples, n], status [len(chain_ids)]); status 0 ok, 1 start outside, 2 unbounded (NaN samples)."""
    A = numpy.asarray(A, dtype=float).reshape(-1, len(start))
    b = numpy.asarray(b, dtype=float).reshape(-1)
    n = A.shape[1]
    ks = numpy.arange(n_chains) if chain_ids is None else numpy.asarray(chain_ids)
    g = numpy.uint64(p) * numpy.uint64(n_chains) + ks.astype(numpy.uint64)
    g_lo, g_hi = g & _MASK, g >> numpy.uint64(32)
    k0, k1 = seed & 0xffffffff, seed >> 32
    C = len(ks)
    th = numpy.tile(numpy.asarray(start, dtype=float).reshape(1, n), (C, 1))
    status = numpy.zeros(C, dtype=numpy.int32)
    out = numpy.full((C, samples, n), numpy.nan)
    npairs = (n + 1) // 2
    for s in range(samples * n_steps):
        live = status == 0
        if not live.any():
            break
        z = numpy.zeros((C, 2 * npairs))
        for j in range(npairs):
            r = philox4x32_10(g_lo, g_hi, s, j, k0, k1)
            u1, u2 = 1.0 - u53(r[0], r[1]), u53(r[2], r[3])
            rad = numpy.sqrt(-2.0 * numpy.log(u1))
            z[:, 2 * j] = rad * numpy.cos(2.0 * numpy.pi * u2)
            z[:, 2 * j + 1] = rad * numpy.sin(2.0 * numpy.pi * u2)
        z = z[:, :n]
        d = z / numpy.linalg.norm(z, axis=1, keepdims=True)
        S = b[None, :] - th @ A.T
        G = d @ A.T
        with numpy.errstate(divide='ignore', invalid='ignore'):
            ratio = S / G
        t_hi = numpy.where(G > 0, ratio, numpy.inf).min(axis=1, initial=numpy.inf)
        t_lo = numpy.where(G < 0, ratio, -numpy.inf).max(axis=1, initial=-numpy.inf)
        if s == 0:
            status[live & (S.min(axis=1, initial=numpy.inf) < 0)] = 1
        status[(status == 0) & live & ~(numpy.isfinite(t_hi) & numpy.isfinite(t_lo))] = 2
        go = live & (status == 0)
        r = philox4x32_10(g_lo, g_hi, s, npairs, k0, k1)
        with numpy.errstate(invalid='ignore'):
            t = t_lo + u53(r[0], r[1]) * (t_hi - t_lo)
            acc = go & ((S - t[:, None] * G).min(axis=1, initial=numpy.inf) >= 0)
        th[acc] = th[acc] + t[acc, None] * d[acc]
        if (s + 1) % n_steps == 0:
            q = (s + 1) // n_steps - 1
            ok = status == 0
            out[ok, q] = th[ok]
    out[status != 0] = numpy.nan
    return out, status


# ---- distribution statistics --------------------------------------------------------------------------------------------
def ks_cdf(x, cdf):
    """Kolmogorov-Smirnov statistic of the sample x against the continuous CDF ``cdf``."""
    x = numpy.sort(numpy.asarray(x, dtype=float).ravel())
    N = len(x)
    F = cdf(x)
    return float(max(numpy.max(numpy.arange(1, N + 1) / N - F), numpy.max(F - numpy.arange(N) / N)))


def ks_limit(N):
    """The issue's threshold 1.95 / sqrt(N) (about the 0.1 % point of the KS distribution)."""
    return 1.95 / numpy.sqrt(N)


def check_uniform_box(X, lo, hi):
    """Every coordinate of X [N, n] uniform on [lo_j, hi_j]: KS <= 1.95/sqrt(N) and the mean within 4 sigma.  Returns the worst
    (KS / limit, |mean error| / 4 sigma)."""
    X = numpy.asarray(X, dtype=float)
    N = len(X)
    U = (X - lo) / (hi - lo)
    ks = max(ks_cdf(U[:, j], lambda v: numpy.clip(v, 0, 1)) for j in range(U.shape[1]))
    mean = numpy.max(numpy.abs(U.mean(axis=0) - 0.5)) / (4 * numpy.sqrt(1 / 12 / N))
    return ks / ks_limit(N), float(mean)


def check_simplex(X):
    """Uniform on the standard simplex {x >= 0, sum x <= 1} in n dimensions: sum x has CDF s^n, each coordinate is Beta(1, n)."""
    X = numpy.asarray(X, dtype=float)
    N, n = X.shape
    ks_sum = ks_cdf(X.sum(axis=1), lambda s: numpy.clip(s, 0, 1) ** n)
    ks_coord = max(ks_cdf(X[:, j], lambda v: 1 - (1 - numpy.clip(v, 0, 1)) ** n) for j in range(n))
    return max(ks_sum, ks_coord) / ks_limit(N)


def hexagon():
    """The regular hexagon of circumradius 1 centred at 0: (A [6, 2], b [6])."""
    ang = numpy.pi / 3 * numpy.arange(6) + numpy.pi / 6
    A = numpy.stack([numpy.cos(ang), numpy.sin(ang)], axis=1)
    return A, numpy.full(6, numpy.sqrt(3) / 2)


def hexagon_cells(X):
    """Cell of every point of the hexagon: 6 sectors (between the vertices) x 2 rings (inside / outside the hexagon scaled by
    1/sqrt(2)); the 12 cells have equal areas."""
    X = numpy.asarray(X, dtype=float)
    A, b = hexagon()
    sector = numpy.floor(numpy.mod(numpy.arctan2(X[:, 1], X[:, 0]), 2 * numpy.pi) / (numpy.pi / 3)).astype(int) % 6
    level = numpy.max(X @ A.T / b, axis=1)          # the hexagonal "radius": 1 on the boundary
    ring = (level > 1 / numpy.sqrt(2)).astype(int)
    return sector * 2 + ring


def chi2_cells(cells, n_cells, alpha=1e-4):
    """(chi2 statistic of equal-area cell counts, the 1 - alpha quantile of chi2 with n_cells - 1 degrees of freedom)."""
    counts = numpy.bincount(cells, minlength=n_cells)
    e = len(cells) / n_cells
    return float(((counts - e) ** 2 / e).sum()), float(scipy.stats.chi2.ppf(1 - alpha, n_cells - 1))


def rotation(n, seed):
    """A random orthogonal n x n matrix (QR of a Gaussian matrix, signs fixed)."""
    rng = numpy.random.default_rng(seed)
    Q, R = numpy.linalg.qr(rng.standard_normal((n, n)))
    return Q * numpy.sign(numpy.diag(R))


def box(lo, hi):
    """{x : lo <= x <= hi} as (A, b)."""
    lo, hi = numpy.asarray(lo, dtype=float), numpy.asarray(hi, dtype=float)
    n = len(lo)
    return numpy.vstack([numpy.eye(n), -numpy.eye(n)]), numpy.concatenate([hi, -lo])


def simplex(n):
    """The standard simplex {x >= 0, sum x <= 1} as (A, b)."""
    return numpy.vstack([-numpy.eye(n), numpy.ones((1, n))]), numpy.concatenate([numpy.zeros(n), [1.0]])
