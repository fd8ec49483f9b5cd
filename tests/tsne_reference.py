# -*- coding: utf-8 -*-
"""Float64 restatement in NumPy of the exact t-SNE layout (oriana_amd/cluster.py: tsne; csrc/tsne.hip), the seeded
cases and the bounds the device results are held to.  Everything dense: the cases have a few hundred rows.

THE BOUNDS, with u = 2^-24 (float32 unit roundoff); all are derived from the arithmetic the header fixes, none is measured.

The repulsive pair, in float32: dx = fl(qx - yx), dy likewise (u each); s = fma(dy, dy, fma(dx, dx, 1)): the squares carry 2u on
their share of s and each fma rounds once, all terms positive, so s is within 4u; w = v_rcp_f32(s), 1 ulp = 2u: w within 6u.
Every w is added in float64: n 2^-53.  w2 = fl(w w): 13u; the force term w2 dx (the product is exact inside the fma that adds
it): 14u.  The force terms of one 8-candidate step are added in float32, at most 8 roundings: 8u of the sum of the absolute
terms; everything beyond is float64: n 2^-53.  One more u covers all second-order terms ((1 + u)^22 - 1 - 22u < 300 u^2).
Hence, componentwise,
    |zrow - ref| <= EPS_Z(n) zrow_ref,           EPS_Z(n) = 7u + n 2^-53      (the issue's ceiling: 16u + n 2^-53)
    |rep - ref|  <= EPS_R(n) sum_j w^2 |q - y_j|, EPS_R(n) = 23u + n 2^-53     (the issue's ceiling: 32u + n 2^-53)
and a bit-identical pair contributes w = 1 and a force of 0 exactly.  No float32 term of the cases is near the underflow
(min_force_term() is checked on the host against MIN_TERM).

The attractive term is float64 throughout: per entry the two differences (exact or one rounding), D (two fma), the division and
the fma into the sum: at most 6 roundings, and at most n more for the sum of a row: EPS_A(n) = (8 + n) 2^-53 of sum_j P w |y_i -
y_j|.  klrow: log P and log D are within 1 ulp (2 2^-53 relative each), their sum and the fma round twice, and D's own 3 2^-53
moves log D by that much ABSOLUTELY (log D may be tiny): |klrow - ref| <= sum_j P_ij [ (8 + n) 2^-53 (|log P_ij| + log D_ij) +
4 2^-53 ].

kl = sum klrow + log Z sum P with Z = sum zrow - n: the n self pairs are exactly 1 and are added in float64, so the 7u of the
pairs apply to Z itself, while the float64 sums (inside a row, then over the rows) err by 2 n 2^-53 of Z + n: Z is within
EPS_PAIR + 2 n 2^-53 (Z + n) / Z relatively and log Z within that absolutely (to first order; 1.001 covers the rest); the other
float64 sums add n 2^-53 of their absolute terms and the logarithm 2^-52 |log Z|.  kl_bound() returns the total; the cases keep
it below the issue's ceiling of 32u (checked on the host).

The gradient 4 (e attr - rep / Z): the two bounds above, rep's own share of Z's error, and 8 2^-53 of the absolute terms for the
float64 torch arithmetic of the driver.

Affinities: every row's entropy within 1e-5 of log(perplexity) (scikit-learn's tolerance); and, since dH/dbeta = -beta Var_p(d),
a search that stops at |H - log perplexity| <= 1e-9 leaves beta within 1e-9 / (beta Var d), which moves log p_j by that times
|d_j - E d|: |p - p_ref| <= (u + |d_j - E d| 1e-9 / (beta Var d)) p_ref + 2^-149, the conditioning taken from the reference.
The cases keep that factor below 1e-3 (checked on the host)."""
import numpy as np

U = 2.0 ** -24
MIN_TERM = 2.0 ** -100


EPS_PAIR = 7 * U


def EPS_Z(n):
    return EPS_PAIR + n * 2.0 ** -53


def EPS_R(n):
    return 23 * U + n * 2.0 ** -53


def EPS_A(n):
    return (8 + n) * 2.0 ** -53


assert EPS_Z(0) <= 16 * U and EPS_R(0) <= 32 * U


# ---- the seeded cases -----------------------------------------------------------------------------------------------------------
def blobs(seed=3, n=300, d=8, n_blobs=5):
    """Unit-scale Gaussian blobs, float32."""
    rng = np.random.default_rng(seed)
    mu = rng.normal(0.0, 3.0, size=(n_blobs, d))
    which = rng.integers(0, n_blobs, size=n)
    return (mu[which] + rng.normal(size=(n, d))).astype(np.float32), which


def graph(Y, k):
    """The exact k nearest OTHER rows under (distance, index): indices (n, k) int32, squared distances float32, padded with
    -1 / +inf where fewer exist.  float64 distances of the float32 rows, rounded once."""
    Y = np.asarray(Y, dtype=np.float64)
    n = Y.shape[0]
    D = ((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1).astype(np.float32)
    np.fill_diagonal(D, np.inf)
    order = np.lexsort((np.broadcast_to(np.arange(n), (n, n)), D), axis=1)[:, :k]
    idx = np.full((n, k), -1, dtype=np.int32)
    d2 = np.full((n, k), np.inf, dtype=np.float32)
    m = min(k, n - 1)
    idx[:, :m] = order[:, :m]
    d2[:, :m] = np.take_along_axis(D, order[:, :m], 1)
    return idx, d2


AFFINITY_CASES = ((5, 2.0), (30, 10.0), (67, 20.0))          # (k, perplexity) on blobs()


def layout(seed, n, scale):
    """A seeded (n, 2) float32 layout: N(0, scale^2)."""
    return (np.random.default_rng(seed).normal(size=(n, 2)) * scale).astype(np.float32)


# ---- affinities -----------------------------------------------------------------------------------------------------------------
def _entropy(beta, e):
    w = np.exp(-beta * e)
    S = w.sum()
    return np.log(S) + beta * (e * w).sum() / S


def affinities(d2, perplexity, tol=1e-14):
    """Per row of d2 (n, k) float32 (ascending, +inf padding): p (n, k) float64 over the finite entries with entropy
    log(perplexity), by bisection on beta to |H - log perplexity| <= tol (or until the bracket no longer shrinks); beta (n);
    and cond (n, k) = |d_j - E d| / (beta Var d), the sensitivity of log p_j to a unit error of H.  A row whose finite entries
    are all equal: uniform, beta = 1, cond = 0."""
    d2 = np.asarray(d2)
    n, k = d2.shape
    target = np.log(float(perplexity))
    p = np.zeros((n, k))
    beta = np.ones(n)
    cond = np.zeros((n, k))
    for i in range(n):
        m = int(np.isfinite(d2[i]).sum())
        if m == 0:
            continue
        e = d2[i, :m].astype(np.float64) - float(d2[i, 0])
        if e[-1] == 0.0:
            p[i, :m] = 1.0 / m
            continue
        lo, hi = 0.0, 1.0
        while _entropy(hi, e) > target and hi < 1e300:
            lo, hi = hi, hi * 2.0
        b = 0.5 * (lo + hi)
        for _ in range(400):
            b = 0.5 * (lo + hi)
            h = _entropy(b, e)
            if abs(h - target) <= tol or not lo < b < hi:
                break
            if h > target:
                lo = b
            else:
                hi = b
        w = np.exp(-b * e)
        p[i, :m] = w / w.sum()
        beta[i] = b
        mean = (p[i, :m] * e).sum()
        var = (p[i, :m] * (e - mean) ** 2).sum()
        cond[i, :m] = np.abs(e - mean) / (b * var)
    return p, beta, cond


def entropy_of(p):
    """-sum p log p per row of p (float32 or float64), in float64, zeros skipped."""
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(p > 0, p * np.log(p), 0.0)
    return -t.sum(1)


def check_affinities(d2, perplexity, p, beta, what=''):
    """Device p (n, k) float32 and beta (n) float64 against the reference; all-equal rows are held to the uniform distribution
    and a finite beta instead of the entropy.  Returns the largest conditioning factor."""
    d2, p, beta = np.asarray(d2), np.asarray(p), np.asarray(beta)
    ref, _, cond = affinities(d2, perplexity)
    finite = np.isfinite(d2)
    assert p.dtype == np.float32 and beta.dtype == np.float64 and np.all(np.isfinite(beta)) and np.all(beta > 0), what
    assert np.all(p[~finite] == 0.0), what
    m = finite.sum(1)
    flat = np.array([m[i] > 0 and d2[i, m[i] - 1] == d2[i, 0] for i in range(len(m))])
    for i in np.nonzero(flat)[0]:
        assert np.all(p[i, :m[i]] == np.float32(1.0 / m[i])), (what, i)
    rows = ~flat & (m > 0)
    H = entropy_of(p)
    print('%s: max |H - log perplexity| = %.3g; max |p - ref| / bound = %.3g; conditioning %.3g' % (
        what, np.abs(H[rows] - np.log(perplexity)).max(),
        (np.abs(p - ref) / ((U + cond * 1e-9) * ref + 2.0 ** -149))[rows].max(), cond.max() * 1e-9))
    assert np.all(np.abs(H[rows] - np.log(perplexity)) <= 1e-5), what
    assert np.all(np.abs(p - ref)[rows] <= ((U + cond * 1e-9) * ref + 2.0 ** -149)[rows]), what
    return cond.max() * 1e-9


# ---- the joint P ----------------------------------------------------------------------------------------------------------------
def joint(idx, p):
    """P = (p_{j|i} + p_{i|j}) / (2 n), dense (n, n) float64 rounded to float32 values (as stored), from idx (n, k) and p (n, k)
    (float32 values are taken as they are); padded slots and zeros dropped."""
    idx, p = np.asarray(idx), np.asarray(p, dtype=np.float64)
    n = idx.shape[0]
    C = np.zeros((n, n))
    for i in range(n):
        keep = (idx[i] >= 0) & (p[i] > 0)
        C[i, idx[i][keep]] = p[i][keep]
    return ((C + C.T) / (2.0 * n)).astype(np.float32).astype(np.float64)


def csr_of(P):
    """(crow int64, col int32, val float32) of a dense P: its non-zeros, columns ascending."""
    r, c = np.nonzero(P)
    crow = np.zeros(P.shape[0] + 1, dtype=np.int64)
    crow[1:] = np.cumsum(np.bincount(r, minlength=P.shape[0]))
    return crow, c.astype(np.int32), P[r, c].astype(np.float32)


def dense_of(crow, col, val, n):
    P = np.zeros((n, n))
    crow = np.asarray(crow)
    rows = np.repeat(np.arange(n), np.diff(crow))
    P[rows, np.asarray(col)] = np.asarray(val, dtype=np.float64)
    return P


# ---- the gradient ---------------------------------------------------------------------------------------------------------------
def pair_sums(Q, Y):
    """rep (nq, 2), zrow (nq), and the absolute sums abs_rep (nq, 2) = sum_j w^2 |q - y_j| of float32 points, in float64."""
    Q, Y = np.asarray(Q, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    diff = Q[:, None, :] - Y[None, :, :]
    w = 1.0 / (1.0 + (diff ** 2).sum(-1))
    return (w[:, :, None] ** 2 * diff).sum(1), w.sum(1), (w[:, :, None] ** 2 * np.abs(diff)).sum(1)


def min_force_term(Q, Y):
    """The smallest non-zero |w^2 (q - y)| over all pairs and both components."""
    Q, Y = np.asarray(Q, dtype=np.float64), np.asarray(Y, dtype=np.float64)
    diff = Q[:, None, :] - Y[None, :, :]
    t = np.abs(diff) / (1.0 + (diff ** 2).sum(-1))[:, :, None] ** 2
    return t[t > 0].min() if (t > 0).any() else np.inf


def check_repulse(Q, Y, rep, zrow, what='', n_total=None):
    """Device rep / zrow of the queries Q against the candidates Y; n_total: the candidates of all accumulated calls."""
    rep, zrow = np.asarray(rep), np.asarray(zrow)
    n = Y.shape[0] if n_total is None else n_total
    r, z, ra = pair_sums(Q, Y)
    assert rep.dtype == np.float64 and zrow.dtype == np.float64 and rep.shape == r.shape and zrow.shape == z.shape, what
    with np.errstate(divide='ignore', invalid='ignore'):
        worst_r = np.nanmax(np.where(ra > 0, np.abs(rep - r) / (EPS_R(n) * ra), 0.0)) if r.size else 0.0
        worst_z = np.nanmax(np.abs(zrow - z) / (EPS_Z(n) * z)) if z.size and n else 0.0
    print('%s: |rep - ref| / bound <= %.3g, |zrow - ref| / bound <= %.3g' % (what, worst_r, worst_z))
    assert np.all(np.abs(rep - r) <= EPS_R(n) * ra), what
    assert np.all(np.abs(zrow - z) <= EPS_Z(n) * z), what


def attract(P, Y):
    """attr (n, 2), klrow (n) and their absolute sums (abs_attr (n, 2), abs_kl (n), psum (n)) for a dense P."""
    Y = np.asarray(Y, dtype=np.float64)
    diff = Y[:, None, :] - Y[None, :, :]
    D = 1.0 + (diff ** 2).sum(-1)
    with np.errstate(divide='ignore', invalid='ignore'):
        logP = np.where(P > 0, np.log(P), 0.0)
    pw = P / D
    attr = (pw[:, :, None] * diff).sum(1)
    klrow = (P * (logP + np.log(D))).sum(1)
    return attr, klrow, (pw[:, :, None] * np.abs(diff)).sum(1), (P * (np.abs(logP) + np.log(D))).sum(1), P.sum(1)


def attract_bounds(P, Y):
    n = P.shape[0]
    _, _, abs_attr, abs_kl, psum = attract(P, Y)
    return EPS_A(n) * abs_attr, EPS_A(n) * abs_kl + 4 * 2.0 ** -53 * psum


def check_attract(P, Y, attr, klrow, what=''):
    a, kl, _, _, _ = attract(P, Y)
    ba, bk = attract_bounds(P, Y)
    attr, klrow = np.asarray(attr), np.asarray(klrow)
    with np.errstate(divide='ignore', invalid='ignore'):
        print('%s: |attr - ref| / bound <= %.3g, |klrow - ref| / bound <= %.3g' % (
            what, np.nanmax(np.where(ba > 0, np.abs(attr - a) / ba, 0.0)), np.nanmax(np.where(bk > 0, np.abs(klrow - kl) / bk, 0.0))))
    assert np.all(np.abs(attr - a) <= ba) and np.all(np.abs(klrow - kl) <= bk), what


def gradient(P, Y, exaggeration=1.0):
    """grad (n, 2) = 4 (exaggeration attr - rep / Z), kl = sum klrow + log Z sum P, Z = sum zrow - n."""
    n = P.shape[0]
    attr, klrow, _, _, _ = attract(P, Y)
    rep, zrow, _ = pair_sums(Y, Y)
    Z = zrow.sum() - n
    return 4.0 * (exaggeration * attr - rep / Z), klrow.sum() + np.log(Z) * P.sum()


def kl_bound(P, Y):
    """The absolute bound of the device kl against gradient()'s (module docstring)."""
    n = P.shape[0]
    _, klrow, _, abs_kl, psum = attract(P, Y)
    _, bk = attract_bounds(P, Y)
    _, zrow, _ = pair_sums(Y, Y)
    Z = zrow.sum() - n
    eps_Z = 1.001 * (EPS_PAIR + 2 * n * 2.0 ** -53 * (Z + n) / Z)
    return bk.sum() + n * 2.0 ** -53 * abs_kl.sum() + (eps_Z + 2.0 ** -52 * abs(np.log(Z))) * psum.sum() + 4 * 2.0 ** -53 * abs(np.log(Z))


def gradient_bound(P, Y, exaggeration=1.0):
    n = P.shape[0]
    _, _, abs_attr, _, _ = attract(P, Y)
    ba, _ = attract_bounds(P, Y)
    _, zrow, abs_rep = pair_sums(Y, Y)
    Z = zrow.sum() - n
    eps_Z = 1.001 * (EPS_PAIR + 2 * n * 2.0 ** -53 * (Z + n) / Z)
    return 4.0 * (exaggeration * ba + (EPS_R(n) + 1.001 * eps_Z) * abs_rep / Z + 8 * 2.0 ** -53 * (exaggeration * abs_attr + abs_rep / Z))


# ---- the start and the optimiser -------------------------------------------------------------------------------------------------
def pca_init(X):
    """The rows of X on the top two principal axes of the covariance (numpy.linalg.eigh, float64), every axis signed so that its
    largest-magnitude loading is positive, rescaled so that the first coordinate has standard deviation 1e-4."""
    X = np.asarray(X, dtype=np.float64)
    Xc = X - X.mean(0)
    _, vec = np.linalg.eigh(Xc.T @ Xc / (X.shape[0] - 1))
    axes = vec[:, -2:][:, ::-1].copy()
    for a in range(2):
        if axes[np.abs(axes[:, a]).argmax(), a] < 0:
            axes[:, a] = -axes[:, a]
    out = Xc @ axes
    return out / out[:, 0].std() * 1e-4


def step(y, update, gains, grad, momentum, lr):
    """One step of scikit-learn's _gradient_descent; returns the new (y, update, gains)."""
    inc = update * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), 0.01)
    update = momentum * update - lr * (gains * grad)
    return y + update, update, gains


def optimise(P, y0, n_iter, exaggeration_iter, early_exaggeration=12.0, learning_rate='auto'):
    """The optimiser of cluster.tsne on a float64 master copy whose float32 cast the gradient reads."""
    n = P.shape[0]
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == 'auto' else float(learning_rate)
    y = np.array(y0, dtype=np.float64)
    for steps, ex, mom in ((exaggeration_iter, early_exaggeration, 0.5), (n_iter - exaggeration_iter, 1.0, 0.8)):
        update, gains = np.zeros_like(y), np.ones_like(y)
        for _ in range(steps):
            grad, _ = gradient(P, y.astype(np.float32), ex)
            y, update, gains = step(y, update, gains, grad, mom, lr)
    return y
