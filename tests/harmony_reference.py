# -*- coding: utf-8 -*-
"""Float64 NumPy restatement of the Harmony batch correction of oriana_amd/cluster.py, the seeded inputs of
its tests and the bounds the tests hold the kernels to.  Every bound comes from the arithmetic (u = 2^-24 is the unit roundoff of
float32; first-order terms carry a factor SLACK = 1.01 for what is of second order), none was measured on the code under test, and
no row is excused.

THE PAIR (oriana_harmony_assign; per row, batch b, c = float32(-log2(e) / sigma))
  dot       |dot' - dot| <= (d + 1) u A_k,  A_k = sum_f |z_f y_kf|: what a chain of d fused multiply-adds keeps.  The kernel's chain
            is compensated (every product's and every addition's rounding is carried along in float32 and added at the end:
            u |dot| + (d u)^2 A_k by Ogita, Rump and Oishi's bound), which is inside it with room.
  dist      one more fused multiply-add:        |dist' - dist| <= ed_k = 2 (d + 1) u A_k + u (|dist_k| + 2 (d + 1) u A_k).
  min       the minimum is 1-Lipschitz:         |m' - m| <= em = max_k ed_k.
  exponent  a' = fl(dist' - m'), t' = fl(a' c') with c' = c (1 + u):  in natural units x = (dist - m) / sigma,
            |x' - x| <= eta_k = (ed_k + em + u a_k) / sigma + 2 u |x_k|.
  exp       the HARDWARE exponential v_exp_f32 (chosen over expf by reading the generated code: 2 instructions against 12; its
            argument is the rounded product, which expf's extended-precision reduction would avoid -- that is the 2 u |x_k| above),
            1 ulp = 2 u relative; a result below 2^-126 is flushed to 0: an absolute 2^-126.
  e_k       times P (one rounding, and a subnormal product loses at most 2^-149):
            |e' - e| <= rho_k e_k + phi_k,  rho_k = expm1(eta_k) (1 + 2 u) + 3 u,  phi_k = 2^-126 P_kb + 2^-149.
  sum       K - 1 additions ascending:  |s' - s| <= sum_k (rho_k e_k + phi_k) + (K - 1) u s.
  R         the correctly rounded reciprocal and one product:
            |R' - R| <= R (rho_k + rho_s + 2 u) + phi_k / s,  rho_s = |s' - s| / s.
The float64 sums (their products are exact, N summands lose at most N 2^-53 of the absolute terms each):
  O_blk     sum_i dR_ik + n 2^-53 sum_i R_ik.
  R dist    sum (dR |dist| + (R + dR) ed) + n K 2^-53 sum R |dist|.
  R log R   f(R) = R log R is convex with its minimum at 1 / e: over [R - dR, R + dR] it moves by at most the larger of its
            moves to the ends and, where 1 / e lies inside, to 1 / e; plus logf's 3 ulp = 6 u of |f|; plus n K 2^-53 sum |f|.
oriana_harmony_moments   T float32 fused multiply-adds before a promotion (T = oriana_harmony_partial_rows(); the first rounds the
  product, the other T - 1 the additions), then float64:  per element  T u sum |r x| + n 2^-52 sum |r x|.
oriana_harmony_correct   K fused multiply-adds and the subtraction:  |zc' - zc| <= K u sum_k |R W| + u |zc|; the norm's chain,
  the root and the quotient are (d / 2 + 2) u <= (d + 2) u relative on top of what the row's own error moves:
  |zcos' - zcos|_f <= (|dzc_f| + |zcos_f| ||dzc||) / ||zc|| + (d + 2) u |zcos_f|.

END TO END (test_harmony_gpu.py, the fixed-rounds case E2E below): the tolerance is measured on the restatement alone -- the
distance of a run whose state is rounded to float32 wherever the device stores float32 (R, centres, Zcos, P, W, the corrected
rows) from the pure float64 run, times E2E_FACTOR.  Measured on the CPU (max |difference|): corrected 5.9e-07 (of entries up to
13), responsibilities 1.6e-07, objective_rounds 2.2e-05 (of values up to 271); the test recomputes them at run time and the host
test holds the record below to within a factor of two of them."""
import math

import numpy as np

U = 2.0 ** -24
SLACK = 1.01
E2E_FACTOR = 4.0
E2E_MEASURED = {'corrected': 5.9e-07, 'responsibilities': 1.6e-07, 'objective_rounds': 2.2e-05}
E2E = dict(K=12, max_iter=3, max_rounds=6, seed=0)              # on blobs(), centres start_centers(Z, 12)
# The stopping-rule case: blobs(seed=0), K = 6 from start_centers(), both thresholds at 0.1.  The derived bound of a round's
# objective is a worst case (every rounding of every pair aligned): about 4e-4 of the objective here, so only decisions with a
# margin above 0.04 can be asserted on the device, and the default thresholds (1e-5, 1e-4) cannot.  In this case every decision of
# the restatement -- five rounds' and five iterations', four of which continue -- has a margin of more than 100 times the derived
# error of its ratio (121 times at the least; test_harmony_host.py asserts it).
STOP = dict(blob_seed=0, K=6, max_iter=10, max_rounds=20, eps_cluster=0.1, eps_harmony=0.1, seed=0)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
def blobs(n=1200, d=8, types=4, batches=3, seed=2, drop=None):
    """Seeded blobs: cell types 4 apart, batch offsets of the size of the type separation, unit noise; float32 rows, int64 type and
    batch of every row.  drop = (type, batch): that type is absent from that batch."""
    rng = np.random.RandomState(seed)
    cell = rng.randint(0, types, size=n)
    batch = rng.randint(0, batches, size=n)
    mu = rng.normal(size=(types, d)) * 4.0
    off = rng.normal(size=(batches, d)) * 4.0
    Z = mu[cell] + off[batch] + rng.normal(size=(n, d))
    if drop is not None:
        keep = ~((cell == drop[0]) & (batch == drop[1]))
        Z, cell, batch = Z[keep], cell[keep], batch[keep]
    return Z.astype(np.float32), cell.astype(np.int64), batch.astype(np.int64)


def start_centers(Z, K, seed=0):
    """K seeded distinct rows of the normalised Z, as explicit start centres."""
    rng = np.random.RandomState(seed + 1000)
    idx = rng.choice(Z.shape[0], size=K, replace=False)
    return normalize_rows(np.asarray(Z, dtype=np.float64))[idx]


def kmeans_start(Z, K, seed=0, iters=25):
    """Start centres for the mixing tests: seeded k-means++ and `iters` Lloyd steps on the normalised rows, float64 NumPy."""
    X = normalize_rows(np.asarray(Z, dtype=np.float64))
    rng = np.random.RandomState(seed)
    c = [X[rng.randint(len(X))]]
    for _ in range(1, K):
        d2 = np.min([((X - ci) ** 2).sum(1) for ci in c], axis=0)
        c.append(X[min(np.searchsorted(np.cumsum(d2), rng.rand() * d2.sum()), len(X) - 1)])
    c = np.array(c)
    for _ in range(iters):
        lab = ((X[:, None, :] - c[None]) ** 2).sum(2).argmin(1)
        for k in range(K):
            if (lab == k).any():
                c[k] = X[lab == k].mean(0)
    return c


def knn_shares(X, labels, k=15):
    """For every row the share of its k nearest other rows that carry its own label, averaged."""
    X = np.asarray(X, dtype=np.float64)
    sq = (X * X).sum(1)
    D = sq[:, None] + sq[None, :] - 2.0 * X @ X.T
    np.fill_diagonal(D, np.inf)
    nn = np.argpartition(D, k, axis=1)[:, :k]
    return float((labels[nn] == labels[:, None]).mean())


# ---- the definition ------------------------------------------------------------------------------------------------------------
def default_clusters(n):
    return max(1, min(int(math.floor(n / 30.0 + 0.5)), 100))


def block_cuts(n, n_blocks=20):
    nb = min(n_blocks, n)
    return [(j * n) // nb for j in range(nb + 1)]


def permutation(n, seed):
    import torch
    g = torch.Generator()
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g).numpy()


def normalize_rows(Z):
    Z = np.asarray(Z, dtype=np.float64)
    nr = np.sqrt((Z * Z).sum(1, keepdims=True))
    return np.where(nr > 0, Z / np.where(nr > 0, nr, 1.0), 0.0)


def pair(Zcos, batch, centers, P, inv_sigma):
    """dist (n, K) and R (n, K), float64."""
    Zc, Y, P = (np.asarray(a, dtype=np.float64) for a in (Zcos, centers, P))
    dist = 2.0 * (1.0 - Zc @ Y.T)
    m = dist.min(1, keepdims=True)
    e = np.exp(-(dist - m) * inv_sigma) * P[:, batch].T
    return dist, e / e.sum(1, keepdims=True)


def xlogx(R):
    return np.where(R > 0, R * np.log(np.where(R > 0, R, 1.0)), 0.0)


def batch_sums(R, batch, B):
    """O (K, B) = sum_{i in b} R_ik."""
    O = np.zeros((R.shape[1], B))
    for b in range(B):
        O[:, b] = R[batch == b].sum(0)
    return O


def assign(Zcos, batch, centers, P, inv_sigma):
    """R, dist, O_blk (K, B), sum R dist, sum R log R of the rows given."""
    P = np.asarray(P, dtype=np.float64)
    dist, R = pair(Zcos, batch, centers, P, inv_sigma)
    return R, dist, batch_sums(R, batch, P.shape[1]), float((R * dist).sum()), float(xlogx(R).sum())


def moments(X, R, batch, B):
    """S (K, B, d), O (K, B) and the sums of absolute terms SA (K, B, d)."""
    X, R = np.asarray(X, dtype=np.float64), np.asarray(R, dtype=np.float64)
    K, d = R.shape[1], X.shape[1]
    S, SA = np.zeros((K, B, d)), np.zeros((K, B, d))
    for b in range(B):
        sel = batch == b
        S[:, b] = R[sel].T @ X[sel]
        SA[:, b] = np.abs(R[sel]).T @ np.abs(X[sel])
    return S, batch_sums(R, batch, B), SA


def ridge_weights(S, O, lam):
    """The closed form (cluster.harmony_ridge_weights), float64: W (K, B, d) and the intercepts w0 (K, d)."""
    lam = np.broadcast_to(np.asarray(lam, dtype=np.float64), (O.shape[1],))
    den = O + lam[None, :]
    g = lam[None, :] / den
    num = (g[:, :, None] * S).sum(1)
    c = (g * O).sum(1)
    ok = c > 0
    w0 = num / np.where(ok, c, 1.0)[:, None]
    W = (S - O[:, :, None] * w0[:, None, :]) / den[:, :, None]
    return np.where(ok[:, None, None], W, 0.0), np.where(ok[:, None], w0, 0.0)


def ridge_solve(Z, R_k, batch, lam):
    """harmonypy's system of one cluster, solved: Phi = [1; one-hot(batch)] ((B + 1, n)), (Phi diag(R_k) Phi^T + diag(0, lam)) W =
    Phi diag(R_k) Z.  Returns W ((B + 1, d)): row 0 is the intercept."""
    Z = np.asarray(Z, dtype=np.float64)
    lam = np.asarray(lam, dtype=np.float64)
    B = lam.shape[0]
    Phi = np.zeros((B + 1, Z.shape[0]))
    Phi[0] = 1.0
    Phi[batch + 1, np.arange(Z.shape[0])] = 1.0
    PR = Phi * np.asarray(R_k, dtype=np.float64)[None, :]
    return np.linalg.solve(PR @ Phi.T + np.diag(np.concatenate([[0.0], lam])), PR @ Z)


def correct(Z, R, batch, W):
    Z, R, W = (np.asarray(a, dtype=np.float64) for a in (Z, R, W))
    Zc = Z - np.einsum('ik,ikf->if', R, W[:, batch].transpose(1, 0, 2))
    return Zc, normalize_rows(Zc)


def diversity_term(O, E, theta, sigma):
    """The third term of the objective from O and E alone."""
    return float(sigma * (theta[None, :] * O * np.log((O + 1.0) / (E + 1.0))).sum())


def diversity_term_per_cell(R, batch, O, E, theta, sigma):
    """harmonypy's form: sigma sum_ik R_ik theta_{b_i} log((O + 1) / (E + 1))_{k b_i}."""
    L = theta[None, :] * np.log((O + 1.0) / (E + 1.0))
    return float(sigma * (R * L[:, batch].T).sum())


def objective(rd, re, O, E, theta, sigma):
    return rd + sigma * re + diversity_term(O, E, theta, sigma)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def harmony(Y, batch, n_clusters=None, theta=2.0, sigma=0.1, ridge=1.0, n_blocks=20, max_iter=10, max_rounds=20, eps_cluster=1e-5,
            eps_harmony=1e-4, centers=None, seed=0, store32=False, with_bounds=False):
    """The whole driver in float64 with the device's permutation and block cuts; `centers` is required (the k-means start is the
    device's).  store32: round the state to float32 wherever the device stores float32.  with_bounds: also 'checks', one
    (ratio, eps, ratio error bound) per stopping decision of a round."""
    rnd = f32 if store32 else (lambda a: a)
    Y = np.asarray(Y, dtype=np.float64)
    batch = np.asarray(batch, dtype=np.int64)
    n, d = Y.shape
    B = int(batch.max()) + 1
    K = default_clusters(n) if n_clusters is None else int(n_clusters)
    theta = np.broadcast_to(np.asarray(theta, dtype=np.float64), (B,)).copy()
    lam = np.broadcast_to(np.asarray(ridge, dtype=np.float64), (B,)).copy()
    sizes = np.bincount(batch, minlength=B)
    Pr = sizes / float(n)
    perm = permutation(n, seed)
    Z, bt = Y[perm], batch[perm]
    cuts = block_cuts(n, n_blocks)
    nb = len(cuts) - 1
    inv_sigma = 1.0 / sigma
    Zcos = rnd(normalize_rows(Z))
    cen = rnd(normalize_rows(np.asarray(centers, dtype=np.float64)))
    cen_exact = normalize_rows(np.asarray(centers, dtype=np.float64))
    R = np.zeros((n, K))
    O_blk, rd, re = np.zeros((nb, K, B)), np.zeros(nb), np.zeros(nb)
    brd, bre, bdO = np.zeros(nb), np.zeros(nb), np.zeros((nb, K, B))          # (with_bounds: the bounds of every block's sums)

    def visit(j, P):
        a, b = cuts[j], cuts[j + 1]
        Rj, dist, Oj, sd, se = assign(Zcos[a:b], bt[a:b], cen, P, inv_sigma)
        R[a:b] = rnd(Rj)
        if store32:
            Oj, sd, se = batch_sums(R[a:b], bt[a:b], B), float((R[a:b] * dist).sum()), float(xlogx(R[a:b]).sum())
        O_blk[j], rd[j], re[j] = Oj, sd, se
        if with_bounds:
            bd = assign_bounds(Zcos[a:b], bt[a:b], cen, P, inv_sigma)
            brd[j], bre[j], bdO[j] = bd['rd'], bd['re'], bd['O_blk']

    def objective_bound(O, E):
        """What the kernels' own error moves a round's objective by: the two sums, and the third term through dO and dE = sum_b dO
        Pr (|d/dO| <= sigma theta (|log((O + 1) / (E + 1))| + 1), |d/dE| = sigma theta O / (E + 1))."""
        dO = bdO.sum(0)
        dE = dO.sum(1)[:, None] * Pr[None, :]
        L = np.abs(np.log((O + 1.0) / (E + 1.0))) + 1.0
        return float(brd.sum() + sigma * bre.sum() + SLACK * sigma * (theta[None, :] * (L * dO + O / (E + 1.0) * dE)).sum())

    for j in range(nb):
        visit(j, np.ones((K, B)))
    O = O_blk.sum(0)
    E = O.sum(1)[:, None] * Pr[None, :]
    obj_iter = [objective(rd.sum(), re.sum(), O, E, theta, sigma)]
    obj_rounds, rounds, checks = [], [], []
    converged, n_iter = False, 0
    Zcorr = Z.copy()
    for it in range(max_iter):
        robj, rerr, nr = [], [], 0
        while nr < max_rounds:
            S, _, _ = moments(Zcos, R, bt, B)
            C = S.sum(1)
            cn = np.sqrt((C * C).sum(1, keepdims=True))
            cen_exact = np.where(cn > 0, C / np.where(cn > 0, cn, 1.0), cen_exact)
            cen = rnd(cen_exact)
            for j in range(nb):
                O = O - O_blk[j]
                E = E - O_blk[j].sum(1)[:, None] * Pr[None, :]
                P = rnd(((E + 1.0) / (O + 1.0)) ** theta[None, :])
                visit(j, P)
                O = O + O_blk[j]
                E = E + O_blk[j].sum(1)[:, None] * Pr[None, :]
            robj.append(objective(rd.sum(), re.sum(), O, E, theta, sigma))
            rerr.append(objective_bound(O, E) if with_bounds else 0.0)
            nr += 1
            if eps_cluster is not None and nr >= 5:
                old, new = robj[-4] + robj[-3] + robj[-2], robj[-3] + robj[-2] + robj[-1]
                ratio = (old - new) / abs(old)
                checks.append((ratio, float(eps_cluster), SLACK * (sum(rerr[-4:-1]) + sum(rerr[-3:])) * (1.0 + abs(ratio)) / abs(old)))
                if ratio < eps_cluster:
                    break
        obj_rounds.extend(robj)
        rounds.append(nr)
        obj_iter.append(robj[-1])
        S, Om, _ = moments(Z, R, bt, B)
        W = rnd(ridge_weights(S, Om, lam)[0])
        Zcorr, Zcos = correct(Z, R, bt, W)
        Zcorr, Zcos = rnd(Zcorr), rnd(normalize_rows(Zcorr) if store32 else Zcos)
        n_iter = it + 1
        if eps_harmony is not None:
            r = abs(obj_iter[-2] - obj_iter[-1]) / abs(obj_iter[-2])
            checks.append((r, float(eps_harmony), SLACK * 2.0 * rerr[-1] * (1.0 + r) / abs(obj_iter[-2])))
            if r < eps_harmony:
                converged = True
                break
    corrected, resp = np.empty_like(Zcorr), np.empty_like(R)
    corrected[perm], resp[perm] = Zcorr, R
    out = {'corrected': corrected, 'responsibilities': resp, 'centers': cen, 'objective': obj_iter, 'objective_rounds': obj_rounds,
           'rounds': rounds, 'n_iter': n_iter, 'converged': converged, 'batch_sizes': sizes}
    if with_bounds:
        out['checks'] = checks
    return out


# ---- the bounds ----------------------------------------------------------------------------------------------------------------
def assign_bounds(Zcos, batch, centers, P, inv_sigma):
    """The bounds of THE PAIR at these inputs: 'R' (n, K) per element, 'O_blk' (K, B), 'rd' and 're' (the two sums).  Asserts that
    the exponent's error stays small enough for the first-order treatment (eta <= 0.01)."""
    Zc, Y, P = (np.asarray(a, dtype=np.float64) for a in (Zcos, centers, P))
    n, d = Zc.shape
    K, B = P.shape
    dist, R = pair(Zc, batch, Y, P, inv_sigma)
    A = np.abs(Zc) @ np.abs(Y).T
    ed = 2.0 * (d + 1) * U * A
    ed = ed + U * (np.abs(dist) + ed)
    em = ed.max(1, keepdims=True)
    a = dist - dist.min(1, keepdims=True)
    x = a * inv_sigma
    eta = (ed + em + U * a) * inv_sigma + 2.0 * U * x
    assert eta.max() <= 0.01, eta.max()
    Pb = P[:, batch].T
    e = np.exp(-x) * Pb
    s = e.sum(1, keepdims=True)
    rho = np.expm1(eta) * (1.0 + 2.0 * U) + 3.0 * U
    phi = 2.0 ** -126 * Pb + 2.0 ** -149
    ds = (rho * e + phi).sum(1, keepdims=True) + (K - 1) * U * s
    rho_s = ds / s
    assert rho_s.max() <= 0.01, rho_s.max()
    dR = SLACK * (R * (rho + rho_s + 2.0 * U) + phi / s)
    dO = np.zeros((K, B))
    for b in range(B):
        sel = batch == b
        dO[:, b] = dR[sel].sum(0) + n * 2.0 ** -53 * R[sel].sum(0)
    drd = float((dR * np.abs(dist) + (R + dR) * ed).sum() + n * K * 2.0 ** -53 * (R * np.abs(dist)).sum())
    f = xlogx(R)
    lo, hi = np.maximum(R - dR, 0.0), R + dR
    mv = np.maximum(np.abs(xlogx(lo) - f), np.abs(xlogx(hi) - f))
    inside = (lo < math.exp(-1)) & (hi > math.exp(-1))
    mv = np.where(inside, np.maximum(mv, np.abs(-math.exp(-1) - f)), mv)
    dre = float((mv + 6.0 * U * (np.abs(f) + mv)).sum() + n * K * 2.0 ** -53 * np.abs(f).sum())
    return {'R': dR, 'O_blk': dO, 'rd': drd, 're': dre}


def sums_order_bound(n, K, R, dist):
    """What two values of `blocks` may differ by in the float64 sums: 2 n 2^-53 of the absolute sums (O_blk per element uses its own
    column; the two scalar sums have n K summands)."""
    return 2.0 * n * K * 2.0 ** -53 * float((np.abs(R) * np.abs(dist)).sum()), 2.0 * n * K * 2.0 ** -53 * float(np.abs(xlogx(R)).sum())


def moments_bounds(SA, OA, n, T):
    """Per element of S and of O, from the sums of absolute terms SA (K, B, d) and OA (K, B) = sum |r|."""
    return (T * U * SLACK + n * 2.0 ** -52) * SA, (T * U * SLACK + n * 2.0 ** -52) * OA


def correct_bounds(Z, R, batch, W):
    """Per element of Zcorr and of Zcos."""
    Z, R, W = (np.asarray(a, dtype=np.float64) for a in (Z, R, W))
    K, d = R.shape[1], Z.shape[1]
    Zc, Zcos = correct(Z, R, batch, W)
    RW = np.einsum('ik,ikf->if', np.abs(R), np.abs(W[:, batch]).transpose(1, 0, 2))
    dzc = SLACK * (K * U * RW + U * np.abs(Zc))
    nr = np.sqrt((Zc * Zc).sum(1, keepdims=True))
    dn = np.sqrt((dzc * dzc).sum(1, keepdims=True))
    safe = np.where(nr > 0, nr, 1.0)
    assert (dn[nr > 0] / nr[nr > 0]).max(initial=0.0) <= 1e-3
    dcos = SLACK * (dzc + np.abs(Zcos) * dn) / safe + (d + 2) * U * np.abs(Zcos)
    return dzc, np.where(nr > 0, dcos, np.inf)


def e2e_distances(Z, batch):
    """The end-to-end case: (the float64 run, the run with float32 state, max |difference| of 'corrected', 'responsibilities' and
    'objective_rounds')."""
    kw = dict(n_clusters=E2E['K'], centers=start_centers(Z, E2E['K']), eps_cluster=None, eps_harmony=None, max_iter=E2E['max_iter'],
              max_rounds=E2E['max_rounds'], seed=E2E['seed'])
    a, b = harmony(Z, batch, **kw), harmony(Z, batch, store32=True, **kw)
    return a, b, {k: float(np.abs(np.asarray(a[k]) - np.asarray(b[k])).max()) for k in ('corrected', 'responsibilities', 'objective_rounds')}
