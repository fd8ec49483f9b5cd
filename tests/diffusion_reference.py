# -*- coding: utf-8 -*-
"""NumPy float64 restatement of cluster.diffusion_graph / graph_components / diffusion_map / diffusion_pseudotime in the stated
order: the dense transition matrix from (indices, sq_distances), connected components, Lanczos with classical
Gram-Schmidt applied twice from a given start vector, and diffusion pseudotime.  Test infrastructure only."""
import numpy as np


def neighbour_sets(indices):
    """N(i): the entries of row i inside [0, n) other than i, in the row's order, and their positions; a repeat is refused."""
    idx = np.asarray(indices)
    n = idx.shape[0]
    out = []
    for i in range(n):
        at = np.flatnonzero((idx[i] >= 0) & (idx[i] < n) & (idx[i] != i))
        v = idx[i, at].astype(np.int64)
        if np.unique(v).size != v.size:
            raise ValueError('a row of indices holds a neighbour twice')
        out.append((v, at))
    return out


def local_scale(indices, sq_distances):
    """sigma_i^2: np.median of the valid squared distances of row i in float64, a zero median replaced by the row's smallest
    positive valid value; ValueError with their number for rows without one."""
    d = np.asarray(sq_distances)
    N = neighbour_sets(indices)
    s2 = np.full(len(N), np.inf)
    for i, (v, at) in enumerate(N):
        x = d[i, at].astype(np.float64)
        if x.size and np.median(x) > 0:
            s2[i] = np.median(x)
        elif (x > 0).any():
            s2[i] = x[x > 0].min()
    if not np.isfinite(s2).all():
        raise ValueError('%d rows hold no positive valid squared distance' % int((~np.isfinite(s2)).sum()))
    return s2


def dense_transition(indices, sq_distances):
    """(T, z, pattern): the dense symmetric transition matrix, z = K 1, and the boolean pattern."""
    d = np.asarray(sq_distances)
    n = d.shape[0]
    N = neighbour_sets(indices)
    s2 = local_scale(indices, sq_distances)
    stored = np.full((n, n), np.nan)                               # stored[i, j]: the value row i holds for j
    for i, (v, at) in enumerate(N):
        stored[i, v] = d[i, at].astype(np.float64)
    has = ~np.isnan(stored)
    P = has | has.T
    I, J = np.nonzero(P)
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    d2 = np.where(has[lo, hi], stored[lo, hi], stored[hi, lo])
    s = np.sqrt(s2)
    den = s2[I] + s2[J]
    W = np.zeros((n, n))
    W[I, J] = np.sqrt(2 * s[I] * s[J] / den) * np.exp(-d2 / den)
    q = W.sum(1)
    K = np.zeros((n, n))
    K[I, J] = W[I, J] / (q[I] * q[J])
    z = K.sum(1)
    T = np.zeros((n, n))
    T[I, J] = K[I, J] / np.sqrt(z[I] * z[J])
    return T, z, P


def csr_of(T, P):
    """(crow int64, col int32, val float64) of the dense T on the pattern P."""
    n = T.shape[0]
    I, J = np.nonzero(P)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(I, minlength=n), out=crow[1:])
    return crow, J.astype(np.int32), T[I, J].astype(np.float64)


def components(P):
    """Labels of the connected components of the boolean pattern P, numbered by their smallest member."""
    n = P.shape[0]
    lab = np.full(n, -1, dtype=np.int64)
    c = 0
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = c
        stack = [s]
        while stack:
            u = stack.pop()
            for v in np.flatnonzero(P[u]):
                if lab[v] < 0:
                    lab[v] = c
                    stack.append(int(v))
        c += 1
    return lab


def cgs2(Q, w, passes=2):
    """Classical Gram-Schmidt of w against the columns of Q, `passes` times: (w_out, h, beta2)."""
    w = np.array(w, dtype=np.float64)
    h = np.zeros(Q.shape[1])
    for _ in range(passes):
        c = Q.T @ w
        w = w - Q @ c
        h += c
    return w, h, float(w @ w)


def sign_rule(psi):
    """Each column with its entry of largest magnitude positive (the smallest index on ties)."""
    psi = np.array(psi)
    for l in range(psi.shape[1]):
        if psi[np.argmax(np.abs(psi[:, l])), l] < 0:
            psi[:, l] = -psi[:, l]
    return psi


def lanczos(T, start, n_comps=15, tol=1e-8, max_steps=None, check_every=10):
    """Lanczos on the dense T with full reorthogonalisation (CGS2), no restarts, as cluster.diffusion_map states it."""
    n = T.shape[0]
    max_steps = min(n, 1000) if max_steps is None else min(int(max_steps), n)
    Q = np.zeros((n, max_steps + 1))
    Q[:, 0] = start / np.sqrt(start @ start)
    alpha, beta = np.zeros(max_steps), np.zeros(max_steps)
    for s in range(max_steps):
        w, h, b2 = cgs2(Q[:, :s + 1], T @ Q[:, s])
        alpha[s], beta[s] = h[s], np.sqrt(b2)
        Q[:, s + 1] = w / beta[s]
        if (s + 1) % check_every and s + 1 < max_steps or s + 1 < n_comps:
            continue
        Tm = np.diag(alpha[:s + 1]) + np.diag(beta[:s], 1) + np.diag(beta[:s], -1)
        theta, S = np.linalg.eigh(Tm)
        top = np.argsort(-theta, kind='stable')[:n_comps]
        res = np.abs(beta[s] * S[-1, top])
        if (res <= tol).all() or s + 1 == max_steps:
            return {'eigenvalues': theta[top], 'components': sign_rule(Q[:, :s + 1] @ S[:, top]), 'residuals': res, 'steps': s + 1,
                    'converged': bool((res <= tol).all())}


def eigh_top(T, m):
    """The m largest eigenpairs of T by numpy.linalg.eigh, descending, under the sign rule, and the whole descending spectrum."""
    lam, V = np.linalg.eigh(T)
    order = np.argsort(-lam, kind='stable')
    return lam[order[:m]], sign_rule(V[:, order[:m]]), lam[order]


def dpt(eigenvalues, components, root):
    lam = np.asarray(eigenvalues, dtype=np.float64)
    psi = np.asarray(components, dtype=np.float64)
    acc = np.zeros(psi.shape[0])
    for l in range(1, lam.size):
        if not lam[l] < 1.0:
            continue
        wl = lam[l] / (1.0 - lam[l])
        d = psi[:, l] - psi[root, l]
        acc = acc + (d * d) * (wl * wl)
    out = np.sqrt(acc)
    return out, (out / out.max() if out.max() > 0 else out.copy())


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a, kind='stable')), np.argsort(np.argsort(b, kind='stable'))
    return float(np.corrcoef(ra, rb)[0, 1])
