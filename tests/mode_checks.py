"""Step 1's solve resolved per time mode (plain numpy / scipy, TEST INFRASTRUCTURE shared by test_mode_checks_cpu.py and
test_hip_mode_resolved.py).

The nodal figure max|got - want| / max|want| of a solve with a white right-hand side is owned by the low time modes: mode ``a`` of the
solution has amplitude about 1 / (lambda + sigma_a + eps) and sigma_a reaches 4 T^2, so a defect of the high modes vanishes under the
tolerance.  Here the right-hand sides are band-limited in time (one octave of modes, inside which sigma varies by about 4x) and every
mode is compared with an extended-precision solve of its own K + (sigma_a + eps) M:

``basis``        Q[t, a] and sigma_a of geometry.time_modes in np.longdouble (the closed form, NOT an eigensolver's basis);
``octaves``      the bands [0], [1], [2, 3], [4..7], ...;
``band_rhs``     a right-hand side whose modes outside a band are rounding only;
``reference``    per mode a dense fp64 LU refined with the residual in long double: xr[a, v];
``mode_errors``  per-mode errors of a nodal solution against ``reference`` and what leaked out of the band;
``plain_solve``  the same operation in plain fp64 (its error against ``reference`` is the yardstick of the tolerances), with knobs
                 for deliberate defects (``MUTATIONS``);
``kappa``, ``tolerances``, ``assert_modes``  the bound 16 max(p, 2^-53 kappa_a) and the assertion that names mode, chunk and band.

Sign and vertex order follow device.laplacian_solve_many: x = (K + (sigma + eps) M)^-1 b with K = - cotangent Laplacian, [T + 1, V] in
the caller's numbering.  Mode 0 at eps = 0 is singular: right-hand sides are consistent (zero plain sum), the reference fixes the gauge
with + m m^T and the mode is compared after removing its mass-weighted mean."""
import functools

import numpy as np
import scipy.linalg as sla
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "mode_checks needs an extended-precision long double (x87: 64-bit mantissa)"

MARGIN = 16.0
U = 2.0 ** -53
REFINE = 4
MUTATIONS = ("offdiag_high", "stale_shift", "inverse_row", "forward_col", "ground_all")
OLD_TOL = {False: 1e-9, True: 1e-10}       # the nodal tolerance of the existing tests: T + 1 <= 256 / above (test_hip_long_horizon.py)


# ---- long-double products through exact fp64 pieces -----------------------------------------------------------------------------
# numpy multiplies long-double matrices with a scalar loop (seconds at T = 1023).  Both factors are cut into PIECES fixed-point pieces
# of BITS bits (rows of the left factor and columns of the right one scaled by a power of two); a product of two pieces summed over
# k <= 1024 terms is an integer below 2^53, so the fp64 BLAS forms it exactly, and the 16 partial products are added in long double.
# What is cut off lies 84 bits below the largest entry of the row / column.
BITS, PIECES, KMAX = 21, 4, 1024


def _pieces(X, axis):
    X = np.asarray(X, dtype=LD)
    big = np.max(np.abs(X), axis=axis, keepdims=True)
    expo = np.where(big > 0, np.ceil(np.log2(np.where(big > 0, big, LD(1)))), LD(0)).astype(np.float64)
    scale = np.ldexp(np.ones_like(expo), expo.astype(np.int64))                 # powers of two, fp64
    Y = X / scale.astype(LD)
    out = []
    for i in range(1, PIECES + 1):
        step = LD(2.0) ** (BITS * i)
        piece = np.rint(Y * step) / step
        out.append(np.asarray(piece, dtype=np.float64))
        Y = Y - piece
    return out, scale


def ld_matmul(A, B, left=None):
    """A @ B for long-double (or fp64) matrices, as a long-double matrix, with the inner dimension at most ``KMAX``.  ``left``: the
    pieces of A, already cut (``_pieces(A, axis=1)``)."""
    A, B = np.asarray(A), np.asarray(B)
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[0] and A.shape[1] <= KMAX, (A.shape, B.shape)
    pa, sa = _pieces(A, axis=1) if left is None else left
    pb, sb = _pieces(B, axis=0)
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=LD)
    for total in range(2 * PIECES - 2, -1, -1):                                   # smallest products first
        for i in range(PIECES):
            j = total - i
            if 0 <= j < PIECES:
                acc += (pa[i] @ pb[j]).astype(LD)
    return acc * sa.astype(LD) * sb.astype(LD)


# ---- the basis ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def basis(T):
    """``(Q, sigma)`` of geometry.time_modes in long double: Q[t, a] = cos(pi (t + 1/2) a / n) sqrt((1 or 2) / n), sigma_a =
    (2 - 2 cos(pi a / n)) / h^2; read-only."""
    n = T + 1
    pi = np.arccos(LD(-1))
    a = np.arange(n).astype(LD)
    j = np.arange(n).astype(LD)
    Q = np.cos(pi * np.outer(j + LD(0.5), a) / LD(n)) * np.sqrt(np.where(np.arange(n) == 0, LD(1), LD(2)) / LD(n))[None, :]
    sigma = (LD(2) - LD(2) * np.cos(pi * a / LD(n))) * LD(T) * LD(T)
    Q.setflags(write=False)
    sigma.setflags(write=False)
    return Q, sigma


@functools.lru_cache(maxsize=None)
def _forward_pieces(T):
    return _pieces(basis(T)[0].T, axis=1)


def forward(T, x):
    """Q^T x in long double for the nodal x[T + 1, V]."""
    return ld_matmul(basis(T)[0].T, np.asarray(x, dtype=np.float64), left=_forward_pieces(T))


def octaves(n):
    """The bands [0], [1], [2, 3], [4..7], ... of the modes 0..n-1 (at most 11: n <= 1024)."""
    out, lo = [np.array([0])], 1
    while lo < n:
        out.append(np.arange(lo, min(2 * lo, n)))
        lo *= 2
    assert len(out) <= 11 and sum(s.size for s in out) == n
    return out


def band_of(a, n):
    return next(k for k, s in enumerate(octaves(n)) if s[0] <= a <= s[-1])


def band_rhs(T, V, S, seed, eps):
    """b[T + 1, V] = Q[:, S] bhat with bhat[S, V] standard normal, formed in long double and rounded once to fp64.  Mode 0 at eps == 0
    is made consistent (zero plain sum over the vertices)."""
    S = np.asarray(S)
    bhat = np.random.default_rng(seed).standard_normal((S.size, V))
    if eps == 0.0 and S[0] == 0:
        bhat[0] -= bhat[0].mean()
    Q, _ = basis(T)
    return np.asarray(ld_matmul(Q[:, S], bhat), dtype=np.float64)


def white_rhs(T, V, seed, eps):
    """The right-hand side of the existing tests: white in space and time, consistent at eps == 0."""
    b = np.random.default_rng(seed).standard_normal((T + 1, V))
    return b - b.mean() if eps == 0.0 else b


# ---- the operator -------------------------------------------------------------------------------------------------------------------
def plan_operator(plan):
    """``(K, mass)`` the device is handed (the plan's CSR and masses), dense and back in the caller's numbering."""
    V = plan.n_vertices
    perm = np.arange(V) if plan.perm_vert is None else np.asarray(plan.perm_vert)
    Kd = sp.csr_matrix((plan.lap_val, plan.lap_col, plan.lap_rowptr), shape=(V, V)).tocoo()
    K = sp.csr_matrix((Kd.data, (perm[Kd.row], perm[Kd.col])), shape=(V, V)).toarray()
    mass = np.empty(V)
    mass[perm] = plan.mass_vert
    return K, mass


def _dense(K):
    return K.toarray() if sp.issparse(K) else np.asarray(K, dtype=np.float64)


def kappa(K, mass, T, eps):
    """kappa_a = (lambda_max + sigma_a + eps) / (lambda_min + sigma_a + eps) from the dense generalized eigenvalues of (K, M);
    lambda_min is 0 (constants), and for mode 0 at eps == 0 the denominator is lambda_2."""
    lam = sla.eigh(_dense(K), np.diag(mass), eigvals_only=True)
    sigma = np.asarray(basis(T)[1], dtype=np.float64)
    low = np.full(T + 1, max(float(lam[0]), 0.0)) + sigma + eps
    if eps == 0.0:
        low[0] = float(lam[1])
    return (float(lam[-1]) + sigma + eps) / low


def remove_mean(x, mass):
    """``x[..., V]`` without its mass-weighted mean."""
    m = np.asarray(mass, dtype=x.dtype)
    return x - (x @ m)[..., None] / m.sum()


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def reference(K, mass, T, eps, b):
    """xr[a, v] in long double for b[T + 1, V], or xr[k, a, v] for a stack b[k, T + 1, V]: per mode a dense fp64 LU of
    K + (sigma_a + eps) M (mode 0 at eps == 0: + m m^T) and ``REFINE`` steps of iterative refinement with the residual in long double."""
    K = _dense(K)
    b = np.asarray(b, dtype=np.float64)
    stack = b if b.ndim == 3 else b[None]
    nb, n, V = stack.shape
    assert n == T + 1 and K.shape == (V, V)
    Q, sigma = basis(T)
    m = np.asarray(mass, dtype=np.float64)
    # bhat[a, k, v]
    bhat = forward(T, np.moveaxis(stack, 1, 0).reshape(n, nb * V)).reshape(n, nb, V)
    shift = np.asarray(sigma + LD(eps), dtype=np.float64)
    gauge = np.outer(m, m) if eps == 0.0 else None
    lus = []
    for a in range(n):
        A = K + np.diag(shift[a] * m)
        if a == 0 and gauge is not None:
            A = A + gauge
        lus.append(sla.lu_factor(A))
    m_ld, K_ld = m.astype(LD), K.astype(LD)
    x = np.zeros((n, nb, V), dtype=LD)
    for _ in range(REFINE + 1):
        Ax = ld_matmul(x.reshape(n * nb, V), K_ld.T).reshape(n, nb, V) + (sigma + LD(eps))[:, None, None] * m_ld * x
        if gauge is not None:
            Ax[0] += (x[0] @ m_ld)[:, None] * m_ld
        r = np.asarray(bhat - Ax, dtype=np.float64)
        for a in range(n):
            x[a] += sla.lu_solve(lus[a], r[a].T).T
    out = np.moveaxis(x, 1, 0)
    return out if b.ndim == 3 else out[0]


def inverse(T, xhat):
    """Q xhat rounded to fp64: the nodal array of a long-double modal one."""
    return np.asarray(ld_matmul(basis(T)[0], xhat), dtype=np.float64)


def mode_errors(x, xr, S, mass, eps):
    """``(e, leak)`` of the nodal x[T + 1, V] against xr[a, v]: e[i] = max_v |xhat_a - xr_a| / max_v |xr_a| for a = S[i] with xhat =
    Q^T x in long double, leak = max over the modes outside S of max_v |xhat_a - xr_a|, over the largest max_v |xr_a| inside S.  Mode 0
    at eps == 0 is compared without its mass-weighted mean."""
    n = xr.shape[0]
    S = np.asarray(S)
    xhat = forward(n - 1, x)
    if eps == 0.0:
        xhat[0], xr = remove_mean(xhat[0], mass), xr.copy()
        xr[0] = remove_mean(xr[0], mass)
    diff = np.max(np.abs(xhat - xr), axis=1)
    size = np.max(np.abs(xr), axis=1)
    e = np.asarray(diff[S] / np.maximum(size[S], LD(1e-300)), dtype=np.float64)
    out = np.ones(n, dtype=bool)
    out[S] = False
    leak = float(diff[out].max() / size[S].max()) if out.any() else 0.0
    return e, leak


def tolerances(p, kap, S):
    """``(tol[i] for a = S[i], tol_leak)``: 16 max(p, 2^-53 kappa_a), the leak with the largest kappa outside the band."""
    S = np.asarray(S)
    out = np.ones(kap.size, dtype=bool)
    out[S] = False
    tol = MARGIN * np.maximum(p, U * kap[S])
    return tol, (MARGIN * max(p, U * float(kap[out].max())) if out.any() else np.inf)


def fp64_floor(K, mass, T, eps, bands):
    """What rounding alone may cost ``plain_solve`` in the modes of every band S of ``bands``, from the basis and the spectrum (not from a solve):
    ``MARGIN`` (2^-53 kappa_a + |sigma64_a - sigma_a| / (lambda_min + sigma_a + eps)) for the per-mode solve with geometry.time_modes'
    fp64 sigma, plus the band's row and column sums of |Q^T Q64 - I| for the two fp64 transforms, times 4 for the ratio of the sizes of
    two modes of an octave."""
    from dots_socp_amd.geometry import time_modes

    Q, sigma = basis(T)
    Q64, sigma64 = time_modes(T)
    kap = kappa(K, mass, T, eps)
    low = (float(sla.eigh(_dense(K), np.diag(mass), eigvals_only=True)[1]) if eps == 0.0 else 0.0) * (np.arange(T + 1) == 0)
    dsig = np.abs(np.asarray(sigma64.astype(LD) - sigma, dtype=np.float64)) / (low + np.asarray(sigma, dtype=np.float64) + eps)
    E = np.abs(np.asarray(ld_matmul(Q.T, Q64) - np.eye(T + 1, dtype=LD), dtype=np.float64))
    return [MARGIN * (U * kap[S] + dsig[S]) + 4.0 * (E[np.ix_(S, S)].sum(axis=1) + E[np.ix_(S, S)].sum(axis=0)) for S in bands]


def describe(a, n):
    return f"mode {int(a)} (chunk {int(a) >> 8}, band {band_of(int(a), n)} of {len(octaves(n))}, T = {n - 1})"


def assert_modes(e, leak, tol, tol_leak, S, n, what=""):
    """Every mode of the band within its bound and the leak within its own; the message names the mode, its chunk a >> 8 and its band."""
    S = np.asarray(S)
    bad = np.nonzero(~(e <= tol))[0]
    if bad.size:
        i = bad[np.argmax(e[bad] / tol[bad])]
        raise AssertionError(f"{what}: {describe(S[i], n)}: error {e[i]:.3e} above {tol[i]:.3e}; {bad.size} of {S.size} modes of the band fail")
    assert leak <= tol_leak, f"{what}: leak out of band {band_of(int(S[0]), n)} (T = {n - 1}): {leak:.3e} above {tol_leak:.3e}"


# ---- the same operation in plain fp64, with deliberate defects ------------------------------------------------------------------------
def top_quarter(n):
    return 4 * np.arange(n) >= 3 * n


def last_chunk(n):
    """The modes of the last chunk of 256 (the sweeps' and the factorisation's cut of the mode axis), the last quarter below that."""
    return np.arange(n) >= ((n - 1) >> 8 << 8) if n > 256 else top_quarter(n)


def plain_solve(K, mass, T, eps, b, mutation=None):
    """Q64 solve_a(Q64^T b) for b[T + 1, V] (or a stack b[k, T + 1, V]) with geometry.time_modes and a dense Cholesky of K + (sigma_a + eps) M per mode; the singular mode 0 at
    eps == 0 is grounded at the last vertex (row and column dropped, x = 0 there) as the factor grounds its root pivot.

    ``mutation``: ``offdiag_high``  K's off-diagonal entries times 1 + 1e-4 in the modes a >= 3 n / 4;
                  ``stale_shift``   the modes of ``last_chunk`` take sigma_{a-1};
                  ``inverse_row``   the inverse transform's last time row times 1 + 1e-6 in the top quarter of modes;
                  ``forward_col``   the same in the forward transform;
                  ``ground_all``    mode 1 is grounded as mode 0 is."""
    from dots_socp_amd.geometry import time_modes

    assert mutation is None or mutation in MUTATIONS, mutation
    K = _dense(K)
    m = np.asarray(mass, dtype=np.float64)
    n, V = T + 1, m.size
    Q, sigma = time_modes(T)
    top, last = top_quarter(n), last_chunk(n)
    Qf, Qi = Q, Q
    if mutation == "forward_col":
        Qf = Q.copy()
        Qf[-1, top] *= 1.0 + 1e-6
    if mutation == "inverse_row":
        Qi = Q.copy()
        Qi[-1, top] *= 1.0 + 1e-6
    b = np.asarray(b, dtype=np.float64)
    stack = b if b.ndim == 3 else b[None]
    nb = stack.shape[0]
    bhat = (Qf.T @ np.moveaxis(stack, 1, 0).reshape(n, nb * V)).reshape(n, nb, V)
    K_off = K + 1e-4 * (K - np.diag(np.diag(K)))
    xhat = np.zeros((n, nb, V))
    for a in range(n):
        sig = sigma[a - 1] if mutation == "stale_shift" and last[a] else sigma[a]
        A = (K_off if mutation == "offdiag_high" and top[a] else K) + np.diag((sig + eps) * m)
        if (a == 0 and eps == 0.0) or (a <= 1 and mutation == "ground_all"):
            xhat[a, :, :-1] = sla.cho_solve(sla.cho_factor(A[:-1, :-1]), bhat[a, :, :-1].T).T
        else:
            xhat[a] = sla.cho_solve(sla.cho_factor(A), bhat[a].T).T
    out = np.moveaxis((Qi @ xhat.reshape(n, nb * V)).reshape(n, nb, V), 1, 0)
    return out if b.ndim == 3 else out[0]


def nodal_rel(x, want, mass, eps):
    """The figure of the existing tests: max|x - want| / max|want| over [T + 1, V], the gauge (the mass-weighted space-time mean)
    removed at eps == 0."""
    if eps == 0.0:
        w = np.broadcast_to(np.asarray(mass)[None, :], x.shape)
        x, want = x - np.sum(x * w) / np.sum(w), want - np.sum(want * w) / np.sum(w)
    return float(np.max(np.abs(x - want)) / max(np.max(np.abs(want)), 1e-300))
