"""QP families whose KKT band is controlled, for the band QP's path tests (test_bandqp_paths.py).

The device solver (csrc/bmpc_bandqp.h) picks its factorisation from the KKT dimension nk, the
bandwidth bw after the reverse Cuthill-McKee ordering and the batch size.  ``unconstrained``
problems have exactly nk = n, bw = b; ``constrained`` problems add rows around a feasible point so
the interior point iterates, with bw only roughly controlled (every test asserts the regime from
the solver's returned info).  Everything is seeded: a table entry is the same problem everywhere.
"""
import numpy as np

LDS_BYTES = 160 * 1024   # LDS of a CU (the analysis default, bmpc_qpplan.h)
NB = 8                   # BMPC_BQP_NB: columns per block of the blocked factorisation


def lds_doubles(nk, W, lb_lds):
    """bandqp_lds_doubles (csrc/bmpc_bandqp.h) restated."""
    return W + nk + (nk * W + nk + 2 * 64 * NB if lb_lds else W * W)


def fits_in_lds(nk, bw):
    """The whole band fits LDS: a batch of at most one problem per CU factors it in place."""
    return lds_doubles(nk, bw + 1, True) * 8 <= LDS_BYTES


def window_fits(nk, bw):
    return lds_doubles(nk, bw + 1, False) * 8 <= LDS_BYTES


def banded_P(n, b, rng):
    """Full symmetric band of half-width b (every entry |i - j| <= b nonzero), strictly
    diagonally dominant: P_ii = 1.25 sum_j |P_ij| + U(1, 2), so cond(P) <= 9 (Gershgorin)."""
    P = np.zeros((n, n))
    for k in range(1, min(b, n - 1) + 1):
        v = rng.uniform(0.2, 1.0, n - k) * rng.choice([-1.0, 1.0], n - k)
        P += np.diag(v, k) + np.diag(v, -k)
    P += np.diag(1.25 * np.abs(P).sum(axis=1) + rng.uniform(1.0, 2.0, n))
    return P


def unconstrained(n, b, seed=0):
    """(P, q, A, l, u) with m = 0: nk = n, bw = b exactly."""
    rng = np.random.default_rng([seed, n, b])
    return banded_P(n, b, rng), rng.normal(size=n) * 3.0, np.zeros((0, n)), np.zeros(0), np.zeros(0)


def unconstrained_reference(P, q):
    """x* = -P^-1 q: LAPACK's solve and one residual correction in extended precision."""
    x = np.linalg.solve(P, -q)
    r = (-q).astype(np.longdouble) - P.astype(np.longdouble) @ x.astype(np.longdouble)
    return (x.astype(np.longdouble) + np.linalg.solve(P, r.astype(np.float64)).astype(np.longdouble)).astype(np.float64)


def unconstrained_bound(P, q, x_ref, b):
    """The bound on |x - x_ref|_inf for a solver that stops at the refinement's rule (see
    test_bandqp_paths.test_*_unconstrained_table): returns (bound, |P^-1|_inf)."""
    u = 2.0 ** -53
    ninv = np.abs(np.linalg.inv(P)).sum(axis=1).max()
    k = 2 * b + 3    # 2b + 1 products and their sums in a row of the band mat-vec, then b - Kx
    matvec = k * u / (1 - k * u) * (np.abs(P) @ np.abs(x_ref) + np.abs(q)).max()
    stop = 1e-15 * max(1.0, np.abs(q).max())
    return 2.0 * (ninv * (stop + matvec) + u * np.abs(x_ref).max()), ninv


def constrained(n, b, box, neq, one, seed=0):
    """Banded P plus ``box`` two-sided rows on single variables, ``neq`` equality rows coupling
    neighbours and ``one`` one-sided rows coupling x_i and x_{i+b}; every bound is built around a
    feasible x0 and the unconstrained minimiser lies far outside the boxes, so rows are active."""
    rng = np.random.default_rng([seed, n, b, box, neq, one])
    P = banded_P(n, b, rng)
    x0 = rng.normal(size=n)
    rows, lo, hi = [], [], []
    for i in np.linspace(0, n - 1, box).round().astype(int) if box else []:
        a = np.zeros(n)
        a[i] = 1.0
        rows.append(a), lo.append(x0[i] - rng.uniform(0.1, 1.0)), hi.append(x0[i] + rng.uniform(0.1, 1.0))
    for i in np.linspace(0, n - 2, neq).round().astype(int) if neq else []:
        a = np.zeros(n)
        a[i], a[i + 1] = 1.0, rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
        rows.append(a), lo.append(a @ x0), hi.append(a @ x0)
    for i in np.linspace(0, n - 1 - max(b, 1), one).round().astype(int) if one else []:
        a = np.zeros(n)
        a[i], a[i + max(b, 1)] = rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
        rows.append(a), lo.append(-np.inf), hi.append(a @ x0 + rng.uniform(0.0, 1.0))
    A = np.array(rows).reshape(len(rows), n)
    q = -P @ (x0 + 3.0 * rng.normal(size=n))
    return P, q, A, np.array(lo, float), np.array(hi, float)


# ---- the shape table ----------------------------------------------------------------------------
# (n, b) of the unconstrained family: the smallest shapes that reach each branch of the kernels
EDGES = [
    (1, 0), (9, 0),                                   # bw = 0: no off-diagonal work at all
    (65, 1),                                          # bw = 1, a second trip of the 64 lanes
    # bw 7 / 8 / 9 around the mat-vec's 8-wide chunks; nk % 8 in {0, 1, 7} on both sides of 64 and
    # of 128 (one row / two rows per lane and trip, a second trip)
    (56, 7), (63, 8), (65, 9), (72, 8), (121, 7), (127, 9), (128, 8), (129, 7), (135, 9),
    (130, 56), (130, 57),                             # last blocked band, first column-at-a-time band in LDS
    (130, 63), (130, 64),                             # W = 64 and W = 65 (entries past the 64 lanes)
    (150, 100),
    (9, 8), (10, 8), (58, 57), (59, 57), (65, 64), (66, 64),   # dense (nk = bw + 1) and nk = bw + 2
    (571, 31), (572, 31),                             # the last band that fits LDS and the first that does not
    (200, 139), (200, 140),                           # wide windows (the window is the whole LDS)
]

# (n, b, box, neq, one) of the constrained family with the regime each must land in
CONSTRAINED = [
    ((20, 3, 6, 3, 4), "bw <= 8"),                              # nk = 39, bw = 7 on the host build
    ((48, 40, 10, 4, 6), "41 <= bw <= 56, nk % 8 != 0"),        # nk = 78, bw = 46
    ((60, 52, 10, 4, 6), "41 <= bw <= 56, nk % 8 != 0"),        # nk = 90, bw = 56: the last blocked band
    ((70, 55, 6, 2, 3), "57 <= bw <= 63"),                      # nk = 87, bw = 58
    ((50, 20, 50, 10, 25), "bw >= 65"),                         # nk = 185, bw = 81
]
REGIME = {
    "bw <= 8": lambda nk, bw: bw <= 8,
    "41 <= bw <= 56, nk % 8 != 0": lambda nk, bw: 41 <= bw <= 56 and nk % 8 != 0,
    "57 <= bw <= 63": lambda nk, bw: 57 <= bw <= 63,
    "bw >= 65": lambda nk, bw: bw >= 65,
}
