"""Every factorisation path of the band QP (csrc/bmpc_bandqp.h) at its switch-over shapes.

The device solver has four factor / solve paths, chosen from the KKT dimension nk, the bandwidth
bw (W = bw + 1) and the batch size: blocked with the band in LDS (a batch of at most one problem
per CU, bw + 8 <= 64), column-at-a-time with the band in LDS (bw >= 57), the ring window with
W <= 64 (more problems than CUs, or a band that does not fit LDS) and the ring window with W > 64
(entries past the 64 lanes loaded at retirement).  The problems of tests/bandqp_families.py pin
nk and bw -- exactly for the unconstrained family, by regime for the constrained one -- and every
test reads the regime from the solver's returned ``info``, never from the generator's arguments.

Checked on the CPU through the host build (tests/hostsim: the column-at-a-time kernels) and on
the GPU through libbmpc.so:
  * the unconstrained table against LAPACK + one extended-precision correction, under a bound
    derived from the refinement's stopping rule (no refinement of the IPM hides a wrong factor:
    the solver returns after one factorisation and one refined solve);
  * the constrained problems and the reference's belief problems against the oracle, x and the
    optimality conditions of y, on every path;
  * (GPU) a problem solved alone (band in LDS) against the same problem as a member of a batch of
    CUs + 1 (ring window): x, y, status and iterations bit for bit;
  * statuses other than 1, max_iter and eps (both part of the analysis cache key), 1e20 as
    infinity, the eviction of the 8-entry analysis cache, the LDS limits.
"""
import functools
import types

import numpy as np
import pytest

import bandqp_families as F
from bmpc.plan import qp_arrays
from test_bandqp import X_TOL, belief_problems, check_kkt, oracle_solve


def host_solve(P, q, A, l, u, max_iter=100, eps=1e-10):
    import hostsim_lib as H
    a = qp_arrays(P, q, A, l, u)
    return H.qp_solve(a["n"], a["m"], a["Pp"], a["Pi"], a["Ap"], a["Ai"], a["Px"], a["q"], a["Ax"], a["l"], a["u"],
                      max_iter=max_iter, eps=eps)


# ---- the table: every problem and its reference, built once ---------------------------------------
@functools.lru_cache(maxsize=None)
def edge(n, b):
    P, q, A, l, u = F.unconstrained(n, b)
    x_ref = F.unconstrained_reference(P, q)
    bound, ninv = F.unconstrained_bound(P, q, x_ref, b)
    for a in (P, q, x_ref):
        a.setflags(write=False)
    return dict(qp=(P, q, A, l, u), x_ref=x_ref, bound=bound, ninv=ninv)


@functools.lru_cache(maxsize=None)
def iterating(key):
    """A constrained-family problem (its argument tuple) or a recorded belief problem (its name),
    with the oracle's optimum."""
    if isinstance(key, tuple):
        qp = F.constrained(*key)
        x_ref, info = oracle_solve(*qp)
        assert info["status_val"] == 1
    else:
        name, t, P, q, A, l, u, x_ref = next(p for p in belief_problems() if p[0] == key)
        qp = (P, q, A, l, u)
    return dict(qp=qp, x_ref=x_ref)


BELIEF = ["belief_m1", "belief_m2"]
ITERATING = [k for k, _ in F.CONSTRAINED] + BELIEF
ids = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


def widest_window(nk):
    """The largest bw whose (bw+1)^2 window, multipliers and solve vector fit the LDS."""
    bw = 0
    while F.window_fits(nk, bw + 1):
        bw += 1
    return bw


def check_edge(r, n, b):
    """Unconstrained problem: |x - x_ref|_inf <= 2 (|P^-1|_inf (1e-15 max(1, |q|_inf) + g |(|P||x| + |q|)|_inf)
    + u |x_ref|_inf), g = k u / (1 - k u), k = 2 b + 3, u = 2^-53.

    The solver's refined solve stops when the residual b - K x it computes falls below
    1e-15 max(1, |b|_inf) (bqp_solve_refined; b = -q here), or after three corrections, whose
    limit for these well-conditioned P is the rounding of the residual itself.  The computed
    residual differs from the true one by the rounding of one band mat-vec -- 2b + 1 products
    summed in a row, then the subtraction from b: at most g (|P||x| + |q|) entrywise -- so
    |P x + q|_inf <= stop + rounding and |x - x*|_inf <= |P^-1|_inf times that.  x_ref carries
    one rounding to double of x* (u |x_ref|).  The stated margin is the factor 2.  The regularised
    pivots (P + 1e-8 I is what gets factored) do not enter: refinement runs on the true matrix.
    Measured: the host build is at 1e-16 .. 8e-16 relative on this table, the bound at 1e-14 to
    3e-14 absolute, the device at or below 4.4e-16 absolute on every path.  Tried on a scratch
    build of the blocked factorisation with the j = NB - 1 term of its trailing update dropped:
    4e-13 .. 1.8e-10 on every blocked shape (bw 1 .. 56), after 1 .. 3 Newton steps the wrong
    factor bought (iters != 0), and the bits of the window path no longer matched."""
    e = edge(n, b)
    err = np.abs(r["x"][0] - e["x_ref"]).max()
    print(f"n {n} bw {b}: |x - x_ref| {err:.2e}, bound {e['bound']:.2e}, |P^-1| {e['ninv']:.3f}, "
          f"status {r['status'][0]}, iters {r['iters'][0]}")
    assert tuple(r["info"][:2]) == (n, b), (n, b, r["info"])       # the regime, from the solver
    assert r["status"][0] == 1, (n, b, r["status"])
    assert err <= e["bound"], (n, b, err, e["bound"])
    # one factorisation, one refined solve: a residual left above eps would buy Newton steps
    assert r["iters"][0] == 0, (n, b, r["iters"])


def check_iterating(r, key, want=None):
    """Constrained problem: x against the oracle at X_TOL, the optimality conditions of y."""
    p = iterating(key)
    P, q, A, l, u = p["qp"]
    nk, bw = (int(v) for v in r["info"][:2])
    if want is not None:
        assert F.REGIME[want](nk, bw), (key, want, nk, bw)
    elif key in BELIEF:
        assert bw < 40 and nk > 4 * bw, (key, nk, bw)
    assert r["status"][0] == 1 and r["iters"][0] >= 5, (key, r["status"], r["iters"])   # the IPM iterated
    xo = p["x_ref"]
    np.testing.assert_allclose(r["x"][0], xo, atol=X_TOL * max(1, np.abs(xo).max()), err_msg=str(key))
    check_kkt(P, q, A, l, u, r["x"][0], r["y"][0])
    return nk, bw


def perturbed_q(q, B, seed):
    return q[None, :] + 0.1 * np.random.default_rng(seed).normal(size=(B, len(q)))


# ---- the status and argument cases, written once for the host build and the GPU --------------------
def small_qp(seed=4, n=8):
    """Two rows on x0 -- a lower bound and an upper bound -- and a few more; the bounds on x0 are
    the caller's to move (feasible [-1, 1], or x0 >= 1 and x0 <= -1: infeasible)."""
    rng = np.random.default_rng(seed)
    P = F.banded_P(n, 2, rng)
    A = np.zeros((5, n))
    A[0, 0] = A[1, 0] = 1.0
    A[2, 1], A[2, 2] = 1.0, -1.0
    A[3, 3], A[3, 5] = 1.0, 0.5
    A[4, n - 1] = 1.0
    l = np.array([-1.0, -np.inf, 0.25, -np.inf, -0.5])
    u = np.array([np.inf, 1.0, 0.25, 0.3, 0.5])
    return P, -P @ (3.0 * rng.normal(size=n)), A, l, u


def infeasible_bounds(l, u):
    l, u = l.copy(), u.copy()
    l[0], u[1] = 1.0, -1.0      # x0 >= 1 and x0 <= -1
    return l, u


def status_and_argument_cases(solve):
    P, q, A, l, u = small_qp()
    li, ui = infeasible_bounds(l, u)
    # an infeasible problem runs out of iterations
    for mi in (25, 100):
        r = solve(P, q, A, li, ui, max_iter=mi)
        assert r["status"][0] == -2 and r["iters"][0] == mi, (mi, r["status"], r["iters"])
    # ... and does not disturb the feasible members of its batch
    B = 5
    qs = perturbed_q(q, B, 1)
    lb, ub = np.tile(l, (B, 1)), np.tile(u, (B, 1))
    lb[2], ub[2] = li, ui
    rb = solve([P] * B, qs, [A] * B, lb, ub)
    assert rb["status"].tolist() == [1, 1, -2, 1, 1] and rb["iters"][2] == 100, (rb["status"], rb["iters"])
    for b in (0, 1, 3, 4):
        one = solve(P, qs[b], A, l, u)
        for k in ("x", "y", "status", "iters"):
            np.testing.assert_array_equal(rb[k][b], one[k][0], err_msg=f"{k} of member {b}")
    # max_iter: three iterations are too few; the same pattern with 100 afterwards is solved
    r3 = solve(P, q, A, l, u, max_iter=3)
    assert r3["status"][0] == -2 and r3["iters"][0] == 3, (r3["status"], r3["iters"])
    full = solve(P, q, A, l, u, max_iter=100)
    assert full["status"][0] == 1 and full["iters"][0] > 3
    xo, _ = oracle_solve(P, q, A, l, u)
    np.testing.assert_allclose(full["x"][0], xo, atol=X_TOL * max(1, np.abs(xo).max()))
    # eps: a looser tolerance stops strictly earlier; going back to 1e-10 gives the first result's bits
    tight = solve(P, q, A, l, u, eps=1e-10)
    loose = solve(P, q, A, l, u, eps=1e-4)
    again = solve(P, q, A, l, u, eps=1e-10)
    assert tight["status"][0] == loose["status"][0] == again["status"][0] == 1
    assert loose["iters"][0] < tight["iters"][0], (loose["iters"], tight["iters"])
    for k in ("x", "y", "iters"):
        np.testing.assert_array_equal(again[k], tight[k], err_msg=k)
        np.testing.assert_array_equal(full[k], tight[k], err_msg=k)
    # +-1e20 is infinity
    big = solve(P, q, A, np.where(np.isinf(l), -1e20, l), np.where(np.isinf(u), 1e20, u))
    for k in ("x", "y", "status", "iters", "info"):
        np.testing.assert_array_equal(big[k], tight[k], err_msg=k)


# ---- CPU: the host build ---------------------------------------------------------------------------
def test_lds_limits_of_the_table():
    """The shapes at the LDS limits are where the table says, recomputed from bandqp_lds_doubles."""
    assert F.fits_in_lds(571, 31) and not F.fits_in_lds(572, 31)
    assert all(F.fits_in_lds(n, b) for n, b in F.EDGES if (n, b) not in ((572, 31), (200, 139), (200, 140)))
    assert widest_window(200) == 140 and F.window_fits(200, 139) and not F.fits_in_lds(200, 139)
    assert (200, widest_window(200)) in F.EDGES and (200, 139) in F.EDGES


@pytest.mark.parametrize("n,b", F.EDGES, ids=lambda v: str(v))
def test_host_build_unconstrained_table(n, b):
    check_edge(host_solve(*edge(n, b)["qp"]), n, b)


def test_host_build_unconstrained_window_path_same_bits():
    """More problems than the analysis' default 256 CUs: the host build streams the band through
    the ring window (one lane: every entry of the entering row is loaded at retirement)."""
    B = 257
    for n, b in [(9, 8), (65, 9), (130, 56), (130, 64), (66, 64), (150, 100)]:
        P, q, A, l, u = edge(n, b)["qp"]
        qs = perturbed_q(q, B, n)
        qs[128] = q
        big = host_solve([P] * B, qs, [A] * B, np.zeros((B, 0)), np.zeros((B, 0)))
        check_edge({k: big[k][128:129] if k != "info" else big[k] for k in big}, n, b)
        for m in (0, 128, B - 1):
            one = host_solve(P, qs[m], A, l, u)
            for k in ("x", "status", "iters"):
                np.testing.assert_array_equal(big[k][m], one[k][0], err_msg=f"{n} {b}: {k} of member {m}")


def test_host_build_rejects_a_window_one_step_too_wide():
    bw = widest_window(200) + 1
    with pytest.raises(RuntimeError, match=f"bandwidth {bw} .*LDS"):
        host_solve(*F.unconstrained(200, bw))


@pytest.mark.parametrize("key,want", F.CONSTRAINED, ids=ids)
def test_host_build_constrained_regimes(key, want):
    check_iterating(host_solve(*iterating(key)["qp"]), key, want)


def test_host_build_status_and_arguments():
    status_and_argument_cases(host_solve)


# ---- libbmpc.so on the GPU -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from bmpc import plan
    plan.context(0)
    return types.SimpleNamespace(qp_solve=plan.qp_solve, cus=torch.cuda.get_device_properties(0).multi_processor_count)


def same_bits_on_both_paths(gpu, qp, what):
    """The problem alone (band in LDS) and as members first, middle and last of a batch of
    CUs + 1 with perturbed q (ring window): identical x, y, status, iters.  Returns the middle member."""
    P, q, A, l, u = qp
    B = gpu.cus + 1
    qs = perturbed_q(q, B, 7)
    qs[B // 2] = q
    m = len(l)
    big = gpu.qp_solve([P] * B, qs, [A] * B, np.tile(l, (B, 1)), np.tile(u, (B, 1)))
    for b in (0, B // 2, B - 1):
        one = gpu.qp_solve(P, qs[b], A, l, u)
        for k in ("x", "y", "status", "iters"):
            np.testing.assert_array_equal(big[k][b], one[k][0], err_msg=f"{what}: {k} of member {b}")
        np.testing.assert_array_equal(big["info"], one["info"])
    assert big["y"].shape == (B, m)
    return {k: big[k][B // 2:B // 2 + 1] if k != "info" else big[k] for k in big}


@pytest.mark.gpu
@pytest.mark.parametrize("n,b", F.EDGES, ids=lambda v: str(v))
def test_gpu_unconstrained_table_on_both_paths(gpu, n, b):
    """Alone: blocked (bw <= 56) or column-at-a-time (bw >= 57) with the band in LDS, or the
    window where the band does not fit; in a batch of CUs + 1: the window.  Each against the
    reference under check_edge's bound, and against each other bit for bit."""
    qp = edge(n, b)["qp"]
    check_edge(gpu.qp_solve(*qp), n, b)
    check_edge(same_bits_on_both_paths(gpu, qp, (n, b)), n, b)


@pytest.mark.gpu
@pytest.mark.parametrize("key", ITERATING, ids=ids)
def test_gpu_iterating_problems_on_both_paths(gpu, key):
    """x against the oracle and the optimality conditions of y on the in-LDS path and on the
    window path, and the two bit for bit, iterations included."""
    want = dict(F.CONSTRAINED).get(key)
    qp = iterating(key)["qp"]
    nk, bw = check_iterating(gpu.qp_solve(*qp), key, want)
    assert (nk, bw) == check_iterating(same_bits_on_both_paths(gpu, qp, key), key, want)


@pytest.mark.gpu
def test_gpu_rejects_a_window_one_step_too_wide(gpu):
    bw = widest_window(200) + 1
    with pytest.raises(RuntimeError, match=rf"\(-22\).*bandwidth {bw} .*LDS"):
        gpu.qp_solve(*F.unconstrained(200, bw))


@pytest.mark.gpu
def test_gpu_status_and_arguments(gpu):
    status_and_argument_cases(gpu.qp_solve)


@pytest.mark.gpu
def test_gpu_analysis_cache_eviction(gpu):
    """Ten patterns through the 8-entry cache, then the first again: its analysis was evicted and
    is rebuilt, the result is the first result exactly."""
    qps = [F.constrained(6 + i, 2, 3, 1, 2, seed=9) for i in range(10)]
    first = [gpu.qp_solve(*qp) for qp in qps]
    assert all(r["status"][0] == 1 for r in first)
    assert len({tuple(r["info"]) for r in first}) == 10
    for i in (0, 1, 9):
        again = gpu.qp_solve(*qps[i])
        for k in ("x", "y", "status", "iters", "info"):
            np.testing.assert_array_equal(again[k], first[i][k], err_msg=f"pattern {i}: {k}")
