"""CPU sweep behind the conditioning guards of the m x m solve (csrc/pdp_riccati.h, inverse_small_fast in csrc/pdp_tile.h); no GPU needed.

The kernels' algebra (K = Quu^-1 Qux, k = Quu^-1 Que, P- = Hxx + F'PF - Qux'K symmetrised, U = -(K X + k)) is emulated in numpy fp64 with the inverse written as in
the kernel source - the lane-parallel cofactor form for m = 4, the adjugate of inverse_small_fast for m = 3, 2 - ALWAYS taken (no guard), and with the pivoted
Gauss-Jordan inverse behind the guards.  Inputs: tests/riccati_conditioning_common.py (rank-1 G and its `near` variant, Huu scaled by s) over a grid of s and seeds.
Each run is compared with the reference's formulas in 40-digit arithmetic (oracle.pdp_oracle.lqr_solver_mp) and reports the smallest guard quantity it met,
    m = 4:     q = |det| / sum of |terms| of the Laplace expansion along row 0
    m = 3, 2:  q = |det| / |product of the diagonal|
so that the error of the unguarded fast path can be read against q.  The guard thresholds are set where that error is still a tenth of the 1e-10 tolerance.

Second part: the smallest q the five shipped systems meet along their stored demonstrations (tests/golden/ref_auxsys_*.npz) - above the thresholds the guards send
them down the same path as before and their results do not change by a bit.

    python probes/riccati_guard_sweep.py > profiles/riccati_guard_sweep.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import riccati_conditioning_common as rc      # noqa: E402


def inv_pivoted(A):
    """inverse_small<M>: Gauss-Jordan with partial pivoting"""
    M = A.shape[0]
    a, b = A.astype(float).copy(), np.eye(M)
    for k in range(M):
        for i in range(k + 1, M):
            if abs(a[i, k]) > abs(a[k, k]):
                a[[k, i]], b[[k, i]] = a[[i, k]], b[[i, k]]
        ip = 1.0 / a[k, k]
        a[k] *= ip
        b[k] *= ip
        for i in range(M):
            if i != k:
                f = a[i, k]
                a[i] = a[i] - f * a[k]
                b[i] = b[i] - f * b[k]
    return b


def _cof3(m):
    return m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0])


def inv_cofactor(A):
    """the kernels' fast path without its guard -> (inverse, guard quantity q)"""
    M = A.shape[0]
    if M == 4:
        C = np.empty((4, 4))
        for i in range(4):
            for j in range(4):
                c = _cof3(np.delete(np.delete(A, i, 0), j, 1))
                C[i, j] = -c if (i + j) & 1 else c
        t = A[0] * C[0]
        det, mag = (t[0] + t[1]) + (t[2] + t[3]), (abs(t[0]) + abs(t[1])) + (abs(t[2]) + abs(t[3]))
        return C.T / det, abs(det) / mag
    a = A.reshape(-1)
    if M == 3:
        c = np.array([a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                      a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                      a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]])
        det = a[0] * c[0] + a[1] * c[3] + a[2] * c[6]
    else:
        c = np.array([a[3], -a[1], -a[2], a[0]])
        det = a[0] * a[3] - a[1] * a[2]
    return (c / det).reshape(M, M), abs(det) / abs(np.prod(np.diag(A)))


def kernel_algebra(pr, inverse):
    """X, U, Lam by the kernels' recursion with the given inverse(A) -> (Z, q); also the smallest q of the sweep"""
    T = pr["F"].shape[0]
    P, W = pr["hxx"], pr["hxe"]
    K, k, PP, WW, qmin = T * [None], T * [None], T * [None], T * [None], np.inf
    for t in range(T - 1, -1, -1):
        F, G, E = pr["F"][t], pr["G"][t], pr["E"][t]
        PP[t], WW[t] = P, W
        PF, PEW = P @ F, P @ E + W
        Quu, Qux, Que = pr["Huu"][t] + G.T @ (P @ G), pr["Hxu"][t].T + G.T @ PF, pr["Hue"][t] + G.T @ PEW
        Z, q = inverse(Quu)
        qmin = min(qmin, q)
        K[t], k[t] = Z @ Qux, Z @ Que
        Pn = pr["Hxx"][t] + F.T @ PF - Qux.T @ K[t]
        W = pr["Hxe"][t] + F.T @ PEW - Qux.T @ k[t]
        P = 0.5 * (Pn + Pn.T)
    X, U, Lam = [pr["X0"]], [], []
    for t in range(T):
        U.append(-(K[t] @ X[t] + k[t]))
        X.append(pr["F"][t] @ X[t] + pr["G"][t] @ U[t] + pr["E"][t])
        Lam.append(PP[t] @ X[t + 1] + WW[t])
    return (np.stack(X), np.stack(U), np.stack(Lam)), qmin


def worst(got, exact):
    return max(rc.rel(g, e) for g, e in zip(got, exact))


def sweep():
    n, p, T = 6, 5, rc.T
    grid = [10.0 ** (-0.5 * k) for k in range(13)]            # s = 1 .. 1e-6
    print("# part 1: error of X, U, Lam (largest of the three, max |diff| / max |exact|) against the 40-digit evaluation, n = %d, p = %d, T = %d" % (n, p, T))
    print("# %-2s %-5s %-4s %-9s %-10s %-12s %-12s %-12s" % ("m", "G", "seed", "s", "q min", "fast path", "pivoted", "reference"))
    rows = []
    for m in (4, 3, 2):
        for near in (False, True):
            for seed in (3, 4, 5, 6):
                for s in grid:
                    pr = rc.lqr_problem(n, m, p, T, s, seed, near)
                    exact = rc.solve_mp(pr)
                    fast, q = kernel_algebra(pr, inv_cofactor)
                    piv, _ = kernel_algebra(pr, lambda A: (inv_pivoted(A), 1.0))
                    row = (m, near, seed, s, q, worst(fast, exact), worst(piv, exact), worst(rc.solve_ref(pr), exact))
                    rows.append(row)
                    print("  %-2d %-5s %-4d %-9.2e %-10.2e %-12.2e %-12.2e %-12.2e" % (m, "near" if near else "rank1", seed, s, *row[4:]))
                    sys.stdout.flush()
    print("#\n# part 2: the unguarded fast path's worst error by decade of q (all seeds, both G variants), and the pivoted path's on the same problems")
    for m in (4, 3, 2):
        for d in range(0, -12, -1):
            sel = [r for r in rows if r[0] == m and 10.0 ** (d - 1) < r[4] <= 10.0 ** d]
            if sel:
                print("  m = %d   1e%-3d < q <= 1e%-3d  runs %-3d  fast path <= %.2e   pivoted <= %.2e" % (m, d - 1, d, len(sel), max(r[5] for r in sel), max(r[6] for r in sel)))
    print("#\n# part 3: for each candidate threshold, the fast path's worst error over the runs that stay above it")
    for m in (4, 3, 2):
        for thr in (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4, 1e-5, 1e-6, 1e-10):
            sel = [r[5] for r in rows if r[0] == m and r[4] > thr]
            print("  m = %d   q > %-7.0e  runs %-3d  fast path <= %s" % (m, thr, len(sel), "%.2e" % max(sel) if sel else "-"))


def shipped():
    from oracle import pdp_oracle as po
    print("#\n# part 4: smallest q along the stored demonstrations of the shipped systems (tests/golden/ref_auxsys_*.npz)")
    for name in ("pendulum", "cartpole", "robotarm", "quadrotor", "rocket"):
        a = np.load(os.path.join(ROOT, "tests", "golden", "ref_auxsys_%s.npz" % name))
        B, T, n, m = a["dynG"].shape
        qmin = np.inf
        for b in range(B):
            sol = po.lqr_solver(*[list(a[k][b]) for k in ("dynF", "dynG", "dynE", "Hxx", "Huu", "Hxu", "Hxe", "Hue")], [a["hxx"][b, 0]], [a["hxe"][b, 0]],
                                np.zeros((n, a["hxe"].shape[-1])), T)
            for t in range(T):
                Quu = a["Huu"][b, t] + a["dynG"][b, t].T @ sol["PP"][t] @ a["dynG"][b, t]
                qmin = min(qmin, 1.0 if m == 1 else inv_cofactor(Quu)[1])
        print("  %-10s m = %d  demos %-3d T = %-3d  q min %s" % (name, m, B, T, "1 (scalar: no cancellation)" if m == 1 else "%.3e" % qmin))


if __name__ == "__main__":
    shipped()
    sweep()
