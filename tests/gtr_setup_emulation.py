"""gtr_setup_kernel (tapir_amd/csrc/gtr_setup_kernel.hpp) restated in numpy, operation by operation and in the kernel's
order, for tests that must know what eigen-system a LocusModel holds for given pi and exchangeabilities without a GPU.  Every
product and sum is rounded on its own; the device may contract some into FMAs, so the last bits differ, the structure does
not.  (Test helper, not a conftest.)

keep="projected" is the kernel: the three vectors kept beside the exact stationary one have their component along sqrt(pi)
removed and are re-orthonormalised (modified Gram-Schmidt, sqrt(pi) first; a component of 8 eps of its own rounding scale or
less (along sqrt(pi): of its own terms; between two kept vectors: of 1) is left alone, so that on a well separated spectrum
nothing moves).  keep="jacobi" is the kernel before that: the three
vectors as the Jacobi iteration left them."""
import collections
import math

import numpy as np

LocusModel = collections.namedtuple("LocusModel", "lam U Ui pi kappa")   # lam [3], U [4, 3], Ui [3, 4], pi [4], kappa
KEEP = ("projected", "jacobi")
K_KEEP = 8 * 2.0 ** -52        # kKeep of the kernel: a component within this of its own rounding scale is left alone


def _jacobi(pi, exch):
    """The kernel up to the end of its sweeps: the normalised pi, sqrt(pi), kappa, the diagonalised A and the vectors V."""
    pi = np.asarray(pi, np.float64)
    psum = 0.0
    for i in range(4):
        psum += pi[i]
    pi = np.array([pi[i] / psum for i in range(4)])
    sq = np.sqrt(pi)
    e = [float(x) for x in exch]
    R = [[0, e[0], e[1], e[2]], [e[0], 0, e[3], e[4]], [e[1], e[3], 0, e[5]], [e[2], e[4], e[5], 0]]
    A, V = np.zeros((4, 4)), np.eye(4)
    kappa = 0.0
    for i in range(4):
        row = 0.0
        for j in range(4):
            if j != i:
                row += R[i][j] * pi[j]
                A[i, j] = sq[i] * R[i][j] * sq[j]
        A[i, i] = -row
        kappa += pi[i] * row
    for _ in range(30):
        off = 0.0
        for p in range(4):
            for q in range(p + 1, 4):
                off += A[p, q] * A[p, q]
        if off < 1e-290:
            break
        for p in range(4):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(over="ignore"):                      # theta and its square may overflow to inf, as in C
                    theta = float((A[q, q] - A[p, p]) / (2.0 * apq))
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for M, cols in ((A, True), (A, False), (V, True)):
                    for k in range(4):
                        a, b = ((k, p), (k, q)) if cols else ((p, k), (q, k))
                        x, y = M[a], M[b]
                        M[a], M[b] = c * x - s * y, s * x + c * y
    return pi, sq, kappa, A, V


def gtr_setup(pi, exch, keep="projected"):
    """The LocusModel the kernel writes for one locus (slot 0, lam = 0 with U[:, 0] = 1 and Ui[0] = pi, is implicit)."""
    assert keep in KEEP
    pi, sq, kappa, A, V = _jacobi(pi, exch)
    z = 0
    for k in range(1, 4):
        if A[k, k] > A[z, z]:
            z = k
    order = [k for k in range(4) if k != z]
    W = np.empty((4, 3))
    for o, k in enumerate(order):
        v = V[:, k].copy()
        if keep == "projected":
            for b in [sq] + [W[:, p] for p in range(o)]:
                d, scale = 0.0, 0.0
                for i in range(4):
                    d += b[i] * v[i]
                    scale += abs(b[i] * v[i])
                if abs(d) > K_KEEP * (scale if b is sq else 1.0):
                    v = np.array([v[i] - d * b[i] for i in range(4)])
            n = 0.0
            for i in range(4):
                n += v[i] * v[i]
            if abs(n - 1.0) > K_KEEP:
                v = v * (1.0 / math.sqrt(n))
        W[:, o] = v
    lam = np.array([A[k, k] for k in order])
    U = np.array([[W[i, o] / sq[i] for o in range(3)] for i in range(4)])
    Ui = np.array([[W[i, o] * sq[i] for i in range(4)] for o in range(3)])
    return LocusModel(lam, U, Ui, pi, kappa)


def transition(m, tau):
    """P(tau) in the stage-2 kernels' product form: P_ij = pi_j + sum_k U_ik e^(lam_k tau) Ui_kj, in fp64."""
    e = [math.exp(x * tau) for x in m.lam]
    return np.array([[m.pi[j] + sum(m.U[i, k] * e[k] * m.Ui[k, j] for k in range(3)) for j in range(4)] for i in range(4)])

