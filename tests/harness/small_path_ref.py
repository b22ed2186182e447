"""Extended-precision references of the small-problem passes (scip-sdp_amd/csrc/kernels.hip: hs_dir_block_small, hs_lp_rows_small,
hs_apply_A_small, hs_lp_dir, hs_vec_mul, hs_axpy3, hs_make_ext, hs_gemv_t, hs_gemv_t3, hs_gemv_n and the four reductions), each written
from the definition in the kernel's comment in numpy's longdouble, together with the first-order rounding bound of a float64
evaluation of that definition:

    |computed - exact| <= (N + k + 4) * EPS * S,     EPS = 2^-52 (twice the unit roundoff: the margin),

for a sum of N products followed by k further operations, S being the same expression evaluated on absolute values.  Whatever order a
kernel adds its N terms in (sequential, strided per thread, shuffle tree), the first-order error of the sum is at most (N - 1) u S, every
product and every further operation adds at most u S (u = 2^-53), and a fused multiply-add only removes roundings.  Every function here
returns (reference, S) as longdouble arrays; the caller multiplies S by its count of operations."""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52


def ld(a):
    return np.asarray(a, dtype=LD)


def bound(nterms, further, S):
    """the bound above as float64"""
    return np.asarray((nterms + further + 4) * LD(EPS) * ld(S), dtype=LD)


def worst_ratio(got, ref, bnd):
    """max |got - ref| / bound (0 / 0 counts as 0: an entry that is exactly right needs no room)"""
    err = np.abs(ld(got) - ld(ref))
    bnd = ld(bnd)
    r = np.where(err == 0, LD(0), err / np.where(bnd > 0, bnd, LD(1e-4000)))
    return float(np.max(r)) if r.size else 0.0


def sym(G):
    return (G + G.T) / 2


def dir_block(c, s1, X, R, E, Zinv):
    """out = s1 Zinv - X - sym((c X R + E) Zinv), E may be None; the bound is (2 n + 8) EPS S"""
    X, R, Zinv = ld(X), ld(R), ld(Zinv)
    Ee = 0 if E is None else ld(E)
    ref = LD(s1) * Zinv - X - sym((LD(c) * (X @ R) + Ee) @ Zinv)
    S = abs(LD(s1)) * np.abs(Zinv) + np.abs(X) + sym((abs(LD(c)) * (np.abs(X) @ np.abs(R)) + np.abs(Ee)) @ np.abs(Zinv))
    return ref, S


def lp_rows(Dext, v, mode, eta, sigmu, x, z, rd, elp):
    """t = Dext v; mode 0: out1 = t - z (out2 not written); mode 1: out1 = t + eta rd, out2 = sigmu / z - x - (x out1 + elp) / z.
    -> (out1, S1, out2, S2), out2 = None in mode 0.  N = m1; further operations: 1 (mode 0), 2 for out1 and 8 for out2 (mode 1: the
    two of out1, a product, a sum, two quotients, two differences)"""
    Dext, v, x, z, rd = ld(Dext), ld(v), ld(x), ld(z), ld(rd)
    t, St = Dext @ v, np.abs(Dext) @ np.abs(v)
    if mode == 0:
        return t - z, St + np.abs(z), None, None
    ee = 0 if elp is None else ld(elp)
    o1, S1 = t + LD(eta) * rd, St + abs(LD(eta)) * np.abs(rd)
    o2 = LD(sigmu) / z - x - (x * o1 + ee) / z
    S2 = abs(LD(sigmu)) / np.abs(z) + np.abs(x) + (np.abs(x) * S1 + np.abs(ee)) / np.abs(z)
    return o1, S1, o2, S2


def apply_A(As, Vs, Dext, vlp, epi, scal, vin):
    """out[i] = sum_k <A_k[i], V_k> + sum_r Dext[r][i] vlp[r]; epi 1: vout[i - 1] = out[i] - scal vin[i - 1]; epi 2: vout[i - 1] =
    vin[i - 1] scal - out[i] (i >= 1); epi 0: vout not written.  -> (out, S, vout, Sv); N = sum of the block sizes + q, 2 further
    operations for vout"""
    m1 = np.shape(As[0])[0]
    out, S = np.zeros(m1, dtype=LD), np.zeros(m1, dtype=LD)
    for A, V in zip(As, Vs):
        out = out + ld(A) @ ld(V).ravel()
        S = S + np.abs(ld(A)) @ np.abs(ld(V).ravel())
    D = ld(Dext).reshape(-1, m1)
    out = out + D.T @ ld(vlp)
    S = S + np.abs(D).T @ np.abs(ld(vlp))
    if epi == 0:
        return out, S, None, None
    vin = ld(vin)
    Sv = S[1:] + abs(LD(scal)) * np.abs(vin)
    vout = out[1:] - LD(scal) * vin if epi == 1 else vin * LD(scal) - out[1:]
    return out, S, vout, Sv


def lp_dir(sigmu, eta, x, z, r, elp):
    """out = sigmu / z - x - (eta x r + elp) / z; 7 operations"""
    x, z, r = ld(x), ld(z), ld(r)
    ee = 0 if elp is None else ld(elp)
    ref = LD(sigmu) / z - x - (LD(eta) * x * r + ee) / z
    S = abs(LD(sigmu)) / np.abs(z) + np.abs(x) + (abs(LD(eta)) * np.abs(x * r) + np.abs(ee)) / np.abs(z)
    return ref, S


def vec_mul(a, b):
    return ld(a) * ld(b), np.abs(ld(a) * ld(b))


def make_ext(s0, s1, v):
    ref = np.concatenate([[LD(s0)], LD(s1) * ld(v)])
    return ref, np.abs(ref)


def axpy(alpha, x, y):
    """y + alpha x; 2 operations"""
    return ld(y) + LD(alpha) * ld(x), np.abs(ld(y)) + abs(LD(alpha)) * np.abs(ld(x))


def gemv_t(A, E, coef, sa, add):
    """out[e] = sum_i coef[i] A[i][e] + sa add[e] over the first E entries of the rows; N = R, 2 further operations with add"""
    A = ld(A)[:, :E]
    ref, S = ld(coef) @ A, np.abs(ld(coef)) @ np.abs(A)
    if add is not None:
        ref, S = ref + LD(sa) * ld(add), S + abs(LD(sa)) * np.abs(ld(add))
    return ref, S


def gemv_n(A, E, V):
    """out[v][i] = sum_e A[i][e] V[v][e] over the first E entries of the rows"""
    A = ld(A)[:, :E]
    return ld(V) @ A.T, np.abs(ld(V)) @ np.abs(A).T


KINDS = ("dot", "absmax", "ratio_min", "lp_s0")


def reduction(kind, a, b, c):
    """one reduction -> (value, S or None when the result is exact, operations per term beyond the product).  dot: sum a b; absmax:
    max |a| (exact); ratio_min: min over b < 0 of -a / b as float64 quotients, 1e300 when there is none (exact: the minimum of
    correctly rounded quotients); lp_s0: sum (a / b) c^2 (a quotient and two products per term: 2 further operations)"""
    if kind == 0:
        return np.sum(ld(a) * ld(b)), np.sum(np.abs(ld(a) * ld(b))), 0
    if kind == 1:
        return LD(np.max(np.abs(a))), None, 0
    if kind == 2:
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        neg = b < 0
        return LD(np.min(-a[neg] / b[neg])) if neg.any() else LD(1e300), None, 0
    t = (ld(a) / ld(b)) * ld(c) * ld(c)
    return np.sum(t), np.sum(np.abs(t)), 2


def combine(kind, held, value):
    """what accumulate = 1 leaves in a slot that held `held`: the same operation"""
    if kind in (0, 3):
        return ld(held) + ld(value)
    return np.maximum(ld(held), ld(value)) if kind == 1 else np.minimum(ld(held), ld(value))


def ill_conditioned_spd(rng, m):
    """M = Q diag(1 .. 1e-12) Q^T, the matrix of tests/test_gpu_units.py::test_corrected_solves_on_an_ill_conditioned_factor"""
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = 10.0 ** (-12.0 * np.arange(m) / max(m - 1, 1))
    M = (Q * lam) @ Q.T
    return 0.5 * (M + M.T)
