"""numpy restatement of the device Frechet distance (csrc/frechet.hip) as include/mstg_hip.h defines it, written from the definition
and independently of the kernels: float64 column means and centred, scaled factors A and B, M = A B^T, and the nuclear norm of M
either from ``numpy.linalg.svd`` (``frechet``: the float64 yardstick of the GPU tests) or from the SAME one-sided Jacobi the device
runs (``jacobi_singular_values``: same pairing, same rotation test, same formulas, so its sweep count is what
MSTG_FRECHET_MAX_SWEEPS is measured from).  ``reference_fid`` is the formula of the reference's m_test.py:37-50 written with
``np.cov`` and ``scipy.linalg.sqrtm``.
"""
import math

import numpy as np

F64 = np.float64
MAX_SAMPLES, MAX_SWEEPS = 256, 44  # MSTG_FRECHET_MAX_SAMPLES, MSTG_FRECHET_MAX_SWEEPS
EPS = float(np.finfo(F64).eps)

# (n1, n2, d) of the issue's cases; the last one sits at the sample cap
CASES = [(2, 2, 1), (7, 5, 3), (33, 64, 16), (48, 40, 13), (24, 24, 64), (100, 100, 2048), (MAX_SAMPLES, MAX_SAMPLES, 32)]
# shapes of the comparison with the sqrtm formula that the design was first checked on
SQRTM_CASES = [(48, 40, 16), (100, 100, 32), (24, 24, 64), (100, 100, 2048), (33, 64, 16), (2, 2, 4), (7, 5, 3)]


class Refused(ValueError):
    pass


def check_shape(n1, n2, d):
    """raises Refused naming the value, in the order of the C entry"""
    if n1 < 2 or n2 < 2:
        raise Refused(f"n1 = {n1}, n2 = {n2}")
    if d < 1:
        raise Refused(f"d = {d}")
    if min(n1, n2) > MAX_SAMPLES:
        raise Refused(f"min(n1, n2) = {min(n1, n2)}")


def draw(n1, n2, d, seed, dtype=np.float32, shift=0.3):
    """two seeded feature sets with different means and column scales, non-negative like pooled activations"""
    rng = np.random.RandomState(seed)
    scale = 0.5 + rng.rand(d)
    x1 = np.abs(rng.randn(n1, d)) * scale
    x2 = np.abs(rng.randn(n2, d) * 1.2 + shift) * scale
    return x1.astype(dtype), x2.astype(dtype)


def factors(x1, x2):
    """(A, B, ssdiff, tr1, tr2): everything in float64, column sums in row order"""
    x1, x2 = np.asarray(x1).astype(F64), np.asarray(x2).astype(F64)
    check_shape(x1.shape[0], x2.shape[0], x1.shape[1])
    out = []
    for x in (x1, x2):
        s = np.zeros(x.shape[1], F64)
        for row in x:
            s = s + row
        mu = s / F64(x.shape[0])
        out.append((mu, (x - mu) / math.sqrt(x.shape[0] - 1)))
    (mu1, A), (mu2, B) = out
    return A, B, float(np.sum((mu1 - mu2) ** 2)), float(np.sum(A * A)), float(np.sum(B * B))


def frechet(x1, x2):
    """{'ssdiff', 'tr1', 'tr2', 'nuclear', 'fid'} with the nuclear norm from numpy's SVD"""
    A, B, ssdiff, tr1, tr2 = factors(x1, x2)
    nuclear = float(np.linalg.svd(A @ B.T, compute_uv=False).sum())
    return {"ssdiff": ssdiff, "tr1": tr1, "tr2": tr2, "nuclear": nuclear, "fid": ((ssdiff + tr1) + tr2) - 2.0 * nuclear}


def round_robin(q):
    """the rounds of the cyclic pairing of q columns: q' = q rounded up to even, q' - 1 rounds of q' / 2 slots; slot 0 pairs the
    fixed player q' - 1 with r, slot i pairs (r + i) and (r - i) modulo q' - 1; a pair with the phantom column q (q odd) is a bye"""
    qe = q + (q & 1)
    rounds = []
    for r in range(qe - 1):
        pairs = []
        for i in range(qe // 2):
            a, b = (qe - 1, r) if i == 0 else ((r + i) % (qe - 1), (r - i + qe - 1) % (qe - 1))
            if a < q and b < q:
                pairs.append((min(a, b), max(a, b)))
        rounds.append(pairs)
    return rounds


def jacobi_singular_values(M, max_sweeps=MAX_SWEEPS):
    """(sigma descending, sweeps used, converged) of the one-sided (Hestenes) Jacobi as the header defines it"""
    M = np.asarray(M, F64)
    G = (M if M.shape[1] <= M.shape[0] else M.T).copy()  # the side with fewer columns
    p, q = G.shape
    tol = EPS * math.sqrt(float(p))
    rounds = round_robin(q)
    sweeps, converged, done = 0, q < 2, q < 2
    while not done and sweeps < max_sweeps:
        rotations = undecided = 0
        for pairs in rounds:
            for a, b in pairs:
                ga, gb = G[:, a].copy(), G[:, b].copy()
                alpha, beta, gamma = float(ga @ ga), float(gb @ gb), float(ga @ gb)
                bar = tol * (math.sqrt(alpha) * math.sqrt(beta)) if alpha >= 0 and beta >= 0 else math.nan
                if abs(gamma) <= bar:
                    continue
                if not abs(gamma) > bar:  # a NaN: no rotation can settle this pair
                    undecided += 1
                    continue
                rotations += 1
                zeta = (beta - alpha) / (2.0 * gamma)
                t = math.copysign(1.0, zeta) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta)) if math.isfinite(zeta) else 0.0
                c = 1.0 / math.sqrt(1.0 + t * t)
                s = c * t
                G[:, a] = c * ga - s * gb
                G[:, b] = s * ga + c * gb
        sweeps += 1
        done = rotations == 0  # nothing moved: another sweep would see the same pairs
        converged = done and undecided == 0
    sigma = np.sqrt(np.sum(G * G, axis=0))
    return np.sort(sigma)[::-1], sweeps, converged


def frechet_jacobi(x1, x2):
    """as ``frechet`` with the nuclear norm from the restated Jacobi; also 'sweeps' and 'converged'"""
    A, B, ssdiff, tr1, tr2 = factors(x1, x2)
    sigma, sweeps, converged = jacobi_singular_values(A @ B.T)
    nuclear = float(sigma.sum())
    return {"ssdiff": ssdiff, "tr1": tr1, "tr2": tr2, "nuclear": nuclear, "fid": ((ssdiff + tr1) + tr2) - 2.0 * nuclear,
            "sweeps": sweeps, "converged": converged}


def reference_fid(real_features, fake_features):
    """m_test.py:37-50: the means in the features' own dtype, np.cov, sqrtm of the product, the real part, the trace
    (np.atleast_2d is added for one feature, where np.cov gives a scalar and the reference's sqrtm refuses it)"""
    from scipy import linalg
    mu1, sigma1 = real_features.mean(0), np.atleast_2d(np.cov(real_features, rowvar=False))
    mu2, sigma2 = fake_features.mean(0), np.atleast_2d(np.cov(fake_features, rowvar=False))
    ssdiff = np.sum((mu1 - mu2) ** 2)
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if np.iscomplexobj(covmean):
        covmean = covmean.real
    return float(ssdiff + np.trace(sigma1 + sigma2 - 2.0 * covmean))


def workspace_doubles(n1, n2, d):
    """doubles of the C entry's workspace: A, B, three partial sums per column, M, the Jacobi's copy, sigma and the nuclear norm"""
    check_shape(n1, n2, d)
    return n1 * d + n2 * d + 3 * d + 2 * n1 * n2 + min(n1, n2) + 1
