"""numpy restatement of DESIGN.md §3.15: one Sim3Solver hypothesis
(ComputeSim3 + CheckInliers, Sim3Solver.cc:215-364) and the walk of
iterate() / find() over stored hypotheses (:140-213).  Every float step is an
np.float32 scalar or array operation (correctly rounded, unfused), every
double step a Python float; atan2, sin and cos are the math module's (the
host's libm).  Written from the specification, not from csrc/orbx_horn.h."""
import math

import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)
MAX_ROTATIONS = 4 * 4 * 30
HYP_DTYPE = np.dtype([("R", "<f4", (9,)), ("t", "<f4", (3,)), ("s", "<f4"), ("n_inliers", "<i4")])
CORR_DTYPE = np.dtype([("X1c", "<f4", (3,)), ("X2c", "<f4", (3,)), ("max_err1", "<f4"), ("max_err2", "<f4")])


def dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def jacobi4(N):
    """cv::eigen of a symmetric 4x4 float matrix: (W descending, V rows)"""
    A = [[F(N[r][c]) for c in range(4)] for r in range(4)]
    V = [[F(1) if r == c else F(0) for c in range(4)] for r in range(4)]
    half = F(0.5)
    rotations = 0
    for _ in range(MAX_ROTATIONS):
        k, l, mv = 0, 1, abs(A[0][1])
        for r in range(3):
            for c in range(r + 1, 4):
                v = abs(A[r][c])
                if mv < v:
                    mv, k, l = v, r, c
        p = A[k][l]
        if abs(p) <= EPS:
            break
        rotations += 1
        y = (A[l][l] - A[k][k]) * half
        t = abs(y) + np.sqrt(p * p + y * y)
        s = np.sqrt(p * p + t * t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        for i in range(4):
            if i == k or i == l:
                continue
            a, b = A[i][k], A[i][l]
            A[i][k] = A[k][i] = a * c - b * s
            A[i][l] = A[l][i] = a * s + b * c
        A[k][k] = A[k][k] - t
        A[l][l] = A[l][l] + t
        A[k][l] = A[l][k] = F(0)
        for i in range(4):
            a, b = V[k][i], V[l][i]
            V[k][i] = a * c - b * s
            V[l][i] = a * s + b * c
    W = [A[r][r] for r in range(4)]
    for r in range(3):
        mx = r
        for i in range(r + 1, 4):
            if W[mx] < W[i]:
                mx = i
        if mx != r:
            W[mx], W[r] = W[r], W[mx]
            V[mx], V[r] = V[r], V[mx]
    return W, V, rotations


def centroid(P):
    """P: 3 points of 3 floats.  Returns (Pr[row][point], C[row])"""
    third = F(1.0 / 3.0)
    C = [((P[0][r] + P[1][r]) + P[2][r]) * third for r in range(3)]
    Pr = [[P[i][r] - C[r] for i in range(3)] for r in range(3)]
    return Pr, C


def rodrigues(v):
    rx, ry, rz = float(v[0]), float(v[1]), float(v[2])
    theta = math.sqrt((rx * rx + ry * ry) + rz * rz)
    if theta < 2.0 ** -52:
        return [F(1) if k % 4 == 0 else F(0) for k in range(9)]
    if math.isinf(theta):
        c = s = float("nan")   # (the library's cos(inf) is NaN; math.cos raises)
    else:
        c, s = math.cos(theta), math.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    x, y, z = rx * it, ry * it, rz * it
    rrt = [x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z]
    rx_ = [0.0, -z, y, z, 0.0, -x, -y, x, 0.0]
    return [F((c * (1.0 if k % 4 == 0 else 0.0) + c1 * rrt[k]) + s * rx_[k]) for k in range(9)]


def horn(P1, P2, fix_scale, detail=None):
    """ComputeSim3 on three point pairs (P1[i], P2[i] float32 triples).
    Returns R[9], t[3], s, T12[12], T21[12] as lists of np.float32.  detail: a
    dict that receives the atan2 arguments and the rotation count."""
    with np.errstate(all="ignore"):
        P1 = [[F(x) for x in p] for p in P1]
        P2 = [[F(x) for x in p] for p in P2]
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = [[dot3(Pr2[i], Pr1[j]) for j in range(3)] for i in range(3)]
        m = [[float(M[i][j]) for j in range(3)] for i in range(3)]
        N11 = F((m[0][0] + m[1][1]) + m[2][2])
        N12 = F(m[1][2] - m[2][1])
        N13 = F(m[2][0] - m[0][2])
        N14 = F(m[0][1] - m[1][0])
        N22 = F((m[0][0] - m[1][1]) - m[2][2])
        N23 = F(m[0][1] + m[1][0])
        N24 = F(m[2][0] + m[0][2])
        N33 = F((-m[0][0] + m[1][1]) - m[2][2])
        N34 = F(m[1][2] + m[2][1])
        N44 = F((-m[0][0] - m[1][1]) + m[2][2])
        N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
        _, V, rotations = jacobi4(N)
        q0, vec = V[0][0], V[0][1:4]
        v = [float(x) for x in vec]
        nrm = math.sqrt(((0.0 + v[0] * v[0]) + v[1] * v[1]) + v[2] * v[2])
        ang = math.atan2(nrm, float(q0))
        if detail is not None:
            detail["atan2"] = (nrm, float(q0))
            detail["rotations"] = rotations
            detail["N"] = N
        inv = 1.0 / nrm if nrm != 0.0 else (float("nan") if nrm != nrm else math.inf)
        alpha = F((2.0 * ang) * inv)
        vec = [x * alpha for x in vec]
        R = rodrigues(vec)
        P3 = [[dot3(R[3 * i:3 * i + 3], [Pr2[0][j], Pr2[1][j], Pr2[2][j]]) for j in range(3)] for i in range(3)]
        if not fix_scale:
            nom = den = 0.0
            for i in range(3):
                for j in range(3):
                    nom += float(Pr1[i][j]) * float(P3[i][j])
                    den += float(P3[i][j] * P3[i][j])
            s = F(np.float64(nom) / np.float64(den))
        else:
            s = F(1.0)
        t = [O1[i] - s * dot3(R[3 * i:3 * i + 3], O2) for i in range(3)]
        sinv = F(np.float64(1.0) / np.float64(s))
        sRinv = [sinv * R[3 * j + i] for i in range(3) for j in range(3)]
        T12, T21 = [], []
        for i in range(3):
            T12 += [s * R[3 * i + j] for j in range(3)] + [t[i]]
            T21 += sRinv[3 * i:3 * i + 3] + [-dot3(sRinv[3 * i:3 * i + 3], t)]
        return R, t, s, T12, T21


def own_projection(X, cam):
    """FromCameraToImage over an (n, 3) float32 array"""
    with np.errstate(all="ignore"):
        invz = F(1) / X[:, 2]
        x, y = X[:, 0] * invz, X[:, 1] * invz
        return F(cam["fx"]) * x + F(cam["cx"]), F(cam["fy"]) * y + F(cam["cy"])


def project(T, X, cam):
    """Project over an (n, 3) float32 array; T: 12 floats, rows of four"""
    with np.errstate(all="ignore"):
        c = [((T[4 * i] * X[:, 0] + T[4 * i + 1] * X[:, 1]) + T[4 * i + 2] * X[:, 2]) + T[4 * i + 3] for i in range(3)]
        invz = F(1) / c[2]
        x, y = c[0] * invz, c[1] * invz
        return F(cam["fx"]) * x + F(cam["cx"]), F(cam["fy"]) * y + F(cam["cy"])


def err(dx, dy):
    d = dx.astype(np.float64), dy.astype(np.float64)
    with np.errstate(all="ignore"):
        return ((0.0 + d[0] * d[0]) + d[1] * d[1]).astype(np.float32)


def errors(T12, T21, corr, cam1, cam2):
    """(err1, err2) of every correspondence under one hypothesis"""
    X1, X2 = np.ascontiguousarray(corr["X1c"]), np.ascontiguousarray(corr["X2c"])
    u1o, v1o = own_projection(X1, cam1)
    u2o, v2o = own_projection(X2, cam2)
    u21, v21 = project(T12, X2, cam1)
    u12, v12 = project(T21, X1, cam2)
    with np.errstate(all="ignore"):
        return err(u1o - u21, v1o - v21), err(u12 - u2o, v12 - v2o)


def check_inliers(T12, T21, corr, cam1, cam2):
    e1, e2 = errors(T12, T21, corr, cam1, cam2)
    with np.errstate(all="ignore"):
        return (e1 < corr["max_err1"]) & (e2 < corr["max_err2"])


def mask_words(inl):
    n = len(inl)
    words = np.zeros((n + 63) // 64, np.uint64)
    for i in np.nonzero(inl)[0]:
        words[i >> 6] |= np.uint64(1) << np.uint64(i & 63)
    return words


def hypothesis(cam1, cam2, fix_scale, corr, triple, detail=None):
    """One hypothesis: (HYP_DTYPE record, inlier bools (n,))"""
    a, b, c = (int(i) for i in triple)
    R, t, s, T12, T21 = horn([corr["X1c"][a], corr["X1c"][b], corr["X1c"][c]],
                             [corr["X2c"][a], corr["X2c"][b], corr["X2c"][c]], fix_scale, detail)
    inl = check_inliers(T12, T21, corr, cam1, cam2)
    if detail is not None:
        detail["T12"], detail["T21"] = T12, T21
    rec = np.zeros(1, HYP_DTYPE)
    rec["R"][0], rec["t"][0], rec["s"][0], rec["n_inliers"][0] = R, t, s, int(inl.sum())
    return rec, inl


def ransac(cam1, cam2, fix_scale, corr, triples, details=None):
    """All hypotheses of one solver: (hyp (h,) HYP_DTYPE, mask (h, ceil(n/64)) uint64)"""
    h, n = len(triples), len(corr)
    hyp = np.zeros(h, HYP_DTYPE)
    mask = np.zeros((h, (n + 63) // 64), np.uint64)
    for k in range(h):
        d = {} if details is not None else None
        rec, inl = hypothesis(cam1[0], cam2[0], fix_scale, corr, triples[k], d)
        hyp[k] = rec[0]
        mask[k] = mask_words(inl)
        if details is not None:
            details.append(d)
    return hyp, mask


def ransac_iterations(N, probability=0.99, min_inliers=6, max_iterations=300):
    """SetRansacParameters' mRansacMaxIts (:114-138): float epsilon, the
    N == minInliers case, max(1, min(., .))"""
    with np.errstate(all="ignore"):
        eps = F(min_inliers) / F(N)
        if min_inliers == N:
            nit = 1
        else:
            den = np.log(np.float64(1) - np.float64(math.pow(float(eps), 3.0)))   # pow(float, int) is double
            v = np.ceil(np.log(np.float64(1 - probability)) / den)
            # (int)ceil(...) of a NaN or an out-of-range double is INT_MIN on x86-64
            nit = int(v) if np.isfinite(v) and abs(v) < 2 ** 31 else -2 ** 31
    return max(1, min(nit, max_iterations))


class Walk:
    """iterate() / find() over stored hypotheses, written as the reference's
    loop (:140-213) with ComputeSim3 + CheckInliers replaced by a lookup"""

    def __init__(self, N, mN1, indices1, hyp, mask, min_inliers=6, max_its=300):
        self.N, self.mN1, self.indices1 = N, mN1, list(indices1)
        self.hyp, self.mask = hyp, mask
        self.min_inliers, self.max_its = min_inliers, max_its
        self.iterations, self.best_inliers, self.best = 0, 0, None

    def iterate(self, n_iterations):
        """Returns (index of the returned hypothesis or None, bNoMore, vbInliers, nInliers)"""
        no_more, vb, n_inl = False, [False] * self.mN1, 0
        if self.N < self.min_inliers:
            return None, True, vb, 0
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            k = self.iterations
            self.iterations += 1
            count = int(self.hyp["n_inliers"][k])
            if count >= self.best_inliers:
                self.best, self.best_inliers = k, count
                if count > self.min_inliers:
                    n_inl = count
                    for i in range(self.N):
                        if (int(self.mask[k][i >> 6]) >> (i & 63)) & 1:
                            vb[self.indices1[i]] = True
                    return k, no_more, vb, n_inl
        if self.iterations >= self.max_its:
            no_more = True
        return None, no_more, vb, n_inl

    def find(self):
        k, _, vb, n_inl = self.iterate(self.max_its)
        return k, vb, n_inl
