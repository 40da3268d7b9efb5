"""The numpy restatement of DESIGN.md §3.16: one pair of CreateNewMapPoints'
inner loop (LocalMapping.cc:334-480), written from the specification with
numpy float32 / float64 scalars so that every operation's type and order is
on the page.  The device kernel, the host compile of orbx_triangulate.h and the
Python mirror are all held to this, bit for bit; test_triangulate_reference.py
holds this to a float64 triangulation on numpy.linalg.svd."""
import numpy as np

F, D = np.float32, np.float64

VIEW_DTYPE = np.dtype([("Tcw", "<f4", (12,)), ("Ow", "<f4", (3,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"),
                       ("cy", "<f4"), ("invfx", "<f4"), ("invfy", "<f4"), ("mbf", "<f4"), ("mb", "<f4"),
                       ("pad", "<f4")])
OBS_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("depth", "<f4"), ("raw_u", "<f4"),
                      ("raw_v", "<f4"), ("sigma2", "<f4"), ("scale", "<f4")])
PAIR_DTYPE = np.dtype([("o1", OBS_DTYPE), ("o2", OBS_DTYPE)])
POINT_DTYPE = np.dtype([("X", "<f4", (3,)), ("status", "<i4")])
assert (VIEW_DTYPE.itemsize, OBS_DTYPE.itemsize, PAIR_DTYPE.itemsize, POINT_DTYPE.itemsize) == (96, 32, 64, 16)

EPS = D(2.0) * D(np.finfo(np.float32).eps)
MAX_SWEEPS = 30
INVALID_STEREO = 9


def dot3(a, b):
    """float (a0 b0 + a1 b1) + a2 b2"""
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def dotd(a, b):
    """double products summed in order from 0.0"""
    s = D(0.0)
    for x, y in zip(a, b):
        s = s + D(x) * D(y)
    return s


def cos_stereo(mb, depth):
    hm = F(F(mb) / F(2.0))
    h, d = D(hm), D(depth)
    return F((d * d - h * h) / (d * d + h * h))


def hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(D(1.0) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(D(1.0) + a * a)
    return D(0.0)


def svd_last_row(A, slip=None):
    """vt.row(3) of the float 4x4 A (rows as given) by §3.16's one-sided Jacobi;
    returns (row (4,) float32, sweeps)"""
    A = np.asarray(A, F).reshape(4, 4)
    At = [[F(A[k][i]) for k in range(4)] for i in range(4)]
    V = [[F(1.0) if i == k else F(0.0) for k in range(4)] for i in range(4)]
    W = [dotd(At[i], At[i]) for i in range(4)]
    sweeps = 0
    while sweeps < MAX_SWEEPS:
        sweeps += 1
        changed = False
        for i, j in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            a, b = W[i], W[j]
            p = dotd(At[i], At[j])
            if abs(p) <= EPS * np.sqrt(a * b):
                continue
            p = p * D(2.0)
            beta = a - b
            gamma = hypot(p, beta)
            if beta < 0:
                delta = (gamma - beta) * D(0.5)
                s = F(np.sqrt(delta / gamma))
                c = F(p / ((gamma * D(s)) * D(2.0)))
            else:
                c = F(np.sqrt((gamma + beta) / (gamma * D(2.0))))
                s = F(p / ((gamma * D(c)) * D(2.0)))
            na = nb = D(0.0)
            for k in range(4):
                t0 = F(F(c * At[i][k]) + F(s * At[j][k]))
                t1 = F(F(F(-s) * At[i][k]) + F(c * At[j][k]))
                At[i][k], At[j][k] = t0, t1
                na = na + D(t0) * D(t0)
                nb = nb + D(t1) * D(t1)
            W[i], W[j] = na, nb
            for k in range(4):
                t0 = F(F(c * V[i][k]) + F(s * V[j][k]))
                t1 = F(F(F(-s) * V[i][k]) + F(c * V[j][k]))
                V[i][k], V[j][k] = t0, t1
            changed = True
        if not changed:
            break
    S = [np.sqrt(w) for w in W]
    for r in range(3):   # selection sort, descending, the first among equals
        mx = r
        for i in range(r + 1, 4):
            if S[mx] < S[i]:
                mx = i
        if mx != r:
            S[mx], S[r] = S[r], S[mx]
            V[mx], V[r] = V[r], V[mx]
    if slip == "vt-column":
        return np.array([V[k][3] for k in range(4)], F), sweeps
    return np.array(V[3], F), sweeps


def obs_invalid(o):
    return bool(o["ur"] >= 0) and not bool(o["depth"] > 0)


def _rows(v):
    T = [F(x) for x in v["Tcw"]]
    return [T[0:3], T[4:7], T[8:11]], [T[3], T[7], T[11]], T


def _rwc_times(R, x):
    return [dot3([R[0][i], R[1][i], R[2][i]], x) for i in range(3)]


def unproject(v, o):
    R, _, _ = _rows(v)
    z = F(o["depth"])
    x = F(F(F(o["raw_u"] - v["cx"]) * z) * v["invfx"])
    y = F(F(F(o["raw_v"] - v["cy"]) * z) * v["invfy"])
    c = _rwc_times(R, [x, y, z])
    return [F(c[i] + F(v["Ow"][i])) for i in range(3)]


def _cam(R, t, r, X):
    return F(dotd(R[r], X) + D(t[r]))


def _reproj_fails(v, o, mbf, z, X):
    R, t, _ = _rows(v)
    x, y = _cam(R, t, 0, X), _cam(R, t, 1, X)
    invz = F(D(1.0) / D(z))
    u = F(F(F(v["fx"] * x) * invz) + v["cx"])
    vv = F(F(F(v["fy"] * y) * invz) + v["cy"])
    ex, ey = F(u - o["u"]), F(vv - o["v"])
    e = F(F(ex * ex) + F(ey * ey))
    if not o["ur"] >= 0:
        return bool(D(e) > D(5.991) * D(o["sigma2"])), e
    ur = F(u - F(F(mbf) * invz))
    er = F(ur - o["ur"])
    e = F(e + F(er * er))
    return bool(D(e) > D(7.8) * D(o["sigma2"])), e


def _dist(X, Ow):
    n = [F(X[i] - F(Ow[i])) for i in range(3)]
    return F(np.sqrt(dotd(n, n)))


def pair(v1, v2, ratio_factor, o1, o2, slip=None):
    """One pair.  Returns (X (3,) float32, status, debug dict); `slip`: one of
    test_triangulate_reference.py's deliberate mistakes."""
    with np.errstate(all="ignore"):
        return _pair(v1, v2, F(ratio_factor), o1, o2, slip)


def _pair(v1, v2, ratio_factor, o1, o2, slip):
    dbg = {"sweeps": 0, "branch": None}
    zero = np.zeros(3, F)
    if obs_invalid(o1) or obs_invalid(o2):
        return zero, INVALID_STEREO, dbg
    st1, st2 = bool(o1["ur"] >= 0), bool(o2["ur"] >= 0)
    R1, t1, T1 = _rows(v1)
    R2, t2, T2 = _rows(v2)
    xn1 = [F(F(o1["u"] - v1["cx"]) * v1["invfx"]), F(F(o1["v"] - v1["cy"]) * v1["invfy"]), F(1.0)]
    xn2 = [F(F(o2["u"] - v2["cx"]) * v2["invfx"]), F(F(o2["v"] - v2["cy"]) * v2["invfy"]), F(1.0)]
    if slip == "rcw-for-rwc":
        r1, r2 = [dot3(R1[i], xn1) for i in range(3)], [dot3(R2[i], xn2) for i in range(3)]
    else:
        r1, r2 = _rwc_times(R1, xn1), _rwc_times(R2, xn2)
    cos_rays = F(dotd(r1, r2) / (np.sqrt(dotd(r1, r1)) * np.sqrt(dotd(r2, r2))))
    cs1 = cs2 = F(cos_rays + F(1.0))
    if st1:
        cs1 = cos_stereo(v1["mb"], o1["depth"])
    elif st2:
        cs2 = cos_stereo(v2["mb"], o2["depth"])
    cs = cs2 if cs2 < cs1 else cs1
    dbg.update(cos_rays=cos_rays, cs1=cs1, cs2=cs2)
    if cos_rays < cs and cos_rays > 0 and (st1 or st2 or D(cos_rays) < D(0.9998)):
        dbg["branch"] = "svd"
        A = np.zeros((4, 4), F)
        if slip == "rows-swapped":   # each camera's rows from the other camera's pose
            T1, T2 = T2, T1
        for j in range(4):
            A[0][j] = F(F(xn1[0] * T1[8 + j]) - T1[j])
            A[1][j] = F(F(xn1[1] * T1[8 + j]) - T1[4 + j])
            A[2][j] = F(F(xn2[0] * T2[8 + j]) - T2[j])
            A[3][j] = F(F(xn2[1] * T2[8 + j]) - T2[4 + j])
        dbg["A"] = A.copy()
        h, dbg["sweeps"] = svd_last_row(A, slip)
        dbg["h"] = h
        if h[3] == 0:
            return zero, 2, dbg
        alpha = F(D(1.0) / D(h[3]))
        X = [F(h[i] * alpha) for i in range(3)]
    elif st1 and cs1 < cs2:
        dbg["branch"] = "stereo1"
        X = unproject(v1, o1)
    elif st2 and cs2 < cs1:
        dbg["branch"] = "stereo2"
        X = unproject(v2, o2)
    else:
        return zero, 1, dbg
    Xa = np.array(X, F)
    z1 = _cam(R1, t1, 2, X)
    dbg["z1"] = z1
    if z1 <= 0:
        return Xa, 3, dbg
    z2 = _cam(R2, t2, 2, X)
    dbg["z2"] = z2
    if z2 <= 0:
        return Xa, 4, dbg
    bad, dbg["err1"] = _reproj_fails(v1, o1, v1["mbf"], z1, X)
    if bad:
        return Xa, 5, dbg
    bad, dbg["err2"] = _reproj_fails(v2, o2, v1["mbf"], z2, X)
    if bad:
        return Xa, 6, dbg
    d1, d2 = _dist(X, v1["Ow"]), _dist(X, v2["Ow"])
    if d1 == 0 or d2 == 0:
        return Xa, 7, dbg
    ratio_dist, ratio_octave = F(d2 / d1), F(F(o1["scale"]) / F(o2["scale"]))
    dbg.update(ratio_dist=ratio_dist, ratio_octave=ratio_octave)
    if F(ratio_dist * ratio_factor) < ratio_octave or ratio_dist > F(ratio_octave * ratio_factor):
        return Xa, 8, dbg
    return Xa, 0, dbg


def triangulate(v1, v2, ratio_factor, pairs, debug=False):
    """All pairs of one neighbour: POINT_DTYPE (n,) (and the debug dicts)"""
    v1, v2 = np.asarray(v1, VIEW_DTYPE).reshape(-1)[0], np.asarray(v2, VIEW_DTYPE).reshape(-1)[0]
    pairs = np.asarray(pairs, PAIR_DTYPE).reshape(-1)
    out, dbg = np.zeros(len(pairs), POINT_DTYPE), []
    for i, k in enumerate(pairs):
        out["X"][i], out["status"][i], d = pair(v1, v2, ratio_factor, k["o1"], k["o2"])
        dbg.append(d)
    return (out, dbg) if debug else out


def triangulate_batch(v1, v2, ratio_factor, pairs, offsets):
    v1, v2 = np.asarray(v1, VIEW_DTYPE).reshape(-1), np.asarray(v2, VIEW_DTYPE).reshape(-1)
    rf = np.broadcast_to(np.asarray(ratio_factor, F), (len(v1),))
    pairs = np.asarray(pairs, PAIR_DTYPE).reshape(-1)
    out = [triangulate(v1[p], v2[p], rf[p], pairs[offsets[p]:offsets[p + 1]]) for p in range(len(v1))]
    return np.concatenate(out) if out else np.zeros(0, POINT_DTYPE)


def has_invalid(pairs):
    pairs = np.asarray(pairs, PAIR_DTYPE).reshape(-1)
    return any(obs_invalid(k["o1"]) or obs_invalid(k["o2"]) for k in pairs)


def walk(pairs_per_neighbour, points_per_neighbour, has_point, stop_after=None):
    """CreateNewMapPoints' loop over stored results (:276-498), the literal
    way: (neighbour, idx1, idx2, X) of every point the reference would create"""
    taken = [bool(b) for b in has_point]
    out = []
    for i in range(len(pairs_per_neighbour)):
        if i > 0 and stop_after is not None and i >= stop_after:
            return out
        for (idx1, idx2), pt in zip(pairs_per_neighbour[i], points_per_neighbour[i]):
            if taken[idx1]:
                continue
            if int(pt["status"]) != 0:
                continue
            out.append((i, int(idx1), int(idx2), np.array(pt["X"], F)))
            taken[idx1] = True
    return out
