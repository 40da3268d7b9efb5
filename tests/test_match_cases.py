"""The constructed matcher cases (match_cases.py) on the CPU.

Reach: every edge a case is named for is counted from the definitions with
numpy (popcount distances, the float comparisons written out, the cell
arithmetic) or, where it depends on the greedy state, from the trace of
pyref's in-order loop, and must be reached at least once.  The oracle's
matcher is not used for this.  A case that stops reaching its edge fails
here rather than passing silently on the GPU.

Expectation: where a case states the outcome it was built for, pyref gives it.

Agreement: oracle == pyref, field by field, on every case.

What the agreement test catches, checked by changing the oracle one comparison
at a time (the change: a case that then fails; * = an earlier CPU test failed too):
  '<=' <-> '<' at TH_LOW / TH_HIGH: init *init-ratio0.9, localmap thresholds100-localmap,
    best-only *thresholds50-bounds-fuse, sim3 sim3-agreement, kf_frame thresholds-kf_frame,
    kf_kf thresholds-kf_kf (also the two swapped), triangulation thresholds-triangulation
  ratio '<' -> '<=' / '>' -> '>=': init-ratio0.6, ratio0.75-kf_frame, ratio0.6-localmap
  ratio product in double: init-ratio0.6, ratio0.6-kf_kf, ratio0.9-localmap
  window '<' -> '<=': *init-window-grid, window-keyframe
  PosInGrid round -> rint, x and y: init-window-grid, grid-keyframe, grid-bounds-keyframe
  rotation bin round -> rint: init-rot-half, rot-half-lastframe, rot-half-triangulation, rot-half-kf_kf
  mvuRight '> 0' <-> '>= 0': *stereo-localmap, *stereo-lastframe, *chi2-fuse
  '> ur_tol' -> '>=': stereo-localmap, stereo-lastframe
  first <-> last minimum: init-ties-steal, ratio1.0-localmap, grid-bounds-keyframe, sim3-agreement,
    ties-kf_frame, ties-triangulation; an equal distance stealing: init-ties-steal
  ComputeThreeMaxima 's > max' -> '>=': init-rot-tie, rot-tie-keyframe
  '< 0.1f * max1' -> '<=' (second and third): init-rot-tenth10, rot-tenth10-keyframe
  epipole gate with one side stereo *, and its '<' -> '<=': tri-gates-triangulation
"""
import numpy as np
import pytest

import match_cases as mc
import pyref

f32 = np.float32
CASES = mc.all_cases()
NAMES = list(CASES)
_RUNS = {}


def run_pyref(c, check_ori=None):
    ori = c.get("check_ori", False) if check_ori is None else check_ori
    key = (c["name"], ori)
    if key in _RUNS:
        return _RUNS[key]
    trace = []
    if c["family"] == "proj":
        r = pyref.search_by_projection(c["variant"], c["keys"], c["desc"], c["queries"], c["qdesc"], c["bounds"],
                                       c["uright"], c["mp_state"], c["inv_sigma2"], c["th_dist"], c["nnratio"], ori,
                                       trace=trace)
    elif c["family"] == "bow":
        r = pyref.search_by_bow(c["variant"], c["A"], c["B"], c["nnratio"], ori, c["tri"])
    elif c["family"] == "sim3":
        k1, k2 = c["kf1"], c["kf2"]
        r = pyref.search_by_sim3(k1["keys"], k1["desc"], k1["bounds"], k2["keys"], k2["desc"], k2["bounds"], c["q1"],
                                 c["qd1"], c["q2"], c["qd2"], c["th_dist"], trace=trace)
    else:
        r = pyref.search_for_initialization(c["k1"], c["d1"], c["k2"], c["d2"], mc.W, mc.H, c["prev"], c["window"],
                                            c["nnratio"], ori, bounds=c["bounds"], trace=trace)
    _RUNS[key] = (r, trace)
    return _RUNS[key]


def run_oracle(c, oracle):
    if c["family"] == "proj":
        return oracle.search_by_projection(c["variant"], c["keys"], c["desc"], c["queries"], c["qdesc"], c["bounds"],
                                           c["uright"], c["mp_state"], c["inv_sigma2"], c["th_dist"], c["nnratio"],
                                           c["check_ori"])
    if c["family"] == "bow":
        return oracle.search_by_bow(c["variant"], c["A"], c["B"], c["nnratio"], c["check_ori"], c["tri"])
    if c["family"] == "sim3":
        k1, k2 = c["kf1"], c["kf2"]
        return oracle.search_by_sim3(k1["keys"], k1["desc"], k1["bounds"], k2["keys"], k2["desc"], k2["bounds"],
                                     c["q1"], c["qd1"], c["q2"], c["qd2"], c["th_dist"])
    return oracle.search_for_initialization(c["k1"], c["d1"], c["k2"], c["d2"], mc.W, mc.H, c["prev"], c["window"],
                                            c["nnratio"], c["check_ori"], bounds=c["bounds"])


FIELDS = {"proj": ("nmatches", "q_idx", "q_dist", "kp_final"), "bow": ("nmatches", "match_a", "match_b"),
          "init": ("nmatches", "matches12", "prev"), "sim3": ("nfound", "matches12")}


def assert_same(c, got, want, who):
    for name, x, y in zip(FIELDS[c["family"]], got, want):
        x, y = np.asarray(x), np.asarray(y)
        bad = np.nonzero(np.atleast_1d(x != y))[0]
        assert len(bad) == 0, f"{c['name']}: {who} {name} differs at {bad[:6]}: {np.atleast_1d(x)[bad[:6]]} vs " \
                              f"{np.atleast_1d(y)[bad[:6]]}"


# ---- definitions, in numpy ---------------------------------------------------------------------------
def popcount(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(2).astype(np.int64)


def rha(v):
    """round(), half away from zero, of float32 values (exact in double)."""
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), -np.floor(-v + 0.5)).astype(np.int64)


def frac_half(v):
    v = np.abs(np.asarray(v, np.float32).astype(np.float64))
    return v - np.floor(v) == 0.5


def geometry(c):
    """Cell coordinates, cell ranges, windows: Frame.cc:354-425 in float32."""
    k, q = c["keys"], c["queries"]
    mnx, mxx, mny, mxy = [f32(b) for b in c["bounds"]]
    invw, invh = f32(64) / f32(mxx - mnx), f32(48) / f32(mxy - mny)
    fx, fy = (k["x"] - mnx) * invw, (k["y"] - mny) * invh
    cx, cy = rha(fx), rha(fy)
    ingrid = (cx >= 0) & (cx < 64) & (cy >= 0) & (cy < 48)
    u0, v0, r = q["u"] - mnx, q["v"] - mny, q["radius"]
    c0, c1 = np.floor((u0 - r) * invw).astype(np.int64), np.ceil((u0 + r) * invw).astype(np.int64)
    r0, r1 = np.floor((v0 - r) * invh).astype(np.int64), np.ceil((v0 + r) * invh).astype(np.int64)
    empty = (c0 >= 64) | (c1 < 0) | (r0 >= 48) | (r1 < 0)
    inrange = ingrid[None] & ~empty[:, None] & (cx[None] >= c0[:, None]) & (cx[None] <= c1[:, None]) & \
        (cy[None] >= r0[:, None]) & (cy[None] <= r1[:, None]) & ((q["flags"] & 1) != 0)[:, None]
    dx = np.abs(k["x"][None] - q["u"][:, None])
    dy = np.abs(k["y"][None] - q["v"][:, None])
    rr = r[:, None]
    octv = k["octave"][None]
    mn, mx = q["min_level"][:, None], q["max_level"][:, None]
    lvl = ~((mn > 0) | (mx >= 0)) | ((octv >= mn) & ((mx < 0) | (octv <= mx)))
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, c0=c0, c1=c1, r0=r0, r1=r1, empty=empty, inrange=inrange, dx=dx, dy=dy,
                r=rr, win=(dx < rr) & (dy < rr), lvl=lvl, cand=inrange & (dx < rr) & (dy < rr) & lvl)


def static_proj(c):
    """Per query: distances of its static candidates in area order (column,
    row, index), from the definitions."""
    g = geometry(c)
    D = popcount(c["qdesc"], c["desc"])
    order = np.lexsort((np.arange(len(g["cx"])), g["cy"], g["cx"]))
    lists = []
    for iq in range(len(c["queries"])):
        idx = order[g["cand"][iq][order]]
        lists.append((idx, D[iq, idx]))
    return g, D, lists


def best_two(d):
    """(best, second, position of best, position of second) as the reference's
    strict '<' scan leaves them (ORBmatcher.cc:98-112)."""
    b = b2 = 256
    p = p2 = -1
    for i, v in enumerate(d):
        if v < b:
            b2, p2, b, p = b, p, int(v), i
        elif v < b2:
            b2, p2 = int(v), i
    return b, b2, p, p2


def rotations(c):
    """Rotation (float32) of every pair matched before the rotation check."""
    (r, _) = run_pyref(c, check_ori=False)
    if c["family"] == "proj":
        qa, ka, m = c["queries"]["angle"], c["keys"]["angle"], r[1]
    elif c["family"] == "bow":
        qa, ka, m = c["A"]["keys"]["angle"], c["B"]["keys"]["angle"], r[1]
    else:
        qa, ka, m = c["k1"]["angle"], c["k2"]["angle"], r[1]
    sel = np.nonzero(m >= 0)[0]
    raw = (qa[sel] - ka[m[sel]]).astype(np.float32)
    rot = np.where(raw < 0, raw + f32(360), raw).astype(np.float32)
    return raw, rot, (rot * (f32(1) / f32(30))).astype(np.float32)


def histo(c):
    _, _, b = rotations(c)
    bins = rha(b)
    bins[bins == 30] = 0
    return np.sort(np.bincount(bins, minlength=30))[::-1]


def bow_static(c):
    """Per A feature in a shared node: (i1, B candidates in node order, distances)."""
    A, B, v = c["A"], c["B"], c["variant"]
    nb = {int(n): j for j, n in enumerate(B["ids"])}
    out = []
    for i, n in enumerate(A["ids"]):
        if int(n) not in nb:
            continue
        j = nb[int(n)]
        fb = B["feat"][B["off"][j]:B["off"][j + 1]]
        if v != "kf_frame":
            fb = fb[(B["flags"][fb] & 1) != 0]
        for i1 in A["feat"][A["off"][i]:A["off"][i + 1]]:
            if A["flags"][i1] & 1:
                out.append((int(i1), fb, popcount(A["desc"][i1:i1 + 1], B["desc"][fb])[0]))
    return out


def candidate_dists(c):
    """A list of distance arrays, one per query / feature with candidates."""
    if c["family"] == "proj":
        return [d for _, d in static_proj(c)[2] if len(d)]
    if c["family"] == "bow":
        return [d for _, _, d in bow_static(c) if len(d)]
    if c["family"] == "sim3":
        g = geometry(dict(keys=c["kf2"]["keys"], queries=c["q1"], bounds=c["kf2"]["bounds"]))
        D = popcount(c["qd1"], c["kf2"]["desc"])
        return [D[i][g["cand"][i]] for i in range(len(c["q1"])) if g["cand"][i].any()]
    _, trace = run_pyref(c)
    return [np.array([s[1] for s in t[1]]) for t in trace if t[0] != "steal"]


def ratio_eq(c):
    r, n = f32(c["nnratio"]), 0
    for d in candidate_dists(c):
        b, b2, _, _ = best_two(d)
        n += len(d) >= 2 and f32(b) == f32(r * f32(b2))
    return n


def n_best(c, value):
    return sum(int(d.min()) == value for d in candidate_dists(c))


def side_counts(*counts):
    return min(int(x) for x in counts)


def reach(c, edge):
    fam = c["family"]
    th = c.get("th_dist", 50)
    if edge.startswith("best=="):
        what = edge[6:]
        value = {"th": th, "th+1": th + 1, "th-1": th - 1}.get(what)
        return n_best(c, int(what) if value is None else value)
    if edge == "second==256":
        return sum(len(d) >= 2 and np.sort(d)[1] == 256 for d in candidate_dists(c))
    if edge == "ratio==":
        return ratio_eq(c)
    if edge == "single-candidate":
        return sum(len(d) == 1 for d in candidate_dists(c))
    if edge == "tie-at-best":
        return sum((d == d.min()).sum() >= 2 for d in candidate_dists(c))
    if edge in ("rot-half-bin", "rot-wrap", "rot-near-360"):
        raw, rot, b = rotations(c)
        return int({"rot-half-bin": frac_half(b).sum(), "rot-wrap": (raw < 0).sum(), "rot-near-360": (rot > 359).sum()}[edge])
    if edge.startswith("histo-"):
        h = histo(c)
        tenth = f32(0.1) * f32(h[0])
        return int({"histo-tie": h[2] == h[3] and h[3] > 0, "histo-tenth==": f32(h[1]) == tenth,
                    "histo-tenth<": 0 < f32(h[1]) < tenth, "histo-third==": f32(h[2]) == tenth and f32(h[1]) > tenth,
                    "histo-two-bins": (h > 0).sum() == 2}[edge])
    if fam == "sim3":
        return reach_sim3(c, edge)
    if fam == "proj":
        return reach_proj(c, edge)
    if fam == "bow":
        return reach_bow(c, edge)
    return reach_init(c, edge)


def reach_proj(c, edge):
    g, D, lists = static_proj(c)
    k, q, th = c["keys"], c["queries"], c["th_dist"]
    (res, trace) = run_pyref(c)
    r = g["r"]
    if edge == "ratio-fail-other-octave":
        n = 0
        for idx, d in lists:
            b, b2, p, p2 = best_two(d)
            n += p2 >= 0 and f32(b) > f32(f32(c["nnratio"]) * f32(b2)) and k["octave"][idx[p]] != k["octave"][idx[p2]]
        return n
    if edge == "|dx|==r":
        return int((g["inrange"] & (g["dx"] == r) & (g["dy"] < r) & (r > 0)).sum())
    if edge == "|dy|==r":
        return int((g["inrange"] & (g["dy"] == r) & (g["dx"] < r) & (r > 0)).sum())
    if edge == "next-inside":
        # the keypoint at the float next to u + r (u - r) on the window's side
        u, v, inf = q["u"][:, None], q["v"][:, None], f32(np.inf)
        return side_counts((g["cand"] & (k["x"][None] == np.nextafter(u + r, -inf))).sum(),
                           (g["cand"] & (k["x"][None] == np.nextafter(u - r, inf))).sum(),
                           (g["cand"] & (k["y"][None] == np.nextafter(v + r, -inf))).sum(),
                           (g["cand"] & (k["y"][None] == np.nextafter(v - r, inf))).sum())
    if edge == "radius0":
        return int((g["inrange"] & (r == 0) & (g["dx"] == 0) & (g["dy"] == 0)).sum())
    if edge == "clamp-each-side":
        ne = ~g["empty"]
        return side_counts((ne & (g["c0"] < 0)).sum(), (ne & (g["c1"] > 63)).sum(), (ne & (g["r0"] < 0)).sum(),
                           (ne & (g["r1"] > 47)).sum())
    if edge == "empty-range":
        return side_counts((g["c0"] >= 64).sum(), (g["c1"] < 0).sum(), (g["r0"] >= 48).sum(), (g["r1"] < 0).sum())
    if edge == "all-columns":
        return int(((g["c0"] <= 0) & (g["c1"] >= 63)).sum())
    if edge == "cell==-.5":
        return side_counts((g["fx"] == f32(-0.5)).sum(), (g["fy"] == f32(-0.5)).sum())
    if edge == "cell==k+.5":
        return side_counts((frac_half(g["fx"]) & (g["fx"] > 0) & (g["cx"] < 64)).sum(),
                           (frac_half(g["fy"]) & (g["fy"] > 0) & (g["cy"] < 48)).sum())
    if edge in ("on-max", "under-max"):
        mxx, mxy = f32(c["bounds"][1]), f32(c["bounds"][3])
        if edge == "under-max":
            mxx, mxy = mc.below(mxx), mc.below(mxy)
        return side_counts((k["x"] == mxx).sum(), (k["y"] == mxy).sum())
    if edge == "nonzero-bounds":
        b = np.array(c["bounds"])
        return int((b != np.round(b)).all()) * int(g["cand"].sum())
    inwin = g["inrange"] & g["win"]
    mn, mx, octv = q["min_level"][:, None], q["max_level"][:, None], k["octave"][None]
    if edge == "no-check":
        return int((inwin & (mn == 0) & (mx == -1)).sum())
    if edge == "min-only":
        return int((inwin & (mn > 0) & (mx < 0)).sum())
    if edge == "octave==min":
        return int((inwin & (mn > 0) & (octv == mn)).sum())
    if edge == "octave==max":
        return int((inwin & (mx >= 0) & (octv == mx)).sum())
    if edge == "octave-outside":
        return side_counts((inwin & (octv < mn)).sum(), (inwin & (mx >= 0) & (octv > mx)).sum())
    if edge in ("uright==0", "|er|==tol", "|er|>tol"):
        ur = c["uright"][None]
        er = np.abs(q["ur"][:, None] - ur)
        tol = q["ur_tol"][:, None]
        return int((g["cand"] & {"uright==0": (ur == 0) & (er > tol), "|er|==tol": (ur > 0) & (er == tol),
                                 "|er|>tol": (ur > 0) & (er > tol) & (er < tol + f32(1e-5))}[edge]).sum())
    if edge in ("tie-across-columns", "tie-across-rows"):
        n = 0
        for idx, d in lists:
            at = idx[d == d.min()] if len(d) else []
            if len(at) >= 2:
                first, other = at[0], at[1:]
                later = other[other < first]       # a lower index that comes later in area order
                if edge == "tie-across-columns":
                    n += int((g["cx"][later] > g["cx"][first]).any())
                else:
                    n += int(((g["cx"][later] == g["cx"][first]) & (g["cy"][later] > g["cy"][first])).any())
        return n
    if edge.startswith("within-th=="):
        want = int(edge[11:])
        return sum(int((d <= th).sum()) == want for _, d in lists)
    if edge == "taken-seen":
        return sum(1 for _, seen in trace for (_, d, free) in seen if not free and d <= th)
    if edge == "chain>64":
        # query i's best static candidate went to query i - 1
        chain = best = 0
        for iq in range(1, len(q)):
            idx, d = lists[iq]
            linked = len(d) and res[1][iq - 1] == idx[int(np.argmin(d))] and res[1][iq] >= 0
            chain = chain + 1 if linked else 0
            best = max(best, chain)
        return best - 64
    if edge == "full-list>512":
        taken = (c["mp_state"] & 3) == 3 if c["variant"] in ("localmap", "lastframe") else (c["mp_state"] & 1) != 0
        n = 0
        for idx, d in lists:
            four = idx[np.argsort(d, kind="stable")[:4]]
            n += len(d) > 4 and taken[four].all()
        return n - 512
    if edge == "hard>cap":
        blocks = (q["flags"] & 2) != 0 if c["variant"] in ("localmap", "lastframe") else np.ones(len(q), bool)
        claims = sum(int((d <= th).sum()) for (_, d), b in zip(lists, blocks) if b and (d <= th).sum() > 4)
        return claims - (4 * len(q) + 4096)
    if edge.startswith("list=="):
        return int((g["inrange"].sum(1) == int(edge[6:])).sum())
    if edge == "nonblocking-retaken":
        n = 0
        for iq in np.nonzero((q["flags"] & 2) == 0)[0]:
            n += res[1][iq] >= 0 and (res[1][iq + 1:] == res[1][iq]).any()
        return n
    if edge.startswith("fuse-") and edge != "fuse-min-late" or edge.startswith("chi2-"):
        ur = c["uright"][None]
        ex, ey, er = q["u"][:, None] - k["x"][None], q["v"][:, None] - k["y"][None], q["ur"][:, None] - ur
        isg = c["inv_sigma2"][k["octave"]][None]
        two = ((ex * ex + ey * ey) * isg).astype(np.float32)
        three = ((ex * ex + ey * ey + er * er) * isg).astype(np.float32)
        cand, st = g["cand"], ur >= 0
        if edge == "fuse-uright==0":     # stereo by '>= 0': the 3-term form rejects what the 2-term form keeps
            return int((cand & (ur == 0) & (three.astype(np.float64) > 7.8) & (two.astype(np.float64) <= 5.99)).sum())
        if edge == "fuse-mono":
            return int((cand & ~st & (three.astype(np.float64) > 7.8) & (two.astype(np.float64) <= 5.99)).sum())
        limit = float(edge.split("-")[1])
        lo, hi = mc.chi2_neighbours(limit)
        chi, branch = (three, st) if limit == 7.8 else (two, ~st)
        return int((cand & branch & (chi == (lo if edge.endswith("-inside") else hi))).sum())
    if edge == "fuse-min-late":
        return sum(len(d) > 4 and int(np.argmin(d)) >= 4 for _, d in lists)
    raise KeyError(edge)


def reach_sim3(c, edge):
    (_, trace) = run_pyref(c)
    m1, m2 = trace[0]
    side = dict(keys=c["kf2"]["keys"], queries=c["q1"], bounds=c["kf2"]["bounds"])      # KF1's points in KF2
    g = geometry(side)
    D = popcount(c["qd1"], c["kf2"]["desc"])
    if edge == "sim3-nonreciprocal":
        return sum(a >= 0 and m2[a] != i for i, a in enumerate(m1))
    if edge in ("sim3-best==th", "sim3-best==th+1"):
        want = c["th_dist"] + (edge.endswith("+1"))
        return sum(g["cand"][i].any() and D[i][g["cand"][i]].min() == want for i in range(len(m1)))
    if edge == "sim3-octave-outside":
        return int((g["inrange"] & g["win"] & ~g["lvl"]).sum())
    if edge == "sim3-one-side-skipped":
        return int(((c["q1"]["flags"] & 1) == 0).sum())
    raise KeyError(edge)


def tri_pairs(c):
    """Per (A feature, B feature) of a shared node, in float32 as the reference
    (ORBmatcher.cc:716-734, CheckDistEpipolarLine :130-158): both monocular,
    squared epipole distance, its limit, den, dsqr, its limit."""
    A, B, t = c["A"], c["B"], c["tri"]
    F, ex, ey, scale, sigma2 = t[:9], t[9], t[10], t[11:19], t[19:27]
    rows = []
    for i1, fb, _ in bow_static(c):
        x1, y1 = A["keys"]["x"][i1], A["keys"]["y"][i1]
        a = f32(f32(f32(x1 * F[0]) + f32(y1 * F[3])) + F[6])
        b = f32(f32(f32(x1 * F[1]) + f32(y1 * F[4])) + F[7])
        cc = f32(f32(f32(x1 * F[2]) + f32(y1 * F[5])) + F[8])
        for i2 in fb:
            k2 = B["keys"][i2]
            dx, dy = f32(ex - k2["x"]), f32(ey - k2["y"])
            num = f32(f32(f32(a * k2["x"]) + f32(b * k2["y"])) + cc)
            den = f32(f32(a * a) + f32(b * b))
            rows.append(dict(mono=not (A["flags"][i1] & 2) and not (B["flags"][i2] & 2),
                             epi=f32(f32(dx * dx) + f32(dy * dy)),
                             epi_lim=f32(f32(100) * scale[k2["octave"]]) if 0 <= k2["octave"] < 8 else f32(0),
                             den=den, dsqr=f32(f32(num * num) / den) if den != 0 else None,
                             lim=3.84 * float(sigma2[k2["octave"]]) if 0 <= k2["octave"] < 8 else 0.0))
    return rows


def reach_bow(c, edge):
    A, B = c["A"], c["B"]
    if edge == "tri-octave-outside":
        oct_b = B["keys"]["octave"]
        return side_counts((oct_b < 0).sum(), (oct_b >= 8).sum())
    if edge in ("epipole-gate-mono", "epipole-gate-stereo", "epipole==limit", "dsqr-inside", "dsqr-outside", "den==0"):
        rows = tri_pairs(c)
        return sum({"epipole-gate-mono": r["mono"] and r["epi"] < r["epi_lim"],
                    "epipole-gate-stereo": not r["mono"] and r["epi"] < r["epi_lim"],
                    "epipole==limit": r["mono"] and r["epi"] == r["epi_lim"],
                    "dsqr-inside": r["dsqr"] is not None and 0 < r["lim"] - float(r["dsqr"]) < 1e-4,
                    "dsqr-outside": r["dsqr"] is not None and r["lim"] > 0 and 0 <= float(r["dsqr"]) - r["lim"] < 1e-4,
                    "den==0": r["den"] == 0}[edge] for r in rows)
    if edge == "b-flag-clear":
        n = 0
        nb = {int(x): j for j, x in enumerate(B["ids"])}
        for i, x in enumerate(A["ids"]):
            if int(x) in nb:
                fb = B["feat"][B["off"][nb[int(x)]]:B["off"][nb[int(x)] + 1]]
                for i1 in A["feat"][A["off"][i]:A["off"][i + 1]]:
                    d = popcount(A["desc"][i1:i1 + 1], B["desc"][fb])[0]
                    n += not (B["flags"][fb[int(np.argmin(d))]] & 1)
        return n
    if edge.startswith("ids==") or edge.startswith("id-"):
        a, b = [int(x) for x in A["ids"]], [int(x) for x in B["ids"]]
        if edge.startswith("ids=="):
            return int(len(b) == int(edge[5:]))
        if edge == "id-first":
            return int(b[0] in a)
        if edge == "id-last":
            return int(b[-1] in a)
        absent = [x for x in a if x not in set(b)]
        between = sum(b[0] < x < b[-1] for x in absent) if len(b) > 1 else 1
        return side_counts(sum(x < b[0] for x in absent), between, sum(x > b[-1] for x in absent))
    if edge == "one-sided-node":
        a, b = set(A["ids"].tolist()), set(B["ids"].tolist())
        return side_counts(len(a - b), len(b - a))
    if edge == "node-sizes":
        nb = {int(x): j for j, x in enumerate(B["ids"])}
        seen = set()
        for i, x in enumerate(A["ids"]):
            if int(x) in nb:
                j = nb[int(x)]
                seen.add((int(A["off"][i + 1] - A["off"][i]), int(B["off"][j + 1] - B["off"][j])))
        sizes = (1, 63, 64, 65, 129)
        return sum((a, b) in seen for a in sizes for b in sizes) - 24
    raise KeyError(edge)


def reach_init(c, edge):
    _, trace = run_pyref(c)
    if edge.startswith("init-"):
        k2, prev, r = c["k2"], c["prev"], f32(c["window"])
        dx, dy = np.abs(k2["x"][None] - prev[:, 0:1]), np.abs(k2["y"][None] - prev[:, 1:2])
        fx, fy = k2["x"] * (f32(64) / f32(mc.W)), k2["y"] * (f32(48) / f32(mc.H))
        inf = f32(np.inf)
        if edge == "init-|d|==r":
            return side_counts(((dx == r) & (dy < r)).sum(), ((dy == r) & (dx < r)).sum())
        if edge == "init-next-inside":
            return side_counts(((dy < r) & (k2["x"][None] == np.nextafter(prev[:, 0:1] + r, -inf))).sum(),
                               ((dy < r) & (k2["x"][None] == np.nextafter(prev[:, 0:1] - r, inf))).sum(),
                               ((dx < r) & (k2["y"][None] == np.nextafter(prev[:, 1:2] + r, -inf))).sum(),
                               ((dx < r) & (k2["y"][None] == np.nextafter(prev[:, 1:2] - r, inf))).sum())
        near = ((dx < r) & (dy < r)).any(0)
        if edge == "init-cell==-.5":
            return side_counts((near & (fx == f32(-0.5))).sum(), (near & (fy == f32(-0.5))).sum())
        if edge == "init-cell==k+.5":
            return int((near & (fx > 0) & frac_half(fx)).sum())
    if edge == "steal":
        return sum(t[0] == "steal" for t in trace)
    if edge == "full-list-walk":
        # fewer than two of the four smallest (distance, position) entries are open (vMatchedDistance > dist)
        # at the query's turn, and an entry past them is
        n = 0
        for t in trace:
            if t[0] == "steal" or len(t[1]) <= 4:
                continue
            order = sorted(range(len(t[1])), key=lambda p: (t[1][p][1], p))
            is_open = [t[1][p][2] > t[1][p][1] for p in order]
            n += sum(is_open[:4]) < 2 and any(is_open[4:])
        return n
    if edge in ("steal-within-64", "steal-beyond-64"):
        # distance, in live queries (best distance <= TH_LOW: the ones the replay batches), from victim to stealer
        rank, n = {}, 0
        for t in trace:
            if t[0] == "steal":
                gap = rank[t[1]] - rank[t[2]]
                n += gap < 64 if edge == "steal-within-64" else gap >= 64
            elif min(e[1] for e in t[1]) <= 50:
                rank[t[0]] = len(rank)
        return n
    if edge == "stolen-pair-decides-bins":
        # the three kept bins with every accepted pair counted (the reference) and with the stolen pairs removed
        (r, _) = run_pyref(c, check_ori=False)
        m = r[1]

        def kept(pairs):
            h = np.zeros(30, int)
            for i1, i2 in pairs:
                rot = f32(c["k1"]["angle"][i1] - c["k2"]["angle"][i2])
                rot = f32(rot + f32(360)) if rot < 0 else rot
                b = int(rha(f32(rot * (f32(1) / f32(30)))))
                h[0 if b == 30 else b] += 1
            m1 = m2 = m3 = 0
            i1_ = i2_ = i3_ = -1
            for i, v in enumerate(h):
                if v > m1:
                    m3, m2, m1, i3_, i2_, i1_ = m2, m1, v, i2_, i1_, i
                elif v > m2:
                    m3, m2, i3_, i2_ = m2, v, i2_, i
                elif v > m3:
                    m3, i3_ = v, i
            return {i1_, i2_, i3_}
        standing = [(i, int(k)) for i, k in enumerate(m) if k >= 0]
        stolen = [(t[2], int(m[t[1]])) for t in trace if t[0] == "steal" and m[t[1]] >= 0]
        return int(bool(stolen) and c["check_ori"] and kept(standing + stolen) != kept(standing))
    if edge == "equal-no-steal":
        return sum(1 for t in trace if t[0] != "steal" for (_, d, md) in t[1] if md == d)
    if edge == ">64-live":
        return sum(t[0] != "steal" for t in trace) - 64
    raise KeyError(edge)


def test_reach_table(capsys):
    rows = [(name, edge, reach(CASES[name], edge)) for name in NAMES for edge in CASES[name]["edges"]]
    with capsys.disabled():
        print()
        for name, edge, n in rows:
            print(f"  {name:34s} {edge:26s} {n}")
    zero = [(name, edge) for name, edge, n in rows if n < 1]
    assert not zero, f"edges not reached: {zero}"


@pytest.mark.parametrize("name", NAMES)
def test_built_outcome(name):
    """pyref gives the outcome the case was constructed for."""
    c = CASES[name]
    (r, _) = run_pyref(c)
    if c.get("expect") is None:
        return
    got = r[1]
    for i, e in enumerate(c["expect"]):
        if e is not None and e != -9:
            assert got[i] == e, f"{name}: query / feature {i} ended with {got[i]}, built for {e}"


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_pyref(name, oracle_mod):
    c = CASES[name]
    (r, _) = run_pyref(c)
    assert_same(c, run_oracle(c, oracle_mod), r, "oracle vs pyref")


def test_case_sizes():
    """At most 256 keypoints and queries a case, except where a capacity needs
    more: under 1,000 for the replay queue and the list lengths, 1610 a side
    for the 5 x 5 matrix of node sizes (1 + 63 + 64 + 65 + 129 features, five
    times), 4100 for the node-id list of more than 4096 ids."""
    for name, c in CASES.items():
        if c["family"] == "proj":
            n, nq = len(c["keys"]), len(c["queries"])
        elif c["family"] == "bow":
            n, nq = len(c["B"]["keys"]), len(c["A"]["keys"])
        elif c["family"] == "sim3":
            n, nq = len(c["kf2"]["keys"]), len(c["kf1"]["keys"])
        else:
            n, nq = len(c["k2"]), len(c["k1"])
        limit = 256
        if name.startswith(("queue-", "list5")):
            limit = 1000
        elif name.startswith("node-sizes-"):
            limit = 1610
        elif name.startswith("node-ids4097-"):
            limit = 4100
        assert n <= limit and nq <= limit, (name, n, nq)
