"""GJK / EPA (include/tmx_gjk.h) at the contacts real scenes are made of: PARALLEL faces and edges, exact touching, gaps down to 1e-15.
tests/test_hull_geometry.py draws its hulls in general position; here every pair is axis-aligned in one common frame Rw (identity, a
signed permutation, a random rotation), so the Minkowski difference has large coplanar facets and the closest feature is a whole face,
edge or vertex - the textbook weak spot of the algorithm.

Reference: exact closed forms, evaluated with mpmath (50 digits) from the DOUBLE inputs the code receives.  In the common frame the link
(a box, or a box swept along an axis - a longer box) and the obstacle (box, mesh box, axis-parallel segment, point) are axis-aligned
boxes [lo, hi]: per-axis gap a_i = max(loA_i - hiB_i, loB_i - hiA_i); some a_i > 0 -> distance sqrt(sum max(a_i, 0)^2), else max a_i
(negative: the penetration depth).  A segment that is parallel to a face but to no edge takes the segment-to-box closed forms (the
piecewise-quadratic distance along the segment, the separating-axis depth).  No Qhull here: coplanar Minkowski points are where it needs
joggling.  (The deep many-vertex penetrations at the end are in general position and keep the Qhull reference.)
orc.hull_contact takes no rounding radius - the collision term subtracts it - so the rounded family goes through its grid twice: its core
like every box, and with the radius through orc.evaluate (test_rounding_radius_on_the_grid).  The kernel-source legs compare the cast
values with the exact form too: link swept between two waypoints = segment (+) box.

Tolerances (set by the reference and the number format, not by the code under test): signed distance 1e-12 * s (right answers measure
<= 5e-16 at s = 1, the exact form's own error from a random Rw that is orthonormal to round-off ~1e-15, the smallest wrong answer of the
parent commit 2.9e-2); normal 1e-13 * s / |g| for |g| >= 1e-9 * s where it is unique (right answers: 4e-16 / g); witnesses inside their
sets to 1e-9 * s."""
import os

import mpmath as mp
import numpy as np
import pytest

import parity_checks as pc
from trajopt_amd import problem as tp, runtime
from trajopt_amd.problem import Robot, _tf12
from test_hull_geometry import _rot, _signed_distance_exact
from test_simt_emulation import simt_lib  # noqa: F401  (fixture)

mp.mp.dps = 50
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "gjk_contact_edges.npz")
SCALES = (0.01, 1.0, 10.0)
GAPS = tuple(sg * g for g in (1e-1, 1e-2, 1e-3, 1e-6, 1e-9, 1e-12, 1e-14, 1e-15) for sg in (1.0, -1.0)) + (0.0,)
CONTACTS = ("face_centred", "face", "edge", "vertex")     # face: with a lateral offset; face_centred: without (the most symmetric case)
PERM = np.array([[0.0, 0, -1], [-1.0, 0, 0], [0, 1.0, 0]])  # a signed permutation: axis-aligned in the world, other faces in front
SIGNS = np.array([[sx, sy, sz] for sx in (-1.0, 1) for sy in (-1.0, 1) for sz in (-1.0, 1)])
# box faces as triangles, counter-clockwise seen from outside (corner indices into SIGNS: 4 sx + 2 sy + sz)
BOX_TRIS = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4), (1, 5, 7), (1, 7, 3)]


def _frames():
    rng = np.random.default_rng(5)
    return {"identity": np.eye(3), "permuted": PERM, "random": _rot(rng)}


FRAMES = _frames()


# ---- exact geometry (mpmath) --------------------------------------------------------------------------------------------------------
def _mpm(a):
    a = np.asarray(a, dtype=np.float64)
    return mp.matrix(a.tolist()) if a.ndim == 2 else mp.matrix([[float(v)] for v in a])


def _to_common(Rw, pts):
    """world points (exact doubles) -> mp rows in the common frame: Rw' x"""
    RT = _mpm(Rw).T
    return [RT * _mpm(x) for x in np.asarray(pts, dtype=np.float64).reshape(-1, 3)]


def _placed(hv, R, t):
    """R v + t for every vertex, in mp from the doubles"""
    Rm, tm = _mpm(R), _mpm(t)
    return [Rm * _mpm(v) + tm for v in np.asarray(hv, dtype=np.float64).reshape(-1, 3)]


def _aabb(P):
    return [min(p[i] for p in P) for i in range(3)], [max(p[i] for p in P) for i in range(3)]


def _exact_boxes(PA, PB):
    """signed distance of two axis-aligned boxes given by their points + whether the contact normal is unique and along -x"""
    (la, ha), (lb, hb) = _aabb(PA), _aabb(PB)
    a = [max(la[i] - hb[i], lb[i] - ha[i]) for i in range(3)]
    if max(a) > 0:
        d = mp.sqrt(sum(max(x, 0) ** 2 for x in a))
        unique = a[0] > 0 and a[1] < 0 and a[2] < 0
    else:
        d = max(a)
        unique = a[0] > a[1] and a[0] > a[2]
    return d, bool(unique and la[0] - hb[0] == a[0])


def _exact_segment_box(PA, e0, e1):
    """signed distance of the segment e0 .. e1 and the axis-aligned box of the points PA (all in the common frame)"""
    lo, hi = _aabb(PA)

    def d2(u):
        x = [e0[i] + u * (e1[i] - e0[i]) for i in range(3)]
        return sum(max(lo[i] - x[i], x[i] - hi[i], 0) ** 2 for i in range(3))
    # the squared distance along the segment is convex and piecewise quadratic: pieces end where a coordinate crosses a box plane
    cuts = {mp.mpf(0), mp.mpf(1)}
    for i in range(3):
        de = e1[i] - e0[i]
        if de != 0:
            for pl in (lo[i], hi[i]):
                u = (pl - e0[i]) / de
                if 0 < u < 1:
                    cuts.add(u)
    cuts = sorted(cuts)
    best = min(d2(u) for u in cuts)
    for u0, u1 in zip(cuts[:-1], cuts[1:]):
        um = (u0 + u1) / 2
        f0, fm, f1 = d2(u0), d2(um), d2(u1)       # the quadratic through three points of the piece, and its vertex
        A = 2 * (f0 - 2 * fm + f1)
        if A > 0:
            w = (3 * f0 - 4 * fm + f1) / (2 * A)   # vertex in the piece's own parameter 0 .. 1
            if 0 < w < 1:
                best = min(best, d2(u0 + w * (u1 - u0)))
    if best > 0:
        return mp.sqrt(best)
    # overlapping: the facets of box - segment have the box's normals and the crosses of the segment with the box's edges
    dvec = [e1[i] - e0[i] for i in range(3)]
    axes = [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -dvec[2], dvec[1]], [dvec[2], 0, -dvec[0]], [-dvec[1], dvec[0], 0]]
    depth = None
    for ax in axes:
        nn = mp.sqrt(sum(c * c for c in ax))
        if nn == 0:
            continue
        for sg in (1, -1):
            n = [sg * c / nn for c in ax]
            hA = sum(max(n[i] * lo[i], n[i] * hi[i]) for i in range(3))
            lB = min(sum(n[i] * e[i] for i in range(3)) for e in (e0, e1))
            depth = hA - lB if depth is None else min(depth, hA - lB)
    return -depth


# ---- shape families -----------------------------------------------------------------------------------------------------------------
# (name, link half extents, obstacle kind, obstacle half extents / segment vector in the common frame, sweep, rounding radius) in
# units of the scale s
FAMILIES = {
    "cube_cube":        ((.5, .5, .5), "box", (.5, .5, .5), None, 0.0),
    "uneven_boxes":     ((.3, .5, .2), "box", (.4, .25, .6), None, 0.0),
    "box_mesh_box":     ((.5, .35, .4), "mesh", (.45, .5, .3), None, 0.0),
    "swept_in_plane":   ((.5, .5, .5), "box", (.5, .5, .5), (0.0, .8, 0.0), 0.0),
    "swept_on_normal":  ((.4, .5, .3), "box", (.5, .3, .5), (-.7, 0.0, 0.0), 0.0),
    "segment_on_face":  ((.5, .4, .45), "segment", (0.0, .4, .4), None, 0.0),     # parallel to the x face, to no edge
    "segment_on_edge":  ((.5, .4, .45), "segment", (0.0, .8, 0.0), None, 0.0),    # parallel to the y edges
    "point_on_face":    ((.5, .4, .45), "point", (0.0, 0.0, 0.0), None, 0.0),
    "rounded_box":      ((.4, .3, .5), "box", (.5, .5, .25), None, 0.05),
}
OBSTACLE_AT = np.array([0.3, -0.2, 0.1])   # common-frame position of the obstacle, in units of s (nothing sits at the world origin)


def _family_case(name, s, Rw, contact, g):
    """the doubles one call receives: dict(hv, R0, t0, R1, t1, oc, axis, box, mesh, radius) for gap g * s"""
    hA, kind, hB, sweep, radius = FAMILIES[name]
    hA = np.array(hA) * s
    ext = np.abs(np.array(hB)) * s * (0.5 if kind == "segment" else 1.0)   # half extents of the obstacle's bounding box
    tot = hA + ext
    c = np.array([tot[0] + g * s, 0.0, 0.0])
    if contact == "face":
        c[1], c[2] = 0.37 * tot[1], -0.23 * tot[2]
    elif contact in ("edge", "vertex"):
        c[1] = tot[1] + g * s
        c[2] = tot[2] + g * s if contact == "vertex" else -0.23 * tot[2]
    oc_c = OBSTACLE_AT * s
    case = dict(hv=SIGNS * hA, R0=Rw, R1=None, t1=None, axis=None, box=None, mesh=None, radius=radius * s, Rw=Rw, kind=kind)
    t_end = Rw @ (oc_c + c)
    if sweep is None:
        case["t0"] = t_end
    elif name == "swept_on_normal":        # arrives at the gap: the end pose is the placed one
        case["t0"], case["R1"], case["t1"] = Rw @ (oc_c + c - np.array(sweep) * s), Rw, t_end
    else:                                   # slides along the face: the sweep is centred on the placement
        case["t0"], case["R1"], case["t1"] = Rw @ (oc_c + c - 0.5 * np.array(sweep) * s), Rw, Rw @ (oc_c + c + 0.5 * np.array(sweep) * s)
    if kind == "box":
        case["oc"], case["box"] = Rw @ oc_c, np.concatenate([np.array(hB) * s, Rw.reshape(-1)])
    elif kind == "mesh":
        corners = (SIGNS * (np.array(hB) * s) + oc_c) @ Rw.T
        case["oc"], case["mesh"] = np.zeros(3), np.array([[corners[i] for i in tri] for tri in BOX_TRIS])
    elif kind == "segment":
        case["oc"], case["axis"] = Rw @ (oc_c - 0.5 * np.array(hB) * s), Rw @ (np.array(hB) * s)
    else:
        case["oc"] = Rw @ oc_c
    return case


def _exact(case):
    """-> (signed core distance, normal is unique and Rw (-1, 0, 0)) from the doubles of the case"""
    Rw = case["Rw"]
    RT = _mpm(Rw).T
    PA = _placed(case["hv"], case["R0"], case["t0"])
    if case["R1"] is not None:
        PA = PA + _placed(case["hv"], case["R1"], case["t1"])
    PA = [RT * p for p in PA]
    if case["kind"] == "segment":
        e0 = RT * _mpm(case["oc"])
        e1 = RT * (_mpm(case["oc"]) + _mpm(case["axis"]))
        return _exact_segment_box(PA, e0, e1), _exact_boxes(PA, [e0, e1])[1]   # (the families keep the segment's middle over the face)
    if case["kind"] == "box":
        h, oc = case["box"][:3], _mpm(case["oc"])
        Rb = _mpm(case["box"][3:].reshape(3, 3))
        PB = [RT * (oc + Rb * _mpm(sg * h)) for sg in SIGNS]
    elif case["kind"] == "mesh":
        PB = _to_common(Rw, case["mesh"])
    else:
        PB = _to_common(Rw, case["oc"])
    return _exact_boxes(PA, PB)


MAIN, Q_PEN = "main", "q of a penetration"


def _report(bad, of=None):
    return f"{len(bad)} failures{'' if of is None else f' of {of}'}, first: " + " | ".join(m for _, m in bad[:5])


def _check_case(orc, case, s, g, label, face=True):
    """one call of the oracle build against the exact forms -> list of failures (property, message); empty: right.  The property is
    Q_PEN for "q of an overlapping pair lies off the obstacle" (reported by a test of its own) and MAIN for every other one"""
    ins, p, q, tau = orc.hull_contact(case["hv"], case["R0"], case["t0"], case["oc"], R1=case["R1"], t1=case["t1"], axis=case["axis"],
                                      box=case["box"], mesh=case["mesh"])
    bad = []
    if not (np.isfinite(p).all() and np.isfinite(q).all() and np.isfinite(tau)):
        return [(MAIN, f"{label}: not finite p {p} q {q} tau {tau}")]
    d_exact, unique = _exact(case)
    got = float(np.linalg.norm(q - p)) * (-1.0 if ins else 1.0)
    err = abs(float(mp.mpf(got) - d_exact))
    if not err <= 1e-12 * s:
        bad.append((MAIN, f"{label}: signed distance {got!r}, exact {float(d_exact)!r}, |error| {err:.3e}"))
    if face and unique and abs(g) * s >= 1e-9 * s and not bad:    # (face-to-face only: an edge or vertex contact has a fan of normals)
        n = (q - p) / np.linalg.norm(q - p) * (-1.0 if ins else 1.0)
        dn = float(np.linalg.norm(n - case["Rw"] @ np.array([-1.0, 0.0, 0.0])))
        if not dn <= 1e-13 * s / (abs(g) * s):
            bad.append((MAIN, f"{label}: normal off by {dn:.3e}"))
    if not 0.0 <= tau <= 1.0:
        bad.append((MAIN, f"{label}: tau {tau}"))
    # witnesses: p in the link's (swept) hull, q in the obstacle - boxes in the common frame
    Rw, tol = case["Rw"], 1e-9 * s
    VA = case["hv"] @ np.asarray(case["R0"]).T + case["t0"]
    if case["R1"] is not None:
        VA = np.vstack([VA, case["hv"] @ np.asarray(case["R1"]).T + case["t1"]])
    VAc, pcm, qcm = VA @ Rw, p @ Rw, q @ Rw
    if not ((pcm >= VAc.min(axis=0) - tol).all() and (pcm <= VAc.max(axis=0) + tol).all()):
        bad.append((MAIN, f"{label}: p outside the link hull"))
    if case["kind"] == "segment":
        e0, ax = case["oc"], case["axis"]
        u = min(1.0, max(0.0, float((q - e0) @ ax / (ax @ ax))))
        off = float(np.linalg.norm(q - (e0 + u * ax)))
    else:
        if case["kind"] == "box":
            VB = (SIGNS * case["box"][:3]) @ case["box"][3:].reshape(3, 3).T + case["oc"]
        elif case["kind"] == "mesh":
            VB = case["mesh"].reshape(-1, 3)
        else:
            VB = case["oc"][None, :]
        VBc = VB @ Rw
        off = float(max((VBc.min(axis=0) - qcm).max(), (qcm - VBc.max(axis=0)).max(), 0.0))
    if not off <= tol:
        bad.append((Q_PEN if ins else MAIN, f"{label}: q {off:.3e} outside the obstacle"))
    return bad


# ---- CPU leg: the oracle build ------------------------------------------------------------------------------------------------------
def sweep_placements(g, n=1500):
    """the seeded sweep of parallel faces: unit cube link against a unit box, both under one random rotation per placement, the cube
    centre at Rw (1 + g, oy, oz) with oy, oz uniform in +-0.9 -> list of (Rw, t)"""
    rng = np.random.default_rng(2)
    out = []
    for _ in range(n):
        Rw = _rot(rng)
        oy, oz = rng.uniform(-0.9, 0.9, 2)
        out.append((Rw, Rw @ np.array([1.0 + g, oy, oz])))
    return out


def _sweep_case(Rw, t):
    return dict(hv=SIGNS * 0.5, R0=Rw, t0=t, R1=None, t1=None, oc=np.zeros(3), axis=None, mesh=None, radius=0.0, Rw=Rw, kind="box",
                box=np.concatenate([[0.5, 0.5, 0.5], Rw.reshape(-1)]))


@pytest.mark.parametrize("g", [1e-2, 1e-3, 1e-6, 1e-9])
def test_parallel_face_sweep(orc, g):
    """1 500 random placements of two parallel unit cubes per gap: every one right (the parent commit of this test got 4 to 6 per gap
    grossly wrong - "inside" with depth 0.3 to 0.7, or "separated" by 0.2 to 1.0 at a true gap of 0.01)"""
    bad = []
    for k, (Rw, t) in enumerate(sweep_placements(g)):
        bad += _check_case(orc, _sweep_case(Rw, t), 1.0, g, f"g {g:g} placement {k}")
    assert not bad, _report(bad)


@pytest.mark.parametrize("g", [0.0, 1e-15, 1e-14])
def test_touching_sweep(orc, g):
    """40 placements per gap at and next to exact touching (the parent commit: 10 of 40 at g = 0, 32 to 37 of 40 next to it reported
    a penetration of the cube's width with the normal reversed)"""
    bad = []
    for k, (Rw, t) in enumerate(sweep_placements(g, 40)):
        bad += _check_case(orc, _sweep_case(Rw, t), 1.0, g, f"g {g:g} placement {k}")
    assert not bad, _report(bad)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("frame", list(FRAMES))
@pytest.mark.parametrize("family", list(FAMILIES))
def test_family_grid(orc, family, frame, s):
    """every contact kind x every gap of one shape family in one frame at one scale: signed distance, normal, p in the link, q in the
    obstacle (separated and touching cases), tau, nothing NaN"""
    bad = [b for b in _grid(orc, family, frame, s) if b[0] != Q_PEN]
    assert not bad, _report(bad, len(CONTACTS) * len(GAPS))


_GRID = {}   # the rows of one (family, frame, scale) are computed once and read by the two tests that assert on them


def _grid(orc, family, frame, s):
    if (family, frame, s) not in _GRID:
        _GRID[family, frame, s] = [b for contact in CONTACTS for g in GAPS for b in
                                   _check_case(orc, _family_case(family, s, FRAMES[frame], contact, g), s, g, f"{family} {frame} s {s:g} {contact} g {g:g}",
                                               face=contact.startswith("face"))]
    return _GRID[family, frame, s]


def test_penetration_witness_on_the_obstacle(orc):
    """q of an OVERLAPPING pair lies in the obstacle to 1e-9 * s, on every row of the grid.
    A test of its own because it failed on its own: with the witnesses taken from EPA's closest TRIANGLE, 51 rows of 5 508 - all
    penetrations with the right depth and the right p - had q off the obstacle by up to its width (0.4 to 0.5 at s = 1, 4.7 at
    s = 10), where the origin projects into the closest facet of the Minkowski difference but outside that triangle.  tmx_gjk_epa now
    takes them from a second GJK run on the sets pulled apart along the face's normal."""
    bad = [b for family in FAMILIES for frame in FRAMES for s in SCALES for b in _grid(orc, family, frame, s) if b[0] == Q_PEN]
    assert not bad, _report(bad)


def _term_problem(hv_link, radius, oc, hB, Rw, n_steps, dist_pen, buffer, cast, reach):
    """three prismatic joints (x, y, z) carry the hull (vertex cloud in the link frame, rounded by radius): the joint values ARE the
    link's world position.  One box obstacle (centre oc, half extents hB, rotation Rw), one single-time-step collision cost with
    coefficient 1 and, with cast, one cast copy; dist_pen above every distance, so each value is dist_pen - (d - radius)"""
    rob = Robot(joint_types=[1, 1, 1], origins=[_tf12(), _tf12(), _tf12()], axes=[np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])],
                lower=np.full(3, -reach), upper=np.full(3, reach))
    rob.link_spheres = [(2, (0.0, 0.0, 0.0), radius, ("hull", hv_link))]
    pci = tp.ProblemConstructionInfo(rob, tp.BasicInfo(n_steps=n_steps))
    pci.obstacles = [(tuple(float(v) for v in oc), 0.0, ("box", tuple(float(v) for v in hB), Rw))]
    pci.cost_infos = [tp.CollisionTermInfo(dist_pen=dist_pen, coeff=1.0, safety_margin_buffer=buffer, evaluator_type=1, name="discrete")]
    if cast:
        pci.cost_infos.append(tp.CollisionTermInfo(dist_pen=dist_pen, coeff=1.0, safety_margin_buffer=buffer, evaluator_type=3, name="cast"))
    return pci


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("frame", list(FRAMES))
def test_rounding_radius_on_the_grid(orc, frame, s):
    """the rounding radius of the rounded_box family.  orc.hull_contact sees the CORE of a rounded hull (test_family_grid checks that
    core like any other box); the radius is applied by the collision term, so every contact kind x every gap of the family goes through
    orc.evaluate as the waypoints of ONE trajectory of a one-link robot, and each cost value is compared with
    dist_pen - (exact core distance - radius) to 1e-12 * s"""
    name, Rw = "rounded_box", FRAMES[frame]
    hA, _, hB, _, radius = FAMILIES[name]
    assert radius > 0.0
    cases = [(contact, g, _family_case(name, s, Rw, contact, g)) for contact in CONTACTS for g in GAPS]
    dist_pen = 0.5 * s                      # the largest distance of the grid is the vertex contact at g = 0.1: 0.1 sqrt(3) s
    pci = _term_problem((SIGNS * (np.array(hA) * s)) @ Rw.T, radius * s, cases[0][2]["oc"], np.array(hB) * s, Rw, len(cases), dist_pen, s, False,
                        100.0 * s)
    x = np.array([c["t0"] for _, _, c in cases])
    cv, _ = orc.evaluate(pci.to_desc(), x, x)
    assert cv.shape == (len(cases),) and np.isfinite(cv).all()
    bad = []
    for k, (contact, g, case) in enumerate(cases):
        # (the term places the cloud (SIGNS hA) Rw' at the identity, hull_contact placed SIGNS hA at Rw: the exact form takes the doubles
        # that THIS path receives)
        seen = dict(case, hv=(SIGNS * (np.array(hA) * s)) @ Rw.T, R0=np.eye(3))
        want = mp.mpf(dist_pen) - (_exact(seen)[0] - mp.mpf(radius * s))
        err = abs(float(mp.mpf(float(cv[k])) - want))
        if not err <= 1e-12 * s:
            bad.append((MAIN, f"{name} {frame} s {s:g} {contact} g {g:g}: cost {float(cv[k])!r}, exact {float(want)!r}, |error| {err:.3e}"))
    assert not bad, _report(bad, len(cases))


def test_deep_penetrations_of_many_vertex_hulls(orc):
    """a non-finding kept as a regression test: near-spherical hulls of 12 to 200 vertices deep inside a random box, in general position
    (Qhull reference of tests/test_hull_geometry.py, 1e-9)"""
    rng = np.random.default_rng(3)
    for nv in (12, 50, 200):
        for _ in range(20):
            hv = rng.standard_normal((nv, 3))
            hv *= (0.3 + 0.02 * rng.uniform(-1, 1, nv) / 1.0)[:, None] / np.linalg.norm(hv, axis=1)[:, None]
            R, t = _rot(rng), rng.standard_normal(3) * 0.1
            h, Rb, oc = rng.uniform(0.3, 0.5, 3), _rot(rng), rng.standard_normal(3) * 0.05
            VB = (SIGNS * h) @ Rb.T + oc
            ins, p, q, _ = orc.hull_contact(hv, R, t, oc, box=np.concatenate([h, Rb.reshape(-1)]))
            ref = _signed_distance_exact(hv @ R.T + t, VB)
            assert ins and ref < -0.05 and abs(-np.linalg.norm(q - p) - ref) <= 1e-9, (nv, ref, np.linalg.norm(q - p))


# ---- kernel-source legs: the same header inside the collision terms, 64 placements in one evaluate() ----------------------------------
DIST_PEN = 3.0
HALF = np.array([0.5, 0.5, 0.5])     # the unit cube link and the unit box obstacle of the recorded placements


def _golden():
    """tests/golden/gjk_contact_edges.npz: one rotation Rw and 64 cube centres t (8 seeds x 8 waypoints) as exact doubles.
    failed_on_parent marks the slots whose discrete contact the commit before this test got wrong by more than 1e-12 (parallel faces at
    gaps 1e-2 .. 1e-9, touching and next to it); the other slots come from the grid: contact says which kind each slot is (0 face,
    1 edge, 2 vertex), with gaps of both signs"""
    z = np.load(GOLDEN)
    return z["Rw"], z["t"].reshape(8, 8, 3), z["failed_on_parent"].reshape(8, 8), z["contact"].reshape(8, 8)


def test_golden_placements_are_what_the_file_says():
    """the recorded slots hold placements that failed before, and edge and vertex contacts next to the parallel faces"""
    Rw, t, failed, contact = _golden()
    assert t.dtype == np.float64 and failed.dtype == np.bool_ and failed.sum() == 48
    assert (contact[failed] == 0).all() and (contact == 1).sum() == 6 and (contact == 2).sum() == 6
    c = np.abs(t.reshape(-1, 3) @ Rw)   # common frame: a face contact has ONE coordinate near 1, an edge two, a vertex three
    assert np.array_equal((np.abs(c - 1.0) < 0.05).sum(axis=1) - 1, contact.reshape(-1))


def _exact_values(hv, Rw, x, radius):
    """the 8 discrete and 7 cast cost values of one seed (8 waypoints x), exact from the doubles: dist_pen - (d - radius).
    Cast: the link swept from waypoint k to k + 1 is segment (+) link box, so its signed distance to the obstacle box is that of the
    segment of the two centres to the obstacle box grown by the link box - the segment-to-box closed form, both signs"""
    RT = _mpm(Rw).T
    box = np.concatenate([HALF, Rw.reshape(-1)])
    out = []
    for k in range(8):
        case = dict(hv=hv, R0=np.eye(3), t0=x[k], R1=None, t1=None, oc=np.zeros(3), axis=None, mesh=None, Rw=Rw, kind="box", box=box)
        out.append(mp.mpf(DIST_PEN) - (_exact(case)[0] - mp.mpf(radius)))
    (ll, lh), (bl, bh) = _aabb([RT * _mpm(v) for v in hv]), _aabb([RT * (_mpm(Rw) * _mpm(sg * HALF)) for sg in SIGNS])
    grown = [mp.matrix([bl[i] - lh[i] for i in range(3)]), mp.matrix([bh[i] - ll[i] for i in range(3)])]
    for k in range(7):
        d = _exact_segment_box(grown, RT * _mpm(x[k]), RT * _mpm(x[k + 1]))
        out.append(mp.mpf(DIST_PEN) - (d - mp.mpf(radius)))
    return out


def _kernel_leg(ctx, orc, radius):
    """64 recorded placements through the discrete and the cast collision term of one build of the kernel sources: the values carry the
    oracle's BITS (one header, one sequence of IEEE operations, no contraction on any tier), every one of the 8 x 15 matches the exact
    form to 1e-12, and the first QP's rows - built from normal and witnesses - agree with the oracle's"""
    Rw, x0, _, _ = _golden()
    hv = (SIGNS * HALF) @ Rw.T
    pci = _term_problem(hv, radius, np.zeros(3), HALF, Rw, 8, DIST_PEN, 1.0, True, 20.0)
    desc = pc.make_ctx_inputs(ctx, pci, x0)
    cv, vv = ctx.evaluate()
    worst, differing = 0.0, 0
    for b in range(8):
        ocv, ovv = orc.evaluate(desc, x0[b], x0[b])
        assert cv[b].shape == ocv.shape == (15,) and vv[b].shape == ovv.shape and np.isfinite(cv[b]).all()
        differing += int((cv[b].view(np.uint64) != ocv.view(np.uint64)).sum() + (vv[b].view(np.uint64) != ovv.view(np.uint64)).sum())
        want = _exact_values(hv, Rw, x0[b], radius)
        err = [abs(float(mp.mpf(float(cv[b, k])) - want[k])) for k in range(15)]
        worst = max(worst, max(err))
        assert max(err) <= 1e-12, (b, int(np.argmax(err)), float(cv[b, int(np.argmax(err))]), float(want[int(np.argmax(err))]))
    print(f"64 placements, radius {radius}: worst |cost - exact| {worst:.2e} over 8 x 15 values, {differing} words differ from the oracle's")
    assert differing == 0, f"{differing} of the values differ in their bits from the oracle's"
    for b in range(8):
        pc.check_first_qp_structure(ctx, orc, desc, x0, b, val_tol=1e-12)


@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_placements_in_the_collision_terms_on_host_build(hostemu_lib, orc, radius):
    ctx = runtime.Context(0, hostemu_lib)
    _kernel_leg(ctx, orc, radius)
    ctx.close()


@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_placements_in_the_collision_terms_on_simt_emulation(simt_lib, orc, radius):
    ctx = runtime.Context(0, simt_lib)
    _kernel_leg(ctx, orc, radius)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [0.0, 0.05])
def test_placements_in_the_collision_terms_on_device(gpu_ctx_factory, orc, radius):
    ctx = gpu_ctx_factory()
    _kernel_leg(ctx, orc, radius)
    ctx.close()
