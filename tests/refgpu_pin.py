"""What the pin against the compiled gpu-version shares (tests/golden/make_ref_gpu_pin.py writes the fixtures; test_reference_gpu_pin.py
holds the restatement to them, test_gpu_reference_gpu_pin.py the kernel): the rays of a record scene, the rule that says which
rays are decided, the fp64 statement of a ray's record, the comparison and its bounds, and the doctored fixtures.

Rays are not stored (3400 rays of six random floats do not compress): they are made again from the scene's primitives and a seed,
and the fixture holds the SHA-256 of their bytes.

DECIDED is a rule on the inputs alone, evaluated in fp64 (ref64's tables, this file's geometry).  A ray is set aside when, for some
primitive, the fp64 geometry is within MARGIN of flipping that primitive's verdict:
  * a rect's plane point within MARGIN (scene units) of an edge, unless the ray's direction is zero along that edge's axis: then
    the coordinate is the origin's, exact in every precision, and an edge hit is decided (inclusive bounds, object.cuh:112);
  * a sphere's or tube's discriminant within MARGIN of zero, relative to hb^2;
  * a tube's root within MARGIN of an open end (object-space z);
  * a root or a rect's t within MARGIN of t_min, relative to max(1, |t|);
  * the two nearest candidates of different primitives within MARGIN of each other, relative to max(1, t) -- unless both compute one
    t by one expression on the same numbers (coplanar rects of one kind, spheres of one centre and radius): there the LATER list
    entry wins in every precision (object.cuh:29, `t > t_max` fails on equality), and the winner is the subject;
and, as classes of input on which the reference parts from fp64 and restatement through a quirk of its own:
  * a ray parallel to a tube's axis (a = dx^2 + dy^2 <= 1e-12 |d|^2 in object space): quadratic() divides 0 by 0, every
    comparison with the NaN fails, cylinder::hit carries t = NaN past its range and end tests (object.cuh:206-207, 248-270) and
    its own assertion on phi (:285) then stops the program: such a ray is never handed to the compiled reference;
  * a ray in a rect's plane (origin on it, direction zero across it): t = 0 / 0, accepted the same way (object.cuh:107-112).  The
    rays made here never are."""
import hashlib
import os

import numpy as np

import ref64 as R
import trace_cases as TC
from ref64_base import _affine, _dot, _rect_axes

RECORD_SCENES = ("zoo", "inside", "ties")
PATH_SCENES = ("glass and lights", "checker furnace", "depth 3")
W, H, SPP, SEED = 48, 27, 8, 2023
DRAWS = 64               # uniforms per sample handed to ref64.trace: 2 for the film, one per dielectric event, depth <= 50
RAY_SEED = 20241021
N_RANDOM, N_AXIS = 3000, (120, 120, 60)   # make_rays-style rays; axis-parallel rays along x, y, z
MARGIN = 5e-4
CAP = 0.05
# what the project holds against fp64 already (test_primitives_fuzz.py, test_gpu_trace.py); to each the fixture adds the reference's own
# measured distance from fp64 for that quantity (triangle inequality)
BOUND = dict(t=2e-6, p=1e-5, normal=1e-5, uv=7e-6)
T_MIN = R.T_MIN


def key(name):
    return name.replace(" ", "_")


# ------------------------------------------------------------------------------------------------------------------- rays
def _to_world(pr, q):
    m = pr["m"].astype(np.float64).reshape(3, 4)
    return q @ m[:, :3].T + m[:, 3]


def make_record_rays(name, prims, seed=RAY_SEED):
    """(origins, directions) float32 of a record scene.  N_RANDOM rays by trace_cases.make_rays (origins in the primitives' box
    scaled 1.5 x, half aimed into the box, half isotropic, |dir| log-uniform in [0.1, 10]), then sum(N_AXIS) axis-parallel rays from
    the same box.  "inside": the first half of the random rays start inside a sphere or a tube, and a quarter of those that start
    in a tube run within 20 degrees of its axis, out through an open end; another 300 start on a tube's axis outside an end and
    aim at a point inside it.  "ties": the axis-parallel rays that run across a rect start exactly over one of its edges."""
    boxes = [TC.prim_box(p) for p in prims]
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    o, d = TC.make_rays(lo, hi, n=N_RANDOM, seed=seed)
    o, d = o.astype(np.float64), d.astype(np.float64)
    rng = np.random.default_rng(seed + 1)
    centre, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    ao, ad = [], []
    for axis, n in enumerate(N_AXIS):
        oo = centre + 1.5 * half * rng.uniform(-1.0, 1.0, (n, 3))
        dd = np.zeros((n, 3))
        dd[:, axis] = rng.choice([-1.0, 1.0], n) * np.exp(rng.uniform(np.log(0.1), np.log(10.0), n))
        ao.append(oo), ad.append(dd)
    ao, ad = np.concatenate(ao), np.concatenate(ad)
    if name == "inside":
        solids = [p for p in prims if int(p["type"]) in (R.SPHERE, R.CYLINDER)]
        tubes = [p for p in prims if int(p["type"]) == R.CYLINDER]
        for i in range(N_RANDOM // 2):
            pr = solids[i % len(solids)]
            f = pr["f"].astype(np.float64)
            if int(pr["type"]) == R.SPHERE:
                q = rng.normal(0.0, 1.0, 3)
                o[i] = f[:3] + 0.9 * abs(f[3]) * rng.uniform(0.0, 1.0) ** (1 / 3) * q / np.sqrt(q @ q)
            else:
                rho, phi, z = 0.9 * f[0] * np.sqrt(rng.uniform()), rng.uniform(0, 2 * np.pi), rng.uniform(f[1], f[2])
                o[i] = _to_world(pr, np.array([rho * np.cos(phi), rho * np.sin(phi), z]))
                if i % 4 == 0:
                    tilt, az = np.deg2rad(rng.uniform(0.5, 20.0)), rng.uniform(0, 2 * np.pi)
                    q = np.array([np.sin(tilt) * np.cos(az), np.sin(tilt) * np.sin(az), rng.choice([-1.0, 1.0]) * np.cos(tilt)])
                    d[i] = (_to_world(pr, q) - _to_world(pr, np.zeros(3))) * np.sqrt(d[i] @ d[i])
        eo, ed = [], []
        for i in range(300):
            pr = tubes[i % len(tubes)]
            f = pr["f"].astype(np.float64)
            end = f[1] - rng.uniform(0.3, 2.0) if i % 2 else f[2] + rng.uniform(0.3, 2.0)
            rho, phi, z = f[0] * rng.uniform(0.0, 1.3), rng.uniform(0, 2 * np.pi), rng.uniform(f[1], f[2])
            a = _to_world(pr, np.array([0.3 * f[0] * rng.uniform(-1, 1), 0.3 * f[0] * rng.uniform(-1, 1), end]))
            b = _to_world(pr, np.array([rho * np.cos(phi), rho * np.sin(phi), z]))
            eo.append(a), ed.append((b - a) * rng.uniform(0.2, 3.0))
        o, d = np.concatenate([o, np.array(eo)]), np.concatenate([d, np.array(ed)])
    if name == "ties":
        rects = [p for p in prims if int(p["type"]) in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT)]
        for i in range(len(ao)):
            axis = int(np.flatnonzero(ad[i])[0])
            mine = [p for p in rects if _rect_axes(p["type"])[0] == axis]
            if not mine:
                continue
            pr = mine[i % len(mine)]
            _, aa, ba = _rect_axes(pr["type"])
            f = pr["f"].astype(np.float64)
            edge = (i // len(mine)) % 4  # a0, a1, b0, b1 in turn; the other coordinate anywhere along the edge and a little past
            ao[i, aa] = f[edge] if edge < 2 else f[0] + (f[1] - f[0]) * rng.uniform(-0.1, 1.1)
            ao[i, ba] = f[edge] if edge >= 2 else f[2] + (f[3] - f[2]) * rng.uniform(-0.1, 1.1)
    o, d = np.concatenate([o, ao]).astype(np.float32), np.concatenate([d, ad]).astype(np.float32)
    return o, d


def digest(o, d):
    return hashlib.sha256(np.ascontiguousarray(o).tobytes() + np.ascontiguousarray(d).tobytes()).hexdigest()


# --------------------------------------------------------------------------------------------------------------- the rule
def _same_t_class(prims):
    """primitives that compute one t by one expression on the same numbers share a class"""
    seen, out = {}, []
    for i, p in enumerate(prims):
        ty = int(p["type"])
        k = (ty, p["f"][4].tobytes()) if ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT) else (ty, p["f"][:4].tobytes()) if ty == R.SPHERE else (ty, i)
        out.append(seen.setdefault(k, len(seen)))
    return np.array(out)


def _t_margin(t):
    return np.abs(t - T_MIN) / np.maximum(1.0, np.abs(t))


def candidates(prims, o, d):
    """per primitive and ray, in fp64: (t at which the primitive alone is hit, NaN where it is not; how far its verdict is from
    flipping; whether the ray belongs to the primitive's quirk class)"""
    n = len(o)
    big = np.full(n, np.inf)
    dd = _dot(d, d)
    T, M, Q = [], [], []
    with np.errstate(all="ignore"):
        for p in prims:
            ty, f = int(p["type"]), p["f"].astype(np.float64)
            quirk = np.zeros(n, bool)
            if ty == R.SPHERE:
                oc = o - f[:3]
                hb = _dot(oc, d)
                disc = hb * hb - dd * (_dot(oc, oc) - f[3] * f[3])
                md = np.abs(disc) / np.maximum(hb * hb, 1e-30)
                sq = np.sqrt(np.maximum(disc, 0))
                t0, t1 = (-hb - sq) / dd, (-hb + sq) / dd
                t = np.where(disc < 0, np.nan, np.where(t0 >= T_MIN, t0, np.where(t1 >= T_MIN, t1, np.nan)))
                m = np.where(disc < 0, md, np.minimum(md, np.minimum(_t_margin(t0), _t_margin(t1))))
            elif ty in (R.XY_RECT, R.XZ_RECT, R.YZ_RECT):
                ka, aa, ba = _rect_axes(ty)
                quirk = (d[:, ka] == 0) & (o[:, ka] == f[4])
                tt = (f[4] - o[:, ka]) / d[:, ka]
                a, b = o[:, aa] + tt * d[:, aa], o[:, ba] + tt * d[:, ba]
                inside = (a >= f[0]) & (a <= f[1]) & (b >= f[2]) & (b <= f[3])
                ea = np.where(d[:, aa] == 0, big, np.minimum(np.abs(a - f[0]), np.abs(a - f[1])))
                eb = np.where(d[:, ba] == 0, big, np.minimum(np.abs(b - f[2]), np.abs(b - f[3])))
                # a point that one exact coordinate already puts outside stays outside whatever the other one does
                out_a = (d[:, aa] == 0) & ((a < f[0]) | (a > f[1]))
                out_b = (d[:, ba] == 0) & ((b < f[2]) | (b > f[3]))
                edge = np.where(out_a | out_b, big, np.minimum(ea, eb))
                ok = np.isfinite(tt) & (tt >= T_MIN)
                t = np.where(ok & inside, tt, np.nan)
                m = np.where(np.isfinite(tt), np.where(tt < T_MIN, _t_margin(tt), np.minimum(edge, _t_margin(tt))), big)
            elif ty == R.CYLINDER:
                Rm, tr = _affine(p["m_inv"], np.float64)
                oo, od = o @ Rm.T + tr, d @ Rm.T
                A = od[:, 0] ** 2 + od[:, 1] ** 2
                quirk = A <= 1e-12 * dd
                hb = od[:, 0] * oo[:, 0] + od[:, 1] * oo[:, 1]
                disc = hb * hb - A * (oo[:, 0] ** 2 + oo[:, 1] ** 2 - f[0] * f[0])
                md = np.abs(disc) / np.maximum(hb * hb, 1e-30)
                sq = np.sqrt(np.maximum(disc, 0))
                t0, t1 = (-hb - sq) / A, (-hb + sq) / A
                z0, z1 = oo[:, 2] + t0 * od[:, 2], oo[:, 2] + t1 * od[:, 2]
                ok0 = (t0 >= T_MIN) & (z0 >= f[1]) & (z0 <= f[2])
                ok1 = (t1 >= T_MIN) & (z1 >= f[1]) & (z1 <= f[2])
                t = np.where(disc < 0, np.nan, np.where(ok0, t0, np.where(ok1, t1, np.nan)))

                def root(tt, z):
                    return np.where(tt < T_MIN, _t_margin(tt), np.minimum(_t_margin(tt), np.minimum(np.abs(z - f[1]), np.abs(z - f[2]))))
                m = np.where(disc < 0, md, np.minimum(md, np.minimum(root(t0, z0), root(t1, z1))))
                m = np.where(quirk, 0.0, m)
            else:
                raise ValueError("the compiled gpu-version has no such primitive")
            T.append(t), M.append(np.nan_to_num(m, nan=0.0)), Q.append(quirk)
    return np.array(T), np.array(M), np.array(Q)


def decided(prims, o32, d32, margin=MARGIN):
    """(decided [n], quirk [n], tie [n]: the earlier entry of a same-t pair both of whose members hold the winning point, -1
    elsewhere) -- a rule on the inputs alone"""
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    T, M, Q = candidates(prims, o, d)
    cls = _same_t_class(prims)
    n = len(o)
    ok = (M > margin).all(axis=0)
    Tn = np.where(np.isnan(T), np.inf, T)
    first = Tn.argmin(axis=0)
    t1 = Tn[first, np.arange(n)]
    other = np.where(cls[:, None] == cls[first][None, :], np.inf, Tn)  # the nearest candidate of another class
    t2 = other.min(axis=0)
    with np.errstate(invalid="ignore"):
        gap = np.where(np.isfinite(t2), (t2 - t1) / np.maximum(1.0, t1), np.inf)
    ok &= ~(np.isfinite(t1) & (gap <= margin))
    quirk = Q.any(axis=0)
    same = (Tn == t1[None, :]) & np.isfinite(t1)[None, :] & (cls[:, None] == cls[first][None, :])
    tie = np.where(same.sum(axis=0) >= 2, same.argmax(axis=0), -1)
    return ok & ~quirk, quirk, tie


# ------------------------------------------------------------------------------------------------- records, fp64 and compared
def fp64_records(S, o32, d32):
    """ref64's statement of the rays' records, in fp64: the dict of rtcheck.RefGpuScene.hit"""
    o, d = o32.astype(np.float64), d32.astype(np.float64)
    t, idx = R.closest_hit(S, o, d, np.inf, np.float64)
    hit = idx >= 0
    out = dict(index=idx.astype(np.int32), front=np.zeros(len(o), np.int32), t=np.where(hit, t, np.inf), p=np.zeros((len(o), 3)),
               normal=np.zeros((len(o), 3)), u=np.zeros(len(o)), v=np.zeros(len(o)))
    if hit.any():
        p, nrm, front = R.hit_record(S, o[hit], d[hit], t[hit], idx[hit], np.float64)
        u, v = R.hit_uv(S, o[hit], d[hit], t[hit], idx[hit], np.float64)
        out["p"][hit], out["normal"][hit], out["front"][hit], out["u"][hit], out["v"][hit] = p, nrm, front, u, v
    return out


def reference_records(rs, prims, o32, d32):
    """rtcheck.RefGpuScene.hit on the rays outside the quirk classes; a ray inside one is reported as a miss and is never judged.
    (The reference cannot be asked: on a ray parallel to a tube's axis its own assertion on phi, object.cuh:285, stops the program.)"""
    _, quirk, _ = decided(prims, o32, d32)
    got = rs.hit(o32[~quirk], d32[~quirk])
    n = len(o32)
    out = dict(index=np.full(n, -1, np.int32), front=np.zeros(n, np.int32), t=np.full(n, np.inf, np.float32),
               p=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    for q in out:
        out[q][~quirk] = got[q]
    return out


def unpack_records(z, n):
    """the reference's records of a fixture (stored for the hits only) as the dict of rtcheck.RefGpuScene.hit"""
    index = z["index"].astype(np.int32)
    hit = index >= 0
    out = dict(index=index, front=np.zeros(n, np.int32), t=np.full(n, np.inf, np.float32), p=np.zeros((n, 3), np.float32),
               normal=np.zeros((n, 3), np.float32), u=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    out["front"][hit] = np.unpackbits(z["front"])[:hit.sum()]
    for q in ("t", "p", "normal", "u", "v"):
        out[q][hit] = z[q]
    return out


def load_record_case(rtmi, golden_dir, name):
    """everything a test needs of a record fixture: the scene (parsed from the stored JSON), its rays (made again, checked against
    the stored digest), the reference's records, the rule's verdicts, the reference's stored distance from fp64 per quantity"""
    z = np.load(os.path.join(golden_dir, f"refgpu_records_{name}.npz"))
    sc = rtmi.Scene.parse(str(z["scene"]))
    prims = sc.prims()
    o, d = make_record_rays(name, prims, int(z["ray_seed"]))
    assert len(o) == int(z["n_rays"]) and digest(o, d) == str(z["rays_sha256"]), "the rays are not the fixture's"
    judged, quirk, tie = decided(prims, o, d, float(z["margin"]))
    return dict(z=z, sc=sc, prims=prims, o=o, d=d, ref=unpack_records(z, len(o)), judged=judged, quirk=quirk, tie=tie,
                dev=dict(zip(("t", "p", "normal", "uv"), z["ref_fp64_dev"][:, 0])))


def records_of_hits(h):
    """Scene.trace's HIT_DTYPE records as that dict"""
    hit = h["prim"] >= 0
    return dict(index=np.where(hit, h["prim"], -1).astype(np.int32), front=np.where(hit, h["front"] != 0, 0).astype(np.int32),
                t=np.where(hit, h["t"], np.inf).astype(np.float32), p=h["point"].copy(), normal=h["normal"].copy(), u=h["u"].copy(),
                v=h["v"].copy())


def _u_period(prims, index):
    """the record's u wraps where the angle's branch is cut: by 1 on a sphere, by 1/2 on a tube (u = (phi + 2 pi) / 4 pi)"""
    ty = prims["type"][np.maximum(index, 0)]
    return np.where(ty == R.SPHERE, 1.0, np.where(ty == R.CYLINDER, 0.5, 0.0))


def deviations(prims, a, b, judged):
    """per quantity, |a - b| over the judged rays that both call a hit of one primitive: t relative to max(1, |t|), p relative to
    max(1, |p|), normal and (u, v) absolute, u up to its period"""
    k = judged & (a["index"] >= 0) & (a["index"] == b["index"])
    A = {q: np.asarray(a[q], np.float64)[k] for q in ("t", "p", "normal", "u", "v")}
    B = {q: np.asarray(b[q], np.float64)[k] for q in ("t", "p", "normal", "u", "v")}
    du = np.abs(A["u"] - B["u"])
    per = _u_period(prims, a["index"][k])
    du = np.where(per > 0, np.minimum(du, np.abs(per - du)), du)
    return dict(t=np.abs(A["t"] - B["t"]) / np.maximum(1.0, np.abs(B["t"])),
                p=np.sqrt(((A["p"] - B["p"]) ** 2).sum(axis=1)) / np.maximum(1.0, np.sqrt((B["p"] ** 2).sum(axis=1))),
                normal=np.abs(A["normal"] - B["normal"]).max(axis=1), uv=np.maximum(du, np.abs(A["v"] - B["v"])))


def measure(prims, a, b, judged):
    """{quantity: (max, median)} of deviations(), and the hit/miss or winner disagreements among the judged rays"""
    dev = deviations(prims, a, b, judged)
    return {q: (float(v.max()), float(np.median(v))) for q, v in dev.items()}, int((judged & (a["index"] != b["index"])).sum())


def compare_records(name, prims, got, ref, judged, ref_dev, min_hits=500):
    """`got` (the restatement's or the kernel's records) against `ref` (the reference's, from the fixture) on the judged rays: hit
    or miss, the winning index and front equal on every one; t, p, normal, (u, v) within BOUND plus the reference's stored
    maximum distance from fp64 (ref_dev[quantity]).  Returns the figures; AssertionError says what differs."""
    wrong = judged & (got["index"] != ref["index"])
    assert not wrong.any(), (name, "hit / miss or winner differs on", int(wrong.sum()), "rays, first", int(np.flatnonzero(wrong)[0]),
                             int(got["index"][wrong][0]), int(ref["index"][wrong][0]))
    hits = judged & (ref["index"] >= 0)
    assert hits.sum() >= min_hits, (name, "too few hits to say anything", int(hits.sum()))
    flipped = hits & (got["front"] != ref["front"])
    assert not flipped.any(), (name, "front differs on", int(flipped.sum()), "rays, first", int(np.flatnonzero(flipped)[0]))
    fig, _ = measure(prims, got, ref, judged)
    for q, (worst, _) in fig.items():
        assert worst <= BOUND[q] + ref_dev[q], (name, q, worst, BOUND[q], ref_dev[q])
    return fig


# ------------------------------------------------------------------------------------------------------- doctored fixtures
def doctored(mistake, prims, ref, tie):
    """a copy of the reference's records with one deliberate mistake; returns (records, the number of rays it changes)"""
    out = {k: v.copy() for k, v in ref.items()}
    hit = ref["index"] >= 0
    ty = prims["type"][np.maximum(ref["index"], 0)]
    if mistake == "cylinder u over 2 pi":       # u = phi / 2 pi with phi = atan2 + 2 pi: twice the reference's
        k = hit & (ty == R.CYLINDER)
        out["u"][k] = 2 * ref["u"][k]
    elif mistake == "rect uv swapped":
        k = hit & np.isin(ty, (R.XY_RECT, R.XZ_RECT, R.YZ_RECT))
        out["u"][k], out["v"][k] = ref["v"][k], ref["u"][k]
    elif mistake == "earlier entry wins a tie":
        k = hit & (tie >= 0) & (tie != ref["index"])
        out["index"][k] = tie[k]
    elif mistake == "normals not face-turned":  # the outward normal whatever side the ray comes from
        k = hit & (ref["front"] == 0)
        out["normal"][k] = -ref["normal"][k]
    else:
        raise ValueError(mistake)
    return out, int(k.sum())


RECORD_MISTAKES = ("cylinder u over 2 pi", "rect uv swapped", "earlier entry wins a tie", "normals not face-turned")


# ---------------------------------------------------------------------------------------------------------------- checker
CHECKER_POINTS = 10000
CHECKER_MARGIN = 1e-4  # fp32 rounds 10 x at |x| <= 5 by at most 4e-6, so a product of sines this large has no factor that can flip


def checker_points():
    return np.random.default_rng(RAY_SEED + 7).uniform(-5.0, 5.0, (CHECKER_POINTS, 3)).astype(np.float32)


def checker_clear(points):
    """the points whose parity is decided: |sin 10x sin 10y sin 10z| > CHECKER_MARGIN in fp64"""
    return np.abs(np.sin(10.0 * points.astype(np.float64)).prod(axis=1)) > CHECKER_MARGIN


# ------------------------------------------------------------------------------------------------------------------ paths
def sample_ids():
    """(x, y, s) of every sample of a path scene, ordered (s, y, x): the order of ref64.uniforms and of one-sample frames"""
    s, y, x = np.meshgrid(np.arange(SPP), np.arange(H), np.arange(W), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), s.ravel()], axis=1).astype(np.int32)


def path_figures(got, ref):
    """share within 1e-4 max(1, |ref|) (the project's gate (a)) and the median of the per-sample error"""
    diff = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    return float((diff <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(axis=1).mean()), float(np.median(diff.max(axis=1)))


def image_of(rgb):
    """(H, W, 3) fp64 sums of per-sample radiance ordered (s, y, x)"""
    return rgb.astype(np.float64).reshape(SPP, H, W, 3).sum(axis=0)


def compare_paths(name, got, ref, ref_median, got_image=None, got_draws=None, ref_draws=None):
    """per-sample radiance `got` against the fixture's `ref`: gate (a) >= 97 % within 1e-4 max(1, |ref|); the median error at most
    2e-6 (test_oracle_pin.py's bound) plus the reference's stored median distance from fp64; G3 on the image as
    test_oracle_pin.py has it; draw counts equal wherever the radiance agrees to 1e-5"""
    share, median = path_figures(got, ref)
    assert share >= 0.97, (name, "only", share, "of per-sample radiances within 1e-4 of the reference")
    assert median <= 2e-6 + ref_median, (name, median, ref_median)
    mine = (image_of(got) if got_image is None else got_image.astype(np.float64)) / SPP
    theirs = image_of(ref) / SPP
    d = np.abs(mine - theirs)
    assert d.mean() <= 2e-3 * np.sqrt(100.0 / SPP), (name, d.mean())
    assert np.median(d) < 1e-6, (name, np.median(d))
    sigma = theirs.std() / np.sqrt(theirs.size * SPP)
    assert abs(mine.mean() - theirs.mean()) <= max(3 * sigma, 2e-4), (name, mine.mean(), theirs.mean())
    if got_draws is not None:
        agree = np.abs(got.astype(np.float64) - ref).max(axis=1) <= 1e-5
        assert agree.sum() > 0.9 * len(ref) and np.array_equal(got_draws[agree], ref_draws[agree]), \
            (name, "draw counts differ on", int((got_draws[agree] != ref_draws[agree]).sum()), "samples of equal radiance")
    return share, median
