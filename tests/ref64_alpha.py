"""Alpha cutouts for the fp64 statement of ref64.py: an alpha-aware closest hit, written from the model's text in
include/rtmi.h -- not from csrc/rt_alpha.h, with which it shares nothing.

The model.  A material may carry a mask: an image texture with an alpha plane and a cutoff.  The mask is read at the hit
record's (u, v) with ref64.image_texel's nearest texel (the row from u, the column from v, clamped).  With a8 the alpha byte
there and c8 = clamp(ceil(255 cutoff), 1, 255), the hit is transparent iff a8 < c8.  A transparent hit is no vertex: the query
goes on from o + t d in the same direction with the usual t_min and t_max - t left of its range, nothing else happens.  One
query passes through at most CAP = 64 transparent hits: the next masked hit counts as opaque whatever its texel says.

closest_hit() below calls ref64.closest_hit, finds the winners' materials and masks, reads the texels through ref64.hit_uv and
ref64.image_texel, and calls again for the rays whose winner is transparent.  It returns the total t from the original origin
and the opaque winner, or -1.

trace() / reference() run ref64.trace / ref64.reference with that function in place of ref64.closest_hit -- its two call sites
are the path query (a scalar t_max) and the shadow query (an array of far ends) -- for the duration of the call, restored in a
`finally`.  ref64.py itself holds no word of alpha; folding this module into it is a follow-up for when that file may change.
What the replaced function cannot see through its arguments -- which samples the rays belong to, and the paths' depth counters
for one deliberate mistake -- it reads from the calling frame's locals (`who`, `m`, `k`, `depth` of ref64.trace).

The tally (new_tally(); counted in the fp64 run alone, or in the run at tally["dtype"]): hits that carried a mask, passes, opaque verdicts, the most passes in
one query, shadow queries that passed through at least one hole, the samples that met a masked hit, and -- for the feature
passes -- first_t / first_idx, every sample's first path query's total t and opaque winner.

Deliberate mistakes (PERTURBATIONS), for the tests that show the comparison can fail:
  al_off            masks ignored
  al_inverted       transparent iff a8 >= c8
  al_uv_swapped     the mask read with the row from v and the column from u
  al_shadow_opaque  shadow rays do not pass
  al_counts_bounce  a pass uses up a bounce
"""
import sys

import numpy as np

import ref64 as R

CAP = 64
PERTURBATIONS = ("al_off", "al_inverted", "al_uv_swapped", "al_shadow_opaque", "al_counts_bounce")
COUNTERS = ("masked_hits", "passes", "opaque", "max_passes", "shadow_through", "shadow_queries", "path_queries")


def cutoff_byte(cutoff):
    """c8 = clamp(ceil(255 cutoff), 1, 255), in fp64"""
    return int(min(max(np.ceil(255.0 * np.float64(cutoff)), 1.0), 255.0))


def masks_of(sc):
    """material -> (alpha plane [rows][cols] uint8, c8) of a product scene"""
    out = {}
    for m in range(len(sc.materials())):
        a = sc.alpha(m)
        if a is not None:
            plane = sc.get_image_alpha(int(a[0]))
            assert plane is not None, (m, a)
            out[m] = (plane, cutoff_byte(a[1]))
    return out


def ref_scene(sc, **kw):
    """ref64.RefScene of a product scene with its masks attached (alpha_masks)"""
    S = R.RefScene(sc, **kw)
    S.alpha_masks = masks_of(sc)
    return S


def new_tally(n=0):
    t = dict.fromkeys(COUNTERS, 0)
    t["sample_masked"] = np.zeros(n, bool)
    t["first_t"] = np.full(n, np.nan)
    t["first_idx"] = np.full(n, -1, np.int64)
    t["first_seen"] = np.zeros(n, bool)
    return t


def closest_hit(S, o, d, t_max, T, plain=None, perturb=(), tally=None, samples=None, depth=None, on_pass=None):
    """the alpha-aware closest hit of the rays (o, d): (total t from o, the opaque winner or -1).  plain: ref64's own
    closest_hit; samples: the rays' sample indices (for the tally); depth: ref64.trace's counters, for al_counts_bounce;
    on_pass(samples or None, points, directions): called with the hole points of every round of passes"""
    plain = plain or R.closest_hit
    masks = {} if "al_off" in perturb else getattr(S, "alpha_masks", {})
    n = len(o)
    shadow = not np.isscalar(t_max)
    if shadow and "al_shadow_opaque" in perturb:
        masks = {}
    left = np.full(n, t_max, T) if np.isscalar(t_max) else np.asarray(t_max).astype(T).copy()
    at = np.array(o, T, copy=True)
    total = np.zeros(n, T)
    passes = np.zeros(n, np.int64)
    out_t = left.copy()
    out_idx = np.full(n, -1, np.int64)
    todo = np.arange(n)
    material = S.prims["material"]
    while len(todo):
        t, idx = plain(S, at[todo], d[todo], left[todo], T)
        through = np.zeros(len(todo), bool)
        if masks:
            mat = np.where(idx >= 0, material[np.clip(idx, 0, None)], -1)
            for m, (plane, c8) in masks.items():
                k = np.flatnonzero(mat == m)
                if len(k) == 0:
                    continue
                u, v = R.hit_uv(S, at[todo[k]], d[todo[k]], t[k], idx[k], T)
                if "al_uv_swapped" in perturb:
                    u, v = v, u
                row, col = R.image_texel(plane, u, v, T)
                a8 = plane[row, col].astype(np.int64)
                clear = (a8 >= c8) if "al_inverted" in perturb else (a8 < c8)
                clear &= passes[todo[k]] < CAP  # the 65th masked hit of a query is opaque whatever its texel says
                through[k] = clear
                if tally is not None:
                    tally["masked_hits"] += len(k)
                    tally["passes"] += int(clear.sum())
                    tally["opaque"] += int((~clear).sum())
                    if samples is not None:
                        tally["sample_masked"][samples[todo[k]]] = True
        done = todo[~through]
        out_t[done] = total[done] + t[~through]
        out_idx[done] = idx[~through]
        go = todo[through]
        at[go] = at[go] + t[through][:, None] * d[go]
        total[go] += t[through]
        left[go] -= t[through]
        passes[go] += 1
        if on_pass is not None and len(go):
            on_pass(None if samples is None else samples[go], at[go], d[go])
        todo = go
    if tally is not None:
        tally["max_passes"] = max(tally["max_passes"], int(passes.max()) if n else 0)
        tally["shadow_queries" if shadow else "path_queries"] += n
        if shadow:
            tally["shadow_through"] += int((passes > 0).sum())
    if depth is not None and "al_counts_bounce" in perturb and not shadow and samples is not None:
        depth[samples] -= passes
    return out_t, out_idx


def _callers_samples(shadow):
    """the sample indices of the rays ref64.trace handed to closest_hit, and its depth counters, from its frame"""
    f = sys._getframe(1)
    while f is not None and not (f.f_code.co_name == "trace" and f.f_globals.get("__name__") == R.__name__):
        f = f.f_back
    if f is None:
        raise RuntimeError("ref64_alpha: ref64.trace is not among the callers of the installed closest_hit")
    loc = f.f_locals
    missing = [name for name in (("m", "k") if shadow else ("who", "depth")) if name not in loc]
    if missing:  # (a rename in ref64.trace: the tally and al_counts_bounce would silently do nothing)
        raise RuntimeError("ref64_alpha: ref64.trace has no local named %s any more" % ", ".join(missing))
    samples = loc["m"][loc["k"]] if shadow else loc["who"]
    return np.asarray(samples), loc.get("depth")


def _installed(call, perturb, tally, on_pass=None):
    """run `call` with the alpha-aware closest hit in ref64.closest_hit's place"""
    plain = R.closest_hit

    def aware(S, o, d, t_max, T):
        samples, depth = _callers_samples(not np.isscalar(t_max))
        assert len(samples) == len(o), (len(samples), len(o))
        tl = tally if (tally is not None and T is tally.get("dtype", np.float64)) else None
        t, idx = closest_hit(S, o, d, t_max, T, plain=plain, perturb=perturb, tally=tl, samples=samples, depth=depth,
                             on_pass=on_pass if T is np.float64 else None)
        if tl is not None and np.isscalar(t_max) and samples is not None:
            first = ~tl["first_seen"][samples]
            tl["first_t"][samples[first]] = t[first]
            tl["first_idx"][samples[first]] = idx[first]
            tl["first_seen"][samples] = True
        return t, idx

    R.closest_hit = aware
    try:
        return call()
    finally:
        R.closest_hit = plain


def _split(perturb):
    mine = tuple(p for p in perturb if p in PERTURBATIONS)
    return mine, tuple(p for p in perturb if p not in PERTURBATIONS)


def trace(S, words, perturb=(), tally=None, on_pass=None, **kw):
    """ref64.trace with alpha cutouts; tally: a dict of new_tally(len(words)) to count into (fp64 runs alone); on_pass: see
    closest_hit (fp64 runs alone)"""
    mine, rest = _split(perturb)
    return _installed(lambda: R.trace(S, words, perturb=rest, **kw), mine, tally, on_pass)


def reference(S, words, shutter=None):
    """ref64.reference with alpha cutouts: (rgb, stable, draws, ref64's tally, the alpha tally of the fp64 run)"""
    tally = new_tally(len(words))
    rgb, stable, draws, tl = _installed(lambda: R.reference(S, words, shutter), (), tally)
    return rgb, stable, draws, tl, summary(tally)


def summary(tally):
    """the tally with the shares the cases assert: of samples that met a masked hit, of masked hits that passed / were opaque"""
    out = {k: tally[k] for k in COUNTERS}
    n = len(tally["sample_masked"])
    out["samples"] = n
    out["masked_share"] = float(tally["sample_masked"].mean()) if n else 0.0
    out["pass_share"] = tally["passes"] / max(tally["masked_hits"], 1)
    out["opaque_share"] = tally["opaque"] / max(tally["masked_hits"], 1)
    out["first_t"], out["first_idx"] = tally["first_t"], tally["first_idx"]
    return out
