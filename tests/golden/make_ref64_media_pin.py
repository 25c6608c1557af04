"""Writes tests/golden/ref64_media_pin.npz: what the fp64 reference returned on the anisotropic-media cases, their
isotropic twins, the media light-sampling cases (7z) and the plain media cases (7f) at the last commit at which 7y and 7z were
path tracers of their own (ref64_phase.trace, ref64_media_nee.trace) beside ref64.trace -- 24 x 14, at fp64 and fp32; four
samples of each pixel on the anisotropic cases and their twins, the first sample of each pixel (as the other pins take it) on the
rest: twenty-two float32 images at four samples each do not fit the size the earlier pins set.  Per case: the draws consumed by
both runs (exact), which samples took the same branches at fp32 (packed bits), the counts of that commit's tally, the fp64
radiance rounded to float32, and the SHA-256 of the fp32 run's radiance.  The signature's layout differed between the three
tracers, so what a signature says is pinned through the flag and the counts.  This script calls that commit's modules, so it
runs on an export of it (git archive <commit> tests ray-tracing-in-cuda_amd/scenes | tar -x -C <dir>), never on the working tree
under test; the package it renders the tables with is the built one of this tree:

    python tests/golden/make_ref64_media_pin.py <dir>/tests
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from __graft_entry__ import load_package  # noqa: E402
import media_nee_scenes as MN  # noqa: E402
import media_scenes as MS  # noqa: E402
import nee_scenes as NS  # noqa: E402
import phase_scenes as PH  # noqa: E402
import ref64 as R  # noqa: E402
import ref64_media_nee as RM  # noqa: E402
import ref64_phase as RP  # noqa: E402

assert os.path.dirname(os.path.abspath(R.__file__)) == os.path.abspath(sys.argv[1]), R.__file__
rtmi = load_package()
W, H = 24, 14
SIZE = {}  # case -> (W, H) where the small frame does not hold the vertices the case is there for
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def small(sc, key):
    w, h = SIZE.get(key, (W, H))
    sc.override(width=w, height=h)
    return sc


def media_counts(S):
    return lambda sig: {k: R.tally(sig, S)[k] for k in R.MEDIA_KEYS}


# group -> (seed, draws, samples per pixel, {case: (scene, trace(S, words, dtype), tally(S) -> (sig -> counts), the counts that must be positive)})
GROUPS = {
    "phase": (PH.REF_SEED, PH.REF_DRAWS, 4, {n: (b(rtmi), lambda S, w, T, sc: RP.trace(S, RP.stored_g(sc), w, dtype=T), lambda S: RP.tally, ("anisotropic_events",))
                                          for n, b in PH.ref_cases().items()}),
    "twin": (PH.REF_SEED, PH.REF_DRAWS, 4, {n: (PH.isotropic_twin(b(rtmi)), lambda S, w, T, sc: R.trace(S, w, dtype=T), media_counts, ("medium_events",))
                                         for n, b in PH.ref_cases().items()}),
    "media_nee": (MN.REF_SEED, NS.REF_DRAWS, 1, {n: (MN.scene(rtmi, n), lambda S, w, T, sc: RM.trace(S, [sc.medium_phase(i) for i in range(len(sc.media()))], w, dtype=T),
                                                  lambda S: RM.tally,
                                                  ("medium_light_samples",) + (("occluded_through_media",) if n == "medium inside a glass shell" else ())
                                                  + (("anisotropic_events",) if "g = " in n else ()))
                                              for n in MN.ref_cases()}),
    "media": (MN.REF_SEED, NS.REF_DRAWS, 1, {n: (b(rtmi), lambda S, w, T, sc: R.trace(S, w, dtype=T), media_counts, ("medium_events",)) for n, b in MS.ref_cases().items()}),
}
cases, rgb64, draws64, draws32, stable = {}, [], [], [], []
for group, (seed, n_draws, K, members) in GROUPS.items():
    for name, (sc, trace, counts, needs) in members.items():
        key = group + "/" + name
        sc = small(sc, key)
        S = R.RefScene(sc)
        words = R.uniforms(rtmi, seed, sc.info.width, sc.info.height, 0, K, n_draws)
        rgb, sig, dr = trace(S, words, np.float64, sc)
        r32, s32, d32 = trace(S, words, np.float32, sc)
        w = max(sig.shape[1], s32.shape[1])
        pad = lambda a: np.pad(a, ((0, 0), (0, w - a.shape[1])), constant_values=R.NONE)
        tally = counts(S)(sig)
        for k in needs:  # the vertices the case is pinned for are there
            assert tally[k] > 0, (key, k, tally)
        assert dr.max() <= n_draws and d32.max() <= n_draws and len(words) % 8 == 0, key  # (whole bytes of flags per case)
        cases[key] = dict(width=sc.info.width, height=sc.info.height, samples=K, seed=seed, draws=n_draws, tally=tally, rgb32=sha(r32))
        rgb64.append(rgb.astype(np.float32))
        draws64.append(dr.astype(np.int16))
        draws32.append((d32 - dr).astype(np.int16))
        stable.append(np.packbits((pad(sig) == pad(s32)).all(axis=1)))
        print(key, tally)
np.savez_compressed(os.path.join(HERE, "ref64_media_pin.npz"), cases=np.array(json.dumps(cases)), rgb64=np.concatenate(rgb64),
                    draws64=np.concatenate(draws64), draws32_minus_64=np.concatenate(draws32), stable=np.concatenate(stable))
