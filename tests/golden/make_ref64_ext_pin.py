"""Writes tests/golden/ref64_ext_pin.npz: what the fp64 reference returned, at the commit to pin, on one case of each of the
eight extensions of DESIGN 7n-7u (48 x 27, the first sample of each pixel), at fp64 and fp32: the draws consumed, the SHA-256
of the signature array's bytes, and the radiance -- the fp64 run's rounded to float32; the fp32 run's as the SHA-256 of its
bytes and, on the analytic-light case, whose light samples are a handful of roundings from the pinned ones by design, as its
distance in float32 steps from the fp64 run's (int16), from which the test rebuilds it exactly.  (Sixteen float32 images do not
fit the size the first pin set.)  The commit to pin is the last one at which each extension was a module of its own that
wrapped ref64's functions for the length of a trace: this script calls those modules' trace(), so it runs on an export of that
commit (git archive <commit> tests ray-tracing-in-cuda_amd/scenes | tar -x -C <dir>), never on the working tree under test;
the package it renders the tables with is the built one of this tree:

    python tests/golden/make_ref64_ext_pin.py <dir>/tests
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
import analytic_light_scenes as ALS  # noqa: E402
import bump_scenes as BS  # noqa: E402
import glass_scenes as GS  # noqa: E402
import mesh_light_scenes as ML  # noqa: E402
import nee_scenes as NS  # noqa: E402
import noise_scenes as NSC  # noqa: E402
import normal_map_scenes as NMS  # noqa: E402
import pbr_scenes as PS  # noqa: E402
import quad_scenes as QS  # noqa: E402
import ref64 as R  # noqa: E402
import ref64_analytic_lights as RA  # noqa: E402
import ref64_bump as RB  # noqa: E402
import ref64_glass as RG  # noqa: E402
import ref64_mesh_lights as RM  # noqa: E402
import ref64_noise as RN  # noqa: E402
import ref64_normal_map as RNM  # noqa: E402
import ref64_pbr as RP  # noqa: E402

assert os.path.dirname(os.path.abspath(R.__file__)) == os.path.abspath(sys.argv[1]), R.__file__
rtmi = load_package()
N = NS.REF_W * NS.REF_H
first = lambda words: words if not isinstance(words, tuple) else words[0]
# family -> (case, its scene, its uniforms, the wrapper module's trace(scene, RefScene, words, dtype))
CASES = {
    "mesh_lights": (ML.MIXED, ML.scene(rtmi, ML.MIXED), ML.inputs(rtmi), lambda sc, S, w, T: RM.trace(S, w, dtype=T)),
    "noise": ("noise_lights", NSC.scene(rtmi, "noise_lights"), NSC.inputs(rtmi, "noise_lights"), lambda sc, S, w, T: RN.trace(sc, S, w, dtype=T)),
    "bump": ("bump_lights", BS.scene(rtmi, "bump_lights"), BS.inputs(rtmi, "bump_lights"), lambda sc, S, w, T: RB.trace(sc, S, w, dtype=T)),
    "quads": (QS.CORNELL, QS.scene(rtmi, QS.CORNELL), QS.inputs(rtmi, QS.CORNELL), lambda sc, S, w, T: QS.trace(sc, S, w, dtype=T)),
    "glass": ("glass_lights", GS.scene(rtmi, "glass_lights"), GS.inputs(rtmi, "glass_lights"), lambda sc, S, w, T: RG.trace(S, w, dtype=T, sc=sc)),
    "analytic_lights": ("two spots + quad + sphere", ALS.scene(rtmi, "two spots + quad + sphere"), ALS.inputs(rtmi),
                        lambda sc, S, w, T: RA.trace(RA.attach(S, sc), w, dtype=T, sc=sc, report={} if T is np.float32 else None)),
    "pbr": ("half-metal floor", PS.scene(rtmi, "half-metal floor"), PS.inputs(rtmi), lambda sc, S, w, T: RP.trace(S, w, sc, dtype=T)),
    "normal_map": ("nm_fog", NMS.scene(rtmi, "nm_fog"), NMS.inputs(rtmi, "nm_fog"), lambda sc, S, w, T: RNM.trace(sc, S, w, dtype=T)),
}
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
cases, rgb64, draws = {}, [], [[], []]
for family, (name, sc, words, trace) in CASES.items():
    cases[family] = dict(case=name)
    for k, (tag, dtype) in enumerate((("64", np.float64), ("32", np.float32))):
        rgb, sig, dr = trace(sc, R.RefScene(sc), first(words)[:N], dtype)
        cases[family]["sig" + tag] = sha(sig)
        draws[k].append(dr.astype(np.int16))
        if tag == "64":
            rgb64.append(rgb.astype(np.float32))
        else:
            cases[family]["rgb32"] = sha(rgb)
            if family == "analytic_lights":
                steps = rgb.view(np.int32).astype(np.int64) - rgb64[-1].view(np.int32)
                assert np.abs(steps).max() < 2 ** 15
                analytic_steps = steps.astype(np.int16)
np.savez_compressed(os.path.join(HERE, "ref64_ext_pin.npz"), cases=np.array(json.dumps(cases)), rgb64=np.stack(rgb64), draws=np.array(draws),
                    analytic_rgb32_steps=analytic_steps)
