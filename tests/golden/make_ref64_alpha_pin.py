"""Writes tests/golden/ref64_alpha_pin.npz: what the fp64 reference returned on two alpha-cutout cases at the last
commit at which the alpha-aware closest hit was a module of its own, ref64_alpha.py, installed in ref64.closest_hit's place for
the length of a trace.  The cases are al_layers (several passes in one query) and al_lights (shadow rays through holes), 48 x 27,
the first sample of each pixel, at fp64 and fp32: the draws consumed, the SHA-256 of the signature array's bytes, the radiance
-- the fp64 run's rounded to float32, the fp32 run's as the SHA-256 of its bytes -- the seven integer counters of that module's
tally and the SHA-256 of first_idx, every sample's first opaque winner.  This script calls that module's trace(), so it runs on
an export of that commit (git archive <commit> tests ray-tracing-in-cuda_amd/scenes | tar -x -C <dir>), never on the working
tree under test; the package it renders the tables with is the built one of this tree:

    python tests/golden/make_ref64_alpha_pin.py <dir>/tests
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
import alpha_scenes as AS  # noqa: E402
import nee_scenes as NS  # noqa: E402
import ref64 as R  # noqa: E402
import ref64_alpha as RA  # noqa: E402

assert os.path.dirname(os.path.abspath(R.__file__)) == os.path.abspath(sys.argv[1]), R.__file__
rtmi = load_package()
N = NS.REF_W * NS.REF_H
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
cases, rgb64, draws = {}, [], [[], []]
for name in ("al_layers", "al_lights"):
    S = RA.ref_scene(AS.scene(rtmi, name))
    words = AS.inputs(rtmi, name)[0][:N]
    cases[name] = {}
    for k, (tag, dtype) in enumerate((("64", np.float64), ("32", np.float32))):
        tally = RA.new_tally(N)
        tally["dtype"] = dtype
        rgb, sig, dr = RA.trace(S, words, dtype=dtype, tally=tally)
        cases[name]["sig" + tag] = sha(sig)
        cases[name]["counters" + tag] = {c: int(tally[c]) for c in RA.COUNTERS}
        cases[name]["first_idx" + tag] = sha(tally["first_idx"].astype(np.int64))
        draws[k].append(dr.astype(np.int16))
        if tag == "64":
            rgb64.append(rgb.astype(np.float32))
        else:
            cases[name]["rgb32"] = sha(rgb)
np.savez_compressed(os.path.join(HERE, "ref64_alpha_pin.npz"), cases=np.array(json.dumps(cases)), rgb64=np.stack(rgb64), draws=np.array(draws))
