"""Writes tests/golden/ref64_trace_pin.npz: what ref64.trace returned, at the commit to pin, on the three glossy-free cases of
test_glossy._existing_cases (48 x 27, the first sample of each pixel), at fp64 and fp32: rgb, the draws consumed and the
SHA-256 of the signature array's bytes.  It imports the tracer, the scenes and the cases from the tests/ directory it is
given -- an export of the commit to pin (git archive <commit> tests ray-tracing-in-cuda_amd/scenes | tar -x -C <dir>), never
the working tree under test; the package it renders the tables with is the built one of this tree:

    python tests/golden/make_ref64_trace_pin.py <dir>/tests
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.abspath(sys.argv[1]))
from __graft_entry__ import load_package  # noqa: E402
import nee_scenes as NS  # noqa: E402
import ref64 as R  # noqa: E402
from test_glossy import _existing_cases  # noqa: E402

assert os.path.dirname(os.path.abspath(R.__file__)) == os.path.abspath(sys.argv[1]), R.__file__
rtmi = load_package()
out = {}
for name, (sc, seed) in _existing_cases(rtmi).items():
    words = R.uniforms(rtmi, seed, NS.REF_W, NS.REF_H, 0, 1, NS.REF_DRAWS)
    for tag, dtype in (("64", np.float64), ("32", np.float32)):
        rgb, sig, draws = R.trace(R.RefScene(sc), words, dtype=dtype)
        out[f"{name}/rgb{tag}"], out[f"{name}/draws{tag}"] = rgb, draws.astype(np.int32)
        out[f"{name}/sig{tag}"] = np.array(hashlib.sha256(np.ascontiguousarray(sig).tobytes()).hexdigest())
np.savez_compressed(os.path.join(HERE, "ref64_trace_pin.npz"), **out)
