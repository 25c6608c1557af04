"""What the GPU tests of the per-sample comparison share (test_gpu_nee_reference.py states the criteria (a)-(d)): the package
with a device behind it, the one-sample frames of a kernel family, the verdict on a comparison, and the refusal check.  Plain
functions: the fixtures stay in the test files, which skip each on its own."""
import os
import sys

import numpy as np
import pytest

import ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu_package():
    """the package, or a skip where there is no device"""
    sys.path.insert(0, ROOT)
    from __graft_entry__ import load_package
    mod = load_package()
    if mod.device_count() < 1:
        pytest.skip("no HIP device")
    return mod


def kernel_samples(rtmi, sc, seed, k, mask, family, variant=0):
    """[k x H x W][3]: the radiance of every sample, from one-sample frames; the kernel family is checked on each, and the
    layout where one is asked for (variant: 0 is the scene's own)"""
    out = []
    for i in range(k):
        st = rtmi.Stats()
        out.append(sc.render(rtmi.Opts(seed=seed, sample_first=i, sample_count=1, variant=variant), st))
        assert st.kernel_variant & mask == family, (st.kernel_variant, family)
        if variant:
            assert st.kernel_variant & ~mask == variant, (st.kernel_variant, variant)
    return np.stack(out).reshape(-1, 3).astype(np.float64)


def assert_agreement(name, j, b):
    """the verdict on R.judge's figures of a kernel (j) and of the plain kernel on the scene's plain twin (b); prints the row"""
    print("\n" + R.row(name, j, b["share_stable"]))
    assert j["flips"] <= 0.01, j["flips"]
    assert j["share"] >= 0.97, j                                                                   # (a)
    assert j["share_stable"] >= b["share_stable"] - 0.005, (j["share_stable"], b["share_stable"])  # (b)
    assert j["bias_ok"], (j["mean_diff"], j["z"])                                                  # (c)


def assert_perturbation_noticed(good, bad):
    """(d): the kernel agrees with the reference and is far from 97 % against a reference with a deliberate mistake"""
    assert good["share"] >= 0.97 and bad["share"] < 0.97, (good["share"], bad["share"])


def refused(rtmi, call):
    with pytest.raises(rtmi.RtmiError) as e:
        call()
    assert e.value.status == 1, str(e.value)  # RT_ERR_ARG
    return str(e.value)
