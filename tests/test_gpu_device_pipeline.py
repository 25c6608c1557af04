"""The frame pipeline on DEVICE buffers on a caller's stream -- rt_render_hip_device, rt_render_hip_adaptive_device,
rt_render_hip_feature_device, rt_denoise_hip_device, rt_display_hip_device -- held to the host entries bit for bit:
  a. each device entry alone, on the null stream and on a torch stream, asynchronous and with its stats;
  b. stream order: the call enqueued behind a long stretch of torch work, its inputs written and its outputs read by that
     stream alone, one synchronisation at the very end;
  c. the whole chain on one stream, and three chains of two frame sizes queued without a synchronisation between them;
  d. a scene edited between two asynchronous renders, and a scene and its clone on two streams.
The host entries pass the null stream and kept buffers of their own and synchronise at once, so none of this shows there.
Every float output starts as NaN and every integer output as -1 (bytes: 255), so an element nobody wrote shows."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_adaptive import _pick_threshold

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_DIR = os.path.join(ROOT, "ray-tracing-in-cuda_amd", "scenes")
SEED = 21
MIN_SPP, MAX_SPP = 4, 64  # the adaptive schedule: 4, 8, 16, 32, 64 (as tests/test_gpu_adaptive.py; the scenes' own spp is 16)
FEATURE_SPP = 8
ACES = 2
SHOW = dict(tonemap=ACES, exposure=0.37, bloom_strength=0.6, bloom_threshold=1.0, bloom_levels=2)
DELAY_MATMULS = 72  # the delay of the stream-order tests: see test_stream_order


def mixed(rtmi):
    """wide tables, the light-sampling kernel"""
    sc = rtmi.Scene.load(os.path.join(SCENE_DIR, "mixed_emissive.json"))
    sc.override(64, 36, 16)
    sc.set_light_sampling(True)
    return sc


def rtiow(rtmi):
    """compact tables (a feature pass runs the linear scan), partial 8 x 8 tiles on both axes"""
    return rtmi.Scene.rtiow(7, 100, 60, 16, 20)


MAKERS = {"mixed": mixed, "rtiow": rtiow}
NAMES = list(MAKERS)


def feature_opts(rtmi, **kw):
    return rtmi.Opts(seed=SEED, sample_count=FEATURE_SPP, **kw)


def host_chain(rtmi, sc, rgb, spp_map, feat):
    """denoiser and display stage through the host entries: (denoised sums, display rgb, display bytes)"""
    den = rtmi.denoise(rgb, sc.spp, *feat, FEATURE_SPP, spp_map=spp_map)
    out, out8 = rtmi.display(den, sc.spp, spp_map=spp_map, **SHOW)
    return den, out, out8


@pytest.fixture(scope="module")
def host(rtmi):
    """What the host entries give for both scenes, computed once and read-only from then on.  It also leaves every scene's
    tables resident and the per-device scratch of the denoiser and the display stage at its largest size."""
    out = {}
    for name, make in MAKERS.items():
        sc = make(rtmi)
        r = SimpleNamespace(sc=sc, h=sc.height, w=sc.width)
        r.img = sc.render(rtmi.Opts(seed=SEED))
        r.thr, r.ad_img, r.ad_map, r.ad_st = _pick_threshold(rtmi, sc, MIN_SPP, MAX_SPP, rtmi.Opts(seed=SEED))
        r.feat = [sc.render_feature(f, feature_opts(rtmi)) for f in range(3)]
        r.plain = host_chain(rtmi, sc, r.img, None, r.feat)
        r.adaptive = host_chain(rtmi, sc, r.ad_img, r.ad_map, r.feat)
        for a in (r.img, r.ad_img, r.ad_map, *r.feat, *r.plain, *r.adaptive):
            a.setflags(write=False)
        out[name] = r
    return out


def same(got, want):
    """equal bits (a device tensor or an array against an array)"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.float32:
        return np.array_equal(got.view(np.uint32), want.view(np.uint32))
    return np.array_equal(got, want)


def nans(torch, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")


def minus_ones(torch, *shape, dtype=None):
    dtype = dtype or torch.int32
    return torch.full(shape, 255 if dtype == torch.uint8 else -1, dtype=dtype, device="cuda:0")


def on_device(torch, a):
    return torch.from_numpy(np.array(a)).to("cuda:0")  # (a copy: the references are read-only)


def make_stream(torch, kind):
    return torch.cuda.Stream() if kind == "torch" else None


def handle(stream):
    return stream.cuda_stream if stream is not None else 0


def adaptive_without_stats(rtmi, sc, thr, d_rgb, d_map, stream):
    """Scene.render_adaptive_device always asks for the schedule; st == NULL goes straight through the C ABI"""
    a, o = rtmi.Adaptive(min_spp=MIN_SPP, max_spp=MAX_SPP, threshold=thr), rtmi.Opts(seed=SEED)
    rc = rtmi._lib.rt_render_hip_adaptive_device(sc._h, C.byref(o), C.byref(a), C.c_void_p(d_rgb.data_ptr()),
                                                 C.c_void_p(d_map.data_ptr()), C.c_void_p(handle(stream)), None)
    assert rc == 0, rtmi._lib.rt_last_error().decode()


# ---- a. each device entry equals its host entry

@pytest.mark.parametrize("with_stats", [False, True], ids=["async", "stats"])
@pytest.mark.parametrize("kind", ["null", "torch"])
@pytest.mark.parametrize("name", NAMES)
def test_adaptive_device_equals_host(rtmi, host, name, kind, with_stats):
    import torch
    r = host[name]
    assert len(np.unique(r.ad_map)) >= 2 and (r.ad_map == MAX_SPP).any()
    d_rgb, d_map = nans(torch, r.h, r.w, 3), minus_ones(torch, r.h, r.w)
    stream = make_stream(torch, kind)
    torch.cuda.synchronize()
    if with_stats:
        st = r.sc.render_adaptive_device(r.thr, d_rgb.data_ptr(), d_map.data_ptr(), MIN_SPP, MAX_SPP, handle(stream),
                                         rtmi.Opts(seed=SEED))
    else:
        adaptive_without_stats(rtmi, r.sc, r.thr, d_rgb, d_map, stream)
    torch.cuda.synchronize()
    assert same(d_map, r.ad_map) and same(d_rgb, r.ad_img)
    if with_stats:
        want = r.ad_st
        assert (st.passes, st.tiles, st.samples) == (want.passes, want.tiles, want.samples)
        assert list(st.spp_after[:st.passes]) == list(want.spp_after[:want.passes])
        assert list(st.active[:st.passes]) == list(want.active[:want.passes])
        assert st.samples == int(r.ad_map.astype(np.int64).sum()) and st.kernel_ms > 0


@pytest.mark.parametrize("kind", ["null", "torch"])
@pytest.mark.parametrize("name", NAMES)
def test_feature_device_equals_host(rtmi, host, name, kind):
    import torch
    r = host[name]
    sc = r.sc
    cases = [(f, dict(variant=layout)) for f in range(3) for layout in (0, 16)]
    cases += [(f, dict(tile_first=1, tile_stride=3, tile_rows=4)) for f in range(3)]  # a row shard
    cases += [(f, dict(sample_first=2, sample_count=3)) for f in range(3)]            # a sample split
    stream = make_stream(torch, kind)
    for feature, kw in cases:
        opts = rtmi.Opts(**dict(dict(seed=SEED, sample_count=FEATURE_SPP), **kw))
        rows = sc.shard_rows(opts)
        assert 0 < rows and (rows < r.h) == ("tile_stride" in kw)
        want = sc.render_feature(feature, opts)
        for stats in (None, rtmi.Stats()):
            d_sum = nans(torch, rows, r.w, 3)
            torch.cuda.synchronize()
            sc.render_feature_device(feature, d_sum.data_ptr(), handle(stream), opts, stats)
            torch.cuda.synchronize()
            assert same(d_sum, want), (feature, kw, stats is not None)
            if stats is not None:
                assert stats.kernel_variant & 512 and stats.local_rows == rows and stats.kernel_ms > 0


@pytest.mark.parametrize("kind", ["null", "torch"])
@pytest.mark.parametrize("name", NAMES)
def test_denoise_device_equals_host(rtmi, host, name, kind):
    import torch
    r = host[name]
    d_feat = [on_device(torch, a) for a in r.feat]
    stream = make_stream(torch, kind)
    for rgb, spp_map in ((r.img, None), (r.ad_img, r.ad_map)):
        d_rgb = on_device(torch, rgb)
        d_map = on_device(torch, spp_map) if spp_map is not None else None
        for iterations in (0, 1, None):
            want = rtmi.denoise(rgb, r.sc.spp, *r.feat, FEATURE_SPP, spp_map=spp_map, iterations=iterations)
            if iterations == 0:
                assert same(want, rgb)
            par = rtmi.Denoise(iterations=rtmi.DENOISE_DEFAULT_ITERATIONS if iterations is None else iterations)
            for timing in (None, []):
                d_out = nans(torch, r.h, r.w, 3)
                torch.cuda.synchronize()
                rtmi.denoise_device(r.w, r.h, d_rgb.data_ptr(), r.sc.spp, *[t.data_ptr() for t in d_feat], FEATURE_SPP,
                                    d_out.data_ptr(), handle(stream), d_spp_map=d_map.data_ptr() if d_map is not None else None,
                                    params=par, timing=timing)
                torch.cuda.synchronize()
                assert same(d_out, want), (spp_map is not None, iterations, timing)
                if timing is not None:
                    assert len(timing) == 1 and (timing[0] > 0) == (iterations != 0)


# ---- b. stream order

_delay_state = {}


def delay(torch, n=DELAY_MATMULS):
    """plain torch work on the current stream: a chain of n 4096 x 4096 fp32 matmuls (the matrix is made, and the matmul
    warmed, once, on the null stream and synchronised)"""
    if "x" not in _delay_state:
        with torch.cuda.stream(torch.cuda.default_stream()):
            x = torch.full((4096, 4096), 1.0 / 4096.0, dtype=torch.float32, device="cuda:0")
            _delay_state["warm"] = x @ x
        torch.cuda.synchronize()
        _delay_state["x"] = x
    x = y = _delay_state["x"]
    for _ in range(n):
        y = y @ x
    return y


ENTRIES = ["render", "adaptive", "feature", "denoise", "display"]
MUST_BE_BUSY = {"denoise", "display"}  # these calls enqueue kernels and nothing else


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", NAMES)
def test_stream_order(rtmi, host, name, entry):
    """The call is enqueued on a torch stream behind `delay`; the same stream then writes the real inputs over NaN, runs the
    call, clones the outputs and zeroes the originals; one synchronisation at the end.  A step of the call that ran on another
    stream, or that read an input when the call was made, meets the NaN or loses to the zeroing.  The two render entries are
    called twice, first into a scrap tensor, so that a clear issued on another stream has earlier queued work to lose to.

    The test can only fail while the delay is still running when the call returns.  For the denoiser (no timing) and the
    display stage (no stats, auto_key 0) that is asserted; for the three render entries it is printed (pytest -s): a first
    upload and the adaptive read-back may rightly wait for the stream.

    Measured on an MI355X, on an idle stream, tables resident (host time of the call / hipEvent time around it, the larger of
    the two scenes): render 0.016 / 0.60 ms (0.07 / 0.84 the first time), feature pass 0.015 / 0.14 ms, denoiser 0.018 /
    0.053 ms, no pass 0.006 / 0.010 ms, display stage 0.026 / 0.031 ms; the adaptive render, which waits for its passes,
    2.9 / 2.9 ms.  One 4096 x 4096 fp32 matmul takes 0.91 ms; the delay of DELAY_MATMULS = 72 takes 65.6 ms: 22 times the
    adaptive call, 78 times the longest of the others (DESIGN.md section 7d has the table)."""
    import torch
    r = host[name]
    sc, h, w = r.sc, r.h, r.w
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    delay(torch, 1)  # (warm)
    real, ins, outs, want = [], [], [], []
    if entry == "denoise":
        real = [on_device(torch, a) for a in (r.ad_img, r.ad_map, *r.feat)]
        want = [r.adaptive[0], r.ad_img]  # the default passes, and no pass
    elif entry == "display":
        real = [on_device(torch, a) for a in (r.adaptive[0], r.ad_map)]
        want = [r.adaptive[1], r.adaptive[2]]
    elif entry == "render":
        want = [r.img]
    elif entry == "adaptive":
        want = [r.ad_img, r.ad_map]
    else:
        want = [r.feat[1]]
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        ins = [nans(torch, *t.shape) if t.dtype == torch.float32 else minus_ones(torch, *t.shape) for t in real]
        outs = [nans(torch, *a.shape) if a.dtype == np.float32 else minus_ones(torch, *a.shape, dtype=getattr(torch, a.dtype.name))
                for a in want]
        scrap = nans(torch, h, w, 3)
        torch.cuda.synchronize()
        t0.record()
        delay(torch)
        t1.record()
        for dst, src in zip(ins, real):
            dst.copy_(src, non_blocking=True)
        busy = []
        if entry == "render":
            for dst in (scrap, outs[0]):
                sc.render_device(rtmi.Opts(seed=SEED), dst.data_ptr(), s)
                busy.append(not stream.query())
        elif entry == "adaptive":
            adaptive_without_stats(rtmi, sc, r.thr, outs[0], outs[1], stream)
            busy.append(not stream.query())
        elif entry == "feature":
            for dst in (scrap, outs[0]):
                sc.render_feature_device(rtmi.FEATURE_NORMAL, dst.data_ptr(), s, feature_opts(rtmi))
                busy.append(not stream.query())
        elif entry == "denoise":
            for dst, it in ((outs[0], rtmi.DENOISE_DEFAULT_ITERATIONS), (outs[1], 0)):
                rtmi.denoise_device(w, h, ins[0].data_ptr(), sc.spp, *[t.data_ptr() for t in ins[2:]], FEATURE_SPP, dst.data_ptr(), s,
                                    d_spp_map=ins[1].data_ptr(), params=rtmi.Denoise(iterations=it))
                busy.append(not stream.query())
        else:
            rtmi.display_device(w, h, ins[0].data_ptr(), sc.spp, outs[0].data_ptr(), outs[1].data_ptr(), s,
                                d_spp_map=ins[1].data_ptr(), params=rtmi.Display(**SHOW))
            busy.append(not stream.query())
        clones = [t.clone() for t in outs]
        for t in outs:
            t.zero_()
    stream.synchronize()
    print(f"stream order, {name} {entry}: delay {t0.elapsed_time(t1):.1f} ms, stream still busy after the call: {busy}")
    if entry in MUST_BE_BUSY:
        assert all(busy), "the delay was over before the call returned: the test saw nothing"
    for k, (got, exp) in enumerate(zip(clones, want)):
        assert same(got, exp), (entry, k)
    for t in outs:
        assert not t.any()


# ---- c. the chain

def device_chain(rtmi, torch, sc, thr, s, adaptive):
    """render (adaptive or plain), three feature passes, denoiser, display stage: enqueued on the stream with handle `s`,
    nothing synchronised here.  Returns the tensors (display rgb, display bytes)."""
    h, w = sc.height, sc.width
    d_rgb, d_den, d_out = nans(torch, h, w, 3), nans(torch, h, w, 3), nans(torch, h, w, 3)
    d_feat = [nans(torch, h, w, 3) for _ in range(3)]
    d_out8 = minus_ones(torch, h, w, 3, dtype=torch.uint8)
    d_map = minus_ones(torch, h, w) if adaptive else None
    if adaptive:
        sc.render_adaptive_device(thr, d_rgb.data_ptr(), d_map.data_ptr(), MIN_SPP, MAX_SPP, s, rtmi.Opts(seed=SEED))
    else:
        sc.render_device(rtmi.Opts(seed=SEED), d_rgb.data_ptr(), s)
    for f in range(3):
        sc.render_feature_device(f, d_feat[f].data_ptr(), s, feature_opts(rtmi))
    m = d_map.data_ptr() if adaptive else None
    rtmi.denoise_device(w, h, d_rgb.data_ptr(), sc.spp, *[t.data_ptr() for t in d_feat], FEATURE_SPP, d_den.data_ptr(), s, d_spp_map=m)
    rtmi.display_device(w, h, d_den.data_ptr(), sc.spp, d_out.data_ptr(), d_out8.data_ptr(), s, d_spp_map=m,
                        params=rtmi.Display(**SHOW))
    # (the tensors of the intermediate stages stay alive with the outputs until the caller has synchronised)
    return d_out, d_out8, (d_rgb, d_den, d_feat, d_map)


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "plain"])
@pytest.mark.parametrize("name", NAMES)
def test_chain_equals_host_chain(rtmi, host, name, adaptive):
    import torch
    r = host[name]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        delay(torch)
        d_out, d_out8, keep = device_chain(rtmi, torch, r.sc, r.thr, stream.cuda_stream, adaptive)
    stream.synchronize()
    _, want, want8 = r.adaptive if adaptive else r.plain
    assert same(d_out, want) and same(d_out8, want8)


@pytest.mark.parametrize("adaptive", [True, False], ids=["adaptive", "plain"])
def test_three_chains_queued_on_one_stream(rtmi, host, adaptive):
    """64 x 36, 100 x 60, 64 x 36 again behind one delay, no synchronisation between the chains, on scene objects that have
    rendered nothing yet: their tables are uploaded and their accumulators allocated and regrown (the adaptive planes are the
    larger ones) under queued work.  The per-device scratch of the denoiser and the display stage regrows here only when
    nothing larger ran in this process before."""
    import torch
    stream = torch.cuda.Stream()
    scenes = [MAKERS[n](rtmi) for n in ("mixed", "rtiow")]
    order = [("mixed", scenes[0]), ("rtiow", scenes[1]), ("mixed", scenes[0])]
    with torch.cuda.stream(stream):
        delay(torch)
        runs = [device_chain(rtmi, torch, sc, host[n].thr, stream.cuda_stream, adaptive) for n, sc in order]
    stream.synchronize()
    for (n, _), (d_out, d_out8, keep) in zip(order, runs):
        _, want, want8 = host[n].adaptive if adaptive else host[n].plain
        assert same(d_out, want) and same(d_out8, want8), n
    assert same(runs[2][0], runs[0][0].cpu().numpy()) and same(runs[2][1], runs[0][1].cpu().numpy())


# ---- d. edits and clones between asynchronous calls

def test_scene_edited_between_two_asynchronous_renders(rtmi):
    """The second call must upload the edited tables, in stream order behind the first call's kernels, and the first must
    have taken its own before the edit (its upload reads pageable memory the edit rewrites)."""
    import torch
    sc = mixed(rtmi)
    before = sc.clone()
    h, w = sc.height, sc.width
    opts = rtmi.Opts(seed=SEED)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        one, two = nans(torch, h, w, 3), nans(torch, h, w, 3)
        delay(torch)
        sc.render_device(opts, one.data_ptr(), stream.cuda_stream)
        sc.sphere((1.5, 0.5, 3.0), 0.5, sc.lambertian((0.8, 0.1, 0.1)))
        sc.set_background((0.4, 0.5, 0.9), sky_gradient=False, defocus_blur=True)
        sc.render_device(opts, two.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    # the references come from clones, whose tables are uploaded afresh: the edited object's own host render would share a
    # stale upload with the call under test
    want_one, want_two = before.render(opts), sc.clone().render(opts)
    background_only = before.clone()
    background_only.set_background((0.4, 0.5, 0.9), sky_gradient=False, defocus_blur=True)
    assert not np.array_equal(want_two, background_only.render(opts))  # (the new sphere is in view: the tables matter)
    assert same(one, want_one)
    assert same(two, want_two)
    assert same(sc.render(opts), want_two)


def test_scene_and_clone_on_two_streams(rtmi):
    """include/rtmi.h: renders of one rt_scene on a device share a stream; rt_scene_clone gives independent concurrent frames"""
    import torch
    opts = rtmi.Opts(seed=SEED)
    for make in MAKERS.values():
        sc = make(rtmi)
        twin = sc.clone()
        h, w = sc.height, sc.width
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        bufs = []
        for scene, stream in zip((sc, twin), streams):
            with torch.cuda.stream(stream):
                buf = nans(torch, h, w, 3)
                delay(torch, DELAY_MATMULS // 4)
                scene.render_device(opts, buf.data_ptr(), stream.cuda_stream)
            bufs.append(buf)
        torch.cuda.synchronize()
        want = sc.render(opts)
        assert same(twin.render(opts), want)
        assert same(bufs[0], want) and same(bufs[1], want)
