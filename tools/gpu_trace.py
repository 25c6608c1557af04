"""Ray-query throughput (rt_trace_hip): Mrays/s from rt_stats.kernel_ms, 1 warm-up + 5 timed runs, min and median.
Scenes: RTIOW (485 spheres), 20 000 spheres (gpu_big.py's), the 20 000-triangle mesh (tests/test_gpu_grid_all.py).
Batches of 1280 x 720 rays each: COHERENT (the camera's pixel-centre rays, row-major, and the same rays ordered by 8 x 8 pixel
tiles -- a work item is 64 consecutive rays, so a wave then traces a tile, as a render does) and INCOHERENT (origins uniform in
the scene's box without its ground sphere, isotropic directions), closest hit and occlusion.
Yardstick: the depth feature pass of the same scene at 1280 x 720 x 1 -- the same number of queries plus generator and
accumulation, on the render kernels -- and the ratio feature ms / coherent closest-hit ms (printed, nothing is asserted).
A last line per scene traces the tile-ordered batch 8 times over in one launch (7.4 M rays): a launch long enough for the
ramp of the persistent waves not to be most of it.
usage: gpu_trace.py [rtiow,spheres,mesh]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package
rtmi = load_package()
W, H = 1280, 720
N = W * H


def spheres20000():
    n = 20000
    rng = np.random.default_rng(n)
    half = 6.0 * (n / 5000.0) ** (1.0 / 3.0)
    sc = rtmi.Scene.new(W, H, 1, 20)
    sc.set_background((0.7, 0.8, 1.0), sky_gradient=True, defocus_blur=False)
    sc.camera((0, half * 0.6, 3.2 * half), (0, 0, 0), (0, 1, 0), 35.0)
    mats = [sc.lambertian(sc.solid_color(tuple(rng.uniform(0.1, 0.9, 3)))) for _ in range(6)]
    mats += [sc.metal(tuple(rng.uniform(0.5, 1.0, 3)), 0.1), sc.dielectric(1.5)]
    sc.sphere((0, -1000 - half, 0), 1000.0, mats[0])
    cen = rng.uniform(-half, half, (n, 3)); rad = rng.uniform(0.05, 0.2, n)
    for i in range(n):
        sc.sphere(tuple(cen[i]), float(rad[i]), mats[i % len(mats)])
    return sc


def mesh20000():
    from test_gpu_grid_all import height_field
    return height_field(rtmi, 100, W, H, 1, depth=20)


def camera_rays(sc):
    """pixel-centre rays, row 0 = bottom, no lens offset (fp32, as rtmi --pick builds them)"""
    cam = sc.get_camera()
    f = lambda k: np.array(getattr(cam, k)[:], np.float32)
    u = ((np.arange(W, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(W - 1)))[None, :, None]
    v = ((np.arange(H, dtype=np.float32) + np.float32(0.5)) * (np.float32(1.0) / np.float32(H - 1)))[:, None, None]
    d = (f("lower_left") + u * f("horizontal") + v * f("vertical") - f("origin")).astype(np.float32).reshape(-1, 3)
    return np.broadcast_to(f("origin"), d.shape).copy(), d


def by_tiles(o, d):
    """the row-major pixel rays reordered so that every 64 consecutive ones are an 8 x 8 tile"""
    idx = np.arange(N).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return o[idx], d[idx]


def random_rays(sc):
    import trace_cases as TC
    prims = sc.prims()
    boxes = [TC.prim_box(p) for p in prims if not (int(p["type"]) == 0 and abs(p["f"][3]) >= 100.0)]
    lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    rng = np.random.default_rng(1)
    o = lo + (hi - lo) * rng.uniform(0, 1, (N, 3))
    d = rng.normal(0, 1, (N, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return o.astype(np.float32), d.astype(np.float32)


def timed(fn):
    fn()
    ts = []
    for _ in range(5):
        st = rtmi.Stats(); fn(st); ts.append(st.kernel_ms)
    return min(ts), float(np.median(ts)), st.kernel_variant


SCENES = {"rtiow": lambda: rtmi.Scene.rtiow(7, W, H, 1, 50), "spheres": spheres20000, "mesh": mesh20000}
for name in (sys.argv[1].split(",") if len(sys.argv) > 1 else list(SCENES)):
    sc = SCENES[name]()
    f_min, f_med, f_kv = timed(lambda st=None: sc.render_feature(rtmi.FEATURE_DEPTH, rtmi.Opts(seed=1, sample_count=1), st))
    print(f"{name}: {sc.info.num_prims} primitives; depth feature pass {W}x{H}x1, kernel variant {f_kv}: min {f_min:.3f} ms, median {f_med:.3f} ms "
          f"({N / f_min / 1e3:.0f} Mqueries/s)", flush=True)
    for batch, (o, d) in (("coherent", camera_rays(sc)), ("coh. tiles", by_tiles(*camera_rays(sc))), ("incoherent", random_rays(sc))):
        for occluded in (False, True):
            t_min, t_med, kv = timed(lambda st=None: sc.trace(o, d, occluded=occluded, stats=st))
            hits = sc.trace(o, d, occluded=True).mean()
            line = (f"  {batch:10s} {'occlusion' if occluded else 'closest  '} layout {kv & ~rtmi.TRACE_LAYOUT}: min {t_min:.3f} ms, median {t_med:.3f} ms, "
                    f"{N / t_min / 1e3:.0f} Mrays/s, {100 * hits:.0f} % hit")
            if batch != "incoherent" and not occluded:
                line += f"; depth pass / query = {f_min / t_min:.2f}"
            print(line, flush=True)
    o8, d8 = (np.tile(a, (8, 1)) for a in by_tiles(*camera_rays(sc)))
    t_min, t_med, kv = timed(lambda st=None: sc.trace(o8, d8, stats=st))
    print(f"  coh. tiles x 8 closest: min {t_min:.3f} ms, median {t_med:.3f} ms, {8 * N / t_min / 1e3:.0f} Mrays/s", flush=True)
