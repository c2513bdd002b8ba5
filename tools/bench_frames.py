"""Frame export: a 240-view video (the orbit of tools/bench_score.py) from Gaussians to uint8 frames in host memory.
  (a) the reference-shaped loop: the per-view GaussianRasterizer under no_grad and the reference's tail per frame
      (training/object_trainer.py:81-118: .cpu() of the fp32 image and depth, depth.max(), the numpy pass);
  (b) frames.render_frames (chunks of 8 through the batched forward, fused quantisation, pipelined copy of the bytes);
  (c) the device time of the quantise launches alone (events around many calls on 16 rendered views, two chunks of 8 taken in
      turn), their bytes per time against the 8 TB/s peak, and a plain device copy of the same number of bytes next to it.
(a) and (b) alternate in one process: only that comparison counts. usage: python tools/bench_frames.py [P res [P res ...]] [--views N]
[--reps N]; default: 500000 1024 100000 512. Prints one JSON line."""
import json, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dreamscene_amd import frames, synth, views, rasterizer as R
from dreamscene_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer

PEAK_BYTES_PER_S = 8.0e12
argv = sys.argv[1:]


def opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = int(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


N_VIEWS, REPS = opt("--views", 240), opt("--reps", 3)
sizes = [(int(argv[i]), int(argv[i + 1])) for i in range(0, len(argv) - 1, 2)] or [(500_000, 1024), (100_000, 512)]
if not torch.cuda.is_available():
    raise SystemExit("bench_frames needs the GPU: there is nothing to time without one")
dev = torch.device("cuda:0")
t = lambda a: torch.tensor(np.asarray(a, dtype=np.float32), device=dev)


def settings(c, H, W):
    return GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=t([1, 1, 1]),
                                         scale_modifier=1.0, viewmatrix=t(c.world_view_transform),
                                         projmatrix=t(c.full_proj_transform), sh_degree=3, campos=t(c.camera_center),
                                         prefiltered=False, score_flag=False)


def wall(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_ms(fn, reps):
    fn(); fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); a.record()
    for _ in range(reps):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def one_size(P, res):
    H = W = res
    g = synth.g_object(P, seed=0, K=16)
    p = {k: torch.tensor(v, device=dev) for k, v in g.items()}
    args = dict(means3D=p["means3D"], opacities=p["opacities"], shs=p["shs"], scales=p["scales"], rotations=p["rotations"])
    m2d = torch.zeros_like(p["means3D"])
    sl = [settings(synth.orbit_camera(5.35, 75.0, 360.0 * i / N_VIEWS, 0.46, H, W), H, W) for i in range(N_VIEWS)]
    rasts = [GaussianRasterizer(raster_settings=s) for s in sl]
    out = frames.Frames(torch.empty((N_VIEWS, H, W, 3), dtype=torch.uint8, pin_memory=True),
                        torch.empty((N_VIEWS, H, W, 1), dtype=torch.uint8, pin_memory=True))
    keep = {}

    def reference_loop():
        img_frames, depth_frames = [], []
        with torch.no_grad():
            for r in rasts:
                rgb, _, da = r(means2D=m2d, **args)
                depth = da[0:1]
                depths = torch.clamp(depth / depth.max(), 0.0, 1.0).detach().cpu().permute(1, 2, 0).numpy()
                depth_frames.append((depths * 255).round().astype(np.uint8))
                image = torch.clamp(rgb, 0.0, 1.0).detach().cpu().permute(1, 2, 0).numpy()
                img_frames.append((image * 255).round().astype(np.uint8))
        keep["a"] = (img_frames, depth_frames)

    def fused():
        keep["b"] = frames.render_frames(sl, chunk=8, out=out, **args)

    reference_loop(); fused()                                          # warm-up: every shape, the capacity hints, the streams
    same = all(np.array_equal(keep["a"][0][k], out.rgb[k].numpy()) and np.array_equal(keep["a"][1][k], out.depth[k].numpy())
               for k in range(N_VIEWS))
    ta, tb = [], []
    for _ in range(REPS):                                              # alternating: both see the same neighbours
        ta.append(wall(reference_loop))
        tb.append(wall(fused))
    a, b = float(np.median(ta)), float(np.median(tb))

    # (c) the quantise launches alone
    rc = R.DEFAULT_CONTEXT.snapshot()
    rc._forward_only = True
    with torch.no_grad():
        sets = []
        for i in (0, 8):
            res_ = views.rasterize_views_forward_raw(sl[i:i + 8], args["means3D"], args["opacities"], args["shs"], None,
                                                     args["scales"], args["rotations"], None, rc=rc)
            sets.append(([o["color"] for o, _ in res_], [o["depth_alpha"] for o, _ in res_]))
    F = len(sets[0][0])
    q_rgb = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    q_dep = torch.empty((F, H, W, 1), dtype=torch.uint8, device=dev)
    turn = [0]

    def quant(depth):
        def fn():
            imgs, das = sets[turn[0] & 1]
            turn[0] += 1
            frames.quantize_frames(imgs, das if depth else None, q_rgb, q_dep if depth else None)
        return fn
    px = F * H * W
    bytes_d, bytes_c = px * (12 + 4 + 4 + 4), px * (12 + 3)          # depth plane read twice (maximum, then quantise)
    ms_d, ms_c = device_ms(quant(True), 40), device_ms(quant(False), 40)
    src = [torch.empty(bytes_d // 2, dtype=torch.uint8, device=dev).random_(0, 255) for _ in range(2)]
    dst = torch.empty(bytes_d // 2, dtype=torch.uint8, device=dev)

    def plain_copy():
        dst.copy_(src[turn[0] & 1])
        turn[0] += 1
    ms_copy = device_ms(plain_copy, 40)
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3)
    return {"P": P, "res": res, "views": N_VIEWS, "reps": REPS, "bytes_equal_to_reference_loop": bool(same),
            "a_reference_loop_s": round(a, 4), "b_render_frames_s": round(b, 4), "a_over_b": round(a / b, 2),
            "a_all_s": [round(x, 4) for x in ta], "b_all_s": [round(x, 4) for x in tb],
            "a_views_per_s": round(N_VIEWS / a, 1), "b_views_per_s": round(N_VIEWS / b, 1),
            "c_quantise_8_views": {
                "with_depth_ms": round(ms_d, 4), "with_depth_bytes": bytes_d, "with_depth_TB_per_s": round(rate(bytes_d, ms_d) / 1e12, 3),
                "with_depth_fraction_of_peak": round(rate(bytes_d, ms_d) / PEAK_BYTES_PER_S, 3),
                "rgb_only_ms": round(ms_c, 4), "rgb_only_bytes": bytes_c, "rgb_only_TB_per_s": round(rate(bytes_c, ms_c) / 1e12, 3),
                "rgb_only_fraction_of_peak": round(rate(bytes_c, ms_c) / PEAK_BYTES_PER_S, 3),
                "plain_copy_same_bytes_ms": round(ms_copy, 4), "plain_copy_TB_per_s": round(rate(bytes_d, ms_copy) / 1e12, 3),
                "plain_copy_fraction_of_peak": round(rate(bytes_d, ms_copy) / PEAK_BYTES_PER_S, 3)}}


results = []
for P, res in sizes:
    results.append(one_size(P, res))
    print(f"done: P={P} {res}x{res}", file=sys.stderr, flush=True)
print(json.dumps({"bench": "frames", "sizes": results}))
