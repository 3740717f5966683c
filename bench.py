#!/usr/bin/env python3
"""Throughput of the RDPN6D hot path on MI355X: RGB-D crops/s, forward + pose solve, 256x256.

  python bench.py --gpus 1 --steps 20 --warmup 3
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

One step = one pass of the hot path over one device-resident synthetic batch of 64 crops
(BASELINE.json configs[1]: LM 13-object inference, batch 64, 256x256): stem -> ResNet-34 trunk ->
point-wise depth fusion -> dense mask/residual/region head -> glue -> ConvPnPNet -> pose decode
+ the per-crop RANSAC/Kabsch pose solve.  Inference shards with no collective: each rank
runs its own batch ("weak" scaling); value = all ranks' crops / max-over-ranks time.

Prints ONE JSON line (rank 0) with the driver's contract plus
  "roofline"     - the dominant kernel (the conv kernel instance that carries most of the step's FLOPs: by default the fp32-accurate
                   h2 eight-phase kernel conv_h2_8ph_kernel_t<false> - two fp16 planes per operand, three partial products; the
                   bf16x3 kernel with --fast x3, conv_igemm_f32_kernel<128,128> with --fast none, the 8-phase 16-bit kernel with
                   --dtype bf16) timed live with events on the launch stream: algorithmic FLOPs of its launches / their
                   total duration vs its MFMA ceiling (833.3 = 2500/3, 416.7 = 2500/6, 157.3, 2500 TFLOP/s; MI355X_MICROARCH.md);
  "train"        - (default run only) a short bf16 B=32 training leg after the timed region: ms_per_step, crops_per_s, tflops,
                   frac_of_2500, the dominant kernel, and where each gradient bucket's all-reduce was issued (--train-leg 0 = off);
  "cpu_baseline" - the torch-CPU oracle (a port of the reference path, pinned to it by golden vectors)
                   timed on this box's host cores on a bounded sample of the same workload.
--dump-outputs DIR also writes what the last timed step returned (DIR/<name>.npy) to compare two builds output for output.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FP32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md, "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 2500.0  # dense bf16 MFMA peak (same guide; never the 2:1-sparsity figure)


def build_model(device, mask_attention="none", bf16=False, graph=False, x3=True, fast="h2", backbone=34, res=256):
    from rdpn6d_amd import synth
    from rdpn6d_amd.config import gdrn_base_cfg
    from rdpn6d_amd.gdrn import build_model_optimizer

    cfg = gdrn_base_cfg(mask_attention=mask_attention, device=str(device))
    if (backbone, res) != (34, 256):  # BASELINE configuration C5: ResNet-50 trunk, 320x320 crops (training line only)
        cfg.MODEL.CDPN.BACKBONE.NUM_LAYERS, cfg.MODEL.CDPN.BACKBONE.INPUT_RES, cfg.MODEL.CDPN.BACKBONE.OUTPUT_RES = backbone, res, res // 4
    cfg.TEST.USE_PNP = True  # the step includes the per-crop RANSAC/Kabsch solve ("fwd+PnP")
    cfg.TEST.PNP_TYPE = "ransac_kabsch"  # the north star's solver (3D-3D on the RGB-D residual geometry); "ransac_pnp" = the 2D-3D one
    cfg.TEST.AMP_TEST = bool(bf16)  # secondary mode: trunk + fusion + head on the 16-bit matrix pipe (bf16 | fp16)
    cfg.TEST.AMP_DTYPE = bf16 if bf16 in ("bf16", "fp16") else "bf16"
    cfg.TEST.HIP_GRAPH = bool(graph)  # the ~90 launches of a step replay as one hipGraph (same kernels, same order)
    # fp32 mode: which fp32-ACCURATE form the wide layers take on the 16-bit matrix pipe: "h2" two fp16 planes / 3 partial
    # products (default), "x3" three bf16 planes / 6 partial products, "none" = every layer on the fp32 MFMA pipe
    cfg.TEST.BF16X3 = bool(x3) and fast in ("h2", "x3")  # master switch
    cfg.TEST.FP16X2 = fast == "h2"
    model, _ = build_model_optimizer(cfg)
    if (backbone, res) != (34, 256):
        sd = synth.make_trained_like_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=7)
    else:
        sd = synth.make_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()}, seed=1234)
        bn = np.load(os.path.join(ROOT, "tests", "golden", "bn_stats_c1.npz"))
        sd.update({k: bn[k] for k in bn.files})
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model.eval()
    return model, sd


def step(model, t):
    return model(t["roi_img"], roi_classes=t["roi_cls"], roi_coord_2d=t["roi_coord_2d"], roi_cams=t["roi_cam"],
                 roi_centers=t["roi_center"], roi_whs=t["roi_wh"], roi_extents=t["roi_extent"],
                 resize_ratios=t["resize_ratio"], do_loss=False, fps=t["fps"])


DUMP_LIMIT_BYTES = 64 * 10**6


def dump_outputs(outs, out_dir, batch, what):
    """`--dump-outputs DIR`: the arrays one call of the timed path returned, as DIR/<name>.npy - floating outputs in float32 (float64
    stays float64), integer / boolean ones in float64 (exact).  At most DUMP_LIMIT_BYTES in all: past that, the same fixed seeded
    sample of the crops (leading dimension `batch`) is taken from every per-crop array and its indices are written as crop_index.npy."""
    arrs = {}
    for k, v in outs.items():
        if v is None:
            continue
        a = v.detach().cpu()
        a = a.double() if (not a.is_floating_point() or a.dtype == torch.float64) else a.float()
        arrs[k] = a.numpy()
    per_crop = sum(a.nbytes // batch for a in arrs.values() if a.ndim and a.shape[0] == batch)
    fixed = sum(a.nbytes for a in arrs.values() if not (a.ndim and a.shape[0] == batch))
    slack = 128 * (len(arrs) + 1) + 8 * batch  # .npy headers, crop_index.npy
    if fixed + per_crop * batch + slack > DUMP_LIMIT_BYTES:
        keep = max(1, (DUMP_LIMIT_BYTES - fixed - slack) // max(per_crop, 1))
        idx = np.sort(np.random.default_rng(0).choice(batch, size=keep, replace=False))
        arrs = {k: a[idx] if a.ndim and a.shape[0] == batch else a for k, a in arrs.items()}
        arrs["crop_index"] = idx.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(out_dir, f"{k}.npy"), a)
    total = sum(a.nbytes for a in arrs.values())
    print(f"[bench] {what}: {len(arrs)} arrays, {total / 1e6:.1f} MB -> {out_dir}", file=sys.stderr)


def conv_flops(d):
    return 2.0 * d.B * d.Ho * d.Wo * d.N * d.ntaps * d.Cin


def roofline(model, t, B, device, reps=3):
    """Event-time every launch of the dominant conv kernel instance inside a real forward."""
    from rdpn6d_amd import _lib

    plan = model.plan(B, device)
    lib = plan.lib
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    classes = {}  # tile -> launches of the conv kernel instance with that tile (bf16: the 64-channel K-chunk variants)
    lowp_fn = getattr(lib, f"rdpn6d_conv2d_{plan.lp or 'bf16'}")
    for L in plan.launches:
        if L.keep and L.fn in (lib.rdpn6d_conv2d_h2, lib.rdpn6d_conv2d_h2_cb):
            classes.setdefault("h2" if lib.rdpn6d_conv_h2_kernel_for(ctypes.byref(L.keep[0])) == 2 else "h2tile", []).append(L)
        elif L.keep and L.fn in (lib.rdpn6d_conv2d_bf16x3, lib.rdpn6d_conv2d_bf16x3_ex):
            # 256x256 8-phase kernel ("x3") or the 128x128..64x64 tile kernel ("x3tile")
            classes.setdefault("x3" if lib.rdpn6d_conv_bf16x3_kernel_for(ctypes.byref(L.keep[0])) == 2 else "x3tile", []).append(L)
        elif L.keep and L.fn in (lowp_fn, lib.rdpn6d_conv2d_f32) and (L.fn is lowp_fn) == plan.bf16:
            d = L.keep[0]
            bm, bn = ctypes.c_int(), ctypes.c_int()
            (getattr(lib, f"rdpn6d_conv_{plan.lp}_tile_for") if plan.bf16 else lib.rdpn6d_conv_tile_for)(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn))
            if not plan.bf16 or d.Cin % 64 == 0:
                classes.setdefault((bm.value, bn.value), []).append(L)
    # the dominant kernel = the instance that carries most of the step's FLOPs
    tile = max(classes, key=lambda k: sum(conv_flops(L.keep[0]) for L in classes[k])) if classes else (128, 128)
    sel = classes.get(tile, [])
    flops = sum(conv_flops(L.keep[0]) for L in sel)
    total_ms, n = 0.0, 0
    step(model, t)
    # the clock the (power-limited) eight-phase kernel runs at: its workgroup 0 leaves shader-clock ticks and the constant 100 MHz
    # counter at its start and end (rdpn6d_conv_h2_set_clock_probe) - boxes of the pool differ by 7 % on exactly this number
    clk = torch.zeros(4, dtype=torch.int64, device=device) if tile == "h2" else None
    ghz = []
    if clk is not None:
        lib.rdpn6d_conv_h2_set_clock_probe(ctypes.c_void_p(clk.data_ptr()))
    for _ in range(reps):
        # replay the plan with events around the selected launches (same stream the kernels run on)
        x = t["roi_img"]
        _lib.check(plan.stem_fn(ctypes.c_void_p(x.data_ptr()), plan.stem_args[0], x.shape[1], *plan.stem_args[2:], st))
        _lib.check(plan.xyz_fn(ctypes.c_void_p(x.data_ptr()), plan.xyz_args[0], x.shape[1], *plan.xyz_args[2:], st))
        evs = []
        for L in plan.launches:
            if L in sel:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(L.fn(*L.args, st), L.name)
                e1.record()
                evs.append((e0, e1))
            else:
                _lib.check(L.fn(*L.args, st), L.name)
        torch.cuda.synchronize()
        total_ms += sum(a.elapsed_time(b) for a, b in evs)
        n += len(evs)
        if clk is not None:  # (the last eight-phase launch of the pass: the head's final layer)
            c = clk.tolist()
            if c[3] > c[1]:
                ghz.append((c[2] - c[0]) / ((c[3] - c[1]) * 10.0))
    if clk is not None:
        lib.rdpn6d_conv_h2_set_clock_probe(None)
    avg_ms = total_ms / max(n, 1)
    achieved = flops / len(sel) / (avg_ms * 1e-3) / 1e12 if sel else 0.0
    extra = {}
    if tile in ("h2", "h2tile"):
        # fp32-accurate products as three fp16 partial products: the ceiling for ALGORITHMIC flops is the fp16 pipe / 3
        kname, peak = ("conv_h2_8ph_kernel_t<false>" if tile == "h2" else "conv_h2_tile_kernel"), round(BF16_MFMA_PEAK_TFLOPS / 3.0, 1)
        extra = {"peak_note": "2500 TFLOP/s dense fp16 MFMA / 3 partial products per fp32 product (157.3 on the fp32 MFMA pipe)",
                 "mfma_tflops_issued": round(3.0 * achieved, 1),
                 # shader clock of the dominant kernel while it runs (s_memtime ticks per 100 MHz s_memrealtime tick, workgroup 0 of the
                 # head's last eight-phase launch, mean of the event-timed passes): the part's peak is quoted at 2.4 GHz
                 "clock_ghz": round(sum(ghz) / len(ghz), 3) if ghz else None}
    elif tile in ("x3", "x3tile"):
        # fp32-accurate products as six bf16 partial products: the ceiling for ALGORITHMIC flops is the bf16 pipe / 6
        kname, peak = ("conv_igemm_bf16x3_kernel" if tile == "x3" else "conv_x3_tile_kernel"), round(BF16_MFMA_PEAK_TFLOPS / 6.0, 1)
        extra = {"peak_note": "2500 TFLOP/s dense bf16 MFMA / 6 partial products per fp32 product (157.3 on the fp32 MFMA pipe)",
                 "mfma_tflops_issued": round(6.0 * achieved, 1)}
    elif plan.bf16:
        kname = ("conv_igemm_bf16_8ph_kernel<0>" if tile == (256, 256)
                 else f"conv_igemm_bf16_kernel<{tile[0]}, {tile[1]}, 128, 2, 2, 2>")
        peak = BF16_MFMA_PEAK_TFLOPS
    else:
        kname, peak = f"conv_igemm_f32_kernel<{tile[0]}, {tile[1]}>", FP32_MFMA_PEAK_TFLOPS
    traffic, traffic_src, prof_us = pmc_traffic(kname, plan.bf16) if B == 64 else (None, None, None)
    # the counters come from a committed profile of this command, not from this process: flag the figure when the kernel it was
    # measured on no longer runs like the one timed here (a changed kernel with a stale profile)
    stale = None if traffic is None else bool(abs(prof_us - avg_ms * 1e3) > 0.25 * avg_ms * 1e3)
    if stale:
        print(f"[bench] roofline.traffic comes from {traffic_src} whose {kname} ran {prof_us:.0f} us/launch, {avg_ms * 1e3:.0f} us here: "
              "re-run tools/pmc_bench.sh", file=sys.stderr)
    return {
        "bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_unit": "bytes/launch (HBM+fabric, PMC)",
        "traffic_source": traffic_src, "traffic_stale": stale,
        # the launch duration of the same kernel in the PROFILE the traffic figure comes from, beside the live one (avg_launch_ms)
        "traffic_profile_avg_launch_ms": None if prof_us is None else round(prof_us * 1e-3, 4),
        "kernel": kname.replace(", ", ","), "launches_per_step": len(sel),
        "avg_launch_ms": round(avg_ms, 4), "algorithmic_gflop_per_launch": round(flops / max(len(sel), 1) / 1e9, 2),
        "share_of_step_flops": round(flops / (44.10e9 * B), 3), **extra,
    }


def pmc_traffic(kernel, bf16=False):
    """HBM-side bytes per launch of `kernel` from the committed rocprofv3 PMC passes (FETCH_SIZE x2 per the gfx950 rule of
    MI355X_MICROARCH.md + WRITE_SIZE; collected in separate --pmc runs of this same command, tools/pmc_bench.sh +
    tools/summarize_pmc.py).  Counters cannot be read from inside the timed process, so the figure comes from profiles/
    (latest summary of the same mode; None if absent)."""
    import glob

    for f in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc_summary.json")), reverse=True):
        if ("bf16" in os.path.basename(f)) != bool(bf16):
            continue
        try:
            d = json.load(open(f))
            e = d[kernel] if kernel in d else next(v for k, v in d.items() if kernel in k)  # (anonymous namespace):: prefix
            return int((e["fetch_MB_x2"] + e["write_MB"]) * 1e6), os.path.relpath(f, ROOT), float(e["avg_us"])
        except (KeyError, ValueError, StopIteration):
            continue
    return None, None, None


def cpu_baseline(sd, budget_s=20.0):
    """torch-CPU oracle (port of the reference path) on a bounded sample of the same workload.

    oneDNN's small convolutions scale badly past a few dozen threads, so the thread count is chosen by
    a short sweep (the best one is what gets reported as ``cores``) before the timed ~budget_s run."""
    from oracle import model_oracle
    from rdpn6d_amd import synth

    ncpu = os.cpu_count() or 1
    # the per-crop RANSAC/Kabsch solve of the step: the C oracle (single thread), when its library is there
    pnp = None
    so = os.path.join(ROOT, "oracle", "liboracle.so")
    if os.path.exists(so):
        P = ctypes.c_void_p
        f = ctypes.CDLL(so).oracle_ransac_kabsch
        f.argtypes = [P, P, P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                      ctypes.c_float, ctypes.c_uint, P, P, P, P]
        f.restype = None

        def pnp(o, inp):
            B, HW, K = 4, 64 * 64, 32
            arrs = [np.ascontiguousarray(torch.cat([o["mask"], o["coor_x"], o["coor_y"], o["coor_z"], o["region"]], 1).reshape(B, 5 + K, HW).numpy()),
                    np.ascontiguousarray(inp["roi_coord_2d"].reshape(B, 5, HW).numpy()), np.ascontiguousarray(inp["fps"].numpy()),
                    np.ascontiguousarray(inp["roi_extent"].numpy()), np.ascontiguousarray(inp["resize_ratio"].numpy()),
                    np.ascontiguousarray(o["region_argmax"].reshape(B, HW).numpy().astype(np.int32)),
                    np.zeros((B, 12), np.float32), np.zeros(B, np.int32), np.zeros((B, HW), np.uint8), np.zeros(B, np.int32)]
            f(*[a.ctypes.data_as(P) for a in arrs[:6]], B, HW, K, 0.5, 0.01, 100, 0.99, 0, *[a.ctypes.data_as(P) for a in arrs[6:]])
    m = model_oracle.GDRNOracle(32, "none")
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    m.eval()
    inp = {k: torch.from_numpy(v) for k, v in synth.make_inputs(4, seed=0).items()}
    args = (inp["roi_img"], inp["roi_coord_2d"], inp["fps"], inp["roi_cam"], inp["roi_center"], inp["roi_wh"], inp["resize_ratio"])
    best_nt, best = 1, float("inf")
    with torch.no_grad():
        for nt in sorted({min(n, ncpu) for n in (8, 16, 32, 64)}):
            torch.set_num_threads(nt)
            m(*args)
            t0 = time.perf_counter()
            m(*args)
            dt = time.perf_counter() - t0
            if dt < best:
                best_nt, best = nt, dt
        torch.set_num_threads(best_nt)
        t0, it = time.perf_counter(), 0
        while True:
            o = m(*args)
            if pnp is not None:
                pnp(o, inp)
            it += 1
            dt = time.perf_counter() - t0
            if dt > budget_s or it >= 400:
                break
    return {"value": round(4 * it / dt, 2), "unit": "crops/s", "cores": best_nt, "kind": "port",
            "sample": f"{it} passes of a B=4 batch (256x256, fp32, torch-CPU oracle incl. glue + pose decode"
                      f"{' + the C oracle of the per-crop RANSAC/Kabsch solve, 1 thread' if pnp is not None else ''}) in "
                      f"{dt:.1f} s with {best_nt} threads (best of an 8/16/32/64 sweep; host has {ncpu} logical CPUs)"}


def train_roofline(eng, one_step, reps=3):
    """The mixed-precision training step's dominant kernel by FLOPs - the 256x256 eight-phase 16-bit convolution kernel, which runs
    the forward AND the input-gradient convolutions of the head's 3x3 layers (and the ConvTranspose phases): every launch of it inside
    real steps is bracketed by events on the launch stream; algorithmic FLOPs / time against the dense 16-bit MFMA peak."""
    import ctypes

    lib = eng.lib
    tile_for = getattr(lib, f"rdpn6d_conv_{eng.lp}_tile_for")

    def is_8ph(fn):
        d = getattr(fn, "desc", None)
        if d is None or getattr(fn, "bn_capable", None) is None:
            return False
        bm, bn = ctypes.c_int(), ctypes.c_int()
        tile_for(ctypes.byref(d), ctypes.byref(bm), ctypes.byref(bn))
        return (bm.value, bn.value) == (256, 256) and d.Cin % 64 == 0

    evs, flops = [], []

    def timed(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            evs.append((e0, e1))
            flops.append(conv_flops(fn.desc))
        return run

    saved_f, saved_b = list(eng.fwd), [list(g) for g in eng.bwd]
    nf = nb = 0
    for i, fn in enumerate(eng.fwd):
        if is_8ph(fn):
            eng.fwd[i] = timed(fn)
            nf += 1
    for g in eng.bwd:
        for j, fn in enumerate(g):
            if is_8ph(fn):
                g[j] = timed(fn)
                nb += 1
    try:
        for _ in range(reps):
            one_step()
        torch.cuda.synchronize()
    finally:
        eng.fwd[:] = saved_f
        for g, sg in zip(eng.bwd, saved_b):
            g[:] = sg
    if not evs:
        return None
    ms = [a.elapsed_time(b) for a, b in evs]
    achieved = sum(flops) / (sum(ms) * 1e-3) / 1e12
    # HBM-side bytes per launch from the committed PMC passes of `bench.py --train --dtype bf16` (profiles/*train_bf16_pmc_summary.json:
    # the forward instantiation <0, true> - it carries the BatchNorm sums - stands for both directions; the fp16 build has no own profile)
    traffic, traffic_src, prof_us = pmc_traffic("conv_igemm_bf16_8ph_kernel<0, true>", bf16=True) if eng.lp == "bf16" else (None, None, None)
    avg_us = sum(ms) / len(ms) * 1e3
    return {"bound": "mfma", "achieved": round(achieved, 1), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / BF16_MFMA_PEAK_TFLOPS, 4), "traffic": traffic, "traffic_unit": "bytes/launch (HBM+fabric, PMC)",
            "traffic_source": traffic_src, "traffic_stale": None if traffic is None else bool(abs(prof_us - avg_us) > 0.25 * avg_us),
            "traffic_profile_avg_launch_ms": None if prof_us is None else round(prof_us * 1e-3, 4),
            "kernel": f"conv_igemm_bf16_8ph_kernel ({eng.lp} build)", "launches_per_step": nf + nb,
            "launches_forward": nf, "launches_input_gradient": nb, "avg_launch_ms": round(sum(ms) / len(ms), 4),
            "algorithmic_gflop_per_launch": round(sum(flops) / len(flops) / 1e9, 2),
            "share_of_step_flops": round(sum(flops) / reps / (132.3e9 * eng.B), 3)}


def train_leg(rank, world, device, dist, dtype="bf16", B=32, backbone=34, res=256, steps=100, warmup=3, preheat=3.0, buckets="stages",
              comm_dtype=None, dump=None):
    """The training step (fwd + nine losses + bwd + per-stage gradient all-reduce + fused Ranger + weight re-pack) timed like the
    headline: W warm-up steps, `preheat` seconds of un-timed steps, barrier, EXACTLY `steps` steps, barrier, max over ranks.  Every rank
    runs the same number of steps (the steps carry the all-reduces).  Returns the figures as a dict (rank 0's view); `--train` prints
    them as its own line, the default run attaches them to the headline line as "train"."""
    from rdpn6d_amd import synth
    from rdpn6d_amd.parallel import GROUPS, STAGES, GradBuckets, stage_params
    from rdpn6d_amd.ranger import Ranger

    model, _ = build_model(device, "mul", backbone=backbone, res=res)
    model.cfg.TEST.USE_PNP = False
    amp = dtype in ("bf16", "fp16")
    model.cfg.SOLVER.AMP.ENABLED = amp  # --dtype bf16 | fp16: mixed precision (16-bit fwd/dgrad/wgrad convolutions, fp32 everything else)
    model.cfg.SOLVER.AMP.DTYPE = dtype if amp else "bf16"
    eng = model.train_engine(B, device)
    if dtype == "fp16":
        eng.loss_scale = 4096.0  # static loss scale (the reference: GradScaler, engine.py:302-309)
    gb = GradBuckets(model, groups=STAGES if buckets == "stages" else GROUPS, always_reduce=bool(os.environ.get("RDPN6D_BENCH_FORCE_DIST")),
                     comm_dtype={None: None, "f32": None, "bf16": torch.bfloat16}[comm_dtype], timing=True)
    order = [p for g in STAGES for p in stage_params(model, g)]
    opt = Ranger(order, lr=1e-4, flat_grad=gb.flat)  # fused HIP step over the same flat gradient buffer
    inp = synth.make_inputs(B, seed=200 + rank, res=res)
    batch = {k: torch.from_numpy(v).to(device) for k, v in {**inp, **synth.make_train_gt(B, inp)}.items()}

    skipped = [0]

    def one_step():
        losses = eng.forward_losses(batch)
        if eng.loss_scale != 1.0:
            eng.seed_backward({n: eng.loss_scale for n in eng.LOSS_NAMES})
        eng.backward(on_group_done=gb.reduce)
        gb.finish()
        if dtype == "fp16":
            # fp16: GradScaler's rule (engine.py:302-309) - a step whose reduced gradients are not finite is SKIPPED and the scale halved
            # (one host read per step, as scaler.step() has); un-skipped, one overflow of an fp16 activation gradient poisons the weights.
            # The un-scaling and the finite check ride in the optimizer's own launches (Ranger.step): one 144-MB read instead of
            # torch's isfinite().all() + mul_() (nine launches, 227 us of a 10.6-ms step).  Keyed on the dtype, not on the scale: a
            # scale that has halved its way down to 1 still needs the guard
            opt.step(grad_scale=eng.loss_scale, skip_if_nonfinite=True)
            if opt.found_inf():
                skipped[0] += 1
                eng.loss_scale = max(eng.loss_scale * 0.5, 1.0)
                return losses
        else:
            opt.step()
        eng.refresh_weights()
        return losses

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(warmup):
        one_step()
    torch.cuda.synchronize()
    # pre-heat: every step carries the gradient all-reduces, so all ranks must run the SAME number of steps - rank 0's clock decides
    # and its decision is broadcast after every block (a per-rank perf_counter() exit would leave the ranks' collective sequences
    # different: a hang)
    tp = time.perf_counter()
    go = torch.ones(1, dtype=torch.int32, device=device if dist is None or dist.get_backend() == "nccl" else "cpu")
    while True:
        go[0] = int(time.perf_counter() - tp < preheat)
        if dist is not None:
            dist.broadcast(go, src=0)
        if not int(go.item()):
            break
        for _ in range(5):
            one_step()
        torch.cuda.synchronize()
    barrier()
    t0 = time.perf_counter()
    for _ in range(steps):
        losses = one_step()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    barrier()
    if dump and rank == 0:  # (before the event-timed steps below take the engine further)
        dump_outputs(losses, dump, B, "losses of the last timed training step")
    el = torch.tensor([elapsed], dtype=torch.float64, device=device if dist is None or dist.get_backend() == "nccl" else "cpu")
    if dist is not None:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    sync = gb.report()  # (events of the LAST timed step: where each stage's all-reduce was issued relative to the backward's end)
    # the event-timed steps carry the gradient all-reduces too: EVERY rank runs them (rank 0 alone would leave the others' collective
    # sequence short - a hang); only rank 0's figures are reported
    roof = train_roofline(eng, one_step) if amp else None
    if dist is not None:
        dist.barrier()
    value = world * B * steps / elapsed
    std = (backbone, res) == (34, 256)
    out = {
        "ms_per_step": round(elapsed / steps * 1e3, 3), "crops_per_s": round(value, 1), "steps": steps, "warmup": warmup, "preheat_s": preheat,
        "batch_per_gpu": B, "global_batch": B * world, "n_gpus": world,
        "dtype": f"{dtype} convolutions (fwd + dgrad + wgrad) and stored activations, fp32 BN math / losses / pose branch / optimizer" if amp else "f32",
        "workload": ("LM-O style" if std else "MP6D style (BASELINE C5 shape)")
                    + f" training step, MASK_ATTENTION=mul, K=32, ResNet-{backbone}, {res}x{res} crops, per-GPU BatchNorm, "
                    + ("SOLVER.AMP.ENABLED" if amp else "fp32"),
        "parallelism": f"dp{world}: flat gradient buffer, {len(gb.groups)} RCCL all-reduces (one per stage of the backward, issued as the "
                       f"stage's gradients complete), fused HIP Ranger",
        "gflop_per_crop": {"fwd+dgrad+wgrad": 132.3} if std else None,
        "tflops": round(132.3e9 * value / 1e12, 2) if std else None,
        "frac_of_2500": round(132.3e9 * value / world / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4) if (amp and std) else None,
        "dominant_kernel": roof, "gradient_sync": sync,
        "allreduce_exposed_ms": None if sync is None else sync["allreduce_exposed_ms"],
        "loss_scale_final": eng.loss_scale if dtype == "fp16" else None, "steps_skipped_for_overflow": skipped[0] if dtype == "fp16" else None,
        "loss_total": round(float(sum(v.item() for v in losses.values())), 4)}
    return out


def train_bench(args, rank, world, device, dist):
    """`--train`: the training step as its own JSON line (SURVEY.md C3 shape: 32 crops per GPU, data parallel, gradient all-reduce over
    RCCL).  Not the headline metric."""
    B = args.batch if args.batch != 64 else 32
    t = train_leg(rank, world, device, dist, dtype=args.dtype, B=B, backbone=args.backbone, res=args.res, steps=args.steps, warmup=args.warmup,
                  preheat=args.preheat, buckets=args.buckets, comm_dtype=args.allreduce_dtype, dump=args.dump_outputs)
    if rank == 0:
        print(json.dumps({
            "metric": f"RGB-D crops/sec, TRAINING step (fwd+losses+bwd+allreduce+Ranger) at {args.res}x{args.res}", "value": t["crops_per_s"],
            "unit": "crops/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": t["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "world": world, "backend": dist.get_backend() if dist is not None else None, "device_count": torch.cuda.device_count(),
            "dtype": t["dtype"], "data": "synthetic",
            "config": {"workload": t["workload"], "batch_per_gpu": B, "global_batch": B * world, "parallelism": t["parallelism"]},
            "achieved_tflops_whole_step": t["tflops"], "whole_step_frac_of_16bit_mfma_peak": t["frac_of_2500"],
            "gflop_per_crop": t["gflop_per_crop"], "preheat_s": args.preheat, "roofline": t["dominant_kernel"],
            "gradient_sync": t["gradient_sync"], "allreduce_exposed_ms": t["allreduce_exposed_ms"],
            "loss_scale_final": t["loss_scale_final"], "steps_skipped_for_overflow": t["steps_skipped_for_overflow"],
            "loss_total": t["loss_total"]}))
    if dist is not None:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--trace", type=int, default=0, metavar="N",
                    help="record the stream time of every block of N steps (events, no extra synchronisation) and report it as "
                         "ms_per_step_trace: shows whether the clock / throughput drifts over a long run (--steps 2000 --trace 100)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preheat", type=float, default=3.0, metavar="SECONDS",
                    help="un-timed steps for this long after the W warm-up steps, before the K timed ones: the timed window then sits on the "
                         "sustained (power-limited) clock whatever K is (reported as preheat_s; 0 = off)")
    ap.add_argument("--batch", type=int, default=64, help="crops per GPU per step (BASELINE configs[1]: 64)")
    ap.add_argument("--mask-attention", default="none", choices=["none", "mul"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-x3", action="store_true",
                    help="fp32 mode: keep every convolution on the fp32 MFMA pipe (= --fast none)")
    ap.add_argument("--fast", default="h2", choices=["h2", "x3", "none"],
                    help="fp32 mode: fp32-accurate form of the wide layers on the 16-bit matrix pipe: h2 = two fp16 planes, 3 partial "
                         "products (cfg.TEST.FP16X2, default) | x3 = three bf16 planes, 6 partial products (cfg.TEST.BF16X3) | none")
    ap.add_argument("--cam", default="lm", choices=["lm", "ycbv"], help="camera intrinsics / object set of the synthetic crops (C4: ycbv)")
    ap.add_argument("--backbone", type=int, default=34, choices=[18, 34, 50, 101],
                    help="--train only: ResNet depth (BASELINE C5 = 50 with --res 320 --dtype fp16)")
    ap.add_argument("--res", type=int, default=256, help="--train only: crop size (C5: 320)")
    ap.add_argument("--test-cfg", default="", metavar="KEY=0|1[,...]",
                    help="override boolean cfg.TEST switches for A/B runs, e.g. FOLD_GLOBAL_MAX=0,CONV_BEFORE_UPSAMPLE=0 "
                         "(the reference's evaluation order of the two algebraic rewrites of the h2 plan)")
    ap.add_argument("--range-check", default="sync", choices=["sync", "deferred"],
                    help="cfg.TEST.H2_RANGE_CHECK: sync (the model's default: every forward reads the fp16-range flag of the h2 kernels for "
                         "itself before handing out its outputs - one host wait per step) | deferred (pipelined serving: the flag is "
                         "looked at by the next forward and once more here after the timed loop)")
    ap.add_argument("--graph", action="store_true",
                    help="replay the step as one hipGraph instead of launching kernel by kernel (measured: no gain, the "
                         "launch queue already runs ahead of the GPU - 2776 vs 2779 crops/s fp32, 10729 vs 10820 bf16)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "fp16"],
                    help="f32 (default, the parity-bearing headline) | bf16: secondary line, cfg.TEST.AMP_TEST mode "
                         "(trunk + fusion + head on the bf16 matrix pipe, fp32 head output / ConvPnPNet / pose / RANSAC)")
    ap.add_argument("--train-leg", type=float, default=1.5, metavar="SECONDS",
                    help="default (inference) run: after the timed region, a short bf16 B=32 training leg - SECONDS of pre-heat + 60 timed "
                         "steps - reported under \"train\" in the same JSON line (not part of `value`); 0 = off")
    ap.add_argument("--buckets", default="stages", choices=["stages", "coarse"],
                    help="training: gradient all-reduce buckets - one per stage of the backward (pnp_net, rot_head_net, layer4, layer3, rest: "
                         "default) | coarse = the three sub-modules (round 5's form: the backbone's 86 MB go out after the backward has ended)")
    ap.add_argument("--allreduce-dtype", default="f32", choices=["f32", "bf16"],
                    help="training: transport dtype of the gradient all-reduce (cfg.SOLVER.ALLREDUCE_DTYPE; bf16 = 72.8 instead of 145.6 MB)")
    ap.add_argument("--train", action="store_true",
                    help="secondary line: training step (fwd + losses + bwd + bucketed RCCL all-reduce + Ranger), B=32/GPU; "
                         "fp32, or mixed precision (cfg.SOLVER.AMP.ENABLED) with --dtype bf16")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the LAST timed step returned as DIR/<name>.npy (rank 0; float32, integer outputs "
                         "as float64; at most 64 MB in all, a fixed seeded sample of the crops past that).  The inputs are seeded: with the "
                         "same arguments two builds compare output for output.  --train: the losses of that step - the weights it ran on "
                         "took every earlier step too, so compare training runs with --preheat 0 (a fixed number of steps)")
    args = ap.parse_args()

    # --gpus N is the number of ranks (one per GPU).  Launched bare (`python bench.py --gpus N`, no WORLD_SIZE in the environment) with
    # N > 1 this process becomes the launcher: it starts `python -m torch.distributed.run --nproc-per-node N bench.py <same args>` as a
    # fresh CHILD and exits with its code - before anything here has touched the GPU, and without exec (the pool forbids replacing a
    # process that has initialised HIP).  Under a launcher WORLD_SIZE must equal --gpus: a mismatch is an error, not a silent 1-rank run.
    if args.gpus < 1:
        raise SystemExit(f"bench.py: --gpus {args.gpus}: need at least one rank")
    if args.steps < 1:
        raise SystemExit(f"bench.py: --steps {args.steps}: need at least one timed step")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        import socket
        import subprocess

        with socket.socket() as s:  # a free rendezvous port on the loop-back interface
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        print(f"[bench] --gpus {args.gpus} without a launcher: starting {' '.join(cmd[1:8])} ...", file=sys.stderr)
        raise SystemExit(subprocess.run(cmd, env={**os.environ, "MASTER_ADDR": "127.0.0.1"}).returncode)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: start it bare (it launches its own ranks) or under "
                         f"torch.distributed.run --nproc-per-node {args.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if local_rank < ndev else local_rank % max(ndev, 1)  # (more ranks than GPUs only in the self-test below)
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    dist = None
    if world > 1 or os.environ.get("RDPN6D_BENCH_FORCE_DIST"):  # (forced at world 1: the one-GPU test of the RCCL code path)
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL ("nccl" on ROCm) in every real run.  RDPN6D_BENCH_BACKEND=gloo exists only to exercise this multi-process
        # path on a ONE-GPU box (two ranks sharing device 0 cannot form an RCCL communicator).
        backend = os.environ.get("RDPN6D_BENCH_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)

    from rdpn6d_amd import synth

    if args.train:
        return train_bench(args, rank, world, device, dist)
    model, sd = build_model(device, args.mask_attention, bf16=args.dtype if args.dtype != "f32" else False, graph=args.graph, x3=not args.no_x3 and args.fast != "none", fast=args.fast)
    for kv in filter(None, args.test_cfg.split(",")):
        k, v = kv.split("=")
        model.cfg.TEST[k.strip()] = bool(int(v))
    model.cfg.TEST.H2_RANGE_CHECK = args.range_check
    B = args.batch
    t = {k: torch.from_numpy(v).to(device) for k, v in synth.make_inputs(B, seed=100 + rank, cam=args.cam).items()}

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    marks = []
    with torch.no_grad():
        for _ in range(args.warmup):
            step(model, t)
        # un-timed pre-heat: the dominant kernel runs on the POWER limit (1.3-1.7 GHz under load, 2.4 idle) - a cold 0.14-s timed
        # window (the driver's --steps 20) would be measured on the way down; --preheat 0 restores the bare W-step warm-up
        torch.cuda.synchronize()
        tp = time.perf_counter()
        while time.perf_counter() - tp < args.preheat:
            for _ in range(10):
                step(model, t)
            torch.cuda.synchronize()
        barrier()
        t0 = time.perf_counter()
        for i in range(args.steps):
            if args.trace and i % args.trace == 0:
                marks.append(torch.cuda.Event(enable_timing=True))
                marks[-1].record()
            o = step(model, t)
        if args.trace:
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        barrier()
    if args.dump_outputs and rank == 0:
        dump_outputs(o, args.dump_outputs, B, "outputs of the last timed step")
    my_elapsed = elapsed
    el = torch.tensor([elapsed], dtype=torch.float64, device=device if dist is None or dist.get_backend() == "nccl" else "cpu")
    per_rank = [el.clone() for _ in range(world)]
    if dist is not None:
        dist.all_gather(per_rank, el)  # every rank's own time: a slow / stalled rank is visible in the line, not only in the max
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    per_rank_rate = [round(B * args.steps / float(x.item()), 1) for x in per_rank]
    print(f"[bench] rank {rank}: {B * args.steps / my_elapsed:.1f} crops/s ({my_elapsed / args.steps * 1e3:.3f} ms/step)", file=sys.stderr)

    roof, cpu = None, None
    dtype_label, dtype_note = args.dtype, None
    if args.dtype == "f32" and model.plan(B, device).x3_launches:
        if model.plan(B, device).fast == "h2":
            dtype_note = ("fp32 accumulation and accuracy; the head and the ResNet trunk hold every operand as two fp16 terms (22 bits) and "
                          "evaluate a product as three exact partial products on the fp16 MFMA pipe (h2, DESIGN.md section 2: error vs fp64 "
                          "BELOW the fp32 MFMA kernel's on every tested shape, incl. the a-priori bound under cancellation); fp32 MFMA "
                          "elsewhere; --fast x3 = three bf16 planes / six products, --fast none = every layer on the fp32 MFMA pipe")
        else:
            dtype_note = ("fp32 storage, accumulation and accuracy; the head and the ResNet trunk evaluate every fp32 product exactly as "
                          "six bf16 partial products on the bf16 MFMA pipe (bf16x3, DESIGN.md section 2: error vs fp64 no larger than the "
                          "fp32 MFMA kernel's, tested); fp32 MFMA elsewhere; --no-x3 keeps every layer on the fp32 MFMA pipe")
    if rank == 0:
        with torch.no_grad():
            roof = roofline(model, t, B, device)
    if dist is not None:
        dist.barrier()
    train = None
    if args.train_leg > 0 and args.dtype == "f32" and B == 64 and not args.graph:
        # the driver's one command also puts the TRAINING step on record: BASELINE C3's per-GPU shape - bf16 AMP,
        # 32 crops per GPU, fwd + losses + bwd + per-stage all-reduce + Ranger - after the headline's timed region, never part of `value`
        train = train_leg(rank, world, device, dist, dtype="bf16", B=32, steps=60, warmup=3, preheat=args.train_leg)
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(sd)
    if dist is not None:
        dist.barrier()
    if rank == 0:
        value = world * B * args.steps / elapsed
        pl = model.plan(B, device)
        skipped_gflop = (3.62 if getattr(pl, "compose_ct", False) else 2.42) if getattr(pl, "fold_gmax", False) else 0.0
        line = {
            "metric": "RGB-D crops/sec (fwd+PnP) at 256x256", "value": round(value, 1), "unit": "crops/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype_label, "data": "synthetic",
            "world": world, "backend": dist.get_backend() if dist is not None else None, "device_count": torch.cuda.device_count(),
            "config": {"workload": ("LM 13-object" if args.cam == "lm" else "YCB-V 21-object (BASELINE C4 shape: YCB-V intrinsics)")
                                   + f" inference, batch={B} per GPU, 256x256 RGB-D crops, K=32 regions, "
                                   "ResNet-34 trunk + dense head + ConvPnPNet + pose decode + per-crop RANSAC/Kabsch (100 hyp.), all on-device",
                       "batch_per_gpu": B, "global_batch": B * world, "mask_attention": args.mask_attention,
                       "parallelism": f"replicated weights, {world} independent shard(s), no collective",
                       "launch": "hipGraph replay" if args.graph else "eager",
                       "h2_range_check": args.range_check},
            # the fp32-accurate form the plan ended on ("h2" unless an activation left the fp16 range and the model switched to "x3")
            "fast_path": model.plan(B, device).fast, "h2_range_exceeded": bool(model.h2_range_exceeded(device, wait=True)),
            # EXECUTED multiply-adds (the rewrites of DESIGN.md section 4 remove 3.62 / 2.42 of the reference's 44.10 GFLOP per crop);
            # the figure on the reference's count is kept beside it, labelled
            "achieved_tflops_whole_step": round((44.10 - skipped_gflop) * 1e9 * value / 1e12, 2),
            "achieved_tflops_reference_flop_count": round(44.10e9 * value / 1e12, 2),
            "gflop_per_crop": {"reference": 44.10, "executed": round(44.10 - skipped_gflop, 2)},
            "preheat_s": args.preheat,
            "flops_note": ("44.10 GFLOP per crop = the reference network's multiply-adds" +
                           ("; the h2 plan evaluates the spatially constant (broadcast global max) half of the ConvTranspose input as a "
                            "per-crop bias and composes conv3 + BatchNorm (no activation in between) into the ConvTranspose weights "
                            "(cfg.TEST.FOLD_GLOBAL_MAX / COMPOSE_CONV3_CONVT, DESIGN.md section 4): identical function, "
                            f"{3.62 if getattr(model.plan(B, device), 'compose_ct', False) else 2.42} GFLOP per crop it does not execute"
                            if getattr(model.plan(B, device), "fold_gmax", False) else "")),
            "per_rank_crops_per_s": per_rank_rate,
            "roofline": roof,
        }
        if args.trace:
            blk = [marks[i].elapsed_time(marks[i + 1]) / min(args.trace, args.steps - i * args.trace) for i in range(len(marks) - 1)]
            line["ms_per_step_trace"] = {"block_steps": args.trace, "ms_per_step": [round(x, 3) for x in blk],
                                         "drift_last_vs_first": round(blk[-1] / blk[0], 4), "timed_seconds": round(elapsed, 2)}
        if dtype_note:
            line["dtype_note"] = dtype_note
        if train is not None:
            line["train"] = train
        if cpu is not None:
            line["cpu_baseline"] = cpu
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
