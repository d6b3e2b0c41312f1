"""The headline measurement: rendered views/sec of the FORGE reconstruction hot path (models/model.py:42-148) on this rank's GPU; with
`--full` also its dominant-kernel roofline, per-kernel and per-stage splits, parity against the oracle and the CPU baseline beside it."""
import os
import sys
import time

import torch

from forge_amd import dist as fdist, synthetic as syn
from benchkit.common import (FP32_MFMA_PEAK_TF, GF_CONVRGB, GF_ENCODER, GF_FUSE, GF_HEADS, HBM_PEAK_GBS, KLOOP_CEILING_TF, ROOT, T_IN, V_OUT,
                             _timed, floor_of, region_sizes, region_stats, timed_region)
from benchkit.cpu import cpu_baseline
from benchkit.dump import dump_outputs, host_copy
from benchkit.emit import emit
from benchkit.extras import extra_configs
from benchkit.kernels import kernel_rooflines, pmc_traffic, rocprof_conv_time, stage_timers
from benchkit.multirank import multi_rank_records


def describe(grid, B):
    """(metric, workload, algorithmic GFLOP per step) of the headline configuration: feature grid `grid`, B scenes per GPU."""
    if grid == 32:
        metric = "rendered views/sec (5 views, 128^2 px, 64^3 voxel)"
        workload = ("BASELINE configs[%d]: FORGE hot path, %d scene(s)/GPU x 5 input views 256^2 -> 32^3x128 feature "
                    "grid -> 64^3 render grid -> 5 views x 128^2 rays x 64 samples -> 5 RGB 256^2; HIP rotate, "
                    "fp32-MFMA implicit-GEMM ResNet-50 trunk / conv1 / ConvGRU (Winograd F(2x2,3x3) x 3 depth taps) / heads / conv_rgb, HIP ray-march (no "
                            "MIOpen/rocBLAS kernel in the step); "
                    "eval BN, random-init seeded weights" % (1 if B == 1 else 2, B))
        gflop = B * (GF_ENCODER + GF_FUSE + GF_HEADS + GF_CONVRGB)
    else:
        metric = "rendered views/sec (5 views, 128^2 px, 128^3 voxel)"
        workload = ("BASELINE configs[3]/[4] grid (synthetic up-scale, SURVEY.md 8d): %d scene(s)/GPU x 5 synthetic feature volumes "
                    "[128,64^3] resident in HBM (the encoder cannot produce them from 256^2 images, models/encoder.py:49) -> HIP rotate at "
                    "D=64 (1.07 GB/scene) -> ConvGRU fusion at M=262144 -> heads -> 128^3 x 17 render volume (142.6 MB) -> 5 views x "
                    "128^2 rays x 64 samples -> conv_rgb -> 5 RGB 256^2; eval BN, random-init seeded weights" % B)
        gflop = B * (8 * (GF_FUSE + GF_HEADS) + GF_CONVRGB)
    return metric, workload, gflop


def run_headline(args, rank, world, dev, affinity):
    from forge_amd.model import FORGE
    cfg = syn.kubric_config()
    B = args.scenes
    ok, err = 1.0, None
    graphed = step = eager_step = strong = None
    B_strong = max(1, 8 // world) if (args.full and world > 1 and not args.no_extra and args.grid == 32 and not args.no_graph) else 0
    try:
        model = FORGE(cfg)
        weights = syn.seeded_state_dict(model.state_dict(), 0)
        model.load_state_dict(weights)
        model = model.to(dev).eval()
        sample_cpu = syn.make_sample(B, T_IN, 256, 1.5, seed=1000 + rank)
        sample = {k: v.to(dev) for k, v in sample_cpu.items()}      # inputs resident in HBM
        dataset = syn.SyntheticDataset(1.5)

        if args.grid == 32:
            def eager_step():
                with torch.no_grad():
                    return model(sample, dataset, dev)
        else:
            # 128^3-voxel scenes: per-view feature volumes [B,5,128,64^3] (671 MB per scene) resident in HBM, GT poses / cameras of the sample
            from forge_amd import geo_utils
            gen = torch.Generator(device=dev).manual_seed(77 + rank)
            feats64 = torch.randn(B, T_IN, 128, 64, 64, 64, device=dev, generator=gen).mul_(0.5).permute(0, 1, 3, 4, 5, 2).contiguous().permute(0, 1, 5, 2, 3,
                    4)
            poses64 = sample["cam_poses_cv2_canonicalized"][:, :T_IN].contiguous()
            cams64 = geo_utils.camera_dict(sample["cam_extrinsics_cv2_canonicalized"][:, :V_OUT], sample["K_cv2"][:, :V_OUT])

            def eager_step():
                with torch.no_grad():
                    return model.reconstruct(feats64, poses64, cams64)[:2]

        # hipGraph capture happens BEFORE the process group exists: no RCCL communicator / watchdog thread is alive while the stream is
        # capturing, so the capture cannot be invalidated by collective-library activity; the barrier / all-reduce below never run inside it.
        if args.no_graph:
            step = eager_step
        elif args.grid == 32:
            # hipGraph(s) of the whole step; replays do all the work. pipeline_depth steps are kept in flight on as many HIP streams: the
            # under-filled ResNet launches of one step share the chip with the MFMA-bound ConvGRU launches of its neighbours
            from forge_amd.graph import PipelinedForward
            graphed = PipelinedForward(model, sample, dataset, dev, depth=max(1, args.pipeline_depth))
            step = lambda: graphed(sample)                              # noqa: E731  (copies the resident inputs into the slot's static buffers)
        else:
            from forge_amd.graph import GraphedCall
            step = GraphedCall(eager_step, dev)
        if B_strong and B_strong != B:                                   # strong scaling: 8 scenes in total over the N ranks
            from forge_amd.graph import PipelinedForward
            s_strong = {k: v.to(dev) for k, v in syn.make_sample(B_strong, T_IN, 256, 1.5, seed=2000 + rank).items()}
            g_strong = PipelinedForward(model, s_strong, dataset, dev, depth=2)
            strong = lambda: g_strong(s_strong)                          # noqa: E731
        elif B_strong:
            strong = step
    except Exception as e:                                                # this rank still joins the rendezvous and the reductions: no hang
        ok, err = 0.0, repr(e)[:400]
        import traceback
        traceback.print_exc()

    fdist.init(allow_shared_gpus=os.environ.get("FORGE_BENCH_ALLOW_SHARED_GPUS") == "1")      # RCCL (backend "nccl") over xGMI when world > 1
    fdist.barrier()

    R = len(region_sizes(args.steps, args.repeats))
    dumped = None
    if ok:
        ok, err, out, dts = timed_region(step, args.steps, args.warmup, R)
        if ok and rank == 0 and args.dump_outputs:
            # now, before any other replay: the graphs' static outputs are overwritten by the next call of their slot
            dumped = host_copy(dict(zip(("rgb", "masks"), out)))
    else:
        for _ in range(2 * R):
            fdist.barrier()
        out, dts = None, [0.0] * R
    pg = fdist.group_info()                                          # which backend actually carried the collectives of this run
    dts = fdist.all_reduce_scalars(dts, dev, "max")                  # every region: the slowest rank's clock
    dt = region_stats(dts, args.steps, 1.0)[0]                      # median region
    # the one exchange of the inference path: (SSE to the target views, pixel count, views rendered) summed over ranks
    # (RCCL all-reduce of a few doubles) -> whole-job PSNR (--full) / view count; ranks_ok rides along
    if ok and args.full:
        tgt_dev = sample["images"][:, :V_OUT].reshape(B * V_OUT, 3, 256, 256)
        sse_local, npix_local = float(((out[0] - tgt_dev) ** 2).sum()), float(tgt_dev.numel())
    else:
        sse_local = npix_local = 0.0
    sse, npix, views_per_step, ranks_ok = fdist.all_reduce_scalars([sse_local, npix_local, float(B * V_OUT) * ok, ok], dev, "sum")
    errors = [e for e in fdist.gather_strings(err) if e]
    views = int(views_per_step) * args.steps

    strong_res = None
    if B_strong:                                                     # bounded: <= 5 steps
        n_s = min(5, args.steps)
        if strong is not None and ok:
            ok_s, err_s, _, dts_s = timed_region(strong, n_s, 1)
            dt_s = dts_s[0]
        else:
            fdist.barrier()
            fdist.barrier()
            ok_s, dt_s = 0.0, 0.0
        dt_s = fdist.all_reduce_scalars([dt_s], dev, "max")[0]
        v_s, r_s = fdist.all_reduce_scalars([float(B_strong * V_OUT) * ok_s, ok_s], dev, "sum")
        strong_res = {"scaling": "strong", "total_scenes": B_strong * world, "scenes_per_gpu": B_strong, "steps": n_s, "ms_per_step": dt_s / n_s * 1e3,
                      "views_per_s": v_s * n_s / dt_s if dt_s > 0 else None, "ranks_ok": int(r_s),
                      "note": "8 scenes in total split over the ranks; the N = 1 point of this curve is extra_configs['configs[2]'] of the --gpus 1 line"}

    # world > 1: the sub-records whose collectives matter (DDP + SyncBatchNorm training, ray-sharded joint step), bounded and under a watchdog that
    # prints the main line below if they do not come back
    multi = None
    if args.full and world > 1 and not args.no_extra and args.grid == 32:
        metric_main = "rendered views/sec (5 views, 128^2 px, 64^3 voxel)"
        minimal = {"metric": metric_main, "value": (int(views_per_step) * args.steps / dt) if (ok and dt > 0) else None, "unit": "views/s", "n_gpus": world,
                   "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
                   "vs_baseline": None, "dtype": "f32", "data": "synthetic", "ranks_ok": int(ranks_ok), "errors": errors, "process_group": pg,
                   "strong_scaling": strong_res, "config": {"workload": "BASELINE configs[1]: FORGE hot path, %d scene(s)/GPU x 5 views (see the full "
                           "line of a run "
                                                                        "whose sub-records finished)" % B, "scenes_per_gpu": B}}
        if graphed is not None:
            graphed.wait()
        multi = multi_rank_records(args, rank, world, dev, minimal)
    # every rank is done with collectives: tear the process group down NOW, so that rank 0's per-kernel measurements, the other
    # configurations and the CPU baseline below never keep the other ranks (or an RCCL watchdog) waiting
    fdist.barrier()
    fdist.shutdown()
    if rank != 0:
        return None
    if not ok:
        emit({"metric": "rendered views/sec (5 views, 128^2 px, 64^3 voxel)", "value": None, "unit": "views/s", "n_gpus": world, "steps": args.steps,
              "warmup": args.warmup, "ranks_ok": int(ranks_ok), "process_group": pg, "errors": errors, "error": err}, args.full_record)
        return None
    metric, workload, gflop = describe(args.grid, B)
    step_ms = dt / args.steps * 1e3
    result = {
        "metric": metric, "value": views / dt, "unit": "views/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": step_ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "ranks_ok": int(ranks_ok), "errors": errors, "process_group": pg,
        "repeats": region_stats(dts, args.steps, float(views_per_step))[1],
        "config": {"workload": workload, "scenes_per_gpu": B, "views_in": T_IN, "views_out": V_OUT, "feature_grid": args.grid,
                   "render_grid": 2 * args.grid, "rank0_affinity": affinity,
                   "steps_in_flight": graphed.depth if graphed is not None else 1,
                   "launch": "eager" if args.no_graph else ("hipGraph replay, %d steps in flight on %d HIP streams" % (graphed.depth, graphed.depth)
                                                            if (graphed is not None and graphed.depth > 1) else "hipGraph replay"),
                   "parallelism": "dp%d (scene-sharded, no data-path collective; 4-scalar RCCL all-reduce of SSE/pixels/views/ok for the PSNR report)" % world},
    }
    if dumped is not None:
        result["dump_outputs"] = dump_outputs(args.dump_outputs, dumped)
    if not args.full:                                                # a plain run: the headline figure and nothing else
        emit(result, args.full_record)
        return result

    # ---- the same steps with the sample handed over as (pinned) HOST buffers, as a DataLoader would: PCIe-inclusive rate (never `value`)
    pcie_views_per_s = None
    if world == 1 and graphed is not None:
        graphed.wait()
        host = {k: v.pin_memory() for k, v in sample_cpu.items()}
        graphed(host)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            graphed(host)
        torch.cuda.synchronize()
        pcie_views_per_s = B * V_OUT * args.steps / (time.perf_counter() - t1)

    # ---- the same replay on ONE stream, back to back (= the latency of a step), and the per-stage split of that replay
    single = stages_replay = None
    if graphed is not None:
        one = graphed.slots[0]
        ms1 = _timed(lambda: one(sample), max(5, min(20, args.steps)))
        single = {"ms_per_step": ms1, "views_per_s": B * V_OUT / ms1 * 1e3, "note": "one hipGraph replay at a time on one stream: step latency"}
        if args.grid == 32 and not args.no_microbench:
            from forge_amd.flopmeter import stage_replay_ms
            stages_replay = {k: round(v, 4) for k, v in stage_replay_ms(model, sample, dev).items()}
    # ---- per-stage HIP-event split of one more step (outside the timed region)
    rec, undo = stage_timers(model)
    for _ in range(3):
        rec.clear()
        eager_step()
    torch.cuda.synchronize()
    conv_rec = {k: rec.pop(k) for k in list(rec) if k.startswith("conv_igemm")}
    wino_rec = {k: rec.pop(k) for k in list(rec) if k.startswith("wino_")}
    stages = {k: sum(a.elapsed_time(b) for a, b in v) for k, v in rec.items()}
    # x[4] (Winograd point-GEMM launches only): direct-convolution FLOPs of the convolution / FLOPs the launch executes
    conv_launch = {k: {"launches_per_step": len(v), "total_ms": sum(x[0].elapsed_time(x[1]) for x in v),
                       "gflop": sum(x[2] for x in v) / 1e9, "gflop_direct_equivalent": sum(x[2] * (x[4] if len(x) > 4 else 1.0) for x in v) / 1e9}
                   for k, v in conv_rec.items()}
    for u in undo:
        u()
    if args.dump_conv:
        for k, v in conv_rec.items():
            for x in v:
                ms = x[0].elapsed_time(x[1])
                print("%-34s M=%-7d N=%-5d taps=%-3d Cin=%-5d %.4f ms  %.1f TF" % ((k,) + x[3] + (ms, x[2] / ms / 1e9)), file=sys.stderr)
    if "encoder_total" in stages:
        stages["encoder_conv1(+layout)"] = stages.pop("encoder_total") - stages.get("encoder_resnet", 0.0)
    stages["render_march(+cam pack)"] = stages.pop("render_total") - stages.get("conv_rgb", 0.0)

    kern = {} if args.no_microbench else kernel_rooflines(dev, B, args.grid)
    for k, v in wino_rec.items():          # Winograd transform kernels of the fusion, as launched inside the step
        ms, by = sum(x[0].elapsed_time(x[1]) for x in v), sum(x[2] for x in v)
        kern[k] = {"bound": "hbm", "launches_per_step": len(v), "ms_total": ms, "bytes": by, "achieved": by / ms / 1e6, "peak": HBM_PEAK_GBS,
                   "unit": "GB/s", "frac": by / ms / 1e6 / HBM_PEAK_GBS, "traffic": pmc_traffic(k),
                   "note": "HIP events around the eager launches of one step (each includes the host launch gap); the transformed operands "
                           "(67-134 MB per launch at one scene) are partly served by the 256 MB Infinity Cache"}
    # dominant kernel of the step: conv_igemm_kernel<BM, BN, waves> - ONE kernel (csrc/conv_igemm.hip) whose tile shape is picked per
    # launch by the plan model, so rocprofv3 lists it under several instantiation names; together they are ~85 % of the step.
    # achieved = sum of the FLOPs its launches EXECUTE in one step (direct convolutions 2 M N taps Cin, Winograd point-GEMM launches
    # 2 x 16 R N kd Cin) / sum of their HIP-event durations. The per-instantiation avg_launch_ms are directly comparable with
    # rocprofv3's per-name AverageNs in profiles/. floor_ms = the same executed FLOPs at the 157.3 TF pipe peak: the step's own time floor.
    convs = {k: v for k, v in conv_launch.items() if k.startswith("conv_igemm_kernel<")}
    tot_ms = sum(v["total_ms"] for v in convs.values())
    tot_gf = sum(v["gflop"] for v in convs.values())
    n_launch = sum(v["launches_per_step"] for v in convs.values())
    alg_gf = sum(v["gflop_direct_equivalent"] for v in convs.values())
    n16_gf = sum(v["gflop"] for k, v in conv_launch.items() if not k.startswith("conv_igemm_kernel<"))
    inst = {k: {"launches_per_step": v["launches_per_step"], "avg_launch_ms": v["total_ms"] / v["launches_per_step"],
                "achieved": v["gflop"] / v["total_ms"], "frac": v["gflop"] / v["total_ms"] / FP32_MFMA_PEAK_TF,
                "gflop_per_step": v["gflop"], "share_of_step": v["total_ms"] / step_ms}
            for k, v in sorted(convs.items(), key=lambda kv: -kv[1]["total_ms"])}
    fl = floor_of(tot_gf + n16_gf, step_ms)
    tr = pmc_traffic("winograd gates" if wino_rec else "conv_igemm_kernel<128")
    rp = rocprof_conv_time() if (args.grid == 32 and B == 1) else None
    ceil_tf = KLOOP_CEILING_TF["64x128"]                              # the tile that carries ~80 % of the step's FLOPs
    roofline = {"kernel": "conv_igemm_kernel<BM, BN, waves> (fp32 MFMA implicit-GEMM conv; all %d launches of one step, %d tile instantiations)"
                          % (n_launch, len(convs)),
                "bound": "mfma", "achieved": tot_gf / tot_ms, "peak": FP32_MFMA_PEAK_TF, "unit": "TFLOP/s", "frac": tot_gf / tot_ms / FP32_MFMA_PEAK_TF,
                # flat keys: HBM-side bytes of the dominant launch from the PMC counters, per launch, next to its algorithmic bytes
                "traffic": tr["hbm_bytes_per_launch"] if tr else None, "traffic_algorithmic_bytes": tr["algorithmic_bytes"] if tr else None,
                "traffic_launch": tr["launch"] if tr else None, "traffic_source": ("profiles/" + tr["source"]) if tr else None,
                # (5b) the same fraction from pure kernel durations: rocprofv3 --kernel-trace --stats of this command, one step in flight
                "frac_rocprof": (tot_gf / rp["ms_per_step"] / FP32_MFMA_PEAK_TF) if rp else None,
                        "rocprof_kernel_ms_per_step": rp["ms_per_step"] if rp else None,
                "rocprof_source": ("profiles/" + rp["source"]) if rp else None,
                # (5c) what the kernel's own LDS -> MFMA loop can do with staging removed (measured on debug builds): the exact-fp32 ceiling of this design
                "ceiling": {"kloop_without_staging_tflops": KLOOP_CEILING_TF, "frac_of_peak": ceil_tf / FP32_MFMA_PEAK_TF,
                            "source": "profiles/TUNING_LOG.md 'K-loop ceiling' (tools/debug/gemm_ceiling.py on FORGE_EXP_* debug builds, direct gates "
                                    "launch K = 6912)"},
                "frac_of_ceiling": (tot_gf / (rp["ms_per_step"] if rp else tot_ms)) / ceil_tf,
                "avg_launch_ms": tot_ms / n_launch,
                "executed_gflop": fl["executed_gflop"], "executed_frac": fl["executed_frac"], "floor_ms": fl["floor_ms"],
                        "step_over_floor": fl["step_over_floor"],
                "kernel_ms_per_step": tot_ms, "share_of_step": tot_ms / step_ms, "instantiations": inst,
                "note": "frac = FLOPs the dominant kernel's launches EXECUTE / their HIP-event time / peak (a statement about the kernel; eager pass, each "
                        "event pair includes the host launch gap and, for split-K launches, the reduction); frac_rocprof = the same FLOPs / the kernels' own "
                        "durations in the committed rocprofv3 trace of this command. executed_frac = floor_ms / ms_per_step = the "
                        "WHOLE step (all kernels, hipGraph replay) against the time its executed matrix-core FLOPs need at peak (a statement about the "
                        "step). In SURVEY.md 8(d)'s direct-convolution FLOPs the same launches are %.0f GF (the Winograd launches execute 2.25x fewer "
                        "multiplies than the convolutions they replace), so a fraction in those units can exceed 1 and is not reported as one; "
                        "traffic = PMC pass of the fusion's point-GEMM launch (L2 -> fabric bytes, Infinity-Cache hits included)" % alg_gf}
    result.update({
        "single_stream": single,
        "roofline": roofline, "conv_launches": conv_launch, "kernels": kern, "stages_ms": {k: round(v, 4) for k, v in stages.items()},
        "stages_ms_replay": stages_replay,
        "gflop_per_step_algorithmic": gflop,
        "views_per_s_with_host_to_device_copy": pcie_views_per_s,
        "psnr_to_target_db_all_ranks": fdist.psnr_from_sse(sse, npix),
    })
    if strong_res is not None:
        result["strong_scaling"] = strong_res
    if multi is not None:
        result["multi_rank"] = multi
    ref = None
    if world == 1 and args.grid == 32 and not (args.no_cpu_baseline and args.no_oracle_check):
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import forge_oracle as fo
        if not args.no_cpu_baseline:
            cb, ref = cpu_baseline(sample_cpu, weights, cfg)
            result["cpu_baseline"] = cb
        else:
            # no timing of the CPU path, but the LAST output of the timed region is still checked against the oracle (one CPU forward of scene 0):
            # a soak run must look at what it produced ("a soak that never looks at its output proves only that nothing crashed")
            one = {k: v[:1] for k, v in sample_cpu.items()}
            with torch.no_grad():
                ref = fo.forward_hot_path(one["images"][:, :T_IN], one["cam_poses_cv2_canonicalized"][:, :T_IN], one["cam_extrinsics_cv2_canonicalized"][:,
                        :T_IN],
                                          one["K_cv2"][:, :T_IN], weights, cfg, order_by_distance=True)
        img0 = out[0][:V_OUT].cpu()
        result["psnr_vs_oracle_db"] = fo.psnr(img0, ref[0])
        result["oracle_note"] = ("oracle = oracle/forge_oracle.py, pinned by golden vectors from the reference's own module code; its ray-marcher restates "
                                 "PyTorch3D 0.7.0 (not installable offline): parity with the PyTorch3D BINARY is unpinned (DESIGN.md section 4)")
        result["max_abs_err_vs_oracle"] = (img0 - ref[0]).abs().max().item()
        # north_star: "PSNR within 0.1 dB of reference" - PSNR of both against the same target images (the scene's input views; with
        # random-init weights the absolute value is meaningless, the DIFFERENCE is the criterion)
        tgt = sample_cpu["images"][0, :V_OUT]
        p_build, p_oracle = fo.psnr(img0, tgt), fo.psnr(ref[0], tgt)
        result["psnr_to_target_db"] = {"build": p_build, "oracle": p_oracle, "abs_diff": abs(p_build - p_oracle)}
        if "cpu_baseline" in result:
            result["speedup_vs_cpu_baseline"] = result["value"] / result["cpu_baseline"]["value"]
    if world == 1 and not args.no_extra and args.grid == 32:
        del graphed, step
        torch.cuda.empty_cache()
        result["extra_configs"] = extra_configs(dev, steps=10)
    emit(result, args.full_record)
    if args.min_psnr_db is not None:
        got = result.get("psnr_vs_oracle_db")
        if got is None or not got >= args.min_psnr_db:
            raise SystemExit("bench.py: the last output of the timed region is %s dB from the oracle, below --min-psnr-db %.1f" % (got, args.min_psnr_db))
    return result
