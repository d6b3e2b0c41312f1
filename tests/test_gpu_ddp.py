"""GPU (-m gpu): the data-parallel TRAINING path (kubric_train_pose_3D.py:119-130): the model wrapped in torch
DistributedDataParallel, one scene per rank, gradients all-reduced in buckets. Two ranks share the single GPU of the test box, so
the process group is gloo (RCCL refuses two ranks on one device; the bucketing / hook logic of DDP is backend-independent); the
averaged gradients must equal those of ONE process that sees both scenes as a batch of 2."""
import os
import socket
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["encoder_3d.fusion_feature.cells.0.conv_gate.weight", "encoder_3d.conv1.0.weight", "encoder_3d.density_head.6.weight",
        "encoder_3d.features_head.0.weight", "encoder_3d.feature_extraction.0.weight", "render.conv_rgb.6.weight",
        "encoder_3d.fusion_feature.fusion_norm.bias"]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _build(dev, batch_stats=False):
    from forge_amd import synthetic as syn
    from forge_amd.model_single_pose_estimator import FORGE_poseEstimator3D
    cfg = syn.kubric_config()
    model = FORGE_poseEstimator3D(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    if not batch_stats:
        for m in model.modules():                   # running statistics: per-rank batch statistics would differ from the batch-of-2 run
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.eval()
    return cfg, model


def _loss(model, sample, dev):
    from forge_amd import synthetic as syn
    imgs, masks = model(sample, syn.SyntheticDataset(1.5), dev)
    b = sample["images"].shape[0]
    tgt_i = sample["images"].repeat(1, 2, 1, 1, 1).reshape(b * 10, 3, 256, 256)
    tgt_m = sample["fg_probabilities"].repeat(1, 2, 1, 1, 1).reshape(b * 10, 1, 256, 256)
    return 5.0 * torch.nn.functional.mse_loss(imgs, tgt_i) + torch.nn.functional.mse_loss(masks, tgt_m)


def _sample(seeds, dev):
    from forge_amd import synthetic as syn
    parts = [syn.make_sample(1, 5, 256, 1.5, seed=s) for s in seeds]
    return {k: torch.cat([p[k] for p in parts], dim=0).to(dev) for k in parts[0]}


def _worker(rank, world, port, q, sync_bn=False):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from forge_amd import dist as fd
    fd.init(allow_shared_gpus=True)                 # 2 ranks on 1 GPU -> gloo, both on cuda:0
    dev = torch.device("cuda", torch.cuda.current_device())
    _, model = _build(dev, batch_stats=sync_bn)
    calls = [0]
    if sync_bn:                                     # the reference's configuration (kubric_train_pose_3D.py:119-124): statistics over all ranks
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model)
        orig_fwd = torch.nn.SyncBatchNorm.forward

        def counted(self, inp):                     # torch's own SyncBatchNorm kernels must not run: the HIP path takes every layer
            calls[0] += 1
            return orig_fwd(self, inp)
        torch.nn.SyncBatchNorm.forward = counted
    ddp = torch.nn.parallel.DistributedDataParallel(model, device_ids=[dev.index], find_unused_parameters=True)
    loss = _loss(ddp, _sample([100 + rank], dev), dev)
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    out = {k: named[k].grad.detach().cpu().numpy() for k in KEYS}      # numpy: pickled by value (tensors travel as fds of a process that may be gone)
    q.put((rank, float(loss.detach()), out, calls[0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("sync_bn", [False, True])
def test_ddp_two_ranks_equal_one_process_batch_of_two(sync_bn):
    """sync_bn = False: BatchNorm on running statistics (eval) in every module; sync_bn = True: SyncBatchNorm.convert_sync_batchnorm + train
    mode, i.e. batch statistics over both ranks - which must equal ordinary train-mode BatchNorm over the batch of 2 in one process."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, sync_bn)) for r in range(2)]
    for p in procs:
        p.start()
    import queue
    import time
    res, deadline = [], time.time() + 420
    while len(res) < len(procs):                     # fail fast when a rank dies instead of waiting out the queue timeout
        try:
            res.append(q.get(timeout=2))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() > deadline:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail("a DDP rank exited with %s before reporting (or the run timed out)" % (dead or "timeout",))
    res.sort(key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert res[0][3] == 0 and res[1][3] == 0, "torch.nn.SyncBatchNorm.forward ran %s times: the HIP SyncBatchNorm path was bypassed" % (res[0][3],)
    # every rank holds the same (averaged) gradients
    for k in KEYS:
        assert (res[0][2][k] == res[1][2][k]).all(), k
    # one process, both scenes as a batch of 2: mean loss over 2 scenes -> the same averaged gradients
    dev = torch.device("cuda:0")
    _, model = _build(dev, batch_stats=sync_bn)
    loss = _loss(model, _sample([100, 101], dev), dev)
    loss.backward()
    assert abs(float(loss.detach()) - 0.5 * (res[0][1] + res[1][1])) < 1e-5 * max(1.0, abs(float(loss.detach())))
    named = dict(model.named_parameters())
    for k in KEYS:
        ref = named[k].grad.detach().cpu()
        err = (torch.from_numpy(res[0][2][k]) - ref).abs().max().item()
        gscale = max(named[kk].grad.abs().max().item() for kk in KEYS)
        assert err < (1e-2 if sync_bn else 2e-4) * max(ref.abs().max().item(), 1e-3 * gscale) + 1e-9, (k, err, ref.abs().max().item())


def _ray_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from forge_amd import dist as fd, ops, synthetic as syn
    fd.init(allow_shared_gpus=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    D, C, V, Hr, S = 64, 16, 3, 128, 64
    feat, dens = syn.blob_volumes(1, D, C, seed=5)
    feat, dens = feat.to(dev), dens.to(dev)
    _, extr, _ = syn.orbit_cameras(10, 1.5, 15.0)
    E = extr[:V]
    K = syn.intrinsics(256) / 2.0
    cam = torch.cat([E[:, :3, :3].reshape(V, 9), E[:, :3, 3], K[0, 0].expand(V, 1), K[1, 1].expand(V, 1), K[0, 2].expand(V, 1),
                     K[1, 2].expand(V, 1)], dim=1).contiguous().to(dev)
    v2v = torch.zeros(V, dtype=torch.int32, device=dev)
    h = [0.5 * (D - 1) / D] * 3
    with torch.no_grad():
        got = fd.render_rays_sharded(feat, dens, cam, v2v, Hr, Hr, S, 0.5, 2.0, h, True)       # each rank marches its row band, one all_gather
        ref = ops.render_rays(feat, dens, cam, v2v, Hr, Hr, S, 0.5, 2.0, h, True)
    torch.cuda.synchronize()
    q.put((rank, [bool(torch.equal(a, b)) for a, b in zip(got, ref)], [tuple(a.shape) for a in got]))
    dist.barrier()
    dist.destroy_process_group()


def test_ray_sharded_render_two_ranks_on_the_gpu():
    """BASELINE configs[4] "per-ray sharding": two ranks (sharing the test box's GPU, gloo) each ray-march a band of image rows of every
    view with the HIP kernel and all_gather the bands; the assembled images equal the single-launch render bit for bit."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ray_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    import queue
    import time
    res, deadline = [], time.time() + 240
    while len(res) < len(procs):
        try:
            res.append(q.get(timeout=2))
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() > deadline:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail("a rank exited with %s before reporting (or the run timed out)" % (dead or "timeout",))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, equal, shapes in res:
        assert all(equal), (rank, equal)
        assert shapes == [(3, 16, 128, 128), (3, 1, 128, 128), (3, 1, 128, 128)]


def _driver_line(stdout):
    """bench.py's stdout as the driver reads it: the last line, the only JSON line, under 4 KB, strict JSON."""
    import json
    lines = stdout.splitlines()
    assert [l for l in lines if l.startswith("{")] == [lines[-1]], stdout[-3000:]
    assert len(lines[-1]) < 4096

    def refuse(tok):
        raise AssertionError("non-strict JSON token %s" % tok)
    return json.loads(lines[-1], parse_constant=refuse)


def test_bench_entry_two_ranks_on_the_shared_gpu(tmp_path):
    """`python bench.py --gpus 2` (no torchrun environment) on the one-GPU test box: the entry starts its own two ranks, each captures its
    hipGraph BEFORE the process group exists, the ranks rendezvous (gloo here: two ranks on one device; RCCL on a real node), time the step
    between barriers, all-reduce time / SSE / view counts, and rank 0 prints one line with n_gpus = 2 and twice the per-rank views. Without
    FORGE_BENCH_ALLOW_SHARED_GPUS the same command must refuse (a scaling number from shared devices would be meaningless)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    full = str(tmp_path / "full.json")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full", "--no-microbench", "--full-record", full]
    bad = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert bad.returncode != 0 and "GPU(s) visible" in (bad.stderr + bad.stdout)
    ok = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=dict(env, FORGE_BENCH_ALLOW_SHARED_GPUS="1"), cwd=root)
    assert ok.returncode == 0, ok.stderr[-2000:]
    c = _driver_line(ok.stdout)                                              # what the driver parses: compact, strict, last
    assert c["n_gpus"] == 2 and c["value"] > 0 and c["ranks_ok"] == 2 and "cpu_baseline" not in c and c["roofline"]["bound"] == "mfma"
    assert c["multi_rank"]["ddp_train"][0] > 0 and c["multi_rank"]["ddp_train"][1] > 200 and c["multi_rank"]["ddp_train"][3] == 2
    assert c["strong_scaling"]["total_scenes"] == 8
    d = json.load(open(full))                                                # the full record
    assert d["value"] == pytest.approx(c["value"], rel=1e-3)
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["value"] > 0 and "cpu_baseline" not in d and d["ranks_ok"] == 2 and not d["errors"]
    assert d["strong_scaling"]["total_scenes"] == 8 and d["strong_scaling"]["scenes_per_gpu"] == 4 and d["strong_scaling"]["ranks_ok"] == 2
    assert abs(d["value"] - 2 * 5 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-6 * d["value"]          # whole-job views / max-over-ranks time
    # the SAME line carries the sub-records whose collectives matter on a real node - DDP + SyncBatchNorm training (configs[3]) with
    # and without the gradient all-reduce, and the ray-sharded joint step (configs[4]) at both grids with the sharded render op in both reduce modes
    m = d["multi_rank"]
    t = m["ddp_train"]
    assert t["ranks_ok"] == 2 and not t["errors"] and t["global_batch"] == 8 and t["ms_per_step"] > 0 and t["ms_per_step_no_sync"] > 0
    assert t["gradient_bytes_all_reduced_per_step"] > 200e6 and t["syncbn_layers"] > 50 and t["process_group"]["world_size"] == 2
    for name, vol in (("ray_sharded_joint", 17 * 64 ** 3 * 4), ("ray_sharded_joint_grid64", 17 * 128 ** 3 * 4)):
        j = m[name]
        assert j["ranks_ok"] == 2 and not j["errors"] and j["band_rows"] == 64 and j["ms_per_step"] > 0 and j["unsharded_ms_per_step"] > 0, (name, j)
        assert j["all_reduce_bytes_per_step"] >= vol and j["all_gather_bytes_per_step"] == 10 * 17 * 128 * 128 * 4
    op = m["ray_sharded_joint"]["sharded_render_op"]
    assert all(op["volume_%d_reduce_%s_fwd_bwd_ms" % (D, mode)] > 0 for D in (64, 128) for mode in ("all", "none"))


def test_plain_bench_run_is_the_headline_only(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W` without --full: the contract keys of the headline, the dump of the last timed step, and none of
    the measurements or checks that --full adds after the timed steps (roofline, per-kernel / per-stage splits, latency, oracle, CPU baseline,
    other configurations)."""
    import json
    import subprocess
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    full, dump = str(tmp_path / "full.json"), str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", dump,
                        "--full-record", full], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    c = _driver_line(r.stdout)
    assert c["n_gpus"] == 1 and c["steps"] == 3 and c["warmup"] == 1 and c["value"] > 0 and c["unit"] == "views/s" and c["dtype"] == "f32"
    assert c["higher_is_better"] is True and c["metric"] == "rendered views/sec (5 views, 128^2 px, 64^3 voxel)"
    assert abs(c["value"] - 5 / (c["ms_per_step"] / 1e3)) < 1e-3 * c["value"]
    d = json.load(open(full))
    for k in ("roofline", "conv_launches", "kernels", "stages_ms", "single_stream", "cpu_baseline", "psnr_vs_oracle_db", "extra_configs",
              "views_per_s_with_host_to_device_copy", "strong_scaling", "multi_rank"):
        assert k not in d and k not in c, k
    assert set(d["dump_outputs"]["arrays"]) == {"rgb", "masks"}
    rgb = np.load(os.path.join(dump, "rgb.npy"))
    assert rgb.shape == (5, 3, 256, 256) and np.isfinite(rgb).all()


def _spawn2(target, args=(), timeout=420):
    """Run `target(rank, 2, port, q, *args)` on two spawned ranks sharing the GPU; returns {rank: payload}; fails fast when a rank dies."""
    import queue
    import time
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, 2, port, q) + tuple(args)) for r in range(2)]
    for p in procs:
        p.start()
    res, deadline = {}, time.time() + timeout
    while len(res) < len(procs):
        try:
            r, payload = q.get(timeout=2)
            res[r] = payload
        except queue.Empty:
            dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
            if dead or time.time() > deadline:
                for p in procs:
                    if p.is_alive():
                        p.terminate()
                pytest.fail("a rank exited with %s before reporting (or the run timed out)" % (dead or "timeout",))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


RAY_KEYS = ["conv_rgb.0.weight", "conv_rgb.3.weight", "conv_rgb.6.weight", "conv_rgb.6.bias"]


def _ray_bwd_case(dev, ray_shard, D=64, reduce="all"):
    """VolRender (seeded conv_rgb, eval-mode BatchNorm, trainable weights) on a D^3 blob volume, 4 cameras: loss of the RGB / mask / depth
    maps against fixed random targets, gradients w.r.t. the feature volume, the density, R / T of the cameras and conv_rgb's weights."""
    from forge_amd import synthetic as syn
    from forge_amd.volume_render import VolRender
    torch.manual_seed(0)
    vr = VolRender(syn.kubric_config())
    pre = "render."
    vr.load_state_dict({k[len(pre):]: v for k, v in syn.seeded_state_dict({pre + k: v for k, v in vr.state_dict().items()}, 4).items()})
    vr = vr.to(dev).eval()
    vr.ray_shard, vr.ray_shard_reduce = ray_shard, reduce
    feat, dens = syn.blob_volumes(1, D, 16, seed=5)
    feat, dens = feat.to(dev).requires_grad_(True), dens.to(dev).requires_grad_(True)
    _, extr, _ = syn.orbit_cameras(10, 1.5, 15.0)
    E = extr[[0, 3, 5, 8]].to(dev)
    R, T = E[:, :3, :3].clone().requires_grad_(True), E[:, :3, 3].clone().requires_grad_(True)
    K = syn.intrinsics(256)[None].repeat(4, 1, 1).to(dev)
    g = torch.Generator().manual_seed(9)
    ti, tm, td = (torch.rand(4, c, 256, 256, generator=g).to(dev) for c in (3, 1, 1))
    rgb, mask, depth = vr({"R": R, "T": T, "K": K}, feat, dens, render_depth=True, view2vol=torch.zeros(4, dtype=torch.int32, device=dev))
    loss = 5.0 * torch.nn.functional.mse_loss(rgb, ti) + torch.nn.functional.mse_loss(mask, tm) + 0.3 * torch.nn.functional.mse_loss(depth, td)
    loss.backward()
    torch.cuda.synchronize()
    named = dict(vr.named_parameters())
    grads = {"feat": feat.grad, "dens": dens.grad, "R": R.grad, "T": T.grad}
    grads.update({k: named[k].grad for k in RAY_KEYS})
    return float(loss.detach()), {k: v.detach().float().cpu().numpy() for k, v in grads.items()}, rgb.detach().cpu().numpy()


def _ray_bwd_worker(rank, world, port, q, D=64, reduce="all"):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from forge_amd import dist as fd
    fd.init(allow_shared_gpus=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    loss, g, rgb = _ray_bwd_case(dev, True, D, reduce)
    if D > 64:                                      # 128^3: the volume gradients are 134 + 8 MB per rank - ship a strided sample and float64 checksums
        g = {k: ((v[:, :, ::3, ::3, ::3].copy(), float(v.astype("float64").sum()), float((v.astype("float64") ** 2).sum())) if v.ndim == 5 else v)
             for k, v in g.items()}
    q.put((rank, (loss, g, rgb)))
    dist.barrier()
    dist.destroy_process_group()




def test_ray_sharded_render_backward_two_ranks_on_the_gpu():
    """the ray-sharded render is differentiable. Two ranks sharing the GPU (gloo) each march and back-propagate
    their band of rows with the HIP kernels (forge_render_fwd / forge_render_bwd), all_gather the maps, all-reduce d(volume) / d(cameras):
    loss, the gradients of the volume, the density, the camera R / T and conv_rgb's weights equal the single-process values on BOTH
    ranks (1e-5 of each gradient's max: fp32 atomics sum in a different order), the images bit for bit."""
    res = _spawn2(_ray_bwd_worker)
    ref_loss, ref_g, ref_rgb = _ray_bwd_case(torch.device("cuda:0"), False)
    import numpy as np
    for r in (0, 1):
        loss, g, rgb = res[r]
        assert np.array_equal(rgb, ref_rgb), r
        assert abs(loss - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss))
        for k, ref in ref_g.items():
            err = float(np.abs(g[k] - ref).max())
            assert err <= 1e-5 * max(float(np.abs(ref).max()), 1e-12) + 1e-12, (r, k, err, float(np.abs(ref).max()))


@pytest.mark.parametrize("reduce", ["all", "none"])
def test_ray_sharded_render_backward_128cube_volume_two_ranks(reduce):
    """BASELINE configs[4]'s volume size: the ray-sharded backward on a 128^3 render volume (142.6 MB of d(volume) per
    rank: the all-reduce payload of reduce="all"), two ranks sharing the GPU over gloo, against the single-process backward - loss 1e-6, the
    camera / conv_rgb gradients and a strided sample + float64 checksums of the volume gradients at 1e-5 of each gradient's max.
    reduce="none" (the partials stay on the ranks for dist.broadcast_from_owner's reduce-to-owner): the two ranks' partials SUM to the
    single-process gradient."""
    import numpy as np
    res = _spawn2(_ray_bwd_worker, args=(128, reduce), timeout=600)
    ref_loss, ref_g, ref_rgb = _ray_bwd_case(torch.device("cuda:0"), False, 128)
    part = ("feat", "dens", "R", "T")                # what the band backward produces (partial under reduce="none")
    for r in (0, 1):
        loss, g, rgb = res[r]
        assert np.array_equal(rgb, ref_rgb), r
        assert abs(loss - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss))
    for k, ref in ref_g.items():
        scale = max(float(np.abs(ref).max()), 1e-12)
        vals = [res[r][1][k] for r in (0, 1)]
        if ref.ndim == 5:                            # volume gradients: (strided sample, sum, sum of squares)
            sub = ref[:, :, ::3, ::3, ::3]
            s1, s2 = float(ref.astype("float64").sum()), float((ref.astype("float64") ** 2).sum())
            if reduce == "none":
                got = vals[0][0] + vals[1][0]
                assert float(np.abs(got - sub).max()) <= 1e-5 * scale, (k, "sample of the summed partials")
                assert abs(vals[0][1] + vals[1][1] - s1) <= 1e-5 * scale * ref.size ** 0.5 + 1e-9, (k, "checksum")
                assert abs(vals[0][1]) > 0 and abs(vals[1][1]) > 0, (k, "both bands contribute")
            else:
                for r in (0, 1):
                    assert float(np.abs(vals[r][0] - sub).max()) <= 1e-5 * scale, (r, k)
                    assert abs(vals[r][1] - s1) <= 1e-5 * scale * ref.size ** 0.5 + 1e-9 and abs(vals[r][2] - s2) <= 1e-4 * s2 + 1e-12, (r, k, "checksums")
        elif k in part and reduce == "none":
            assert float(np.abs(vals[0] + vals[1] - ref).max()) <= 1e-5 * scale + 1e-12, (k, "summed camera partials")
        else:
            for r in (0, 1):
                assert float(np.abs(vals[r] - ref).max()) <= 1e-5 * scale + 1e-12, (r, k)


JOINT_KEYS = ["pose_head.4.weight", "encoder_traj.pose_head_1.3.weight", "encoder_3d.conv1.0.weight", "encoder_3d.fusion_feature.cells.0.out_gate.weight",
              "encoder_3d.features_head.0.weight", "encoder_3d.density_head.6.weight", "render.conv_rgb.6.weight",
              "encoder_3d.feature_extraction.4.0.conv1.weight"]


def _joint_step(dev, ray_shard):
    """One iteration of the joint 2D3D fine-tune (kubric_train_joint.py:136-141 -> compute_all_loss_nvs): FORGE with predicted poses,
    5 input + 5 novel views, loss, backward. BatchNorm on running statistics and Dropout off so that two processes are comparable."""
    from forge_amd import synthetic as syn, train
    from forge_amd.model import FORGE
    # The pose networks of the joint model run on stock PyTorch kernels whose default backward algorithms (MIOpen / rocBLAS) are not
    # reproducible run to run; their gradients flow back into the trunk / conv1 and made two SINGLE-process runs differ by 5e-3 relative L2
    # (tools/debug/joint_shard_noise.py). Pinned to their deterministic algorithms the same two runs agree to 2e-6 - what is left is the
    # distance the test is about: this repo's kernels, sharded vs not.
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    torch.use_deterministic_algorithms(True, warn_only=True)
    cfg = syn.kubric_config(use_gt_pose=False, parameter="joint")
    model = FORGE(cfg)
    model.load_state_dict(syn.seeded_state_dict(model.state_dict(), 0))
    model = model.to(dev).train()
    for m in model.modules():
        if isinstance(m, (torch.nn.modules.batchnorm._BatchNorm, torch.nn.Dropout)):
            m.eval()
    model.render.ray_shard = ray_shard
    sample = {k: v.to(dev) for k, v in syn.make_sample(1, 10, 256, 1.5, seed=12).items()}
    loss, losses, _, _ = train.compute_all_loss_nvs(cfg, 0, sample, syn.SyntheticDataset(1.5), model, {}, dev)
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    torch.use_deterministic_algorithms(False)
    torch.backends.cudnn.deterministic = False
    return float(loss.detach()), losses, {k: named[k].grad.detach().cpu().numpy() for k in JOINT_KEYS}


def _joint_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from forge_amd import dist as fd
    fd.init(allow_shared_gpus=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    q.put((rank, _joint_step(dev, True)))
    dist.barrier()
    dist.destroy_process_group()


def test_joint_finetune_step_ray_sharded_two_ranks_equal_one_process():
    """VERDICT r2 item 1(c) / BASELINE configs[4]: the joint fine-tune step with the ray-march of its 10 views split into row bands over
    two ranks (model.render.ray_shard): loss terms and parameter gradients from the pose head, the 3-D pose estimator, the trunk, conv1,
    the GRU, both heads and conv_rgb equal the single-process step on both ranks."""
    import numpy as np
    # the single-process step FIRST: on a fresh box the first processes to run the stock-torch pose networks find a cold MIOpen kernel cache
    # and (two ranks racing through it) end up on other solvers than any later process - their gradients then differ by 1e-2 from everybody
    # else's, and from each other (tools/debug/joint_shard_noise.py with JOINT_SPAWN_FIRST=1); with the cache warmed here all processes agree
    ref_loss, ref_terms, ref_g = _joint_step(torch.device("cuda:0"), False)
    res = _spawn2(_joint_worker, timeout=600)
    rel = lambda a, b: float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-20))
    for r in (0, 1):
        loss, terms, g = res[r]
        assert abs(loss - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss)), (r, loss, ref_loss)
        for k, v in ref_terms.items():
            assert abs(terms[k] - v) <= 1e-6 * max(1.0, abs(v)), (r, k)
        for k, ref in ref_g.items():
            # a FIXED bound (round 3 had to use the run-to-run noise of the step, up to 4e-3): the ray-march backward is deterministic now and the
            # stock-torch pose networks are pinned to their deterministic algorithms (_joint_step), so two single-process runs agree to <= 3e-6
            # relative L2 (the weight-gradient kernels' fp32 atomics) and so does the sharded step: measured <= 3.2e-6 on every key
            # (tools/debug/joint_shard_noise.py)
            assert rel(g[k], ref) <= 2e-5, (r, k, rel(g[k], ref))


def _syncbn_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from forge_amd import dist as fd
    from forge_amd.fusion import bn_act_rows
    fd.init(allow_shared_gpus=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x, dy, w, b = _syncbn_case()
    rows = slice(0, 5) if rank == 0 else slice(5, 8)                       # UNEQUAL shards: 5 and 3 of the 8 batch elements
    bn = torch.nn.SyncBatchNorm(48).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    xr = x[rows].to(dev).requires_grad_(True)
    y = bn_act_rows(bn, xr, 0.01)
    y.backward(dy[rows].to(dev))
    torch.cuda.synchronize()
    q.put((rank, {k: v.detach().cpu().numpy() for k, v in dict(y=y, dx=xr.grad, dw=bn.weight.grad, db=bn.bias.grad, rm=bn.running_mean,
                                                              rv=bn.running_var).items()}))
    dist.barrier()
    dist.destroy_process_group()


def _syncbn_case():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(8, 6, 6, 6, 48, generator=g) * 1.7 + 0.4
    return x, torch.randn(8, 6, 6, 6, 48, generator=g), torch.rand(48, generator=g) + 0.5, torch.randn(48, generator=g)


def test_hip_sync_batchnorm_two_ranks_equal_one_process_batch():
    """HIP SyncBatchNorm - bn_stats partials (float64) -> ONE all-reduce -> apply; backward likewise. Two ranks with UNEQUAL
    shards (5 + 3 batch elements) == one process running train-mode BatchNorm over all 8: outputs, input gradients and running statistics
    to 1e-6, per-rank weight / bias gradients summing to the single-process ones (DDP averages them afterwards, as with torch's module)."""
    import numpy as np
    from forge_amd.fusion import bn_act_rows
    res = _spawn2(_syncbn_worker, timeout=240)
    dev = torch.device("cuda:0")
    x, dy, w, b = _syncbn_case()
    bn = torch.nn.BatchNorm3d(48).to(dev).train()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    xr = x.to(dev).requires_grad_(True)
    y = bn_act_rows(bn, xr, 0.01)
    y.backward(dy.to(dev))
    cat = lambda k: np.concatenate([res[0][k], res[1][k]], axis=0)
    assert np.abs(cat("y") - y.detach().cpu().numpy()).max() < 1e-6 * max(1.0, float(y.detach().abs().max()))
    assert np.abs(cat("dx") - xr.grad.cpu().numpy()).max() < 1e-6 * max(1.0, float(xr.grad.abs().max()))
    for k, ref in (("dw", bn.weight.grad), ("db", bn.bias.grad)):
        assert np.abs(res[0][k] + res[1][k] - ref.cpu().numpy()).max() < 2e-6 * max(1.0, float(ref.abs().max())), k
    for r in (0, 1):
        assert np.abs(res[r]["rm"] - bn.running_mean.cpu().numpy()).max() < 1e-6
        assert np.abs(res[r]["rv"] - bn.running_var.cpu().numpy()).max() < 1e-6


def test_bench_train_mode_two_ranks_and_n1_paths_agree():
    """(i) `bench.py --train --gpus 2` - FORGE_poseEstimator3D under SyncBatchNorm (HIP kernels) + DDP on two ranks
    sharing the GPU - prints one line with n_gpus = 2, both ranks ok; (ii) the N = 1 line is the same measurement whether bench.py runs
    plainly or under torch.distributed.run with one rank (same views counted, values within the noise of a 3-step run)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    bench = os.path.join(ROOT, "bench.py")
    tr = subprocess.run([sys.executable, bench, "--gpus", "2", "--train", "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=1200,
                        env=dict(env, FORGE_BENCH_ALLOW_SHARED_GPUS="1"), cwd=ROOT)
    assert tr.returncode == 0, tr.stderr[-3000:]
    d = _driver_line(tr.stdout)
    assert d["n_gpus"] == 2 and d["ranks_ok"] == 2 and not d.get("errors") and d["value"] > 0 and d["config"]["global_batch"] == 2
    # configs[3]'s real per-GPU shape through the same entry: --grid 64 (128^3-voxel render grid from synthetic 64^3 feature volumes in the sample)
    t64 = subprocess.run([sys.executable, bench, "--gpus", "2", "--train", "--grid", "64", "--steps", "1", "--warmup", "1", "--repeats", "1"], capture_output=True,
                         text=True, timeout=1200, env=dict(env, FORGE_BENCH_ALLOW_SHARED_GPUS="1"), cwd=ROOT)
    assert t64.returncode == 0, t64.stderr[-3000:]
    d64 = _driver_line(t64.stdout)
    assert d64["n_gpus"] == 2 and d64["ranks_ok"] == 2 and not d64.get("errors") and d64["value"] > 0 and d64["config"]["feature_grid"] == 64 and "128^3" in d64["metric"]
    quick = ["--steps", "3", "--warmup", "1", "--no-microbench", "--no-cpu-baseline", "--no-extra"]
    plain = subprocess.run([sys.executable, bench, "--gpus", "1"] + quick, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert plain.returncode == 0, plain.stderr[-2000:]
    port = _free_port()
    launched = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                               "--master-port", str(port), bench, "--gpus", "1"] + quick, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert launched.returncode == 0, launched.stderr[-2000:]
    a, b = (_driver_line(r.stdout) for r in (plain, launched))
    assert a["n_gpus"] == b["n_gpus"] == 1 and a["metric"] == b["metric"] and a["config"]["workload"] == b["config"]["workload"]
    assert abs(a["value"] - b["value"]) < 0.15 * a["value"], (a["value"], b["value"])


def test_rccl_backend_single_rank_runs_the_collectives_this_package_issues():
    """The test box has one GPU, so every multi-rank test above runs over gloo. This one at least drives RCCL itself (backend "nccl", world
    size 1, in a subprocess): the collectives forge_amd issues - float64 all_reduce (SyncBatchNorm statistics, bench scalars), fp32 all_reduce /
    all_gather on volume-sized tensors (ray-sharded render), broadcast / reduce (owner mode), all_gather_object (per-rank error strings), the
    device-bound barrier - load the library, create a communicator and complete on the MI355X."""
    import subprocess
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=%r)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", init_method="env://", rank=0, world_size=1)
from forge_amd import dist as fd
dev = torch.device("cuda:0")
a = torch.arange(257, dtype=torch.float64, device=dev); dist.all_reduce(a); assert float(a.sum()) == 257 * 256 / 2
v = torch.randn(1, 16, 64, 64, 64, device=dev).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)      # channels-last volume, 16.8 MB
w = v.clone(); dist.all_reduce(fd._dense_view(w)); assert torch.equal(w, v)
parts = [torch.empty(3, 4, 64, 128, device=dev)]; dist.all_gather(parts, torch.ones(3, 4, 64, 128, device=dev)); assert float(parts[0].sum()) == 3 * 4 * 64 * 128
b = torch.full((5,), 2.0, device=dev); dist.broadcast(b, src=0); dist.reduce(b, dst=0); assert float(b.sum()) == 10.0
assert fd.gather_strings("rank0 ok") == ["rank0 ok"] or fd.gather_strings("x") == ["x"]
out = [None]; dist.all_gather_object(out, {"err": None}); assert out == [{"err": None}]
fd.barrier(); dist.barrier(device_ids=[0])
torch.cuda.synchronize()
print("RCCL_OK", dist.get_backend())
dist.destroy_process_group()
''' % (ROOT, str(_free_port()))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "RCCL_OK nccl" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


def test_multi_rank_bench_records_run_on_rccl_with_one_rank():
    """The sub-records of `bench.py --gpus N` (benchkit.multirank.ddp_train_record / ray_sharded_joint_record) on the REAL backend: the test box has one GPU, so the
    2-rank tests above run their collectives over gloo; here the same two functions run in a subprocess whose default process group is RCCL (backend "nccl",
    world size 1) - DistributedDataParallel's reducer (bucketed all-reduce of this package's gradients, find_unused_parameters, no_sync), SyncBatchNorm-converted
    modules, `train.train_step`'s sample broadcast and loss all-reduce, and `multi_rank_records`' own gathers all go through the RCCL communicator."""
    import json
    import subprocess
    code = r'''
import json, os, sys, types, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=%r)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", init_method="env://", rank=0, world_size=1)
from benchkit import multirank as bench
dev = torch.device("cuda", 0)
args = types.SimpleNamespace(steps=2)
rec = bench.multi_rank_records(args, 0, 1, dev, {"metric": "rehearsal"}, records=(
    ("ddp_train", lambda: bench.ddp_train_record(0, 1, dev, 2, scenes=1, grid=32)),
    ("ray_sharded_joint", lambda: bench.ray_sharded_joint_record(0, 1, dev, 2, grid=32))))
torch.cuda.synchronize()
print("RECORDS " + json.dumps(rec))
dist.destroy_process_group()
''' % (ROOT, str(_free_port()))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("RECORDS ")][0][len("RECORDS "):])
    for name in ("ddp_train", "ray_sharded_joint"):
        assert rec[name]["ranks_ok"] == 1 and not rec[name]["errors"] and rec[name]["process_group"]["backend"] == "nccl", rec[name]
    assert rec["ddp_train"]["ms_per_step"] > 0 and rec["ddp_train"]["ms_per_step_no_sync"] > 0 and rec["ddp_train"]["gradient_bytes_all_reduced_per_step"] > 200e6
    assert rec["ray_sharded_joint"]["unsharded_ms_per_step"] > 0 and rec["ray_sharded_joint"]["ms_per_step"] > 0
